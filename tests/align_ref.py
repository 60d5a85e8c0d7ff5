"""numpy restatements the word-timestamp tests compare against (no GPU, no torch).

``dtw`` is transformers' ``_dynamic_time_warping`` (fp32 cost, the same tie rule and
backtrace) evaluated over anti-diagonals so that 445 x 1500 cells take milliseconds;
``median_filter`` is its ``_median_filter`` along the last axis; ``token_frames`` is the
``jumps`` rule of openai-whisper's ``find_alignment``.
"""
from __future__ import annotations

import numpy as np


def dtw(x: np.ndarray):
    """(text_indices, time_indices) of the fp32 DTW over cost matrix ``x`` [T][F]."""
    x = np.asarray(x, dtype=np.float32)
    T, F = x.shape
    cost = np.full((T + 1, F + 1), np.inf, np.float32)
    trace = np.full((T + 1, F + 1), -1, np.int8)
    cost[0, 0] = 0
    for d in range(2, T + F + 1):          # cells (i, j = d - i), all independent
        i = np.arange(max(1, d - F), min(T, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        t = np.where(diag, 0, np.where(up, 1, 2)).astype(np.int8)
        c = np.where(diag, c0, np.where(up, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c    # fp32 + fp32
        trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = T, F
    ti, fi = [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        fi.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti[::-1], np.int64), np.array(fi[::-1], np.int64)


def token_frames(text_indices: np.ndarray, time_indices: np.ndarray) -> np.ndarray:
    """time_indices[jumps], jumps = pad(diff(text_indices), (1, 0), 1) != 0."""
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    return np.asarray(time_indices)[jumps]


def path_cost(x: np.ndarray, text_indices, time_indices) -> float:
    return float(np.asarray(x, np.float64)[np.asarray(text_indices), np.asarray(time_indices)].sum())


def median_filter(a: np.ndarray, width: int) -> np.ndarray:
    """Median of ``width`` along the last axis with reflect padding; inputs no longer than
    ``width // 2`` are returned unchanged."""
    if width <= 0 or width % 2 != 1:
        raise ValueError("width should be an odd number")
    pad = width // 2
    a = np.asarray(a)
    if a.shape[-1] <= pad:
        return a
    p = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(p, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def tie_matrix(rng: np.random.Generator, T: int, F: int) -> np.ndarray:
    """Integer entries in -8..8 (most of them from {-1, 0, 1}, so ties abound); every partial
    sum stays an exact fp32 integer."""
    small = rng.integers(-1, 2, size=(T, F))
    wide = rng.integers(-8, 9, size=(T, F))
    return np.where(rng.random((T, F)) < 0.8, small, wide).astype(np.float32)
