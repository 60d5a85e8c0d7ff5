"""numpy float32 restatement of the two history rules (CTranslate2's RepetitionPenalty and
NoRepeatNgram as faster-whisper passes them; arithmetic pinned to transformers' processors in
tests/test_history_rules_cpu.py).  Shared by the CPU and the GPU tests; not product code."""
from __future__ import annotations

import numpy as np


def history_rules(logits, history, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0) -> np.ndarray:
    """One row: ``logits`` [V] float32, ``history`` the ids sampled so far.  Returns a copy
    with the penalty applied (once per distinct id), then the n-gram bans."""
    x = np.array(logits, dtype=np.float32, copy=True)
    h = [int(t) for t in history]
    n = len(h)
    p = np.float32(repetition_penalty)
    if n and p > 0 and p != 1:
        ids = np.unique(np.asarray(h, dtype=np.int64))
        g = x[ids]
        with np.errstate(all="ignore"):
            x[ids] = np.where(g < 0, g * p, g / p).astype(np.float32)
    m = int(no_repeat_ngram_size)
    if m > 0 and n >= m:
        tail = h[n - m + 1:]
        for i in range(n - m + 1):
            if h[i:i + m - 1] == tail:
                x[h[i + m - 1]] = -np.inf
    return x


def has_repeated_ngram(tokens, m: int) -> bool:
    """Whether any m-gram occurs twice in ``tokens``."""
    seen = set()
    for i in range(len(tokens) - m + 1):
        g = tuple(tokens[i:i + m])
        if g in seen:
            return True
        seen.add(g)
    return False
