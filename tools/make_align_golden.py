#!/usr/bin/env python
"""Word-timestamp goldens: tests/golden/align_tiny.npz and align_turbo.npz.

CPU, transformers fp32 with eager attention, the hash-initialised weights the GPU
regenerates (as tools/make_golden.py): one teacher-forced forward per window over
[sot, language, transcribe, no_timestamps, t_0 .. t_{n-1}, eot] with
``output_attentions=True``, then openai-whisper ``find_alignment`` restated with
transformers' own ``_median_filter`` and ``_dynamic_time_warping``:

    softmax over the 1500 keys (the model's own) -> crop to F = num_frames // 2 frames ->
    (w - mean) / std over all n + 5 positions, per (head, frame), population std ->
    median of 7 along the frames -> mean over the alignment heads ->
    rows 3 .. n + 3 = M [n + 1][F] -> DTW over -M in fp32 -> token_frame = time[jumps]

and token_prob[k] = softmax(logits[3 + k][:eot])[t_k].

matrix_tol is measured on this reference alone: the fp32 encoder output is perturbed by
uniform noise of the amplitude the encoder parity tests already accept (2e-2 at tiny dims,
1e-2 at turbo dims), M recomputed, max |dM| over 8 noise seeds taken and doubled for the
fp16 storage of the K projection.  Only M (and the single-head M of head (L-1, 0)) is
stored, not the per-head tensor, so each file stays well under 1 MiB.

    python tools/make_align_golden.py [--only tiny|turbo] [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import osw_path  # noqa: E402

osw_path.load()
from open_speech_amd import dims as D  # noqa: E402
from open_speech_amd import synth, weights  # noqa: E402

from make_golden import TINY_EMB_STD, TINY_SEED, TURBO_SEED, build_model, fe_mel  # noqa: E402
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter  # noqa: E402

WIDTH = 7
NOISE_SEEDS = 8
TINY_NOISE = 2e-2    # tests/test_gpu_parity.py: encoder output vs the fp16 oracle, atol
TURBO_NOISE = 1e-2   # tests/test_gpu_turbo.py: encoder rows vs the fp32 golden


def default_heads(d):
    L, H = d.n_text_layer, d.n_text_head
    return [(l, h) for l in range(L - L // 2, L) for h in range(H)]


def window_mel(mel: np.ndarray, seek: int, size: int) -> np.ndarray:
    """frames [seek, seek + size) zero padded to 3000 (faster-whisper pad_or_trim)."""
    out = np.zeros((mel.shape[0], 3000), np.float32)
    out[:, :size] = mel[:, seek:seek + size]
    return out


def forward(model, enc: torch.Tensor, forced: list):
    with torch.no_grad():
        o = model(encoder_outputs=(enc,), decoder_input_ids=torch.tensor([forced]), output_attentions=True,
                  use_cache=False)
    return o.logits[0].double(), o.cross_attentions


def matrix(cross, heads, n: int, num_frames: int) -> np.ndarray:
    w = torch.stack([cross[l][0, h] for l, h in heads])[None]     # [1][heads][P][1500] probabilities
    w = w[..., : num_frames // 2]
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    w = (w - mean) / std
    w = _median_filter(w, WIDTH)
    return w.mean(dim=1)[0, 3:n + 4].float().numpy()              # rows no_timestamps, t_0 .. t_{n-1}


def token_frames(ti, fi):
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    return fi[jumps]


def one_window(model, d, st, enc, tokens, lang, num_frames, noise):
    n = len(tokens)
    forced = [st.sot, lang, st.transcribe, st.no_timestamps] + list(tokens) + [st.eot]
    logits, cross = forward(model, enc, forced)
    heads = default_heads(d)
    M = matrix(cross, heads, n, num_frames)
    M1 = matrix(cross, [(d.n_text_layer - 1, 0)], n, num_frames)
    ti, fi = _dynamic_time_warping(-M.astype(np.float32))
    tp = np.array([float(torch.softmax(logits[3 + k, :st.eot], -1)[tokens[k]]) for k in range(n)])
    dm, dm1 = 0.0, 0.0
    for s in range(NOISE_SEEDS):
        rng = np.random.default_rng(1000 + s)
        e2 = enc + torch.from_numpy(rng.uniform(-noise, noise, size=tuple(enc.shape)).astype(np.float32))
        _, c2 = forward(model, e2, forced)
        dm = max(dm, float(np.abs(matrix(c2, heads, n, num_frames) - M).max()))
        dm1 = max(dm1, float(np.abs(matrix(c2, [(d.n_text_layer - 1, 0)], n, num_frames) - M1).max()))
    print(f"  n {n} frames {num_frames}: M {M.shape} |M| max {np.abs(M).max():.3f}, path {len(ti)}, "
          f"noise {noise:g} -> max |dM| {dm:.4g} (single head {dm1:.4g}), sensitivity {dm / noise:.3g}")
    return dict(forced=np.array(forced, np.int32), num_frames=np.int32(num_frames), M=M, M_head=M1,
                text_indices=ti.astype(np.int32), time_indices=fi.astype(np.int32),
                token_frame=token_frames(ti, fi).astype(np.int32), token_prob=tp,
                matrix_tol=np.float64(2 * dm), noise_dm=np.float64(dm), noise_dm_head=np.float64(dm1))


def save(path, wins, extra):
    flat = dict(extra)
    for i, w in enumerate(wins):
        for k, v in w.items():
            flat[f"w{i}/{k}"] = v
    flat["n_windows"] = np.int32(len(wins))
    flat["matrix_tol"] = np.float64(max(float(w["matrix_tol"]) for w in wins))
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes; matrix_tol", float(flat["matrix_tol"]))


TINY_WINDOWS = [(0, 3000, 37), (500, 1234, 9), (2000, 5, 1)]   # (seek, num_frames, n text tokens)


def gen_tiny(out):
    d = D.TINY_TEST
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    model = build_model(d, weights.random_weights(d, seed=TINY_SEED, emb_std=TINY_EMB_STD))
    mel = fe_mel(synth.chirp_clip(3, 30.0), d.n_mels)
    z = np.load(os.path.join(out, "tiny_model.npz"))
    lang = int(z["language"])
    ids = np.load(os.path.join(out, "tiny_text.npz"))["ids"]
    text = [int(t) for t in ids if t < st.eot]           # distinct text ids of the varied-text golden
    wins, used = [], 0
    for seek, nf, n in TINY_WINDOWS:
        with torch.no_grad():
            enc = model.model.encoder(input_features=torch.from_numpy(window_mel(mel, seek, nf))[None]).last_hidden_state
        w = one_window(model, d, st, enc, text[used:used + n], lang, nf, TINY_NOISE)
        w["seek"] = np.int32(seek)
        used += n
        wins.append(w)
    save(os.path.join(out, "align_tiny.npz"), wins, dict(language=np.int32(lang), noise=np.float64(TINY_NOISE)))


def gen_turbo(out):
    d = D.LARGE_V3_TURBO
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    model = build_model(d, weights.random_weights(d, seed=TURBO_SEED))
    mel = fe_mel(synth.chirp_clip(0, 30.0), d.n_mels)[:, :3000]
    z = np.load(os.path.join(out, "turbo_model.npz"))
    lang = int(z["language"])
    text = [int(t) for t in z["ids"] if t < st.eot][:60]
    assert len(text) == 60
    with torch.no_grad():
        enc = model.model.encoder(input_features=torch.from_numpy(mel)[None]).last_hidden_state
    w = one_window(model, d, st, enc, text, lang, 3000, TURBO_NOISE)
    w["seek"] = np.int32(0)
    save(os.path.join(out, "align_turbo.npz"), [w], dict(language=np.int32(lang), noise=np.float64(TURBO_NOISE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", choices=["tiny", "turbo"])
    a = ap.parse_args()
    torch.manual_seed(0)
    if a.only in (None, "tiny"):
        gen_tiny(a.out)
    if a.only in (None, "turbo"):
        gen_turbo(a.out)


if __name__ == "__main__":
    main()
