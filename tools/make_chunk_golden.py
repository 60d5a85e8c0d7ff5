#!/usr/bin/env python
"""Goldens for a shorter encoder window (chunk_length 5: 500 mel frames, T = 250 encoder
positions): tests/golden/chunk_tiny.npz and align_chunk_tiny.npz.

CPU, transformers fp32 with eager attention, tiny dims with ``max_source_positions = 250``, the
encoder positional table cropped to its first 250 rows and the hash-initialised weights the GPU
regenerates (as tools/make_golden.py and tools/make_align_golden.py, whose methods these are):

* chunk_tiny.npz: the varied-text weights (tools/make_golden.py TEXT_SEED, TINY_TEXT_AMP), the
  first 5 s of chirp_clip(3, 30 s): greedy ids to 448 positions with the faster-whisper logits
  rules, the raw logits of the first 3 steps, the language and the no-speech probability.  The
  smallest top-2 margin must be >= 0.5 (asserted) and goes to tests/golden/chunk_tiny.json (this
  golden's own metadata file, beside tests/golden/meta.json, which the other tools write);
* align_chunk_tiny.npz: the weights of align_tiny.npz, three windows of at most 500 frames:
  M, the DTW path, token_frame, token probabilities, and matrix_tol measured on the reference
  alone (make_align_golden.one_window: softmax over the model's own 250 keys, then the crop).

    python tools/make_chunk_golden.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import json
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

from make_align_golden import TINY_NOISE, one_window, save  # noqa: E402
from make_golden import (TEXT_SEED, TINY_EMB_STD, TINY_SEED, TINY_TEXT_AMP, build_model, fe_mel,  # noqa: E402
                         greedy_golden)

CHUNK_LENGTH = 5
MIN_MARGIN = 0.5
ALIGN_WINDOWS = [(0, 500, 37), (1700, 333, 9), (2900, 5, 1)]   # (seek, num_frames, n text tokens)


def window_mel(mel: np.ndarray, seek: int, size: int, n_frames: int) -> np.ndarray:
    """frames [seek, seek + size) zero padded to n_frames (faster-whisper pad_or_trim)."""
    out = np.zeros((mel.shape[0], n_frames), np.float32)
    out[:, :size] = mel[:, seek:seek + size]
    return out


def encode(model, mel_window):
    with torch.no_grad():
        return model.model.encoder(input_features=torch.from_numpy(mel_window)[None]).last_hidden_state


def gen_greedy(out, d):
    w = weights.random_weights(d, seed=TEXT_SEED, text_pos=TINY_TEXT_AMP)
    assert w["enc.pos"].shape[0] == d.n_audio_ctx
    model = build_model(d, w)
    mel = fe_mel(synth.chirp_clip(3, 30.0), d.n_mels)
    enc = encode(model, window_mel(mel, 0, d.n_frames, d.n_frames))
    assert tuple(enc.shape) == (1, d.n_audio_ctx, d.n_audio_state)
    g = greedy_golden(model, d, enc, None, n_full_first=3)
    margin = float(g["margins"].min())
    assert margin >= MIN_MARGIN, f"smallest top-2 margin {margin} < {MIN_MARGIN}"
    keep = {k: g[k] for k in ("ids", "full_logits", "full_steps", "margins", "logprobs", "language", "no_speech_prob",
                              "sum_logprob")}
    keep["enc_rownorm"] = np.linalg.norm(enc[0].numpy().astype(np.float64), axis=1)
    path = os.path.join(out, "chunk_tiny.npz")
    np.savez_compressed(path, **keep)
    ids = g["ids"]
    meta = {"seed": TEXT_SEED, "text_pos": TINY_TEXT_AMP, "chunk_length": CHUNK_LENGTH, "n_audio_ctx": d.n_audio_ctx,
            "clip": "chirp_clip(3, 30 s), first 5 s", "n_ids": int(len(ids)),
            "distinct_ids": int(len(set(ids.tolist()))), "min_top2_margin": margin}
    print("chunk tiny", meta, os.path.getsize(path), "bytes")
    return meta


def gen_align(out, d):
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    model = build_model(d, weights.random_weights(d, seed=TINY_SEED, emb_std=TINY_EMB_STD))
    mel = fe_mel(synth.chirp_clip(3, 30.0), d.n_mels)
    lang = st.first_lang
    ids = np.load(os.path.join(out, "tiny_text.npz"))["ids"]
    text = [int(t) for t in ids if t < st.eot]
    wins, used = [], 0
    for seek, nf, n in ALIGN_WINDOWS:
        enc = encode(model, window_mel(mel, seek, nf, d.n_frames))
        w = one_window(model, d, st, enc, text[used:used + n], lang, nf, TINY_NOISE)
        w["seek"] = np.int32(seek)
        used += n
        wins.append(w)
    save(os.path.join(out, "align_chunk_tiny.npz"), wins, dict(language=np.int32(lang), noise=np.float64(TINY_NOISE),
                                                                chunk_length=np.int32(CHUNK_LENGTH)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    d = D.TINY_TEST.with_chunk_length(CHUNK_LENGTH)
    meta = {"generator": "tools/make_chunk_golden.py", "chunk_tiny": gen_greedy(a.out, d)}
    gen_align(a.out, d)
    with open(os.path.join(a.out, "chunk_tiny.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
