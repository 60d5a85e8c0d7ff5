#!/usr/bin/env python
"""Cost of word-timestamp alignment next to the decode it follows.

One process, one GPU, whisper-large-v3-turbo dims with random weights: for 64 windows and
for 1 window, time ``decode`` (greedy, length-controlled to the golden's token count, since
random weights never emit <|endoftext|>) and then ``align`` of the same windows with that
many text tokens each.  Prints one JSON line and writes it to profiles/align_bench.json.

    python tools/align_bench.py [--tokens 60] [--reps 5] [--out profiles/align_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import osw_path  # noqa: E402

osw_path.load()
from open_speech_amd import dims as D  # noqa: E402
from open_speech_amd import synth  # noqa: E402
from open_speech_amd.engine import AlignWindow, DecodeConfig, WhisperEngine  # noqa: E402
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens  # noqa: E402


def timed(fn, reps):
    fn()                      # warm-up: graph capture, lazy buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=60, help="text tokens per window (the turbo golden's count)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    a = ap.parse_args()
    d = D.LARGE_V3_TURBO
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    eng = WhisperEngine(d, device=0, max_batch=64)
    eng.init_random(seed=0)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    rng = np.random.default_rng(0)
    result = {"metric": "align_vs_decode_ms", "model": "large-v3-turbo (random weights)", "text_tokens": a.tokens,
              "reps": a.reps, "cases": []}
    for nw in (64, 1):
        eng.log_mel([synth.chirp_clip(i, 30.0) for i in range(nw)])
        eng.encode([(i, 0, 3000) for i in range(nw)])
        # decode: text tokens + about as many timestamp tokens as a real transcript carries is
        # not reproducible with random weights, so the budget is the text-token count alone
        cfg = DecodeConfig(suppress_tokens=sup, token_budget=tuple([a.tokens] * nw))
        outs = eng.decode(nw, cfg)
        steps = eng.profile()["decode_steps"]
        wins = [AlignWindow(window=i, tokens=rng.integers(0, st.eot, a.tokens).tolist(), num_frames=3000,
                            language=outs[i].language) for i in range(nw)]
        dec_ms = timed(lambda: eng.decode(nw, cfg), a.reps)
        al_ms = timed(lambda: eng.align(wins), a.reps)
        result["cases"].append({"windows": nw, "decode_ms": round(dec_ms, 3), "decode_steps": int(steps),
                                "align_ms": round(al_ms, 3), "align_steps": a.tokens + 5,
                                "align_over_decode": round(al_ms / dec_ms, 3)})
    eng.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
