#!/usr/bin/env python
"""Cost of the history rules (repetition_penalty / no_repeat_ngram_size) on the decode.

One process, one GPU, whisper-large-v3-turbo dims with random weights, every window
length-controlled to ``--tokens`` sampled tokens (random weights never emit <|endoftext|>).
Decode ms (median of ``--reps`` repeats after a warm-up, with min / max) for
    64 windows greedy, 1 window greedy (the case that gives up the fused selection),
    64 windows x beam 5,
each with the rules off, with no_repeat_ngram_size = 3, and with repetition_penalty = 1.3
and no_repeat_ngram_size = 3 together; and the kernel's own time per launch (HIP events).
Prints one JSON line and writes it to profiles/history_rules_bench.json.

On a tree without the rules (the parent commit, for the rules-off comparison in the same
GPU visit) only the rules-off cases run.

    python tools/history_rules_bench.py [--tokens 60] [--reps 5] [--out profiles/history_rules_bench.json]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import osw_path  # noqa: E402

osw_path.load()
from open_speech_amd import dims as D  # noqa: E402
from open_speech_amd import synth  # noqa: E402
from open_speech_amd.engine import DecodeConfig, WhisperEngine  # noqa: E402
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens  # noqa: E402

HAS_RULES = "repetition_penalty" in {f.name for f in dataclasses.fields(DecodeConfig)}
RULES = [("off", {})]
if HAS_RULES:
    RULES += [("ngram3", dict(no_repeat_ngram_size=3)),
              ("penalty1.3_ngram3", dict(repetition_penalty=1.3, no_repeat_ngram_size=3))]


def timed(fn, reps):
    fn()                      # warm-up: graph capture, lazy buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=60, help="sampled tokens per window (token budget)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_rules_bench.json"))
    a = ap.parse_args()
    d = D.LARGE_V3_TURBO
    eng = WhisperEngine(d, device=0, max_batch=64)
    eng.init_random(seed=0)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    result = {"metric": "history_rules_decode_ms", "model": "large-v3-turbo (random weights)", "label": a.label,
              "token_budget": a.tokens, "reps": a.reps, "cases": [], "kernel_us_per_launch": []}
    for nw, beam in ((64, 1), (1, 1), (64, 5)):
        eng.log_mel([synth.chirp_clip(i, 30.0) for i in range(nw)])
        eng.encode([(i, 0, 3000) for i in range(nw)])
        case = {"windows": nw, "beam_size": beam}
        for name, kw in RULES:
            cfg = DecodeConfig(suppress_tokens=sup, beam_size=beam, token_budget=tuple([a.tokens] * nw), **kw)
            t = timed(lambda: eng.decode(nw, cfg), a.reps)
            t["decode_steps"] = int(eng.profile()["decode_steps"])
            case[name] = t
        for name, _ in RULES[1:]:
            extra = case[name]["median_ms"] - case["off"]["median_ms"]
            case[name]["over_off_ms"] = round(extra, 3)
            case[name]["over_off_us_per_step"] = round(extra * 1e3 / max(1, case[name]["decode_steps"]), 3)
        result["cases"].append(case)
    if HAS_RULES:
        for rows in (1, 64, 320):
            for n_hist in (1, 60, 447):
                for name, kw in RULES[1:]:
                    us = eng.debug_history_rules_time(rows, n_hist, iters=200, **kw)
                    result["kernel_us_per_launch"].append({"rows": rows, "n_hist": n_hist, "rules": name,
                                                           "us": round(us, 3)})
    eng.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
