#!/usr/bin/env python
"""Cost of the confidences (per-token log-probabilities and language probabilities,
DecodeConfig.confidences) on the decode.

One process, one GPU, whisper-large-v3-turbo dims with random weights, every window
length-controlled to ``--tokens`` sampled tokens (random weights never emit <|endoftext|>).
Decode ms (median of ``--reps`` repeats after a warm-up, with min / max) for
    64 windows greedy (64 decoder rows), 1 window greedy (the fused batch-1 selection),
    64 windows x beam 5 (320 decoder rows),
each with the flag off and on, the difference per decoder step, and the time of one
``detect_language`` call for 1 and 64 windows.  The on-side timing includes the read-back of
the values (the getters after the decode call), as a caller pays it; ``getters_ms`` is that
host-side share measured alone, ``over_off_less_getters_us_per_step`` what remains per step.
Prints one JSON line and writes it to profiles/confidences_bench.json.

On a tree without the flag (the parent commit, for the flag-off comparison in the same GPU
visit) only the flag-off cases run.

    python tools/confidences_bench.py [--tokens 60] [--reps 5] [--out profiles/confidences_bench.json]
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

HAS_FLAG = "confidences" in {f.name for f in dataclasses.fields(DecodeConfig)}
FLAGS = [("off", {})] + ([("on", dict(confidences=True))] if HAS_FLAG else [])


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidences_bench.json"))
    a = ap.parse_args()
    d = D.LARGE_V3_TURBO
    eng = WhisperEngine(d, device=0, max_batch=64)
    eng.init_random(seed=0)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    result = {"metric": "confidences_decode_ms", "model": "large-v3-turbo (random weights)", "label": a.label,
              "token_budget": a.tokens, "reps": a.reps, "cases": [], "detect_language_ms": []}
    for nw, beam in ((64, 1), (1, 1), (64, 5)):
        eng.log_mel([synth.chirp_clip(i, 30.0) for i in range(nw)])
        eng.encode([(i, 0, 3000) for i in range(nw)])
        case = {"windows": nw, "beam_size": beam, "decoder_rows": nw * beam}
        for name, kw in FLAGS:
            cfg = DecodeConfig(suppress_tokens=sup, beam_size=beam, token_budget=tuple([a.tokens] * nw), **kw)
            t = timed(lambda: eng.decode(nw, cfg), a.reps)
            t["decode_steps"] = int(eng.profile()["decode_steps"])
            if name == "on":   # the host-side share: the getters alone, on the windows just decoded
                outs = eng.decode(nw, cfg)
                t["getters_ms"] = timed(lambda: eng._fetch_confidences(outs), a.reps)["median_ms"]
            case[name] = t
        if HAS_FLAG:
            extra = case["on"]["median_ms"] - case["off"]["median_ms"]
            case["on"]["over_off_ms"] = round(extra, 3)
            case["on"]["over_off_us_per_step"] = round(extra * 1e3 / max(1, case["on"]["decode_steps"]), 3)
            dev = extra - case["on"]["getters_ms"]   # what is left for the device and the read-back copies
            case["on"]["over_off_less_getters_us_per_step"] = round(dev * 1e3 / max(1, case["on"]["decode_steps"]), 3)
        result["cases"].append(case)
        if HAS_FLAG and beam == 1:
            t = timed(lambda: eng.detect_language(nw), a.reps)
            t["windows"] = nw
            result["detect_language_ms"].append(t)
    eng.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
