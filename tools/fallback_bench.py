#!/usr/bin/env python
"""Cost of a temperature-fallback retry through the window-list decode (osw_decode_window_list).

One process, one GPU, whisper-large-v3-turbo dims with random weights, 16 windows encoded once,
every window length-controlled to ``--tokens`` sampled tokens (random weights never emit
<|endoftext|>).  Decode ms (median of ``--reps`` repeats after a warm-up, with min / max) of
    the plain decode of all 16 windows (greedy and beam 5: attempt 0 of a chunk),
    a retry of 1, 4 and 16 of them through the list entry, sampled at temperature 0.4 with
    best_of 5 rows per window (faster-whisper's retry), and greedy (the same rows as the plain
    decode, so the map's own cost shows),
and, for scale, what a retry would cost without the list entry: encoding the 1 / 4 windows again
and decoding them.  Prints one JSON line and writes it to profiles/fallback_bench.json.

    python tools/fallback_bench.py [--tokens 60] [--reps 5] [--out profiles/fallback_bench.json]
"""
from __future__ import annotations

import argparse
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

N_WINDOWS = 16


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fallback_bench.json"))
    a = ap.parse_args()
    d = D.LARGE_V3_TURBO
    eng = WhisperEngine(d, device=0, max_batch=N_WINDOWS)
    eng.init_random(seed=0)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    eng.log_mel([synth.chirp_clip(i, 30.0) for i in range(N_WINDOWS)])
    wins = [(i, 0, 3000) for i in range(N_WINDOWS)]
    eng.encode(wins)

    def cfg(n, **kw):
        return DecodeConfig(suppress_tokens=sup, token_budget=tuple([a.tokens] * n), **kw)

    result = {"metric": "fallback_retry_decode_ms", "model": "large-v3-turbo (random weights)",
              "windows_encoded": N_WINDOWS, "token_budget": a.tokens, "reps": a.reps, "plain": {}, "retry": []}
    for name, kw in (("greedy", {}), ("beam5", dict(beam_size=5))):
        result["plain"][name] = timed(lambda: eng.decode(N_WINDOWS, cfg(N_WINDOWS, **kw)), a.reps)
    for n in (1, 4, N_WINDOWS):
        # the failed windows are spread over the chunk, the last one included
        which = sorted({N_WINDOWS - 1 - (i * N_WINDOWS) // n for i in range(n)})
        row = {"windows": n, "list": which}
        row["sampled_t0.4_best_of5"] = timed(
            lambda: eng.decode(n, cfg(n, temperature=0.4, best_of=5, seed=1), windows=which), a.reps)
        row["greedy"] = timed(lambda: eng.decode(n, cfg(n), windows=which), a.reps)
        result["retry"].append(row)
    for row in result["retry"][:2]:   # without the list entry: the failed windows through the encoder again
        n, which = row["windows"], row["list"]

        def again():
            eng.encode([wins[i] for i in which])
            eng.decode(n, cfg(n, temperature=0.4, best_of=5, seed=1))
        row["encode_again_sampled_t0.4_best_of5"] = timed(again, a.reps)
    eng.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
