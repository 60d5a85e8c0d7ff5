#!/usr/bin/env python3
"""What a shorter encoder window buys on the benchmarked model.

whisper-large-v3-turbo dims, random weights, at chunk_length 30, 15, 10 and 5 (clips of exactly
one window each), written to profiles/chunk_length_bench.json:

  encoder_ms        the encoder stage (conv stem + 32 layers + ln_post) at 1, 4 and 64 windows
  batch1_p50_ms     one transcribe_batch call on one clip, greedy and beam 5, 24 new tokens
  xattn_us          microseconds per launch of the decoder cross-attention kernel at 64 windows,
                    greedy (dec_xattn_chunk_kernel<1, XU>) and beam 5 (dec_xattn_mfma_kernel<5, NT>),
                    with the instantiation the launcher picks at that T ("short") and with the
                    full-width form forced ("full", OSW_XATTN_FULL=1): what decides whether the
                    short instantiations are kept

Every measurement runs in a child process of its own (a fresh context; OSW_XATTN_FULL is read once
per process) under its own time limit, one after the other; the first child that fails, faults or
runs out of time ends the run.  Run it once per GPU visit:

    python tools/chunk_length_bench.py [--out profiles/chunk_length_bench.json] [--chunks 30,15,10,5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 150


def child(kind: str, s: int) -> dict:
    sys.path.insert(0, ROOT)
    import numpy as np

    import osw_path
    osw_path.load()
    from open_speech_amd import dims as D
    from open_speech_amd import synth
    from open_speech_amd.engine import DecodeConfig, WhisperEngine
    from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

    d = D.LARGE_V3_TURBO.with_chunk_length(s)
    nb = 64 if kind in ("enc", "xattn") else 1
    eng = WhisperEngine(d, device=0, max_batch=nb)
    try:
        eng.init_random(seed=0)
        sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
        clips = [synth.chirp_clip(i % 8, float(s)) for i in range(nb)]
        out = {"chunk_length": s, "n_audio_ctx": d.n_audio_ctx}
        if kind == "enc":
            out["encoder_ms"] = {}
            for n in (1, 4, 64):
                eng.log_mel(clips[:n])
                wins = [(i, 0, d.n_frames) for i in range(n)]
                eng.encode(wins)            # warm
                eng.encode(wins)
                ms = []
                for _ in range(7):
                    eng.set_profiling(True)
                    eng.encode(wins)
                    ms.append(eng.profile()["encoder_ms"])
                eng.set_profiling(False)
                out["encoder_ms"][str(n)] = {"p50": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
        elif kind == "batch1":
            out["batch1_p50_ms"] = {}
            for name, beam in (("greedy", 1), ("beam5", 5)):
                cfg = DecodeConfig(suppress_tokens=sup, max_length=3 + 24, beam_size=beam)
                for _ in range(3):
                    eng.transcribe_batch(clips[:1], cfg)
                ms = []
                for _ in range(15):
                    t = time.perf_counter()
                    eng.transcribe_batch(clips[:1], cfg)
                    ms.append(1e3 * (time.perf_counter() - t))
                out["batch1_p50_ms"][name] = {"p50": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
        else:
            out["form"] = "full" if os.environ.get("OSW_XATTN_FULL") else "short"
            out["xattn_us"] = {}
            n = 64
            eng.log_mel(clips[:n])
            for name, beam in (("greedy", 1), ("beam5", 5)):
                eng.encode([(i, 0, d.n_frames) for i in range(n)])
                cfg = DecodeConfig(suppress_tokens=sup, max_length=3 + 16, beam_size=beam)
                eng.decode(n, cfg)          # warm
                per = []
                for _ in range(5):
                    eng.set_profiling(True, eager_decode=True)
                    eng.decode(n, cfg)
                    p = eng.profile()
                    per.append(1e3 * p["xattn_ms"] / max(1, p["xattn_launches"]))
                eng.set_profiling(False)
                out["xattn_us"][name] = {"windows": n, "p50": float(np.median(per)), "min": float(min(per)),
                                         "max": float(max(per))}
        return out
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_length_bench.json"))
    ap.add_argument("--chunks", default="30,15,10,5")
    ap.add_argument("--child", nargs=2, metavar=("KIND", "SECONDS"))
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child[0], int(a.child[1]))))
        return 0
    results = {"model": "large-v3-turbo (random weights)", "runs": []}
    steps = []
    for s in (int(x) for x in a.chunks.split(",")):
        steps += [("enc", s, {}), ("batch1", s, {}), ("xattn", s, {}), ("xattn", s, {"OSW_XATTN_FULL": "1"})]
    rc = 0
    for kind, s, env in steps:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", kind, str(s)]
        p = subprocess.run(cmd, env={**os.environ, **env}, capture_output=True, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(f"{kind} chunk_length {s} {env}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
            results["stopped_at"] = {"kind": kind, "chunk_length": s, "env": env, "exit_status": p.returncode}
            rc = 1
            break
        results["runs"].append(json.loads(line[len("RESULT "):]))
        print(kind, s, env, line[len("RESULT "):], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(results, fh, indent=1)
    print("wrote", a.out)
    return rc


if __name__ == "__main__":
    sys.exit(main())
