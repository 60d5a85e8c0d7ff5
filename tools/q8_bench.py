#!/usr/bin/env python3
"""What int8 decoder weights (STT_COMPUTE_TYPE=int8_float16) buy on the benchmarked model
(DESIGN.md §4.9).  whisper-large-v3-turbo dims, numpy-random int8 decoder matrices with their
multipliers; the float16 side holds fp16(q * mult), the same model.  float16 and int8 alternate
within every measurement.  Written to profiles/q8_bench.json:

  projections     per-launch HIP-event microseconds of launch_gemm_skinny_partial at the decoder's
                  four projection shapes, 1, 5 and 64 hi/lo rows, >= 200 launches each after a
                  warm-up, over weight replicas totalling >= 512 MB per stream (walked round robin:
                  a launch finds its weights where a decoder step does, not in the L2);
                  algorithmic weight bytes (N K 2 float16; N K + 4 N int8) and bytes / p50 as TB/s
  logits_select   the batch-1 logits GEMM with the fused selection (51866 x 1280), per launch, from
                  HIP events around it in eagerly launched greedy steps: the mean over a run's 223
                  launches, two runs per compute type (both kept), the lower one reported
  batch1_p50_ms   one greedy transcribe_batch call on one 30 s clip, 64 new tokens
  batch64         greedy audio-seconds per second at 64 clips of 30 s, 64 new tokens

  --float16-only  only the float16 side of batch1_p50_ms and batch64, through calls that exist
                  without int8 support; with --root CHECKOUT the package of another checkout (the
                  parent commit, built) is measured by the same call pattern, for the run-to-run and
                  commit-to-commit spread of the default path.

Every measurement runs in a child process under its own time limit, one after the other; the first
child that fails, faults or runs out of time ends the run.

    python tools/q8_bench.py [--out profiles/q8_bench.json] [--float16-only] [--root CHECKOUT]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT_S = 420
PROJ = ((3840, 1280), (1280, 1280), (5120, 1280), (1280, 5120))
ROWS = (1, 5, 64)
NEW_TOKENS = 64


def stats(x):
    import numpy as np
    x = np.asarray(x, dtype=np.float64)
    return {"p50": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "mean": float(x.mean()),
            "n": int(x.size)}


def random_q8(rng, N, K, std):
    """numpy-random int8 with one multiplier per row: q * mult has about the given standard deviation."""
    import numpy as np
    q = rng.integers(-127, 128, (N, K), dtype=np.int8)
    mult = (std / 73.3 * rng.uniform(0.8, 1.25, N)).astype(np.float32)   # std of U{-127..127} is 73.3
    return q, mult


def child_proj(root):
    import numpy as np
    from open_speech_amd import dims as D
    from open_speech_amd.engine import WhisperEngine
    eng = WhisperEngine(D.MICRO_TEST, device=0, max_batch=1)
    rng = np.random.default_rng(0)
    out = {"projections": []}
    try:
        for N, K in PROJ:
            q, mult = random_q8(rng, N, K, 0.02)
            copies = -(-(512 << 20) // (N * K * 2))
            for M in ROWS:
                a = rng.uniform(-1, 1, (M, K)).astype(np.float32)
                hi = a.astype(np.float16)
                lo = (a - hi.astype(np.float32)).astype(np.float16)
                f16, q8 = eng.debug_dec_gemm_time(hi, lo, q, mult, copies=copies, warm=20, launches=200)
                b16, b8 = N * K * 2, N * K + 4 * N
                row = {"N": N, "K": K, "M": M, "copies": copies, "float16_us": stats(f16), "int8_us": stats(q8),
                       "float16_weight_bytes": b16, "int8_weight_bytes": b8}
                row["float16_TBps"] = b16 / (row["float16_us"]["p50"] * 1e-6) / 1e12
                row["int8_TBps"] = b8 / (row["int8_us"]["p50"] * 1e-6) / 1e12
                out["projections"].append(row)
                print(json.dumps(row), flush=True)
    finally:
        eng.close()
    return out


def make_engines(nb, float16_only):
    """Two turbo engines on one model: float16 holding fp16(q * mult), int8 holding q and mult."""
    import numpy as np
    from open_speech_amd import dims as D
    from open_speech_amd.engine import WhisperEngine
    d = D.LARGE_V3_TURBO
    rng = np.random.default_rng(1)
    names = ["dec.tok"] + [f"dec.l{i}.{k}.w" for i in range(d.n_text_layer) for k in ("qkv", "o", "xq", "xo", "fc1", "fc2")]
    Dd = d.n_text_state
    shape = {"tok": (d.n_vocab, Dd), "qkv": (3 * Dd, Dd), "o": (Dd, Dd), "xq": (Dd, Dd), "xo": (Dd, Dd),
             "fc1": (4 * Dd, Dd), "fc2": (Dd, 4 * Dd)}
    engines = {"float16": WhisperEngine(d, device=0, max_batch=nb)}
    if not float16_only:
        engines["int8"] = WhisperEngine(d, device=0, max_batch=nb)
    for e in engines.values():
        e.init_random(seed=0)
    for n in names:
        kind = "tok" if n == "dec.tok" else n.split(".")[2]
        q, mult = random_q8(rng, *shape[kind], 0.02)
        engines["float16"].set_weight(n, (q.astype(np.float32) * mult[:, None]).astype(np.float16))
        if not float16_only:
            engines["int8"].set_weight_q8(n, q, mult)
    return d, engines


def child_model(root, float16_only):
    import numpy as np
    from open_speech_amd import synth
    from open_speech_amd.engine import DecodeConfig
    from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens
    nb = 64
    d, engines = make_engines(nb, float16_only)
    out = {}
    try:
        sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
        clips = [synth.chirp_clip(i % 8, 30.0) for i in range(nb)]
        cfg = DecodeConfig(suppress_tokens=sup, max_length=3 + NEW_TOKENS)
        order = list(engines)
        # batch-1 greedy p50
        ms = {k: [] for k in order}
        for k in order:
            for _ in range(3):
                engines[k].transcribe_batch(clips[:1], cfg)
        for _ in range(15):
            for k in order:
                t = time.perf_counter()
                engines[k].transcribe_batch(clips[:1], cfg)
                ms[k].append(1e3 * (time.perf_counter() - t))
        out["batch1_p50_ms"] = {k: stats(v) for k, v in ms.items()}
        print(json.dumps(out["batch1_p50_ms"]), flush=True)
        # 64 clips
        s = {k: [] for k in order}
        for k in order:
            engines[k].transcribe_batch(clips, cfg)
        for _ in range(5):
            for k in order:
                t = time.perf_counter()
                engines[k].transcribe_batch(clips, cfg)
                s[k].append(nb * 30.0 / (time.perf_counter() - t))
        out["batch64"] = {k: {"audio_s_per_s": stats(v)} for k, v in s.items()}
        print(json.dumps(out["batch64"]), flush=True)
        if not float16_only:
            # the logits GEMM with the fused selection, per launch (eager steps, HIP events)
            long_cfg = DecodeConfig(suppress_tokens=sup, max_length=3 + 220)
            per = {k: [] for k in order}
            for _ in range(2):
                for k in order:
                    e = engines[k]
                    e.set_profiling(True, eager_decode=True)
                    e.transcribe_batch(clips[:1], long_cfg)
                    ms_, n = e.debug_logits_profile()
                    e.set_profiling(False)
                    per[k].append({"us_per_launch": 1e3 * ms_ / max(1, n), "launches": n})
            b16, b8 = d.n_vocab * d.n_text_state * 2, d.n_vocab * d.n_text_state + 4 * d.n_vocab
            out["logits_select"] = {"N": d.n_vocab, "K": d.n_text_state, "float16_weight_bytes": b16,
                                    "int8_weight_bytes": b8, "runs": per}
            for k, b in (("float16", b16), ("int8", b8)):   # the figure: the lower of the two runs' means
                us = min(r["us_per_launch"] for r in per[k])
                out["logits_select"][k + "_us"] = us
                out["logits_select"][k + "_TBps"] = b / (us * 1e-6) / 1e12
            print(json.dumps(out["logits_select"]), flush=True)
    finally:
        for e in engines.values():
            e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q8_bench.json"))
    ap.add_argument("--float16-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is measured")
    ap.add_argument("--child", metavar="KIND")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.abspath(a.root))
        import osw_path
        osw_path.load()
        r = child_proj(a.root) if a.child == "proj" else child_model(a.root, a.float16_only)
        print("RESULT " + json.dumps(r))
        return 0
    results = {"model": "large-v3-turbo dims, numpy-random int8 decoder matrices", "root": os.path.relpath(os.path.abspath(a.root), ROOT),
               "float16_only": a.float16_only}
    rc = 0
    for kind in (["model"] if a.float16_only else ["proj", "model"]):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", kind,
               "--root", a.root] + (["--float16-only"] if a.float16_only else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(f"{kind}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
            results["stopped_at"] = {"kind": kind, "exit_status": p.returncode}
            rc = 1
            break
        results.update(json.loads(line[len("RESULT "):]))
        print(kind, line[len("RESULT "):][:2000], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(results, fh, indent=1)
    print("wrote", a.out)
    return rc


if __name__ == "__main__":
    sys.exit(main())
