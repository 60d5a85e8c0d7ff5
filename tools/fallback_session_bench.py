#!/usr/bin/env python3
"""What a temperature ladder costs on the continuous-batching lanes, on
random:large-v3-turbo with length control, printed as JSON lines and written to --out.

(a) the mixed-length REST load of tools/rest_probe.py (clips of 4-75 s, C callers x R calls,
    jittered think time) with the ladder (0.0, 0.4, 0.8) on every call and a log_prob_threshold
    placed at the --share quantile of the windows' temperature-0 avg_logprob (a calibration pass
    without the ladder), so that about that share of the windows retries:
    STT_HIP_FALLBACK_SESSIONS=0 (the batched seek loop of an idle lane: the routing before the
    sessions retried windows in place) against =1.  Two backends stay loaded, one per setting, and
    the rounds alternate between them; calls/s and latency percentiles per round.
(b) the price of arming: the time of one decoder chunk (4 steps) of a session with W windows
    decoding, none of which fails, begun without retries (today's ladder-free session) and with
    retries (best_of rows per slot in a greedy session, the extra select path in a beam-5 one).
(c) one retry: the time from ``session_retry`` of one held window (token budget 60, best_of 5 at
    T = 0.4: the shape of §4.6's list-decode retry) to the step that returns it, beside N windows
    that go on decoding.

usage: fallback_session_bench.py --part a|b|c [--callers 16] [--calls 6] [--jitter-ms 40] [--rounds 3]
                                 [--share 0.25] [--out profiles/fallback_session_bench.json]
(one part per run: each fits one GPU visit; --out is appended to, part by part)"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osw_path  # noqa: E402

osw_path.load()
from open_speech_amd import dims as D  # noqa: E402
from open_speech_amd import synth  # noqa: E402
from open_speech_amd.audio import pcm_to_wav  # noqa: E402
from open_speech_amd.backend import HipWhisperBackend  # noqa: E402
from open_speech_amd.dims import SpecialTokens  # noqa: E402
from open_speech_amd.engine import DecodeConfig, WhisperEngine  # noqa: E402
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens  # noqa: E402

MID = "random:large-v3-turbo"
LENS = (4.0, 12.0, 30.0, 45.0, 75.0, 20.0, 8.0, 60.0)     # tools/rest_probe.py's mix
LADDER = (0.0, 0.4, 0.8)


def emit(rows, **kw):
    rows.append(kw)
    print(json.dumps(kw), flush=True)


# ------------------------------------------------------------------ (a) the REST mix
def load_round(be, wavs, callers, calls, jitter_ms, thr):
    lat, lock = [], threading.Lock()
    temps = []

    def caller(i):
        rng = np.random.default_rng(i)
        for k in range(calls):
            time.sleep(rng.exponential(jitter_ms / 1000.0))
            t = time.perf_counter()
            r = be.transcribe(audio=wavs[(i + k) % len(wavs)], model=MID, language=None, response_format="verbose_json",
                              temperature=LADDER, log_prob_threshold=thr, compression_ratio_threshold=1e9)
            with lock:
                lat.append((time.perf_counter() - t) * 1e3)
                temps.extend(s["temperature"] for s in r.get("segments", []))

    ts = [threading.Thread(target=caller, args=(i,)) for i in range(callers)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    wall = time.perf_counter() - t0
    return dict(calls_per_s=len(lat) / wall, p50_ms=float(np.median(lat)), p95_ms=float(np.percentile(lat, 95)),
                audio_s_per_s=sum(LENS[(i + k) % 8] for i in range(callers) for k in range(calls)) / wall,
                segments_retried_share=float(np.mean([t > 0 for t in temps])) if temps else 0.0)


def rest_mix(rows, a):
    wavs = [pcm_to_wav(synth.chirp_clip(800 + i, s).tobytes(), 16000) for i, s in enumerate(LENS)]
    backends = {}
    for knob in ("0", "1"):     # (the runner reads the knob when the model loads)
        os.environ["STT_HIP_FALLBACK_SESSIONS"] = knob
        be = HipWhisperBackend(length_control=4.0)
        be.load_model(MID)
        backends[knob] = be
    os.environ.pop("STT_HIP_FALLBACK_SESSIONS")
    try:
        # calibration: the windows' temperature-0 avg_logprob without the ladder
        avgs = []
        for w in wavs:
            r = backends["1"].transcribe(audio=w, model=MID, language=None, response_format="verbose_json")
            avgs += [s["avg_logprob"] for s in r.get("segments", [])]
        thr = float(np.quantile(avgs, a.share))
        emit(rows, part="a", what="calibration", segments=len(avgs), share=a.share, log_prob_threshold=thr,
             share_below=float(np.mean([x < thr for x in avgs])))
        same = []
        for knob, be in backends.items():   # warm: graphs of both paths; and the answers agree
            for w in (wavs[0], wavs[3]):
                r = be.transcribe(audio=w, model=MID, language=None, response_format="verbose_json", temperature=LADDER,
                                  log_prob_threshold=thr, compression_ratio_threshold=1e9)
                same.append(json.dumps(r, sort_keys=True))
            load_round(be, wavs, a.callers, 1, a.jitter_ms, thr)
        emit(rows, part="a", what="answers of the two paths equal (4 s and 45 s clips)",
             equal=same[0] == same[2] and same[1] == same[3])
        for rnd in range(a.rounds):
            for knob, be in backends.items():
                emit(rows, part="a", fallback_sessions=int(knob), round=rnd, callers=a.callers, calls=a.calls,
                     jitter_ms=a.jitter_ms, **load_round(be, wavs, a.callers, a.calls, a.jitter_ms, thr))
        for knob in backends:
            rs = [r for r in rows if r.get("part") == "a" and r.get("fallback_sessions") == int(knob)]
            emit(rows, part="a", summary=True, fallback_sessions=int(knob),
                 calls_per_s=[round(r["calls_per_s"], 2) for r in rs], p50_ms=[round(r["p50_ms"], 1) for r in rs],
                 p95_ms=[round(r["p95_ms"], 1) for r in rs],
                 segments_retried_share=[round(r["segments_retried_share"], 3) for r in rs])
    finally:
        for be in backends.values():
            be.unload_model(MID)


# ------------------------------------------------------------------ (b), (c): one engine
def engine():
    d = D.LARGE_V3_TURBO
    eng = WhisperEngine(d, device=0, max_batch=16)
    eng.init_random(seed=0)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    return d, eng, sup


def window(tag, pcm, lang, budget):
    return dict(tag=tag, clip=tag, pcm=pcm, seek=0, segment_size=3000, language_token=lang, token_budget=budget)


def arming(rows, a):
    d, eng, sup = engine()
    st = SpecialTokens.for_vocab(d.n_vocab)
    try:
        pcms = [synth.chirp_clip(10 + i, 30.0) for i in range(8)]
        for beam in (1, 5):
            cfg = DecodeConfig(suppress_tokens=sup, max_length=448, beam_size=beam)
            for n_win in (1, 4, 8):
                for rnd in range(2):
                    for retries in (None, 5):
                        eng.session_begin(cfg, hold=True, retries=retries)
                        try:
                            # no budget: every window runs to max_length (111 chunks), none finishes here
                            eng.session_add([window(i, pcms[i], st.first_lang, 0) for i in range(n_win)])
                            eng.session_step(max_chunks=0)
                            ts = []
                            for i in range(60):
                                t0 = time.perf_counter()
                                done, _, _ = eng.session_step(max_chunks=1)
                                assert not done
                                if i >= 10:     # (the first chunks capture the graph)
                                    ts.append((time.perf_counter() - t0) * 1e3)
                        finally:
                            eng.session_end()
                        emit(rows, part="b", beam=beam, windows=n_win, round=rnd, retries=retries or 0,
                             rows_per_slot=max(beam, retries or 0), chunk_ms_median=round(float(np.median(ts)), 3),
                             chunk_ms_p10=round(float(np.percentile(ts, 10)), 3),
                             chunk_ms_p90=round(float(np.percentile(ts, 90)), 3))
    finally:
        eng.close()


def one_retry(rows, a):
    d, eng, sup = engine()
    st = SpecialTokens.for_vocab(d.n_vocab)
    try:
        pcms = [synth.chirp_clip(10 + i, 30.0) for i in range(9)]
        for beam in (1, 5):
            cfg = DecodeConfig(suppress_tokens=sup, max_length=448, beam_size=beam)
            for n_busy in (0, 1, 7):
                eng.session_begin(cfg, hold=True, retries=5)
                try:
                    if n_busy:
                        eng.session_add([window(100 + i, pcms[1 + i], st.first_lang, 0) for i in range(n_busy)])
                    eng.session_add([window(1, pcms[0], st.first_lang, 60)])
                    eng.session_step(max_chunks=0)
                    out = None
                    while out is None:
                        done, _, _ = eng.session_step(max_chunks=1)
                        out = dict(done).get(1)
                    ts, chunks = [], []
                    for rep in range(4):        # (rep 0 warms; the busy windows run 111 chunks in all)
                        t0 = time.perf_counter()
                        eng.session_retry([(1, 0.4, 1000 + rep, out.language)])
                        n, got = 0, None
                        while got is None:
                            done, _, _ = eng.session_step(max_chunks=1)
                            n += 1
                            got = dict(done).get(1)
                        if rep:
                            ts.append((time.perf_counter() - t0) * 1e3)
                            chunks.append(n)
                    emit(rows, part="c", beam=beam, busy_windows=n_busy, best_of=5, temperature=0.4, token_budget=60,
                         retry_ms=[round(x, 2) for x in ts], retry_ms_median=round(float(np.median(ts)), 2),
                         chunks=chunks, list_decode_retry_ms_section_4_6=17.39)
                finally:
                    eng.session_end()
    finally:
        eng.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=("a", "b", "c"), required=True)
    p.add_argument("--callers", type=int, default=16)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--jitter-ms", type=float, default=40.0)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--share", type=float, default=0.25)
    p.add_argument("--out", default=os.path.join("profiles", "fallback_session_bench.json"))
    a = p.parse_args()
    rows = []
    try:
        {"a": rest_mix, "b": arming, "c": one_retry}[a.part](rows, a)
    finally:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        with open(a.out, "w") as f:
            json.dump([r for r in old if r.get("part") != a.part] + rows, f, indent=1)


if __name__ == "__main__":
    main()
