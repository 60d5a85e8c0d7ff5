#!/usr/bin/env python3
"""What word timestamps cost on the continuous-batching lanes, on
random:large-v3-turbo with length control, printed as JSON lines and written to --out.

(a) the mixed-length REST load of tools/rest_probe.py (clips of 4-75 s, C callers x R calls,
    jittered think time) with word timing on every call: STT_HIP_WORD_SESSIONS=0 (the batched seek
    loop of an idle lane: the routing before the sessions held windows) against =1 (hold / align /
    release on the sessions).  Two backends stay loaded, one per setting, and the rounds alternate
    between them, so both see the same machine; calls/s and latency percentiles per round.
(b) one engine, one hold session with a long window decoding throughout: the wall time of one
    osw_session_align call against its windows and token counts (the call ends in a stream
    synchronise), the time of a decoder chunk of the co-resident window on its own, and the gap
    that window sees from the end of one chunk to the end of the next with such a call in between.

usage: word_session_bench.py [--callers 16] [--calls 6] [--jitter-ms 40] [--rounds 3] [--skip-load]
                             [--skip-align] [--out profiles/word_session_bench.json]"""
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
from open_speech_amd.engine import AlignWindow, DecodeConfig, WhisperEngine  # noqa: E402
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens  # noqa: E402

MID = "random:large-v3-turbo"
LENS = (4.0, 12.0, 30.0, 45.0, 75.0, 20.0, 8.0, 60.0)     # tools/rest_probe.py's mix


def emit(rows, **kw):
    rows.append(kw)
    print(json.dumps(kw), flush=True)


# ------------------------------------------------------------------ (a) the REST mix
def load_round(be, wavs, callers, calls, jitter_ms):
    lat, lock = [], threading.Lock()

    def caller(i):
        rng = np.random.default_rng(i)
        for k in range(calls):
            time.sleep(rng.exponential(jitter_ms / 1000.0))
            t = time.perf_counter()
            be.transcribe(audio=wavs[(i + k) % len(wavs)], model=MID, language=None, response_format="verbose_json",
                          word_timestamps=True)
            with lock:
                lat.append((time.perf_counter() - t) * 1e3)

    ts = [threading.Thread(target=caller, args=(i,)) for i in range(callers)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    wall = time.perf_counter() - t0
    return dict(calls_per_s=len(lat) / wall, p50_ms=float(np.median(lat)), p95_ms=float(np.percentile(lat, 95)),
                audio_s_per_s=sum(LENS[(i + k) % 8] for i in range(callers) for k in range(calls)) / wall)


def rest_mix(rows, a):
    wavs = [pcm_to_wav(synth.chirp_clip(800 + i, s).tobytes(), 16000) for i, s in enumerate(LENS)]
    backends = {}
    for knob in ("0", "1"):     # (the runner reads the knob when the model loads)
        os.environ["STT_HIP_WORD_SESSIONS"] = knob
        be = HipWhisperBackend(length_control=4.0)
        be.load_model(MID)
        backends[knob] = be
    os.environ.pop("STT_HIP_WORD_SESSIONS")
    try:
        same = []
        for knob, be in backends.items():   # warm: graphs of both paths; and the answers agree
            for w in (wavs[0], wavs[3]):
                r = be.transcribe(audio=w, model=MID, language=None, response_format="verbose_json", word_timestamps=True)
                same.append(json.dumps(r, sort_keys=True))
            load_round(be, wavs, a.callers, 1, a.jitter_ms)
        emit(rows, part="a", what="answers of the two paths equal (4 s and 45 s clips)",
             equal=same[0] == same[2] and same[1] == same[3])
        for rnd in range(a.rounds):
            for knob, be in backends.items():
                emit(rows, part="a", word_sessions=int(knob), round=rnd, callers=a.callers, calls=a.calls,
                     jitter_ms=a.jitter_ms, **load_round(be, wavs, a.callers, a.calls, a.jitter_ms))
        for knob in backends:
            rs = [r for r in rows if r.get("part") == "a" and r.get("word_sessions") == int(knob)]
            emit(rows, part="a", summary=True, word_sessions=int(knob),
                 calls_per_s=[round(r["calls_per_s"], 2) for r in rs], p50_ms=[round(r["p50_ms"], 1) for r in rs],
                 p95_ms=[round(r["p95_ms"], 1) for r in rs])
    finally:
        for be in backends.values():
            be.unload_model(MID)


# ------------------------------------------------------------------ (b) one align call
def align_cost(rows, a):
    d = D.LARGE_V3_TURBO
    st = SpecialTokens.for_vocab(d.n_vocab)
    eng = WhisperEngine(d, device=0, max_batch=16)
    try:
        eng.init_random(seed=0)
        sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
        for beam in (1, 5):
            cfg = DecodeConfig(suppress_tokens=sup, max_length=448, beam_size=beam)
            long_pcm, short_pcm = synth.chirp_clip(1, 30.0), synth.chirp_clip(2, 30.0)
            for n_win, n_tok in ((1, 8), (1, 32), (1, 128), (1, 224), (4, 32), (4, 128), (8, 32)):
                toks = [(200 + 37 * j) % (st.eot - 1) + 1 for j in range(n_tok)]
                eng.session_begin(cfg, hold=True)
                try:
                    # the co-resident window: no budget, runs to max_length (111 chunks of 4 steps)
                    eng.session_add([dict(tag=0, clip=0, pcm=long_pcm, seek=0, segment_size=3000,
                                          language_token=st.first_lang, token_budget=0)])
                    t_align, t_gap, t_step = [], [], []
                    tag = 0
                    for rep in range(4):        # (rep 0 warms: graph capture of this shape)
                        new = []
                        for _ in range(n_win):
                            tag += 1
                            new.append(dict(tag=tag, clip=1, pcm=short_pcm if tag == 1 else None, seek=0,
                                            segment_size=3000, language_token=st.first_lang, token_budget=4))
                        eng.session_add(new)
                        eng.session_step(max_chunks=0)
                        held = {}
                        while len(held) < n_win:
                            done, active, _ = eng.session_step(max_chunks=1)
                            held.update(done)
                            assert 0 not in held, "the long window ended: shorten the sweep"
                        t_end = time.perf_counter()                         # the end of a chunk
                        req = [(t, AlignWindow(window=0, tokens=toks, num_frames=3000, language=o.language))
                               for t, o in held.items()]
                        t0 = time.perf_counter()
                        eng.session_align(req)
                        t1 = time.perf_counter()
                        done, _, _ = eng.session_step(max_chunks=1)
                        t2 = time.perf_counter()
                        assert not done
                        if rep:
                            t_align.append((t1 - t0) * 1e3)
                            t_gap.append((t2 - t_end) * 1e3)
                        for _ in range(3):                                  # the long window on its own
                            t0 = time.perf_counter()
                            done, _, _ = eng.session_step(max_chunks=1)
                            assert not done
                            if rep:
                                t_step.append((time.perf_counter() - t0) * 1e3)
                    emit(rows, part="b", beam=beam, windows=n_win, n_tokens=n_tok, forced_steps=n_tok + 5,
                         align_ms=[round(x, 2) for x in t_align], align_ms_median=round(float(np.median(t_align)), 2),
                         chunk_alone_ms_median=round(float(np.median(t_step)), 2),
                         chunk_gap_with_align_ms_median=round(float(np.median(t_gap)), 2))
                finally:
                    eng.session_end()
    finally:
        eng.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--callers", type=int, default=16)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--jitter-ms", type=float, default=40.0)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--skip-load", action="store_true")
    p.add_argument("--skip-align", action="store_true")
    p.add_argument("--out", default=os.path.join("profiles", "word_session_bench.json"))
    a = p.parse_args()
    rows = []
    try:
        if not a.skip_align:
            align_cost(rows, a)
        if not a.skip_load:
            rest_mix(rows, a)
    finally:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
