"""Decoder time per step, English-only vs multilingual decoding at the same dims in one run:
TINY_TEST / TINY_EN_TEST and the turbo dims with n_vocab 51866 / 51864, greedy at batch 1 (the
fused selection), batch 16 (select_kernel) and beam 5 at batch 4, token budgets fixing the
length.  Prints one JSON line."""
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import osw_path

osw_path.load()
from open_speech_amd import dims as D
from open_speech_amd import synth
from open_speech_amd.engine import DecodeConfig, WhisperEngine

N_TOK = 96
REPS = 7


def run(d, label):
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    eng = WhisperEngine(d, device=0, max_batch=16)
    eng.init_random(seed=0)
    sup = (st.transcribe, st.translate, st.sot, st.sot_prev, st.sot_lm)
    clips = [synth.chirp_clip(i, 30.0) for i in range(16)]
    out = {}
    for name, nb, beam in (("greedy_b1", 1, 1), ("greedy_b16", 16, 1), ("beam5_b4", 4, 5)):
        eng.log_mel(clips[:nb])
        eng.encode([(i, 0, 3000) for i in range(nb)])
        cfg = DecodeConfig(suppress_tokens=sup, max_length=448, beam_size=beam, token_budget=(N_TOK,) * nb,
                           language_token=st.first_lang if st.multilingual else None)
        ts = []
        steps = None
        for r in range(REPS + 2):
            t0 = time.perf_counter()
            o = eng.decode(nb, cfg)
            ts.append(time.perf_counter() - t0)
            steps = eng.profile()["decode_steps"] if hasattr(eng, "profile") else None
        ts = sorted(ts[2:])
        n = len(o[0].tokens)
        out[name] = {"ms_median": round(ts[len(ts) // 2] * 1e3, 3), "ms_min": round(ts[0] * 1e3, 3),
                     "ms_max": round(ts[-1] * 1e3, 3), "tokens": n, "decode_steps": steps,
                     "us_per_step": round(ts[len(ts) // 2] * 1e6 / max(1, steps or n), 2)}
    eng.close()
    return out


res = {}
for label, d in (("tiny_multilingual", D.TINY_TEST), ("tiny_english", D.TINY_EN_TEST),
                 ("turbo_multilingual", D.LARGE_V3_TURBO),
                 ("turbo_english", dataclasses.replace(D.LARGE_V3_TURBO, n_vocab=51864))):
    res[label] = run(d, label)
print(json.dumps({"what": "decode wall time, token budget %d, median of %d" % (N_TOK, REPS), "results": res}))
