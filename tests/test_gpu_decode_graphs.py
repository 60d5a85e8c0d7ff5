"""Which decode calls share a captured graph (csrc/plan.h DecodePlan::key): a fresh child process
with OSW_TRACE_GRAPH=1 makes seven calls on the tiny model and this test counts the `instantiated`
lines the library writes to stderr during each.  The counts follow from the key rule alone: a
graph is captured once per (mode, selection parameters, rows, chunk), and the seed, the language
token and the rest of a call's data replay it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import dataclasses, sys
sys.path.insert(0, %r)
import osw_path
osw_path.load()
from open_speech_amd import dims as D, synth, weights
from open_speech_amd.dims import SpecialTokens
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

def mark(k):
    sys.stderr.write("[call %%d]\\n" %% k)
    sys.stderr.flush()

d = D.TINY_TEST
st = SpecialTokens.for_vocab(d.n_vocab)
eng = WhisperEngine(d, device=0, max_batch=2)
eng.load_weights(weights.random_weights(d, seed=1234, emb_std=0.5))
sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
clips = [synth.chirp_clip(40, 30.0), synth.chirp_clip(41, 12.5)]
cfg = DecodeConfig(suppress_tokens=sup, max_length=40, token_budget=(12, 12))
mark(1)
first = eng.transcribe_batch(clips, cfg)
mark(2)
eng.transcribe_batch(clips, dataclasses.replace(cfg, seed=77, language_token=st.first_lang + 3))
mark(3)
eng.transcribe_batch(clips, dataclasses.replace(cfg, max_length=48))
mark(4)
eng.transcribe_batch(clips, dataclasses.replace(cfg, beam_size=2))
mark(5)
eng.transcribe_refill(clips, cfg, refill_min=1)
mark(6)
eng.session_begin(dataclasses.replace(cfg, token_budget=None))
wins = [dict(tag=i, pcm=p, seek=0, segment_size=min(3000, len(p) // 160), token_budget=12)
        for i, p in enumerate(clips)]
eng.session_add(wins)
done, guard = 0, 0
while done < 2:
    res, active, queued = eng.session_step(max_chunks=4, refill_min=1)
    done += len(res)
    guard += 1
    assert guard < 100
eng.session_end()
mark(7)
again = eng.transcribe_batch(clips, cfg)
mark(8)
assert [o.tokens for o in again] == [o.tokens for o in first], (first, again)
eng.close()
print("OK")
"""


def test_graphs_per_call():
    env = dict(os.environ, OSW_TRACE_GRAPH="1")
    env.pop("OSW_NO_GRAPH", None)
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD % ROOT], env=env,
                       capture_output=True, text=True, timeout=150)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("OK")
    counts, call = {}, 0
    for line in p.stderr.splitlines():
        if line.startswith("[call "):
            call = int(line[6:-1])
        elif line.startswith("[osw-graph]") and line.endswith(" instantiated"):
            counts[call] = counts.get(call, 0) + 1
    # 1: a new graph.  2: another seed and language token replay it.  3: max_length is in the key.
    # 4: beam 2.  5: refill (its own mode, rows = max_batch).  6: a session at beam 1 whose two
    # windows share a budget, so it only ever steps 2 occupied rows: one graph.  7: call 1's graph.
    assert [counts.get(k, 0) for k in range(1, 8)] == [1, 0, 1, 1, 1, 1, 0], (counts, p.stderr[-3000:])
