"""The token-selection kernels on crafted logits and state: select_kernel<0..2> (select.h
select_partial_body / combine_parts / select_finalize), beam_slice_body and beam_update_body<5|8>
(csrc/decode.hip), one step at a time through osw_debug_select_step, against the float64
reference tests/select_ref.py (pinned to oracle.decode in test_select_ref_cpu.py).

The inputs are the scenarios of tests/select_cases.py, at the three vocabularies the project
serves (51864, 51865, 51866): crafted single steps, and scripted runs of 28 to 36 steps on a stub
model, compared with the reference after every step and with oracle.decode at the end.  Discrete
outputs (tokens, state integers, histories, ancestry, BeamWin counts, best_tok, step counters,
the arrival / ticket counters left zeroed) are compared exactly; floats (sum_lp, lp_hist, best_lp,
best_raw, best_norm, log nsp, log lang_probs) within 1e-4 + 1e-3 |ref|, the per-token replay bound
of test_gpu_confidences.py.  test_select_ref_cpu.py asserts on the reference alone that every
deciding comparison of every scenario is an exact tie of identical inputs or >= 1e-2 apart.

Worst observed ratio to the float bound (MI355X; also in DESIGN.md section 2): 0.015 log lang_probs
(sot_step_groups), 0.005 log nsp (sot_step), 0.004 sum_lp of greedy single steps, 0.002 scripted
greedy / sampling runs, 0.004 the scripted beam 5 session run, 0.0005 every other beam scenario.  The bound is not tightened to them."""
import numpy as np
import pytest

import select_cases as sc
import select_ref as R
from open_speech_amd.engine import WhisperEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(V):
        if V not in made:
            made[V] = WhisperEngine(sc.dims(V), device=0, max_batch=16)   # selection alone: no weights needed
        return made[V]

    yield get
    for e in made.values():
        e.close()


def _run(eng, case):
    """The case's steps on the GPU, each compared with the reference; (worst ratio, final state)."""
    sr, steps = sc.run_reference(case)
    assert sr.gaps.min >= R.GAP, (sr.gaps.min, sr.gaps.where)
    g = R.to_engine(case.state)
    worst = 0.0
    for i, (_, logits) in enumerate(steps[:-1]):
        out = eng.debug_select_step(case.cfg, {**g, "logits": logits}, case.mode, case.n_prefix)
        worst = max(worst, R.compare(out, steps[i + 1][0], sr, f"step {i}"))
        g = {k: v for k, v in out.items() if k not in ("counters", "logits")}
    return sr, worst, g


@pytest.mark.parametrize("name", sorted(sc.SCENARIOS))
def test_scenario(engines, name):
    case = sc.SCENARIOS[name]()
    sr, worst, g = _run(engines(case.V), case)
    print(f"{name}: worst ratio to the bound {worst:.4f}")
    if case.expect is None:
        return
    for w, (toks, raw) in case.expect.items():     # the scripted run ends where oracle.decode ends
        s = g["state"][w * sr.group]
        assert s["done"] == 1
        if sr.beam > 1:
            bw = g["bwin"][w]
            got, got_raw = g["best_tok"][w, :bw["best_len"]].tolist(), bw["best_raw"]
        else:
            got, got_raw = g["tokens"][w, :s["n_sampled"]].tolist(), s["sum_lp"]
        assert got == toks, (name, w, got, toks)
        assert R.bound_ratio(got_raw, raw) <= 1.0, (name, w, got_raw, raw)


def test_entry_refuses_bad_arguments(engines):
    """Everything that could make a kernel index out of bounds is refused on the host, before any
    launch; a valid call afterwards still finds the counters zeroed and passes."""
    V = 51865
    eng = engines(V)
    ctx = sc.dims(V).n_text_ctx

    def refused(case, **change):
        st = {**R.to_engine(case.state), "logits": case.logits}
        mode = change.pop("mode", case.mode)
        for k, f in change.items():
            st[k] = f(st[k].copy())
        with pytest.raises(RuntimeError):
            eng.debug_select_step(case.cfg, st, mode, case.n_prefix)

    def put(idx, val, field=None):
        def f(a):
            if field:
                a[field][idx] = val
            else:
                a[idx] = val
            return a
        return f

    greedy = sc.SCENARIOS[f"timestamp_pairs-{V}"]()       # refill, 8 rows
    beam = sc.SCENARIOS[f"beam_eot-top-{V}"]()            # batch, beam 5, one window, 2 tokens in
    sess = sc.SCENARIOS[f"beam_long_history-{V}"]()       # session, beam 5, 3 windows
    mt = greedy.ref().max_tok
    for bad in (-1, ctx):
        refused(greedy, pos=put(3, bad))                   # a step counter outside [0, n_text_ctx)
    refused(greedy, pos=put(3, 9))                         # a sampling row's counter is not plen - 1 + n_sampled
    for bad in (-1, mt + 1):
        refused(greedy, state=put(2, bad, "n_sampled"))
    refused(greedy, state=put(2, 3, "plen"))               # plen outside a session
    refused(greedy, state=put(2, V, "lang"))
    for bad in (-1, V):
        refused(greedy, tokens=put((0, 1), bad))           # a history token outside [0, V)
        refused(greedy, prompt=put((1, 2), bad))           # a prompt token; -1 only at the language position
    refused(greedy, prompt=put((1, 0), V))
    refused(greedy, tokens=lambda a: a[:, :-1])            # undersized: not the plan's max_tok
    refused(greedy, logits=lambda a: a[:-1])
    refused(greedy, cur_tok=lambda a: a[:-1])
    refused(greedy, lp_hist=lambda a: a[:, :-1])
    refused(greedy, mode="session")                        # the prompt stride is not a session's
    big = sc.Case(V, greedy.cfg, greedy.ref().initial_state(17), "refill", logits=np.zeros((17, V), np.float32))
    refused(big)                                           # more windows than max_batch
    refused(beam, state=lambda a: a[:4], logits=lambda a: a[:4])       # rows not a multiple of the beam
    refused(beam, state=put(3, 1, "n_sampled"))            # rows of one window differ
    refused(beam, state=put(3, 1, "done"))
    refused(beam, anc=put((2, 1), 5))                      # an ancestry entry outside the window's rows
    refused(beam, anc=put((2, 0), -1))
    refused(beam, anc=lambda a: a[:, :-1])
    refused(beam, bwin=lambda a: a[:0])
    refused(sess, state=put(slice(10, 15), 2, "plen"))     # a session row's plen below the start sequence
    refused(sess, state=put(slice(10, 15), ctx, "plen"))
    refused(sess, pos=put(11, 1))                          # rows of one window at different counters
    refused(sess, anc=put((7, 1), 4))                      # window 1's rows are 5..9
    for case in (greedy, beam, sess):
        _run(eng, case)
