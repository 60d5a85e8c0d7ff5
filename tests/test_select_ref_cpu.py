"""tests/select_ref.py against the pinned oracle, and the margins of every GPU scenario.

1. A stub model whose logits are a seeded function of the tokens fed so far is decoded twice:
   by ``oracle.decode.greedy_from_encoder`` / ``beam_from_encoder``, and by driving
   ``SelectRef.step`` one physical-row step at a time.  Tokens, hypotheses and scores must be
   the same, exactly.
2. Every scenario of tests/select_cases.py (what test_gpu_select.py feeds the kernels) is run
   through the reference alone: each deciding comparison must be an exact tie of identical
   inputs or at least ``GAP`` apart, so no case sits where a float32 kernel may differ."""
import dataclasses

import numpy as np
import pytest

import english_ref as er
import select_cases as sc
import select_ref as R
from open_speech_amd import dims as D
from open_speech_amd.engine import DecodeConfig
from oracle import decode as odec


def _dims(V):
    return dataclasses.replace(D.MICRO_TEST, n_vocab=V)


def _result(sr, state, w=0):
    s = state["state"][w * sr.group]
    if sr.beam > 1:
        bw = state["bwin"][w]
        return [int(t) for t in state["best_tok"][w, :bw["best_len"]]], float(bw["best_raw"])
    return [int(t) for t in state["tokens"][w, :s["n_sampled"]]], float(s["sum_lp"])


@pytest.mark.parametrize("V", [51864, 51865, 51866])
@pytest.mark.parametrize("without_ts", [False, True])
@pytest.mark.parametrize("beam", [1, 2, 5, 8])
def test_stepwise_reference_reproduces_the_oracle(V, without_ts, beam):
    d = _dims(V)
    st = D.SpecialTokens.for_vocab(V)
    for seed, max_length, patience, lp in ((1, 28, 1.0, 1.0), (2, 40, 2.0, 0.0)):
        cfg = DecodeConfig(without_timestamps=without_ts, max_length=max_length, beam_size=beam, patience=patience,
                           length_penalty=lp, num_hypotheses=1 if seed == 1 else 3,
                           suppress_tokens=(1, 31, 32, 50000, V - 1))
        fn = R.make_logits_fn(V, 100 * beam + seed, st)
        sr = R.SelectRef(d, cfg, "batch")
        state = R.drive(sr, sr.initial_state(1), fn, max_length, sr.step)
        if st.multilingual:
            ref_fn = odec.greedy_from_encoder if beam == 1 else odec.beam_from_encoder
            kw = {} if beam == 1 else dict(beam=odec.BeamOptions(beam_size=beam, patience=patience, length_penalty=lp,
                                                                num_hypotheses=cfg.num_hypotheses))
            ref = ref_fn(R.StubOracle(fn), None, st, opts=sr.opts, **kw)
        else:
            ref = (er.greedy_from_encoder(R.StubOracle(fn), None, st, opts=sr.opts) if beam == 1 else
                   er.beam_from_encoder(R.StubOracle(fn), None, st, opts=sr.opts, beam=odec.BeamOptions(
                       beam_size=beam, patience=patience, length_penalty=lp, num_hypotheses=cfg.num_hypotheses)))
        toks, raw = _result(sr, state)
        s0 = state["state"][0]
        assert toks == ref.tokens and raw == ref.sum_logprob, (toks, ref.tokens, raw, ref.sum_logprob)
        assert float(s0["nsp"]) == ref.no_speech_prob
        if st.multilingual:
            assert int(s0["lang"]) == ref.language
        if beam > 1:
            assert [(t, s, n) for _, t, s, n in sr.finished] == ref.hypotheses
            assert state["bwin"]["done"][0] == 1 and state["bwin"]["n_hyp"][0] == len(ref.hypotheses)
        assert s0["done"] == 1 and len(toks) > 2


@pytest.mark.parametrize("name", sorted(sc.SCENARIOS))
def test_scenario_margins(name):
    """The reference alone: every deciding comparison of the scenario is a tie of identical inputs
    or >= GAP apart, and no row enters a step with a cumulative score of -inf."""
    case = sc.SCENARIOS[name]()
    sr, steps = sc.run_reference(case)
    assert sr.gaps.count > 0
    assert sr.gaps.min >= R.GAP, (name, sr.gaps.min, sr.gaps.where)
    for state, _ in steps[:-1]:
        live = state["state"]["done"] == 0
        assert np.all(np.isfinite(state["state"]["sum_lp"][live])), name


def test_bound_ratio_and_compare_bite():
    assert R.bound_ratio([1.0, -np.inf], [1.0, -np.inf]) == 0.0
    assert R.bound_ratio([-np.inf], [-5.0]) == np.inf
    assert R.bound_ratio([-5.0 - 0.0052], [-5.0]) > 1.0 > R.bound_ratio([-5.0 - 0.0050], [-5.0])
