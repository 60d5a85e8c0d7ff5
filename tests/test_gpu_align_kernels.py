"""The word-timestamp alignment kernels of csrc/align.hip one at a time, each through the
production launcher (osw_debug_align_post / _tail / _self_attn / _scores), against the float64
references of tests/align_kernels_ref.py on crafted inputs (the same cases the CPU tests check
the conditions of: tests/test_align_kernels_ref_cpu.py).

Bounds.  u = 2^-24 is the fp32 unit roundoff; every fp32 add, multiply, fma, divide and sqrt is
correctly rounded (relative u); expf and logf are taken at the 1 ulp (2 u relative) the HIP math
API documentation states.  All bounds are first order, times 1.001 for the higher-order terms.

  block_sum of n positive terms: a thread adds its ceil(n/256) terms in order, the wave tree
      has 6 levels, the four wave sums take 3 adds: depth(n) = ceil(n/256) - 1 + 9 roundings on
      the longest path, so the sum is relative depth(n) u from the sum of the terms as computed.
  stats (align_softmax_stats_kernel): the maximum is exact.  A term expf(x - m) carries the
      rounding of x - m (absolute |x - m| u in the exponent, so relative |x - m| u) and expf's
      2 u.  The sum is within (depth(TK) + 2 + dbar) u relative, dbar = sum(w d) / sum(w) the
      term-weighted mean of d = m - x, w = e^-d: (TK/256 + c) u with c <= 11 + dbar, dbar <= ln TK.
  p = expf(x - m) / s from the GPU's own m and s: |p_gpu - p| <= ep = p (|x - m| + 2 + 1) u.
  colstats (align_colstats_kernel), from the scores and the GPU's stats: the mean adds P
      positive terms in order and divides: |mean_gpu - mean| <= P u mean + mean(ep), relative
      (P + c) u.  The variance sums fma(d, d, var) over d = p - mean_gpu: a common shift of all d
      by the mean's error e_m changes sum d^2 only by P e_m^2 (sum d = 0), so
      |sum d_gpu^2 - sum d^2| <= sum(2 |d| (ep + u |d|) + (ep + |e_m| + u |d|)^2) + (P + 1) u sum d^2
      (P fmas and the division), and the std is relative half of that over sum d^2, plus u for
      the sqrt.  A column whose sum d^2 is exactly 0 must give exactly 0.
  M (align_matrix_kernel), from the scores and the GPU's stats and colstats:
      z = (p - mean) / std has |z_gpu - z| <= (ep + 2 u (p + |mean|)) / std, which is
      C u (p + |mean|) / std with C = 2 + (|x - m| + 3) p / (p + |mean|) <= 5 + |x - m|.  The
      median (any order statistic) is 1-Lipschitz in the sup norm, so a filtered element is
      within the largest such bound over its window (reflect-padded); the bound of M[t][f] is
      the largest over the window and over the heads, plus n_heads u mean_h max|z| for the head
      mean's n_heads - 1 adds and one division.  NaN: an element is NaN in the reference
      (np.sort orders NaN last, as torch.sort does in transformers' _median_filter) exactly where
      it must be NaN on the GPU; the bound holds on the rest.
  tail: (lg[tok] - m) - logf(s): u |lg[tok] - m| + the relative bound of s (absolute in the log)
      + 2 u |ln s| for logf + u |result|.
  self-attention: q, k and v are the fp32 in-order slab sums the reference restates bit for bit
      (the cache rows at pos are compared exactly).  A score is 64 sequential fmas:
      |ds| <= 64 u sum|k q| / 8.  A weight e^(s - m) is relative e = ds + ds_max + u (m - s) + 2 u.
      out = sum w v / sum w: the weights' errors enter numerator and denominator (2 max e), the
      sum l depth(n) u, the 4-way P V sums ceil(n/4) fmas + 3 adds, one division, all times
      a = sum p |v|.  The fp16 hi + lo pair adds 2^-22 |out| + 2^-25 (lo may be subnormal).
  scores: q is bit-identical to fp16 of the fp32 slab sum in reduce_head's order (checked
      exactly through unit-vector keys, where a score is q[d] / 8); otherwise 64 sequential
      fmas: 64 u sum|k q| / 8.

Each test prints its largest error / bound ratio (DESIGN.md records them).
"""
import numpy as np
import pytest

from open_speech_amd import dims as D
from open_speech_amd import weights
from open_speech_amd.engine import WhisperEngine

import align_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    d = D.MICRO_TEST
    e = WhisperEngine(d, device=0, max_batch=1)
    e.load_weights(weights.random_weights(d, seed=1, emb_std=0.5))
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ratio(err, bound):
    """max err / bound over the finite entries (err == 0 counts as 0 whatever the bound)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nanmax(r)) if r.size else 0.0


# ------------------------------------------------------------------------------ post-processing
def run_post(eng, case):
    sl = np.array(case["slots"], np.int32)
    return eng.debug_align_post(case["scores"], sl[:, 0], sl[:, 1], sl[:, 2], sl[:, 3])


def check_post(case, stats, cs, M):
    """Stage by stage: every kernel judged on the inputs it received.  Returns the three ratios."""
    live_st, live_cs, live_M = R.live_masks(case)
    for name, got, live in (("stats", stats, live_st), ("colstats", cs, live_cs), ("M", M, live_M)):
        assert (bits(got)[~live] == R.FILL).all(), f"{name}: a store outside the live region"
    worst = [0.0, 0.0, 0.0]
    for s, (P, hd, F, W) in enumerate(case["slots"]):
        sc = case["scores"][s]
        # stats from the scores
        ref = R.softmax_stats(sc[:, :P])
        np.testing.assert_array_equal(stats[s, :, :P, 0], sc[:, :P].max(-1))
        rs = np.abs(stats[s, :, :P, 1] - ref[..., 1]) / ref[..., 1]
        worst[0] = max(worst[0], ratio(rs, R.stats_sum_rel_bound(sc[:, :P])))
        # colstats from the scores and the GPU's stats
        cref = R.colstats(sc, stats[s], P, F)
        tm, ts = R.colstats_bounds(sc, stats[s], P, F)
        zero = cref[..., 1] == 0
        assert (cs[s, :, :F, 1][zero] == 0).all(), "a zero-variance column must have std exactly 0"
        worst[1] = max(worst[1], ratio(np.abs(cs[s, :, :F, 0] - cref[..., 0]), tm),
                       ratio(np.abs(cs[s, :, :F, 1] - cref[..., 1])[~zero], ts[~zero]))
        # M from the scores, the GPU's stats and the GPU's colstats
        with np.errstate(invalid="ignore", divide="ignore"):
            Mref = R.matrix(sc, stats[s], cs[s], P, F, hd, W)
            bound = R.matrix_bound(sc, stats[s], cs[s], P, F, hd, W)
        got = M[s, :P - hd - 1, :F]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(Mref), err_msg="NaN where the reference has none, or the reverse")
        fin = ~np.isnan(Mref)
        if not case["degenerate"]:
            assert fin.all()
        both_inf = np.isinf(Mref) & (got == Mref)
        err = np.where(both_inf, 0.0, np.abs(got.astype(np.float64) - Mref))
        worst[2] = max(worst[2], ratio(err[fin], bound[fin]))
    print(f"{case['name']}: max error/bound  stats {worst[0]:.3f}  colstats {worst[1]:.3f}  M {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst
    return worst


POST = {c["name"]: c for c in R.post_cases()}


@pytest.mark.parametrize("name", list(POST))
def test_post_stages_against_float64(eng, name):
    case = POST[name]
    stats, cs, M = run_post(eng, case)
    check_post(case, stats, cs, M)
    if "nan_columns" in case:   # the constant columns, and only they, are NaN before the filter
        P, hd, F, W = case["slots"][0]
        assert sorted(np.flatnonzero(cs[0, 0, :F, 1] == 0).tolist()) == case["nan_columns"]


def test_post_row_offset_leaves_matrix_unchanged(eng):
    """+1e4 on two rows (exact in fp32 on the 1/64 grid) is the same softmax: M moves by no more
    than the two launches' end-to-end bounds."""
    base, off = POST["peaked"], POST["peaked_offset"]
    P, hd, F, W = base["slots"][0]
    assert np.array_equal(R.matrix_full(base["scores"][0], P, F, hd, W), R.matrix_full(off["scores"][0], P, F, hd, W))
    out = [run_post(eng, c) for c in (base, off)]
    b = [R.matrix_bound(c["scores"][0], st[0], cs[0], P, F, hd, W, end_to_end=True) for c, (st, cs, M) in zip((base, off), out)]
    diff = np.abs(out[0][2][0, :P - hd - 1, :F].astype(np.float64) - out[1][2][0, :P - hd - 1, :F])
    r = ratio(diff, b[0] + b[1])
    print(f"row offset: max |dM| {diff.max():.3e}, error/bound {r:.3f}")
    assert r <= 1.0
    # and each launch against the float64 chain from the scores alone
    for c, (st, cs, M), bb in zip((base, off), out, b):
        ref = R.matrix_full(c["scores"][0], P, F, hd, W)
        r = ratio(np.abs(M[0, :P - hd - 1, :F] - ref), bb)
        print(f"{c['name']}: end-to-end error/bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("case", R.multi_slot_cases(), ids=lambda c: c["name"])
def test_post_slots_of_one_launch(eng, case):
    """Three slots that differ in len, head, frames and width: each is right by itself (float64),
    equals its single-slot launch bit for bit, and nothing outside the live regions is written."""
    stats, cs, M = run_post(eng, case)
    check_post(case, stats, cs, M)
    for s in range(len(case["slots"])):
        st1, cs1, M1 = run_post(eng, R.single_slot(case, s))
        np.testing.assert_array_equal(bits(st1[0]), bits(stats[s]))
        np.testing.assert_array_equal(bits(cs1[0]), bits(cs[s]))
        np.testing.assert_array_equal(bits(M1[0]), bits(M[s]))


def test_post_argument_errors(eng):
    from open_speech_amd._lib import OswError
    sc = np.zeros((1, 1, 16, 8), np.float32)
    good = dict(length=[8], head=[3], frames=[8], width=[7])
    eng.debug_align_post(sc, **good)
    for bad in (dict(length=[17]), dict(length=[4]), dict(frames=[0]), dict(frames=[9]), dict(width=[6]),
                dict(width=[17]), dict(head=[2])):
        with pytest.raises(OswError):
            eng.debug_align_post(sc, **{**good, **bad})
    with pytest.raises(OswError):   # pstride % 16
        eng.debug_align_post(np.zeros((1, 1, 12, 8), np.float32), **good)


# ------------------------------------------------------------------------------ tail
@pytest.mark.parametrize("head", [1, 3])
@pytest.mark.parametrize("eot", R.TAIL_EOTS)
def test_tail_logprob_and_row_state(eng, eot, head):
    case = R.tail_case(eot, head)
    worst, far = 0.0, 0
    for pos in R.TAIL_POSITIONS:
        lp0, ct0, dn0 = R.tail_fill(case)
        lp, ct, dn = eng.debug_align_tail(case["logits"], eot, pos, case["slot"], case["length"], case["head"],
                                          case["forced"], lp0, ct0, dn0)
        elp, wr, ect, edn = R.tail_expected(pos, case["slot"], case["length"], case["head"], case["forced"],
                                            lp0, ct0, dn0, case["logits"], eot)
        np.testing.assert_array_equal(ct, ect)
        np.testing.assert_array_equal(dn, edn)
        assert (bits(lp)[~wr] == R.FILL).all(), f"pos {pos}: a log-probability written where none belongs"
        for sl, i in zip(*np.nonzero(wr)):
            r = int(np.flatnonzero(case["slot"] == sl)[0])
            tok = int(case["forced"][r, pos + 1])
            assert np.isfinite(lp[sl, i])
            far += elp[sl, i] < -150
            worst = max(worst, abs(float(lp[sl, i]) - elp[sl, i]) / R.tail_bound(case["logits"][r], eot, tok))
    print(f"eot {eot} head {head}: max error/bound {worst:.3f} ({far} tokens 200 below the maximum)")
    assert worst <= 1.0
    assert far >= 1 or eot < 5


def test_tail_argument_errors(eng):
    from open_speech_amd._lib import OswError
    case = R.tail_case(5, 3)
    lp0, ct0, dn0 = R.tail_fill(case)
    args = [case["logits"], 5, 0, case["slot"], case["length"], case["head"], case["forced"], lp0, ct0, dn0]
    for i, bad in ((1, 0), (1, 13), (2, -1), (3, [0, 0, 1, 2]), (3, [0, 1, 2, 3]), (4, [25, 1, 1, 1])):
        a = list(args)
        a[i] = bad
        with pytest.raises(OswError):
            eng.debug_align_tail(*a)
    f = case["forced"].copy()
    f[0, 0] = 12
    a = list(args)
    a[6] = f
    with pytest.raises(OswError):
        eng.debug_align_tail(*a)


# ------------------------------------------------------------------------------ self-attention
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("pos", R.SELF_POSITIONS)
def test_self_attn_against_float64(eng, pos, H, ks):
    c = R.self_attn_case(pos, H, ks)
    out, kc, vc = eng.debug_align_self_attn(c["slabs"], c["bias"], c["kc"], c["vc"], pos, c["done"])
    ref, rkc, rvc = R.self_attn(c["slabs"], c["bias"], c["kc"], c["vc"], pos, c["done"])
    # the cache: fp32 k and v at min(pos, ctx - 1) exactly, every other position bit-identical
    np.testing.assert_array_equal(bits(kc), bits(rkc))
    np.testing.assert_array_equal(bits(vc), bits(rvc))
    assert np.isnan(out[1]).all() and not np.isnan(out[[0, 2]]).any()   # the done row keeps its fill
    bound = R.self_attn_bound(c["slabs"], c["bias"], c["kc"], c["vc"], pos, c["done"])
    r = [ratio(np.abs(out[b] - ref[b]), bound[b]) for b in (0, 2)]
    print(f"pos {pos} H {H} ks {ks}: max error/bound peaked {r[0]:.3f} near-uniform {r[1]:.3f}")
    assert max(r) <= 1.0


# ------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("ks", R.SCORE_KS)
@pytest.mark.parametrize("T", R.SCORE_TS)
def test_scores_against_float64(eng, T, ks):
    worst = 0.0
    for with_bias, pos in ((True, 0), (False, R.SCORE_PSTRIDE - 1)):
        c = R.scores_case(T, ks, with_bias, pos)
        got = eng.debug_align_scores(c["slabs"], c["bias"], c["K"], c["layer_heads"], c["n_heads"], pos, c["slot"],
                                     c["length"], c["scores"])
        ref, wr, bound = R.scores(c["slabs"], c["bias"], c["K"], c["layer_heads"], c["n_heads"], pos, c["slot"],
                                  c["length"], c["scores"])
        assert wr.sum() == 2 * 2 * T                       # two live rows, two listed heads, row pos only
        assert (bits(got)[~wr] == R.FILL).all(), "a score written outside row pos of a live slot's listed heads"
        # unit-vector keys: q bit-identical to fp16 of the fp32 slab sum in reduce_head's order
        np.testing.assert_array_equal(got[1, :, pos][wr[1, :, pos]], ref[1, :, pos][wr[1, :, pos]].astype(np.float32))
        worst = max(worst, ratio(np.abs(got[2][wr[2]] - ref[2][wr[2]]), bound[2][wr[2]]))
    print(f"T {T} ks {ks}: max error/bound {worst:.3f}")
    assert worst <= 1.0


def test_scores_argument_errors(eng):
    from open_speech_amd._lib import OswError
    c = R.scores_case(7, 1, True, 0)
    ok = dict(layer_heads=c["layer_heads"], n_heads=3, pos=0, slot=c["slot"], length=c["length"])
    for bad in (dict(layer_heads=[(6, 0)]), dict(layer_heads=[(0, 3)]), dict(layer_heads=[(0, 1), (2, 1)]),
                dict(slot=[0, 0, 1, 2]), dict(slot=[3, -1, 0, 1]), dict(length=[17, 1, 1, 1]), dict(pos=-1)):
        kw = {**ok, **bad}
        with pytest.raises(OswError):
            eng.debug_align_scores(c["slabs"], c["bias"], c["K"], kw["layer_heads"], kw["n_heads"], kw["pos"], kw["slot"],
                                   kw["length"], c["scores"])
