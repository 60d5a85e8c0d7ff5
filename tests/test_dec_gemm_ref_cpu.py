"""What the bounds of tests/dec_gemm_ref.py catch, shown on the CPU: the faithful float32
restatement meets every bound, and each wrong kernel the GPU tests are meant to catch misses
its bound by at least 20x on the inputs those tests use.  Every test prints
faithful-versus-mutant ratios (worst |err| / bound; <= 1 passes)."""
import numpy as np
import pytest

import dec_gemm_ref as R

F64 = np.float64
MISS = 20.0


def _gemm_ratio(C, hi, lo, W):
    return float((np.abs(C.astype(F64) - R.gemm_ref(hi, lo, W).sum(0)) / (R.G * R.gemm_scale(hi, lo, W))).max())


def test_measured_constants():
    """The constants written into dec_gemm_ref.py are what its measure_* functions give."""
    rows = R.measure_gemm()
    for fam, K, ks, e in rows:
        print(f"GEMM restatement {fam:9s} K {K:4d} ks {ks:2d}: worst |err|/S = {e:.3e}")
    worst = max(e for *_, e in rows)
    print(f"G_MEASURED = {worst:.4e}  G = {4 * worst:.4e}")
    assert worst <= R.G_MEASURED <= 1.01 * worst
    assert R.G == 4 * R.G_MEASURED
    ln = R.measure_ln()
    print("LN_RESTATE_WORST =", {k: f"{v:.3e}" for k, v in ln.items()})
    for k, v in ln.items():
        assert v <= R.LN_RESTATE_WORST[k] <= 1.02 * v
    ge = R.measure_gelu()
    print(f"GELU_RESTATE_WORST = {ge:.3e}")
    assert ge <= R.GELU_RESTATE_WORST <= 1.02 * ge


def test_exact_family_is_exact():
    """Every slab depth the GPU tests use keeps the exact family's partial sums in fp32, the
    float32 restatement and a float32 matrix product equal the float64 reference bit for bit, rows
    and columns are pairwise distinct, and every mutant moves an element by >= 2^-6."""
    for K, ks in R.GEMM_CASES:
        hi, lo, W = R.exact_inputs(40, 48, K, seed=K)
        R.assert_exact(hi, lo, W, K // ks)
        assert len(np.unique(np.concatenate([hi, lo], 1), axis=0)) == 40 and len(np.unique(W, axis=0)) == 48
        ref = R.gemm_ref(hi, lo, W, ks)
        assert np.array_equal(R.restate_gemm(hi, lo, W, ks).astype(F64), ref)
        assert np.array_equal(R.gemm_ref_exact(hi, lo, W, ks).astype(F64), ref)
        for mut in (dict(use_lo=False), dict(lo_row=np.r_[0:32, 0:8]), dict(skip=((ks - 1, K // ks // 32 - 1),))):
            d = np.abs(R.restate_gemm(hi, lo, W, ks, **mut).astype(F64) - ref)
            assert d.max() >= 2.0 ** -6, mut


@pytest.mark.parametrize("K,ks", R.GEMM_CASES)
def test_lo_half_ignored(K, ks):
    hi, lo, W = R.same_sign_inputs(16, 48, K, seed=3 * K + ks)
    ok = _gemm_ratio(R.sum_slabs(R.restate_gemm(hi, lo, W, ks)), hi, lo, W)
    bad = _gemm_ratio(R.sum_slabs(R.restate_gemm(hi, lo, W, ks, use_lo=False)), hi, lo, W)
    print(f"lo ignored, K {K} ks {ks}: faithful {ok:.3f}, mutant {bad:.1f}")
    assert ok <= 1 and bad >= MISS


@pytest.mark.parametrize("K,ks", [(384, 3), (1280, 5)])
def test_lo_from_row_minus_32(K, ks):
    """Rows 32..63 read the lo half of rows 0..31 (a second 32-row group staged from the first
    group's lo image)."""
    M = 64
    hi, lo, W = R.same_sign_inputs(M, 16, K, seed=K)
    wrong = np.r_[0:32, 0:32]
    ok = _gemm_ratio(R.sum_slabs(R.restate_gemm(hi, lo, W, ks)), hi, lo, W)
    bad = _gemm_ratio(R.sum_slabs(R.restate_gemm(hi, lo, W, ks, lo_row=wrong)), hi, lo, W)
    print(f"lo from row r - 32, K {K} ks {ks}: faithful {ok:.3f}, mutant {bad:.1f}")
    assert ok <= 1 and bad >= MISS


@pytest.mark.parametrize("family", ["same-sign", "uniform"])
def test_k32_step_skipped_at_the_seam(family):
    """kc = 384 in 256-deep chunks (the one-operand and the fused kernels): the second chunk is
    short and staged shifted; its first k32 step (step 8) is lost."""
    K, ks = 384, 1
    hi, lo, W = R.FAMILIES[family](16, 48, K, seed=17)
    for use in (lo, None):   # the hi/lo kernel and the one-operand kernel
        ok = _gemm_ratio(R.sum_slabs(R.restate_gemm(hi, use, W, ks)), hi, use, W)
        bad = _gemm_ratio(R.sum_slabs(R.restate_gemm(hi, use, W, ks, skip=((0, 8),))), hi, use, W)
        print(f"k32 step 8 of 12 skipped, {family}, lo {use is not None}: faithful {ok:.3f}, mutant {bad:.1f}")
        assert ok <= 1 and bad >= MISS


def _ln_ratio(y, tol, ref):
    return float((np.abs(y.astype(F64) - ref) / tol).max())


@pytest.mark.parametrize("ks", [20, 25])
def test_last_slab_left_out(ks):
    """The prologue's batched slab loads (24 per batch; 8 in the standalone kernel) lose the last
    slab: 20 is fc2's count at width 1280, 25 is past one batch."""
    for kind in R.LN_KINDS:
        x, slabs, b, g, sh, xp = R.ln_case(kind, 1, 1280, ks, True)
        tol, ref, _ = R.ln_tolerance(xp, g, sh)
        ok = _ln_ratio(R.restate_ln(xp, g, sh), tol, ref)
        xm = R.restate_resid(x, b, slabs[:-1])
        bad = _ln_ratio(R.restate_ln(xm, g, sh), tol, ref)
        print(f"last of {ks} slabs lost, {kind}: faithful {ok:.3f}, mutant {bad:.1f}")
        assert not np.array_equal(xm, xp)          # x' itself is compared bit for bit
        assert ok <= 1 and bad >= MISS


@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_one_pass_variance(D):
    x, slabs, b, g, sh, xp = R.ln_case("large-mean", 3, D, 3, True)
    tol, ref, _ = R.ln_tolerance(xp, g, sh)
    ok = _ln_ratio(R.restate_ln(xp, g, sh), tol, ref)
    bad = _ln_ratio(R.restate_ln(xp, g, sh, one_pass=True), tol, ref)
    print(f"one-pass variance, D {D}: faithful {ok:.3f}, mutant {bad:.1f}")
    assert ok <= 1 and bad >= MISS


@pytest.mark.parametrize("kind", R.LN_KINDS)
def test_tail_columns_left_out_of_the_statistics(kind):
    """Width 1280: the columns 1024 + t (one per thread) missing from the mean and the variance."""
    x, slabs, b, g, sh, xp = R.ln_case(kind, 3, 1280, 3, True)
    tol, ref, _ = R.ln_tolerance(xp, g, sh)
    ok = _ln_ratio(R.restate_ln(xp, g, sh), tol, ref)
    bad = _ln_ratio(R.restate_ln(xp, g, sh, drop_tail=True), tol, ref)
    print(f"columns 1024+t out of the statistics, {kind}: faithful {ok:.3f}, mutant {bad:.1f}")
    assert ok <= 1 and bad >= MISS


def test_restatements_are_what_they_say():
    """restate_resid / restate_gelu_sum add in slab order from the stated start; the embedding
    entry clamps ids into [0, V) and positions to ctx - 1; split_pair / pair_is_canonical agree."""
    rng = np.random.default_rng(0)
    x, slabs, b, g, sh = R.ln_inputs("plain", 2, 256, 9, seed=1)
    a = x + b
    s = np.zeros_like(x)
    for k in range(9):
        s = s + slabs[k]
    assert np.array_equal(R.restate_resid(x, b, slabs), a + s)
    assert not np.array_equal(R.restate_resid(x, b, slabs), R.restate_resid(x, b, slabs[::-1]))
    te = rng.standard_normal((10, 8)).astype(np.float16)
    pe = rng.standard_normal((6, 8)).astype(np.float32)
    e = R.restate_embed(te, pe, [-1, 10, 3], [2, 9, 0], 1)
    assert np.array_equal(e, te[[0, 9, 3]].astype(np.float32) + pe[[2, 5, 0]])
    e0 = R.restate_embed(te, pe, [-1, 10, 3], [7], 0)
    assert np.array_equal(e0, te[[0, 9, 3]].astype(np.float32) + pe[[5, 5, 5]])
    y = rng.standard_normal(1000).astype(np.float32)
    hi, lo = R.split_pair(y)
    assert R.pair_is_canonical(hi, lo)
    assert (np.abs(R.pair_sum(hi, lo).astype(F64) - y) <= R.pair_term(y)).all()
    assert not R.pair_is_canonical(hi, np.zeros_like(lo) + np.float16(0.25))
    parts, bias = R.gelu_inputs(5, 64, 9, seed=2)
    v = R.restate_gelu_sum(parts, bias)
    assert v.min() < -5.9 and v.max() > 5.9 and (np.abs(v) < 1e-3).any()
    tol, ref, worst = R.gelu_tolerance(v)
    assert (np.abs(R.restate_gelu(v).astype(F64) - ref) <= tol).all()
