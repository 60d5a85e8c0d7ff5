"""References, inputs and float32 restatements for the decoder's linear path: the hi/lo
skinny / wide GEMMs (gemm.hip), the residual update + LayerNorm and the GELU reduce
(resln.h).  Plain numpy, no GPU.  tests/test_gpu_dec_gemm.py runs the kernels against these
(osw_debug_dec_gemm / osw_debug_dec_resln / osw_debug_dec_gelu); tests/test_dec_gemm_ref_cpu.py
shows that every bound below is met by a faithful evaluation and missed by >= 20x by a
kernel that drops the lo half, reads lo from another row group, skips a k32 step, loses a
slab, computes a one-pass variance or leaves columns out of the statistics.

References are float64: (hi + lo)·Wᵀ per slab over its K range (how well hi + lo carries the
fp32 activation is the pair's own property, bounded separately by PAIR_REL / PAIR_ABS),
LayerNorm, GELU with the exact erf.

Input families of the GEMM:
  exact      small-integer hi and W, lo small multiples of 2^-6: every partial sum of every
             slab is a multiple of 2^-6 below 2^18, exactly representable in fp32 whatever the
             summation order (assert_exact), so the GPU slabs must EQUAL the reference and a
             dropped, repeated or misplaced k32 step, row, column, K range or row group is an
             integer difference.  Values are independent draws per (row, k) and (column, k).
  same-sign  a = h ± 0.4 ulp(h), h an fp16 value in (0.5, 1), W in [0.5, 1): nothing cancels,
             lo has one sign within a row (+ in even 32-row groups, - in odd ones, so the lo
             rows of neighbouring groups are not interchangeable).  A lost lo half costs
             2.6e-4·S, S = |A|·|W|ᵀ.
  uniform    a ~ U(-1, 1) split into its pair, W ~ U(-1, 1).

Bounds.  None is taken from a kernel's output: each is measured on the float32 restatement
(restate_gemm: per slab the k32 steps in order, hi then lo, fp32 products accumulated one by
one; slabs summed in order) against the float64 reference.
  GEMM       |C - ref| <= G * S per element, G = 4 x the restatement's worst |err| / S over
             GEMM_CASES x {same-sign, uniform} (the 4 allows for the MFMA's internal summation
             order, which nobody has measured).
  LayerNorm  4 x the float32 restatement's worst error of the case + PAIR_REL |y| + PAIR_ABS
  GELU       0.5 |v| 1.5e-7 (erf_fast's stated bound) + 4 x the float32 restatement's worst
             error of the case + the same pair term
The measured constants at the end of the file were printed by
    python -m pytest tests/test_dec_gemm_ref_cpu.py -s -k measured
"""
import numpy as np

F32, F16, F64 = np.float32, np.float16, np.float64

PAIR_REL, PAIR_ABS = 2.0 ** -22, 2.0 ** -25   # |y - (hi + lo)| of an fp16 pair (lo's rounding; lo subnormal)
ERF_FAST_ERR = 1.5e-7                          # common.h erf_fast


# --------------------------------------------------------------------------- launch arithmetic
def skinny_ksplit(N, K):          # gemm.hip skinny_ksplit
    nbn = (N + 63) // 64
    if nbn >= 512:
        return 1
    if K % 256:
        return K // 128
    kc = 256
    while (K // kc) * nbn > 2048 and K % (2 * kc) == 0:
        kc *= 2
    return K // kc


def tiled_ksplit(M, N, K):        # gemm.hip tiled_ksplit
    tiles = ((M + 63) // 64) * ((N + 127) // 128)
    best = 1
    for ks in range(1, K // 64 + 1):
        if K % ks or (K // ks) % 64:
            continue
        if K // ks < 256 and ks > 1:
            break
        if tiles * ks > 1280:
            break
        best = ks
    return best


# --------------------------------------------------------------------------- inputs
def split_pair(a):
    """fp32 -> (hi, lo) fp16 pair: hi = fp16(a), lo = fp16(a - hi) (common.h split_h16)."""
    a = np.asarray(a, F32)
    hi = a.astype(F16)
    return hi, (a - hi.astype(F32)).astype(F16)


def exact_inputs(M, N, K, seed):
    rng = np.random.default_rng([seed, 1])
    hi = rng.integers(-4, 5, (M, K)).astype(F16)
    lo = (rng.integers(-3, 4, (M, K)) * 2.0 ** -6).astype(F16)
    W = rng.integers(-4, 5, (N, K)).astype(F16)
    return hi, lo, W


def assert_exact(hi, lo, W, kc):
    """Every partial sum of a kc-deep slab, in any order, is exactly representable in fp32: all
    terms are multiples of q = 2^-6 and no sum of their magnitudes reaches 2^24 q."""
    q = 2.0 ** -6
    for a in (hi, lo, W):
        if a is None:
            continue
        a = np.asarray(a, F64)
        assert np.array_equal(a, np.round(a / q) * q)
    amax = float(np.abs(np.asarray(hi, F64)).max() + (0.0 if lo is None else np.abs(np.asarray(lo, F64)).max()))
    assert kc * amax * float(np.abs(np.asarray(W, F64)).max()) / q < 2 ** 24


def same_sign_inputs(M, N, K, seed):
    rng = np.random.default_rng([seed, 2])
    h = ((1024 + rng.integers(1, 1024, (M, K))) / 2048.0).astype(F32)   # fp16 values in (0.5, 1): ulp 2^-11
    sign = np.where((np.arange(M) // 32) % 2 == 0, 1.0, -1.0).astype(F32)[:, None]
    hi, lo = split_pair(h + sign * F32(0.4 * 2.0 ** -11))
    assert np.array_equal(hi.astype(F32), h) and (np.sign(lo.astype(F32)) == sign).all()
    W = ((1024 + rng.integers(0, 1024, (N, K))) / 2048.0).astype(F16)
    return hi, lo, W


def uniform_inputs(M, N, K, seed):
    rng = np.random.default_rng([seed, 3])
    hi, lo = split_pair(rng.uniform(-1, 1, (M, K)).astype(F32))
    return hi, lo, rng.uniform(-1, 1, (N, K)).astype(F16)


FAMILIES = {"exact": exact_inputs, "same-sign": same_sign_inputs, "uniform": uniform_inputs}


# --------------------------------------------------------------------------- GEMM reference / restatement
def pair_value(hi, lo):
    a = np.asarray(hi, F64)
    return a if lo is None else a + np.asarray(lo, F64)


def gemm_ref(hi, lo, W, ks=1):
    """float64 slabs [ks][M][N] of (hi + lo)·Wᵀ, slab s over k in [s K/ks, (s+1) K/ks)."""
    a, w = pair_value(hi, lo), np.asarray(W, F64)
    K = a.shape[1]
    kc = K // ks
    return np.stack([a[:, s * kc:(s + 1) * kc] @ w[:, s * kc:(s + 1) * kc].T for s in range(ks)])


def gemm_ref_exact(hi, lo, W, ks=1):
    """gemm_ref for the exact family through a float32 product (cheap at vocabulary width): with
    every partial sum representable, any summation order in fp32 gives the exact slabs."""
    a = np.asarray(hi, F32) if lo is None else np.asarray(hi, F32) + np.asarray(lo, F32)
    w = np.asarray(W, F32)
    kc = a.shape[1] // ks
    return np.stack([a[:, s * kc:(s + 1) * kc] @ w[:, s * kc:(s + 1) * kc].T for s in range(ks)])


def gemm_scale(hi, lo, W):
    """S = |A|·|W|ᵀ (float64): what every rounding error of the product is proportional to."""
    return np.abs(pair_value(hi, lo)) @ np.abs(np.asarray(W, F64)).T


def restate_gemm(hi, lo, W, ks, use_lo=True, lo_row=None, skip=()):
    """The accumulation in float32: per slab the k32 steps in order, each step's 32 hi products
    added one by one, then its 32 lo products (the kernels issue one MFMA per operand half and
    step into the same accumulator).  fp16 x fp16 products are exact in fp32.  Returns [ks][M][N].
    Mutations for the sensitivity tests: use_lo False drops the lo half; lo_row maps row r to the
    row whose lo half it (wrongly) reads; skip lists (slab, k32 step) pairs left out."""
    h, w = np.asarray(hi, F32), np.asarray(W, F32)
    l = None if (lo is None or not use_lo) else np.asarray(lo, F32)
    if l is not None and lo_row is not None:
        l = l[np.asarray(lo_row)]
    M, K = h.shape
    kc = K // ks
    out = np.zeros((ks, M, w.shape[0]), F32)
    for s in range(ks):
        acc = out[s]
        for st in range(kc // 32):
            if (s, st) in skip:
                continue
            for a in (h, l):
                if a is None:
                    continue
                for k in range(s * kc + st * 32, s * kc + st * 32 + 32):
                    acc += a[:, k, None] * w[None, :, k]
    return out


def sum_slabs(slabs):
    """Σ_k slabs[k] in slab order, in the slabs' own precision (splitk_reduce_kernel's order)."""
    s = np.zeros_like(slabs[0])
    for p in slabs:
        s = s + p
    return s


# (K, ksplit) of every GEMM the GPU tests launch: kc 128 (K % 256 != 0), 256, and the unsplit
# vocabulary projections (kc = K = 384, 1280)
GEMM_CASES = ((384, 3), (1280, 5), (1536, 6), (5120, 20), (384, 1), (1280, 1))


def measure_gemm(M=8, N=64):
    """Worst |restatement - float64| / S per (family, K, ks) at M x N outputs."""
    rows = []
    for fam in ("same-sign", "uniform"):
        for K, ks in GEMM_CASES:
            hi, lo, W = FAMILIES[fam](M, N, K, seed=K + ks)
            err = np.abs(sum_slabs(restate_gemm(hi, lo, W, ks)).astype(F64) - gemm_ref(hi, lo, W).sum(0))
            rows.append((fam, K, ks, float((err / gemm_scale(hi, lo, W)).max())))
    return rows


# --------------------------------------------------------------------------- residual + LayerNorm
def restate_resid(x, bias, slabs):
    """x' = (x + bias) + Σ_k slabs[k], the sum from zero in slab order (resln_rows): float32,
    bit-exact by construction (the kernel runs under fp contract(off))."""
    a = np.asarray(x, F32)
    if bias is not None:
        a = a + np.asarray(bias, F32)
    return a + sum_slabs(np.asarray(slabs, F32))


def restate_embed(tok_emb, pos_emb, tok, pos, pos_row):
    """The embedding entry: x' = fp32(tok_emb[clamp(tok, 0, V-1)]) + pos_emb[min(pos, ctx-1)];
    row r's position is pos[r] with pos_row, else pos[0]."""
    te, pe = np.asarray(tok_emb, F16), np.asarray(pos_emb, F32)
    tk = np.clip(np.asarray(tok), 0, te.shape[0] - 1)
    p = np.atleast_1d(np.asarray(pos))
    p = np.minimum(p if pos_row else np.repeat(p[:1], len(tk)), pe.shape[0] - 1)
    return te[tk].astype(F32) + pe[p]


def ln_ref(xp, gain, shift):
    """float64 LayerNorm (eps 1e-5) of the fp32 rows xp."""
    x = np.asarray(xp, F64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * np.asarray(gain, F64) + np.asarray(shift, F64)


def _thread_columns(D):
    """resln_rows' layout: thread t of 256 owns columns 4t..4t+3 and 1024 + t; -> [256][5] column
    ids, -1 where the thread has none."""
    t = np.arange(256)
    c = np.full((256, 5), -1)
    for i in range(4):
        c[:, i] = np.where(4 * t < D, 4 * t + i, -1)
    c[:, 4] = np.where(1024 + t < D, 1024 + t, -1)
    return c


def _block_sum(v):
    """[rows][256] per-thread values -> the workgroup's sum as resln_rows forms it: wave_sum's
    xor butterfly (32, 16, 8, 4, 2, 1) within each 64-lane wave, the 4 wave partials in order."""
    s = v.reshape(v.shape[0], 4, 64).astype(F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    w = s[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def restate_ln(xp, gain, shift, one_pass=False, drop_tail=False):
    """LayerNorm in float32 in resln_rows' order (two-pass variance, the thread's 5 columns in
    order, then _block_sum).  Mutations: one_pass computes E[x^2] - mean^2; drop_tail leaves the
    columns 1024 + t out of both statistics."""
    xp = np.asarray(xp, F32)
    rows, D = xp.shape
    cols = _thread_columns(D)
    has = cols >= 0
    if drop_tail:
        has = has & (np.arange(5) < 4)
    v = np.where(has, xp[:, np.maximum(cols, 0)], F32(0)).astype(F32)   # [rows][256][5]
    s = np.zeros((rows, 256), F32)
    for i in range(5):
        s = s + v[:, :, i]
    mean = (_block_sum(s) / F32(D)).astype(F32)[:, None]
    q = np.zeros((rows, 256), F32)
    for i in range(5):
        d = v[:, :, i] - mean
        t = (d if not one_pass else v[:, :, i]).astype(F64)
        q = np.where(has[:, i], (t * t + q.astype(F64)).astype(F32), q)   # fmaf(d, d, q)
    var = (_block_sum(q) / F32(D)).astype(F32)
    if one_pass:
        var = var - (mean[:, 0] * mean[:, 0]).astype(F32)
    rstd = (F32(1) / np.sqrt(var + F32(1e-5), dtype=F32)).astype(F32)[:, None]
    g, b = np.asarray(gain, F32), np.asarray(shift, F32)
    n = ((xp - mean) * rstd).astype(F32)
    return (n.astype(F64) * g.astype(F64) + b.astype(F64)).astype(F32)    # fmaf(n, g, b)


def ln_inputs(kind, rows, D, ks, seed):
    """(x, slabs [ks][rows][D], bias, gain, shift).  plain: unit-scale everything; large-mean:
    x' ~ 100 + 0.1 N(0, 1) (the mean is 1000 standard deviations: a one-pass variance loses it);
    dominant: one column of x is 1000, the rest unit scale."""
    rng = np.random.default_rng([seed, rows, D, ks])
    x = rng.standard_normal((rows, D)).astype(F32)
    slabs = (rng.standard_normal((ks, rows, D)) / np.sqrt(ks)).astype(F32)
    bias = rng.standard_normal(D).astype(F32)
    if kind == "large-mean":
        x, slabs, bias = (100 + x * 0.05).astype(F32), (slabs * 0.05).astype(F32), (bias * 0.05).astype(F32)
    elif kind == "dominant":
        x[:, (7 * D) // 11] = 1000.0
    gain = (1 + 0.2 * rng.standard_normal(D)).astype(F32)
    shift = (0.2 * rng.standard_normal(D)).astype(F32)
    return x, slabs, bias, gain, shift


def pair_sum(hi, lo):
    """The fp32 value hi + lo as the GEMM's accumulator forms it (hi x 1, then + lo x 1)."""
    return np.asarray(hi, F32) + np.asarray(lo, F32)


def pair_is_canonical(hi, lo):
    """What `lo == fp16(y - hi)` can assert from the pair alone: hi is a nearest fp16 value to
    hi + lo, i.e. lo lies within half a step of hi on its own side (a tie included: y just short
    of one rounds its lo half up to it).  A lo half that is stale, belongs to another element or
    was scaled fails; fp16(y - hi) == lo is then automatic, hi + lo being exact in float64."""
    h = np.asarray(hi, F16)
    l = np.asarray(lo, F64)
    up = (np.nextafter(h, F16(np.inf)).astype(F64) - h.astype(F64)) / 2
    dn = (h.astype(F64) - np.nextafter(h, F16(-np.inf)).astype(F64)) / 2
    return bool(np.isfinite(l).all() and ((l <= up) & (-l <= dn)).all())


def pair_term(y):
    return PAIR_REL * np.abs(y) + PAIR_ABS


def ln_tolerance(xp, gain, shift):
    """Per element: 4 x the float32 restatement's worst error on these rows + the pair term."""
    ref = ln_ref(xp, gain, shift)
    worst = float(np.abs(restate_ln(xp, gain, shift).astype(F64) - ref).max())
    return 4 * worst + pair_term(ref), ref, worst


# --------------------------------------------------------------------------- GELU reduce
def restate_gelu_sum(slabs, bias):
    """gelu_reduce_one's argument: v = bias, then += slabs[k] in slab order; float32, bit-exact."""
    slabs = np.asarray(slabs, F32)
    v = np.broadcast_to(np.asarray(bias, F32), slabs.shape[1:]).copy()
    for p in slabs:
        v = v + p
    return v


def _erf(x):
    from scipy.special import erf
    return erf(x)


def gelu_ref(v):
    v = np.asarray(v, F64)
    return 0.5 * v * (1.0 + _erf(v / np.sqrt(2.0)))


def restate_gelu(v):
    """0.5 v (1 + erf(v / sqrt 2)) with every operation rounded to float32 and a correctly
    rounded erf (gelu_erf's operations; erf_fast's own error is the bound's first term)."""
    v = np.asarray(v, F32)
    e = _erf((v * F32(0.70710678118654752)).astype(F64)).astype(F32)
    return ((F32(0.5) * v) * (F32(1) + e)).astype(F32)


def gelu_tolerance(v):
    ref = gelu_ref(v)
    worst = float(np.abs(restate_gelu(v).astype(F64) - ref).max())
    return 0.5 * np.abs(np.asarray(v, F64)) * ERF_FAST_ERR + 4 * worst + pair_term(ref), ref, worst


def gelu_inputs(M, K4, ks, seed):
    """Slabs and bias whose sums v span [-6, 6]: a ramp over the columns with ±0, ±6 and the
    tails' neighbourhood pinned, split into ks random parts."""
    rng = np.random.default_rng([seed, M, K4, ks])
    v = rng.uniform(-6, 6, (M, K4))
    pins = np.array([0.0, -0.0, 6.0, -6.0, 5.5, -5.5, 1e-4, -1e-4, 0.5, -0.5, 3.0, -3.0])
    v[:, :len(pins)] = pins
    bias = rng.uniform(-0.5, 0.5, K4).astype(F32)
    parts = rng.standard_normal((ks, M, K4))
    parts = parts - parts.mean(0) + (v - bias) / ks
    return parts.astype(F32), bias


# --------------------------------------------------------------------------- the GPU tests' cases
LN_WIDTHS = (256, 384, 1024, 1280)
LN_KS = (1, 3, 8, 9, 20)
LN_ROWS = (1, 3)
LN_KINDS = ("plain", "large-mean", "dominant")
GELU_KS = (1, 3, 5, 9)
GELU_ROWS = (1, 5)
GELU_K4 = 1536


def ln_case(kind, rows, D, ks, with_bias):
    """-> (x, slabs, bias or None, gain, shift, x' restated)."""
    x, slabs, bias, gain, shift = ln_inputs(kind, rows, D, ks, seed=11)
    b = bias if with_bias else None
    return x, slabs, b, gain, shift, restate_resid(x, b, slabs)


def measure_ln():
    """Worst float32-restatement LayerNorm error per input kind over the GPU tests' cases."""
    worst = {}
    for kind in LN_KINDS:
        for D in LN_WIDTHS:
            for ks in LN_KS:
                for rows in LN_ROWS:
                    for wb in (True, False):
                        _, _, _, g, b, xp = ln_case(kind, rows, D, ks, wb)
                        worst[kind] = max(worst.get(kind, 0.0), ln_tolerance(xp, g, b)[2])
    return worst


def measure_gelu():
    worst = 0.0
    for ks in GELU_KS:
        for M in GELU_ROWS:
            s, b = gelu_inputs(M, GELU_K4, ks, seed=5)
            worst = max(worst, gelu_tolerance(restate_gelu_sum(s, b))[2])
    return worst


# --------------------------------------------------------------------------- measured constants
# python -m pytest tests/test_dec_gemm_ref_cpu.py -s -k measured
G_MEASURED = 3.061e-6   # worst |restatement - float64| / S over GEMM_CASES x {same-sign, uniform}
                        # (same-sign, K = 1280 unsplit; split at kc 256: 5.2e-7; uniform: 1.7e-7)
G = 4 * G_MEASURED      # the GEMM bound's factor
# worst float32-restatement errors over the GPU tests' cases (measure_ln / measure_gelu); the tests
# take 4 x the worst of their own case, these are the record
LN_RESTATE_WORST = {"plain": 7.52e-7, "large-mean": 2.75e-4, "dominant": 6.96e-6}
GELU_RESTATE_WORST = 4.45e-7
