"""References and float32 restatements for int8 decoder weights (STT_COMPUTE_TYPE=int8_float16):
W[n][k] ~ q[n][k] * mult[n], the activations the hi/lo fp16 pairs of dec_gemm_ref.  Plain numpy,
no GPU.  tests/test_gpu_q8.py runs the kernels against these; tests/test_q8_ref_cpu.py shows that
the bound below is met by a faithful evaluation and missed by >= 100x by a kernel that takes its
neighbour's multiplier, drops the multiplier or scales the bias with the product.

What the kernels compute (gemm.hip, GemmArgs::wscale): the float16 MFMA chain of dec_gemm_ref on
fp16(q) (exact: |q| <= 127), per slab the k32 steps in order, hi then lo, into an fp32 accumulator;
the accumulator is multiplied ONCE by mult[n] and rounded to fp32 as it leaves (a C element or a
split-K slab element); a bias is added after that.

Bound (per element of the slab sum, the bias excluded):
    |C - ref| <= G * S + 2^-24 * |ref|
ref = float64 (hi + lo) . (q * mult)^T (q * mult is exact in float64), S = |A| . |q * mult|^T, G
dec_gemm_ref.G.  The accumulation is the float16 path's on fp16(q) with every term scaled by
mult[n] afterwards, so its error keeps the factor G per unit S; 2^-24 |ref| is the one extra
rounding of fp32(acc * mult[n]) (half an ulp of the result).  With ks slabs each slab is rounded
so, at most 2^-24 * sum_k |slab_k| <= 2^-24 * S in all, which the 3/4 of G that is headroom
(9.2e-6 per unit S) carries 150 times over.  test_q8_ref_cpu.test_restatement_meets_the_bound
measures the restatement against it on every GPU case.
"""
import numpy as np

import dec_gemm_ref as R

F32, F16, F64 = np.float32, np.float16, np.float64

# (form, N, K, row counts) of tests/test_gpu_q8.py's kernel-level cases
GPU_CASES = (
    (0, 384, 384, (65, 33, 17, 5, 1)),
    (0, 384, 1536, (65, 33, 17, 5, 1)),
    (2, 1002, 384, (23, 1)),
    (2, 32730, 384, (65, 24, 23, 1)),
    (1, 1536, 1536, (65,)),
)


def case_ksplit(form, M, N, K):
    """Slabs the launcher writes (form 2: slabs summed by splitk_reduce_kernel, 1 when unsplit or on
    the wide kernel)."""
    if form == 1:
        return R.tiled_ksplit(M, N, K)
    if form == 2 and N >= 16384:   # skinny unsplit below 24 rows (N / 64 >= 512 blocks), wide above
        return 1
    return R.skinny_ksplit(N, K)


# --------------------------------------------------------------------------- the int8 fragment layout
def frag_q8_bytes(N, K):
    return (N + 15) // 16 * 16 * K


def frag_q8_offset(n, k, K):
    """Byte offset of q[n][k] in the int8 fragment-major copy (GemmArgs::Wq), from its definition:
    [ceil(N/16)][K/64][64 lanes][16 B]; lane = 16 * ((k % 32) // 8) + n % 16 holds column n % 16 of
    block n // 16; bytes 0-7 are its eight k values of k32 step 2j, bytes 8-15 those of step 2j + 1,
    j = k // 64."""
    blk, col = n // 16, n % 16
    j, step, kin = k // 64, (k % 64) // 32, k % 32
    lane = 16 * (kin // 8) + col
    return ((blk * (K // 64) + j) * 64 + lane) * 16 + 8 * step + kin % 8


def pack_frag_q8(q):
    """The packed buffer (uint8, each byte q + 128; q = 0 past N), by the offset model."""
    N, K = q.shape
    out = np.full(frag_q8_bytes(N, K), 128, np.uint8)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    out[frag_q8_offset(n, k, K)] = (q.astype(np.int16) + 128).astype(np.uint8)
    return out


# --------------------------------------------------------------------------- inputs
def q8_inputs(fam, M, N, K, seed):
    """dec_gemm_ref's activation family with W quantised from the family's W (weights.quantize_rows).
    exact: q = the family's small-integer W itself, multipliers powers of two (2^-(n % 5))."""
    from open_speech_amd import weights
    hi, lo, W = R.FAMILIES[fam](M, N, K, seed)
    if fam == "exact":
        return hi, lo, W.astype(np.int8), (2.0 ** -(np.arange(N) % 5)).astype(F32)
    qm = weights.quantize_rows(W.astype(F32))
    return hi, lo, qm.q, qm.mult


def varied_rows(W, seed):
    """W with even rows scaled by a factor in [1/4, 1/2] and odd rows by one in [1, 4]: the factor
    at least doubles or halves between neighbours, so that a neighbour's multiplier is a different one (the wrong-restatement tests)."""
    rng = np.random.default_rng([seed, 9])
    N = W.shape[0]
    f = np.where(np.arange(N) % 2 == 0, rng.uniform(0.25, 0.5, N), rng.uniform(1.0, 4.0, N))
    return (W.astype(F32) * f[:, None].astype(F32)).astype(F32)


# --------------------------------------------------------------------------- reference / bound
def deq64(q, mult):
    return np.asarray(q, F64) * np.asarray(mult, F64)[:, None]


def q8_ref(hi, lo, q, mult):
    """float64 (hi + lo) . (q * mult)^T, [M][N]."""
    return R.pair_value(hi, lo) @ deq64(q, mult).T


def q8_scale(hi, lo, q, mult):
    return np.abs(R.pair_value(hi, lo)) @ np.abs(deq64(q, mult)).T


def q8_bound(hi, lo, q, mult):
    ref = q8_ref(hi, lo, q, mult)
    return R.G * q8_scale(hi, lo, q, mult) + 2.0 ** -24 * np.abs(ref), ref


# --------------------------------------------------------------------------- float32 restatement
def restate_q8(hi, lo, q, mult, ks, bias=None, wrong=None):
    """k32 steps, hi then lo, then one multiply: dec_gemm_ref.restate_gemm on fp16(q), each slab
    element multiplied by mult[n] in float32 (one rounding), the slabs summed in order, the bias
    added last.  Returns (slabs [ks][M][N], C [M][N]).
    wrong: "neighbour" takes the multiplier of column n + 1 (the last column: of column 0),
    "dropped" multiplies by nothing, "bias" adds the bias before the multiply."""
    m = np.asarray(mult, F32)
    if wrong == "neighbour":
        m = np.roll(m, -1)
    if wrong == "dropped":
        m = np.ones_like(m)
    acc = R.restate_gemm(hi, lo, np.asarray(q).astype(F16), ks)
    b = None if bias is None else np.asarray(bias, F32)
    if wrong == "bias" and b is not None:       # (only an unsplit product can make this mistake)
        assert ks == 1
        slabs = ((acc + b) * m).astype(F32)
        return slabs, slabs[0]
    slabs = (acc * m).astype(F32)
    C = R.sum_slabs(slabs)
    return slabs, C if b is None else (C + b).astype(F32)


def scale_slabs(slabs, mult):
    """What the kernels do to the float16 path's slabs (or product): one float32 multiply by the
    column's multiplier.  With the same MFMA inputs the int8 result equals this bit for bit."""
    return (np.asarray(slabs, F32) * np.asarray(mult, F32)).astype(F32)


# --------------------------------------------------------------------------- power-of-two model weights
def pow2_quantize(w):
    """Per row the largest k <= 14 with |rint(w * 2^k)| <= 127: q int8, mult = 2^-k.  q * 2^-k is then
    a normal fp16 (|q| >= 1 times 2^-14 or more), so fp16(q * mult) is exact and a float16 engine
    loaded with it multiplies by exactly what the int8 engine does; scaling an MFMA operand's column
    by a power of two scales every partial sum exactly, so the two engines agree bit for bit."""
    w = np.asarray(w, F32)
    amax = np.abs(w).max(axis=1)
    k = np.floor(np.log2(127.0 / np.where(amax > 0, amax, 1.0))).astype(np.int64)
    k = np.minimum(k, 14)
    q = np.rint(w * (2.0 ** k)[:, None].astype(F32))
    while (over := np.abs(q).max(axis=1) > 127).any():   # rint pushed a row's maximum to 128
        k = np.where(over, k - 1, k)
        q = np.rint(w * (2.0 ** k)[:, None].astype(F32))
    mult = (2.0 ** -k).astype(F32)
    q = q.astype(np.int8)
    deq = q.astype(F32) * mult[:, None]
    assert np.array_equal(deq.astype(F16).astype(F32), deq)
    return q, mult, deq.astype(F16)
