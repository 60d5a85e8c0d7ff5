"""The decoder's linear path kernel by kernel, one production launcher per call on host data
(osw_debug_dec_gemm / osw_debug_dec_resln / osw_debug_dec_gelu), against the float64
references of tests/dec_gemm_ref.py: gemm_skinny_kernel with hi/lo operands, fragment-major
weights, split-K slabs, 32-row groups on the remapped grid and the fused PRO_RESLN / PRO_GELU
prologues; the logits route (split + splitk_reduce_kernel, unsplit, gemm_wide_kernel<true, 256>);
the tiled split-K GEMM; dec_resid_ln_kernel and dec_reduce_gelu_kernel.

The exact input family must come back bit for bit; the same-sign and uniform families within
G·S (dec_gemm_ref.G, measured on the float32 restatement, never on a kernel).  The bounds are
derived in dec_gemm_ref.py; tests/test_dec_gemm_ref_cpu.py shows what they catch.  Every test
prints its worst |err| / bound.

Measured on an MI355X (DESIGN.md §2 has the record; every figure is printed by its test): GEMM
worst |err| / S 1.40e-6 (same-sign, vocabulary projection with K = 1280 unsplit; split-K slabs
3.3e-7; uniform 1.7e-7) against G = 1.22e-5; LayerNorm worst |y - ref| 1.2e-6 plain, 1.7e-4
large-mean, 6.4e-6 dominant, at most 0.92 of the case's bound; GELU 9.0e-7, 0.31 of its bound.
"""
import functools

import numpy as np
import pytest

import dec_gemm_ref as R
from open_speech_amd import dims as D
from open_speech_amd.engine import WhisperEngine

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
MMAX = 97


@pytest.fixture(scope="module")
def eng():
    d = D.WhisperDims(n_mels=80, n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128,
                      n_text_head=2, n_text_layer=1)
    e = WhisperEngine(d, device=0, max_batch=1)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=4)
def gemm_case(fam, M, N, K, with_lo=True):
    """Inputs of one (family, shape) with the float64 reference of the whole product and S; rows
    [:m] serve every smaller row count (row r's inputs do not depend on M)."""
    hi, lo, W = R.FAMILIES[fam](M, N, K, seed=N + K)
    if not with_lo:
        lo = None
    if fam == "exact":
        R.assert_exact(hi, lo, W, K)   # the deepest slab is the whole K
        ref, S = None, None            # (check_product takes gemm_ref_exact of the rows it got)
    else:
        ref = R.pair_value(hi, lo) @ W.astype(F64).T
        S = np.abs(R.pair_value(hi, lo)).astype(F32) @ np.abs(W.astype(F32)).T
    return hi, lo, W, ref, S


def check_product(C, fam, hi, lo, W, ref, S, ks, what):
    """C: slabs [ks][M][N] (or the product [M][N] with ks None) of rows [:M] of the case."""
    slabs = C if ks is not None else C[None]
    M = slabs.shape[1]
    assert np.isfinite(slabs).all(), f"{what}: an element was not written"
    if fam == "exact":
        want = R.gemm_ref_exact(hi[:M], None if lo is None else lo[:M], W, slabs.shape[0])
        bad = np.argwhere(slabs != want)
        assert bad.size == 0, (what, "first differences (slab, row, column):", bad[:8].tolist(),
                               slabs[tuple(bad[0])], want[tuple(bad[0])])
        return 0.0
    total = R.sum_slabs(slabs).astype(F64)
    r = float((np.abs(total - ref[:M]) / (R.G * S[:M].astype(F64))).max())
    print(f"{what}: worst |err| / (G S) = {r:.3f}  (|err|/S = {r * R.G:.3e}, G = {R.G:.3e})")
    assert r <= 1, (what, r)
    return r * R.G


# --------------------------------------------------------------------------- partial slabs (form 0)
FORM0_ROWS = (97, 65, 64, 33, 32, 17, 16, 5, 1)


@pytest.mark.parametrize("fam", ["exact", "same-sign", "uniform"])
@pytest.mark.parametrize("N,K,rows", [(384, 384, FORM0_ROWS), (1280, 1280, FORM0_ROWS), (384, 1536, FORM0_ROWS),
                                      (1280, 5120, (33, 1))], ids=["384x384", "1280x1280", "384x1536", "1280x5120"])
def test_skinny_partial_slabs(eng, fam, N, K, rows):
    """launch_gemm_skinny_partial with hi/lo rows: MT 1 and 2, one group, two, three and four
    32-row groups with a 1-row last group (pair_rows grid), kc 128 (K = 384, ks 3) and 256 (ks 5,
    6, 20), the weight preload.  Per row count: the plain and the fragment-major weights give the
    same bits; the exact family equals the reference slab by slab; the others' slab sums are
    within G·S; and a row's slabs are the same bits at every row count.
    Measured (MI355X): worst |err| / S 3.1e-7 same-sign, 4.9e-8 uniform (G = 1.22e-5)."""
    hi, lo, W, ref, S = gemm_case(fam, MMAX, N, K)
    ks = R.skinny_ksplit(N, K)
    first = None
    for M in rows:
        what = f"skinny partial {fam} M {M} N {N} K {K}"
        s = eng.debug_dec_gemm(0, hi[:M], lo[:M], W, use_wf=False)
        sf = eng.debug_dec_gemm(0, hi[:M], lo[:M], W, use_wf=True)
        assert s.shape == (ks, M, N), what
        assert same_bits(s, sf), f"{what}: fragment-major weights change the result"
        check_product(s, fam, hi, lo, W, ref, S, ks, what)
        if first is None:
            first = s
        else:
            assert same_bits(s, np.ascontiguousarray(first[:, :M])), f"{what}: a row's bits depend on the row count"


@pytest.mark.parametrize("M,N,K", [(48, 384, 384), (64, 1280, 1280)])
def test_skinny_partial_one_operand(eng, M, N, K):
    """MT 3 and MT 4 (48 and 64 rows in one group), which hi/lo rows never reach: one fp16 operand,
    256-deep chunks (kc 128 at K = 384: the chunk is deeper than the K range, its tail clamped)."""
    for fam in ("exact", "uniform"):
        hi, _, W, ref, S = gemm_case(fam, M, N, K, False)
        for wf in (False, True):
            s = eng.debug_dec_gemm(0, hi, None, W, use_wf=wf)
            check_product(s, fam, hi, None, W, ref, S, R.skinny_ksplit(N, K), f"one operand {fam} M {M} N {N} K {K} wf {wf}")


# --------------------------------------------------------------------------- logits (form 2)
@pytest.mark.parametrize("fam", ["exact", "same-sign", "uniform"])
@pytest.mark.parametrize("N,K,rows", [(1002, 384, (23, 1)), (32730, 384, (65, 64, 24, 23, 5, 1)),
                                      (51866, 1280, (64, 1))], ids=["1002x384", "32730x384", "51866x1280"])
def test_logits_route(eng, fam, N, K, rows):
    """The vocabulary projection as decoder_step launches it, N no multiple of 16: (1002, 384)
    split-K (kc 128) + splitk_reduce_kernel; (32730, 384) and (51866, 1280) unsplit through the
    skinny kernel below 24 rows (kc = K in 128- or 64-deep chunks) and through
    gemm_wide_kernel<true, 256> from 24 rows on (65 rows: two row tiles).  The result buffer's
    guard band (debug_dec_gemm raises if it changed) shows that no column past N was written.
    Measured (MI355X): worst |err| / S same-sign 2.8e-7 / 6.9e-7 / 1.40e-6 at the three widths
    (the unsplit K = 1280 is the deepest fp32 accumulation of the path), uniform <= 1.7e-7."""
    Mmax = max(rows)
    hi, lo, W, ref, S = gemm_case(fam, Mmax, N, K)
    first = None
    for M in rows:
        what = f"logits {fam} M {M} N {N} K {K}"
        c = eng.debug_dec_gemm(2, hi[:M], lo[:M], W, use_wf=False)
        assert c.shape == (M, N)
        check_product(c, fam, hi, lo, W, ref, S, None, what)
        if M < 24:   # the skinny kernel reads the fragment-major copy; the wide kernel never does
            assert same_bits(c, eng.debug_dec_gemm(2, hi[:M], lo[:M], W, use_wf=True)), what


@pytest.mark.parametrize("M", [1, 5, 23])
def test_logits_one_operand_short_last_chunk(eng, M):
    """(32730, 384) unsplit with one fp16 operand: 256-deep chunks, so the second chunk is short
    (4 of 8 k32 steps), staged from kc - 256 and read with the image shift.  (With hi/lo rows the
    chunks are 128 or 64 deep and 384 has no short chunk.)"""
    N, K = 32730, 384
    for fam in ("exact", "uniform"):
        hi, _, W, ref, S = gemm_case(fam, 23, N, K, False)
        for wf in (False, True):
            c = eng.debug_dec_gemm(2, hi[:M], None, W, use_wf=wf)
            check_product(c, fam, hi, None, W, ref, S, None, f"logits one operand {fam} M {M} wf {wf}")


# --------------------------------------------------------------------------- tiled split-K (form 1)
@pytest.mark.parametrize("fam", ["exact", "same-sign", "uniform"])
@pytest.mark.parametrize("M,N,K", [(65, 3840, 1280), (130, 1536, 1536)])
def test_tiled_partial_slabs(eng, fam, M, N, K):
    """launch_gemm_tiled_partial (gemm_wide_kernel<true> with split-K slabs, the opt-in route of
    beam rows): same split depth and MFMA order as the skinny row groups, so also the same bits."""
    hi, lo, W, ref, S = gemm_case(fam, M, N, K)
    ks = R.tiled_ksplit(M, N, K)
    s = eng.debug_dec_gemm(1, hi, lo, W)
    assert s.shape == (ks, M, N)
    check_product(s, fam, hi, lo, W, ref, S, ks, f"tiled {fam} M {M} N {N} K {K}")
    if ks == R.skinny_ksplit(N, K):
        assert same_bits(s, eng.debug_dec_gemm(0, hi, lo, W, use_wf=True)), "tiled and skinny slabs differ"


# --------------------------------------------------------------------------- residual + LayerNorm
def check_pair(hi, lo, tol, ref, what):
    assert R.pair_is_canonical(hi, lo), f"{what}: lo != fp16(y - hi)"
    err = np.abs(R.pair_sum(hi, lo).astype(F64) - ref)
    return float((err / tol).max()), float(err.max())


@pytest.mark.parametrize("kind", R.LN_KINDS)
@pytest.mark.parametrize("Dm", R.LN_WIDTHS)
def test_resid_ln_standalone(eng, Dm, kind):
    """dec_resid_ln_kernel over ks in {1, 3, 8, 9, 20} slabs, 1 and 3 rows, with and without the
    bias: x' equals the float32 restatement bit for bit, the pair is canonical, and its sum is
    within 4 x the restatement's own error + the pair term of the float64 LayerNorm of x'.
    Measured (MI355X) worst |y - ref|: plain 1.2e-6, large-mean 1.7e-4, dominant 6.4e-6; worst
    |err| / bound 0.45, 0.25, 0.92 (the restatement's own worst errors over these cases, which the
    bounds quadruple: 7.5e-7, 2.7e-4, 7.0e-6)."""
    worst = (0.0, 0.0)
    for ks in R.LN_KS:
        for rows in R.LN_ROWS:
            for wb in (True, False):
                x, slabs, b, g, sh, xp = R.ln_case(kind, rows, Dm, ks, wb)
                what = f"resid+LN {kind} D {Dm} ks {ks} rows {rows} bias {wb}"
                xo, hi, lo = eng.debug_dec_resln(x, g, sh, slabs=slabs, bias=b)
                assert same_bits(xo, xp), f"{what}: x' differs from its restatement"
                tol, ref, _ = R.ln_tolerance(xp, g, sh)
                worst = max(worst, check_pair(hi, lo, tol, ref, what))
    print(f"resid+LN {kind} D {Dm}: worst |err| / bound = {worst[0]:.3f}, worst |err| = {worst[1]:.3e}")
    assert worst[0] <= 1


@pytest.mark.parametrize("Dm", [256, 1280])
def test_resid_ln_embedding_entry(eng, Dm):
    """The embedding entry: ids -1 and V are clamped to 0 and V - 1, positions >= ctx to ctx - 1;
    pos_row 0 takes pos[0] for every row, pos_row 1 the row's own."""
    V, ctx, rows = 50, 12, 5
    rng = np.random.default_rng(Dm)
    te = rng.standard_normal((V, Dm)).astype(np.float16)
    pe = rng.standard_normal((ctx, Dm)).astype(F32)
    g = (1 + 0.2 * rng.standard_normal(Dm)).astype(F32)
    sh = (0.2 * rng.standard_normal(Dm)).astype(F32)
    tok = np.array([-1, V, 7, 0, V - 1], np.int32)
    x = np.zeros((rows, Dm), F32)
    for pos_row, pos in ((0, [3]), (0, [ctx + 5]), (1, [0, ctx, 5, ctx - 1, 1000])):
        xp = R.restate_embed(te, pe, tok, pos, pos_row)
        what = f"embedding D {Dm} pos_row {pos_row} pos {pos}"
        xo, hi, lo = eng.debug_dec_resln(x, g, sh, embed=(te, pe, tok, pos, pos_row))
        assert same_bits(xo, xp), what
        tol, ref, _ = R.ln_tolerance(xp, g, sh)
        r, e = check_pair(hi, lo, tol, ref, what)
        print(f"{what}: worst |err| / bound = {r:.3f}")
        assert r <= 1


# --------------------------------------------------------------------------- GELU reduce
def test_reduce_gelu_standalone(eng):
    """dec_reduce_gelu_kernel over ks in {1, 3, 5, 9} slabs, 1 and 5 rows, v spanning [-6, 6] with
    ±0 and the tails: within 0.5 |v| 1.5e-7 + 4 x the float32 restatement's error + the pair term
    of the float64 GELU of the bit-exact sum v.
    Measured (MI355X): worst |err| 9.0e-7, worst |err| / bound 0.31."""
    worst = (0.0, 0.0)
    for ks in R.GELU_KS:
        for M in R.GELU_ROWS:
            s, b = R.gelu_inputs(M, R.GELU_K4, ks, seed=5)
            v = R.restate_gelu_sum(s, b)
            hi, lo = eng.debug_dec_gelu(s, b)
            tol, ref, _ = R.gelu_tolerance(v)
            worst = max(worst, check_pair(hi, lo, tol, ref, f"GELU reduce ks {ks} M {M}"))
    print(f"GELU reduce: worst |err| / bound = {worst[0]:.3f}, worst |err| = {worst[1]:.3e}")
    assert worst[0] <= 1


# --------------------------------------------------------------------------- fused prologues
@pytest.mark.parametrize("ks", [1, 8, 9, 20, 25])
@pytest.mark.parametrize("Dm", [384, 1280])
def test_pro_resln_identity(eng, Dm, ks):
    """PRO_RESLN with W the fp16 identity: the slab sum (and the direct output) is exactly
    hi + lo of the prologue's LayerNorm, which must be the standalone kernel's pair bit for bit.
    ks 8 / 9 straddle the 8-slab batch, 20 is fc2's count, 25 is past one 24-slab batch.  x' goes to
    the second buffer (equal to the restatement: written, once, whole) and x stays untouched."""
    x, slabs, b, g, sh, xp = R.ln_case("plain", 1, Dm, ks, True)
    _, hi, lo = eng.debug_dec_resln(x, g, sh, slabs=slabs, bias=b)
    want = R.pair_sum(hi, lo)
    eye = np.eye(Dm, dtype=np.float16)
    for direct in (False, True):
        for wf in (False, True):
            what = f"PRO_RESLN identity D {Dm} ks {ks} direct {direct} wf {wf}"
            xo, out, x_after = eng.debug_dec_resln(x, g, sh, slabs=slabs, bias=b, W=eye, direct=direct, use_wf=wf)
            assert same_bits(xo, xp), f"{what}: x'"
            assert same_bits(x_after, x), f"{what}: the residual input buffer was written"
            assert np.isfinite(out).all(), what
            got = out if direct else R.sum_slabs(out)
            assert same_bits(got, want), (what, np.argwhere(got != want)[:8].tolist())


@pytest.mark.parametrize("Dm,N", [(384, 1152), (1280, 1280)])
def test_pro_resln_equals_standalone_then_gemm(eng, Dm, N):
    """PRO_RESLN slabs with a random W are the bits of dec_resid_ln_kernel followed by
    launch_gemm_skinny_partial on its pair; the embedding entry (layer 0's qkv) included."""
    rng = np.random.default_rng(Dm + N)
    W = rng.uniform(-1, 1, (N, Dm)).astype(np.float16)
    for ks in (3, 20):
        x, slabs, b, g, sh, xp = R.ln_case("plain", 1, Dm, ks, True)
        _, hi, lo = eng.debug_dec_resln(x, g, sh, slabs=slabs, bias=b)
        want = eng.debug_dec_gemm(0, hi, lo, W, use_wf=True)
        for wf in (False, True):
            xo, out, _ = eng.debug_dec_resln(x, g, sh, slabs=slabs, bias=b, W=W, use_wf=wf)
            assert same_bits(xo, xp) and same_bits(out, want), f"PRO_RESLN D {Dm} N {N} ks {ks} wf {wf}"
    te = rng.standard_normal((20, Dm)).astype(np.float16)
    pe = rng.standard_normal((8, Dm)).astype(F32)
    emb = (te, pe, np.array([20], np.int32), [9], 0)
    x, _, _, g, sh, _ = R.ln_case("plain", 1, Dm, 1, False)
    xs, hi, lo = eng.debug_dec_resln(x, g, sh, embed=emb)
    xo, out, _ = eng.debug_dec_resln(x, g, sh, embed=emb, W=W, use_wf=True)
    assert same_bits(xo, xs) and same_bits(xo, R.restate_embed(te, pe, [20], [9], 0))
    assert same_bits(out, eng.debug_dec_gemm(0, hi, lo, W, use_wf=True))


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("K4,N", [(1536, 384), (5120, 1280)])
def test_pro_gelu_equals_standalone_then_gemm(eng, K4, N, M):
    """PRO_GELU (the 1 / 2 / 4 / 8-row forms, rows past M repeating row M - 1) gives the bits of
    dec_reduce_gelu_kernel followed by launch_gemm_skinny_partial on its pair."""
    rng = np.random.default_rng(K4 + M)
    W = rng.uniform(-1, 1, (N, K4)).astype(np.float16)
    ks = R.skinny_ksplit(K4, N)   # fc1's split at this width
    s, b = R.gelu_inputs(M, K4, ks, seed=M)
    hi, lo = eng.debug_dec_gelu(s, b)
    want = eng.debug_dec_gemm(0, hi, lo, W, use_wf=True)
    for wf in (False, True):
        out = eng.debug_dec_gelu(s, b, W=W, use_wf=wf)
        assert same_bits(out, want), f"PRO_GELU M {M} K {K4} N {N} wf {wf}"


def test_preconditions_are_errors(eng):
    """A shape a launcher or kernel does not serve is refused before any launch."""
    h = np.zeros((65, 192), np.float16)
    w = np.zeros((64, 192), np.float16)
    with pytest.raises(Exception):
        eng.debug_dec_gemm(0, h[:1], h[:1], w)                 # K % 128
    h = np.zeros((65, 256), np.float16)
    w = np.zeros((64, 256), np.float16)
    with pytest.raises(Exception):
        eng.debug_dec_gemm(0, h, None, w)                      # > 64 rows without lo
    with pytest.raises(Exception):
        eng.debug_dec_gemm(1, h, h, np.zeros((63, 256), np.float16))   # odd N on the wide kernel
    x = np.zeros((2, 256), F32)
    g = np.ones(256, F32)
    with pytest.raises(Exception):
        eng.debug_dec_resln(x, g, g, slabs=x[None], W=w)       # PRO_RESLN serves one row
    with pytest.raises(Exception):
        eng.debug_dec_resln(np.zeros((1, 1284), F32), np.ones(1284, F32), np.ones(1284, F32),
                            slabs=np.zeros((1, 1, 1284), F32))  # D > 1280
    with pytest.raises(Exception):
        eng.debug_dec_resln(np.zeros((1, 130), F32), np.ones(130, F32), np.ones(130, F32),
                            slabs=np.zeros((1, 1, 130), F32))   # D % 4
    s9 = np.zeros((1, 9, 256), F32)
    with pytest.raises(Exception):
        eng.debug_dec_gelu(s9, np.zeros(256, F32), W=w)        # PRO_GELU serves <= 8 rows
    with pytest.raises(Exception):
        eng.debug_dec_gelu(np.zeros((1, 1, 1024), F32), np.zeros(1024, F32),
                           W=np.zeros((32768, 1024), np.float16))   # unsplit: kc 1024 > GELU_KC
