"""Host-side audit of the skinny decoder GEMM's addressing (gemm_skinny_kernel and its
launchers, csrc/gemm.hip), for every decoder projection shape and the row counts the
decoder step produces (greedy 1..64, beam / best_of rows up to 5 x 64).

It restates the kernel's index arithmetic per (workgroup, wave, lane) and checks:
every global activation / weight load and every split-K slab store stays inside its
buffer; the LDS staging pieces cover each row of the image exactly once and stay
inside the array; and every k the MFMA loop reads from LDS is the k its weight fragment
multiplies (the staged chunk, its XOR swizzle and the short-last-chunk shift agree).
Written for VERDICT r2 item 2 (the r02_ao illegal access): the committed launcher and
kernel pass at every configuration; the one hazard it found (48 hi/lo rows with
64-deep chunks left rows 32-47 unstaged, unreachable from the launchers) is fixed by a
static_assert-backed chunk depth.  If gemm.hip's indexing changes, change this file
with it."""
import numpy as np
import pytest

from open_speech_amd import dims as D


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


def partial_launch(M, N, K, lo):   # launch_gemm_skinny_partial
    ks = skinny_ksplit(N, K)
    gr = 32 if (lo and M > 32) else 64
    m = min(M, gr)
    mt = 1 if m <= 16 else 2 if m <= 32 else 3 if m <= 48 else 4
    return ks, (M + gr - 1) // gr, mt


def kernel_consts(MT, LO):         # gemm_skinny_kernel<MT, ..., LO, PRO_NONE>
    # (<= 16 hi/lo rows: OSW_SKINNY_CK1 = 4 k32 steps per chunk; one operand: 8)
    CK = (4 if MT == 3 else 2) if (LO and MT >= 2) else 4 if LO else 8
    CKK = CK * 32
    CPR = CKK // 8
    RPP = 64 // CPR
    SWM = min(CPR, 16) - 1
    ROWS = MT * 16
    APIECES = ROWS // RPP // 4
    return CK, CKK, CPR, RPP, SWM, ROWS, APIECES


def frag_index(N, K, n, k):
    """launch_frag_pack: element (n, k) of W[N][K] -> its index in the fragment-major copy
    [ceil(N/16)][K/32][64 lanes][8]: lane = (n % 16) + 16 ((k % 32) // 8)."""
    lane = (n % 16) + 16 * ((k % 32) // 8)
    return (((n // 16) * (K // 32) + k // 32) * 64 + lane) * 8 + k % 8


def audit_frag(N, K, nb, k0, st):
    """gemm_skinny_kernel with GemmArgs::Wf: the lane's 16 B at Wf + ((blk K/32 + k0/32) 512
    + 8 lane) + 512 st hold W[nb + lane % 16][k0 + 8 (lane // 16) + 32 st .. +8] for every
    column < N (a block past the padded N is clamped; its columns are discarded)."""
    npad = (N + 15) // 16 * 16
    lane = np.arange(64)
    blk = min(nb, npad - 16) >> 4
    e = ((blk * (K >> 5) + (k0 >> 5)) * 512 + lane * 8) + 512 * st
    assert e.min() >= 0 and (e + 7).max() < npad * K
    n = nb + (lane & 15)
    k = k0 + 8 * (lane >> 4) + 32 * st
    ok = (n < N) & (nb < npad)
    np.testing.assert_array_equal(e[ok], frag_index(N, K, n[ok], k[ok]))


def test_frag_pack_layout():
    """The pack kernel's mapping (one thread per 16-B piece p: lane = p % 64, step =
    (p // 64) % (K/32), block = p // (64 K/32)) is the inverse of frag_index, and a
    wave's k32 fragment is one contiguous 1-KB piece."""
    rng = np.random.default_rng(0)
    for N, K in ((37, 64), (51866 % 4096 + 5, 128), (96, 256)):
        W = rng.integers(0, 60000, size=(N, K)).astype(np.uint16)
        npad = (N + 15) // 16 * 16
        pieces = npad // 16 * (K // 32) * 64
        Wf = np.zeros(pieces * 8, np.uint16)
        p = np.arange(pieces)
        lane, t = p & 63, p >> 6
        st, blk = t % (K // 32), t // (K // 32)
        n = blk * 16 + (lane & 15)
        k = st * 32 + 8 * (lane >> 4)
        for j in range(8):
            Wf[p * 8 + j] = np.where(n < N, W[np.minimum(n, N - 1), k + j], 0)
        nn, kk = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
        np.testing.assert_array_equal(Wf[frag_index(N, K, nn, kk)], W)
        assert Wf.size == npad * K
        pad = (p * 8)[(n >= N)]            # pieces of the padded columns hold zeros
        assert all(not Wf[q:q + 8].any() for q in pad)


def test_frag_logits_addressing():
    """The batch-1 logits GEMM (direct, kc = K, N = the vocabulary) through Wf."""
    for dims in (D.MICRO_TEST, D.TINY_TEST, D.LARGE_V3_TURBO):
        N, K = dims.n_vocab, dims.n_text_state
        for bx in sorted({0, (N + 63) // 64 - 2, (N + 63) // 64 - 1}):
            for wave in range(4):
                for st in (0, K // 32 - 1):
                    audit_frag(N, K, bx * 64 + wave * 16, 0, st)


def audit(M, N, K, lo, R):
    """One launch: activations [R or 2R][lda = K] (hi rows, then lo rows R later, as
    decoder_step lays out xdn / dattn / dh), weights [N][K], slabs [ks][M][N]."""
    ks, nz, MT = partial_launch(M, N, K, lo)
    CK, CKK, CPR, RPP, SWM, ROWS, APIECES = kernel_consts(MT, lo)
    assert APIECES * 4 * RPP == ROWS, (MT, lo)        # the kernel's static_assert
    kc = K // ks
    assert K % ks == 0 and kc % 32 == 0 and (kc // 32) % 4 == 0 or kc == K
    nsteps = kc // 32
    nch = (nsteps + CK - 1) // CK
    lda = K
    a_elems = (2 * R if lo else R) * lda
    lane = np.arange(64)
    li, gq = lane & 15, lane >> 4
    nbx = (N + 63) // 64
    for bx in sorted({0, nbx - 1}):
        for wave in range(4):
            nb = bx * 64 + wave * 16
            n = np.minimum(nb + li, N - 1)
            for by in sorted({0, ks - 1}):
                k0 = by * kc
                # weight fragments: wf[u] = W[n][k0 + 8 gq + 32 st], st <= nsteps - 1
                for c in range(nch):
                    for u in range(CK):
                        st = min(c * CK + u, nsteps - 1)
                        e = n * K + k0 + 8 * gq + 32 * st
                        assert e.min() >= 0 and (e + 7).max() < N * K
                        audit_frag(N, K, nb, k0, st)
                for bz in range(nz):
                    mb = bz * ROWS
                    # staging: LDS[row][(lane % CPR) * 8 ..] <- A[gr][k0 + min(kk + acl, kc - 8) ..]
                    staged = {}
                    for c in range(nch):
                        kk = min(c * CKK, kc - CKK if kc - CKK > 0 else 0)
                        cover = np.zeros((ROWS, CPR), int)
                        for w2 in range(4):
                            for i in range(APIECES):
                                j = i * 4 + w2
                                row = RPP * j + lane // CPR
                                acl = ((lane % CPR) ^ (row & SWM)) * 8
                                gr = np.minimum(mb + row, M - 1)
                                koff = np.minimum(kk + acl, kc - 8)
                                for img in range(2 if lo else 1):
                                    e = img * R * lda + gr * lda + k0 + koff
                                    assert e.min() >= 0 and (e + 7).max() < a_elems
                                lds = RPP * j * CKK + lane * 8
                                assert (lds + 7).max() < ROWS * CKK
                                assert ((lds // CKK) == row).all()
                                cover[row, lane % CPR] += 1
                                for r_, p_, kq in zip(row, lane % CPR, koff):
                                    staged[(c, int(r_), int(p_))] = int(kq)
                        assert (cover == 1).all(), "every (row, 16-B piece) staged exactly once"
                    # consume: row = mt*16 + li reads LDS[row][ch*8 ..], ch = ((u+shift)*4 + gq) ^ (row & SWM)
                    for c in range(nch):
                        steps = min(CK, nsteps - c * CK)
                        shift = (c * CKK - (kc - CKK)) // 32 if (c * CKK > kc - CKK and kc >= CKK) else 0
                        for u in range(steps):
                            for mt in range(MT):
                                row = mt * 16 + li
                                ch = ((u + shift) * 4 + gq) ^ (row & SWM)
                                assert (ch < CPR).all()
                                got = np.array([staged[(c, int(r_), int(p_))] for r_, p_ in zip(row, ch)])
                                want = c * CKK + u * 32 + gq * 8       # the weight fragment's k (minus k0)
                                np.testing.assert_array_equal(got, want)
                    # slab stores: part[(ks*M + m)*N + col] for m < M, col < N
                    col = nb + li
                    for mt in range(MT):
                        for i in range(4):
                            m = mb + mt * 16 + gq * 4 + i
                            ok = (m < M) & (col < N)
                            e = ((by * M + m) * N + col)[ok]
                            if e.size:
                                assert e.min() >= 0 and e.max() < ks * M * N


SHAPES = lambda d: [(3 * d, d), (d, d), (4 * d, d), (d, 4 * d)]   # qkv, o / xq / xo, fc1, fc2


@pytest.mark.parametrize("dims", [D.MICRO_TEST, D.TINY_TEST, D.LARGE_V3_TURBO], ids=["micro", "tiny", "turbo"])
def test_skinny_partial_addressing(dims):
    dd = dims.n_text_state
    rows = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 127, 128, 160, 320]
    for M in rows:
        R = max(M, 64)
        for N, K in SHAPES(dd):
            if M > 64 and N > 1536:
                continue   # > 64 rows and N > 1536: the tiled split-K GEMM, not this kernel (decoder_step)
            audit(M, N, K, True, R)


# every (M, N, K, lo) tests/test_gpu_dec_gemm.py sends through gemm_skinny_kernel without a
# prologue (osw_debug_dec_gemm lays lo M rows after hi: R = M): the partial slabs, the
# one-operand groups of 48 and 64 rows, and the logits route's split and unsplit forms
# (launch_gemm_skinny picks the same MT and split as partial_launch at <= 32 hi/lo rows)
_FORM0_ROWS = (1, 5, 16, 17, 32, 33, 64, 65, 97)
DEC_GEMM_TEST_SHAPES = (
    [(M, N, K, True) for N, K in ((384, 384), (1280, 1280), (384, 1536)) for M in _FORM0_ROWS] +
    [(M, 1280, 5120, True) for M in (1, 2, 3, 4, 5, 8, 33)] +
    [(48, 384, 384, False), (64, 1280, 1280, False)] +
    [(M, 1002, 384, True) for M in (1, 23)] +
    [(M, 32730, 384, lo) for M in (1, 5, 23) for lo in (True, False)] +
    [(1, 51866, 1280, True)] +
    [(M, N, K, True) for N, K in ((1152, 384), (1280, 1280), (384, 1536)) for M in (1, 2, 3, 4, 5, 8)] +
    [(65, 3840, 1280, True), (130, 1536, 1536, True)])


@pytest.mark.parametrize("M,N,K,lo", DEC_GEMM_TEST_SHAPES)
def test_dec_gemm_test_shapes_addressing(M, N, K, lo):
    audit(M, N, K, lo, M)


def test_kernel_constants_cover_rows():
    for MT in (1, 2, 3, 4):
        for lo in (False, True):
            CK, CKK, CPR, RPP, SWM, ROWS, APIECES = kernel_consts(MT, lo)
            assert APIECES * 4 * RPP == ROWS, (MT, lo)


def test_pair_rows_grid_is_a_bijection():
    """pair_rows (launch_gemm_skinny_partial, > 1 row group): the 1-D grid's workgroups
    cover every (column block, K range, row group) exactly once, and the row groups of
    one (column block, K range) share an XCD (workgroup id % 8) with adjacent ids."""
    for dims in (D.MICRO_TEST, D.TINY_TEST, D.LARGE_V3_TURBO):
        for M in (33, 64, 65, 128, 320):
            for N, K in SHAPES(dims.n_text_state):
                ks, nz, MT = partial_launch(M, N, K, True)
                if nz == 1:
                    continue
                gx = (N + 63) // 64
                kc = K // ks
                units = gx * (K // kc)
                seen = {}
                for bid in range(8 * ((units + 7) // 8) * nz):
                    j = bid >> 3
                    u = (j // nz) * 8 + (bid & 7)
                    if u >= units:
                        continue
                    key = (u % gx, u // gx, j % nz)
                    assert key not in seen, key
                    seen[key] = bid
                assert len(seen) == units * nz
                for bx in range(gx):
                    for by in range(ks):
                        ids = [seen[(bx, by, z)] for z in range(nz)]
                        assert len({i % 8 for i in ids}) == 1
                        assert ids == list(range(ids[0], ids[0] + 8 * nz, 8))
