"""The encoder's tiled GEMM family and LayerNorm kernel by kernel, one launch per call on host data
(osw_debug_enc_gemm / osw_debug_enc_layernorm), against the float64 references, addressing models
and bounds of tests/enc_gemm_ref.py: all seven tile kernels with each of the six epilogues, with and
without a bias, over grouped and overlapping A rows (the conv stem's implicit GEMMs), grouped C rows at
an offset (conv1's zero border rows), the positional table, the in-place residual and the head-major
scatter with slot redirection; then the production argument sets of encode() / encoder_layer() at the
tiny width and two windows through the chooser.

Per (geometry, epilogue, bias): the seven kernels' C buffers are bit-identical; one buffer is within
the bound of the float64 reference on every element the scatter model writes; every other element of
the buffer has the canary's bits; a group's output is the same bits when it is launched alone.
tests/test_enc_gemm_ref_cpu.py shows what the bounds and the canary catch.  Every test prints its
worst |err| / bound, and the module's worst per epilogue at the end.

Measured on an MI355X (enc_gemm_ref.py's docstring has the record): every set of launches bit-identical;
worst |err| / bound 0.946 EPI_F16, 0.938 EPI_F16_GELU, 0.928 EPI_HEADS (the fp16 rounding), 0.008 EPI_F32,
0.011 EPI_F32_RESID, 0.008 EPI_F32_GELU_POS; LayerNorm 0.996 plain, 0.906 large-mean, 0.972 dominant.
"""
import functools

import numpy as np
import pytest

import dec_gemm_ref as R
import enc_gemm_ref as E
from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd.engine import WhisperEngine

pytestmark = pytest.mark.gpu
F32, F16, F64 = np.float32, np.float16, np.float64
WORST = {}


@pytest.fixture(scope="module")
def eng():
    d = D.WhisperDims(n_mels=80, n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128,
                      n_text_head=2, n_text_layer=1)
    e = WhisperEngine(d, device=0, max_batch=1)
    yield e
    e.close()
    for k in sorted(WORST):
        print(f"worst |err| / bound, {k}: {WORST[k]:.3f}")


def launch(eng, case, inp, variant):
    return eng.debug_enc_gemm(inp.A, inp.W, E.canary_buffer(case, inp), M=case.M, epi=case.epi, variant=variant,
                              lda=case.lda, a_grp_rows=case.a_grp_rows, a_grp_stride=case.a_grp_stride, ldc=case.ldc,
                              c_grp_rows=case.c_grp_rows, c_grp_stride=case.c_grp_stride, c_offset=case.c_offset,
                              bias=inp.bias, pos=inp.pos, heads=case.heads, heads_slot=case.slots)


@functools.lru_cache(maxsize=2)
def case_data(case, wb):
    inp = E.make_inputs(case, wb)
    return (inp,) + E.reference(case, inp)


def record(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def check_case(eng, case, wb, variants):
    """All `variants` give the same bits; the first one's buffer is within the bound where the model
    writes and the canary everywhere else.  -> that buffer."""
    inp, ref, bound = case_data(case, wb)
    what = f"{case.name} {E.EPI_NAMES[case.epi]} {'bias' if wb else 'no bias'}"
    bufs = [launch(eng, case, inp, v) for v in variants]
    ratio, touched = E.check_buffer(case, inp, bufs[0], ref, bound)
    print(f"{what}: variant {variants[0]} worst |err| / bound = {ratio:.3f}, unwritten elements changed: {touched}")
    differ = [v for v, b in zip(variants[1:], bufs[1:]) if not np.array_equal(E.bits(b), E.bits(bufs[0]))]
    assert touched == 0, f"{what}: {touched} elements outside the scatter model's set were written"
    assert ratio <= 1, (what, ratio)
    assert not differ, f"{what}: variants {differ} differ from variant {variants[0]} in bits"
    record(E.EPI_NAMES[case.epi], ratio)
    return bufs[0]


def check_groups_alone(eng, case, wb, full):
    """Group (window) q launched alone, through the chooser and each of the seven kernels, gives the
    bits it has in the launch of all groups, within the bound, and writes nothing else."""
    inp, ref, bound = case_data(case, wb)
    idx = E.c_index(case)
    rows = case.heads[0] if case.heads else case.c_grp_rows
    for q in range(case.groups):
        sub, sin = E.group_inputs(case, inp, q)
        sl = slice(q * rows, q * rows + sub.M)
        want = E.bits(full.ravel()[idx[sl]])
        for v in ALL:
            got = launch(eng, sub, sin, v)
            ratio, touched = E.check_buffer(sub, sin, got, ref[sl], bound[sl])
            assert touched == 0 and ratio <= 1, (case.name, q, v, ratio, touched)
            assert np.array_equal(E.bits(got.ravel()[E.c_index(sub)]), want), \
                f"{case.name}: group {q} alone (variant {v}) differs from the same group among {case.groups}"


def guard_rows_intact(case, full):
    """The rows in front of and behind the written rows, and the pad columns of every row, are canary."""
    canary = E.CANARY16 if E.is_f16(case.epi) else E.CANARY32
    rows = E.bits(full).reshape(-1, case.ldc)
    first = case.c_offset // case.ldc
    assert rows.shape[0] - first - case.M >= E.GUARD_ROWS
    return bool((rows[:first] == canary).all() and (rows[first + case.M:] == canary).all()
                and (rows[:, case.N:] == canary).all())


ALL = (0,) + E.VARIANTS


@pytest.mark.parametrize("wb", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", E.CONV1_SMALL, ids=lambda c: f"N{c.N}-{E.EPI_NAMES[c.epi]}")
def test_conv1_like(eng, case, wb):
    """Overlapping A rows (lda = C1, K = 3 C1) in 3 groups of 150 with a 2-row gap, C at an offset with a
    one-row gap between groups: 64-, 128- and 256-row tiles straddle the groups, the last column tile is
    partial, and row 0 of every window and the row after the last window keep the canary."""
    full = check_case(eng, case, wb, ALL)
    rows = E.bits(full).reshape(-1, case.N)
    border = [w * (E.SMALL_R + 1) for w in range(E.SMALL_G + 1)]
    assert (rows[border] == E.CANARY16).all(), "a conv1 border row was written"
    check_groups_alone(eng, case, wb, full)


@pytest.mark.parametrize("wb", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", E.CONV2_SMALL, ids=lambda c: f"G{c.groups}")
def test_conv2_like(eng, case, wb):
    """Stride-2 overlapping A rows (lda = 2 De, K = 3 De) in 3 and 4 groups of 75, gelu(acc + bias) +
    pos[row in its group]; the two rows behind the last group keep the canary."""
    full = check_case(eng, case, wb, ALL)
    assert guard_rows_intact(case, full), "a row behind the last group was written"
    check_groups_alone(eng, case, wb, full)


@pytest.mark.parametrize("M,N,K", E.PLAIN_SHAPES)
def test_plain_rows_every_epilogue(eng, M, N, K):
    """One group, contiguous rows, partial last row and column tiles at every tile size: the five
    epilogues that take these widths (the head-major one needs N % 128 == 0), with and without a bias;
    EPI_F32_RESID accumulates onto a random residual.  The C rows lie between one canary row in front and
    two behind (a row stored past M lands there, not outside the allocation), and at K = 192 they are
    N + 8 apart (a chunk stored past N lands on the pad columns, not on the next row's own store)."""
    for case in E.plain_cases(M, N, K):
        for wb in (True, False):
            full = check_case(eng, case, wb, ALL)
            assert guard_rows_intact(case, full), f"{case.name} {E.EPI_NAMES[case.epi]}: a guard row or pad column was written"


@pytest.mark.parametrize("wb", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", E.HEADS_SMALL, ids=lambda c: f"N{c.N}-nb{c.heads[2]}")
def test_head_major(eng, case, wb):
    """[which][nb][H][T][64] with T = 150, H = 2, two windows: without slots every element of the buffer
    is written exactly once (a permutation: no canary left, nothing outside); with slots (3, 0) of 4 the
    windows land in slots 3 and 0, and slots 1 and 2 keep the canary."""
    full = check_case(eng, case, wb, ALL)
    T, H, nb = case.heads
    b = E.bits(full).reshape(-1, nb, H * T * 64)
    if case.slots is None:
        assert (b != E.CANARY16).all()
    else:
        assert (b[:, (1, 2)] == E.CANARY16).all() and (b[:, (0, 3)] != E.CANARY16).all()
    check_groups_alone(eng, case, wb, full)


@pytest.mark.parametrize("case", E.production_cases(), ids=lambda c: c.name.replace(" ", "_"))
def test_production_geometry_through_the_chooser(eng, case):
    """encode()'s and encoder_layer()'s argument sets at the tiny width (De 384, C1 128 with 80 live mel
    columns, 3000 frames, T 1500) and two windows, through launch_gemm's own choice of kernel."""
    full = check_case(eng, case, True, (0,))
    if case.name.startswith("conv1"):
        rows = E.bits(full).reshape(-1, case.N)
        assert (rows[[0, 3001, 6002]] == E.CANARY16).all(), "a conv1 border row was written"
    elif not case.heads:
        assert guard_rows_intact(case, full), f"{case.name}: a row past M was written"


@pytest.mark.parametrize("kind", R.LN_KINDS)
@pytest.mark.parametrize("Dm", E.ENC_LN_WIDTHS)
def test_encoder_layernorm(eng, Dm, kind):
    """layernorm_kernel<1, 2, 3> (D 128, 256, 384) and layernorm4_kernel<2 .. 5> (512 .. 1280), 1, 5 and 7
    rows (one wave per row, four per block: the row >= M exit) into an 8-row buffer: within 4 x the
    float32 restatement's error + one fp16 rounding of the float64 LayerNorm; rows past M keep the canary."""
    worst = 0.0
    for M in E.ENC_LN_ROWS:
        x, g, b = E.enc_ln_case(kind, M, Dm)
        y0 = np.full((E.ENC_LN_ALLOC, Dm), E.CANARY16, np.uint16).view(F16)
        y = eng.debug_enc_layernorm(x, g, b, y0)
        assert (E.bits(y[M:]) == E.CANARY16).all(), f"D {Dm} M {M}: a row past M was written"
        tol, ref, _ = E.enc_ln_tolerance(x, g, b)
        err = np.abs(y[:M].astype(F64) - ref)
        assert not np.isnan(err).any(), f"D {Dm} M {M}: an element was not written"
        worst = max(worst, float((err / tol).max()))
    print(f"encoder LN {kind} D {Dm}: worst |err| / tolerance = {worst:.3f}")
    assert worst <= 1
    record(f"layernorm {kind}", worst)


def test_preconditions_are_errors(eng):
    """Every argument set a kernel could read or write out of bounds with, or that would run another
    kernel than the one named, is refused (OSW_EINVAL) before anything is launched."""
    M, N, K = 64, 64, 64
    A = np.zeros(M * K, F16)
    W = np.zeros((N, K), F16)
    c16, c32 = np.zeros(M * N, F16), np.zeros(M * N, F32)
    bias = np.zeros(N, F32)
    ok = dict(M=M, epi=E.EPI_F16, variant=1)
    eng.debug_enc_gemm(A, W, c16, **ok)                                    # the base case itself is served
    W68, c68 = np.zeros((68, K), F16), np.zeros(M * 68, F32)
    bad = [
        ("K % 64", (np.zeros(M * 96, F16), np.zeros((N, 96), F16), c16), ok),
        ("lda % 8", (np.zeros(M * 68, F16), W, c16), dict(ok, lda=68)),
        ("a_grp_stride % 8", (np.zeros(2 * M * K, F16), W, c16), dict(ok, a_grp_rows=32, a_grp_stride=32 * K + 4)),
        ("A row past the buffer", (A[:-8], W, c16), ok),
        ("A group past the buffer", (A, W, c16), dict(ok, a_grp_rows=32, a_grp_stride=32 * K + 8)),
        ("C row past the buffer", (A, W, c16[:-8]), ok),
        ("C group past the buffer", (A, W, c16), dict(ok, c_grp_rows=32, c_grp_stride=32 * N + 8)),
        ("C offset past the buffer", (A, W, c16), dict(ok, c_offset=8)),
        ("C offset % 8", (A, W, np.zeros(M * N + 8, F16)), dict(ok, c_offset=4)),
        ("N % 8, fp16", (A, W68, np.zeros(M * 68, F16)), ok),
        ("ldc % 8, fp16", (A, W, np.zeros(M * 68, F16)), dict(ok, ldc=68)),
        ("c_grp_stride % 8, fp16", (A, W, np.zeros(M * N + 8, F16)), dict(ok, c_grp_rows=32, c_grp_stride=32 * N + 4)),
        ("N % 4, residual", (A, np.zeros((66, K), F16), np.zeros(M * 66, F32)), dict(ok, epi=E.EPI_F32_RESID)),
        ("ldc % 4, residual", (A, W, np.zeros(M * 66, F32)), dict(ok, epi=E.EPI_F32_RESID, ldc=66)),
        ("ldc % 4, gelu + pos", (A, W, np.zeros(M * 66, F32)),
         dict(ok, epi=E.EPI_F32_GELU_POS, ldc=66, pos=np.zeros((M, N), F32))),
        ("pos missing", (A, W, c32), dict(ok, epi=E.EPI_F32_GELU_POS)),
        ("pos short", (A, W, c32), dict(ok, epi=E.EPI_F32_GELU_POS, pos=np.zeros((M - 1, N), F32))),
        ("pos of another group size", (A, W, c32),
         dict(ok, epi=E.EPI_F32_GELU_POS, c_grp_rows=32, c_grp_stride=32 * N, pos=np.zeros((M, N), F32))),
        ("heads: N % (64 H)", (A, W, c16), dict(ok, epi=E.EPI_HEADS, heads=(32, 2, 2))),
        ("heads: M % T", (A, W, c16), dict(ok, epi=E.EPI_HEADS, heads=(48, 1, 2))),
        ("heads: extent", (A, W, c16), dict(ok, epi=E.EPI_HEADS, heads=(32, 1, 3))),
        ("heads: more windows than nb", (A, W, c16), dict(ok, epi=E.EPI_HEADS, heads=(32, 1, 1))),
        ("heads: slots equal", (A, W, np.zeros(2 * M * N, F16)), dict(ok, epi=E.EPI_HEADS, heads=(32, 1, 4), heads_slot=[1, 1])),
        ("heads: slot >= nb", (A, W, np.zeros(2 * M * N, F16)), dict(ok, epi=E.EPI_HEADS, heads=(32, 1, 4), heads_slot=[0, 4])),
        ("heads: slot < 0", (A, W, np.zeros(2 * M * N, F16)), dict(ok, epi=E.EPI_HEADS, heads=(32, 1, 4), heads_slot=[0, -1])),
        ("variant 11 without r128_ok", (A, W68, c68), dict(ok, epi=E.EPI_F32, variant=11)),
        ("variant 16 with N % 8", (A, W68, c68), dict(ok, epi=E.EPI_F32, variant=16)),
        ("N % 8, residual", (A, W68, c68), dict(ok, epi=E.EPI_F32_RESID)),
        ("ldc % 8, residual", (A, W, c68), dict(ok, epi=E.EPI_F32_RESID, ldc=68)),
        ("c_grp_stride % 8, gelu + pos", (A, W, np.zeros(M * N + 4, F32)),
         dict(ok, epi=E.EPI_F32_GELU_POS, c_grp_rows=32, c_grp_stride=32 * N + 4, pos=np.zeros((32, N), F32))),
        ("ldc < N", (A, W, c16), dict(ok, ldc=56)),
        ("C groups overlap", (A, W, c16), dict(ok, c_grp_rows=32, c_grp_stride=32 * N - 8)),
        ("C groups overlap, residual", (A, W, c32), dict(ok, epi=E.EPI_F32_RESID, c_grp_rows=32, c_grp_stride=31 * N)),
        ("epi 6", (A, W, c16), dict(ok, epi=6)),
        ("M 0", (A, W, c16), dict(ok, M=0)),
    ] + [(f"variant {v}", (A, W, c16), dict(ok, variant=v)) for v in (3, 5, 8, 9, 10, 12, 17, 18, -1, 99)]
    for what, (a, w, c), kw in bad:
        with pytest.raises(_lib.OswError) as ei:
            eng.debug_enc_gemm(a, w, c, **kw)
        assert not isinstance(ei.value, _lib.OswDeviceError), (what, str(ei.value))
        print(f"{what}: {ei.value}")
    # the plain fp32 store is served at N % 4 == 0 (run_gemm holds it to no rule; the 256-row tiles' 16-B chunks to this one)
    eng.debug_enc_gemm(A, W68, c68, M=M, epi=E.EPI_F32, variant=1)
    x = np.zeros((4, 640), F32)
    for xx, y in ((x, np.zeros((4, 640), F16)),                           # 5 x 128: no kernel
                  (np.zeros((4, 130), F32), np.zeros((4, 130), F16)),     # not a multiple of 128
                  (np.zeros((4, 1408), F32), np.zeros((4, 1408), F16)),   # wider than any kernel
                  (np.zeros((4, 256), F32), np.zeros((3, 256), F16))):    # M > M_alloc
        with pytest.raises(_lib.OswError) as ei:
            eng.debug_enc_layernorm(xx, np.ones(xx.shape[1], F32), np.zeros(xx.shape[1], F32), y)
        assert not isinstance(ei.value, _lib.OswDeviceError)
