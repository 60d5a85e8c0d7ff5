"""References, addressing models, inputs, bounds and wrong restatements for the encoder's tiled
GEMM family (gemm.hip: seven tile kernels x six epilogues, grouped A and C rows, the head-major
scatter) and the encoder's LayerNorm (misc.hip).  Plain numpy, no GPU.
tests/test_gpu_enc_gemm.py runs one launch per call against these (osw_debug_enc_gemm /
osw_debug_enc_layernorm); tests/test_enc_gemm_ref_cpu.py shows that every bound below is met by
a faithful float32 evaluation and missed by >= 20x (or caught by the canary) by each entry of
MUTATIONS: a plausible kernel bug restated as a one-line change of the model.

Addressing is written here from the layout's definition with integer // and %, never from the
kernels' code (which divides by a float reciprocal with a correction step):
  A row m     at (m // a_grp_rows) * a_grp_stride + (m % a_grp_rows) * lda, K elements
  C row m     at c_offset + (m // c_grp_rows) * c_grp_stride + (m % c_grp_rows) * ldc, N elements
  head-major  element (m, n) at c_offset + ((((n // 64H) * nb + slot[m // T]) * H + (n % 64H) // 64) * T
              + m % T) * 64 + n % 64

References are float64: v = A·Wᵀ + bias, gelu(v) with the exact erf, C0 + v, gelu(v) + pos[m % c_grp_rows].

Inputs: A and W fp16 ~ U(-1, 1); the bias ~ N(0, K / 9), the standard deviation of a product, and
different in every column; a positional table and a residual ~ N(0, 1), different in every element.
(A wrong bias column, positional row or a lost residual then moves an element by the size of the
element itself, >= 1000 x its bound.)

Bounds per element, from terms the project already states (dec_gemm_ref.G, measured on a float32
restatement of the accumulation; erf_fast's 1.5e-7; fp16's 2^-11 relative and 2^-25 absolute rounding;
fp32's 2^-24 relative rounding per add; max |gelu'| = 1.13):
  f32(v)      = G S + 2^-24 |v| with a bias, G S without (the epilogues then add -0.0, exactly)
                S = |A|·|W|ᵀ gathered the same way
  EPI_F32           f32(v)
  EPI_F16, _HEADS   f32(v) + r16(v),  r16(x) = 2^-11 |x| + 2^-25
  EPI_F16_GELU      1.13 f32(v) + 0.5 |v| 1.5e-7 + r16(gelu(v))
  EPI_F32_RESID     f32(v) + 2^-24 |C0 + v|
  EPI_F32_GELU_POS  1.13 f32(v) + 0.5 |v| 1.5e-7 + 2^-24 |gelu(v) + pos|
Unwritten elements are compared bit for bit with the canary (one fixed NaN pattern per type); every
buffer but the slot-less head-major ones has such elements: border or guard rows behind the last written
row (the fp32 epilogues' buffers too) and, on the padded plain shapes, 8 columns behind every row.

LayerNorm: the float64 reference and a float32 restatement of each kernel's scheme (one wave per
row, float2 or float4 per lane, the lane's pieces summed in order, the xor butterfly, two-pass
variance); the tolerance is 4 x the restatement's own worst error on the case + r16(reference) for
the one fp16 rounding, as dec_gemm_ref.ln_tolerance (no pair term: the output is one fp16).

Measured on an MI355X (every figure is printed by its test in tests/test_gpu_enc_gemm.py), worst
|err| / bound per epilogue over every geometry, with and without a bias, the chooser and all seven
kernels bit-identical throughout:
  EPI_F16 0.946   EPI_F16_GELU 0.938   EPI_HEADS 0.928   (the fp16 rounding itself: its worst case is r16)
  EPI_F32 0.008   EPI_F32_RESID 0.011  EPI_F32_GELU_POS 0.008
  LayerNorm worst |err| / tolerance: plain 0.996, large-mean 0.906, dominant 0.972 (the fp16 rounding again)
The faithful float32 restatement gives the same worst ratios on the CPU (0.946 over the GEMM cases;
0.996 / 0.906 / 0.972).  The wrong restatements miss by >= 1000x (the smallest: the residual
overwritten, 1050x; the positional row of the global m, 1810x) or change an unwritten element.
"""
from dataclasses import dataclass, replace

import numpy as np

import dec_gemm_ref as R

F32, F16, F64 = np.float32, np.float16, np.float64
EPI_F16, EPI_F16_GELU, EPI_F32_RESID, EPI_F32_GELU_POS, EPI_F32, EPI_HEADS = range(6)
EPI_NAMES = ("f16", "f16_gelu", "f32_resid", "f32_gelu_pos", "f32", "heads")
VARIANTS = (1, 2, 4, 6, 7, 11, 16)   # 128 double buffered, 256, 8-phase, 64 ring, 64, 128 ring, half-width
TILE_ROWS = {1: 128, 2: 256, 4: 256, 6: 64, 7: 64, 11: 128, 16: 256}
TILE_COLS = {1: 128, 2: 256, 4: 256, 6: 64, 7: 64, 11: 128, 16: 128}

CANARY16 = np.uint16(0x7E5A)          # fp16 NaN
CANARY32 = np.uint32(0x7FC5A5A5)      # fp32 NaN
GELU_SLOPE = 1.13                     # max |gelu'|


def is_f16(epi):
    return epi in (EPI_F16, EPI_F16_GELU, EPI_HEADS)


# --------------------------------------------------------------------------- geometry
@dataclass(frozen=True)
class Case:
    """One launch's argument set (osw_enc_gemm_desc without the data)."""
    name: str
    M: int
    N: int
    K: int
    epi: int
    lda: int
    a_grp_rows: int
    a_grp_stride: int
    a_count: int
    ldc: int = 0
    c_grp_rows: int = 0
    c_grp_stride: int = 0
    c_offset: int = 0
    c_count: int = 0
    heads: tuple = None        # (heads_T, heads_H, heads_nb)
    slots: tuple = None
    a_live: int = 0            # columns of every lda-long A row that are not zero (0: all)

    @property
    def groups(self):
        return -(-self.M // (self.heads[0] if self.heads else self.c_grp_rows))


GUARD_ROWS = 2    # rows of canary behind the last C row of every non-head-major buffer (one in front too)


def plain_case(M, N, K, epi, pad=0):
    """One group of contiguous A rows; C rows ldc = N + pad apart between one guard row in front and
    GUARD_ROWS behind, which (with the pad columns) no kernel may write: a row stored past M or a chunk
    stored past N lands on the canary instead of outside the allocation or on the next row."""
    ldc = N + pad
    return Case(f"plain {M}x{N}x{K} ldc {ldc}", M, N, K, epi, lda=K, a_grp_rows=M, a_grp_stride=0, a_count=M * K,
                ldc=ldc, c_grp_rows=M, c_offset=ldc, c_count=(1 + M + GUARD_ROWS) * ldc)


def conv1_case(R_, G, C1, N, epi, live=0, name="conv1-like"):
    """The stem's first convolution as an implicit GEMM: window w holds R_ + 2 rows of C1, GEMM row
    (w, t) reads rows t .. t+2 (K = 3 C1, lda = C1); C row (w, t) is row 1 + t of window w's R_ + 1
    output rows, and one more row follows the last window: row 0 of every window and that last row
    are conv2's zero padding and must not be written."""
    return Case(f"{name} {G}x{R_} N {N}", G * R_, N, 3 * C1, epi, lda=C1, a_grp_rows=R_, a_grp_stride=(R_ + 2) * C1,
                a_count=G * (R_ + 2) * C1, ldc=N, c_grp_rows=R_, c_grp_stride=(R_ + 1) * N, c_offset=N,
                c_count=(G * (R_ + 1) + 1) * N, a_live=live)


def conv2_case(Rp, G, De, N, name="conv2-like"):
    """The stride-2 convolution: window w holds 2 Rp + 1 rows of De, GEMM row (w, t) reads rows
    2t .. 2t+2 (K = 3 De, lda = 2 De); C contiguous per window, GUARD_ROWS rows of canary behind the
    last window; gelu + pos[t]."""
    return Case(f"{name} {G}x{Rp} N {N}", G * Rp, N, 3 * De, EPI_F32_GELU_POS, lda=2 * De, a_grp_rows=Rp,
                a_grp_stride=(2 * Rp + 1) * De, a_count=(G * (2 * Rp + 1) + 1) * De, ldc=N, c_grp_rows=Rp,
                c_grp_stride=Rp * N, c_offset=0, c_count=(G * Rp + GUARD_ROWS) * N)


def heads_case(T, H, windows, N, K, nb=None, slots=None, name="heads"):
    nb = windows if nb is None else nb
    M = windows * T
    return Case(f"{name} {windows}x{T} H {H} N {N} nb {nb} slots {slots}", M, N, K, EPI_HEADS, lda=K, a_grp_rows=M,
                a_grp_stride=0, a_count=M * K, ldc=0, c_grp_rows=M, c_offset=0,
                c_count=(N // (64 * H)) * nb * H * T * 64, heads=(T, H, nb), slots=None if slots is None else tuple(slots))


def one_group(case, q):
    """The launch that computes group (window) q of `case` alone, over the same buffers' layout:
    -> (case of one group, element offset of its A rows in case's A buffer)."""
    if case.heads:
        T, H, nb = case.heads
        sub = replace(case, M=T, a_grp_rows=T, a_count=T * case.K, c_grp_rows=T,
                      slots=None if case.slots is None else (case.slots[q],))
        return sub, q * T * case.lda
    rows = min(case.a_grp_rows, case.M - q * case.a_grp_rows)
    assert case.a_grp_rows == case.c_grp_rows
    a0 = q * case.a_grp_stride
    return replace(case, M=rows, a_grp_rows=rows, c_grp_rows=rows, a_count=case.a_count - a0), a0


# the GPU tests' small geometries -------------------------------------------------------------
SMALL_R, SMALL_G = 150, 3
CONV1_SMALL = [conv1_case(SMALL_R, SMALL_G, 64, N, epi) for N in (136, 264) for epi in (EPI_F16_GELU, EPI_F16)]
CONV2_SMALL = [conv2_case(75, G, 128, 136) for G in (3, 4)]
PLAIN_SHAPES = [(M, N, K) for M in (257, 450) for N in (136, 264) for K in (64, 192)]
# (EPI_HEADS needs N % (64 H) == 0, which neither 136 nor 264 is: the head-major scatter has HEADS_SMALL)
PLAIN_EPIS = (EPI_F16, EPI_F16_GELU, EPI_F32_RESID, EPI_F32_GELU_POS, EPI_F32)
HEADS_SMALL = [heads_case(150, 2, 2, N, 128, nb, slots)
               for N in (3 * 128, 2 * 2 * 128) for nb, slots in ((2, None), (4, (3, 0)))]
GROUPED_SMALL = CONV1_SMALL + CONV2_SMALL + HEADS_SMALL


def production_cases(n=2, De=384, H=6, C1=128, mels=80, Rf=3000, T=1500, text_layers=4, slots_nb=3, slots=(2, 0)):
    """The arguments of encode() and encoder_layer() at the tiny width for n windows."""
    M = n * T
    plain = lambda nm, N, K, epi: replace(plain_case(M, N, K, epi), name=nm)
    return [
        conv1_case(Rf, n, C1, De, EPI_F16_GELU, live=mels, name="conv1"),
        replace(conv2_case(T, n, De, De, name="conv2"), a_grp_stride=(Rf + 1) * De, a_count=(n * (Rf + 1) + 1) * De),
        heads_case(T, H, n, 3 * De, De, name="qkv"),
        plain("out-projection", De, De, EPI_F32_RESID),
        plain("fc1", 4 * De, De, EPI_F16_GELU),
        plain("fc2", De, 4 * De, EPI_F32_RESID),
        heads_case(T, H, n, text_layers * 2 * De, De, name="cross-K/V"),
        heads_case(T, H, n, text_layers * 2 * De, De, nb=slots_nb, slots=slots, name="cross-K/V"),
    ]


def plain_cases(M, N, K):
    """The five epilogues on one plain shape; the K = 192 shapes with 8 pad columns behind every C row."""
    return [plain_case(M, N, K, e, pad=8 if K == 192 else 0) for e in PLAIN_EPIS]


def all_cases():
    """Every (case, with_bias) the GPU tests launch (the one-group launches of the group-count check aside)."""
    small = GROUPED_SMALL + [c for s in PLAIN_SHAPES for c in plain_cases(*s)]
    return [(c, wb) for c in small for wb in (True, False)] + [(c, True) for c in production_cases()]


def straddling_tiles(case, tile):
    """Row tiles [i tile, (i+1) tile) of the launch that hold rows of two groups (windows)."""
    rows = case.heads[0] if case.heads else case.c_grp_rows
    return [i for i in range(-(-case.M // tile))
            if (i * tile) // rows != (min((i + 1) * tile, case.M) - 1) // rows]


# --------------------------------------------------------------------------- addressing models
def a_offsets(case, short_stride=False):
    m = np.arange(case.M, dtype=np.int64)
    stride = case.a_grp_stride - (case.lda if short_stride else 0)
    return (m // case.a_grp_rows) * stride + (m % case.a_grp_rows) * case.lda


def gather_a(case, Abuf, short_stride=False):
    """[M][K]: the GEMM's A rows out of the flat buffer."""
    return Abuf[a_offsets(case, short_stride)[:, None] + np.arange(case.K, dtype=np.int64)[None, :]]


def c_index(case, mut=None):
    """[M][N] int64: the element of the C buffer that output (m, n) goes to."""
    m = np.arange(case.M, dtype=np.int64)[:, None]
    n = np.arange(case.N, dtype=np.int64)[None, :]
    if case.heads:
        T, H, nb = case.heads
        Dh = 64 * (H + 1 if mut == "heads-width" else H)      # the width `which` and `h` are decoded with
        which, h, d = n // Dh, (n % Dh) // 64, n % 64
        w = m // T
        slot = np.asarray(case.slots, np.int64)[w] if (case.slots is not None and mut != "slot-ignored") else w
        return case.c_offset + ((((which * nb + slot) * H + h) * T + m % T) * 64 + d)
    stride = case.c_grp_stride - (case.ldc if mut == "c-stride-short" else 0)
    return case.c_offset + (m // case.c_grp_rows) * stride + (m % case.c_grp_rows) * case.ldc + n


def naive_a(case, Abuf):
    out = np.zeros((case.M, case.K), Abuf.dtype)
    for m in range(case.M):
        g, r = divmod(m, case.a_grp_rows)
        for k in range(case.K):
            out[m, k] = Abuf[g * case.a_grp_stride + r * case.lda + k]
    return out


def naive_c_index(case):
    out = np.zeros((case.M, case.N), np.int64)
    for m in range(case.M):
        for n in range(case.N):
            if case.heads:
                T, H, nb = case.heads
                w, t = divmod(m, T)
                which, rest = divmod(n, 64 * H)
                h, d = divmod(rest, 64)
                b = case.slots[w] if case.slots is not None else w
                out[m, n] = case.c_offset + ((((which * nb) + b) * H + h) * T + t) * 64 + d
            else:
                g, r = divmod(m, case.c_grp_rows)
                out[m, n] = case.c_offset + g * case.c_grp_stride + r * case.ldc + n
    return out


# --------------------------------------------------------------------------- inputs
@dataclass
class Inputs:
    A: np.ndarray          # fp16 [a_count]
    W: np.ndarray          # fp16 [N][K]
    bias: np.ndarray       # fp32 [N] or None
    pos: np.ndarray        # fp32 [c_grp_rows][N] or None
    C0: np.ndarray         # fp32 [M][N] (EPI_F32_RESID: the residual already in C) or None


def make_inputs(case, with_bias=True, seed=0):
    """Row m's A data, W, the bias and the tables depend on (seed, shape) only, not on the epilogue."""
    rng = np.random.default_rng([seed, case.a_count, case.N, case.K])
    A = rng.uniform(-1, 1, case.a_count).astype(F16)
    if case.a_live:
        A = np.where(np.arange(case.a_count) % case.lda < case.a_live, A, F16(0))
    W = rng.uniform(-1, 1, (case.N, case.K)).astype(F16)
    bias = (rng.standard_normal(case.N) * np.sqrt(case.K) / 3).astype(F32)
    rows = case.c_grp_rows if not case.heads else 1
    pos = rng.standard_normal((rows, case.N)).astype(F32) if case.epi == EPI_F32_GELU_POS else None
    C0 = rng.standard_normal((case.M, case.N)).astype(F32) if case.epi == EPI_F32_RESID else None
    return Inputs(A, W, bias if with_bias else None, pos, C0)


def group_inputs(case, inp, q):
    """The inputs of one_group(case, q): the same data, A from the group's first row on."""
    sub, a0 = one_group(case, q)
    rows = slice(q * case.c_grp_rows, q * case.c_grp_rows + sub.M) if not case.heads else None
    return sub, Inputs(inp.A[a0:a0 + sub.a_count], inp.W, inp.bias, inp.pos, None if inp.C0 is None else inp.C0[rows])


def canary_buffer(case, inp):
    """The C buffer before the launch: the canary everywhere, the residual where EPI_F32_RESID reads it."""
    if is_f16(case.epi):
        return np.full(case.c_count, CANARY16, np.uint16).view(F16)
    buf = np.full(case.c_count, CANARY32, np.uint32).view(F32)
    if case.epi == EPI_F32_RESID:
        buf[c_index(case)] = inp.C0
    return buf


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == F16 else np.uint32)


# --------------------------------------------------------------------------- reference and bounds
def r16(x):
    return 2.0 ** -11 * np.abs(x) + 2.0 ** -25


def f32_bound(S, v, with_bias):
    """|fp32 accumulator (+ bias) - v|: G S for the MFMA chain, one fp32 rounding for the bias add."""
    return R.G * S + (2.0 ** -24 * np.abs(v) if with_bias else 0.0)


def f16_bound(acc, v):
    return acc + r16(v)


def gelu_f16_bound(acc, v, gelu):
    """fp16(gelu_erf(x)) against gelu(v), |x - v| <= acc (test_gpu_kernels.py's fp16 GELU epilogues too)."""
    return GELU_SLOPE * acc + 0.5 * np.abs(v) * R.ERF_FAST_ERR + r16(gelu)


def reference(case, inp):
    """-> (ref [M][N] float64, bound [M][N]) of the epilogue's output."""
    A = gather_a(case, inp.A)
    v = A.astype(F64) @ inp.W.astype(F64).T
    S = (np.abs(A).astype(F32) @ np.abs(inp.W).astype(F32).T).astype(F64)
    wb = inp.bias is not None
    if wb:
        v = v + inp.bias.astype(F64)
    acc = f32_bound(S, v, wb)
    e = case.epi
    if e == EPI_F32:
        return v, acc
    if e in (EPI_F16, EPI_HEADS):
        return v, f16_bound(acc, v)
    if e == EPI_F32_RESID:
        ref = inp.C0.astype(F64) + v
        return ref, acc + 2.0 ** -24 * np.abs(ref)
    g = R.gelu_ref(v)
    if e == EPI_F16_GELU:
        return g, gelu_f16_bound(acc, v, g)
    ref = g + inp.pos.astype(F64)[np.arange(case.M) % case.c_grp_rows]
    return ref, GELU_SLOPE * acc + 0.5 * np.abs(v) * R.ERF_FAST_ERR + 2.0 ** -24 * np.abs(ref)


def check_buffer(case, inp, buf, ref, bound):
    """-> (worst |err| / bound over the written elements (inf for a NaN), number of elements the
    model does not write whose bits are not the canary's)."""
    idx = c_index(case)
    flat = np.ascontiguousarray(buf).ravel()
    assert flat.size == case.c_count and flat.dtype == (F16 if is_f16(case.epi) else F32)
    written = np.zeros(case.c_count, bool)
    written[idx] = True
    canary = CANARY16 if is_f16(case.epi) else CANARY32
    touched = int((bits(flat)[~written] != canary).sum())
    err = np.abs(flat[idx].astype(F64) - ref)
    ratio = err / np.maximum(bound, 1e-300)
    ratio[np.isnan(err)] = np.inf
    return float(ratio.max()), touched


# --------------------------------------------------------------------------- restatements
# name -> what a kernel with that bug would produce; each is one changed line of restate()
MUTATIONS = ("bias-dropped", "bias-n+16", "bias-tile-column", "pos-global-row", "gelu-skipped", "resid-overwritten",
             "a-stride-short", "c-stride-short", "row-past-group", "slot-ignored", "heads-width", "last-chunk-dropped", "chunk-past-n")


def mutation_applies(mut, case, with_bias):
    e = case.epi
    return {"bias-dropped": with_bias, "bias-n+16": with_bias, "bias-tile-column": with_bias,
            "pos-global-row": e == EPI_F32_GELU_POS and case.groups > 1,
            "gelu-skipped": e in (EPI_F16_GELU, EPI_F32_GELU_POS),
            "resid-overwritten": e == EPI_F32_RESID,
            "a-stride-short": case.M > case.a_grp_rows,
            "c-stride-short": not case.heads and case.M > case.c_grp_rows,
            "row-past-group": not case.heads,      # (one group: the row past M)
            "chunk-past-n": not case.heads,
            "slot-ignored": case.slots is not None,
            "heads-width": case.heads is not None,
            "last-chunk-dropped": True}[mut]


def restate(case, inp, mut=None):
    """The launch in float32 with the kernels' fp16 rounding points (the product by an fp32 matmul: the
    MFMA's own summation order is G's business), scattered into a canary buffer.  -> (buffer, number of
    stores that fell outside the buffer).  mut: one of MUTATIONS."""
    A = gather_a(case, inp.A, short_stride=mut == "a-stride-short")
    v = A.astype(F32) @ inp.W.astype(F32).T
    n = np.arange(case.N)
    if inp.bias is not None and mut != "bias-dropped":
        col = (n + 16) % case.N if mut == "bias-n+16" else (n // 64) * 64 if mut == "bias-tile-column" else n
        v = v + inp.bias[col]
    e = case.epi
    if e in (EPI_F16_GELU, EPI_F32_GELU_POS) and mut != "gelu-skipped":
        v = R.restate_gelu(v)
    if e == EPI_F32_GELU_POS:
        m = np.arange(case.M)
        v = v + inp.pos[np.minimum(m, case.c_grp_rows - 1) if mut == "pos-global-row" else m % case.c_grp_rows]
    if e == EPI_F32_RESID and mut != "resid-overwritten":
        v = inp.C0 + v
    v = v.astype(F16 if is_f16(e) else F32)
    buf = canary_buffer(case, inp).copy()
    idx = c_index(case, mut)
    if mut == "last-chunk-dropped":
        idx, v = idx[:, :-8], v[:, :-8]
    if mut == "chunk-past-n":       # every row's last 16-B chunk stored once more, one chunk further
        c = 8 if is_f16(e) else 4
        idx, v = np.concatenate([idx, idx[:, -c:] + c], 1), np.concatenate([v, v[:, -c:]], 1)
    if mut == "row-past-group":     # every group's last row stored once more, one row further
        last = np.minimum((np.arange(case.groups) + 1) * case.c_grp_rows, case.M) - 1
        idx, v = np.concatenate([idx, idx[last] + case.ldc]), np.concatenate([v, v[last]])
    ok = (idx >= 0) & (idx < case.c_count)
    buf[idx[ok]] = v[ok]
    return buf, int((~ok).sum())


# --------------------------------------------------------------------------- LayerNorm
ENC_LN_WIDTHS = (128, 256, 384, 512, 768, 1024, 1280)
ENC_LN_ROWS = (1, 5, 7)
ENC_LN_ALLOC = 8


def ln_vec(D):
    """Elements per lane and piece of the kernel launch_layernorm picks: layernorm4_kernel (float4) for
    D = 512, 768, 1024, 1280; layernorm_kernel (float2) for 128, 256, 384."""
    return 4 if D % 256 == 0 and 2 <= D // 256 <= 5 else 2


def _wave_sum(v):
    """[rows][64] -> wave_sum's xor butterfly (32, 16, 8, 4, 2, 1), every lane's total; lane 0's is returned."""
    s = v.astype(F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def _piece_sum(p):
    """[..., vec] -> the piece's sum as the kernels write it: x + y, or (x + y) + (z + w)."""
    return p[..., 0] + p[..., 1] if p.shape[-1] == 2 else (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])


def restate_enc_ln(x, gain, shift, one_pass=False):
    """The encoder's LayerNorm in float32 in the kernel's order, before the fp16 rounding: lane l's piece i
    is columns vec (64 i + l) .. + vec; the lane adds its pieces' sums in order, the wave sum is the xor
    butterfly; two-pass variance.  one_pass (a wrong kernel): E[x^2] - mean^2."""
    x = np.asarray(x, F32)
    rows, D = x.shape
    vec = ln_vec(D)
    v = x.reshape(rows, D // (64 * vec), 64, vec)           # [rows][piece][lane][vec]
    s = np.zeros((rows, 64), F32)
    for i in range(v.shape[1]):
        s = s + _piece_sum(v[:, i])
    mean = (_wave_sum(s) / F32(D)).astype(F32)[:, None, None, None]
    d = v if one_pass else (v - mean).astype(F32)
    q = np.zeros((rows, 64), F32)
    for i in range(v.shape[1]):
        q = q + _piece_sum((d[:, i] * d[:, i]).astype(F32))
    var = (_wave_sum(q) / F32(D)).astype(F32)
    if one_pass:
        var = var - (mean[:, 0, 0, 0] * mean[:, 0, 0, 0]).astype(F32)
    rstd = (F32(1) / np.sqrt(var + F32(1e-5), dtype=F32)).astype(F32)[:, None]
    g, b = np.asarray(gain, F32), np.asarray(shift, F32)
    return (((x - mean[:, :, 0, 0]) * rstd).astype(F32) * g).astype(F32) + b


def enc_ln_case(kind, rows, D):
    """-> (x [rows][D], gain, shift): dec_gemm_ref.ln_inputs' kinds, x the residual after its update."""
    _, _, _, gain, shift, xp = R.ln_case(kind, rows, D, 1, True)
    return xp, gain, shift


def enc_ln_tolerance(x, gain, shift):
    """Per element: 4 x the float32 restatement's worst error on these rows + r16(reference)."""
    ref = R.ln_ref(x, gain, shift)
    worst = float(np.abs(restate_enc_ln(x, gain, shift).astype(F64) - ref).max())
    return 4 * worst + r16(ref), ref, worst


def measure_enc_ln():
    """Worst float32-restatement error per input kind over the GPU tests' cases."""
    worst = {}
    for kind in R.LN_KINDS:
        for D in ENC_LN_WIDTHS:
            for rows in ENC_LN_ROWS:
                x, g, b = enc_ln_case(kind, rows, D)
                worst[kind] = max(worst.get(kind, 0.0), enc_ln_tolerance(x, g, b)[2])
    return worst


# python -m pytest tests/test_enc_gemm_ref_cpu.py -s -k measured
# (the tests take 4 x the worst of their own case; these are the record)
ENC_LN_RESTATE_WORST = {"plain": 7.25e-7, "large-mean": 2.09e-4, "dominant": 4.55e-6}
