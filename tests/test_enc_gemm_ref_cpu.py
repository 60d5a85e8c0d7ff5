"""What the bounds and canaries of tests/enc_gemm_ref.py catch, shown on the CPU: on every case the
GPU tests launch, the faithful float32 restatement meets its bound and leaves every unwritten
element alone, and each wrong restatement (enc_gemm_ref.MUTATIONS) misses the bound by at least
20x or is caught by the canary.  Every test prints faithful-versus-mutant ratios (worst |err| /
bound; <= 1 passes)."""
import numpy as np
import pytest

import dec_gemm_ref as R
import enc_gemm_ref as E

F64 = np.float64
MISS = 20.0
CASES = E.all_cases()


def _id(cw):
    c, wb = cw
    return f"{c.name} {E.EPI_NAMES[c.epi]} {'bias' if wb else 'nobias'}".replace(" ", "_")


@pytest.mark.parametrize("cw", CASES, ids=_id)
def test_faithful_meets_and_mutants_miss(cw):
    case, wb = cw
    inp = E.make_inputs(case, wb)
    ref, bound = E.reference(case, inp)
    buf, outside = E.restate(case, inp)
    ratio, touched = E.check_buffer(case, inp, buf, ref, bound)
    print(f"{_id(cw)}: faithful {ratio:.3f}")
    assert ratio <= 1 and touched == 0 and outside == 0
    for mut in E.MUTATIONS:
        if not E.mutation_applies(mut, case, wb):
            continue
        buf, outside = E.restate(case, inp, mut)
        r, touched = E.check_buffer(case, inp, buf, ref, bound)
        print(f"    {mut:20s} worst |err| / bound {r:10.3g}, unwritten elements changed {touched}, stores outside {outside}")
        assert r >= MISS or touched > 0 or outside > 0, mut
        if mut == "c-stride-short" and case.name.startswith("conv1"):
            assert touched > 0, f"{mut} must land in a border row"
        if mut in ("row-past-group", "chunk-past-n"):
            # every epilogue, the fp32 ones included: a row stored past M (or past a group into a gap) and a
            # chunk stored past N in the last row land on canary rows or pad columns of the buffer itself
            assert touched > 0 and outside == 0, f"{mut} must land on the canary"


def test_the_canary_check_is_never_vacuous():
    """Every buffer that is not head-major holds whole rows the model does not write, behind its last
    written row (the fp32 epilogues' buffers included), and the padded shapes a column tail per row; the
    head-major buffers without slots are written whole by definition (a permutation)."""
    padded = set()
    for case, _ in CASES:
        written = np.zeros(case.c_count, bool)
        written[E.c_index(case)] = True
        if case.heads:
            assert written.all() == (case.slots is None)
            continue
        rows = written.reshape(-1, case.ldc)
        last = np.flatnonzero(rows.any(1)).max()
        assert rows.shape[0] - 1 - last >= 1 and not rows[last + 1:].any(), case.name
        if not E.is_f16(case.epi):
            assert rows.shape[0] - 1 - last >= E.GUARD_ROWS, case.name
        if case.ldc > case.N:
            assert not rows[:, case.N:].any()
            padded.add(case.epi)
    assert padded == set(E.PLAIN_EPIS)


def test_every_mutation_is_exercised():
    for mut in E.MUTATIONS:
        n = sum(E.mutation_applies(mut, c, wb) for c, wb in CASES)
        print(f"{mut:20s} applies to {n} of {len(CASES)} cases")
        assert n >= 2, mut


def test_addressing_models_against_loops():
    """The vectorised gather and scatter models equal a naive loop over (m, n) / (m, k) written from the
    layout's definition, every output has its own element, and the conv1 layout leaves exactly the
    border rows unwritten."""
    tiny = [E.conv1_case(5, 3, 8, 16, E.EPI_F16), E.conv2_case(4, 3, 8, 16), E.plain_case(7, 16, 8, E.EPI_F32),
            E.heads_case(5, 2, 2, 256, 8), E.heads_case(5, 2, 2, 384, 8, nb=4, slots=(3, 0))]
    for case in tiny:
        A = np.arange(case.a_count, dtype=np.int64)
        assert np.array_equal(E.gather_a(case, A), E.naive_a(case, A)), case.name
        idx = E.c_index(case)
        assert np.array_equal(idx, E.naive_c_index(case)), case.name
        assert np.unique(idx).size == idx.size and idx.min() >= 0 and idx.max() < case.c_count
    c1 = tiny[0]
    written = np.zeros(c1.c_count, bool)
    written[E.c_index(c1)] = True
    rows = written.reshape(-1, c1.N)
    border = [w * 6 for w in range(3)] + [18]
    assert rows.all(1).sum() == 15 and not rows[border].any()
    h = tiny[3]
    assert E.c_index(h).size == h.c_count                     # no slots: a permutation of the whole buffer
    hs = tiny[4]
    w = np.zeros(hs.c_count, bool)
    w[E.c_index(hs)] = True
    assert not w.reshape(3, 4, -1)[:, (1, 2)].any() and w.reshape(3, 4, -1)[:, (0, 3)].all()
    # conv rows overlap: row t + 1 starts lda after row t and shares K - lda elements with it
    a = E.gather_a(c1, np.arange(c1.a_count))
    assert np.array_equal(a[1, :16], a[0, 8:]) and a[5, 0] == 7 * 8


@pytest.mark.parametrize("case", E.GROUPED_SMALL + [c for c in E.production_cases() if c.groups > 1],
                         ids=lambda c: c.name.replace(" ", "_"))
def test_grouped_geometries_straddle(case):
    """Each grouped shape has a 64-, a 128- and a 256-row tile holding rows of two groups, and (the
    head-major shapes aside: 128 H divides their N, so only the 256-column tiles can be partial) a
    partial last column tile at every tile width, computed from the shapes."""
    assert set(E.TILE_ROWS.values()) == {64, 128, 256} and set(E.TILE_COLS.values()) == {64, 128, 256}
    for tile in (64, 128, 256):
        assert E.straddling_tiles(case, tile), (case.name, tile)
        if not case.heads and case in E.GROUPED_SMALL:
            assert case.N % tile, (case.name, tile)


def test_plain_shapes_have_partial_tiles():
    for M, N, K in E.PLAIN_SHAPES:
        for tile in (64, 128, 256):
            assert M % tile and N % tile, (M, N, tile)
        assert N % 8 == 0 and K % 64 == 0
    for c in E.HEADS_SMALL:
        assert c.N % 256 or c.N == 512      # qkv (384): a partial 256-column tile; the 512-wide one has none


def test_one_group_is_the_group():
    """one_group(case, q) addresses the same A rows and, through its own C model, the same outputs."""
    for case in E.GROUPED_SMALL:
        inp = E.make_inputs(case)
        full = E.gather_a(case, inp.A)
        rows = case.heads[0] if case.heads else case.c_grp_rows
        for q in range(case.groups):
            sub, sin = E.group_inputs(case, inp, q)
            assert np.array_equal(E.gather_a(sub, sin.A), full[q * rows:q * rows + sub.M]), (case.name, q)
            assert E.c_index(sub).max() < sub.c_count


# --------------------------------------------------------------------------- LayerNorm
def test_measured_constants():
    ln = E.measure_enc_ln()
    print("ENC_LN_RESTATE_WORST =", {k: f"{v:.3e}" for k, v in ln.items()})
    for k, v in ln.items():
        assert v <= E.ENC_LN_RESTATE_WORST[k] <= 1.02 * v


def test_ln_kernel_choice():
    assert [E.ln_vec(D) for D in E.ENC_LN_WIDTHS] == [2, 2, 2, 4, 4, 4, 4]


@pytest.mark.parametrize("kind", R.LN_KINDS)
def test_ln_faithful_meets_tolerance(kind):
    worst = 0.0
    for D in E.ENC_LN_WIDTHS:
        for rows in E.ENC_LN_ROWS:
            x, g, b = E.enc_ln_case(kind, rows, D)
            tol, ref, _ = E.enc_ln_tolerance(x, g, b)
            y = E.restate_enc_ln(x, g, b).astype(np.float16).astype(F64)
            worst = max(worst, float((np.abs(y - ref) / tol).max()))
    print(f"encoder LN {kind}: faithful restatement rounded to fp16, worst |err| / tolerance = {worst:.3f}")
    assert worst <= 1


@pytest.mark.parametrize("D", E.ENC_LN_WIDTHS)
def test_ln_one_pass_variance_misses(D):
    x, g, b = E.enc_ln_case("large-mean", 5, D)
    tol, ref, _ = E.enc_ln_tolerance(x, g, b)
    bad = E.restate_enc_ln(x, g, b, one_pass=True).astype(np.float16).astype(F64)
    r = float((np.abs(bad - ref) / tol).max())
    print(f"encoder LN one-pass variance D {D}: worst |err| / tolerance = {r:.3g}")
    assert r >= MISS or not np.isfinite(r)
