"""The four production epilogues of the persistent 8-phase encoder GEMM under the co-residency budget
(csrc/coresidency.h; tests/test_kernel_resources_cpu.py holds the register numbers): one launch per
call on host data (osw_debug_enc_gemm) with the 8-phase tile forced, bit for bit against the unchanged
128-row double-buffered tile of the same epilogue.

Per epilogue, M = 300 (two row tiles, the second ragged) and 512, N = 256 and 512, K = 128 (an even
K-tile count: variant 21 leaves through the NEXT0 epilogue) and 192 (odd: never), with and without a
bias, through
  variant 4   the production form, one workgroup per tile (prefetch depth RESID_PF),
  variant 20  the fp32 epilogues' other prefetch depth (the same kernel as 4 for the fp16 ones),
  variant 21  one workgroup over all tiles with the next tile's first K-tile staged under each
              epilogue: every tile but the last leaves through staged_epilogue_next0.
EPI_F32_RESID accumulates in place onto a random residual; EPI_F32_GELU_POS has grouped C rows
(c_grp_rows 150) and a positional table; EPI_HEADS has 2 heads and T = 150 at M = 300 (a row tile
crosses the window boundary) and T = 128 at M = 512 (M must be a multiple of T).  The first buffer is
also held to enc_gemm_ref's float64 bound and canary, so "identical" cannot mean "identically wrong".
"""
import numpy as np
import pytest

import enc_gemm_ref as E
from open_speech_amd import dims as D
from open_speech_amd.engine import WhisperEngine

pytestmark = pytest.mark.gpu

BASE = 1                      # the 128-row double-buffered tile (gemm_kernel): not touched by the budget work
FORMS = (4, 20, 21)
SHAPES = [(M, N, K) for M in (300, 512) for N in (256, 512) for K in (128, 192)]
EPIS = (E.EPI_F16_GELU, E.EPI_HEADS, E.EPI_F32_RESID, E.EPI_F32_GELU_POS)


def grouped_pos_case(M, N, K, rows=150):
    """Contiguous A rows; C in groups of `rows` rows (the last one short at M = 512) with GUARD_ROWS of
    canary behind the last; gelu(acc + bias) + pos[row in its group]."""
    G = -(-M // rows)
    return E.Case(f"grouped-pos {M}x{N}x{K}", M, N, K, E.EPI_F32_GELU_POS, lda=K, a_grp_rows=M, a_grp_stride=0,
                  a_count=M * K, ldc=N, c_grp_rows=rows, c_grp_stride=rows * N, c_offset=0,
                  c_count=(G * rows + E.GUARD_ROWS) * N)


def case_of(epi, M, N, K):
    if epi == E.EPI_HEADS:
        T = 150 if M % 150 == 0 else 128
        return E.heads_case(T, 2, M // T, N, K)
    if epi == E.EPI_F32_GELU_POS:
        return grouped_pos_case(M, N, K)
    return E.plain_case(M, N, K, epi, pad=8 if K == 192 else 0)


@pytest.fixture(scope="module")
def eng():
    d = D.WhisperDims(n_mels=80, n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128,
                      n_text_head=2, n_text_layer=1)
    e = WhisperEngine(d, device=0, max_batch=1)
    yield e
    e.close()


def launch(eng, case, inp, variant):
    return eng.debug_enc_gemm(inp.A, inp.W, E.canary_buffer(case, inp), M=case.M, epi=case.epi, variant=variant,
                              lda=case.lda, a_grp_rows=case.a_grp_rows, a_grp_stride=case.a_grp_stride, ldc=case.ldc,
                              c_grp_rows=case.c_grp_rows, c_grp_stride=case.c_grp_stride, c_offset=case.c_offset,
                              bias=inp.bias, pos=inp.pos, heads=case.heads, heads_slot=case.slots)


@pytest.mark.parametrize("epi", EPIS, ids=lambda e: E.EPI_NAMES[e])
def test_budgeted_8phase_forms_bit_identical_to_the_128_tile(eng, epi):
    worst = 0.0
    for M, N, K in SHAPES:
        case = case_of(epi, M, N, K)
        for wb in (True, False):
            inp = E.make_inputs(case, wb)
            ref, bound = E.reference(case, inp)
            base = launch(eng, case, inp, BASE)
            ratio, touched = E.check_buffer(case, inp, base, ref, bound)
            what = f"{case.name} {E.EPI_NAMES[epi]} {'bias' if wb else 'no bias'}"
            assert touched == 0 and ratio <= 1, (what, ratio, touched)
            worst = max(worst, ratio)
            if epi == E.EPI_F32_RESID:
                assert np.abs(inp.C0).min() > 0 and not np.array_equal(E.bits(base), E.bits(E.canary_buffer(case, inp)))
            for v in FORMS:
                got = launch(eng, case, inp, v)
                diff = int((E.bits(got) != E.bits(base)).sum())
                assert diff == 0, f"{what}: variant {v} differs from the 128 tile in {diff} elements"
    print(f"{E.EPI_NAMES[epi]}: {len(SHAPES) * 2} argument sets x variants {FORMS} bit-identical to variant {BASE}; "
          f"worst |err| / bound {worst:.3f}")
