"""The co-residency budget of csrc/coresidency.h, held at build time: gemm.hip and decode.hip are
compiled device-only for gfx950 with the Makefile's flags and the compiler's resource remarks
(tests/kernel_resources.py), and

  * each production form of the persistent 8-phase encoder GEMM, gemm8p_kernel<EPI, 0> for the four
    epilogues a 64-window encoder launches, has <= ENC_GEMM_MAX_VGPRS VGPRs, no VGPR or SGPR spill and
    2 waves per SIMD;
  * every decoder kernel of the greedy 64-row step fits in what that leaves on the CU: <=
    CORES_DEC_MAX_VGPRS allocated VGPRs (rounded up to the granule of 8) and <= CORES_DEC_MAX_LDS
    bytes of static LDS.

The one documented exception is the 64-row logits GEMM, gemm_wide_kernel<true, 256, ...>: its 128 KiB of
dynamic LDS cannot sit beside an encoder workgroup, so nothing is asserted on it.
Only VGPR, spill, occupancy and LDS numbers are read; no instruction is looked at.
"""
import functools
import os
import re

import pytest

import kernel_resources as KR

pytestmark = pytest.mark.skipif(not os.path.exists(KR.HIPCC), reason="no hipcc at /opt/rocm/bin")

EPI_FORMS = {1: "EPI_F16_GELU (fc1, conv1)", 5: "EPI_HEADS (qkv, cross-K/V)", 2: "EPI_F32_RESID (o, fc2)",
             3: "EPI_F32_GELU_POS (conv2)"}
# the greedy 64-row step's kernels, by demangled signature or (where the demangler gives up on
# the _Float16 parameters) by the mangled name
DECODER = {
    "dec_xattn_chunk_kernel<1, 6>": r"dec_xattn_chunk_kernel(<1, 6>|ILi1ELi6EE)",
    "dec_self_attn_kernel<0, 0, 0>": r"dec_self_attn_kernel(<false, false, false>|ILb0ELb0ELb0EE)",
    "dec_resid_ln_kernel": r"dec_resid_ln_kernel(\(|E)",
    "dec_reduce_gelu_kernel": r"dec_reduce_gelu_kernel(\(|E)",
    "select_kernel<0>": r"select_kernel(<0>|ILi0EE)",
    # MT 2 (33-64 rows), plain fp32 partials, hi/lo activations, no prologue, no tail; fp16 or int8 weights
    "gemm_skinny_kernel<2, ...> (64 rows)": r"gemm_skinny_kernel<2, (true|false), 4, true, 0, false, 0, [012]>",
}
EXCEPTION = r"gemm_wide_kernel<true, 256"


def budget():
    text = open(os.path.join(KR.CSRC, "coresidency.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", text)}


@functools.lru_cache(maxsize=None)
def resources(src):
    return KR.kernel_resources(src, demangled=True)


def both():
    d = dict(resources("decode.hip"))
    d.update(resources("gemm.hip"))
    return d


def test_budget_header():
    b = budget()
    assert b["ENC_GEMM_MAX_VGPRS"] == 216 and b["CORES_DEC_MAX_VGPRS"] == 80 and b["CORES_DEC_MAX_LDS"] == 30720
    assert 2 * KR.allocated_vgprs(b["ENC_GEMM_MAX_VGPRS"]) + b["CORES_DEC_MAX_VGPRS"] <= 512


def test_encoder_gemm_forms_within_budget():
    cap = budget()["ENC_GEMM_MAX_VGPRS"]
    res = resources("gemm.hip")
    bad = []
    for epi, what in EPI_FORMS.items():
        (name, r), = [(k, v) for k, v in res.items() if f"gemm8p_kernel<{epi}, 0>" in k]
        regs = r["vgprs"] + r.get("agprs", 0)
        print(f"gemm8p_kernel<{epi}, 0> {what}: {regs} VGPRs (allocates {KR.allocated_vgprs(regs)}), "
              f"spills {r['vgpr_spill']} VGPR / {r['sgpr_spill']} SGPR, {r['occupancy']} waves/SIMD")
        if regs > cap or r["vgpr_spill"] or r["sgpr_spill"] or r["occupancy"] != 2:
            bad.append(f"gemm8p_kernel<{epi}, 0> {what}: {regs} VGPRs (<= {cap}), spills {r['vgpr_spill']} VGPR / "
                       f"{r['sgpr_spill']} SGPR (0 / 0), {r['occupancy']} waves/SIMD (2)")
    assert not bad, "over the co-residency budget:\n  " + "\n  ".join(bad)


def test_decoder_step_kernels_fit_beside_an_encoder_workgroup():
    b = budget()
    res = both()
    bad = []
    for what, pat in DECODER.items():
        hits = {k: v for k, v in res.items() if re.search(pat, k)}
        assert hits, f"{what}: no such kernel in gemm.hip / decode.hip"
        for k, r in hits.items():
            alloc = KR.allocated_vgprs(r["vgprs"] + r.get("agprs", 0))
            print(f"{what}: {r['vgprs']} + {r.get('agprs', 0)} VGPRs (allocates {alloc}), {r['lds']} B of LDS")
            if alloc > b["CORES_DEC_MAX_VGPRS"] or r["lds"] > b["CORES_DEC_MAX_LDS"]:
                bad.append(f"{k[:100]}: allocates {alloc} VGPRs (<= {b['CORES_DEC_MAX_VGPRS']}), "
                           f"{r['lds']} B of LDS (<= {b['CORES_DEC_MAX_LDS']})")
    assert not bad, "does not fit beside an encoder workgroup:\n  " + "\n  ".join(bad)
    assert any(re.search(EXCEPTION, k) for k in res), "the documented exception (the 64-row logits GEMM) is gone"
