// The co-residency budget of the persistent 8-phase encoder GEMM, stated
// once.  Host and device code may include this; tests/test_kernel_resources_cpu.py reads the numbers
// from here and holds the compiled kernels to them.
//
// An encoder workgroup (gemm8p_kernel) is 8 waves, 2 per SIMD, one per CU.  A SIMD has 512 VGPRs per
// lane, allocated to a wave in units of 8, and a CU has 160 KiB of LDS.  With at most
// ENC_GEMM_MAX_VGPRS per encoder wave and its 128 KiB operand ring / epilogue image, every SIMD keeps
// 512 - 2 * 216 = 80 VGPRs and the CU 32 KiB of LDS, of which a workgroup of <= 30720 B starts at
// once and one of 32768 B does not (measured: tools/coresidency_probe.hip), for one wave per SIMD of ANOTHER lane's
// decoder kernel: the HBM-bound decoder work then overlaps the MFMA-bound encoder phase instead of
// waiting on the quarter of the chip the encoder grid leaves free.
#pragma once

namespace osw {

// most VGPRs (AGPRs included) of a production gemm8p_kernel<EPI, 0> form; 217 allocates 224 and
// leaves 64 per SIMD
constexpr int ENC_GEMM_MAX_VGPRS = 216;
// most allocated VGPRs (rounded up to 8) of a decoder kernel of the greedy 64-row step
constexpr int CORES_DEC_MAX_VGPRS = 80;
// most LDS bytes of a decoder workgroup of that step
constexpr int CORES_DEC_MAX_LDS = 30720;

static_assert(2 * ENC_GEMM_MAX_VGPRS + CORES_DEC_MAX_VGPRS <= 512, "two encoder waves and a decoder wave per SIMD");

}  // namespace osw
