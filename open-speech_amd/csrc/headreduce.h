// reduce_head: the decoder projections' split-K slab reduction for one (row, head), shared by
// the cross-attention kernels (decode.hip) and the alignment score capture (align.hip), so
// both see the same q bits.  Included inside each file's anonymous namespace (as selfattn.h).
// Sum the split-K partial slabs of a decoder projection for one (row, 64-column
// head slice) and round to fp16 (the GEMM output precision the oracle emulates).
// 256 threads: wave w sums slabs s = w, w+4, ... (independent loads in flight), then
// lane d adds the 4 wave sums in fixed order (deterministic).
__device__ __forceinline__ void reduce_head(const float* __restrict__ part, int ks, int64_t slab, int64_t off,
                                            const float* __restrict__ bias, int col, h16* dst, float* red4) {
    const int d = threadIdx.x & 63, w = threadIdx.x >> 6;
    float v = 0.f;
    int s = w;
    for (; s + 4 < ks; s += 8) v += part[s * slab + off + d] + part[(s + 4) * slab + off + d];
    if (s < ks) v += part[s * slab + off + d];
    red4[w * 64 + d] = v;
    __syncthreads();
    if (w == 0) {
        float r = bias ? bias[col + d] : 0.f;
        r += red4[d] + red4[64 + d] + red4[128 + d] + red4[192 + d];
        dst[d] = (h16)r;
    }
    __syncthreads();
}
