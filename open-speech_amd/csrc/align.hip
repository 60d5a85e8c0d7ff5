// Word-timestamp alignment kernels (openai-whisper find_alignment, as faster-whisper's
// WhisperModel.find_alignment / CTranslate2 Whisper::align run it): see align.h.
//
// The decoder's cross-attention is flash-decoding over key chunks and never materialises a
// probability, so a teacher-forced pass (osw.hip align()) captures the raw scaled scores of
// the alignment heads here; everything after that works on the captured tensor.  Every
// reduction below has a fixed order and no kernel mixes windows, so a window's result does
// not depend on what else is aligned in the same call.
#include "align.h"

#include <cmath>

namespace osw {

namespace {
constexpr int HD = 64;
#include "headreduce.h"

// block-wide max / sum of 256 threads in a fixed order (wave DPP tree, then waves 0..3)
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (layer heads x rows, key blocks of 256): q of (row, head) exactly as the
// cross-attention kernels form it (reduce_head: slabs + bias, rounded to fp16), dotted with
// the window's resident keys in fp32, times the exact 1/8.  wmap (osw_session_align): row b
// reads the keys of window wmap[b], one uniform load per workgroup; null = the identity.  Only
// the key address depends on it: the q slabs, the slot and the scores row keep b.
__global__ __launch_bounds__(256) void align_scores_kernel(const float* __restrict__ part, int ks,
                                                           const float* __restrict__ bias,
                                                           const h16* __restrict__ xk, int rows, int H, int T,
                                                           const int* __restrict__ lh, int n_lh, int n_heads,
                                                           const int* __restrict__ pos, const int* __restrict__ slot,
                                                           const int* __restrict__ len, float* __restrict__ scores,
                                                           int pstride, const int* __restrict__ wmap) {
    __shared__ h16 q16[HD];
    __shared__ float red4[256];
    __shared__ float qf[HD];
    const int b = blockIdx.x / n_lh, e = blockIdx.x % n_lh;
    const int sl = slot[b], p = pos[0];
    if (sl < 0 || p >= len[b]) return;  // (uniform over the workgroup)
    const int h = lh[2 * e], hi = lh[2 * e + 1];
    const int D = H * HD;
    reduce_head(part, ks, (int64_t)rows * D, (int64_t)b * D + h * HD, bias, h * HD, q16, red4);
    if (threadIdx.x < HD) qf[threadIdx.x] = (float)q16[threadIdx.x];
    __syncthreads();
    const int key = blockIdx.y * 256 + threadIdx.x;
    if (key >= T) return;
    const h16* kr = xk + (((int64_t)(wmap ? wmap[b] : b) * H + h) * T + key) * HD;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const h16x8 kv = *(const h16x8*)(kr + 8 * c);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf((float)kv[i], qf[8 * c + i], acc);
    }
    scores[(((int64_t)sl * n_heads + hi) * pstride + p) * T + key] = acc * 0.125f;
}

// grid H x rows: the forced pass's self-attention with q, k and v kept in fp32 (its own fp32
// K/V cache).  The decode path rounds all three to fp16 (q and the cache); at tiny dims that
// rounding alone moves a forced token's log-probability by 1.3e-3 from the fp32 reference
// (oracle/model.py with only "dec_qkv" rounded), past the 1e-3 the token probabilities are
// held to, so the alignment pass does not take it over.  Slabs are summed in index order.
__global__ __launch_bounds__(256) void align_self_attn_kernel(const float* __restrict__ part, int ks,
                                                              const float* __restrict__ bias,
                                                              float* __restrict__ kcache, float* __restrict__ vcache,
                                                              const int* __restrict__ pos_ptr, int H, int B, int ctx,
                                                              h16* __restrict__ out, int64_t lo_off,
                                                              const SelState* __restrict__ st) {
    __shared__ float q[HD], kcur[HD], vcur[HD], sc[512], red[4], pv[4][HD];
    const int b = blockIdx.x / H, h = blockIdx.x % H, tid = threadIdx.x;
    if (st[b].done) return;  // (uniform) a row that is not aligned, or whose sequence has ended
    const int p = min(pos_ptr[0], min(ctx, 512) - 1);
    const int D = H * HD;
    const int64_t slab = (int64_t)B * 3 * D, row = (int64_t)b * 3 * D;
    float* kc = kcache + ((int64_t)b * H + h) * ctx * HD;
    float* vc = vcache + ((int64_t)b * H + h) * ctx * HD;
    if (tid < 3 * HD) {
        const int which = tid >> 6, d = tid & 63;
        const int64_t off = row + which * D + h * HD + d;
        float v = bias[which * D + h * HD + d];
        for (int s = 0; s < ks; ++s) v += part[s * slab + off];
        if (which == 0) {
            q[d] = v;
        } else if (which == 1) {
            kcur[d] = v;
            kc[(int64_t)p * HD + d] = v;
        } else {
            vcur[d] = v;
            vc[(int64_t)p * HD + d] = v;
        }
    }
    __syncthreads();
    float m = -INFINITY;
    for (int key = tid; key <= p; key += 256) {
        const float* kr = kc + (int64_t)key * HD;
        float acc = 0.f;
        for (int d = 0; d < HD; ++d) acc = fmaf(key == p ? kcur[d] : kr[d], q[d], acc);
        acc *= 0.125f;
        sc[key] = acc;
        m = fmaxf(m, acc);
    }
    m = block_max(m, red);
    float l = 0.f;
    for (int key = tid; key <= p; key += 256) {
        const float e = expf(sc[key] - m);
        sc[key] = e;
        l += e;
    }
    l = block_sum(l, red);  // (its barriers publish sc)
    const int wv = tid >> 6, d = tid & 63;
    float o = 0.f;
    for (int key = wv; key <= p; key += 4) o = fmaf(sc[key], key == p ? vcur[d] : vc[(int64_t)key * HD + d], o);
    pv[wv][d] = o;
    __syncthreads();
    if (tid < HD) {
        const float r = (((pv[0][d] + pv[1][d]) + pv[2][d]) + pv[3][d]) / l;
        split_h16(r, out, out + lo_off, (int64_t)b * D + h * HD + d);
    }
}

// grid rows: log softmax(logits[:eot])[forced token] for the positions that predict a text
// token, then the row's next forced token (or its done flag)
__global__ __launch_bounds__(256) void align_tail_kernel(const float* __restrict__ logits, int V, int eot, int ctx,
                                                         const int* __restrict__ pos, const int* __restrict__ slot,
                                                         const int* __restrict__ len, const int* __restrict__ head,
                                                         const int* __restrict__ forced,
                                                         float* __restrict__ token_logprob, int* __restrict__ cur_tok,
                                                         SelState* __restrict__ st) {
    __shared__ float red[4];
    const int b = blockIdx.x, sl = slot[b], p = pos[0], L = len[b];
    if (sl < 0 || p >= L) return;
    const int hd = head[b];  // <|notimestamps|>'s position: 3, English-only 1
    if (p >= hd && p <= L - 3) {
        const float* lg = logits + (int64_t)b * V;
        const int tok = forced[(int64_t)b * ctx + p + 1];
        float m = -INFINITY;
        for (int i = threadIdx.x; i < eot; i += 256) m = fmaxf(m, lg[i]);
        m = block_max(m, red);
        float s = 0.f;
        for (int i = threadIdx.x; i < eot; i += 256) s += expf(lg[i] - m);
        s = block_sum(s, red);
        // the log-probability: a forced token may be far too unlikely for an fp32 probability
        if (threadIdx.x == 0) token_logprob[(int64_t)sl * ctx + p - hd] = (lg[tok] - m) - logf(s);
    }
    if (threadIdx.x == 0) {
        if (p + 1 < L) cur_tok[b] = forced[(int64_t)b * ctx + p + 1];
        else st[b].done = 1;
    }
}

__global__ void align_bump_kernel(int* pos) { *pos += 1; }

// grid slots x heads x pstride: max and sum of exp over the keys of one captured score row.
// The softmax runs over all TK keys of the context's window (50 per second of chunk_length)
// and the crop to F frames follows it (transformers /
// CTranslate2 order); cropping first (openai-whisper) is `nk = F` here.
__global__ __launch_bounds__(256) void align_softmax_stats_kernel(const float* __restrict__ scores, int n_heads,
                                                                  int pstride, int TK,
                                                                  const int* __restrict__ slot_len,
                                                                  float* __restrict__ stats) {
    __shared__ float red[4];
    const int p = blockIdx.x % pstride, sh = blockIdx.x / pstride, sl = sh / n_heads;
    if (p >= slot_len[sl]) return;
    const int nk = TK;
    const float* row = scores + (int64_t)blockIdx.x * TK;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nk; i += 256) m = fmaxf(m, row[i]);
    m = block_max(m, red);
    float s = 0.f;
    for (int i = threadIdx.x; i < nk; i += 256) s += expf(row[i] - m);
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        stats[2 * (int64_t)blockIdx.x] = m;
        stats[2 * (int64_t)blockIdx.x + 1] = s;
    }
}

__device__ __forceinline__ float align_prob(const float* __restrict__ scores, const float* __restrict__ stats,
                                            int64_t row, int f, int TK) {
    return expf(scores[row * TK + f] - stats[2 * row]) / stats[2 * row + 1];
}

// grid (frame blocks, heads, slots): mean and population standard deviation over all the
// forced positions of one (head, frame), positions in order
__global__ __launch_bounds__(256) void align_colstats_kernel(const float* __restrict__ scores,
                                                             const float* __restrict__ stats, int n_heads, int pstride,
                                                             int TK, const int* __restrict__ slot_len,
                                                             const int* __restrict__ slot_frames,
                                                             float* __restrict__ colstats) {
    const int f = blockIdx.x * 256 + threadIdx.x, hi = blockIdx.y, sl = blockIdx.z;
    const int P = slot_len[sl];
    if (P <= 0 || f >= slot_frames[sl]) return;
    const int64_t row0 = ((int64_t)sl * n_heads + hi) * pstride;
    float sum = 0.f;
    for (int p = 0; p < P; ++p) sum += align_prob(scores, stats, row0 + p, f, TK);
    const float mean = sum / (float)P;
    float var = 0.f;
    for (int p = 0; p < P; ++p) {
        const float d = align_prob(scores, stats, row0 + p, f, TK) - mean;
        var = fmaf(d, d, var);
    }
    const int64_t o = 2 * ((row0 / pstride) * TK + f);
    colstats[o] = mean;
    colstats[o + 1] = sqrtf(var / (float)P);
}

// median of the W normalised weights around frame f (reflect padding), W odd.  NaN (a zero-
// variance column gives 0/0) orders last, as torch.sort does in transformers' _median_filter:
// fminf / fmaxf would drop it, so a NaN enters the network as +inf and the result is NaN when
// the median's slot lies among the NaNs.
template <int WC>
__device__ __forceinline__ float align_median(const float* __restrict__ scores, const float* __restrict__ stats,
                                              const float* __restrict__ cs, int64_t row, int f, int F, int W,
                                              int TK) {
    constexpr int CAP = WC ? WC : ALIGN_MAX_WIDTH;
    const int w = WC ? WC : W, pad = w / 2;
    float v[CAP];
    int n_nan = 0;
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
        if (k >= w) {
            v[k] = INFINITY;  // sorts behind the w live values
            continue;
        }
        int g = f + k - pad;
        g = g < 0 ? -g : g;
        g = g >= F ? 2 * (F - 1) - g : g;
        const float z = (align_prob(scores, stats, row, g, TK) - cs[2 * g]) / cs[2 * g + 1];
        n_nan += z != z;
        v[k] = z != z ? INFINITY : z;
    }
    // full compare-exchange network (every pair, fixed loops: the array stays in registers)
#pragma unroll
    for (int a = 0; a < CAP; ++a)
#pragma unroll
        for (int b = 0; b + 1 < CAP - a; ++b) {
            const float lo = fminf(v[b], v[b + 1]), hi = fmaxf(v[b], v[b + 1]);
            v[b] = lo;
            v[b + 1] = hi;
        }
    float r = v[0];
#pragma unroll
    for (int k = 0; k < CAP; ++k)
        if (k == pad) r = v[k];
    return pad >= w - n_nan ? NAN : r;
}

// grid (frame blocks, T rows, slots): M[t][f] = mean over heads (list order) of the median-
// filtered normalised weight of forced position t + slot_head (<|notimestamps|>'s position)
__global__ __launch_bounds__(256) void align_matrix_kernel(const float* __restrict__ scores,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ colstats, int n_heads,
                                                           int pstride, int TK, const int* __restrict__ slot_len,
                                                           const int* __restrict__ slot_head,
                                                           const int* __restrict__ slot_frames,
                                                           const int* __restrict__ slot_width, float* __restrict__ M) {
    const int f = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y, sl = blockIdx.z;
    const int P = slot_len[sl], F = slot_frames[sl], W = slot_width[sl], hd = slot_head[sl];
    if (t >= P - hd - 1 || f >= F) return;
    const bool filter = F > W / 2;  // transformers' _median_filter leaves shorter inputs unchanged
    float acc = 0.f;
    for (int hi = 0; hi < n_heads; ++hi) {
        const int64_t sh = (int64_t)sl * n_heads + hi, row = sh * pstride + t + hd;
        const float* cs = colstats + 2 * sh * TK;
        float v;
        if (!filter) v = (align_prob(scores, stats, row, f, TK) - cs[2 * f]) / cs[2 * f + 1];
        else if (W == 7) v = align_median<7>(scores, stats, cs, row, f, F, W, TK);
        else v = align_median<0>(scores, stats, cs, row, f, F, W, TK);
        acc += v;
    }
    M[((int64_t)sl * pstride + t) * TK + f] = acc / (float)n_heads;
}

// One workgroup per window.  cost[i][j] = x[i-1][j-1] + min(cost[i-1][j-1], cost[i-1][j],
// cost[i][j-1]) runs as a wavefront over the anti-diagonals d = i + j: thread t owns rows
// t + 1 and t + 257 (T <= 511), the two previous diagonals stay in LDS indexed by row, and
// the move taken (0 diagonal, 1 up, 2 left; transformers' _dynamic_time_warping tie rule)
// goes to global memory as one byte per cell.  Each row's x values are read in order, the
// next one issued a diagonal ahead.  Lane 0 then walks the trace back from (T, F).
__global__ __launch_bounds__(256) void align_dtw_kernel(const float* __restrict__ X, int64_t xstride, int ldx, int neg,
                                                        const int* __restrict__ Ts, const int* __restrict__ Fs,
                                                        unsigned char* __restrict__ trace, int64_t tstride,
                                                        int* __restrict__ path, int pcap, int* __restrict__ path_len,
                                                        int* __restrict__ token_frame, int tf_stride) {
    __shared__ float dg[3][ALIGN_DTW_ROWS + 1];
    const int sl = blockIdx.x, T = Ts[sl], F = Fs[sl], tid = threadIdx.x;
    if (T <= 0 || F <= 0 || T > ALIGN_DTW_ROWS) {
        if (tid == 0) path_len[sl] = 0;
        return;
    }
    const float* x = X + (int64_t)sl * xstride;
    unsigned char* tr = trace + (int64_t)sl * tstride;
    const float sgn = neg ? -1.f : 1.f;
    float xn[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = tid + 1 + 256 * r;
        xn[r] = i <= T ? x[(int64_t)(i - 1) * ldx] : 0.f;  // column j = 1
    }
    for (int d = 2; d <= T + F; ++d) {
        const int cur = d % 3, p1 = (d + 2) % 3, p2 = (d + 1) % 3;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = tid + 1 + 256 * r, j = d - i;
            if (i > T || j < 1 || j > F) continue;
            const float xv = xn[r] * sgn;
            if (j < F) xn[r] = x[(int64_t)(i - 1) * ldx + j];  // next diagonal's cell of this row
            // borders: cost[0][0] = 0, every other cell of row 0 and column 0 is +inf
            const float c0 = i == 1 ? (j == 1 ? 0.f : INFINITY) : (j == 1 ? INFINITY : dg[p2][i - 1]);
            const float c1 = i == 1 ? INFINITY : dg[p1][i - 1];
            const float c2 = j == 1 ? INFINITY : dg[p1][i];
            float cmin;
            unsigned char t;
            if (c0 < c1 && c0 < c2) {
                cmin = c0;
                t = 0;
            } else if (c1 < c0 && c1 < c2) {
                cmin = c1;
                t = 1;
            } else {
                cmin = c2;
                t = 2;
            }
            dg[cur][i] = xv + cmin;
            tr[(int64_t)i * (F + 1) + j] = t;
        }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int i = T, j = F, k = 0;
        int* pt = path + (int64_t)sl * 2 * pcap;
        int* pf = pt + pcap;
        while ((i > 0 || j > 0) && k < pcap) {
            pt[pcap - 1 - k] = i - 1;
            pf[pcap - 1 - k] = j - 1;
            // the first path entry of a text index (forward order) is the last one met here
            if (i > 0 && i - 1 < tf_stride) token_frame[(int64_t)sl * tf_stride + i - 1] = j - 1;
            const int t = i == 0 ? 2 : j == 0 ? 1 : tr[(int64_t)i * (F + 1) + j];
            ++k;
            if (t == 0) {
                --i;
                --j;
            } else if (t == 1) {
                --i;
            } else {
                --j;
            }
        }
        path_len[sl] = k;
    }
}
}  // namespace

void launch_align_scores(const float* part, int ks, const float* bias, const h16* xk, int rows, int H, int T,
                         const int* layer_heads, int n_layer_heads, int n_heads, const int* pos, const int* slot,
                         const int* len, float* scores, int pstride, hipStream_t s, const int* wmap) {
    if (n_layer_heads <= 0) return;
    align_scores_kernel<<<dim3(n_layer_heads * rows, (T + 255) / 256), 256, 0, s>>>(
        part, ks, bias, xk, rows, H, T, layer_heads, n_layer_heads, n_heads, pos, slot, len, scores, pstride, wmap);
}

void launch_align_self_attn(const float* part, int ks, const float* bias, float* kc, float* vc, const int* pos, int B,
                            int H, int ctx, h16* out, int64_t lo_off, const SelState* st, hipStream_t s) {
    align_self_attn_kernel<<<H * B, 256, 0, s>>>(part, ks, bias, kc, vc, pos, H, B, ctx, out, lo_off, st);
}

void launch_align_tail(const float* logits, int rows, int V, int eot, int ctx, const int* pos, const int* slot,
                       const int* len, const int* head, const int* forced, float* token_logprob, int* cur_tok,
                       SelState* st, hipStream_t s) {
    align_tail_kernel<<<rows, 256, 0, s>>>(logits, V, eot, ctx, pos, slot, len, head, forced, token_logprob, cur_tok,
                                           st);
}

void launch_align_bump(int* pos, hipStream_t s) { align_bump_kernel<<<1, 1, 0, s>>>(pos); }

void launch_align_post(const float* scores, int n_slots, int n_heads, int pstride, int TK, const int* slot_len,
                       const int* slot_head, const int* slot_frames, const int* slot_width, float* stats, float* colstats, float* M,
                       hipStream_t s) {
    const int fb = (TK + 255) / 256;
    align_softmax_stats_kernel<<<n_slots * n_heads * pstride, 256, 0, s>>>(scores, n_heads, pstride, TK, slot_len, stats);
    align_colstats_kernel<<<dim3(fb, n_heads, n_slots), 256, 0, s>>>(scores, stats, n_heads, pstride, TK, slot_len,
                                                                      slot_frames, colstats);
    align_matrix_kernel<<<dim3(fb, pstride, n_slots), 256, 0, s>>>(scores, stats, colstats, n_heads, pstride, TK,
                                                                    slot_len, slot_head, slot_frames, slot_width, M);
}

void launch_align_dtw(const float* x, int64_t xstride, int ldx, int neg, int n_slots, const int* T, const int* F,
                      unsigned char* trace, int64_t tstride, int* path, int pcap, int* path_len, int* token_frame,
                      int tf_stride, hipStream_t s) {
    align_dtw_kernel<<<n_slots, 256, 0, s>>>(x, xstride, ldx, neg, T, F, trace, tstride, path, pcap, path_len,
                                             token_frame, tf_stride);
}

}  // namespace osw
