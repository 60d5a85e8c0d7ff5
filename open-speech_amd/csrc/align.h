// Word-timestamp alignment (align.hip): cross-attention score capture during a
// teacher-forced decoder pass, the normalise / median-filter / head-mean pass that turns
// the captured scores into the alignment matrix M, the forced tokens' probabilities and
// dynamic time warping over -M.  The host pipeline is osw.hip's align().
#pragma once
#include "decode.h"

namespace osw {

constexpr int ALIGN_MAX_WIDTH = 15;  // widest median filter (odd); the default is 7
constexpr int ALIGN_DTW_ROWS = 511;  // DTW rows per window (T = text tokens + 1 <= n_text_ctx - 4)

// Armed on a context while osw_align_windows steps the decoder: decoder_step then
// launches the score capture after each cross-attention of a layer with alignment heads.
// Rows are the windows of the last encode call (one decoder row per window); slot[row] is
// the window's index in the align call (-1: not aligned), len[row] its forced length.
struct AlignCapture {
    float* scores = nullptr;        // [slot][head_idx][pstride][TK] raw scaled scores, fp32
    const int* slot = nullptr;      // [rows]
    const int* len = nullptr;       // [rows]
    const int* layer_heads = nullptr;  // {head, head_idx} pairs grouped by layer
    const int* layer_first = nullptr;  // host: [L + 1] offsets (in pairs) into layer_heads
    int n_heads = 0, pstride = 0;
    float *kc32 = nullptr, *vc32 = nullptr;  // the pass's own fp32 self-K/V cache, [L][rows][H][ctx][64]
};

void launch_align_scores(const float* part, int ks, const float* bias, const h16* xk, int rows, int H, int T,
                         const int* layer_heads, int n_layer_heads, int n_heads, const int* pos, const int* slot,
                         const int* len, float* scores, int pstride, hipStream_t s, const int* wmap = nullptr);
// the forced pass's self-attention in fp32 (kc / vc: this layer's fp32 cache, [rows][H][ctx][64])
void launch_align_self_attn(const float* part, int ks, const float* bias, float* kc, float* vc, const int* pos, int B,
                            int H, int ctx, h16* out, int64_t lo_off, const SelState* st, hipStream_t s);
// log token_prob of the forced token predicted at this position (positions head .. len - 3,
// head[row] = <|notimestamps|>'s position: 3, or 1 in an English-only model's forced sequence),
// the next forced token into cur_tok, and the row's done flag once its sequence ends
void launch_align_tail(const float* logits, int rows, int V, int eot, int ctx, const int* pos, const int* slot,
                       const int* len, const int* head, const int* forced, float* token_logprob, int* cur_tok,
                       SelState* st, hipStream_t s);
void launch_align_bump(int* pos, hipStream_t s);
// scores -> M [slot][T = len - slot_head - 1][TK-float rows, F used]; stats: 2 floats per (slot, head,
// position), colstats: 2 floats per (slot, head, frame)
void launch_align_post(const float* scores, int n_slots, int n_heads, int pstride, int TK, const int* slot_len,
                       const int* slot_head, const int* slot_frames, const int* slot_width, float* stats, float* colstats, float* M,
                       hipStream_t s);
// DTW over x (neg: over -x) of slot i: x + i * xstride, rows of ldx floats, T[i] x F[i] cells.
// trace: (T + 1)(F + 1) bytes per slot at i * tstride; path: [slot][2][pcap] ints, filled from
// the end (text then time indices), path_len[slot] entries; token_frame: [slot][tf_stride].
void launch_align_dtw(const float* x, int64_t xstride, int ldx, int neg, int n_slots, const int* T, const int* F,
                      unsigned char* trace, int64_t tstride, int* path, int pcap, int* path_len, int* token_frame,
                      int tf_stride, hipStream_t s);

}  // namespace osw
