// Decoder-side state and launchers shared by decode.hip (kernels) and the host pipeline.
#pragma once
#include "common.h"
#include "seltypes.h"

namespace osw {

// the row's prompt length and <|startoftranscript|> position
__host__ __device__ __forceinline__ int row_plen(const SelParams& P, const SelState& s) {
    return s.plen > 0 ? s.plen : P.prompt_len;
}

// Batch-1 greedy steps: the logits GEMM runs the token selection in its epilogue
// (gemm.hip, gemm_skinny_kernel<.., SEL>): every workgroup reduces its 64 columns to one
// slice record, the last to arrive merges them in workgroup order, finalises the row
// (select.h select_finalize) and advances the step counter -- no select launch.
struct SelFuse {
    SelParams P;
    const float* logits;  // this GEMM's output row (read back by the finaliser)
    int* pos;
    const unsigned* supmask;
    const int* prompt;
    SelState* st;
    int* cur_tok;
    int* tokens;
    int max_tokens;
    void* parts;   // one slice record per logits workgroup
    int* ticket;   // arrival counter (zero between launches)
};

constexpr int XPART = 72;     // floats per (decoder row, head, key chunk) cross-attention partial: m, l, pad, acc[64]
constexpr int XCHUNKS = 8;    // fixed key chunks per (window, head) in cross-attention

void launch_session_rows(const int* pack, int k, int ps, int group, int pstride, int ctx, int* prompt, int* budget,
                         int* cur_tok, int* pos, SelState* st, int* anc, BeamWin* bwin, hipStream_t s);
// Retry sessions (osw_session_retries): the rows of admitted or retried slots with their sampling
// state, pack stride ps = RETRY_PACK_HEAD + ctx (decode.hip session_retry_rows_kernel); and the two
// done-flag copies a greedy retry session's two cross-attention launches read
constexpr int RETRY_PACK_HEAD = 8;
void launch_session_retry_rows(const int* pack, int k, int ps, int group, int pstride, int ctx, int* prompt,
                               int* budget, int* cur_tok, int* pos, SelState* st, int* anc, BeamWin* bwin,
                               float* row_inv_temp, unsigned long long* row_seed, hipStream_t s);
void launch_retry_xmask(const SelState* st, const float* row_inv_temp, int group, int rows, SelState* single,
                        SelState* grouped, hipStream_t s);
void launch_refill_rows(const int* pack, int k, int P, int* prompt, int* budget, int* cur_tok, int* pos, SelState* st,
                        hipStream_t s);
void launch_select(const float* logits, int rows, int* pos, const SelParams& P, const int* prompt,
                   const unsigned* supmask, SelState* st, int* cur_tok, int* tokens, int max_tokens, void* sel_parts,
                   int* arrive, bool bump, void* cand, hipStream_t s);
// the last window's update advances *pos (arrive: a zeroed counter, left zeroed)
void launch_beam(const float* logits, int windows, int* pos, const SelParams& P, const unsigned* supmask,
                 SelState* st, const void* sel_parts, void* cand, int* seq, int* anc, int ctx, BeamWin* bw,
                 int* best_tok, int* cur_tok, int max_tokens, int* arrive, hipStream_t s);
// History rules (osw_decode_opts::repetition_penalty / no_repeat_ngram_size), in place on the raw
// logits [rows][P.V] before launch_select: one workgroup per decoder row, its history the
// n_sampled tokens of tokens[row * max_tokens ..] (<= 448).  A caller with both rules off does not
// launch it (history_rules_on, seltypes.h).
void launch_history_rules(float* logits, int rows, const int* pos, const SelParams& P, const SelState* st,
                          const int* tokens, int max_tokens, float penalty, int ngram, hipStream_t s);
int sel_parts_bytes();
int sel_fused_parts_bytes(int V);  // SelFuse::parts of the batch-1 logits GEMM (one record per 64 columns)
int beam_cand_bytes(int beam);
void launch_count_done(const SelState* st, int rows, int* out, hipStream_t s);

}  // namespace osw
