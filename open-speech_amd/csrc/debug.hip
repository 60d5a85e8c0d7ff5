// The osw_debug_* entry points: single kernels and launch forms on host data, for the parity
// tests and the probes.
#include "ctx.h"

extern "C" {

int osw_debug_dtw(osw_ctx* c, const float* x, int32_t T, int32_t F, int32_t* text_idx, int32_t* time_idx,
                  int32_t* len) {
    return guard([&] {
        REQUIRE(c && x && text_idx && time_idx && len, "null argument");
        REQUIRE(T >= 1 && T <= ALIGN_DTW_ROWS && F >= 1 && F <= 4096, "DTW shape out of range");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        std::vector<void*> tmp;
        const int pcap = T + F;
        float* xd = dalloc<float>((size_t)T * F, tmp);
        unsigned char* tr = dalloc<unsigned char>((size_t)(T + 1) * (F + 1), tmp);
        int* ib = dalloc<int>((size_t)3 + 2 * pcap + T, tmp);  // T, F, path_len, path, token_frame
        int hdr[3] = {T, F, 0};
        hipError_t e = hipMemcpyAsync(xd, x, (size_t)T * F * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ib, hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream);
        std::vector<int> back((size_t)3 + 2 * pcap);
        if (e == hipSuccess) {
            launch_align_dtw(xd, 0, F, 0, 1, ib, ib + 1, tr, 0, ib + 3, pcap, ib + 2, ib + 3 + 2 * pcap, T, c->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(back.data(), ib, back.size() * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        dfree(xd, tmp);
        dfree(tr, tmp);
        dfree(ib, tmp);
        HIPCHK(e);
        const int k = back[2];
        *len = k;
        for (int i = 0; i < k; ++i) {
            text_idx[i] = back[3 + pcap - k + i];
            time_idx[i] = back[3 + pcap + pcap - k + i];
        }
    });
}

int osw_debug_history_rules(osw_ctx* c, float* logits, int32_t rows, int32_t V, const int32_t* tokens, int32_t stride,
                            const int32_t* n_hist, float repetition_penalty, int32_t no_repeat_ngram_size) {
    return guard([&] {
        REQUIRE(c && logits && tokens && n_hist, "null argument");
        REQUIRE(rows >= 1 && rows <= 65535 && V >= 1 && stride >= 1, "history rules shape out of range");
        REQUIRE(stride <= c->d.n_text_ctx && stride <= 448, "history stride exceeds n_text_ctx");
        for (int r = 0; r < rows; ++r) {
            REQUIRE(n_hist[r] >= 0 && n_hist[r] <= stride, "history longer than its stride");
            for (int i = 0; i < n_hist[r]; ++i)
                REQUIRE(tokens[(size_t)r * stride + i] >= 0 && tokens[(size_t)r * stride + i] < V,
                        "history token outside the vocabulary");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        // every row samples at step 0 of a one-token prompt with n_hist[r] tokens behind it
        SelParams SP{};
        SP.prompt_len = 1;
        SP.V = V;
        std::vector<SelState> st(rows);
        for (int r = 0; r < rows; ++r) {
            st[r] = SelState{};
            st[r].n_sampled = n_hist[r];
        }
        std::vector<void*> tmp;
        float* xd = dalloc<float>((size_t)rows * V, tmp);
        int* td = dalloc<int>((size_t)rows * stride + 1, tmp);  // histories, then the step counter
        SelState* sd = dalloc<SelState>((size_t)rows, tmp);
        const int zero = 0;
        hipError_t e = hipMemcpyAsync(xd, logits, (size_t)rows * V * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(td, tokens, (size_t)rows * stride * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(td + (size_t)rows * stride, &zero, 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(sd, st.data(), (size_t)rows * sizeof(SelState), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && history_rules_on(repetition_penalty, no_repeat_ngram_size)) {
            launch_history_rules(xd, rows, td + (size_t)rows * stride, SP, sd, td, stride, repetition_penalty,
                                 no_repeat_ngram_size, c->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(logits, xd, (size_t)rows * V * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        dfree(xd, tmp);
        dfree(td, tmp);
        dfree(sd, tmp);
        HIPCHK(e);
    });
}

int osw_debug_history_rules_time(osw_ctx* c, int32_t rows, int32_t V, int32_t n_hist, float repetition_penalty,
                                 int32_t no_repeat_ngram_size, int32_t iters, float* us) {
    return guard([&] {
        REQUIRE(c && us, "null argument");
        REQUIRE(rows >= 1 && rows <= 65535 && V >= 4 && iters >= 1, "history rules shape out of range");
        REQUIRE(n_hist >= 0 && n_hist <= c->d.n_text_ctx && n_hist <= 448, "history longer than n_text_ctx");
        REQUIRE(history_rules_on(repetition_penalty, no_repeat_ngram_size), "both rules are off: nothing to time");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        const int stride = std::max(1, (int)n_hist);
        SelParams SP{};
        SP.prompt_len = 1;
        SP.V = V;
        std::vector<SelState> st(rows);
        for (auto& q : st) q = SelState{}, q.n_sampled = n_hist;
        std::vector<int> hist((size_t)rows * stride + 1, 0);  // period 3 (every thread's prefix matches), then the step counter
        for (int r = 0; r < rows; ++r)
            for (int i = 0; i < stride; ++i) hist[(size_t)r * stride + i] = 1 + i % 3;
        std::vector<void*> tmp;
        float* xd = dalloc<float>((size_t)rows * V, tmp);
        int* td = dalloc<int>(hist.size(), tmp);
        SelState* sd = dalloc<SelState>((size_t)rows, tmp);
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        try {
            HIPCHK(hipMemsetAsync(xd, 0, (size_t)rows * V * 4, c->stream));
            HIPCHK(hipMemcpyAsync(td, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(sd, st.data(), (size_t)rows * sizeof(SelState), hipMemcpyHostToDevice, c->stream));
            auto run = [&] {
                launch_history_rules(xd, rows, td + (size_t)rows * stride, SP, sd, td, stride, repetition_penalty,
                                     no_repeat_ngram_size, c->stream);
            };
            run();  // warm
            HIPCHK(hipEventRecord(e0, c->stream));
            for (int i = 0; i < iters; ++i) run();
            HIPCHK(hipEventRecord(e1, c->stream));
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventSynchronize(e1));
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, e0, e1));
            *us = t * 1e3f / iters;
        } catch (...) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            for (void* p : tmp) (void)hipFree(p);
            throw;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        for (void* p : tmp) (void)hipFree(p);
    });
}

// One selection step on host state (osw.h osw_debug_select_step): the plan the decode paths
// build, bound to the context's buffers, one plan_select.  Everything a kernel indexes with is
// checked here first; the row modes restate select.h sel_mode on the host.
// rows_per_slot > 0 (osw_debug_select_step_rows): the plan of a retry session with that many rows
// per slot and the rows' sampling state, so the launches are a retry session's.
static int select_step(osw_ctx* c, const osw_decode_opts* o, const osw_select_io* io, int rows_per_slot,
                       const float* row_inv_temp, const uint64_t* row_seed) {
    return guard([&] {
        static_assert(sizeof(SelState) == 40 && sizeof(BeamWin) == 24, "the word layouts osw.h documents");
        REQUIRE(c && o && io, "null argument");
        REQUIRE(io->mode >= OSW_SELECT_BATCH && io->mode <= OSW_SELECT_SESSION, "select step: unknown mode");
        const bool retry = rows_per_slot > 0;
        if (retry) {
            REQUIRE(io->mode == OSW_SELECT_SESSION, "select step: row temperatures belong to session mode");
            REQUIRE(row_inv_temp && row_seed, "select step: null row temperatures / seeds");
            REQUIRE(rows_per_slot <= 5 && rows_per_slot >= std::max(1, o->beam_size) && o->beam_size <= 5,
                    "select step: beam_size <= rows_per_slot <= 5");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        REQUIRE(!c->sess, "select step: a decode session is open");
        const osw_dims& d = c->d;
        const int V = d.n_vocab, ctx = d.n_text_ctx;
        const DecodeMode mode = io->mode == OSW_SELECT_BATCH    ? DecodeMode::Batch
                                : io->mode == OSW_SELECT_REFILL ? DecodeMode::Refill
                                                                : DecodeMode::Session;
        // the caller's prompts carry the prefix contents; the plan needs only their count
        osw_decode_opts oo = *o;
        oo.n_prefix = mode == DecodeMode::Batch ? io->n_prefix : 0;
        oo.prefix_tokens = io->prompt;
        oo.token_budget = io->budget;
        oo.language_tokens = nullptr;
        DecodePlan plan(mode, &oo, d, oo.n_prefix, 0, rows_per_slot);
        const SelParams& sp = plan.sp;
        const int rows = io->rows, group = plan.group, K = plan.beam, max_tok = plan.max_tok, pstride = sp.pstride;
        REQUIRE(rows >= 1 && rows % group == 0 && rows <= c->R, "select step: rows must be a multiple of the group, at most the row capacity");
        const int windows = rows / group;
        REQUIRE(windows <= c->B, "select step: more windows than max_batch");
        REQUIRE(io->max_tok == max_tok && io->pstride == pstride, "select step: max_tok / pstride are not the plan's");
        REQUIRE(K == 1 || ctx <= 448, "select step: beam rows hold at most 448 positions");
        REQUIRE(sp.eot >= 0 && sp.eot < V && sp.no_speech >= 0 && sp.no_speech < V && sp.tb >= 0 && sp.tb <= V,
                "select step: special token outside the vocabulary");
        REQUIRE(sp.first_lang >= 0 && sp.n_langs >= 0 && sp.first_lang + sp.n_langs <= V && sp.n_langs <= LANG_CAP &&
                    (plan.ss.english || sp.n_langs >= 1),
                "select step: language token range");
        const bool per_row = sp.pos_row != 0, beam = K > 1, conf = c->conf;
        const bool langp = conf && !plan.ss.english;
        const int64_t n_pos = per_row ? rows : 1;
        auto need = [&](const void* p, int64_t len, int64_t want, const char* what) {
            if (!(p && len >= want)) throw OswError(OSW_EINVAL, std::string("select step: undersized array: ") + what);
        };
        need(io->logits, io->logits_len, (int64_t)rows * V, "logits");
        need(io->pos, io->pos_len, n_pos, "pos");
        need(io->state, io->state_len, (int64_t)rows * 10, "state");
        need(io->prompt, io->prompt_len, (int64_t)rows * pstride, "prompt");
        need(io->cur_tok, io->cur_tok_len, rows, "cur_tok");
        need(io->tokens, io->tokens_len, (int64_t)rows * max_tok, "tokens");
        need(io->counters, io->counters_len, 1 + rows, "counters");
        if (io->budget) need(io->budget, io->budget_len, rows, "budget");
        if (beam) {
            need(io->anc, io->anc_len, (int64_t)rows * ctx, "anc");
            need(io->bwin, io->bwin_len, (int64_t)windows * 6, "bwin");
            need(io->best_tok, io->best_tok_len, (int64_t)windows * max_tok, "best_tok");
        }
        if (conf) need(io->lp_hist, io->lp_hist_len, (int64_t)rows * ctx, "lp_hist");
        if (conf && beam) need(io->best_lp, io->best_lp_len, (int64_t)windows * ctx, "best_lp");
        if (langp) need(io->lang_probs, io->lang_probs_len, (int64_t)windows * sp.n_langs, "lang_probs");
        const SelState* st = (const SelState*)io->state;
        for (int r = 0; r < rows; ++r) {
            const SelState& s = st[r];
            const int step = io->pos[per_row ? r : 0];
            if (retry) REQUIRE(std::isfinite(row_inv_temp[r]) && row_inv_temp[r] >= 0.f, "select step: bad row temperature");
            REQUIRE(step >= 0 && step < ctx, "select step: step counter outside [0, n_text_ctx)");
            if (mode == DecodeMode::Session)
                REQUIRE(s.plen >= sp.tail && s.plen < sp.max_length && s.plen <= pstride, "select step: plen out of range");
            else
                REQUIRE(s.plen == 0, "select step: plen is a session row's");
            const int pl = row_plen(sp, s), sot = pl - sp.tail;
            REQUIRE(s.n_sampled >= 0 && s.n_sampled <= max_tok, "select step: n_sampled outside [0, max_tok]");
            REQUIRE(s.lang >= 0 && s.lang < V, "select step: language outside the vocabulary");
            for (int i = 0; i < pl; ++i) {
                const int t = io->prompt[(size_t)r * pstride + i];
                REQUIRE((t >= 0 && t < V) || (t == -1 && !plan.ss.english && i == sot + 1),
                        "select step: prompt token outside the vocabulary");
            }
            for (int i = 0; i < s.n_sampled; ++i) {
                const int t = io->tokens[(size_t)r * max_tok + i];
                REQUIRE(t >= 0 && t < V, "select step: history token outside the vocabulary");
            }
            // (select.h sel_mode) a row past its prompt and not done samples
            if (step >= pl - 1 && !s.done)
                REQUIRE(step == pl - 1 + s.n_sampled, "select step: a sampling row's counter is not plen - 1 + n_sampled");
            if (!beam) continue;
            // (a retry session: the checks below hold for the first K rows of a temperature-0 slot)
            if (retry && (row_inv_temp[r - r % group] > 0.f || r % group >= K)) continue;
            const int r0 = r - r % group;
            const SelState& s0 = st[r0];
            REQUIRE(s.n_sampled == s0.n_sampled && s.plen == s0.plen && (s.done != 0) == (s0.done != 0) &&
                        step == io->pos[per_row ? r0 : 0],
                    "select step: rows of one beam window differ in n_sampled / plen / done / counter");
            for (int p = 0; p < step; ++p) {
                const int a = io->anc[(size_t)r * ctx + p];
                REQUIRE(a >= r0 && a < r0 + K, "select step: ancestry entry outside the window's rows");
            }
        }
        // the state up, one selection, everything back
        if (retry) retry_reserve(c);
        bind_plan(c, plan, &oo);
        auto up = [&](void* dst, const void* src, int64_t words) {
            HIPCHK(hipMemcpyAsync(dst, src, (size_t)words * 4, hipMemcpyHostToDevice, c->stream));
        };
        auto down = [&](void* dst, const void* src, int64_t words) {
            HIPCHK(hipMemcpyAsync(dst, src, (size_t)words * 4, hipMemcpyDeviceToHost, c->stream));
        };
        up(c->logits, io->logits, (int64_t)rows * V);
        up(c->pos, io->pos, n_pos);
        up(c->sel, io->state, (int64_t)rows * 10);
        up(c->prompt, io->prompt, (int64_t)rows * pstride);
        up(c->cur_tok, io->cur_tok, rows);
        up(c->tokens, io->tokens, (int64_t)rows * max_tok);
        if (io->budget) up(c->budget, io->budget, rows);
        else HIPCHK(hipMemsetAsync(c->budget, 0, (size_t)rows * 4, c->stream));
        if (beam) {
            up(c->anc, io->anc, (int64_t)rows * ctx);
            up(c->bwin, io->bwin, (int64_t)windows * 6);
            up(c->btok, io->best_tok, (int64_t)windows * max_tok);
        }
        if (conf) up(c->lp_hist, io->lp_hist, (int64_t)rows * ctx);
        if (conf && beam) up(c->best_lp, io->best_lp, (int64_t)windows * ctx);
        if (langp) up(c->lang_probs, io->lang_probs, (int64_t)windows * sp.n_langs);
        if (retry) {
            up(c->row_inv_temp, row_inv_temp, rows);
            up(c->row_seed, row_seed, (int64_t)rows * 2);
        }
        plan_select(c, plan, rows, windows);
        HIPCHK(hipGetLastError());
        if (plan.hr.on) down(io->logits, c->logits, (int64_t)rows * V);
        down(io->pos, c->pos, n_pos);
        down(io->state, c->sel, (int64_t)rows * 10);
        down(io->cur_tok, c->cur_tok, rows);
        down(io->tokens, c->tokens, (int64_t)rows * max_tok);
        if (beam) {
            down(io->anc, c->anc, (int64_t)rows * ctx);
            down(io->bwin, c->bwin, (int64_t)windows * 6);
            down(io->best_tok, c->btok, (int64_t)windows * max_tok);
        }
        if (conf) down(io->lp_hist, c->lp_hist, (int64_t)rows * ctx);
        if (conf && beam) down(io->best_lp, c->best_lp, (int64_t)windows * ctx);
        if (langp) down(io->lang_probs, c->lang_probs, (int64_t)windows * sp.n_langs);
        down(io->counters, c->sel_arrive, 1 + rows);
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_debug_select_step(osw_ctx* c, const osw_decode_opts* o, const osw_select_io* io) {
    return select_step(c, o, io, 0, nullptr, nullptr);
}

int osw_debug_select_step_rows(osw_ctx* c, const osw_decode_opts* o, const osw_select_io* io, int32_t rows_per_slot,
                               const float* row_inv_temp, const uint64_t* row_seed) {
    if (rows_per_slot < 1) return guard([] { REQUIRE(false, "select step: rows_per_slot must be >= 1"); });
    return select_step(c, o, io, rows_per_slot, row_inv_temp, row_seed);
}

int osw_encoder_layer_debug(osw_ctx* c, int32_t layer, const float* x, float* y, int32_t T) {
    return guard([&] {
        REQUIRE(c && x && y, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        REQUIRE(c->finalized, "weights not finalized");
        REQUIRE(T == c->T, "T must be the context's n_audio_ctx");
        REQUIRE(layer >= 0 && layer < c->d.n_audio_layer, "layer out of range");
        const int64_t n = (int64_t)T * c->d.n_audio_state;
        HIPCHK(hipMemcpyAsync(c->X, x, n * 4, hipMemcpyHostToDevice, c->stream));
        encoder_layer(c, layer, 1);
        HIPCHK(hipMemcpyAsync(y, c->X, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        resolve_events(c);
    });
}

int osw_debug_gemm(osw_ctx* c, int32_t M, int32_t N, int32_t K, int32_t variant, const void* A, const void* Wt,
                   float* C, int32_t iters, float* ms) {
    return guard([&] {
        REQUIRE(c && A && Wt && C && ms, "null argument");
        REQUIRE(M >= 1 && N >= 1 && K >= 64 && K % 64 == 0 && iters >= 1, "bad GEMM shape");
        REQUIRE(variant != 3 || (M <= 64 && K % 128 == 0), "skinny needs M <= 64 and K % 128 == 0");
        REQUIRE(variant < 8 || variant > 19 || variant == 11 || N % 8 == 0,
                "the 8-phase debug variants need N % 8 == 0 (their epilogues store 8-column chunks)");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        std::vector<void*> tmp;
        h16* dA = dalloc<h16>((size_t)M * K, tmp);
        h16* dW = dalloc<h16>((size_t)N * K, tmp);
        float* dC = dalloc<float>((size_t)M * N, tmp);
        float* dP = variant == 3 ? dalloc<float>((size_t)skinny_ksplit(N, K) * M * N, tmp) : nullptr;
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        try {
            HIPCHK(hipMemcpyAsync(dA, A, (size_t)M * K * 2, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dW, Wt, (size_t)N * K * 2, hipMemcpyHostToDevice, c->stream));
            GemmArgs g = gemm_plain(dA, K, dW, nullptr, M, N, K, dC, N, EPI_F32);
            auto run = [&] {
                if (variant == 3) launch_gemm_skinny(g, dP, c->stream);
                else launch_gemm_variant(g, variant, c->stream);
            };
            run();  // warm
            HIPCHK(hipEventRecord(e0, c->stream));
            for (int i = 0; i < iters; ++i) run();
            HIPCHK(hipEventRecord(e1, c->stream));
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventSynchronize(e1));
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, e0, e1));
            *ms = t / iters;
            HIPCHK(hipMemcpyAsync(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        } catch (...) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            for (void* p : tmp) (void)hipFree(p);
            throw;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        for (void* p : tmp) (void)hipFree(p);
    });
}

namespace {
// temporary device buffers of one debug call: freed when the call ends, however it ends
struct TmpBufs {
    std::vector<void*> v;
    ~TmpBufs() {
        GateLock gate_(capture_gate());
        for (void* p : v) (void)hipFree(p);
    }
};
}  // namespace

int osw_debug_enc_attn(osw_ctx* c, const void* qkv, int32_t nb, int32_t H, int32_t form, void* out) {
    return guard([&] {
        REQUIRE(c && qkv && out, "null argument");
        REQUIRE(nb >= 1 && nb <= 64 && H >= 1 && H <= 20, "encoder attention shape out of range");
        REQUIRE(form >= 0 && form < 16 && (form == 0 || (form & 1)), "form: 0 (auto) or 1 | 2 eager | 4 128-query | 8 pipelined");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t n = (size_t)nb * H * c->T * 64;
        h16* dq = dalloc<h16>(3 * n, tmp.v);
        h16* dout = dalloc<h16>(n, tmp.v);
        HIPCHK(hipMemcpyAsync(dq, qkv, 3 * n * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(dout, 0xff, n * 2, c->stream));  // NaN: an unwritten element shows
        if (form == 0) launch_enc_attn(dq, dout, c->T, H, nb, c->stream);
        else launch_enc_attn_form(dq, dout, c->T, H, nb, (form & 2) != 0, !(form & 4), (form & 8) != 0, 1 << 30, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, dout, n * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

namespace {
// one cross-attention launch on host data; window_map null: K / V hold one window per row group
// (kv_windows == rows / beam), else row group w attends window window_map[w] of kv_windows
int debug_dec_xattn(osw_ctx* c, const float* q_slabs, int32_t ks, const float* bias, const void* K, const void* V,
                    int32_t kv_windows, const int32_t* window_map, int32_t rows, int32_t beam, int32_t legacy,
                    float* out) {
    return guard([&] {
        REQUIRE(c && q_slabs && K && V && out, "null argument");
        REQUIRE(ks >= 1 && ks <= 32, "ks out of range");
        REQUIRE(beam >= 1 && beam <= MAX_BEAM && rows >= beam && rows % beam == 0, "rows must be windows x beam, beam <= 8");
        REQUIRE(legacy >= 0 && legacy <= 2, "legacy: 0 (chunk kernels), 1 (one workgroup per row and head), 2 (full chunk forms)");
        const bool full = legacy == 2;
        legacy = legacy == 1;
        const int H = c->d.n_text_head, D = c->d.n_text_state, W = rows / beam;
        REQUIRE(W <= c->B, "more windows than the context's max_batch (its arrival tickets)");
        if (window_map) {
            REQUIRE(kv_windows >= 1 && kv_windows <= c->B && W <= kv_windows, "window map: 1 <= row groups <= kv_windows <= max_batch");
            std::vector<char> seen((size_t)kv_windows, 0);
            for (int i = 0; i < W; ++i) {
                REQUIRE(window_map[i] >= 0 && window_map[i] < kv_windows, "window map: index outside K / V");
                REQUIRE(!seen[window_map[i]], "window map: a window appears twice");
                seen[window_map[i]] = 1;
            }
        } else {
            REQUIRE(kv_windows == W, "K / V hold one window per row group");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t nq = (size_t)ks * rows * D, nkv = (size_t)kv_windows * H * c->T * 64, no = (size_t)rows * D;
        float* dq = dalloc<float>(nq, tmp.v);
        float* db = dalloc<float>(D, tmp.v);
        // 64 NaN keys behind the last key of K and V: a load past a window's T keys shows
        const size_t canary = 64 * 64;
        h16* dk = dalloc<h16>(nkv + canary, tmp.v);
        h16* dv = dalloc<h16>(nkv + canary, tmp.v);
        HIPCHK(hipMemsetAsync(dk + nkv, 0xff, canary * 2, c->stream));
        HIPCHK(hipMemsetAsync(dv + nkv, 0xff, canary * 2, c->stream));
        h16* dout = dalloc<h16>(2 * no, tmp.v);  // hi, then lo
        int* dmap = nullptr;
        if (window_map) {
            dmap = dalloc<int>((size_t)W, tmp.v);
            HIPCHK(hipMemcpyAsync(dmap, window_map, (size_t)W * 4, hipMemcpyHostToDevice, c->stream));
        }
        float* ws = legacy ? nullptr : dalloc<float>((size_t)rows * H * XCHUNKS * XPART, tmp.v);
        SelState* st = dalloc<SelState>((size_t)rows, tmp.v);
        HIPCHK(hipMemcpyAsync(dq, q_slabs, nq * 4, hipMemcpyHostToDevice, c->stream));
        // the chunk kernels read the bias unconditionally: "none" is a zero bias for them
        if (bias) HIPCHK(hipMemcpyAsync(db, bias, (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemsetAsync(db, 0, (size_t)D * 4, c->stream));
        HIPCHK(hipMemcpyAsync(dk, K, nkv * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dv, V, nkv * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(dout, 0xff, 2 * no * 2, c->stream));
        HIPCHK(hipMemsetAsync(st, 0, (size_t)rows * sizeof(SelState), c->stream));
        launch_dec_cross_attn(dq, ks, (legacy && !bias) ? nullptr : db, dk, dv, rows, H, c->T, beam, dout, (int64_t)no, ws,
                              c->xticket, st, c->stream, dmap, full);
        hipError_t e = hipGetLastError();
        // the tickets are zero between launches (the last arriver resets its own); after a
        // failed launch they may not be, and the decode path shares them
        hipError_t e2 = hipMemsetAsync(c->xticket, 0, (size_t)W * H * sizeof(int), c->stream);
        HIPCHK(e);
        HIPCHK(e2);
        std::vector<h16> back(2 * no);
        HIPCHK(hipMemcpyAsync(back.data(), dout, 2 * no * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < no; ++i) out[i] = (float)back[i] + (float)back[no + i];
    });
}
}  // namespace

int osw_debug_dec_xattn(osw_ctx* c, const float* q_slabs, int32_t ks, const float* bias, const void* K, const void* V,
                        int32_t rows, int32_t beam, int32_t legacy, float* out) {
    return debug_dec_xattn(c, q_slabs, ks, bias, K, V, beam >= 1 ? rows / beam : 0, nullptr, rows, beam, legacy, out);
}

int osw_debug_dec_xattn_windows(osw_ctx* c, const float* q_slabs, int32_t ks, const float* bias, const void* K,
                                const void* V, int32_t kv_windows, const int32_t* window_map, int32_t rows, int32_t beam,
                                int32_t legacy, float* out) {
    if (!window_map) return guard([&] { REQUIRE(false, "null window map"); });
    return debug_dec_xattn(c, q_slabs, ks, bias, K, V, kv_windows, window_map, rows, beam, legacy, out);
}

int osw_debug_dec_self_attn(osw_ctx* c, const float* qkv_slabs, int32_t ks, const float* bias, void* kcache, void* vcache,
                            int32_t rows, const int32_t* pos, int32_t pos_per_row, const int32_t* ancestry,
                            int32_t group, float* out) {
    return guard([&] {
        REQUIRE(c && qkv_slabs && bias && kcache && vcache && pos && out, "null argument");
        REQUIRE(ks >= 1 && ks <= 32, "ks out of range");
        REQUIRE(rows >= 1 && rows <= 1024, "rows out of range");
        const int H = c->d.n_text_head, D = c->d.n_text_state, ctx = c->d.n_text_ctx;
        REQUIRE(ctx >= 1 && ctx <= 448, "n_text_ctx out of range");
        for (int r = 0; r < (pos_per_row ? rows : 1); ++r) REQUIRE(pos[r] >= 0 && pos[r] < ctx, "position outside the cache");
        if (ancestry) {
            REQUIRE(group >= 1 && group <= MAX_BEAM && rows % group == 0, "rows must be windows x group, group <= 8");
            for (size_t i = 0; i < (size_t)rows * ctx; ++i)
                REQUIRE(ancestry[i] >= 0 && ancestry[i] < rows, "ancestry names a row outside the cache");
        } else {
            REQUIRE(group == 1, "group needs an ancestry table");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t nq = (size_t)ks * rows * 3 * D, nkv = (size_t)rows * H * ctx * 64, no = (size_t)rows * D;
        float* dq = dalloc<float>(nq, tmp.v);
        float* db = dalloc<float>((size_t)3 * D, tmp.v);
        h16* dk = dalloc<h16>(nkv, tmp.v);
        h16* dv = dalloc<h16>(nkv, tmp.v);
        h16* dout = dalloc<h16>(2 * no, tmp.v);
        int* dpos = dalloc<int>((size_t)rows, tmp.v);
        int* danc = ancestry ? dalloc<int>((size_t)rows * ctx, tmp.v) : nullptr;
        SelState* st = dalloc<SelState>((size_t)rows, tmp.v);
        HIPCHK(hipMemcpyAsync(dq, qkv_slabs, nq * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(db, bias, (size_t)3 * D * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dk, kcache, nkv * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dv, vcache, nkv * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dpos, pos, (size_t)(pos_per_row ? rows : 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (danc) HIPCHK(hipMemcpyAsync(danc, ancestry, (size_t)rows * ctx * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(dout, 0xff, 2 * no * 2, c->stream));
        HIPCHK(hipMemsetAsync(st, 0, (size_t)rows * sizeof(SelState), c->stream));
        launch_dec_self_attn(dq, ks, db, dk, dv, dpos, rows, H, ctx, dout, (int64_t)no, danc, group, st, c->stream,
                             pos_per_row ? 1 : 0);
        HIPCHK(hipGetLastError());
        std::vector<h16> back(2 * no);
        HIPCHK(hipMemcpyAsync(back.data(), dout, 2 * no * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(kcache, dk, nkv * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(vcache, dv, nkv * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < no; ++i) out[i] = (float)back[i] + (float)back[no + i];
    });
}

namespace {
// what launch_gemm_skinny_partial / launch_gemm_skinny_pro and gemm_skinny_kernel rely on: whole
// 128-deep K ranges (the kernel's k32 steps come in fours, its chunk clamps assume kc >= 128)
void require_skinny_split(int K, int ks) {
    REQUIRE(K >= 128 && K % 128 == 0, "the skinny GEMM needs K a multiple of 128");
    REQUIRE(ks >= 1 && K % ks == 0 && (K / ks) % 128 == 0, "the skinny GEMM needs K / ksplit a multiple of 128");
}

// W[N][K] (host fp16) on the device, with its fragment-major copy when asked for
struct DebugW {
    h16* w = nullptr;
    h16* wf = nullptr;
};
void upload_w(osw_ctx* c, const void* W, int N, int K, bool use_wf, TmpBufs& tmp, DebugW& d) {
    d.w = dalloc<h16>((size_t)N * K, tmp.v);
    HIPCHK(hipMemcpyAsync(d.w, W, (size_t)N * K * 2, hipMemcpyHostToDevice, c->stream));
    if (use_wf) {
        d.wf = dalloc<h16>((size_t)((N + 15) / 16) * 16 * K, tmp.v);
        launch_frag_pack(d.w, K, N, K, d.wf, c->stream);
        HIPCHK(hipGetLastError());
    }
}

// the fp32 result buffer of a debug call: out_floats floats of 0xff bytes (a NaN pattern), so an
// element the kernel did not write, and a write past the `need` floats it owns, both show
float* result_buf(osw_ctx* c, int64_t out_floats, TmpBufs& tmp) {
    float* d = dalloc<float>((size_t)out_floats, tmp.v);
    HIPCHK(hipMemsetAsync(d, 0xff, (size_t)out_floats * 4, c->stream));
    return d;
}
}  // namespace

int osw_debug_dec_gemm(osw_ctx* c, int32_t form, int32_t M, int32_t N, int32_t K, const void* A_hi, const void* A_lo,
                       const void* W, int32_t use_wf, float* out, int64_t out_floats, int32_t* ks_out) {
    return guard([&] {
        REQUIRE(c && A_hi && W && out && ks_out, "null argument");
        REQUIRE(form >= 0 && form <= 2, "form: 0 skinny slabs, 1 tiled slabs, 2 logits route");
        REQUIRE(M >= 1 && M <= 1024 && N >= 1 && N <= 65536 && K >= 64 && K <= 8192, "GEMM shape out of range");
        REQUIRE(A_lo || M <= 64, "more than 64 rows need the lo operand (32-row groups)");
        int ks = 1;
        bool skinny = true;
        GemmArgs g = gemm_plain(nullptr, K, nullptr, nullptr, M, N, K, nullptr, N, EPI_F32);
        if (form == 0) {
            ks = skinny_ksplit(N, K);
            require_skinny_split(K, ks);
        } else if (form == 1) {
            REQUIRE(A_lo, "the tiled split-K GEMM serves hi/lo decoder rows");
            REQUIRE(K % 64 == 0 && N % 2 == 0, "the wide kernel needs K % 64 == 0 and an even N (8-byte stores)");
            ks = tiled_ksplit(M, N, K);
            REQUIRE(K % ks == 0 && (K / ks) % 64 == 0, "tiled split: K / ksplit a multiple of 64");
            skinny = false;
        } else {
            skinny = skinny_ok(g);  // run_gemm's test (shape and epilogue only)
            if (skinny) {
                ks = skinny_ksplit(N, K);
                require_skinny_split(K, ks);
            } else {
                REQUIRE(A_lo, "the logits route beyond the skinny kernel serves hi/lo rows");
                REQUIRE(K % 64 == 0 && N % 2 == 0, "the wide kernel needs K % 64 == 0 and an even N (8-byte stores)");
            }
        }
        const int64_t need = form == 2 ? (int64_t)M * N : (int64_t)ks * M * N;
        REQUIRE(out_floats >= need && out_floats <= ((int64_t)1 << 27), "out_floats: the result's floats plus a guard band");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t na = (size_t)M * K;  // lo sits R = M rows after hi, as xdn / dattn / dh hold the pair
        h16* dA = dalloc<h16>(2 * na, tmp.v);
        HIPCHK(hipMemcpyAsync(dA, A_hi, na * 2, hipMemcpyHostToDevice, c->stream));
        if (A_lo) HIPCHK(hipMemcpyAsync(dA + na, A_lo, na * 2, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemsetAsync(dA + na, 0, na * 2, c->stream));
        DebugW dw;
        upload_w(c, W, N, K, use_wf != 0, tmp, dw);
        float* dout = result_buf(c, out_floats, tmp);
        g.A = dA;
        g.A_lo = A_lo ? dA + na : nullptr;
        g.W = dw.w;
        g.Wf = dw.wf;
        if (form == 0) {
            const int got = launch_gemm_skinny_partial(g, dout, c->stream);
            REQUIRE(got == ks, "launch_gemm_skinny_partial chose another split");
        } else if (form == 1) {
            launch_gemm_tiled_partial(g, dout, ks, c->stream);
        } else {
            // decoder_step's logits GEMM: run_gemm's choice (with a workspace of this call's own)
            g.C = dout;
            g.share_cus = c->share_cus;
            if (skinny) {
                float* part = dalloc<float>((size_t)ks * M * N, tmp.v);
                launch_gemm_skinny(g, part, c->stream);
            } else {
                launch_gemm(g, c->stream);
            }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, dout, (size_t)out_floats * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *ks_out = ks;
    });
}

int osw_debug_dec_gemm_quant(osw_ctx* c, int32_t form, int32_t M, int32_t N, int32_t K, const void* A_hi, const void* A_lo,
                          const int8_t* q, const float* mult, int32_t use_q8_stream, float* out, int64_t out_floats,
                          int32_t* ks_out) {
    return guard([&] {
        REQUIRE(c && A_hi && A_lo && q && mult && out && ks_out, "null argument (int8 weights serve hi/lo rows)");
        REQUIRE(form >= 0 && form <= 4, "form: 0 skinny slabs, 1 tiled slabs, 2 logits route, 3 GELU tail, 4 attention tail");
        REQUIRE(M >= 1 && M <= 1024 && N >= 1 && N <= 65536 && K >= 64 && K <= 8192, "GEMM shape out of range");
        REQUIRE(K % 64 == 0, "int8 fragments need K a multiple of 64");
        for (int n = 0; n < N; ++n) REQUIRE(std::isfinite(mult[n]), "a multiplier is not finite");
        int ks = 1;
        bool skinny = true;
        GemmArgs g = gemm_plain(nullptr, K, nullptr, nullptr, M, N, K, nullptr, N, EPI_F32);
        if (form == 0 || form == 3 || form == 4) {
            ks = skinny_ksplit(N, K);
            require_skinny_split(K, ks);
        } else if (form == 1) {
            REQUIRE(N % 2 == 0, "the wide kernel needs an even N (8-byte stores)");
            ks = tiled_ksplit(M, N, K);
            REQUIRE(K % ks == 0 && (K / ks) % 64 == 0, "tiled split: K / ksplit a multiple of 64");
            skinny = false;
        } else {
            skinny = skinny_ok(g);  // run_gemm's test (shape and epilogue only)
            if (skinny) {
                ks = skinny_ksplit(N, K);
                require_skinny_split(K, ks);
            } else {
                REQUIRE(N % 2 == 0, "the wide kernel needs an even N (8-byte stores)");
            }
        }
        const int64_t need = form == 2 ? (int64_t)M * N : (int64_t)ks * M * N;
        REQUIRE(out_floats >= need && out_floats <= ((int64_t)1 << 27), "out_floats: the result's floats plus a guard band");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t na = (size_t)M * K, nw = (size_t)N * K;
        h16* dA = dalloc<h16>(2 * na, tmp.v);
        HIPCHK(hipMemcpyAsync(dA, A_hi, na * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dA + na, A_lo, na * 2, hipMemcpyHostToDevice, c->stream));
        // what osw_set_weight_quant leaves on the device: fp16(q) row-major (and its fragment copy when
        // that is the stream), the multipliers, the int8 fragments
        std::vector<h16> half(nw);
        for (size_t i = 0; i < nw; ++i) half[i] = (h16)(float)q[i];
        DebugW dw;
        upload_w(c, half.data(), N, K, !use_q8_stream, tmp, dw);
        float* dm = dalloc<float>((size_t)N, tmp.v);
        HIPCHK(hipMemcpyAsync(dm, mult, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        g.A = dA;
        g.A_lo = dA + na;
        g.W = dw.w;
        g.Wf = dw.wf;
        g.wscale = dm;
        if (use_q8_stream) {
            int8_t* dq = dalloc<int8_t>(nw, tmp.v);
            int8_t* dqf = dalloc<int8_t>((size_t)((N + 15) / 16) * 16 * K, tmp.v);
            HIPCHK(hipMemcpyAsync(dq, q, nw, hipMemcpyHostToDevice, c->stream));
            launch_frag_pack_q8(dq, N, K, dqf, c->stream);
            HIPCHK(hipGetLastError());
            g.Wq = dqf;
        }
        float* dout = result_buf(c, out_floats, tmp);
        HIPCHK(hipStreamSynchronize(c->stream));  // before `half` goes, and before a refusal below
        if (form == 0) {
            const int got = launch_gemm_skinny_partial(g, dout, c->stream);
            REQUIRE(got == ks, "launch_gemm_skinny_partial chose another split");
        } else if (form == 1) {
            launch_gemm_tiled_partial(g, dout, ks, c->stream);
        } else if (form == 2) {
            g.C = dout;
            g.share_cus = c->share_cus;
            if (skinny) {
                float* part = dalloc<float>((size_t)ks * M * N, tmp.v);
                launch_gemm_skinny(g, part, c->stream);
            } else {
                launch_gemm(g, c->stream);
            }
        } else if (form == 3) {  // the opt-in last-arriver tails: refused with int8 weights
            ProArgs pt{};
            launch_gemm_skinny_gelu_tail(g, dout, pt, c->stream);
        } else {
            ProArgs pa{};
            launch_gemm_skinny_pro(g, PRO_RESLN, pa, false, dout, c->stream, false, true);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, dout, (size_t)out_floats * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *ks_out = ks;
    });
}

int osw_debug_dec_gemm_time(osw_ctx* c, int32_t M, int32_t N, int32_t K, const void* A_hi, const void* A_lo,
                           const int8_t* q, const float* mult, int32_t copies, int32_t warm, int32_t launches,
                           float* us_f16, float* us_q8) {
    return guard([&] {
        REQUIRE(c && A_hi && A_lo && q && mult && us_f16 && us_q8, "null argument");
        REQUIRE(M >= 1 && M <= 64 && N >= 1 && N <= 65536 && K >= 128 && K <= 8192, "GEMM shape out of range");
        REQUIRE(copies >= 1 && copies <= 1024 && warm >= 0 && launches >= 1 && launches <= 100000, "counts out of range");
        const int ks = skinny_ksplit(N, K);
        require_skinny_split(K, ks);
        const size_t frag = (size_t)((N + 15) / 16) * 16 * K;   // elements of one fragment copy
        REQUIRE(frag * 3 * (size_t)copies <= ((size_t)8 << 30), "more than 8 GiB of weight copies");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t na = (size_t)M * K, nw = (size_t)N * K;
        h16* dA = dalloc<h16>(2 * na, tmp.v);
        HIPCHK(hipMemcpyAsync(dA, A_hi, na * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dA + na, A_lo, na * 2, hipMemcpyHostToDevice, c->stream));
        std::vector<h16> half(nw);
        for (size_t i = 0; i < nw; ++i) half[i] = (h16)(float)q[i];
        DebugW dw;
        upload_w(c, half.data(), N, K, true, tmp, dw);
        int8_t* dq = dalloc<int8_t>(nw, tmp.v);
        HIPCHK(hipMemcpyAsync(dq, q, nw, hipMemcpyHostToDevice, c->stream));
        float* dm = dalloc<float>((size_t)N, tmp.v);
        HIPCHK(hipMemcpyAsync(dm, mult, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        // `copies` replicas of each stream, walked round robin, so a launch finds its weights where a
        // decoder step does (183 MB of other weights were read since their last use), not in the L2
        h16* wf = dalloc<h16>(frag * copies, tmp.v);
        int8_t* wq = dalloc<int8_t>(frag * copies, tmp.v);
        launch_frag_pack_q8(dq, N, K, wq, c->stream);
        HIPCHK(hipGetLastError());
        for (int i = 0; i < copies; ++i) {
            HIPCHK(hipMemcpyAsync(wf + frag * i, dw.wf, frag * 2, hipMemcpyDeviceToDevice, c->stream));
            if (i) HIPCHK(hipMemcpyAsync(wq + frag * i, wq, frag, hipMemcpyDeviceToDevice, c->stream));
        }
        float* part = dalloc<float>((size_t)ks * M * N, tmp.v);
        HIPCHK(hipStreamSynchronize(c->stream));
        GemmArgs g = gemm_plain(dA, K, dw.w, nullptr, M, N, K, nullptr, N, EPI_F32);
        g.A_lo = dA + na;
        hipEvent_t ev[4];
        for (auto& e : ev) e = get_ev(c);
        auto run = [&](int i, bool q8, hipEvent_t a, hipEvent_t b) {
            GemmArgs h = g;
            if (q8) {
                h.Wq = wq + frag * (i % copies);
                h.wscale = dm;
            } else {
                h.Wf = wf + frag * (i % copies);
            }
            if (a) HIPCHK(hipEventRecord(a, c->stream));
            launch_gemm_skinny_partial(h, part, c->stream);
            if (b) HIPCHK(hipEventRecord(b, c->stream));
        };
        try {
            for (int i = 0; i < warm; ++i) {
                run(i, false, nullptr, nullptr);
                run(i, true, nullptr, nullptr);
            }
            for (int i = 0; i < launches; ++i) {   // float16 and int8 alternate, one event pair per launch
                run(warm + i, false, ev[0], ev[1]);
                run(warm + i, true, ev[2], ev[3]);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(c->stream));
                float a = 0.f, b = 0.f;
                HIPCHK(hipEventElapsedTime(&a, ev[0], ev[1]));
                HIPCHK(hipEventElapsedTime(&b, ev[2], ev[3]));
                us_f16[i] = 1e3f * a;
                us_q8[i] = 1e3f * b;
            }
        } catch (...) {
            for (auto e : ev) c->ev_free.push_back(e);
            throw;
        }
        for (auto e : ev) c->ev_free.push_back(e);
    });
}

int osw_debug_logits_profile(osw_ctx* c, double* ms, int64_t* launches) {
    return guard([&] {
        REQUIRE(c && ms && launches, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        resolve_events(c);
        *ms = c->logits_ms;
        *launches = c->logits_launches;
    });
}

int osw_debug_dec_resln(osw_ctx* c, int32_t fused, int32_t direct, int32_t rows, int32_t D, const float* slabs,
                        int32_t ks, const float* bias, float* x, const float* gain, const float* shift,
                        const void* tok_emb, const float* pos_emb, const int32_t* tok, const int32_t* pos, int32_t ctx,
                        int32_t V, int32_t pos_row, const void* W, int32_t N, int32_t use_wf, float* x_out, void* y_hi,
                        void* y_lo, float* out, int64_t out_floats, int32_t* ks_out) {
    return guard([&] {
        REQUIRE(c && x && gain && shift && x_out, "null argument");
        REQUIRE(rows >= 1 && rows <= 64, "rows out of range");
        REQUIRE(D >= 4 && D % 4 == 0 && D <= 1280, "LayerNorm width: a multiple of 4, at most 1280");
        const bool embed = slabs == nullptr;
        if (embed) {
            REQUIRE(tok_emb && pos_emb && tok && pos, "the embedding entry needs tok_emb, pos_emb, tok and pos");
            REQUIRE(V >= 1 && V <= 65536 && ctx >= 1 && ctx <= 448, "embedding tables out of range");
            // (a token id is clamped into [0, V) by the kernel; a position only from above)
            for (int r = 0; r < (pos_row ? rows : 1); ++r) REQUIRE(pos[r] >= 0, "negative position");
        } else {
            REQUIRE(ks >= 1 && ks <= 64, "ks out of range");
        }
        int gks = 1;
        int64_t need = 0;
        if (fused) {
            REQUIRE(W && out && ks_out, "null argument");
            REQUIRE(rows <= PRO_ROWS, "PRO_RESLN serves at most PRO_ROWS rows");
            REQUIRE(N >= 1 && N <= 65536, "N out of range");
            gks = direct ? 1 : skinny_ksplit(N, D);
            require_skinny_split(D, gks);
            need = (int64_t)gks * rows * N;
            REQUIRE(out_floats >= need && out_floats <= ((int64_t)1 << 27), "out_floats: the result's floats plus a guard band");
        } else {
            REQUIRE(y_hi && y_lo, "null argument");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t nx = (size_t)rows * D;
        float* dx = dalloc<float>(nx, tmp.v);
        float* dg = dalloc<float>(D, tmp.v);
        float* db = dalloc<float>(D, tmp.v);
        float* dbias = bias ? dalloc<float>(D, tmp.v) : nullptr;
        float* dpart = nullptr;
        h16* dte = nullptr;
        float* dpe = nullptr;
        int *dtok = nullptr, *dpos = nullptr;
        HIPCHK(hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dg, gain, (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(db, shift, (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        if (bias) HIPCHK(hipMemcpyAsync(dbias, bias, (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        if (embed) {
            dte = dalloc<h16>((size_t)V * D, tmp.v);
            dpe = dalloc<float>((size_t)ctx * D, tmp.v);
            dtok = dalloc<int>((size_t)rows, tmp.v);
            dpos = dalloc<int>((size_t)rows, tmp.v);
            HIPCHK(hipMemcpyAsync(dte, tok_emb, (size_t)V * D * 2, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dpe, pos_emb, (size_t)ctx * D * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dtok, tok, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dpos, pos, (size_t)(pos_row ? rows : 1) * 4, hipMemcpyHostToDevice, c->stream));
        } else {
            dpart = dalloc<float>((size_t)ks * nx, tmp.v);
            HIPCHK(hipMemcpyAsync(dpart, slabs, (size_t)ks * nx * 4, hipMemcpyHostToDevice, c->stream));
        }
        if (!fused) {
            h16* dy = dalloc<h16>(2 * nx, tmp.v);  // hi, then lo
            HIPCHK(hipMemsetAsync(dy, 0xff, 2 * nx * 2, c->stream));
            launch_dec_resid_ln(dpart, ks, rows, D, dbias, dx, dg, db, dy, (int64_t)nx, dte, dpe, dtok, dpos, ctx, V,
                                c->stream, pos_row ? 1 : 0);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(x_out, dx, nx * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(y_hi, dy, nx * 2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(y_lo, dy + nx, nx * 2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            return;
        }
        // the fused step's ping-pong: every workgroup reads x, one writes x' to the other buffer
        float* dx2 = dalloc<float>(nx, tmp.v);
        HIPCHK(hipMemsetAsync(dx2, 0xff, nx * 4, c->stream));
        DebugW dw;
        upload_w(c, W, N, D, use_wf != 0, tmp, dw);
        float* dout = result_buf(c, out_floats, tmp);
        GemmArgs g = gemm_plain(nullptr, D, dw.w, nullptr, rows, N, D, direct ? dout : nullptr, direct ? N : 0, EPI_F32);
        g.Wf = dw.wf;
        ProArgs pa{};
        pa.ln = ResLnArgs{dpart, ks, (int64_t)nx, dbias, dx, dx2, dg, db, dte, dpe, dtok, dpos, ctx, D, V, pos_row ? 1 : 0};
        const int got = launch_gemm_skinny_pro(g, PRO_RESLN, pa, direct != 0, direct ? nullptr : dout, c->stream);
        HIPCHK(hipGetLastError());
        REQUIRE(got == gks, "launch_gemm_skinny_pro chose another split");
        HIPCHK(hipMemcpyAsync(x_out, dx2, nx * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(x, dx, nx * 4, hipMemcpyDeviceToHost, c->stream));  // must come back unchanged
        HIPCHK(hipMemcpyAsync(out, dout, (size_t)out_floats * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *ks_out = gks;
    });
}

int osw_debug_dec_gelu(osw_ctx* c, int32_t fused, int32_t M, int32_t K4, const float* slabs, int32_t ks,
                       const float* bias, const void* W, int32_t N, int32_t use_wf, void* y_hi, void* y_lo, float* out,
                       int64_t out_floats, int32_t* ks_out) {
    return guard([&] {
        REQUIRE(c && slabs && bias, "null argument");
        REQUIRE(M >= 1 && M <= 1024 && K4 >= 1 && K4 <= 8192, "shape out of range");
        REQUIRE(ks >= 1 && ks <= 64, "ks out of range");
        int gks = 1;
        int64_t need = 0;
        if (fused) {
            REQUIRE(W && out && ks_out, "null argument");
            REQUIRE(N >= 1 && N <= 65536, "N out of range");
            REQUIRE(M <= GELU_ROWS, "PRO_GELU serves at most GELU_ROWS rows");
            REQUIRE(K4 >= 128 && K4 % 128 == 0, "the skinny GEMM needs K a multiple of 128");
            gks = skinny_ksplit(N, K4);
            require_skinny_split(K4, gks);
            REQUIRE(K4 / gks <= GELU_KC, "PRO_GELU: a workgroup's K range is at most GELU_KC deep");
            need = (int64_t)gks * M * N;
            REQUIRE(out_floats >= need && out_floats <= ((int64_t)1 << 27), "out_floats: the result's floats plus a guard band");
        } else {
            REQUIRE(y_hi && y_lo, "null argument");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t n = (size_t)M * K4;
        float* dpart = dalloc<float>((size_t)ks * n, tmp.v);
        float* dbias = dalloc<float>(K4, tmp.v);
        HIPCHK(hipMemcpyAsync(dpart, slabs, (size_t)ks * n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dbias, bias, (size_t)K4 * 4, hipMemcpyHostToDevice, c->stream));
        if (!fused) {
            h16* dy = dalloc<h16>(2 * n, tmp.v);  // hi, then lo
            HIPCHK(hipMemsetAsync(dy, 0xff, 2 * n * 2, c->stream));
            launch_dec_reduce_gelu(dpart, ks, M, K4, dbias, dy, (int64_t)n, c->stream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(y_hi, dy, n * 2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(y_lo, dy + n, n * 2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            return;
        }
        DebugW dw;
        upload_w(c, W, N, K4, use_wf != 0, tmp, dw);
        float* dout = result_buf(c, out_floats, tmp);
        GemmArgs g = gemm_plain(nullptr, K4, dw.w, nullptr, M, N, K4, nullptr, 0, EPI_F32);
        g.Wf = dw.wf;
        ProArgs pg{};
        pg.part = dpart;
        pg.ks = ks;
        pg.bias = dbias;
        const int got = launch_gemm_skinny_pro(g, PRO_GELU, pg, false, dout, c->stream);
        HIPCHK(hipGetLastError());
        REQUIRE(got == gks, "launch_gemm_skinny_pro chose another split");
        HIPCHK(hipMemcpyAsync(out, dout, (size_t)out_floats * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *ks_out = gks;
    });
}

namespace {
// one past the farthest element that rows 0 .. M-1 of a grouped layout touch, each row `width`
// elements wide (row m at (m / grp_rows) * grp_stride + (m % grp_rows) * ld): the last row of
// every group is a candidate (a short last group may end before the one in front of it)
int64_t grouped_extent(int64_t M, int64_t grp_rows, int64_t grp_stride, int64_t ld, int64_t width) {
    int64_t end = 0;
    for (int64_t q = 0; q * grp_rows < M; ++q) {
        const int64_t rows = std::min(grp_rows, M - q * grp_rows);
        end = std::max(end, q * grp_stride + (rows - 1) * ld + width);
    }
    return end;
}
}  // namespace

int osw_debug_enc_gemm(osw_ctx* c, const osw_enc_gemm_desc* d) {
    return guard([&] {
        REQUIRE(c && d && d->A && d->W && d->C, "null argument");
        const int M = d->M, N = d->N, K = d->K, epi = d->epi, variant = d->variant;
        REQUIRE(M >= 1 && M <= 65536 && N >= 1 && N <= 8192 && K >= 64 && K <= 8192, "GEMM shape out of range");
        REQUIRE(K % 64 == 0, "GEMM K must be a multiple of 64");
        REQUIRE(epi >= EPI_F16 && epi <= EPI_HEADS, "epi: one of the six OSW_EPI_* epilogues");
        REQUIRE(variant == 0 || variant == 1 || variant == 2 || variant == 4 || variant == 6 || variant == 7 ||
                    variant == 11 || variant == 16 || variant == 20 || variant == 21,
                "variant: 0 (chooser), 1, 2, 4, 6, 7, 11, 16, 20 or 21");
        REQUIRE((variant != 20 && variant != 21) || N % 8 == 0, "the 8-phase debug variants need N % 8 == 0");
        // A: 16-B pieces (global_load_lds), every row's K elements inside the buffer
        REQUIRE(d->lda >= 0 && d->lda <= ((int64_t)1 << 24) && d->lda % 8 == 0, "lda: a multiple of 8 elements (16 B)");
        REQUIRE(d->a_grp_rows >= 1 && d->a_grp_rows <= M, "a_grp_rows out of range");
        REQUIRE(d->a_grp_stride >= 0 && d->a_grp_stride <= ((int64_t)1 << 31) && d->a_grp_stride % 8 == 0,
                "a_grp_stride: a multiple of 8 elements (16 B)");
        REQUIRE(d->a_count >= 1 && d->a_count <= ((int64_t)1 << 28), "a_count out of range");
        REQUIRE(grouped_extent(M, d->a_grp_rows, d->a_grp_stride, d->lda, K) <= d->a_count,
                "an A row reads past the A buffer");
        // C
        const bool heads = epi == EPI_HEADS;
        const bool f32 = epi == EPI_F32_RESID || epi == EPI_F32_GELU_POS || epi == EPI_F32;
        const int64_t esz = f32 ? 4 : 2;
        REQUIRE(d->c_bytes >= esz && d->c_bytes <= ((int64_t)1 << 30) && d->c_bytes % esz == 0, "c_bytes out of range");
        const int64_t c_count = d->c_bytes / esz;
        REQUIRE(d->c_offset >= 0 && d->c_offset < c_count, "c_offset outside the C buffer");
        REQUIRE(d->ldc >= 0 && d->ldc <= ((int64_t)1 << 24), "ldc out of range");
        REQUIRE(d->c_grp_rows >= 1 && d->c_grp_rows <= M, "c_grp_rows out of range");
        REQUIRE(d->c_grp_stride >= 0 && d->c_grp_stride <= ((int64_t)1 << 31), "c_grp_stride out of range");
        if (f32) {
            // f32x4 accesses of the staged fp32 epilogues (bias, residual, positional rows, stores);
            // the plain fp32 store too, which the 256-row tiles stage the same way
            REQUIRE(N % 4 == 0 && d->ldc % 4 == 0 && d->c_grp_stride % 4 == 0 && d->c_offset % 4 == 0,
                    "fp32 epilogues need N, ldc, the C group stride and the C offset to be multiples of 4 (16-B rows)");
            // the two fused fp32 epilogues as run_gemm serves them (the chooser's kernel depends on it)
            REQUIRE(epi == EPI_F32 || (N % 8 == 0 && d->ldc % 8 == 0 && d->c_grp_stride % 8 == 0),
                    "GEMM epilogue needs N, ldc and the C group stride to be multiples of 8");
        } else {
            // run_gemm's rule: 16-B chunks, only each chunk's first column is tested against N
            REQUIRE(N % 8 == 0 && d->c_offset % 8 == 0 && (heads || (d->ldc % 8 == 0 && d->c_grp_stride % 8 == 0)),
                    "GEMM epilogue needs N, ldc, the C group stride and the C offset to be multiples of 8");
        }
        int nwin = 0;
        if (heads) {
            REQUIRE(d->heads_T >= 1 && d->heads_H >= 1 && d->heads_H <= 64 && d->heads_nb >= 1 && d->heads_nb <= 1024,
                    "head-major geometry out of range");
            REQUIRE(N % (64 * d->heads_H) == 0, "EPI_HEADS needs N a multiple of 64 * heads_H");
            REQUIRE(M % d->heads_T == 0, "EPI_HEADS needs M = windows * heads_T");
            nwin = M / d->heads_T;
            if (d->heads_slot) {
                std::vector<char> seen(d->heads_nb, 0);
                for (int i = 0; i < nwin; ++i) {
                    const int sl = d->heads_slot[i];
                    REQUIRE(sl >= 0 && sl < d->heads_nb && !seen[sl], "heads_slot: distinct slots < heads_nb");
                    seen[sl] = 1;
                }
            } else {
                REQUIRE(nwin <= d->heads_nb, "more windows than heads_nb");
            }
            const int64_t extent = (int64_t)(N / (64 * d->heads_H)) * d->heads_nb * d->heads_H * d->heads_T * 64;
            REQUIRE(d->c_offset + extent <= c_count, "the head-major output does not fit the C buffer");
        } else {
            // rows and groups do not overlap in C (in-bounds stores that race; EPI_F32_RESID reads them too)
            REQUIRE(d->ldc >= N || M == 1, "ldc shorter than a row");
            REQUIRE(M <= d->c_grp_rows || d->c_grp_stride >= d->c_grp_rows * d->ldc, "C groups overlap");
            REQUIRE(d->c_offset + grouped_extent(M, d->c_grp_rows, d->c_grp_stride, d->ldc, N) <= c_count,
                    "a C row ends past the C buffer");
        }
        if (epi == EPI_F32_GELU_POS)
            REQUIRE(d->pos && d->pos_count == d->c_grp_rows * (int64_t)N, "EPI_F32_GELU_POS needs pos [c_grp_rows][N]");
        // an explicit variant must run the kernel it names (launch_gemm_variant falls through otherwise)
        if (variant == 11)
            REQUIRE(N % 8 == 0 && (heads || d->ldc % 8 == 0) && d->c_grp_stride % 8 == 0,
                    "the 128 ring needs N, ldc and the C group stride to be multiples of 8");
        if (variant == 16) REQUIRE(N % 8 == 0, "the half-width tile needs N % 8 == 0");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        h16* dA = dalloc<h16>((size_t)d->a_count, tmp.v);
        h16* dW = dalloc<h16>((size_t)N * K, tmp.v);
        char* dC = dalloc<char>((size_t)d->c_bytes, tmp.v);
        float* dbias = d->bias ? dalloc<float>((size_t)N, tmp.v) : nullptr;
        float* dpos = epi == EPI_F32_GELU_POS ? dalloc<float>((size_t)d->pos_count, tmp.v) : nullptr;
        int* dslot = heads && d->heads_slot ? dalloc<int>((size_t)nwin, tmp.v) : nullptr;
        HIPCHK(hipMemcpyAsync(dA, d->A, (size_t)d->a_count * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dW, d->W, (size_t)N * K * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dC, d->C, (size_t)d->c_bytes, hipMemcpyHostToDevice, c->stream));
        if (dbias) HIPCHK(hipMemcpyAsync(dbias, d->bias, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        if (dpos) HIPCHK(hipMemcpyAsync(dpos, d->pos, (size_t)d->pos_count * 4, hipMemcpyHostToDevice, c->stream));
        if (dslot) HIPCHK(hipMemcpyAsync(dslot, d->heads_slot, (size_t)nwin * 4, hipMemcpyHostToDevice, c->stream));
        GemmArgs g{};
        g.A = dA; g.lda = d->lda; g.a_grp_rows = d->a_grp_rows; g.a_grp_stride = d->a_grp_stride;
        g.W = dW; g.ldw = K; g.bias = dbias; g.M = M; g.N = N; g.K = K;
        g.C = dC + d->c_offset * esz; g.ldc = d->ldc; g.c_grp_rows = d->c_grp_rows; g.c_grp_stride = d->c_grp_stride;
        g.pos = dpos; g.epi = epi;
        g.heads_T = d->heads_T; g.heads_H = d->heads_H; g.heads_nb = d->heads_nb; g.heads_slot = dslot;
        g.share_cus = c->share_cus;
        launch_gemm_variant(g, variant, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(d->C, dC, (size_t)d->c_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_debug_enc_layernorm(osw_ctx* c, int32_t M, int32_t M_alloc, int32_t D, const float* x, const float* gain,
                            const float* shift, void* y) {
    return guard([&] {
        REQUIRE(c && x && gain && shift && y, "null argument");
        REQUIRE(M >= 1 && M <= M_alloc && M_alloc <= 65536, "rows: 1 <= M <= M_alloc <= 65536");
        REQUIRE(layernorm_width_ok(D), "no LayerNorm kernel for this width");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        float* dx = dalloc<float>((size_t)M * D, tmp.v);
        float* dg = dalloc<float>((size_t)D, tmp.v);
        float* db = dalloc<float>((size_t)D, tmp.v);
        h16* dy = dalloc<h16>((size_t)M_alloc * D, tmp.v);
        HIPCHK(hipMemcpyAsync(dx, x, (size_t)M * D * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dg, gain, (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(db, shift, (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dy, y, (size_t)M_alloc * D * 2, hipMemcpyHostToDevice, c->stream));
        launch_layernorm(dx, M, D, dg, db, dy, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(y, dy, (size_t)M_alloc * D * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_debug_get_logmel(osw_ctx* c, int32_t clip, float* out, int64_t out_floats, float* clip_max) {
    return guard([&] {
        REQUIRE(c && out && clip_max, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        REQUIRE(clip >= 0 && clip < c->n_clips, "clip out of range");
        const int64_t n = (int64_t)c->nframes[clip] * c->d.n_mels;
        REQUIRE(out_floats >= n, "output buffer too small");
        int32_t ordered = 0;
        HIPCHK(hipMemcpyAsync(out, c->logmel + c->mel_off[clip], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&ordered, c->clip_max + clip, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        // float_to_ordered's inverse (common.h), on the host
        const int32_t bits = ordered >= 0 ? ordered : (ordered ^ 0x7fffffff);
        std::memcpy(clip_max, &bits, 4);
    });
}

int osw_debug_mel_windows(osw_ctx* c, const osw_window* windows, int32_t n, void* out_halfs, int64_t out_count) {
    return guard([&] {
        REQUIRE(c && windows && out_halfs, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        REQUIRE(!c->sess, "a decode session is open on this context (osw_session_end first)");
        REQUIRE(n >= 1 && n <= c->B, "window count out of range");
        const int64_t need = (int64_t)n * (c->NF + 2) * c->C1;
        REQUIRE(out_count >= need, "output buffer too small");
        const std::vector<int> hw = pack_windows(c, windows, n);  // a refused window: no launch
        HIPCHK(hipMemcpyAsync(c->win, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, c->stream));
        launch_mel_window(c->logmel, c->mel_off_d, c->nframes_d, c->clip_max, c->win, c->win + n, c->win + 2 * n, n,
                          c->d.n_mels, c->C1, c->NF, c->X1, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out_halfs, c->X1, (size_t)need * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

// ---- the word-timestamp alignment kernels, one production launcher per call (osw.h) ----
namespace {
extern "C++" {
template <typename T>
T* upload(osw_ctx* c, const T* src, size_t n, TmpBufs& tmp) {
    T* d = dalloc<T>(n, tmp.v);
    HIPCHK(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return d;
}
}

// rows' slots: -1 (not aligned) or distinct indices below n_slots (two rows of one slot would race)
void require_slots(const int32_t* slot, int rows, int n_slots) {
    std::vector<char> seen((size_t)n_slots, 0);
    for (int r = 0; r < rows; ++r) {
        REQUIRE(slot[r] >= -1 && slot[r] < n_slots, "slot outside [-1, n_slots)");
        if (slot[r] < 0) continue;
        REQUIRE(!seen[slot[r]], "a slot appears twice");
        seen[slot[r]] = 1;
    }
}
}  // namespace

int osw_debug_align_post(osw_ctx* c, const float* scores, int32_t n_slots, int32_t n_heads, int32_t pstride, int32_t TK,
                         const int32_t* len, const int32_t* head, const int32_t* frames, const int32_t* width,
                         float* stats, float* colstats, float* M) {
    return guard([&] {
        REQUIRE(c && scores && len && head && frames && width && stats && colstats && M, "null argument");
        REQUIRE(n_slots >= 1 && n_slots <= 64 && n_heads >= 1 && n_heads <= 64, "slots / heads out of range");
        REQUIRE(pstride >= 16 && pstride % 16 == 0 && pstride <= 448, "pstride: a multiple of 16, at most 448");
        REQUIRE(TK >= 1 && TK <= 4096, "TK out of range");
        for (int s = 0; s < n_slots; ++s) {
            REQUIRE(head[s] == 1 || head[s] == 3, "head: 1 or 3");
            REQUIRE(len[s] <= pstride && len[s] >= head[s] + 2, "len outside [head + 2, pstride]");
            REQUIRE(frames[s] >= 1 && frames[s] <= TK, "frames outside [1, TK]");
            REQUIRE(width[s] >= 1 && width[s] % 2 == 1 && width[s] <= ALIGN_MAX_WIDTH, "width: odd, at most 15");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const size_t rows = (size_t)n_slots * n_heads * pstride;
        const size_t ns = rows * TK, nst = rows * 2, ncs = (size_t)n_slots * n_heads * TK * 2;
        const size_t nm = (size_t)n_slots * pstride * TK;
        float* ds = upload(c, scores, ns, tmp);
        std::vector<int> meta((size_t)4 * n_slots);  // len, head, frames, width
        for (int s = 0; s < n_slots; ++s) {
            meta[s] = len[s];
            meta[n_slots + s] = head[s];
            meta[2 * n_slots + s] = frames[s];
            meta[3 * n_slots + s] = width[s];
        }
        int* dm = upload(c, meta.data(), meta.size(), tmp);
        float* dst = result_buf(c, (int64_t)nst, tmp);
        float* dcs = result_buf(c, (int64_t)ncs, tmp);
        float* dM = result_buf(c, (int64_t)nm, tmp);
        launch_align_post(ds, n_slots, n_heads, pstride, TK, dm, dm + n_slots, dm + 2 * n_slots, dm + 3 * n_slots, dst,
                          dcs, dM, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(stats, dst, nst * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(colstats, dcs, ncs * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(M, dM, nm * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_debug_align_tail(osw_ctx* c, const float* logits, int32_t rows, int32_t V, int32_t eot, int32_t ctx, int32_t pos,
                         const int32_t* slot, const int32_t* len, const int32_t* head, const int32_t* forced,
                         int32_t n_slots, float* token_logprob, int32_t* cur_tok, int32_t* done) {
    return guard([&] {
        REQUIRE(c && logits && slot && len && head && forced && token_logprob && cur_tok && done, "null argument");
        REQUIRE(rows >= 1 && rows <= 1024 && n_slots >= 1 && n_slots <= 1024, "rows / slots out of range");
        REQUIRE(V >= 1 && V <= 65536 && eot >= 1 && eot <= V, "eot outside [1, V]");
        REQUIRE(ctx >= 1 && ctx <= 448 && pos >= 0, "ctx / pos out of range");
        require_slots(slot, rows, n_slots);
        for (int r = 0; r < rows; ++r) {
            REQUIRE(head[r] == 1 || head[r] == 3, "head: 1 or 3");
            REQUIRE(len[r] >= 0 && len[r] <= ctx, "len outside [0, ctx]");
            for (int i = 0; i < len[r]; ++i)
                REQUIRE(forced[(size_t)r * ctx + i] >= 0 && forced[(size_t)r * ctx + i] < V,
                        "forced token outside the vocabulary");
        }
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        std::vector<SelState> st((size_t)rows);
        for (int r = 0; r < rows; ++r) {
            st[r] = SelState{};
            st[r].done = done[r];
        }
        float* dl = upload(c, logits, (size_t)rows * V, tmp);
        std::vector<int> meta((size_t)1 + 3 * rows);  // pos, slot, len, head
        meta[0] = pos;
        for (int r = 0; r < rows; ++r) {
            meta[1 + r] = slot[r];
            meta[1 + rows + r] = len[r];
            meta[1 + 2 * rows + r] = head[r];
        }
        int* dm = upload(c, meta.data(), meta.size(), tmp);
        int* df = upload(c, forced, (size_t)rows * ctx, tmp);
        float* dlp = upload(c, token_logprob, (size_t)n_slots * ctx, tmp);
        int* dct = upload(c, cur_tok, (size_t)rows, tmp);
        SelState* dst = upload(c, st.data(), (size_t)rows, tmp);
        launch_align_tail(dl, rows, V, eot, ctx, dm, dm + 1, dm + 1 + rows, dm + 1 + 2 * rows, df, dlp, dct, dst,
                          c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(token_logprob, dlp, (size_t)n_slots * ctx * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(cur_tok, dct, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(st.data(), dst, (size_t)rows * sizeof(SelState), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int r = 0; r < rows; ++r) done[r] = st[r].done;
    });
}

int osw_debug_align_self_attn(osw_ctx* c, const float* qkv_slabs, int32_t ks, const float* bias, float* kcache,
                              float* vcache, int32_t rows, int32_t H, int32_t ctx, int32_t pos, const int32_t* done,
                              float* out) {
    return guard([&] {
        REQUIRE(c && qkv_slabs && bias && kcache && vcache && done && out, "null argument");
        REQUIRE(ks >= 1 && ks <= 32, "ks out of range");
        REQUIRE(rows >= 1 && rows <= 1024 && H >= 1 && H <= 20, "rows / heads out of range");
        REQUIRE(ctx >= 1 && ctx <= 448, "ctx out of range (the kernel's score buffer holds 512)");
        REQUIRE(pos >= 0, "negative position");  // (one past ctx - 1 is clamped by the kernel)
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const int D = H * 64;
        const size_t nq = (size_t)ks * rows * 3 * D, nkv = (size_t)rows * H * ctx * 64, no = (size_t)rows * D;
        std::vector<SelState> st((size_t)rows);
        for (int r = 0; r < rows; ++r) {
            st[r] = SelState{};
            st[r].done = done[r];
        }
        float* dq = upload(c, qkv_slabs, nq, tmp);
        float* db = upload(c, bias, (size_t)3 * D, tmp);
        float* dk = upload(c, kcache, nkv, tmp);
        float* dv = upload(c, vcache, nkv, tmp);
        int* dpos = upload(c, &pos, 1, tmp);
        SelState* dst = upload(c, st.data(), (size_t)rows, tmp);
        h16* dout = dalloc<h16>(2 * no, tmp.v);  // hi, then lo
        HIPCHK(hipMemsetAsync(dout, 0xff, 2 * no * 2, c->stream));
        launch_align_self_attn(dq, ks, db, dk, dv, dpos, rows, H, ctx, dout, (int64_t)no, dst, c->stream);
        HIPCHK(hipGetLastError());
        std::vector<h16> back(2 * no);
        HIPCHK(hipMemcpyAsync(back.data(), dout, 2 * no * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(kcache, dk, nkv * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(vcache, dv, nkv * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < no; ++i) out[i] = (float)back[i] + (float)back[no + i];
    });
}

int osw_debug_align_scores(osw_ctx* c, const float* q_slabs, int32_t ks, const float* bias, const void* K, int32_t rows,
                           int32_t H, int32_t T, const int32_t* layer_heads, int32_t n_layer_heads, int32_t n_heads,
                           int32_t pos, const int32_t* slot, const int32_t* len, int32_t pstride, int32_t n_slots,
                           float* scores) {
    return guard([&] {
        REQUIRE(c && q_slabs && K && layer_heads && slot && len && scores, "null argument");
        REQUIRE(ks >= 1 && ks <= 32, "ks out of range");
        REQUIRE(rows >= 1 && rows <= 1024 && H >= 1 && H <= 20 && T >= 1 && T <= 4096, "rows / heads / T out of range");
        REQUIRE(n_heads >= 1 && n_heads <= 64 && n_layer_heads >= 1 && n_layer_heads <= n_heads, "head list out of range");
        REQUIRE(n_slots >= 1 && n_slots <= 1024 && pstride >= 1 && pstride <= 448 && pos >= 0, "slots / pstride / pos out of range");
        std::vector<char> seen((size_t)n_heads, 0);
        for (int e = 0; e < n_layer_heads; ++e) {
            const int h = layer_heads[2 * e], hi = layer_heads[2 * e + 1];
            REQUIRE(h >= 0 && h < H && hi >= 0 && hi < n_heads && !seen[hi], "layer_heads: {head < H, distinct head_idx < n_heads}");
            seen[hi] = 1;
        }
        require_slots(slot, rows, n_slots);
        for (int r = 0; r < rows; ++r) REQUIRE(len[r] >= 0 && len[r] <= pstride, "len outside [0, pstride]");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        TmpBufs tmp;
        const int D = H * 64;
        const size_t nq = (size_t)ks * rows * D, nk = (size_t)rows * H * T * 64;
        const size_t ns = (size_t)n_slots * n_heads * pstride * T;
        float* dq = upload(c, q_slabs, nq, tmp);
        float* db = bias ? upload(c, bias, (size_t)D, tmp) : nullptr;
        h16* dk = upload(c, (const h16*)K, nk, tmp);
        std::vector<int> meta((size_t)1 + 2 * rows + 2 * n_layer_heads);  // pos, slot, len, layer_heads
        meta[0] = pos;
        for (int r = 0; r < rows; ++r) {
            meta[1 + r] = slot[r];
            meta[1 + rows + r] = len[r];
        }
        for (int i = 0; i < 2 * n_layer_heads; ++i) meta[1 + 2 * rows + i] = layer_heads[i];
        int* dm = upload(c, meta.data(), meta.size(), tmp);
        float* dsc = upload(c, scores, ns, tmp);
        launch_align_scores(dq, ks, db, dk, rows, H, T, dm + 1 + 2 * rows, n_layer_heads, n_heads, dm, dm + 1,
                            dm + 1 + rows, dsc, pstride, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(scores, dsc, ns * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_debug_hold_capture(osw_ctx* c, int32_t hold_ms) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        REQUIRE(hold_ms >= 0 && hold_ms <= 10000, "hold_ms out of range");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        // exactly the locks decode_graph holds around a capture
        std::unique_lock<std::mutex> no_encoder;
        if (c->baton) no_encoder = std::unique_lock<std::mutex>(c->baton->mu);
        GateLock gate_(capture_gate());
        HIPCHK(hipStreamSynchronize(c->stream));
        hipGraph_t gr = nullptr;
        c->capturing = true;
        try {
            HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            HIPCHK(hipMemsetAsync(c->done, 0, sizeof(int), c->stream));  // one captured node
            const auto t0 = std::chrono::steady_clock::now();
            while (std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(hold_ms)) {
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
                hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
                HIPCHK(hipStreamIsCapturing(c->stream, &st));
                REQUIRE(st == hipStreamCaptureStatusActive, "the capture was invalidated while held");
            }
            HIPCHK(hipStreamEndCapture(c->stream, &gr));
        } catch (...) {
            c->capturing = false;
            hipGraph_t junk = nullptr;
            (void)hipStreamEndCapture(c->stream, &junk);
            if (junk) (void)hipGraphDestroy(junk);
            (void)hipGetLastError();
            throw;
        }
        c->capturing = false;
        REQUIRE(gr != nullptr, "empty capture");
        hipGraphExec_t ge = nullptr;
        hipError_t e = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        HIPCHK(e);
        (void)hipGraphExecDestroy(ge);
    });
}

}  // extern "C"
