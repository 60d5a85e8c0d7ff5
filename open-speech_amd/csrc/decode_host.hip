// The decoder's host side: one decoder step, the decode-graph cache, the decode plan's glue
// (plan.h) and the batch / refill decode loops and language detection built on it.
#include "ctx.h"

namespace osw {
// Alignment pass only (c->acap set by align()): the raw scaled scores of layer l's alignment
// heads, from the same q slabs the cross-attention launch beside it reduces, and through the
// same window map (c->xmap: osw_session_align's rows read their held slots' keys)
void align_capture(osw_ctx* c, int l, const float* part, int ks, int nb, int64_t xkv_which) {
    const AlignCapture& a = *c->acap;
    const int first = a.layer_first[l], cnt = a.layer_first[l + 1] - first;
    if (cnt <= 0) return;
    launch_align_scores(part, ks, WF(c, "dec.l" + std::to_string(l) + ".xq.b"), c->XKV + (2 * l) * xkv_which, nb,
                        c->d.n_text_head, c->T, a.layer_heads + 2 * first, cnt, a.n_heads, c->pos, a.slot, a.len,
                        a.scores, a.pstride, c->stream, c->xmap);
}

// ---------------------------- decoder --------------------------------------
// The step's cross-attention launch.  A greedy retry session (c->xsplit: beam 1, best_of > 1 rows
// per slot) makes two: a temperature-0 slot decodes on its first row alone and must see what its
// decode alone sees, the one-row kernel (the row-group kernels round differently), while a
// sampling slot's rows go through the row-group kernel a batch decode with best_of rows takes.
// Each launch skips the other kind's rows by its own copy of the done flags (retry_xmask_kernel,
// once per step); the one-row launch reads each row's slot through a row -> slot map and has its
// own tickets, one per (row, head).
namespace {
bool split_cross_attn(const osw_ctx* c) { return c->xsplit && !c->acap; }

void step_cross_attn(osw_ctx* c, const float* part, int ks, const float* bias, const h16* xk, const h16* xv, int nb,
                     int H, int group, int64_t lo_d) {
    if (split_cross_attn(c)) {
        launch_dec_cross_attn(part, ks, bias, xk, xv, nb, H, c->T, 1, c->dattn, lo_d, c->xws, c->xrow_ticket,
                              c->xdone_single, c->stream, c->xrow_map);
        launch_dec_cross_attn(part, ks, bias, xk, xv, nb, H, c->T, group, c->dattn, lo_d, c->xws, c->xticket,
                              c->xdone_group, c->stream, c->xmap);
        return;
    }
    launch_dec_cross_attn(part, ks, bias, xk, xv, nb, H, c->T, group, c->dattn, lo_d, c->xws, c->xticket, c->sel,
                          c->stream, c->xmap);
}
}  // namespace

// One decoder row (batch-1 latency; PRO_ROWS): the
// residual+LayerNorm and GELU-reduce kernels are not launched; each runs as the prologue
// of the projection that consumes it (gemm_skinny_kernel<.., PRO>, resln.h), and the
// embedding is the prologue of layer 0's qkv: 51 -> 34 launches per step, 4 x [qkv,
// self-attn, o, q, cross-attn, xo, fc1, fc2] + logits + select.  The residual stream
// ping-pongs between xd and xd2 (every workgroup of a GEMM reads x, one writes x'), the
// slabs between part and part2 (a GEMM's prologue reads its producer's slabs while its
// epilogue writes its own).  Same arithmetic as decoder_step's separate kernels.
void decoder_step_fused(osw_ctx* c, int nb, int group, bool gather, const SelFuse* sf) {
    const osw_dims& d = c->d;
    const int D = d.n_text_state, H = d.n_text_head, L = d.n_text_layer, ctx = d.n_text_ctx;
    const int64_t xkv_which = (int64_t)(c->xkv_windows ? c->xkv_windows : nb / group) * H * c->T * 64;
    const int64_t kv_layer = (int64_t)(c->kv_rows ? c->kv_rows : nb) * H * ctx * 64;
    const int64_t lo_d = (int64_t)c->R * D;
    float* xs[2] = {c->xd, c->xd2};
    float* ps[2] = {c->part, c->part2};
    int xi = 0, last = 1, ks = 0;  // residual buffer holding x; slab buffer of the last GEMM
    auto gemm = [&](const h16* A, const std::string& w, int N, int K) {
        GemmArgs g = gemm_plain(A, D, WH(c, w), nullptr, nb, N, K, nullptr, 0, EPI_F32);
        gemm_weights(c, w, g);
        g.A_lo = A ? A + lo_d : nullptr;
        return g;
    };
    // residual + LayerNorm prologue over the last GEMM's slabs (bias = its bias); part ==
    // nullptr: the embedding entry
    auto resln = [&](const float* bias, const std::string& ln, bool embed) {
        ProArgs pa{};
        pa.ln = ResLnArgs{embed ? nullptr : ps[last], ks, (int64_t)nb * D, bias, xs[xi], xs[xi ^ 1],
                          WF(c, ln + ".g"), WF(c, ln + ".b"), WH(c, "dec.tok"), WF(c, "dec.pos"), c->cur_tok, c->pos,
                          ctx, D, d.n_vocab, c->row_pos ? 1 : 0, embed ? tok_scale(c) : nullptr};
        xi ^= 1;
        return pa;
    };
    auto plain = [&](const h16* A, const std::string& w, int N, int K) {
        ks = launch_gemm_skinny_partial(gemm(A, w, N, K), ps[last ^ 1], c->stream);
        last ^= 1;
    };
    auto fused = [&](int pro, const ProArgs& pa, const std::string& w, int N, int K) {
        ks = launch_gemm_skinny_pro(gemm(nullptr, w, N, K), pro, pa, false, ps[last ^ 1], c->stream);
        last ^= 1;
    };
    // OSW_B1_ATTN_TAIL=1: the self-attention as the qkv GEMM's last-arriver tail per head
    // (TAIL_ATTN, the same device function as the standalone kernel, so the same bits; the
    // whole GPU suite is green with it).  Measured slower: the tailed qkv takes 15.9 us per
    // launch against 8.0 + 6.4 us for the GEMM and the self-attention kernel, batch-1 p50
    // 111.4 / 111.6 vs 107.1 / 108.7 ms (profiles/r06_s2d_b1_attn_tail_ab.txt): the in-launch
    // seam (ticket, device-scope slab loads) costs more than the kernel boundary it removes
    static const bool attn_tail_on = [] {
        const char* e = getenv("OSW_B1_ATTN_TAIL");
        return e && e[0] == '1';
    }();
    const bool attn_tail = attn_tail_on && nb == 1 && !gather && !c->acap;
    // (opt-in, and refused with int8 weights by the launcher: never a silent float16 fall-back)
    for (int l = 0; l < L; ++l) {
        const std::string p = "dec.l" + std::to_string(l), pp = "dec.l" + std::to_string(l - 1);
        ProArgs pq = l == 0 ? resln(nullptr, p + ".ln1", true) : resln(WF(c, pp + ".fc2.b"), p + ".ln1", false);
        if (attn_tail) {
            pq.tail_ticket = c->tail_ticket + 2048;  // [H] (the GELU tails use the first 160)
            pq.attn = SelfAttnTail{WF(c, p + ".qkv.b"), c->kc + l * kv_layer, c->vc + l * kv_layer, c->pos, H, ctx,
                                   c->row_pos ? 1 : 0, c->dattn, lo_d, c->sel};
            ks = launch_gemm_skinny_pro(gemm(nullptr, p + ".qkv.w", 3 * D, D), PRO_RESLN, pq, false, ps[last ^ 1],
                                        c->stream, false, true);
            last ^= 1;
        } else {
            fused(PRO_RESLN, pq, p + ".qkv.w", 3 * D, D);
            if (c->acap)  // alignment pass: fp32 q / k / v and its own fp32 cache (align.hip)
                launch_align_self_attn(ps[last], ks, WF(c, p + ".qkv.b"), c->acap->kc32 + l * kv_layer,
                                       c->acap->vc32 + l * kv_layer, c->pos, nb, H, ctx, c->dattn, lo_d, c->sel,
                                       c->stream);
            else
            launch_dec_self_attn(ps[last], ks, WF(c, p + ".qkv.b"), c->kc + l * kv_layer, c->vc + l * kv_layer, c->pos,
                                 nb, H, ctx, c->dattn, lo_d, gather ? c->anc : nullptr, group, c->sel, c->stream,
                                 c->row_pos);
        }
        plain(c->dattn, p + ".o.w", D, D);
        fused(PRO_RESLN, resln(WF(c, p + ".o.b"), p + ".ln2", false), p + ".xq.w", D, D);
        {
            Timed t(c, CL_XATTN, 2.0 * nb * H * (double)c->T * 64 * 2);
            step_cross_attn(c, ps[last], ks, WF(c, p + ".xq.b"), c->XKV + (2 * l) * xkv_which,
                            c->XKV + (2 * l + 1) * xkv_which, nb, H, group, lo_d);
        }
        if (c->acap) align_capture(c, l, ps[last], ks, nb, xkv_which);
        plain(c->dattn, p + ".xo.w", D, D);
        fused(PRO_RESLN, resln(WF(c, p + ".xo.b"), p + ".ln3", false), p + ".fc1.w", 4 * D, D);
        ProArgs pg{};
        pg.part = ps[last]; pg.ks = ks; pg.bias = WF(c, p + ".fc1.b");
        fused(PRO_GELU, pg, p + ".fc2.w", D, 4 * D);
    }
    const std::string pl = "dec.l" + std::to_string(L - 1);
    GemmArgs gl = gemm(nullptr, "dec.tok", d.n_vocab, D);
    gl.C = c->logits;
    gl.ldc = d.n_vocab;
    ProArgs pl_args = resln(WF(c, pl + ".fc2.b"), "dec.lnpost", false);
    if (sf) pl_args.sel = *sf;
    {
        Timed t(c, CL_LOGITS, 0);  // (profiling only)
        launch_gemm_skinny_pro(gl, PRO_RESLN, pl_args, true, nullptr, c->stream, sf != nullptr);
    }
    HIPCHK(hipGetLastError());
}

// One decoder step for nb windows.  Every projection is a split-K skinny GEMM whose
// partial slabs are reduced by the kernel that consumes them (self/cross attention
// for q/k/v, residual+LayerNorm for the out-projections and fc2, GELU for fc1).
// nb = decoder rows (windows x group); the `group` rows of one window are adjacent
// (beam hypotheses or best_of samples); `gather` = beam rows read the self-K/V cache
// through the ancestry table.
// sf (batch-1 greedy): the logits GEMM also selects the token and advances the step
// counter; returns whether it did (the caller then launches no select).
bool decoder_step(osw_ctx* c, int nb, int group, bool gather, const SelFuse* sf) {
    const osw_dims& d = c->d;
    const int D = d.n_text_state, H = d.n_text_head, L = d.n_text_layer, ctx = d.n_text_ctx;
    const int64_t xkv_which = (int64_t)(c->xkv_windows ? c->xkv_windows : nb / group) * H * c->T * 64;
    const int64_t kv_layer = (int64_t)(c->kv_rows ? c->kv_rows : nb) * H * ctx * 64;
    REQUIRE(nb <= c->R && D <= 1280, "decoder step: rows <= capacity and D <= 1280");
    require_embedding_kind(c);
    REQUIRE(ctx <= 448, "decoder self-attention holds at most 448 positions");
    // the decoder's GEMM operands are hi/lo fp16 pairs (fp32-accurate activations: the
    // logits stay within 1e-3 of an fp32 decoder); lo = hi + R rows
    const int64_t lo_d = (int64_t)c->R * D, lo_4d = (int64_t)c->R * 4 * D;
    // <= 64 rows: split-K skinny GEMM; more (beam search): see below
    auto partial = [&](const h16* A, int lda, const std::string& w, int N, int K) {
        const h16* Wt = WH(c, w);
        const int64_t lo = lda == 4 * D ? lo_4d : lo_d;
        // > 64 rows (beam search): skinny row groups for every projection.  Round 3 put N > 1536
        // (qkv, fc1) on 64x128 split-K tiles (alone at 320 rows: N = 3840 12.8 vs 17.9 us,
        // N = 5120 20.4 vs 21.7); round 6 re-measured the whole beam-5 bench on one box: 3-lane
        // 3145 / 3138 (skinny everywhere) vs 3098 / 3104 audio-s/s (tiles for N > 1536), one
        // lane 2617 / 2613 vs 2647 / 2650 (profiles/r06_s2k_beam_gemm_ab.txt): the 16-KiB skinny
        // workgroups share the CUs with the other lanes' encoders better.  Same split-K depth
        // (kc 256) and MFMA order either way: the same bits.  OSW_BEAM_GEMM=1: the tiles for
        // N > 1536 (the round-3 choice), 3: tiles everywhere.
        static const int force = getenv("OSW_BEAM_GEMM") ? atoi(getenv("OSW_BEAM_GEMM")) : 2;
        if (nb > 64 && (force == 3 || (force == 1 && N > 1536))) {
            const int ks = tiled_ksplit(nb, N, K);
            REQUIRE((int64_t)ks * nb * N <= c->part_floats, "decoder workspace too small");
            GemmArgs g = gemm_plain(A, lda, Wt, nullptr, nb, N, K, nullptr, 0, EPI_F32);
            gemm_weights(c, w, g);  // (the tiles read W; int8: with the multipliers in the epilogue)
            g.A_lo = A + lo;
            launch_gemm_tiled_partial(g, c->part, ks, c->stream);
            return ks;
        }
        GemmArgs g = gemm_plain(A, lda, Wt, nullptr, nb, N, K, nullptr, 0, EPI_F32);
        gemm_weights(c, w, g);
        g.A_lo = A + lo;
        REQUIRE((int64_t)skinny_ksplit(N, K) * nb * N <= c->part_floats, "split-K workspace too small");
        return launch_gemm_skinny_partial(g, c->part, c->stream);
    };
    if (split_cross_attn(c))
        launch_retry_xmask(c->sel, c->row_inv_temp, group, nb, c->xdone_single, c->xdone_group, c->stream);
    static const bool no_fuse = getenv("OSW_NO_FUSE") != nullptr;  // A/B switch
    if (nb <= PRO_ROWS && !no_fuse) {
        decoder_step_fused(c, nb, group, gather, nb == 1 ? sf : nullptr);
        return sf != nullptr && nb == 1;
    }
    static const bool no_gelu_pro = getenv("OSW_NO_GELU_PRO") != nullptr;  // A/B switch
    const bool gelu_pro = nb <= GELU_ROWS && !no_gelu_pro && 4 * D / skinny_ksplit(D, 4 * D) <= GELU_KC;
    // OSW_GELU_TAIL=1: fc1's last workgroup per column block reduces + GELUs its slabs (no
    // reduce kernel).  Measured slower in the 3-lane headline (5018 / 5016 vs 5049 audio-s/s,
    // profiles/r06_b_gelu_tail_ab.txt): with the lanes overlapping, a launch fewer buys less
    // than the serial tail costs, so it is opt-in
    static const bool gelu_tail_on = getenv("OSW_GELU_TAIL") && getenv("OSW_GELU_TAIL")[0] == '1';
    const bool gelu_tail = !gelu_pro && nb <= 64 && gelu_tail_on && (4 * D) % 64 == 0;
    // x = tok_emb[tok] + pos_emb[pos]; xdn = LN1_0(x)
    launch_dec_resid_ln(nullptr, 0, nb, D, nullptr, c->xd, WF(c, "dec.l0.ln1.g"), WF(c, "dec.l0.ln1.b"), c->xdn, lo_d,
                        WH(c, "dec.tok"), WF(c, "dec.pos"), c->cur_tok, c->pos, ctx, d.n_vocab, c->stream, c->row_pos,
                        tok_scale(c));
    for (int l = 0; l < L; ++l) {
        const std::string p = "dec.l" + std::to_string(l);
        int ks = partial(c->xdn, D, p + ".qkv.w", 3 * D, D);
        if (c->acap)  // alignment pass: fp32 q / k / v and its own fp32 cache (align.hip)
            launch_align_self_attn(c->part, ks, WF(c, p + ".qkv.b"), c->acap->kc32 + l * kv_layer,
                                   c->acap->vc32 + l * kv_layer, c->pos, nb, H, ctx, c->dattn, lo_d, c->sel,
                                   c->stream);
        else
        launch_dec_self_attn(c->part, ks, WF(c, p + ".qkv.b"), c->kc + l * kv_layer, c->vc + l * kv_layer, c->pos, nb,
                             H, ctx, c->dattn, lo_d, gather ? c->anc : nullptr, group, c->sel, c->stream, c->row_pos);
        ks = partial(c->dattn, D, p + ".o.w", D, D);
        launch_dec_resid_ln(c->part, ks, nb, D, WF(c, p + ".o.b"), c->xd, WF(c, p + ".ln2.g"), WF(c, p + ".ln2.b"),
                            c->xdn, lo_d, nullptr, nullptr, nullptr, nullptr, ctx, d.n_vocab, c->stream);
        ks = partial(c->xdn, D, p + ".xq.w", D, D);
        {
            Timed t(c, CL_XATTN, 2.0 * nb * H * (double)c->T * 64 * 2);
            step_cross_attn(c, c->part, ks, WF(c, p + ".xq.b"), c->XKV + (2 * l) * xkv_which,
                            c->XKV + (2 * l + 1) * xkv_which, nb, H, group, lo_d);
        }
        if (c->acap) align_capture(c, l, c->part, ks, nb, xkv_which);
        ks = partial(c->dattn, D, p + ".xo.w", D, D);
        launch_dec_resid_ln(c->part, ks, nb, D, WF(c, p + ".xo.b"), c->xd, WF(c, p + ".ln3.g"), WF(c, p + ".ln3.b"),
                            c->xdn, lo_d, nullptr, nullptr, nullptr, nullptr, ctx, d.n_vocab, c->stream);
        // (a whole-K fc1 with the GELU epilogue fused has only N/64 = 80 workgroups at
        // turbo: 22.7 us vs 9.6 + 4.7 us for split-K + reduce, measured)
        const float* fc2_part = c->part;
        if (gelu_tail) {
            // 9..64 rows: split-K fc1 whose last workgroup per column block reduces that
            // block's slabs + bias + GELU (TAIL_GELU): no reduce kernel
            GemmArgs g = gemm_plain(c->xdn, D, WH(c, p + ".fc1.w"), nullptr, nb, 4 * D, D, nullptr, 0, EPI_F32);
            gemm_weights(c, p + ".fc1.w", g);  // (int8: the launcher refuses the tail)
            g.A_lo = c->xdn + lo_d;
            ProArgs pt{};
            pt.bias = WF(c, p + ".fc1.b");
            pt.tail_ticket = c->tail_ticket;
            pt.tail_y = c->dh;
            pt.tail_lo = lo_4d;
            launch_gemm_skinny_gelu_tail(g, c->part, pt, c->stream);
            HIPCHK(hipGetLastError());
            ks = partial(c->dh, 4 * D, p + ".fc2.w", D, 4 * D);
        } else {
        ks = partial(c->xdn, D, p + ".fc1.w", 4 * D, D);
        if (gelu_pro) {
            // <= 8 rows: the GELU reduce is fc2's prologue (each workgroup reduces only its own
            // K range of the fc1 slabs, resln.h), fc2's slabs go to part2
            ProArgs pg{};
            pg.part = c->part; pg.ks = ks; pg.bias = WF(c, p + ".fc1.b");
            GemmArgs g = gemm_plain(nullptr, D, WH(c, p + ".fc2.w"), nullptr, nb, D, 4 * D, nullptr, 0, EPI_F32);
            gemm_weights(c, p + ".fc2.w", g);
            ks = launch_gemm_skinny_pro(g, PRO_GELU, pg, false, c->part2, c->stream);
            fc2_part = c->part2;
        } else {
            launch_dec_reduce_gelu(c->part, ks, nb, 4 * D, WF(c, p + ".fc1.b"), c->dh, lo_4d, c->stream);
            ks = partial(c->dh, 4 * D, p + ".fc2.w", D, 4 * D);
        }
        }
        const std::string nx = l + 1 < L ? "dec.l" + std::to_string(l + 1) + ".ln1" : std::string("dec.lnpost");
        launch_dec_resid_ln(fc2_part, ks, nb, D, WF(c, p + ".fc2.b"), c->xd, WF(c, nx + ".g"), WF(c, nx + ".b"), c->xdn,
                            lo_d, nullptr, nullptr, nullptr, nullptr, ctx, d.n_vocab, c->stream);
    }
    GemmArgs gl = gemm_plain(c->xdn, D, WH(c, "dec.tok"), nullptr, nb, d.n_vocab, D, c->logits, d.n_vocab, EPI_F32);
    gemm_weights(c, "dec.tok", gl);  // Wf / Wq: the skinny kernel (< 24 rows); the wide kernel reads W
    gl.A_lo = c->xdn + lo_d;
    run_gemm(c, gl, 0);
    return false;
}

// The decode graph for `key` (CH steps of one_step), captured and instantiated on first use;
// at most 16 per context, the least recently used one destroyed to make room.
hipGraphExec_t decode_graph(osw_ctx* c, const std::vector<int64_t>& key, const std::function<void()>& one_step,
                            int CH) {
    auto hit = c->dgraphs.find(key);
    if (hit != c->dgraphs.end()) {
        hit->second.second = ++c->dgraph_tick;
        return hit->second.first;
    }
    {
        constexpr size_t kMaxGraphs = 16;
        // A sibling lane's encoder waits on the baton event, which this lane may have
        // recorded on this stream: HIP refuses that wait while this stream captures
        // ("dependency created on uncaptured work in another stream"), so no sibling
        // enqueues an encoder (which holds the baton's mutex) during a capture.  And no
        // thread of the process touches the legacy stream or synchronises implicitly while
        // it captures: the capture gate (capture_gate) is held from here to the instantiation.
        std::unique_lock<std::mutex> no_encoder;
        if (c->baton) no_encoder = std::unique_lock<std::mutex>(c->baton->mu);
        GateLock gate_(capture_gate());
        if (c->dgraphs.size() >= kMaxGraphs) {  // evict the least recently used
            auto lru = c->dgraphs.begin();
            for (auto it = c->dgraphs.begin(); it != c->dgraphs.end(); ++it)
                if (it->second.second < lru->second.second) lru = it;
            HIPCHK(hipStreamSynchronize(c->stream));
            trace_graph(c, "destroy (LRU)");
            HIPCHK(hipGraphExecDestroy(lru->second.first));
            c->dgraphs.erase(lru);
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        hipGraph_t gr = nullptr;
        hipGraphExec_t ge = nullptr;
        c->capturing = true;
        try {
            trace_graph(c, "capture begin");
            HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            for (int i = 0; i < CH; ++i) one_step();
            HIPCHK(hipStreamEndCapture(c->stream, &gr));
            trace_graph(c, "capture end");
        } catch (...) {
            c->capturing = false;
            hipGraph_t junk = nullptr;
            (void)hipStreamEndCapture(c->stream, &junk);
            if (junk) (void)hipGraphDestroy(junk);
            throw;
        }
        c->capturing = false;
        hipError_t e = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
        trace_graph(c, "instantiated");
        (void)hipGraphDestroy(gr);
        HIPCHK(e);
        c->dgraphs[key] = {ge, ++c->dgraph_tick};
        return ge;
    }
}

// ---------------------------- decode plan glue ------------------------------
// What decode, decode_refill and session_step share, all driven by a DecodePlan (plan.h).

// The plan's device side: the context's buffers bound (plan.h DecodePlan::bind; with confidences
// on, the recording pointers), the seed and the suppress mask uploaded.
void bind_plan(osw_ctx* c, DecodePlan& p, const osw_decode_opts* o) {
    c->conf_valid = false;
    const bool rows = p.best_of > 0;  // a retry session's plan (osw_debug_select_step_rows)
    p.bind(c->seed_d, c->budget, c->conf, c->lp_hist, c->best_lp, c->lang_probs, rows ? c->row_inv_temp : nullptr,
           rows ? c->row_seed : nullptr);
    HIPCHK(hipMemcpyAsync(c->seed_d, &o->seed, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->supmask, p.mask.data(), p.mask.size() * 4, hipMemcpyHostToDevice, c->stream));
}

// The selection on the step's raw logits: the history rules (repetition_penalty /
// no_repeat_ngram_size, per row), the select kernel, the beam update.  The select kernel
// (greedy) or the beam update advances the step counter.
void plan_select(osw_ctx* c, const DecodePlan& p, int rows, int windows) {
    if (p.hr.on)
        launch_history_rules(c->logits, rows, c->pos, p.sp, c->sel, c->tokens, p.max_tok, p.hr.penalty, p.hr.ngram,
                             c->stream);
    launch_select(c->logits, rows, c->pos, p.sp, c->prompt, c->supmask, c->sel, c->cur_tok, c->tokens, p.max_tok,
                  c->selp, c->sel_arrive, p.beam == 1, c->bcand, c->stream);
    if (p.beam > 1)
        launch_beam(c->logits, windows, c->pos, p.sp, c->supmask, c->sel, c->selp, c->bcand, c->tokens, c->anc,
                    c->d.n_text_ctx, c->bwin, c->btok, c->cur_tok, p.max_tok, c->sel_arrive, c->stream);
}

// One decoder step of `rows` rows (`windows` x plan.group) and its selection.  sf (decode(),
// batch-1 greedy): the logits GEMM selects in its epilogue instead.
void plan_step(osw_ctx* c, const DecodePlan& p, int rows, int windows, const SelFuse* sf = nullptr) {
    if (!decoder_step(c, rows, p.group, p.beam > 1, sf)) plan_select(c, p, rows, windows);
}

hipGraphExec_t plan_graph(osw_ctx* c, const DecodePlan& p, int rows, int windows, int CH, const SelFuse* sf) {
    return decode_graph(c, p.key(rows, CH), [&] { plan_step(c, p, rows, windows, sf); }, CH);
}

// CH steps: one replay of the plan's graph for this shape, or (graph off, profiling mode 2, a
// tail shorter than a chunk) CH eager steps.
void run_chunk(osw_ctx* c, const DecodePlan& p, int rows, int windows, int CH, bool graph,
               const SelFuse* sf) {
    if (graph) {
        hipGraphExec_t ge = plan_graph(c, p, rows, windows, CH, sf);
        trace_graph(c, "launch");
        HIPCHK(hipGraphLaunch(ge, c->stream));
    } else {
        for (int i = 0; i < CH; ++i) plan_step(c, p, rows, windows, sf);
    }
    HIPCHK(hipGetLastError());
}

// read_state / read_tokens enqueue their copies on the context's stream; the caller synchronises
void read_state(osw_ctx* c, const DecodePlan& p, int rows, int windows, Readback& rb) {
    rb.st.resize(rows);
    HIPCHK(hipMemcpyAsync(rb.st.data(), c->sel, (size_t)rows * sizeof(SelState), hipMemcpyDeviceToHost, c->stream));
    if (p.beam == 1) return;
    rb.bw.resize(windows);
    HIPCHK(hipMemcpyAsync(rb.bw.data(), c->bwin, (size_t)windows * sizeof(BeamWin), hipMemcpyDeviceToHost, c->stream));
}
// by_row (a beam retry session with a finished sampling slot): also the rows' own tokens and
// cumulative log-probs (rb.rtoks / rb.rcum), which a sampling slot's result is read from
void read_tokens(osw_ctx* c, const DecodePlan& p, int rows, int windows, Readback& rb, bool by_row) {
    if (by_row && p.beam > 1) {
        rb.rtoks.resize((size_t)rows * p.max_tok);
        HIPCHK(hipMemcpyAsync(rb.rtoks.data(), c->tokens, rb.rtoks.size() * 4, hipMemcpyDeviceToHost, c->stream));
        if (c->conf) {
            rb.rcum.resize((size_t)rows * p.sp.lp_stride);
            HIPCHK(hipMemcpyAsync(rb.rcum.data(), c->lp_hist, rb.rcum.size() * 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    const size_t units = p.beam > 1 ? windows : rows;
    rb.toks.resize(units * p.max_tok);
    HIPCHK(hipMemcpyAsync(rb.toks.data(), p.beam > 1 ? c->btok : c->tokens, rb.toks.size() * 4, hipMemcpyDeviceToHost,
                          c->stream));
    if (!c->conf) return;
    rb.cum.resize(units * p.sp.lp_stride);
    rb.lang.resize((size_t)windows * p.ss.n_langs);
    HIPCHK(hipMemcpyAsync(rb.cum.data(), p.beam > 1 ? c->best_lp : c->lp_hist, rb.cum.size() * 4, hipMemcpyDeviceToHost,
                          c->stream));
    if (!rb.lang.empty())
        HIPCHK(hipMemcpyAsync(rb.lang.data(), c->lang_probs, rb.lang.size() * 4, hipMemcpyDeviceToHost, c->stream));
}

// Window `win`'s result, read from decoder row `row`, into r[out] and (confidences on)
// conf_res[out].  n0 / n: the token count before / after the caller's max_tokens clamp; a row that
// recorded n0 + 1 log-probs ended with an <|endoftext|> step, whose entry stays the last one.
// sampled (retry sessions): the window's rows sampled, so its result is row `row`'s own whatever the
// plan's beam (a beam session: from rb.rtoks / rb.rcum).
void write_window(osw_ctx* c, const DecodePlan& p, osw_window_result* r, size_t out, const Readback& rb, size_t row,
                  size_t win, bool sampled) {
    const SelState& q = rb.st[row];
    const BeamWin* bw = p.beam > 1 && !sampled ? &rb.bw[win] : nullptr;
    const size_t unit = bw ? win : row;
    const std::vector<int>& toks = sampled && p.beam > 1 ? rb.rtoks : rb.toks;
    const std::vector<float>& cums = sampled && p.beam > 1 ? rb.rcum : rb.cum;
    const int n0 = bw ? bw->best_len : q.n_sampled;
    const int n = std::min(n0, std::min(p.max_tok, r->max_tokens));
    r->n_tokens[out] = n;
    std::copy_n(&toks[unit * p.max_tok], n, r->tokens + out * r->max_tokens);
    r->sum_logprob[out] = bw ? bw->best_raw : q.sum_lp;
    r->no_speech_prob[out] = q.nsp;
    r->language[out] = p.ss.english ? -1 : q.lang;
    if (!c->conf) return;
    if (c->conf_res.size() <= out) c->conf_res.resize(out + 1);
    osw_ctx::ConfResult& cr = c->conf_res[out];
    const float* cum = &cums[unit * p.sp.lp_stride];
    const int nlp = bw ? bw->best_nlp : q.n_lp;
    cr.cum.assign(cum, cum + std::min(n, nlp));
    if (nlp == n0 + 1) cr.cum.push_back(cum[nlp - 1]);
    cr.lang.assign(rb.lang.data() + win * p.ss.n_langs, rb.lang.data() + (win + 1) * p.ss.n_langs);
}

// After a chunk of a refill or session decode: the window slots `live` names that have finished
// (beam: the window's stop rule, else its row), with their tokens read back into rb.
// armed (retry sessions): armed(i) > 0 rows of slot i sample, and the slot has finished when all
// of them have.
std::vector<int> finished_windows(osw_ctx* c, const DecodePlan& p, int rows, int windows,
                                  const std::function<bool(int)>& live, Readback& rb,
                                  const std::function<int(int)>& armed) {
    read_state(c, p, rows, windows, rb);
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int> fin;
    bool by_row = false;
    for (int i = 0; i < windows; ++i) {
        if (!live(i)) continue;
        const int n = armed ? armed(i) : 0;
        bool done = n > 0 ? true : (p.beam > 1 ? rb.bw[i].done != 0 : rb.st[(size_t)i * p.group].done != 0);
        for (int k = 0; k < n; ++k) done = done && rb.st[(size_t)i * p.group + k].done;
        if (!done) continue;
        fin.push_back(i);
        by_row = by_row || n > 0;
    }
    if (fin.empty()) return fin;
    read_tokens(c, p, rows, windows, rb, by_row);
    HIPCHK(hipStreamSynchronize(c->stream));
    return fin;
}

// best_of: of rows [first, first + n), the sample with the highest sum_logprob /
// n_sampled**length_penalty (the first on ties)
size_t best_sample(const Readback& rb, size_t first, int n, float length_penalty) {
    auto norm = [&](const SelState& q) {
        if (q.n_sampled == 0) return length_penalty != 0.f ? -INFINITY : q.sum_lp;
        return q.sum_lp / std::pow((float)q.n_sampled, length_penalty);
    };
    size_t best = first;
    for (int k = 1; k < n; ++k)
        if (norm(rb.st[first + k]) > norm(rb.st[best])) best = first + k;
    return best;
}

// Refill and sessions start with every row finished (nothing to step until a window is admitted)
// and the per-row step counters at 0.
void park_rows(osw_ctx* c, int R) {
    std::vector<SelState> st(R);
    for (auto& q : st) q = SelState{}, q.done = 1;
    HIPCHK(hipMemcpyAsync(c->sel, st.data(), (size_t)R * sizeof(SelState), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->pos, 0, (size_t)R * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->cur_tok, 0, (size_t)R * 4, c->stream));
}

// windows (osw_decode_window_list): decoder row group i attends encoded window windows[i]; the
// cross-K/V planes keep the encode call's window count as their stride (c->xkv_windows, as in
// sessions) and the cross-attention kernels read the K/V head offset through c->xmap.  Nothing
// else knows: prompts, row state, tickets and results are those of a plain decode of nb windows.
void decode(osw_ctx* c, int nb, const osw_decode_opts* o, osw_window_result* r, const int32_t* windows) {
    if (windows) {
        REQUIRE(nb >= 1 && nb <= c->n_encoded, "window list: 1 <= n <= the last encode call's window count");
        std::vector<char> seen((size_t)c->n_encoded, 0);
        for (int i = 0; i < nb; ++i) {
            REQUIRE(windows[i] >= 0 && windows[i] < c->n_encoded, "window list: index outside the last encode call");
            REQUIRE(!seen[windows[i]], "window list: a window appears twice");
            seen[windows[i]] = 1;
        }
    } else {
        REQUIRE(nb >= 1 && nb == c->n_encoded, "decode window count must equal the last encode call");
    }
    REQUIRE(o && r && r->tokens && r->n_tokens && r->sum_logprob && r->no_speech_prob && r->language,
            "null decode argument");
    struct Mapped {  // the map and the plane stride hold for this call only
        osw_ctx* c;
        ~Mapped() {
            c->xmap = nullptr;
            c->xkv_windows = 0;
        }
    };
    std::unique_ptr<Mapped> mapped;
    if (windows) {
        mapped.reset(new Mapped{c});
        c->xkv_windows = c->n_encoded;
        c->xmap = c->xmap_d;
        HIPCHK(hipMemcpyAsync(c->xmap_d, windows, (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
    }
    const osw_dims& d = c->d;
    const int V = d.n_vocab;
    // a mapped decode bakes the map's address and the plane stride into its launches: its own
    // graphs (the plan's key holds the plane stride; the map's contents are data, not key)
    DecodePlan plan(DecodeMode::Batch, o, d, o->n_prefix, windows ? c->n_encoded : 0);
    const int n_pre = plan.n_pre, beam = plan.beam, group = plan.group, P = plan.P, max_len = plan.max_len,
              max_tok = plan.max_tok;
    const int rows = nb * group;
    REQUIRE(rows <= c->R, "windows x beam_size (best_of) exceeds the decoder row capacity (5 x max_batch)");
    REQUIRE(group == 1 || !r->logits_dump, "logits dump needs one decoder row per window");
    // one prompt per decoder row (the beam rows of a window share it)
    std::vector<int> prompt((size_t)rows * P);
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < group; ++k) {
            int* pr = &prompt[((size_t)b * group + k) * P];
            for (int i = 0; i < n_pre; ++i) pr[i] = o->prefix_tokens[(size_t)b * n_pre + i];
            plan.ss.tokens(o->language_tokens ? o->language_tokens[b] : o->language_token, pr + n_pre);
        }
    std::vector<int> first(rows);
    for (int b = 0; b < rows; ++b) first[b] = prompt[(size_t)b * P];
    HIPCHK(hipMemcpyAsync(c->prompt, prompt.data(), prompt.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->cur_tok, first.data(), rows * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->pos, 0, 4, c->stream));
    HIPCHK(hipMemsetAsync(c->sel, 0, (size_t)rows * sizeof(SelState), c->stream));
    std::vector<int> anc0;
    if (beam > 1) {
        anc0.resize((size_t)rows * d.n_text_ctx);
        for (int b = 0; b < rows; ++b)
            for (int p = 0; p < d.n_text_ctx; ++p) anc0[(size_t)b * d.n_text_ctx + p] = b;
        HIPCHK(hipMemcpyAsync(c->anc, anc0.data(), anc0.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(c->bwin, 0, (size_t)nb * sizeof(BeamWin), c->stream));
        HIPCHK(hipMemsetAsync(c->btok, 0, (size_t)nb * max_tok * 4, c->stream));
    }
    if (o->token_budget) {
        std::vector<int> bud(rows);
        for (int i = 0; i < rows; ++i) bud[i] = o->token_budget[i / group];
        HIPCHK(hipMemcpyAsync(c->budget, bud.data(), rows * 4, hipMemcpyHostToDevice, c->stream));
    }
    bind_plan(c, plan, o);
    // batch-1 greedy: the selection runs in the logits GEMM's epilogue (SelFuse, decode.h);
    // not with a history rule on, which has to see the whole row before the selection
    static const bool no_fuse_sel = getenv("OSW_NO_FUSE_SELECT") != nullptr;  // A/B switch
    SelFuse sf{plan.sp, c->logits, c->pos, c->supmask, c->prompt, c->sel, c->cur_tok, c->tokens, max_tok, c->selp1,
               c->sel_arrive + 1};
    const SelFuse* sfp = (rows == 1 && beam == 1 && !plan.sampling && !no_fuse_sel && !plan.hr.on) ? &sf : nullptr;
    const int CH = 8;
    const bool graph = c->use_graph && !r->logits_dump && !c->prof_eager;
    if (graph) plan_graph(c, plan, rows, nb, CH, sfp);  // captured before the timed stage
    int steps = 0;
    {
        Timed t(c, CL_STAGE_DEC, 0);
        int since_check = 0;
        while (steps < max_len) {
            const int samp = steps - (P - 1);
            int did = 1;
            if (graph && max_len - steps >= CH) {
                run_chunk(c, plan, rows, nb, did = CH, true, sfp);
            } else if (r->logits_dump && samp >= 0 && samp < r->dump_steps) {
                const bool selected = decoder_step(c, rows, group, beam > 1, sfp);
                for (int b = 0; b < nb; ++b)
                    HIPCHK(hipMemcpyAsync(r->logits_dump + ((size_t)b * r->dump_steps + samp) * V,
                                          c->logits + (size_t)b * V, (size_t)V * 4, hipMemcpyDeviceToHost,
                                          c->stream));
                if (!selected) plan_select(c, plan, rows, nb);
                HIPCHK(hipGetLastError());
            } else {
                run_chunk(c, plan, rows, nb, 1, false, sfp);
            }
            steps += did;
            since_check += did;
            if (steps >= P && (since_check >= CH || steps >= max_len)) {
                since_check = 0;
                launch_count_done(c->sel, rows, c->done, c->stream);
                HIPCHK(hipMemcpyAsync(c->done_host, c->done, 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                if (*c->done_host >= rows) break;
            }
        }
    }
    c->pf.decode_steps = steps;
    Readback rb;
    read_state(c, plan, rows, nb, rb);
    read_tokens(c, plan, rows, nb, rb, false);
    c->conf_res.clear();
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < nb; ++b)
        write_window(c, plan, r, b, rb, plan.sampling ? best_sample(rb, (size_t)b * group, group, o->length_penalty)
                                                      : (size_t)b * group, b);
    c->conf_valid = c->conf;
}

// osw_detect_language: one decoder step on <|startoftranscript|> (no prefix) for the n windows
// last encoded, then the select kernel's <|startoftranscript|> branch with the language softmax
// on.  Launched eagerly on the context's stream; every buffer it writes (row state, step
// counter, position 0 of the self-K/V cache) is reset or rewritten by the next decode call, and
// the encoder output and cross-K/V are only read.
void detect_language(osw_ctx* c, int nb, const osw_decode_opts* o, float* probs, float* raw) {
    REQUIRE(nb >= 1 && nb == c->n_encoded, "detect window count must equal the last encode call");
    REQUIRE(o && probs, "null detect argument");
    REQUIRE(o->task_token >= 0, "an English-only model (task_token < 0) has no language to detect");
    const osw_dims& d = c->d;
    const int V = d.n_vocab, P = 3;
    REQUIRE(V <= SEL_SPLIT * 4096, "vocabulary too large for the selection kernels");
    REQUIRE(o->n_langs >= 1 && o->n_langs <= LANG_CAP && o->first_lang >= 0 && o->first_lang + o->n_langs <= V,
            "language token range");
    REQUIRE(nb <= c->R && P < d.n_text_ctx, "decoder rows");
    std::vector<int> prompt((size_t)nb * P), first(nb, o->sot);
    for (int b = 0; b < nb; ++b) {
        prompt[(size_t)b * P] = o->sot;
        prompt[(size_t)b * P + 1] = -1;
        prompt[(size_t)b * P + 2] = o->task_token;
    }
    HIPCHK(hipMemcpyAsync(c->prompt, prompt.data(), prompt.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->cur_tok, first.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->pos, 0, 4, c->stream));
    HIPCHK(hipMemsetAsync(c->sel, 0, (size_t)nb * sizeof(SelState), c->stream));
    SelParams SP{};
    SP.prompt_len = P; SP.sot_pos = 0; SP.lang_pos = 1; SP.max_length = d.n_text_ctx;
    SP.pstride = P; SP.tail = P;
    SP.V = V; SP.eot = o->eot; SP.no_speech = std::max(0, std::min(o->no_speech, V - 1));
    SP.no_ts = o->no_timestamps; SP.tb = o->timestamp_begin;
    SP.blank = o->blank; SP.first_lang = o->first_lang; SP.n_langs = o->n_langs;
    SP.beam = 1; SP.num_hyp = 1; SP.max_cand = 1;
    SP.seed = c->seed_d;
    SP.lp_group = 1; SP.lp_stride = d.n_text_ctx;
    SP.lang_probs = c->lang_probs;
    decoder_step(c, nb, 1, false, nullptr);
    launch_select(c->logits, nb, c->pos, SP, c->prompt, c->supmask, c->sel, c->cur_tok, c->tokens, 1, c->selp,
                  c->sel_arrive, true, c->bcand, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(probs, c->lang_probs, (size_t)nb * o->n_langs * 4, hipMemcpyDeviceToHost, c->stream));
    if (raw)
        HIPCHK(hipMemcpy2DAsync(raw, (size_t)o->n_langs * 4, c->logits + o->first_lang, (size_t)V * 4,
                                (size_t)o->n_langs * 4, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

// Greedy decoding with row refill (osw_transcribe_refill): the decoder keeps c->B rows and
// every row has its own step counter (pos[row], SelParams::pos_row), so when a window
// finishes, a queued clip's window is encoded straight into that row's cross-K/V slot and
// starts at position 0 beside rows that are mid-way.  A batch then costs what its windows'
// own lengths cost instead of its longest window's.  Every row's arithmetic is the plain
// greedy decode's (rows are independent in every kernel), so each clip's result equals
// osw_transcribe_batch's for it.  Windows are admitted once refill_min rows are free (or
// when no row is active); empty rows stay finished and are skipped by the attention kernels.
void decode_refill(osw_ctx* c, int n_clips, const osw_decode_opts* o, osw_window_result* r, int refill_min) {
    REQUIRE(o && r && r->tokens && r->n_tokens && r->sum_logprob && r->no_speech_prob && r->language,
            "null decode argument");
    REQUIRE(!(o->temperature > 0.f) && o->beam_size <= 1, "row refill decodes greedily (temperature 0, beam_size 1)");
    REQUIRE(o->n_prefix == 0, "row refill takes no prefix tokens");
    REQUIRE(!r->logits_dump, "row refill has no logits dump");
    const int R = c->B;
    DecodePlan plan(DecodeMode::Refill, o, c->d);
    REQUIRE(R <= c->R, "decoder rows");
    const int P = plan.P;
    refill_min = std::max(1, std::min(refill_min, R));
    bind_plan(c, plan, o);
    c->conf_res.clear();
    park_rows(c, R);
    HIPCHK(hipMemsetAsync(c->prompt, 0, (size_t)R * P * 4, c->stream));
    struct RowPos {
        osw_ctx* c;
        ~RowPos() { c->row_pos = false; c->n_encoded = 0; }
    } row_pos_scope{c};
    c->row_pos = true;
    const int CH = 8;
    const bool graph = c->use_graph && !c->prof_eager;
    if (graph) plan_graph(c, plan, R, R, CH, nullptr);  // captured before the first encoder is enqueued
    std::vector<int> row_clip(R, -1), pack;
    Readback rb;
    int next = 0, active = 0, steps = 0;
    while (true) {
        std::vector<int> free_rows;
        for (int i = 0; i < R; ++i)
            if (row_clip[i] < 0) free_rows.push_back(i);
        const int left = n_clips - next;
        if (left > 0 && (active == 0 || (int)free_rows.size() >= std::min(refill_min, left))) {
            const int k = std::min((int)free_rows.size(), left);
            std::vector<osw_window> wins(k);
            std::vector<int> slots(k);
            pack.assign((size_t)k * (2 + P), 0);
            for (int i = 0; i < k; ++i) {
                const int clip = next + i, row = free_rows[i];
                wins[i] = osw_window{clip, 0, std::max(1, std::min(c->NF, c->nframes[clip] - 1))};
                slots[i] = row;
                int* e = &pack[(size_t)i * (2 + P)];
                e[0] = row;
                e[1] = o->token_budget ? o->token_budget[clip] : 0;
                plan.ss.tokens(o->language_tokens ? o->language_tokens[clip] : o->language_token, e + 2);
                row_clip[row] = clip;
            }
            encode(c, wins.data(), k, slots.data());
            c->n_encoded = 0;
            HIPCHK(hipMemcpyAsync(c->refill_pack, pack.data(), pack.size() * 4, hipMemcpyHostToDevice, c->stream));
            launch_refill_rows(c->refill_pack, k, P, c->prompt, plan.sp.budget ? c->budget : nullptr, c->cur_tok, c->pos,
                               c->sel, c->stream);
            HIPCHK(hipGetLastError());
            next += k;
            active += k;
        }
        if (active == 0) break;
        run_chunk(c, plan, R, R, CH, graph);
        steps += CH;
        for (int i : finished_windows(c, plan, R, R, [&](int i) { return row_clip[i] >= 0; }, rb)) {
            write_window(c, plan, r, row_clip[i], rb, i, i);
            row_clip[i] = -1;
            --active;
        }
    }
    c->pf.decode_steps = steps;
    if (c->conf) c->conf_res.resize(n_clips);
    c->conf_valid = c->conf;
}
}  // namespace osw
