// libosw_hip.so runtime: context, weights, resident buffers, log-mel, the encoder pipeline,
// word alignment and the C ABI of include/osw.h (the decoder: decode_host.hip, session.hip).
//
// One context = one device, one HIP stream, buffers sized for `max_batch` windows
// at creation (nothing is allocated in the per-call hot path except when a call
// brings more PCM / mel than any earlier call).  Calls on one context are
// serialised by a mutex; independent contexts (one per GPU) run concurrently.
#include "ctx.h"

namespace osw {
thread_local std::string g_err;

// The capture gate (one per process; what takes it and why: ctx.h)
std::recursive_mutex& capture_gate() {
    static std::recursive_mutex m;
    return m;
}

// OSW_TRACE_GRAPH=1: one stderr line per decode-graph event (capture, instantiate, launch,
// LRU destroy) with the calling thread and context, to correlate host-side crashes of a
// tool that intercepts HIP (e.g. a profiler) with what the lanes were doing
void trace_graph(const osw_ctx* c, const char* what) {
    static const bool on = [] {
        const char* e = std::getenv("OSW_TRACE_GRAPH");
        return e && e[0] == '1';
    }();
    if (!on) return;
    std::fprintf(stderr, "[osw-graph] thread %zx ctx %p %s\n", (size_t)pthread_self(), (const void*)c, what);
    std::fflush(stderr);
}

hipEvent_t get_ev(osw_ctx* c) {
    if (!c->ev_free.empty()) {
        hipEvent_t e = c->ev_free.back();
        c->ev_free.pop_back();
        return e;
    }
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    return e;
}

void resolve_events(osw_ctx* c) {
    if (c->evs.empty()) return;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto& e : c->evs) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
        osw_profile& p = c->pf;
        switch (e.cls) {
            case CL_ENC_GEMM: p.enc_gemm_ms += ms; p.enc_gemm_launches++; p.enc_gemm_flops += e.work; break;
            case CL_ENC_ATTN: p.enc_attn_ms += ms; p.enc_attn_launches++; p.enc_attn_flops += e.work; break;
            case CL_MEL: p.mel_kernel_ms += ms; p.mel_kernel_launches++; p.mel_kernel_bytes += e.work; break;
            case CL_XATTN: p.xattn_ms += ms; p.xattn_launches++; p.xattn_bytes += e.work; break;
            case CL_LOGITS: c->logits_ms += ms; c->logits_launches++; break;
            case CL_STAGE_MEL: p.mel_ms += ms; break;
            case CL_STAGE_ENC: p.encoder_ms += ms; break;
            case CL_STAGE_XKV: p.crosskv_ms += ms; break;
            case CL_STAGE_DEC: p.decoder_ms += ms; break;
        }
        c->ev_free.push_back(e.a);
        c->ev_free.push_back(e.b);
    }
    c->evs.clear();
}

// ---------------------------------------------------------------------------
void add_tensor(osw_ctx* c, const std::string& name, int64_t numel, bool f16) {
    Tensor t;
    t.numel = numel;
    t.f16 = f16;
    c->w[name] = t;
}

void build_weight_table(osw_ctx* c) {
    const osw_dims& d = c->d;
    const int64_t De = d.n_audio_state, Dd = d.n_text_state, L = d.n_text_layer;
    add_tensor(c, "enc.conv1.w", De * 3 * c->C1, true);  // stored padded [De][3][C1]
    add_tensor(c, "enc.conv1.b", De, false);
    add_tensor(c, "enc.conv2.w", De * 3 * De, true);
    add_tensor(c, "enc.conv2.b", De, false);
    add_tensor(c, "enc.pos", (int64_t)d.n_audio_ctx * De, false);
    for (int i = 0; i < d.n_audio_layer; ++i) {
        const std::string p = "enc.l" + std::to_string(i);
        add_tensor(c, p + ".ln1.g", De, false);
        add_tensor(c, p + ".ln1.b", De, false);
        add_tensor(c, p + ".qkv.w", 3 * De * De, true);
        add_tensor(c, p + ".qkv.b", 3 * De, false);
        add_tensor(c, p + ".o.w", De * De, true);
        add_tensor(c, p + ".o.b", De, false);
        add_tensor(c, p + ".ln2.g", De, false);
        add_tensor(c, p + ".ln2.b", De, false);
        add_tensor(c, p + ".fc1.w", 4 * De * De, true);
        add_tensor(c, p + ".fc1.b", 4 * De, false);
        add_tensor(c, p + ".fc2.w", 4 * De * De, true);
        add_tensor(c, p + ".fc2.b", De, false);
    }
    add_tensor(c, "enc.lnpost.g", De, false);
    add_tensor(c, "enc.lnpost.b", De, false);
    add_tensor(c, "dec.tok", (int64_t)d.n_vocab * Dd, true);
    add_tensor(c, "dec.pos", (int64_t)d.n_text_ctx * Dd, false);
    add_tensor(c, "dec.crosskv.w", L * 2 * Dd * De, true);
    add_tensor(c, "dec.crosskv.b", L * 2 * Dd, false);
    for (int i = 0; i < d.n_text_layer; ++i) {
        const std::string p = "dec.l" + std::to_string(i);
        add_tensor(c, p + ".ln1.g", Dd, false);
        add_tensor(c, p + ".ln1.b", Dd, false);
        add_tensor(c, p + ".qkv.w", 3 * Dd * Dd, true);
        add_tensor(c, p + ".qkv.b", 3 * Dd, false);
        add_tensor(c, p + ".o.w", Dd * Dd, true);
        add_tensor(c, p + ".o.b", Dd, false);
        add_tensor(c, p + ".ln2.g", Dd, false);
        add_tensor(c, p + ".ln2.b", Dd, false);
        add_tensor(c, p + ".xq.w", Dd * Dd, true);
        add_tensor(c, p + ".xq.b", Dd, false);
        add_tensor(c, p + ".xo.w", Dd * Dd, true);
        add_tensor(c, p + ".xo.b", Dd, false);
        add_tensor(c, p + ".ln3.g", Dd, false);
        add_tensor(c, p + ".ln3.b", Dd, false);
        add_tensor(c, p + ".fc1.w", 4 * Dd * Dd, true);
        add_tensor(c, p + ".fc1.b", 4 * Dd, false);
        add_tensor(c, p + ".fc2.w", 4 * Dd * Dd, true);
        add_tensor(c, p + ".fc2.b", Dd, false);
    }
    add_tensor(c, "dec.lnpost.g", Dd, false);
    add_tensor(c, "dec.lnpost.b", Dd, false);
    // fragment-major copies of what the skinny decoder GEMMs stream (+ 0.3 GB at turbo):
    // measured on the 133 MB logits matrix (tools/gemv_probe.hip), the 1-KB contiguous
    // fragment loads stream 5.2-5.4 TB/s against 3.9-4.2 TB/s for 16 rows x 64 B
    auto frag = [&](const std::string& n, int64_t N, int64_t K) {
        Tensor& t = c->w[n];
        t.frag_n = (int)N;
        t.frag_k = (int)K;
        t.q8 = std::make_shared<std::atomic<int>>(0);
        add_tensor(c, n + ".frag", (N + 15) / 16 * 16 * K, true);
        c->w[n + ".frag"].set = true;  // derived: written by pack_frag
        // the row multipliers of int8 weights (osw_set_weight_quant); the int8 fragments take half
        // of the ".frag" region
        add_tensor(c, n + ".scale", N, false);
        c->w[n + ".scale"].set = true;
    };
    frag("dec.tok", d.n_vocab, Dd);
    for (int i = 0; i < d.n_text_layer; ++i) {
        const std::string p = "dec.l" + std::to_string(i);
        frag(p + ".qkv.w", 3 * Dd, Dd);
        frag(p + ".o.w", Dd, Dd);
        frag(p + ".xq.w", Dd, Dd);
        frag(p + ".xo.w", Dd, Dd);
        frag(p + ".fc1.w", 4 * Dd, Dd);
        frag(p + ".fc2.w", Dd, 4 * Dd);
    }

    // one arena, every tensor 256-B aligned
    size_t total = 0;
    for (auto& kv : c->w) total += ((size_t)kv.second.numel * (kv.second.f16 ? 2 : 4) + 255) & ~(size_t)255;
    void* ap = nullptr;
    GateLock gate_(capture_gate());
    if (hipMalloc(&ap, total) != hipSuccess)
        throw OswError(OSW_ENOMEM, "hipMalloc " + std::to_string(total) + " B (weights) failed");
    const int dev = c->device;
    c->arena = std::shared_ptr<void>(ap, [dev](void* p) {
        GateLock gate_(capture_gate());
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(dev);
        (void)hipFree(p);
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    });
    c->siblings = std::make_shared<std::atomic<int>>(0);
    char* arena = (char*)ap;
    HIPCHK(hipMemsetAsync(arena, 0, total, c->stream));
    size_t off = 0;
    for (auto& kv : c->w) {
        kv.second.ptr = arena + off;
        off += ((size_t)kv.second.numel * (kv.second.f16 ? 2 : 4) + 255) & ~(size_t)255;
    }
}

Tensor& W(osw_ctx* c, const std::string& n) {
    auto it = c->w.find(n);
    if (it == c->w.end()) throw OswError(OSW_EINVAL, "unknown tensor " + n);
    return it->second;
}
const h16* WH(osw_ctx* c, const std::string& n) { return (const h16*)W(c, n).ptr; }
const float* WF(osw_ctx* c, const std::string& n) { return (const float*)W(c, n).ptr; }
// the fragment-major copy of a decoder matrix (GemmArgs::Wf); OSW_NO_WFRAG=1: row-major (A/B)
const h16* WFR(osw_ctx* c, const std::string& n) {
    static const bool off = getenv("OSW_NO_WFRAG") != nullptr;
    if (off) return nullptr;
    auto it = c->w.find(n + ".frag");
    return it == c->w.end() ? nullptr : (const h16*)it->second.ptr;
}
bool is_q8(osw_ctx* c, const std::string& n) {
    const Tensor& t = W(c, n);
    return t.q8 && t.q8->load(std::memory_order_relaxed) != 0;
}
void gemm_weights(osw_ctx* c, const std::string& n, GemmArgs& g) {
    g.W = WH(c, n);
    g.ldw = g.K;
    if (is_q8(c, n)) {  // the int8 fragments, whatever OSW_NO_WFRAG says: there is no float16 form of them
        g.Wf = nullptr;
        g.Wq = (const int8_t*)W(c, n + ".frag").ptr;
        g.wscale = WF(c, n + ".scale");
    } else {
        g.Wf = WFR(c, n);
    }
}
const float* tok_scale(osw_ctx* c) { return is_q8(c, "dec.tok") ? WF(c, "dec.tok.scale") : nullptr; }
// The embedding is layer 0's qkv prologue in the one-row step, and the float16 prologues are
// compiled without the embedding's multipliers: an int8 dec.tok needs an int8 dec.l0.qkv.w.  Checked
// when the weights are finalized and at every decoder step (a matrix may be set again later), at
// every row count, so the same weights never decode at one batch size and fail at another.
void require_embedding_kind(osw_ctx* c) {
    REQUIRE(!is_q8(c, "dec.tok") || is_q8(c, "dec.l0.qkv.w"),
            "int8 dec.tok with a float16 dec.l0.qkv.w: quantise dec.l0.qkv.w too, or neither");
}
// A matrix changes between float16 and int8 only while nothing has its kind baked in: decode
// graphs hold the kernels chosen at capture, and a sibling's graphs cannot be seen from here.
void set_kind(osw_ctx* c, const std::string& n, Tensor& t, bool q8) {
    if (!t.q8) {
        REQUIRE(!q8, "tensor " + n + ": int8 weights are accepted for dec.tok and dec.lN.{qkv,o,xq,xo,fc1,fc2}.w");
        return;
    }
    if ((t.q8->load() != 0) == q8) return;
    REQUIRE(c->dgraphs.empty() && (!c->siblings || c->siblings->load() == 0),
            "tensor " + n + ": float16 <-> int8 is refused once decode graphs or sibling contexts exist");
    t.q8->store(q8 ? 1 : 0);
}
// rewrite the fragment-major copy after the matrix was written (on the context's stream)
void pack_frag(osw_ctx* c, const std::string& n) {
    const Tensor& t = W(c, n);
    if (!t.frag_n) return;
    launch_frag_pack((const h16*)t.ptr, t.frag_k, t.frag_n, t.frag_k, (h16*)W(c, n + ".frag").ptr, c->stream);
    HIPCHK(hipGetLastError());
}

// --------------------------- mel constants ---------------------------------
double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

void setup_mel(osw_ctx* c) {
    const int n_mels = c->d.n_mels;
    std::vector<float2> tw(400);
    std::vector<float> hn(400);
    for (int j = 0; j < 400; ++j) {
        const double a = 2.0 * M_PI * j / 400.0;
        tw[j] = make_float2((float)std::cos(a), (float)-std::sin(a));
        hn[j] = (float)(0.5 - 0.5 * std::cos(a));
    }
    // slaney mel bank (librosa / faster-whisper get_mel_filters), double precision
    std::vector<double> mel_f(n_mels + 2);
    const double mmin = hz_to_mel(0.0), mmax = hz_to_mel(8000.0);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(mmin + (mmax - mmin) * i / (n_mels + 1));
    std::vector<int> lo(n_mels), cnt(n_mels), off(n_mels);
    std::vector<float> wts;
    for (int m = 0; m < n_mels; ++m) {
        const double enorm = 2.0 / (mel_f[m + 2] - mel_f[m]);
        int first = -1, last = -1;
        std::vector<float> row(201);
        for (int k = 0; k < 201; ++k) {
            const double f = k * 16000.0 / 400.0;
            const double lower = -(mel_f[m] - f) / (mel_f[m + 1] - mel_f[m]);
            const double upper = (mel_f[m + 2] - f) / (mel_f[m + 2] - mel_f[m + 1]);
            const double v = std::max(0.0, std::min(lower, upper)) * enorm;
            row[k] = (float)v;
            if (v > 0) {
                if (first < 0) first = k;
                last = k;
            }
        }
        if (first < 0) first = last = 0;
        lo[m] = first;
        cnt[m] = last - first + 1;
        off[m] = (int)wts.size();
        for (int k = first; k <= last; ++k) wts.push_back(row[k]);
    }
    // (the host vectors live until the copies are done: synchronised before returning)
    c->tw400 = dalloc<float2>(400, c->owned);
    c->hann = dalloc<float>(400, c->owned);
    c->flo = dalloc<int>(n_mels, c->owned);
    c->fcnt = dalloc<int>(n_mels, c->owned);
    c->foff = dalloc<int>(n_mels, c->owned);
    c->fw = dalloc<float>(wts.size(), c->owned);
    HIPCHK(hipMemcpyAsync(c->tw400, tw.data(), 400 * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->hann, hn.data(), 400 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->flo, lo.data(), n_mels * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->fcnt, cnt.data(), n_mels * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->foff, off.data(), n_mels * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->fw, wts.data(), wts.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
}

void setup_workspace(osw_ctx* c) {
    const osw_dims& d = c->d;
    const int64_t B = c->B, De = d.n_audio_state, Dd = d.n_text_state;
    const int64_t Me = B * c->T;
    auto& o = c->owned;
    c->win = dalloc<int>(3 * B, o);
    c->X1 = dalloc<h16>(B * (c->NF + 2) * c->C1, o);
    c->H1 = dalloc<h16>(B * (c->NF + 1) * De, o);
    HIPCHK(hipMemsetAsync(c->H1, 0, (size_t)B * (c->NF + 1) * De * 2, c->stream));  // row 0 of every window stays zero
    c->X = dalloc<float>(Me * De, o);
    c->Xn = dalloc<h16>(Me * De, o);
    c->QKV = dalloc<h16>(3 * Me * De, o);
    c->O = dalloc<h16>(Me * De, o);
    c->Hf = dalloc<h16>(Me * 4 * De, o);
    c->E = dalloc<h16>(Me * De, o);
    c->XKV = dalloc<h16>((int64_t)d.n_text_layer * 2 * Me * Dd, o);
    const int64_t R = c->R;
    c->xd = dalloc<float>(R * Dd, o);
    c->xd2 = dalloc<float>(std::min<int64_t>(R, PRO_ROWS) * Dd, o);
    c->xdn = dalloc<h16>(2 * R * Dd, o);
    c->dqkv = dalloc<h16>(R * 3 * Dd, o);
    c->dattn = dalloc<h16>(2 * R * Dd, o);
    c->dq = dalloc<h16>(R * Dd, o);
    c->dh = dalloc<h16>(2 * R * 4 * Dd, o);
    const int64_t kvn = (int64_t)d.n_text_layer * R * d.n_text_ctx * Dd;
    c->kc = dalloc<h16>(kvn, o);
    c->vc = dalloc<h16>(kvn, o);
    c->logits = dalloc<float>(R * d.n_vocab, o);
    c->cur_tok = dalloc<int>(R, o);
    c->pos = dalloc<int>(R, o);  // [0]: the shared step counter; [row] in decode_refill
    c->slot_d = dalloc<int>(B, o);
    c->refill_pack = dalloc<int>(B * (3 + d.n_text_ctx), o);  // (sessions: {slot, plen, budget, prompt})
    c->tokens = dalloc<int>(R * d.n_text_ctx, o);
    c->prompt = dalloc<int>(R * d.n_text_ctx, o);
    c->done = dalloc<int>(1, o);
    c->supmask = dalloc<unsigned>((d.n_vocab + 31) / 32, o);
    c->sel = dalloc<SelState>(R, o);
    c->selp = dalloc<char>((size_t)R * sel_parts_bytes(), o);
    c->selp1 = dalloc<char>((size_t)sel_fused_parts_bytes(d.n_vocab), o);
    c->anc = dalloc<int>(R * d.n_text_ctx, o);
    c->btok = dalloc<int>(B * d.n_text_ctx, o);
    c->bwin = dalloc<BeamWin>(B, o);
    c->bcand = dalloc<char>((size_t)R * beam_cand_bytes(MAX_BEAM), o);
    c->xws = dalloc<float>(R * d.n_text_head * XCHUNKS * XPART, o);
    c->xticket = dalloc<int>(B * d.n_text_head, o);
    HIPCHK(hipMemsetAsync(c->xticket, 0, (size_t)B * d.n_text_head * sizeof(int), c->stream));
    c->xmap_d = dalloc<int>(B, o);
    c->budget = dalloc<int>(R, o);
    c->lp_hist = dalloc<float>(R * d.n_text_ctx, o);
    c->best_lp = dalloc<float>(B * d.n_text_ctx, o);
    c->lang_probs = dalloc<float>(B * LANG_CAP, o);
    c->seed_d = dalloc<unsigned long long>(1, o);
    c->tail_ticket = dalloc<int>(4096, o);  // GEMM tails: [column blocks x row groups] (zero between launches)
    HIPCHK(hipMemsetAsync(c->tail_ticket, 0, 4096 * sizeof(int), c->stream));
    c->sel_arrive = dalloc<int>(1 + R, o);  // [0] rows finalised, [1 + row] slice tickets
    HIPCHK(hipMemsetAsync(c->sel_arrive, 0, (1 + (size_t)R) * sizeof(int), c->stream));
    {
        const int64_t shapes[][2] = {{3 * Dd, Dd}, {Dd, Dd}, {4 * Dd, Dd}, {Dd, 4 * Dd}, {d.n_vocab, Dd}};
        for (auto& nk : shapes)  // skinny split-K slabs: decoder projections at any row count
            c->part_floats = std::max<int64_t>(c->part_floats,
                                               skinny_ksplit((int)nk[0], (int)nk[1]) * nk[0] *
                                                   (nk[0] == d.n_vocab ? std::min<int64_t>(R, 64) : R));
        for (auto& nk : shapes)  // > 64 rows: split-K slabs of the tiled GEMM
            if (R > 64 && nk[0] != d.n_vocab)
                c->part_floats = std::max<int64_t>(c->part_floats,
                                                   (int64_t)tiled_ksplit((int)R, (int)nk[0], (int)nk[1]) * R * nk[0]);
        c->part = dalloc<float>(c->part_floats, o);
        int64_t p2 = 0;
        for (auto& nk : shapes)
            if (nk[0] != d.n_vocab) p2 = std::max<int64_t>(p2, (int64_t)skinny_ksplit((int)nk[0], (int)nk[1]) * nk[0]);
        c->part2 = dalloc<float>(p2 * std::min<int64_t>(R, GELU_ROWS), o);
    }
    GateLock gate_(capture_gate());
    HIPCHK(hipHostMalloc((void**)&c->done_host, sizeof(int), 0));
}

// ------------------------------ GEMM helper ---------------------------------
GemmArgs gemm_plain(const h16* A, int64_t lda, const h16* Wt, const float* bias, int M, int N, int K, void* C,
                    int64_t ldc, int epi) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.a_grp_rows = M; g.a_grp_stride = 0;
    g.W = Wt; g.ldw = K; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.C = C; g.ldc = ldc; g.c_grp_rows = M; g.c_grp_stride = 0; g.pos = nullptr; g.epi = epi;
    return g;
}

bool skinny_ok(const GemmArgs& g) {
    // very wide N (logits) at >= 24 rows: the 128x128 LDS-tiled kernel streams the
    // weights faster (measured 36 vs 44 us at M = 64, N = 51866)
    // (32-row skinny groups for the 64-row logits, which would fit beside another lane's
    // encoder workgroup: 4707 vs 4789 audio-s/s, measured; again with the fragment-major
    // weights in round 4: 5020 / 5019 vs 5065 / 5048, gpurun_out/r04_ag)
    if (g.N >= 16384 && g.M >= 24) return false;
    return g.M <= 64 && g.K % 128 == 0 &&
           (g.epi == EPI_F16 || g.epi == EPI_F16_GELU || g.epi == EPI_F32_RESID || g.epi == EPI_F32);
}

void run_gemm(osw_ctx* c, const GemmArgs& g0, int cls) {
    GemmArgs g = g0;
    g.share_cus = c->share_cus;
    REQUIRE(g.K % 64 == 0, "GEMM K must be a multiple of 64");
    REQUIRE(!g.A_lo || g.epi == EPI_F32, "hi/lo operands feed fp32 outputs only");
    const bool skinny = skinny_ok(g);
    // the tiled kernels' non-fp32 epilogues leave through an LDS image in 16-B chunks
    // (staged_epilogue_sq, the 256-tile staged epilogues) and check only each chunk's
    // first column against N: every row start must be 16-B aligned and N whole chunks
    REQUIRE(skinny || g.epi == EPI_F32 ||
                (g.N % 8 == 0 && (g.epi == EPI_HEADS || (g.ldc % 8 == 0 && g.c_grp_stride % 8 == 0))),
            "GEMM epilogue needs N, ldc and the C group stride to be multiples of 8");
    Timed t(c, cls, 2.0 * g.M * g.N * g.K);
    if (skinny) {
        REQUIRE((int64_t)skinny_ksplit(g.N, g.K) * g.M * g.N <= c->part_floats, "split-K workspace too small");
        launch_gemm_skinny(g, c->part, c->stream);
    } else {
        launch_gemm(g, c->stream);
    }
    HIPCHK(hipGetLastError());
}

// ---------------------------- encoder --------------------------------------
void encoder_layer(osw_ctx* c, int i, int nb) {
    const osw_dims& d = c->d;
    const int De = d.n_audio_state, H = d.n_audio_head;
    const int M = nb * c->T;
    const std::string p = "enc.l" + std::to_string(i);
    launch_layernorm(c->X, M, De, WF(c, p + ".ln1.g"), WF(c, p + ".ln1.b"), c->Xn, c->stream);
    GemmArgs g = gemm_plain(c->Xn, De, WH(c, p + ".qkv.w"), WF(c, p + ".qkv.b"), M, 3 * De, De, c->QKV, 0, EPI_HEADS);
    g.heads_T = c->T; g.heads_H = H; g.heads_nb = nb;
    run_gemm(c, g, CL_ENC_GEMM);
    {
        Timed t(c, CL_ENC_ATTN, 4.0 * nb * H * (double)c->T * c->T * 64);
        launch_enc_attn(c->QKV, c->O, c->T, H, nb, c->stream);
        HIPCHK(hipGetLastError());
    }
    run_gemm(c, gemm_plain(c->O, De, WH(c, p + ".o.w"), WF(c, p + ".o.b"), M, De, De, c->X, De, EPI_F32_RESID),
             CL_ENC_GEMM);
    launch_layernorm(c->X, M, De, WF(c, p + ".ln2.g"), WF(c, p + ".ln2.b"), c->Xn, c->stream);
    run_gemm(c, gemm_plain(c->Xn, De, WH(c, p + ".fc1.w"), WF(c, p + ".fc1.b"), M, 4 * De, De, c->Hf, 4 * De,
                           EPI_F16_GELU), CL_ENC_GEMM);
    run_gemm(c, gemm_plain(c->Hf, 4 * De, WH(c, p + ".fc2.w"), WF(c, p + ".fc2.b"), M, De, 4 * De, c->X, De,
                           EPI_F32_RESID), CL_ENC_GEMM);
}

// The windows of one launch_mel_window, checked against the resident clips: clip, seek and size
// (trimmed to the window's NF = 2 T frames) as the kernel's three int arrays, [3][n].  encode() and
// osw_debug_mel_windows both take their windows through here.
std::vector<int> pack_windows(osw_ctx* c, const osw_window* wins, int n) {
    std::vector<int> hw(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        REQUIRE(wins[i].clip >= 0 && wins[i].clip < c->n_clips, "window clip out of range");
        REQUIRE(wins[i].seek >= 0 && wins[i].seek < c->nframes[wins[i].clip], "window seek out of range");
        REQUIRE(wins[i].segment_size >= 1, "empty window");
        hw[i] = wins[i].clip;
        hw[n + i] = wins[i].seek;
        hw[2 * n + i] = std::min(wins[i].segment_size, c->NF);
    }
    return hw;
}

// slots (row refill): window i's cross K/V goes to decoder row slots[i] of a c->B-row layout
void encode(osw_ctx* c, const osw_window* wins, int n, const int* slots) {
    REQUIRE(c->finalized, "weights not finalized");
    REQUIRE(n >= 1 && n <= c->B, "window count out of range");
    const osw_dims& d = c->d;
    const int De = d.n_audio_state;
    if (slots) {
        std::vector<char> seen(c->B, 0);
        for (int i = 0; i < n; ++i) {
            REQUIRE(slots[i] >= 0 && slots[i] < c->B && !seen[slots[i]], "refill slots must be distinct rows < max_batch");
            seen[slots[i]] = 1;
        }
    }
    const std::vector<int> hw = pack_windows(c, wins, n);
    HIPCHK(hipMemcpyAsync(c->win, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, c->stream));
    std::unique_lock<std::mutex> baton;  // held while this encoder is enqueued (EncBaton)
    // Encoders of fewer than c->baton_min (9) windows skip the baton: a streaming call's
    // 1-4-window encoder fills a fraction of the GPU, so sibling lanes' small encoders run
    // side by side.  Basis: the 4-concurrent-caller probe, 161.6 -> 169.0 calls/s
    // (gpurun_out/r03_ai); the config-5 simulation moved 149.0 -> 154.9 calls/s in that run,
    // but it spreads 148.6-156.0 run to run, so its gain is within noise.
    // The 64-window batches keep the baton.
    if (c->baton && n >= c->baton_min) baton = std::unique_lock<std::mutex>(c->baton->mu);
    // the encoder's kernels go to the low-priority encoder stream (swapped in as c->stream
    // for the launch helpers), fenced by events on both sides
    hipStream_t dec_stream = c->stream;
    struct Restore {
        osw_ctx* c;
        hipStream_t s;
        bool share;
        ~Restore() { c->stream = s; c->share_cus = share; }
    } restore{c, dec_stream, c->share_cus};
    // the CU reservation for sibling decoders (GemmArgs::share_cus) only for the batched
    // encoders: the small ones (streaming calls, session admissions) finish sooner on
    // every CU (OSW_GEMM_GRID=256 in the config-5 simulation: 158.6 -> 164.0 calls/s)
    static const bool share_small = getenv("OSW_SHARE_SMALL") != nullptr;  // A/B switch
    if (n < c->baton_min && !share_small) c->share_cus = false;
    if (c->enc_stream) {
        HIPCHK(hipEventRecord(c->enc_in, dec_stream));
        HIPCHK(hipStreamWaitEvent(c->enc_stream, c->enc_in, 0));
        c->stream = c->enc_stream;
    }
    if (baton.owns_lock() && c->baton->recorded) HIPCHK(hipStreamWaitEvent(c->stream, c->baton->ev, 0));
    {
        Timed t(c, CL_STAGE_ENC, 0);
        launch_mel_window(c->logmel, c->mel_off_d, c->nframes_d, c->clip_max, c->win, c->win + n, c->win + 2 * n, n,
                          d.n_mels, c->C1, c->NF, c->X1, c->stream);
        // conv1: A row (w, t) = X1[w][t .. t+2][:] (3 rows of C1) ; C row -> H1[w][1 + t]
        GemmArgs g{};
        g.A = c->X1; g.lda = c->C1; g.a_grp_rows = c->NF; g.a_grp_stride = (c->NF + 2LL) * c->C1;
        g.W = WH(c, "enc.conv1.w"); g.ldw = 3 * c->C1; g.bias = WF(c, "enc.conv1.b");
        g.M = n * c->NF; g.N = De; g.K = 3 * c->C1;
        g.C = c->H1 + De; g.ldc = De; g.c_grp_rows = c->NF; g.c_grp_stride = (c->NF + 1LL) * De; g.epi = EPI_F16_GELU;
        run_gemm(c, g, CL_ENC_GEMM);
        // conv2 (stride 2): A row (w, t) = H1[w][2t .. 2t+2][:]  (H1 row r = input frame r-1)
        GemmArgs g2{};
        g2.A = c->H1; g2.lda = 2LL * De; g2.a_grp_rows = c->T; g2.a_grp_stride = (c->NF + 1LL) * De;
        g2.W = WH(c, "enc.conv2.w"); g2.ldw = 3LL * De; g2.bias = WF(c, "enc.conv2.b");
        g2.M = n * c->T; g2.N = De; g2.K = 3 * De;
        g2.C = c->X; g2.ldc = De; g2.c_grp_rows = c->T; g2.c_grp_stride = (int64_t)c->T * De;
        g2.pos = WF(c, "enc.pos"); g2.epi = EPI_F32_GELU_POS;
        run_gemm(c, g2, CL_ENC_GEMM);
        for (int i = 0; i < d.n_audio_layer; ++i) encoder_layer(c, i, n);
        launch_layernorm(c->X, (int64_t)n * c->T, De, WF(c, "enc.lnpost.g"), WF(c, "enc.lnpost.b"), c->E, c->stream);
    }
    {
        Timed t(c, CL_STAGE_XKV, 0);
        GemmArgs g = gemm_plain(c->E, De, WH(c, "dec.crosskv.w"), WF(c, "dec.crosskv.b"), n * c->T,
                                d.n_text_layer * 2 * d.n_text_state, De, c->XKV, 0, EPI_HEADS);
        g.heads_T = c->T; g.heads_H = d.n_text_head; g.heads_nb = n;
        if (slots) {
            HIPCHK(hipMemcpyAsync(c->slot_d, slots, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            g.heads_nb = c->B;
            g.heads_slot = c->slot_d;
        }
        run_gemm(c, g, 0);
    }
    HIPCHK(hipGetLastError());
    if (baton.owns_lock()) {
        HIPCHK(hipEventRecord(c->baton->ev, c->stream));
        c->baton->recorded = true;
    }
    if (c->enc_stream) {
        HIPCHK(hipEventRecord(c->enc_out, c->enc_stream));
        HIPCHK(hipStreamWaitEvent(dec_stream, c->enc_out, 0));
    }
    c->n_encoded = n;
}

// ------------------------------ word-timestamp alignment ------------------------------
// The alignment heads grouped by layer on the device; the default set is every head of the
// last n_text_layer / 2 layers (openai-whisper's default when a model names none).
void align_sync_heads(osw_ctx* c) {
    AlignBufs& A = c->al;
    const int L = c->d.n_text_layer, H = c->d.n_text_head;
    if (!A.heads_dirty) return;
    std::vector<int> hd = A.heads;
    if (hd.empty())
        for (int l = L - L / 2; l < L; ++l)
            for (int h = 0; h < H; ++h) {
                hd.push_back(l);
                hd.push_back(h);
            }
    const int n = (int)hd.size() / 2;
    if (!A.lh) A.lh = dalloc<int>((size_t)2 * L * H, c->owned);
    std::vector<int> lh;
    A.layer_first.assign(L + 1, 0);
    for (int l = 0; l < L; ++l) {
        A.layer_first[l] = (int)lh.size() / 2;
        for (int i = 0; i < n; ++i)
            if (hd[2 * i] == l) {
                lh.push_back(hd[2 * i + 1]);
                lh.push_back(i);
            }
    }
    A.layer_first[L] = (int)lh.size() / 2;
    HIPCHK(hipMemcpyAsync(A.lh, lh.data(), lh.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    A.n_heads = n;
    A.heads_dirty = false;
    ++A.gen;
}

void align_reserve(osw_ctx* c, int n_slots, int pstride, int rows) {
    AlignBufs& A = c->al;
    const int ctx = c->d.n_text_ctx;
    auto& o = c->owned;
    if (rows > A.cap_rows) {
        HIPCHK(hipStreamSynchronize(c->stream));
        dfree(A.kc32, o);
        dfree(A.vc32, o);
        const size_t n = (size_t)c->d.n_text_layer * rows * ctx * c->d.n_text_state;
        A.kc32 = dalloc<float>(n, o);
        A.vc32 = dalloc<float>(n, o);
        A.cap_rows = rows;
        ++A.gen;
    }
    if (!A.slot) {
        A.slot = dalloc<int>(c->R, o);
        A.len = dalloc<int>(c->R, o);
        A.forced = dalloc<int>((size_t)c->R * ctx, o);
        A.slot_len = dalloc<int>(c->B, o);
        A.slot_frames = dalloc<int>(c->B, o);
        A.slot_width = dalloc<int>(c->B, o);
        A.slot_T = dalloc<int>(c->B, o);
        A.head = dalloc<int>(c->R, o);
        A.slot_head = dalloc<int>(c->B, o);
        A.path_len = dalloc<int>(c->B, o);
        A.tf = dalloc<int>((size_t)c->B * ctx, o);
        A.tokprob = dalloc<float>((size_t)c->B * ctx, o);
        A.sel = dalloc<SelState>(c->R, o);
        A.cur_tok = dalloc<int>(c->R, o);
        A.pos = dalloc<int>(c->R, o);
    }
    if (n_slots <= A.cap_slots && pstride <= A.cap_pstride && A.n_heads <= A.cap_heads) return;
    HIPCHK(hipStreamSynchronize(c->stream));
    dfree(A.scores, o);
    dfree(A.stats, o);
    dfree(A.colstats, o);
    dfree(A.M, o);
    dfree(A.trace, o);
    dfree(A.path, o);
    const int64_t S = A.cap_slots = std::max(A.cap_slots, n_slots), P = A.cap_pstride = std::max(A.cap_pstride, pstride),
                  NH = A.cap_heads = std::max(A.cap_heads, A.n_heads);
    A.scores = dalloc<float>((size_t)(S * NH * P * c->T), o);
    A.stats = dalloc<float>((size_t)(S * NH * P * 2), o);
    A.colstats = dalloc<float>((size_t)(S * NH * c->T * 2), o);
    A.M = dalloc<float>((size_t)(S * P * c->T), o);
    A.trace = dalloc<unsigned char>((size_t)(S * P * (c->T + 1)), o);
    A.path = dalloc<int>((size_t)(S * 2 * (P + c->T)), o);
    ++A.gen;
}

// The argument checks and the forced sequences of one alignment call, packed per decoder row.
// Host only: nothing is launched and nothing of the context changes, so a refused call leaves
// no trace.  Entry i goes to decoder row w[i].window (osw_align_windows: one row per encoded
// window) or, with `compact`, to row i (osw_session_align, which ignores w[i].window).
struct AlignPack {
    std::vector<int> slot, len, forced, head;        // per decoder row
    std::vector<int> s_len, s_fr, s_w, s_T, s_head;  // per aligned window (slot)
    std::vector<int> win, T, F;                      // AlignBufs::win / T / F of this call
    std::vector<int> row;                            // entry i's decoder row
    int pmax = 0, eot = 0;
};
AlignPack align_pack(osw_ctx* c, int n, const osw_align_window* w, const osw_align_result* r, int nb, bool compact) {
    REQUIRE(n >= 1 && w && r && r->token_frame && r->token_prob, "null align argument");
    const osw_dims& d = c->d;
    const int ctx = d.n_text_ctx, V = d.n_vocab;
    AlignPack P;
    std::vector<int>&slot = P.slot, &len = P.len, &forced = P.forced, &head = P.head;
    slot.assign(nb, -1), len.assign(nb, 0), forced.assign((size_t)nb * ctx, 0), head.assign(nb, 3);
    std::vector<int>&s_len = P.s_len, &s_fr = P.s_fr, &s_w = P.s_w, &s_T = P.s_T, &s_head = P.s_head;
    int& pmax = P.pmax;
    const int eot = P.eot = w[0].eot;
    for (int i = 0; i < n; ++i) {
        osw_align_window a = w[i];
        if (compact) a.window = i;
        P.row.push_back(a.window);
        REQUIRE(a.window >= 0 && a.window < nb, "align: stale window index");
        REQUIRE(slot[a.window] < 0 && len[a.window] == 0, "align: a window appears twice");
        REQUIRE(a.n_tokens >= 0 && (a.n_tokens == 0 || a.tokens), "align: bad token list");
        // language and task both negative: an English-only model's forced sequence
        // [sot, no_timestamps, tokens..., eot] (find_alignment passes the tokenizer's sot_sequence)
        REQUIRE((a.language < 0) == (a.task < 0), "align: language and task are both negative (English-only) or neither");
        const bool en = a.language < 0;
        const int hd = en ? 1 : 3;  // forced positions before <|notimestamps|>, the first kept row
        REQUIRE(a.n_tokens + hd + 2 <= ctx, "align: forced sequence longer than n_text_ctx");
        REQUIRE(a.n_tokens + 1 <= r->stride, "align: result stride too small");
        REQUIRE(a.eot == eot && eot > 0 && eot < V, "align: one <|endoftext|> id per call");
        const int W = a.median_filter_width > 0 ? a.median_filter_width : 7;
        REQUIRE(W % 2 == 1 && W <= ALIGN_MAX_WIDTH, "align: median filter width must be odd and <= 15");
        len[a.window] = -1;  // seen
        if (a.n_tokens == 0) continue;  // no text: no work, empty results
        const int F = std::min(c->T, a.num_frames / 2);
        REQUIRE(F >= 1, "align: num_frames < 2");
        for (int t : {a.sot, en ? a.sot : a.language, en ? a.sot : a.task, a.no_timestamps})
            REQUIRE(t >= 0 && t < V, "align: bad special token");
        int* f = &forced[(size_t)a.window * ctx];
        f[0] = a.sot;
        if (!en) f[1] = a.language, f[2] = a.task;
        f[hd] = a.no_timestamps;
        for (int k = 0; k < a.n_tokens; ++k) {
            REQUIRE(a.tokens[k] >= 0 && a.tokens[k] < eot, "align: text tokens must be below <|endoftext|>");
            f[hd + 1 + k] = a.tokens[k];
        }
        f[hd + 1 + a.n_tokens] = eot;
        const int plen = a.n_tokens + hd + 2;
        head[a.window] = hd;
        s_head.push_back(hd);
        slot[a.window] = (int)P.win.size();
        len[a.window] = plen;
        P.win.push_back(a.window);
        P.T.push_back(a.n_tokens + 1);
        P.F.push_back(F);
        s_len.push_back(plen);
        s_fr.push_back(F);
        s_w.push_back(W);
        s_T.push_back(a.n_tokens + 1);
        pmax = std::max(pmax, plen);
    }
    for (int b = 0; b < nb; ++b) len[b] = std::max(len[b], 0);
    return P;
}

// What the forced pass may write of the decoder's row state, and how its rows find their
// cross-K/V.  osw_align_windows: the context's own state (nothing else is decoding), row b
// attends encoded window b (wmap null, plane 0: the step's own row count).  osw_session_align:
// the pass's own SelState / token / position buffers (AlignBufs), since the context's belong to
// the rows that are still decoding, and row i attends the held slot wmap[i] of `plane` windows.
struct AlignRows {
    bool own;         // AlignBufs::sel / cur_tok / pos instead of the context's
    const int* wmap;  // host, nb entries, or null (the identity)
    int plane;        // cross-K/V windows per plane (c->xkv_windows during the pass)
};

// The core both entry points share: a teacher-forced pass of nb decoder rows through decoder_step
// with the capture armed (rows not aligned are marked finished, which every attention kernel
// skips), then M, DTW and the read-back of P's windows into r.
void align_core(osw_ctx* c, const AlignPack& P, int nb, const AlignRows& rows, int n, const osw_align_window* w,
                osw_align_result* r) {
    const osw_dims& d = c->d;
    const int ctx = d.n_text_ctx, V = d.n_vocab, eot = P.eot, pmax = P.pmax;
    AlignBufs& A = c->al;
    const std::vector<int>&slot = P.slot, &len = P.len, &forced = P.forced, &head = P.head;
    const std::vector<int>&s_len = P.s_len, &s_fr = P.s_fr, &s_w = P.s_w, &s_T = P.s_T, &s_head = P.s_head;
    A.win = P.win;
    A.T = P.T;
    A.F = P.F;
    const int ns = (int)A.win.size();
    if (ns == 0) return;
    align_sync_heads(c);
    const int pstride = (pmax + 15) / 16 * 16;
    align_reserve(c, ns, pstride, nb);
    A.pstride = pstride;
    SelState* const sel = rows.own ? A.sel : c->sel;
    int* const cur_tok = rows.own ? A.cur_tok : c->cur_tok;
    int* const pos = rows.own ? A.pos : c->pos;
    std::vector<SelState> st(nb);
    std::vector<int> first(nb);
    for (int b = 0; b < nb; ++b) {
        st[b] = SelState{};
        st[b].done = slot[b] < 0 ? 1 : 0;
        first[b] = forced[(size_t)b * ctx];
    }
    auto up = [&](void* dst, const void* src, size_t bytes) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    };
    up(A.slot, slot.data(), nb * 4);
    up(A.len, len.data(), nb * 4);
    up(A.forced, forced.data(), forced.size() * 4);
    up(A.slot_len, s_len.data(), ns * 4);
    up(A.slot_frames, s_fr.data(), ns * 4);
    up(A.slot_width, s_w.data(), ns * 4);
    up(A.slot_T, s_T.data(), ns * 4);
    up(A.head, head.data(), nb * 4);
    up(A.slot_head, s_head.data(), ns * 4);
    up(sel, st.data(), nb * sizeof(SelState));
    up(cur_tok, first.data(), nb * 4);
    HIPCHK(hipMemsetAsync(pos, 0, 4, c->stream));
    if (rows.wmap) up(c->xmap_d, rows.wmap, nb * 4);
    AlignCapture cap;
    cap.scores = A.scores; cap.slot = A.slot; cap.len = A.len; cap.layer_heads = A.lh;
    cap.layer_first = A.layer_first.data(); cap.n_heads = A.n_heads; cap.pstride = pstride;
    cap.kc32 = A.kc32; cap.vc32 = A.vc32;
    {
        // decoder_step reads the row state, the step-counter form, the cache strides and the window
        // map off the context: the pass puts its own in place and this guard puts back what it
        // found, on every way out (a decode session goes on with its rows as it left them)
        struct Armed {
            osw_ctx* c;
            SelState* sel = c->sel;
            int *cur_tok = c->cur_tok, *pos = c->pos;
            bool row_pos = c->row_pos;
            int kv_rows = c->kv_rows, xkv_windows = c->xkv_windows;
            const int* xmap = c->xmap;
            ~Armed() {
                c->acap = nullptr;
                c->sel = sel, c->cur_tok = cur_tok, c->pos = pos;
                c->row_pos = row_pos, c->kv_rows = kv_rows, c->xkv_windows = xkv_windows;
                c->xmap = xmap;
            }
        } armed{c};
        c->acap = &cap;
        c->sel = sel, c->cur_tok = cur_tok, c->pos = pos;
        c->row_pos = false;  // one scalar position for the pass's rows
        c->kv_rows = 0;      // kc32 / vc32 hold nb rows per layer
        c->xkv_windows = rows.plane;
        c->xmap = rows.wmap ? c->xmap_d : nullptr;
        auto one_step = [&] {
            decoder_step(c, nb, 1, false, nullptr);
            launch_align_tail(c->logits, nb, V, eot, ctx, pos, A.slot, A.len, A.head, A.forced, A.tokprob, cur_tok, sel,
                              c->stream);
            launch_align_bump(pos, c->stream);
        };
        const int CH = 8;
        hipGraphExec_t ge = nullptr;
        // its own key (no decode key starts below 1), with what shapes the launches: the rows, the
        // buffers' generation, the score stride, the cross-K/V plane stride, whether the rows read
        // it through the map and whose row state they write (the map's contents and the forced
        // tokens are data: another call of the same shape on other slots replays the graph)
        if (c->use_graph && !c->prof_eager && pmax >= CH)
            ge = decode_graph(c, {-77, nb, A.gen, pstride, eot, rows.plane, rows.wmap ? 1 : 0, rows.own ? 1 : 0},
                              one_step, CH);
        for (int steps = 0; steps < pmax;) {
            if (ge && pmax - steps >= CH) {
                HIPCHK(hipGraphLaunch(ge, c->stream));
                steps += CH;
            } else {
                one_step();
                steps += 1;
            }
            HIPCHK(hipGetLastError());
        }
    }
    launch_align_post(A.scores, ns, A.n_heads, pstride, c->T, A.slot_len, A.slot_head, A.slot_frames, A.slot_width, A.stats,
                      A.colstats, A.M, c->stream);
    launch_align_dtw(A.M, (int64_t)pstride * c->T, c->T, 1, ns, A.slot_T, A.slot_frames, A.trace,
                     (int64_t)pstride * (c->T + 1), A.path, pstride + c->T, A.path_len, A.tf, ctx, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<int> tf((size_t)ns * ctx);
    std::vector<float> tp((size_t)ns * ctx);
    HIPCHK(hipMemcpyAsync(tf.data(), A.tf, tf.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tp.data(), A.tokprob, tp.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
        const int sl = slot[P.row[i]];
        if (sl < 0) continue;
        for (int k = 0; k <= w[i].n_tokens; ++k) r->token_frame[(size_t)i * r->stride + k] = tf[(size_t)sl * ctx + k];
        for (int k = 0; k < w[i].n_tokens; ++k) r->token_prob[(size_t)i * r->stride + k] = std::exp((double)tp[(size_t)sl * ctx + k]);
    }
}

// osw_align_windows: over the resident cross-K/V of the last encode call, one decoder row per
// encoded window, on the context's own row state.
void align(osw_ctx* c, int n, const osw_align_window* w, osw_align_result* r) {
    const int nb = c->n_encoded;
    REQUIRE(nb >= 1 && nb <= c->R, "no encoded windows are resident (encode or decode first)");
    REQUIRE(n <= nb, "more windows than the last encode call holds");
    const AlignPack P = align_pack(c, n, w, r, nb, false);
    align_core(c, P, nb, AlignRows{false, nullptr, 0}, n, w, r);
}

// osw_session_align: n held windows of an open session, entry i in session slot slots[i] (distinct,
// below max_batch).  One decoder row per entry; the rows that are still decoding keep their state.
void align_held(osw_ctx* c, int n, const int* slots, const osw_align_window* w, osw_align_result* r) {
    REQUIRE(n >= 1 && n <= c->B, "more windows than the session has slots");
    for (int i = 0; i < n; ++i) REQUIRE(slots[i] >= 0 && slots[i] < c->B, "session slot out of range");
    const AlignPack P = align_pack(c, n, w, r, n, true);
    align_core(c, P, n, AlignRows{true, slots, c->B}, n, w, r);
}

// ------------------------------ mel ----------------------------------------
// Room for n resident clips whose frame counts are in c->mel_off: the per-clip tables and the
// log-mel buffer grow (superseded buffers are freed, which waits for the device, not kept).
void reserve_clips(osw_ctx* c, int n) {
    if (n > c->clips_cap) {
        const int cap = std::max(n, 2 * c->clips_cap);
        dfree(c->offsets, c->owned);
        dfree(c->mel_off_d, c->owned);
        dfree(c->nframes_d, c->owned);
        dfree(c->clip_max, c->owned);
        c->offsets = dalloc<int64_t>(cap + 1, c->owned);
        c->mel_off_d = dalloc<int64_t>(cap + 1, c->owned);
        c->nframes_d = dalloc<int>(cap, c->owned);
        c->clip_max = dalloc<int>(cap, c->owned);
        c->clips_cap = cap;
    }
    if ((size_t)c->mel_off[n] <= c->logmel_cap) return;
    c->logmel_cap = (size_t)c->mel_off[n] + (size_t)c->mel_off[n] / 2;
    dfree(c->logmel, c->owned);
    c->logmel = dalloc<float>(c->logmel_cap, c->owned);
}

void log_mel(osw_ctx* c, const int16_t* pcm, const int64_t* offsets, int n, int on_device, int* nf_out) {
    REQUIRE(n >= 1, "need at least one clip");
    REQUIRE(pcm && offsets, "null pcm/offsets");
    const int n_mels = c->d.n_mels;
    const int64_t total = offsets[n] - offsets[0];
    REQUIRE(total >= 0, "bad offsets");
    std::vector<int64_t> offs(n + 1);
    for (int i = 0; i <= n; ++i) {
        offs[i] = offsets[i] - offsets[0];
        if (i) REQUIRE(offs[i] >= offs[i - 1], "offsets must be non-decreasing");
    }
    c->nframes.assign(n, 0);
    c->mel_off.assign(n + 1, 0);
    int max_nf = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t N = offs[i + 1] - offs[i];
        c->nframes[i] = (int)((N + 160) / 160);
        c->mel_off[i + 1] = c->mel_off[i] + (int64_t)c->nframes[i] * n_mels;
        max_nf = std::max(max_nf, c->nframes[i]);
    }
    reserve_clips(c, n);
    const int16_t* src = pcm + offsets[0];
    if (!on_device) {
        if ((size_t)total > c->pcm_cap) {
            c->pcm_cap = (size_t)total + (size_t)total / 2 + 1;
            dfree(c->pcm, c->owned);
            c->pcm = dalloc<int16_t>(c->pcm_cap, c->owned);
        }
        if (total) HIPCHK(hipMemcpyAsync(c->pcm, src, (size_t)total * 2, hipMemcpyHostToDevice, c->stream));
        src = c->pcm;
    }
    HIPCHK(hipMemcpyAsync(c->offsets, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->mel_off_d, c->mel_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->nframes_d, c->nframes.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    {
        Timed t(c, CL_STAGE_MEL, 0);
        Timed k(c, CL_MEL, (double)total * 2 + (double)c->mel_off[n] * 4);
        launch_mel(src, c->offsets, c->mel_off_d, c->nframes_d, n, max_nf, c->tw400, c->hann, c->flo, c->fcnt,
                   c->foff, c->fw, n_mels, c->logmel, c->clip_max, c->stream);
        HIPCHK(hipGetLastError());
    }
    c->n_clips = n;
    if (nf_out)
        for (int i = 0; i < n; ++i) nf_out[i] = c->nframes[i];
}

// ------------------------------ ingest --------------------------------------
// Per-device state of the context-free ingest entry points (osw_ingest_*): a stream
// and scratch buffers grown on demand, one mutex per device.
struct IngestDev {
    std::mutex mu;
    hipStream_t s = nullptr;
    std::vector<void*> owned;
    int16_t* in = nullptr;
    size_t in_cap = 0;
    int16_t* out = nullptr;
    size_t out_cap = 0;
    float* sums = nullptr;   // [full blocks | tail leaves]
    size_t sums_cap = 0;
    int2* leaves = nullptr;  // tail leaves (<= 128)
    float* taps = nullptr;
    size_t taps_cap = 0;
};
std::mutex g_ingest_mu;
std::map<int, std::unique_ptr<IngestDev>> g_ingest;

IngestDev& ingest_dev(int device) {
    std::lock_guard<std::mutex> lk(g_ingest_mu);
    auto& p = g_ingest[device];
    if (!p) {
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");
        p.reset(new IngestDev());
        DeviceScope dev_scope_((device));
        GateLock gate_(capture_gate());
        HIPCHK(hipStreamCreateWithFlags(&p->s, hipStreamNonBlocking));
        p->leaves = dalloc<int2>(128, p->owned);
    }
    return *p;
}

template <typename T>
T* grow(T*& ptr, size_t& cap, size_t n, std::vector<void*>& owned) {
    if (n > cap) {
        // the caller holds the device mutex and its last call synchronised the stream, so
        // the old buffer is idle: free it rather than keep every superseded size alive
        dfree(ptr, owned);
        cap = n + n / 2 + 1024;
        ptr = dalloc<T>(cap, owned);
    }
    return ptr;
}

// numpy FLOAT_pairwise_sum tree of one block of n elements: leaves in order
void pw_leaves(int64_t off, int64_t n, std::vector<int2>& out) {
    if (n <= 128) {
        out.push_back(make_int2((int)off, (int)n));
        return;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    pw_leaves(off, n2, out);
    pw_leaves(off + n2, n - n2, out);
}
// the same tree combining the leaf sums (float32 adds, left + right)
float pw_combine(int64_t n, const float*& leaf) {
    if (n <= 128) return *leaf++;
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    const float a = pw_combine(n2, leaf);
    const float b = pw_combine(n - n2, leaf);
    return a + b;
}

// numpy: np.mean(np.square(mono(pcm) / 32768)) as float32, bit for bit
float ingest_mean_square(IngestDev& g, const int16_t* pcm, int64_t n, int ch) {
    const int64_t full = n / 8192, tail = n % 8192;
    std::vector<int2> lv;
    if (tail) pw_leaves(0, tail, lv);
    REQUIRE(lv.size() <= 128, "tail leaves");
    const size_t ns = (size_t)full + lv.size();
    grow(g.sums, g.sums_cap, ns + 1, g.owned);
    if (!lv.empty()) HIPCHK(hipMemcpyAsync(g.leaves, lv.data(), lv.size() * sizeof(int2), hipMemcpyHostToDevice, g.s));
    launch_ingest_sumsq(pcm, ch, (int)full, g.leaves, (int)lv.size(), g.sums, g.sums + full, g.s);
    HIPCHK(hipGetLastError());
    std::vector<float> h(ns);
    if (ns) HIPCHK(hipMemcpyAsync(h.data(), g.sums, ns * 4, hipMemcpyDeviceToHost, g.s));
    HIPCHK(hipStreamSynchronize(g.s));
    // np.add.reduce: the 8192-element blocks' pairwise sums added in order
    float acc = 0.f;
    for (int64_t b = 0; b < full; ++b) acc = b == 0 ? h[0] : acc + h[b];
    if (tail) {
        const float* p = h.data() + full;
        const float t = pw_combine(tail, p);
        acc = full ? acc + t : t;
    }
    return acc / (float)n;
}

int64_t upfirdn_output_len(int64_t len_h, int64_t n_in, int64_t up, int64_t down) {
    const int64_t nt = (n_in + (len_h + ((up - len_h % up) % up)) / up - 1) * up;
    return nt / down + (nt % down ? 1 : 0);
}

// The frame of an entry point that runs the pipeline on a context without a session: the context
// locked, its device current, the call counted on the lane's baton, the profile events resolved.
template <typename F>
int lane_call(osw_ctx* c, bool args_ok, const char* null_msg, F&& f) {
    return guard([&] {
        REQUIRE(args_ok, null_msg);
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(!c->sess, "a decode session is open on this context (osw_session_end first)");
        DeviceScope dev_scope_((c->device));
        LaneCall call_(c);
        f();
        resolve_events(c);
    });
}
}  // namespace osw

// ============================== C ABI =======================================
extern "C" {

const char* osw_version(void) { return "osw-hip 0.2 gfx950"; }
const char* osw_last_error(void) { return g_err.c_str(); }

int osw_device_count(int32_t* out) {
    return guard([&] {
        int n = 0;
        HIPCHK(hipGetDeviceCount(&n));
        *out = n;
    });
}

void make_streams(osw_ctx* c) {
    // measured: 4651 / 4625 vs 4748 / 4743 audio-s/s (12 steps, baton on), so opt-in only
    const char* ep = std::getenv("OSW_ENC_PRIO");
    if (!ep || ep[0] != '1') {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        return;
    }
    int lo = 0, hi = 0;  // least and greatest priority (greatest is numerically lowest)
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
    HIPCHK(hipStreamCreateWithPriority(&c->enc_stream, hipStreamNonBlocking, lo));
    HIPCHK(hipEventCreateWithFlags(&c->enc_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->enc_out, hipEventDisableTiming));
}

void destroy_streams(osw_ctx* c) {
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->enc_stream) (void)hipStreamDestroy(c->enc_stream);
    if (c->enc_in) (void)hipEventDestroy(c->enc_in);
    if (c->enc_out) (void)hipEventDestroy(c->enc_out);
}

// a context whose creation failed half-way (c may be null)
static int drop_partial(osw_ctx* c, int rc) {
    if (!c) return rc;
    GateLock gate_(capture_gate());
    for (void* p : c->owned) (void)hipFree(p);
    destroy_streams(c);
    delete c;
    return rc;
}

int osw_create(const osw_dims* dims, int32_t device, int32_t max_batch, osw_ctx** out) {
    osw_ctx* c = nullptr;
    int rc = guard([&] {
        REQUIRE(dims && out, "null argument");
        REQUIRE(max_batch >= 1 && max_batch <= 1024, "max_batch out of range");
        REQUIRE(dims->n_audio_state % 128 == 0 && dims->n_text_state % 128 == 0, "model width must be a multiple of 128");
        REQUIRE(dims->n_audio_state / dims->n_audio_head == 64 && dims->n_text_state / dims->n_text_head == 64,
                "head_dim must be 64");
        // the encoder window: chunk_length s = 1..30 seconds, 50 positions each.  Every such T keeps
        // the last cross-attention key chunk non-empty (decode.hip, XCH); anything else is refused here
        REQUIRE(dims->n_audio_ctx >= 50 && dims->n_audio_ctx <= 1500 && dims->n_audio_ctx % 50 == 0,
                "n_audio_ctx must be 50 * chunk_length, chunk_length 1..30 (50, 100, ..., 1500)");
        REQUIRE((XCHUNKS - 1) * ((dims->n_audio_ctx + XCHUNKS - 1) / XCHUNKS) < dims->n_audio_ctx,
                "n_audio_ctx leaves a cross-attention key chunk empty");
        REQUIRE(dims->n_text_ctx <= 448, "n_text_ctx must be <= 448");
        REQUIRE(dims->n_audio_state == dims->n_text_state, "encoder and decoder width must match");
        REQUIRE(dims->n_audio_state <= 1280, "model width > 1280 unsupported");
        REQUIRE(layernorm_width_ok(dims->n_audio_state),
                "model width must be one of 128, 256, 384, 512, 768, 1024, 1280 (no LayerNorm kernel for 640, 896, 1152)");
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");
        GateLock gate_(capture_gate());  // streams, allocations, kernel attributes
        c = new osw_ctx();
        c->device = device;
        c->d = *dims;
        c->B = max_batch;
        c->R = max_batch * 5;  // room for the reference's beam_size = 5 at full batch
        c->C1 = (dims->n_mels + 63) / 64 * 64;
        c->T = dims->n_audio_ctx;
        c->NF = 2 * c->T;
        if (const char* e = std::getenv("OSW_NO_GRAPH")) c->use_graph = !(e[0] == '1');
        // OSW_BATON_MIN_WINDOWS=n: encoders below n windows skip the baton (0: never skip)
        if (const char* e = std::getenv("OSW_BATON_MIN_WINDOWS")) c->baton_min = atoi(e);
        DeviceScope dev_scope_((device));
        prepare_gemm_kernels();  // no kernel attribute is set lazily beside other lanes' launches
        make_streams(c);
        const char* eb = std::getenv("OSW_ENC_BATON");
        if (!eb || eb[0] != '0') {
            c->baton = std::make_shared<EncBaton>();
            HIPCHK(hipEventCreateWithFlags(&c->baton->ev, hipEventDisableTiming));
        }
        build_weight_table(c);
        setup_mel(c);
        setup_workspace(c);
        HIPCHK(hipStreamSynchronize(c->stream));
        *out = c;
    });
    return rc == OSW_OK ? rc : drop_partial(c, rc);
}

int osw_create_sibling(osw_ctx* parent, int32_t max_batch, osw_ctx** out) {
    osw_ctx* c = nullptr;
    int rc = guard([&] {
        REQUIRE(parent && out, "null argument");
        REQUIRE(max_batch >= 1 && max_batch <= 1024, "max_batch out of range");
        std::lock_guard<std::mutex> lk(parent->mu);
        REQUIRE(parent->finalized, "parent context weights not finalized");
        GateLock gate_(capture_gate());
        c = new osw_ctx();
        c->device = parent->device;
        c->d = parent->d;
        c->B = max_batch;
        c->R = max_batch * 5;
        c->C1 = parent->C1;
        c->T = parent->T;
        c->NF = parent->NF;
        c->use_graph = parent->use_graph;
        c->baton_min = parent->baton_min;
        DeviceScope dev_scope_((c->device));
        make_streams(c);
        c->w = parent->w;          // same device pointers
        c->arena = parent->arena;  // keeps the weights alive past the parent's destroy
        c->siblings = parent->siblings;
        if (c->siblings) c->siblings->fetch_add(1);
        c->baton = parent->baton;
        c->sibling = true;
        c->finalized = true;
        setup_mel(c);
        setup_workspace(c);
        HIPCHK(hipStreamSynchronize(c->stream));
        *out = c;
    });
    return rc == OSW_OK ? rc : drop_partial(c, rc);
}

int osw_destroy(osw_ctx* c) {
    if (!c) return OSW_OK;
    return guard([&] {
        {
            std::lock_guard<std::mutex> lk(c->mu);
            DeviceScope dev_scope_((c->device));
            HIPCHK(hipStreamSynchronize(c->stream));
            GateLock gate_(capture_gate());
            for (auto& e : c->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
            for (auto e : c->ev_free) (void)hipEventDestroy(e);
            for (auto& kv : c->dgraphs) (void)hipGraphExecDestroy(kv.second.first);
            session_destroy(c);
            for (void* p : c->owned) (void)hipFree(p);
            if (c->done_host) (void)hipHostFree(c->done_host);
            destroy_streams(c);
            if (c->sibling && c->siblings) c->siblings->fetch_sub(1);
            c->arena.reset();
        }
        delete c;
    });
}

int osw_set_weight(osw_ctx* c, const char* name, const void* host, int64_t nbytes) {
    return guard([&] {
        REQUIRE(c && name && host, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(!c->sibling, "sibling contexts share their parent's weights (read-only)");
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());  // weight upload (a model loading while another serves)
        Tensor& t = W(c, name);
        const std::string nm(name);
        set_kind(c, nm, t, false);
        if (nm == "enc.conv1.w" && c->C1 != c->d.n_mels) {
            const int64_t De = c->d.n_audio_state, M = c->d.n_mels;
            REQUIRE(nbytes == De * 3 * M * 2, "enc.conv1.w: wrong byte count");
            std::vector<uint16_t> pad((size_t)De * 3 * c->C1, 0);
            const uint16_t* src = (const uint16_t*)host;
            for (int64_t o = 0; o < De; ++o)
                for (int k = 0; k < 3; ++k)
                    std::memcpy(&pad[(o * 3 + k) * c->C1], &src[(o * 3 + k) * M], M * 2);
            HIPCHK(hipMemcpyAsync(t.ptr, pad.data(), pad.size() * 2, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));  // before `pad` goes
        } else {
            REQUIRE(nbytes == t.numel * (t.f16 ? 2 : 4), "tensor " + nm + ": wrong byte count");
            HIPCHK(hipMemcpyAsync(t.ptr, host, nbytes, hipMemcpyHostToDevice, c->stream));
        }
        pack_frag(c, nm);
        HIPCHK(hipStreamSynchronize(c->stream));
        t.set = true;
    });
}

int osw_set_weight_quant(osw_ctx* c, const char* name, const int8_t* q, const float* mult, int64_t n_q,
                      int64_t n_mult) {
    return guard([&] {
        REQUIRE(c && name && q && mult, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(!c->sibling, "sibling contexts share their parent's weights (read-only)");
        DeviceScope dev_scope_((c->device));
        GateLock gate_(capture_gate());
        const std::string nm(name);
        Tensor& t = W(c, nm);
        REQUIRE(t.q8 && t.frag_n, "tensor " + nm + ": int8 weights are accepted for dec.tok and dec.lN.{qkv,o,xq,xo,fc1,fc2}.w");
        REQUIRE(n_q == t.numel && n_mult == t.frag_n, "tensor " + nm + ": wrong element count");
        const int N = t.frag_n, K = t.frag_k;
        REQUIRE(K % 64 == 0, "tensor " + nm + ": int8 fragments need K a multiple of 64");
        for (int n = 0; n < N; ++n) REQUIRE(std::isfinite(mult[n]), "tensor " + nm + ": a multiplier is not finite");
        set_kind(c, nm, t, true);
        std::vector<h16> half((size_t)t.numel);
        for (size_t i = 0; i < half.size(); ++i) half[i] = (h16)(float)q[i];  // exact
        std::vector<void*> tmp;
        int8_t* dq = dalloc<int8_t>((size_t)t.numel, tmp);
        HIPCHK(hipMemcpyAsync(t.ptr, half.data(), half.size() * 2, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(W(c, nm + ".scale").ptr, mult, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dq, q, (size_t)t.numel, hipMemcpyHostToDevice, c->stream));
        launch_frag_pack_q8(dq, N, K, (int8_t*)W(c, nm + ".frag").ptr, c->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        dfree(dq, tmp);
        HIPCHK(e);
        t.set = true;
    });
}

int osw_weight_is_quant(osw_ctx* c, const char* name, int32_t* out) {
    return guard([&] {
        REQUIRE(c && name && out, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        const Tensor& t = W(c, name);
        REQUIRE(t.q8, std::string("tensor ") + name + ": not a matrix that can hold int8 weights");
        *out = t.q8->load() ? 1 : 0;
    });
}

int osw_get_weight(osw_ctx* c, const char* name, void* host, int64_t nbytes) {
    return guard([&] {
        REQUIRE(c && name && host, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        Tensor& t = W(c, name);
        REQUIRE(nbytes == t.numel * (t.f16 ? 2 : 4), std::string("tensor ") + name + ": wrong byte count");
        HIPCHK(hipMemcpyAsync(host, t.ptr, nbytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_init_weight_uniform(osw_ctx* c, const char* name, uint64_t seed, int64_t stream, float scale, float offset,
                            int64_t zero_lo, int64_t zero_hi) {
    return guard([&] {
        REQUIRE(c && name, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(!c->sibling, "sibling contexts share their parent's weights (read-only)");
        DeviceScope dev_scope_((c->device));
        Tensor& t = W(c, name);
        REQUIRE(!(std::string(name) == "enc.conv1.w" && c->C1 != c->d.n_mels),
                "enc.conv1.w needs osw_set_weight when n_mels is not a multiple of 64");
        set_kind(c, name, t, false);
        launch_init_uniform(t.ptr, t.f16, t.numel, hash_stream_key(seed, stream), scale, offset, zero_lo, zero_hi,
                            c->stream);
        HIPCHK(hipGetLastError());
        pack_frag(c, name);
        HIPCHK(hipStreamSynchronize(c->stream));
        t.set = true;
    });
}

int osw_finalize(osw_ctx* c) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        std::string missing;
        for (auto& kv : c->w)
            if (!kv.second.set) missing += kv.first + " ";
        REQUIRE(missing.empty(), "missing tensors: " + missing);
        require_embedding_kind(c);
        c->finalized = true;
    });
}

int osw_log_mel(osw_ctx* c, const int16_t* pcm, const int64_t* offsets, int32_t n_clips, int32_t pcm_on_device,
                int32_t* n_frames) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        log_mel(c, pcm, offsets, n_clips, pcm_on_device, n_frames);
        HIPCHK(hipStreamSynchronize(c->stream));
        resolve_events(c);
    });
}

int osw_get_mel(osw_ctx* c, int32_t clip, float* out, int64_t out_floats) {
    return guard([&] {
        REQUIRE(c && out, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        REQUIRE(clip >= 0 && clip < c->n_clips, "clip out of range");
        const int nf = c->nframes[clip];
        const int64_t n = (int64_t)nf * c->d.n_mels;
        REQUIRE(out_floats >= n, "output buffer too small");
        std::vector<void*> tmp_owned;  // (dalloc / dfree take the capture gate)
        float* tmp = dalloc<float>((size_t)n, tmp_owned);
        launch_mel_normalize(c->logmel, c->mel_off[clip], nf, c->d.n_mels, c->clip_max, clip, tmp, c->stream);
        hipError_t e = hipMemcpyAsync(out, tmp, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        dfree(tmp, tmp_owned);
        HIPCHK(e);
    });
}

int osw_encode_windows(osw_ctx* c, const osw_window* windows, int32_t n) {
    return lane_call(c, c && windows, "null argument", [&] {
        encode(c, windows, n);
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_get_encoder_output(osw_ctx* c, int32_t window, float* out, int64_t out_floats) {
    return guard([&] {
        REQUIRE(c && out, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        REQUIRE(window >= 0 && window < c->n_encoded, "window out of range");
        const int64_t n = (int64_t)c->T * c->d.n_audio_state;
        REQUIRE(out_floats >= n, "output buffer too small");
        std::vector<_Float16> tmp(n);
        HIPCHK(hipMemcpyAsync(tmp.data(), c->E + window * n, n * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < n; ++i) out[i] = (float)tmp[i];
    });
}

int osw_decode_windows(osw_ctx* c, int32_t n, const osw_decode_opts* opts, osw_window_result* res) {
    return lane_call(c, c, "null ctx", [&] { decode(c, n, opts, res); });
}

int osw_decode_window_list(osw_ctx* c, int32_t n, const int32_t* windows, const osw_decode_opts* opts,
                           osw_window_result* res) {
    return lane_call(c, c && windows, "null argument", [&] { decode(c, n, opts, res, windows); });
}

int osw_set_confidences(osw_ctx* c, int32_t enable) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(!c->sess, "a decode session is open on this context (osw_session_end first)");
        c->conf = enable != 0;
        c->conf_valid = false;
        c->conf_res.clear();
    });
}

namespace {
const osw_ctx::ConfResult* conf_result(osw_ctx* c, int32_t i) {
    if (!c->conf || !c->conf_valid)
        throw OswError(OSW_ESTATE, "no confidences recorded (osw_set_confidences(ctx, 1), then a decode call)");
    REQUIRE(i >= 0 && (size_t)i < c->conf_res.size(), "result index out of range");
    return &c->conf_res[i];
}
}  // namespace

int osw_get_token_logprobs(osw_ctx* c, int32_t i, float* cum, int32_t cap, int32_t* n) {
    return guard([&] {
        REQUIRE(c && n, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        const osw_ctx::ConfResult& q = *conf_result(c, i);
        *n = (int32_t)q.cum.size();
        if (!cum) return;  // (query the count)
        REQUIRE(cap >= *n, "output buffer too small");
        std::copy(q.cum.begin(), q.cum.end(), cum);
    });
}

int osw_get_language_probs(osw_ctx* c, int32_t i, float* probs, int32_t n_langs) {
    return guard([&] {
        REQUIRE(c && probs, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        const osw_ctx::ConfResult& q = *conf_result(c, i);
        if (q.lang.empty())
            throw OswError(OSW_ESTATE, "an English-only decode (task_token < 0) records no language probabilities");
        REQUIRE(n_langs == (int32_t)q.lang.size(), "n_langs differs from the decode call's");
        std::copy(q.lang.begin(), q.lang.end(), probs);
    });
}

int osw_detect_language(osw_ctx* c, int32_t n, const osw_decode_opts* opts, float* probs, float* raw_logits) {
    return lane_call(c, c, "null ctx", [&] { detect_language(c, n, opts, probs, raw_logits); });
}

int osw_set_alignment_heads(osw_ctx* c, const int32_t* layer_head_pairs, int32_t n) {
    return guard([&] {
        REQUIRE(c && n >= 0 && (n == 0 || layer_head_pairs), "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(n <= c->d.n_text_layer * c->d.n_text_head, "more alignment heads than the decoder has");
        for (int i = 0; i < n; ++i)
            REQUIRE(layer_head_pairs[2 * i] >= 0 && layer_head_pairs[2 * i] < c->d.n_text_layer &&
                        layer_head_pairs[2 * i + 1] >= 0 && layer_head_pairs[2 * i + 1] < c->d.n_text_head,
                    "alignment head out of range");
        c->al.heads.assign(layer_head_pairs, layer_head_pairs + 2 * (size_t)n);
        c->al.heads_dirty = true;
    });
}

int osw_align_windows(osw_ctx* c, int32_t n, const osw_align_window* w, osw_align_result* res) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(!c->sess, "a decode session is open on this context (osw_session_end first)");
        DeviceScope dev_scope_((c->device));
        LaneCall call_(c);
        align(c, n, w, res);
    });
}

int osw_get_alignment_matrix(osw_ctx* c, int32_t window, float* out, int64_t out_floats, int32_t* T, int32_t* F) {
    return guard([&] {
        REQUIRE(c && T && F, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        const AlignBufs& A = c->al;
        int sl = -1;
        for (size_t i = 0; i < A.win.size(); ++i)
            if (A.win[i] == window) sl = (int)i;
        *T = *F = 0;
        if (sl < 0) return;  // not aligned by the last call (or no text tokens): an empty matrix
        *T = A.T[sl];
        *F = A.F[sl];
        if (!out) return;
        REQUIRE(out_floats >= (int64_t)A.T[sl] * A.F[sl], "output buffer too small");
        HIPCHK(hipMemcpy2DAsync(out, (size_t)A.F[sl] * 4, A.M + (int64_t)sl * A.pstride * c->T, (size_t)c->T * 4,
                                (size_t)A.F[sl] * 4, A.T[sl], hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    });
}

int osw_transcribe_batch(osw_ctx* c, const int16_t* pcm, const int64_t* offsets, int32_t n_clips,
                         int32_t pcm_on_device, const osw_decode_opts* opts, osw_window_result* res) {
    return lane_call(c, c, "null ctx", [&] {
        REQUIRE(n_clips >= 1 && n_clips <= c->B, "n_clips out of range");
        log_mel(c, pcm, offsets, n_clips, pcm_on_device, nullptr);
        std::vector<osw_window> wins(n_clips);
        for (int i = 0; i < n_clips; ++i)
            wins[i] = osw_window{i, 0, std::max(1, std::min(c->NF, c->nframes[i] - 1))};
        encode(c, wins.data(), n_clips);
        decode(c, n_clips, opts, res);
    });
}

int osw_transcribe_refill(osw_ctx* c, const int16_t* pcm, const int64_t* offsets, int32_t n_clips,
                          int32_t pcm_on_device, const osw_decode_opts* opts, osw_window_result* res,
                          int32_t refill_min) {
    return lane_call(c, c, "null ctx", [&] {
        REQUIRE(n_clips >= 1, "n_clips out of range");
        log_mel(c, pcm, offsets, n_clips, pcm_on_device, nullptr);
        decode_refill(c, n_clips, opts, res, refill_min);
    });
}

int osw_set_encoder_baton_min(osw_ctx* c, int32_t min_windows) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        REQUIRE(min_windows >= 0, "min_windows must be >= 0");
        std::lock_guard<std::mutex> lk(c->mu);
        c->baton_min = min_windows;
    });
}

int osw_set_profiling(osw_ctx* c, int32_t enable) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(enable >= 0 && enable <= 2, "profiling mode must be 0, 1 or 2");
        c->prof = enable != 0;
        c->prof_eager = enable == 2;
        c->pf = osw_profile{};
        c->logits_ms = 0;
        c->logits_launches = 0;
    });
}

int osw_get_profile(osw_ctx* c, osw_profile* out) {
    return guard([&] {
        REQUIRE(c && out, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        resolve_events(c);
        *out = c->pf;
    });
}

void* osw_stream(osw_ctx* c) { return c ? (void*)c->stream : nullptr; }

int osw_ingest_mean_square(int32_t device, const int16_t* pcm, int64_t n_frames, int32_t channels, float* out_mean) {
    return guard([&] {
        REQUIRE(pcm && out_mean, "null argument");
        REQUIRE(n_frames >= 1 && channels >= 1 && channels <= 64, "bad PCM shape");
        IngestDev& g = ingest_dev(device);
        std::lock_guard<std::mutex> lk(g.mu);
        DeviceScope dev_scope_((device));
        const size_t n = (size_t)n_frames * channels;
        grow(g.in, g.in_cap, n, g.owned);
        HIPCHK(hipMemcpyAsync(g.in, pcm, n * 2, hipMemcpyHostToDevice, g.s));
        *out_mean = ingest_mean_square(g, g.in, n_frames, channels);
    });
}

int osw_ingest_apply_gain(int32_t device, const int16_t* pcm, int64_t n_frames, int32_t channels, int32_t apply_gain,
                          float gain, int16_t* out) {
    return guard([&] {
        REQUIRE(pcm && out, "null argument");
        REQUIRE(n_frames >= 1 && channels >= 1 && channels <= 64, "bad PCM shape");
        IngestDev& g = ingest_dev(device);
        std::lock_guard<std::mutex> lk(g.mu);
        DeviceScope dev_scope_((device));
        const size_t n = (size_t)n_frames * channels;
        grow(g.in, g.in_cap, n, g.owned);
        grow(g.out, g.out_cap, (size_t)n_frames, g.owned);
        HIPCHK(hipMemcpyAsync(g.in, pcm, n * 2, hipMemcpyHostToDevice, g.s));
        launch_ingest_gain(g.in, n_frames, channels, apply_gain, gain, g.out, g.s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, g.out, (size_t)n_frames * 2, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
    });
}

int osw_ingest_resample(int32_t device, const int16_t* pcm, int64_t n_in, int32_t up, int32_t down, const float* h,
                        int32_t n_h, int16_t* out, int64_t n_out) {
    return guard([&] {
        REQUIRE(pcm && h && out, "null argument");
        REQUIRE(n_in >= 2 && up >= 1 && down >= 1 && n_h >= 1 && (n_h & 1), "bad resample arguments");
        const int64_t want = (n_in * up) / down + ((n_in * up) % down ? 1 : 0);
        REQUIRE(n_out == want, "n_out must be ceil(n_in * up / down)");
        // resample_poly's zero padding of the filter (scipy/signal/_signaltools.py)
        const int64_t half_len = (n_h - 1) / 2;
        const int64_t pre = down - half_len % down;
        const int64_t pre_remove = (half_len + pre) / down;
        int64_t post = 0;
        while (upfirdn_output_len(n_h + pre + post, n_in, up, down) < n_out + pre_remove) ++post;
        const int64_t len_h = n_h + pre + post;
        const int64_t padlen = len_h + (up - len_h % up) % up;
        const int64_t hpp = padlen / up;
        // _pad_h: htf[p * hpp + j] = h_full[(hpp - 1 - j) * up + p]
        std::vector<float> full((size_t)padlen, 0.f), htf((size_t)padlen);
        for (int64_t i = 0; i < n_h; ++i) full[(size_t)(pre + i)] = h[i];
        for (int64_t p = 0; p < up; ++p)
            for (int64_t j = 0; j < hpp; ++j) htf[(size_t)(p * hpp + j)] = full[(size_t)((hpp - 1 - j) * up + p)];
        IngestDev& g = ingest_dev(device);
        std::lock_guard<std::mutex> lk(g.mu);
        DeviceScope dev_scope_((device));
        grow(g.in, g.in_cap, (size_t)n_in, g.owned);
        grow(g.out, g.out_cap, (size_t)n_out, g.owned);
        grow(g.taps, g.taps_cap, (size_t)padlen, g.owned);
        HIPCHK(hipMemcpyAsync(g.in, pcm, (size_t)n_in * 2, hipMemcpyHostToDevice, g.s));
        HIPCHK(hipMemcpyAsync(g.taps, htf.data(), htf.size() * 4, hipMemcpyHostToDevice, g.s));
        launch_ingest_resample(g.in, n_in, g.taps, (int)hpp, up, down, pre_remove, n_out, g.out, g.s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, g.out, (size_t)n_out * 2, hipMemcpyDeviceToHost, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
    });
}

}  // extern "C"
