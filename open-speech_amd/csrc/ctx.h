// Internal header of libosw_hip.so's host units (osw.hip, decode_host.hip, session.hip, debug.hip):
// the context, the error / locking / allocation helpers and what the units call of each other.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <pthread.h>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/osw.h"
#include "common.h"
#include "align.h"
#include "decode.h"
#include "plan.h"
#include "resln.h"

namespace osw {
// launchers from the other translation units
void launch_mel(const int16_t*, const int64_t*, const int64_t*, const int*, int, int, const float2*, const float*,
                const int*, const int*, const int*, const float*, int, float*, int*, hipStream_t);
void launch_mel_window(const float*, const int64_t*, const int*, const int*, const int*, const int*, const int*, int,
                       int, int, int, h16*, hipStream_t);
void launch_mel_normalize(const float*, int64_t, int, int, const int*, int, float*, hipStream_t);
void launch_enc_attn(const h16*, h16*, int, int, int, hipStream_t);
void launch_enc_attn_form(const h16*, h16*, int, int, int, bool eager, bool small, bool pipe, int grid_cap,
                          hipStream_t);
void launch_init_uniform(void*, bool, int64_t, uint64_t, float, float, int64_t, int64_t, hipStream_t);
uint64_t hash_stream_key(uint64_t, int64_t);
void launch_dec_self_attn(const float*, int, const float*, h16*, h16*, const int*, int, int, int, h16*, int64_t,
                          const int*, int, const SelState*, hipStream_t, int pos_row = 0);
void launch_dec_cross_attn(const float*, int, const float*, const h16*, const h16*, int, int, int, int, h16*, int64_t,
                           float*, int*, const SelState*, hipStream_t, const int* wmap = nullptr,
                           bool full = false);  // full: the 6-key / 3-tile chunk forms at any T (debug A/B)
void launch_dec_resid_ln(const float*, int, int, int, const float*, float*, const float*, const float*, h16*, int64_t,
                         const h16*, const float*, const int*, const int*, int, int, hipStream_t, int pos_row = 0,
                         const float* tok_scale = nullptr);  // tok_scale: ResLnArgs::tok_scale (int8 embedding)
void launch_dec_reduce_gelu(const float*, int, int, int, const float*, h16*, int64_t, hipStream_t);
void launch_ingest_sumsq(const int16_t*, int, int, const int2*, int, float*, float*, hipStream_t);
void launch_ingest_gain(const int16_t*, int64_t, int, int, float, int16_t*, hipStream_t);
void launch_ingest_resample(const int16_t*, int64_t, const float*, int, int, int, int64_t, int64_t, int16_t*,
                            hipStream_t);

extern thread_local std::string g_err;  // osw_last_error()'s text (osw.hip)

// Stream-capture errors are refusals of an operation, not device faults: the context and
// the GPU stay usable, so they get their own code (OSW_ECAPTURE) and the serving layer does
// not fail the GPU over on them (runner.py).
inline int hip_code(hipError_t e) {
    switch (e) {
        case hipErrorStreamCaptureUnsupported:
        case hipErrorStreamCaptureInvalidated:
        case hipErrorStreamCaptureMerge:
        case hipErrorStreamCaptureUnmatched:
        case hipErrorStreamCaptureUnjoined:
        case hipErrorStreamCaptureIsolation:
        case hipErrorStreamCaptureImplicit:
        case hipErrorCapturedEvent:
        case hipErrorStreamCaptureWrongThread:
            return OSW_ECAPTURE;
        default:
            return OSW_EHIP;
    }
}
#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess)                                                                      \
            throw OswError(hip_code(e_), std::string(#x) + ": " + hipGetErrorString(e_) + " @" +   \
                                             std::to_string(__LINE__));                            \
    } while (0)

template <typename F>
int guard(F&& f) {
    try {
        f();
        return OSW_OK;
    } catch (const OswError& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "out of host memory";
        return OSW_ENOMEM;
    } catch (const std::exception& e) {
        g_err = e.what();
        return OSW_ESTATE;
    }
}

struct Tensor {
    void* ptr = nullptr;
    int64_t numel = 0;
    bool f16 = true;
    bool set = false;
    // a decoder matrix the skinny GEMM streams: N x K, with a fragment-major copy in the
    // tensor "<name>.frag" (GemmArgs::Wf), repacked whenever the matrix is written
    int frag_n = 0, frag_k = 0;
    // such a matrix holds int8 weights (osw_set_weight_quant): this tensor is fp16(q), "<name>.scale"
    // its row multipliers and "<name>.frag" the int8 fragments (GemmArgs::Wq).  Per matrix; the
    // flag is shared with sibling contexts, as the arena is (null: not a matrix kind with a copy)
    std::shared_ptr<std::atomic<int>> q8;
};

// The capture gate (one per process).  While a stream is being captured into a hipGraph,
// HIP refuses every operation that would make the legacy (null) stream depend on it
// ("operation would make the legacy stream depend on a capturing blocking stream") and
// invalidates the capture; its capture-status check spans every stream of the process, so
// a synchronous hipMemcpy / hipMemset, hipMalloc / hipFree, hipDeviceSynchronize or stream
// creation on one lane's thread breaks a sibling lane's capture (GPUTEST_r05).  So:
//   * a decode graph is captured only while holding this gate (decode_graph);
//   * every allocation, free, stream / pinned-buffer creation or destruction and every
//     implicitly synchronising call takes it too (dalloc / dfree, osw_create,
//     osw_create_sibling, osw_destroy, osw_set_weight, osw_get_mel, osw_debug_gemm, ingest);
//   * everything else a call does runs on the context's own non-blocking stream
//     (hipMemcpyAsync / hipMemsetAsync + hipStreamSynchronize), never on the legacy stream.
// Recursive: osw_create holds it across setup_workspace's dalloc calls.  Lock order: a
// context's mu, then the encoder baton's mu, then this gate; nothing is locked under it.
std::recursive_mutex& capture_gate();  // (defined once, in osw.hip)
using GateLock = std::lock_guard<std::recursive_mutex>;

template <typename T>
T* dalloc(size_t n, std::vector<void*>& owned) {
    GateLock gate_(capture_gate());
    void* p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) throw OswError(OSW_ENOMEM, "hipMalloc " + std::to_string(n * sizeof(T)) + " B failed");
    owned.push_back(p);
    return (T*)p;
}

// Frees a buffer dalloc'd into `owned` (implicitly synchronises the device; growth only).
template <typename T>
void dfree(T*& p, std::vector<void*>& owned) {
    if (!p) return;
    for (auto it = owned.begin(); it != owned.end(); ++it)
        if (*it == (void*)p) {
            owned.erase(it);
            break;
        }
    GateLock gate_(capture_gate());
    (void)hipFree(p);
    p = nullptr;
}

// Makes `device` current for one C-ABI call and restores the caller's device after it:
// a host thread that calls into the library and then issues its own HIP / torch work
// stays on the GPU it was on.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int device) {
        HIPCHK(hipGetDevice(&prev));
        if (prev != device) HIPCHK(hipSetDevice(device));
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

struct EventPair {
    hipEvent_t a, b;
    int cls;
    double work;
};

// Encoder baton, shared by a context and its siblings (the lanes of one GPU): each
// lane's encoder waits on the GPU for the previous lane's encoder to finish.  The
// encoder is MFMA-bound and fills every CU, so two encoders side by side only
// time-slice; lanes started together would otherwise stay in lock-step (all encoders,
// then all decoders) and never overlap an encoder with the others' HBM/latency-bound
// decoders, which is what the lanes are for.
struct EncBaton {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    bool recorded = false;
    // calls in flight over the contexts sharing this baton (LaneCall): with more than one,
    // the encoder GEMMs leave a quarter of the CUs to the other lanes (GemmArgs::share_cus)
    std::atomic<int> in_call{0};
    ~EncBaton() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

// Word-timestamp alignment state of a context (osw_align_windows): the device buffers,
// sized lazily for the largest call so far, and what the last call aligned
struct AlignBufs {
    int *slot = nullptr, *len = nullptr, *forced = nullptr, *lh = nullptr;  // per decoder row; {head, idx} pairs
    int *slot_len = nullptr, *slot_frames = nullptr, *slot_width = nullptr, *slot_T = nullptr, *path_len = nullptr;
    int *head = nullptr, *slot_head = nullptr;  // per row / per slot: forced positions before the first kept row
    int *tf = nullptr, *path = nullptr;
    float *tokprob = nullptr /* log-probabilities */, *scores = nullptr, *stats = nullptr, *colstats = nullptr, *M = nullptr;
    unsigned char* trace = nullptr;
    float *kc32 = nullptr, *vc32 = nullptr;  // fp32 self-K/V cache of the forced pass, [L][cap_rows][H][ctx][64]
    // osw_session_align: the pass's own row state ([R] each; one scalar position), so that the
    // session's decoding rows keep theirs (c->sel / c->cur_tok / c->pos)
    SelState* sel = nullptr;
    int *cur_tok = nullptr, *pos = nullptr;
    int cap_slots = 0, cap_pstride = 0, cap_heads = 0, cap_rows = 0;
    int64_t gen = 0;                // bumps when a buffer moves or the heads change (decode-graph key)
    std::vector<int> heads;         // the caller's (layer, head) pairs; empty: the default set
    std::vector<int> layer_first;   // [L + 1] offsets into lh (pairs), heads grouped by layer
    int n_heads = 0;
    bool heads_dirty = true;
    std::vector<int> win, T, F;     // last call: window index (osw_session_align: entry index), rows and frames of each slot
    int pstride = 0;
};
}  // namespace osw

using namespace osw;

struct osw_ctx {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    osw_dims d{};
    int B = 0;    // max windows per call
    int R = 0;    // decoder row capacity (windows x beam hypotheses)
    int C1 = 0;   // conv1 input channels padded to a multiple of 64
    int T = 0;    // encoder positions per window: d.n_audio_ctx = 50 * chunk_length (1500 at the 30 s default)
    int NF = 0;   // mel frames per window, 2 * T
    std::vector<void*> owned;
    std::map<std::string, Tensor> w;
    std::shared_ptr<void> arena;  // weight arena, shared with sibling contexts (osw_create_sibling)
    // live sibling contexts on this arena (shared by all of them; osw_create_sibling / osw_destroy):
    // their decode graphs cannot be seen from here, so a matrix keeps its kind while any exists
    std::shared_ptr<std::atomic<int>> siblings;
    bool sibling = false;         // weights belong to another context: read-only here
    bool finalized = false;
    std::shared_ptr<EncBaton> baton;  // shared with sibling contexts; null: encoders not serialised
    int baton_min = 9;                // encoders of fewer windows skip the baton (osw_set_encoder_baton_min)
    bool share_cus = false;           // this call's encoder GEMMs leave CUs to sibling lanes
    // OSW_ENC_PRIO=1: the encoder runs on its own low-priority stream, the decoder on a
    // high-priority `stream` (measured slower: the default is one stream per lane)
    hipStream_t enc_stream = nullptr;
    hipEvent_t enc_in = nullptr, enc_out = nullptr;

    // mel constants
    float2* tw400 = nullptr;
    float* hann = nullptr;
    int *flo = nullptr, *fcnt = nullptr, *foff = nullptr;
    float* fw = nullptr;
    // resident mel
    int16_t* pcm = nullptr;
    size_t pcm_cap = 0;
    int64_t* offsets = nullptr;
    int64_t* mel_off_d = nullptr;
    int* nframes_d = nullptr;
    int* clip_max = nullptr;
    int clips_cap = 0;
    float* logmel = nullptr;
    size_t logmel_cap = 0;
    int n_clips = 0;
    std::vector<int> nframes;
    std::vector<int64_t> mel_off;

    // encoder workspace
    int* win = nullptr;  // [3][B]
    h16 *X1 = nullptr, *H1 = nullptr, *Xn = nullptr, *QKV = nullptr, *O = nullptr, *Hf = nullptr, *E = nullptr,
        *XKV = nullptr;
    float* X = nullptr;
    int n_encoded = 0;
    bool row_pos = false;             // decode_refill / sessions: per-row step counters (pos[row])
    int kv_rows = 0;                  // sessions: self-K/V cache rows per layer (0: the step's row count)
    int xkv_windows = 0;              // sessions: cross-K/V windows per layer (0: the step's windows)
    struct Session* sess = nullptr;   // an open decode session (osw_session_*)
    struct ClipStore* cstore = nullptr;  // decode sessions' resident clip log-mels (created on first use)
    int* slot_d = nullptr;            // encode into slots: window -> decoder row
    int* refill_pack = nullptr;       // decode_refill: rows to admit {row, budget, prompt}

    // decoder workspace.  xdn / dattn / dh (the GEMM operands) are hi/lo fp16 pairs:
    // the lo halves sit R rows after the hi halves (lo_off below)
    float* xd = nullptr;
    float* xd2 = nullptr;      // second residual buffer of the fused small-batch step (ping-pong)
    h16 *xdn = nullptr, *dqkv = nullptr, *dattn = nullptr, *dq = nullptr, *dh = nullptr, *kc = nullptr, *vc = nullptr;
    float* logits = nullptr;
    int *cur_tok = nullptr, *pos = nullptr, *tokens = nullptr, *prompt = nullptr, *done = nullptr;
    unsigned* supmask = nullptr;
    SelState* sel = nullptr;   // per decoder row
    void* selp = nullptr;      // per-row vocabulary-slice partial stats
    void* selp1 = nullptr;     // batch-1 fused selection: one record per logits workgroup
    int* anc = nullptr;        // beam: [R][ctx] row whose cache slot holds position p of this hypothesis
    int* btok = nullptr;       // beam: [B][ctx] best finished hypothesis per window
    BeamWin* bwin = nullptr;   // beam: [B]
    void* bcand = nullptr;     // beam: [R][SEL_SPLIT][2 lists][2*MAX_BEAM] candidates (beam_slice_body)
    int* done_host = nullptr;  // pinned
    float* part = nullptr;     // split-K partial slabs of the decoder GEMMs
    float* part2 = nullptr;    // second slab buffer of the fused small-batch step (<= PRO_ROWS rows)
    float* xws = nullptr;      // cross-attention per-chunk partials [R][H][XCHUNKS][XPART]
    int* xticket = nullptr;    // cross-attention arrival tickets [B][H] (zero between launches)
    int* xmap_d = nullptr;     // osw_decode_window_list: [B] row group -> encoded window (a fixed address: graphs replay it)
    const int* xmap = nullptr; // xmap_d while a list decode runs, else null (the identity)
    int* tail_ticket = nullptr; // split-K GEMM tails (ProArgs::tail_ticket)
    int* sel_arrive = nullptr; // select arrival counters: rows finalised + per-row slice tickets (zero between launches)
    int* budget = nullptr;     // per-row token budgets (osw_decode_opts::token_budget)
    unsigned long long* seed_d = nullptr;  // sampling seed of the current decode call
    // Retry sessions (osw_session_retries), allocated by the context's first one: the rows' sampling
    // state (SelParams::row_inv_temp / row_seed), the admission / retry pack, and for a greedy
    // session with best_of > 1 (xsplit) the second cross-attention launch's done-flag copies,
    // row -> slot map and tickets (decode_host.hip step_cross_attn)
    float* row_inv_temp = nullptr;             // [R]
    unsigned long long* row_seed = nullptr;    // [R]
    int* retry_pack = nullptr;                 // [B][RETRY_PACK_HEAD + n_text_ctx]
    SelState *xdone_single = nullptr, *xdone_group = nullptr;  // [R]
    int* xrow_map = nullptr;                   // [R]
    int* xrow_ticket = nullptr;                // [R][H] (zero between launches)
    bool xsplit = false;                       // the open session is a greedy retry session with best_of > 1
    int64_t part_floats = 0;

    // decode-step graphs (CH steps per replay), one per key (batch rows, prompt length,
    // decode options); a small LRU so a serving mix of batch sizes replays instead of
    // re-capturing (the streaming collator meets batches of 1..4 windows)
    std::map<std::vector<int64_t>, std::pair<hipGraphExec_t, uint64_t>> dgraphs;
    uint64_t dgraph_tick = 0;
    bool capturing = false;
    bool prof_eager = false;  // profiling mode 2: decode steps launched eagerly so the per-kernel timers see them
    bool use_graph = true;

    // confidences (osw_set_confidences): per-token cumulative log-probs and language probabilities
    bool conf = false;
    float* lp_hist = nullptr;     // [R][n_text_ctx] (SelParams::lp_hist)
    float* best_lp = nullptr;     // beam: [B][n_text_ctx] (SelParams::best_lp)
    float* lang_probs = nullptr;  // [B][<= LANG_CAP] (SelParams::lang_probs; osw_detect_language writes it too)
    struct ConfResult {
        std::vector<float> cum, lang;
    };
    std::vector<ConfResult> conf_res;  // results of the last result-producing call, in its order
    bool conf_valid = false;

    AlignBufs al;
    const AlignCapture* acap = nullptr;  // set while osw_align_windows / osw_session_align steps the decoder

    // profiling
    bool prof = false;
    osw_profile pf{};
    // the fused step's logits GEMM (batch-1: with the selection in its epilogue), per launch, while
    // profiling (osw_debug_logits_profile; tools/q8_bench.py)
    double logits_ms = 0;
    int64_t logits_launches = 0;
    std::vector<EventPair> evs;
    std::vector<hipEvent_t> ev_free;
};

namespace osw {

void trace_graph(const osw_ctx* c, const char* what);
hipEvent_t get_ev(osw_ctx* c);

// class ids for per-launch accounting
enum { CL_ENC_GEMM = 1, CL_ENC_ATTN = 2, CL_MEL = 3, CL_XATTN = 4, CL_LOGITS = 5, CL_STAGE_MEL = 10, CL_STAGE_ENC = 11,
       CL_STAGE_XKV = 12, CL_STAGE_DEC = 13 };

struct Timed {
    osw_ctx* c;
    EventPair p{};
    bool on;
    Timed(osw_ctx* c_, int cls, double work) : c(c_), on(c_->prof && !c_->capturing) {
        if (!on) return;
        p.a = get_ev(c);
        p.b = get_ev(c);
        p.cls = cls;
        p.work = work;
        HIPCHK(hipEventRecord(p.a, c->stream));
    }
    ~Timed() {
        if (!on) return;
        if (hipEventRecord(p.b, c->stream) == hipSuccess) c->evs.push_back(p);
    }
};

// A transcription call in flight on a context: counted on the baton its siblings share,
// and decides whether this call's encoder GEMMs share the CUs (another lane is busy too)
struct LaneCall {
    osw_ctx* c;
    explicit LaneCall(osw_ctx* c_) : c(c_) {
        c->share_cus = c->baton && c->baton->in_call.fetch_add(1) > 0;
    }
    ~LaneCall() {
        if (c->baton) c->baton->in_call.fetch_sub(1);
    }
};

// osw.hip
void resolve_events(osw_ctx* c);
Tensor& W(osw_ctx* c, const std::string& n);
const h16* WH(osw_ctx* c, const std::string& n);
const float* WF(osw_ctx* c, const std::string& n);
const h16* WFR(osw_ctx* c, const std::string& n);
bool is_q8(osw_ctx* c, const std::string& n);  // the matrix holds int8 weights (osw_set_weight_quant)
// the weight operands of a decoder GEMM on matrix n: W, Wf, and for int8 weights Wq and wscale
void gemm_weights(osw_ctx* c, const std::string& n, GemmArgs& g);
void require_embedding_kind(osw_ctx* c);  // an int8 dec.tok needs an int8 dec.l0.qkv.w (osw.hip)
const float* tok_scale(osw_ctx* c);  // dec.tok's row multipliers when it is int8, else nullptr
GemmArgs gemm_plain(const h16* A, int64_t lda, const h16* Wt, const float* bias, int M, int N, int K, void* C,
                    int64_t ldc, int epi);
bool skinny_ok(const GemmArgs& g);
void run_gemm(osw_ctx* c, const GemmArgs& g0, int cls);
void encoder_layer(osw_ctx* c, int i, int nb);
std::vector<int> pack_windows(osw_ctx* c, const osw_window* wins, int n);
void encode(osw_ctx* c, const osw_window* wins, int n, const int* slots = nullptr);
void reserve_clips(osw_ctx* c, int n);
// osw_session_align's pass: entry i of w aligned over the cross-K/V of session slot slots[i]
void align_held(osw_ctx* c, int n, const int* slots, const osw_align_window* w, osw_align_result* r);

// decode_host.hip
bool decoder_step(osw_ctx* c, int nb, int group, bool gather, const SelFuse* sf = nullptr);
hipGraphExec_t decode_graph(osw_ctx* c, const std::vector<int64_t>& key, const std::function<void()>& one_step,
                            int CH);
void decode(osw_ctx* c, int nb, const osw_decode_opts* o, osw_window_result* r, const int32_t* windows = nullptr);
void detect_language(osw_ctx* c, int nb, const osw_decode_opts* o, float* probs, float* raw);
void decode_refill(osw_ctx* c, int n_clips, const osw_decode_opts* o, osw_window_result* r, int refill_min);
// Host copies of what the rows hold.  Tokens and cumulative log-probs come per window in beam
// mode (the best finished hypothesis: btok / best_lp) and per row otherwise (tokens / lp_hist).
struct Readback {
    std::vector<SelState> st;
    std::vector<BeamWin> bw;
    std::vector<int> toks;
    std::vector<float> cum, lang;
    std::vector<int> rtoks;   // a beam retry session: the rows' own tokens / cumulative log-probs,
    std::vector<float> rcum;  // read when a sampling slot finished
};
void bind_plan(osw_ctx* c, DecodePlan& p, const osw_decode_opts* o);
void plan_select(osw_ctx* c, const DecodePlan& p, int rows, int windows);
void run_chunk(osw_ctx* c, const DecodePlan& p, int rows, int windows, int CH, bool graph,
               const SelFuse* sf = nullptr);
std::vector<int> finished_windows(osw_ctx* c, const DecodePlan& p, int rows, int windows,
                                  const std::function<bool(int)>& live, Readback& rb,
                                  const std::function<int(int)>& armed = nullptr);
size_t best_sample(const Readback& rb, size_t first, int n, float length_penalty);
void park_rows(osw_ctx* c, int R);
void write_window(osw_ctx* c, const DecodePlan& p, osw_window_result* r, size_t out, const Readback& rb, size_t row,
                  size_t win, bool sampled = false);

// session.hip
void retry_reserve(osw_ctx* c);     // the context's retry-session buffers (osw_ctx::row_inv_temp ...), once
void session_destroy(osw_ctx* c);  // the open session and the clip store, at osw_destroy
}  // namespace osw
