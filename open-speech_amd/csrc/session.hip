// Decode sessions (osw_session_*): the resident clip store, admission, the chunked step and the
// session entry points of the C ABI.
#include "ctx.h"
#include "slots.h"

// ------------------------------ decode sessions ------------------------------
// Continuous batching (osw_session_*, include/osw.h): c->B window slots, `beam` decoder rows
// each (rows slot*beam .. slot*beam+beam-1), per-row step counters (pos[row]), per-row prompts
// (SelState::plen, prompt rows of n_text_ctx ints).  The self-K/V cache and the cross-K/V
// keep their full-capacity layouts (ctx->kv_rows, ctx->xkv_windows), so a step may cover only
// the rows up to the highest occupied slot.  Windows are admitted between chunks of CH steps:
// their log-mel, their encoder straight into the slots' cross-K/V, then the rows' reset.
// With osw_session_hold a finished window keeps its slot (slots.h) until osw_session_align has
// run the word-timing pass over its cross-K/V or osw_session_release has let it go.
// With osw_session_retries a slot keeps max(beam, best_of) rows, and osw_session_retry sends a held
// window back to decoding in its slot with best_of sampled rows (temperature fallback), beside
// slots that go on at temperature 0; the rows' sampling state is data the selection kernels read
// (SelParams::row_inv_temp / row_seed), so arming a retry replays the session's decode graph.
struct SessionWin {
    int64_t clip;            // ClipStore key (a private key < 0 for a window that brought its own PCM)
    std::vector<int> prefix;
    osw_session_window w;
};

// The log-mel of every clip a decode session holds windows of, computed ONCE when the clip's
// first window is added and kept on the device until the caller releases the clip
// (osw_session_release_clip) or the session ends: a long file's later windows are staged
// from it (a device-to-device copy of the window's frames and the clip's max) instead of
// re-uploading the whole clip and recomputing its log-mel per window.  One
// arena per context, first-fit spans, grown by doubling (the old contents keep their
// offsets); per-clip maxima in a slot array.  Lives as long as the context.
struct ClipStore {
    struct Clip {
        int64_t off = 0;   // first float of the clip's [nframes][n_mels] log10 mel in the arena
        int nframes = 0;
        int slot = 0;      // its max (ordered int) at maxv[slot]
        bool priv = false; // registered for one window (no caller key): released at its admission
    };
    std::map<int64_t, Clip> clips;
    int64_t next_priv = -2;
    float* arena = nullptr;
    int64_t cap = 0;                   // floats
    std::map<int64_t, int64_t> spans;  // free spans: offset -> length (coalesced)
    int* maxv = nullptr;
    int slots_cap = 0;
    std::vector<int> free_slots;
    int64_t* hdr = nullptr;            // one clip's mel launch: pcm offsets {0, n}, mel_off {off, end}, nframes
};
struct Session {
    DecodePlan plan;  // session-wide: beam, start sequence (plan.P positions), max_length, history rules
    int W = 0;
    SlotTable slots;  // free / decoding / held, and the tags
    std::deque<SessionWin> queue;
    int64_t steps = 0;
    // retry sessions (plan.best_of > 0): per slot, the admitted window's prompt (its language
    // position as admitted: -1 for a detected language) and token budget, kept for its retries,
    // and how many of the slot's rows sample now (0: the temperature-0 mode)
    struct SlotWin {
        std::vector<int> prompt;
        int budget = 0;
    };
    std::vector<SlotWin> win;
    std::vector<int> armed;
};

namespace {
using osw::SelState;

ClipStore& clip_store(osw_ctx* c) {
    if (!c->cstore) {
        c->cstore = new ClipStore();
        c->cstore->hdr = dalloc<int64_t>(6, c->owned);
    }
    return *c->cstore;
}

int64_t store_alloc(osw_ctx* c, ClipStore& cs, int64_t len) {
    for (auto it = cs.spans.begin(); it != cs.spans.end(); ++it)
        if (it->second >= len) {
            const int64_t off = it->first, rest = it->second - len;
            cs.spans.erase(it);
            if (rest) cs.spans[off + len] = rest;
            return off;
        }
    // grow: a bigger arena holding the old one's contents at the same offsets
    const int64_t ncap = std::max<int64_t>(std::max<int64_t>(2 * cs.cap, cs.cap + len),
                                           (int64_t)std::max(4, c->B) * (c->NF + 1) * c->d.n_mels);
    float* na = dalloc<float>((size_t)ncap, c->owned);
    if (cs.arena) {
        HIPCHK(hipMemcpyAsync(na, cs.arena, (size_t)cs.cap * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        dfree(cs.arena, c->owned);
    }
    int64_t tail_off = cs.cap, tail_len = ncap - cs.cap;
    if (!cs.spans.empty()) {
        auto last = std::prev(cs.spans.end());
        if (last->first + last->second == cs.cap) {
            tail_off = last->first;
            tail_len += last->second;
            cs.spans.erase(last);
        }
    }
    cs.arena = na;
    cs.cap = ncap;
    cs.spans[tail_off + len] = tail_len - len;
    if (tail_len == len) cs.spans.erase(tail_off + len);
    return tail_off;
}

void store_free(ClipStore& cs, int64_t off, int64_t len) {
    auto it = cs.spans.emplace(off, len).first;
    if (it != cs.spans.begin()) {
        auto prev = std::prev(it);
        if (prev->first + prev->second == off) {
            prev->second += it->second;
            cs.spans.erase(it);
            it = prev;
        }
    }
    auto next = std::next(it);
    if (next != cs.spans.end() && it->first + it->second == next->first) {
        it->second += next->second;
        cs.spans.erase(next);
    }
}

// Registers a clip: its PCM uploaded and its log-mel computed into the store (on the stream)
void store_add(osw_ctx* c, int64_t key, const int16_t* pcm, int64_t n, bool priv) {
    ClipStore& cs = clip_store(c);
    REQUIRE(n >= 0, "bad clip length");
    const int n_mels = c->d.n_mels;
    ClipStore::Clip cl;
    cl.nframes = (int)((n + 160) / 160);
    cl.priv = priv;
    cl.off = store_alloc(c, cs, (int64_t)cl.nframes * n_mels);
    if (cs.free_slots.empty()) {
        const int ncap = std::max(64, 2 * cs.slots_cap);
        int* nm = dalloc<int>(ncap, c->owned);
        if (cs.maxv) {
            HIPCHK(hipMemcpyAsync(nm, cs.maxv, (size_t)cs.slots_cap * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            dfree(cs.maxv, c->owned);
        }
        for (int i = ncap - 1; i >= cs.slots_cap; --i) cs.free_slots.push_back(i);
        cs.maxv = nm;
        cs.slots_cap = ncap;
    }
    cl.slot = cs.free_slots.back();
    cs.free_slots.pop_back();
    if ((size_t)n > c->pcm_cap) {
        c->pcm_cap = (size_t)n + (size_t)n / 2 + 1;
        dfree(c->pcm, c->owned);
        c->pcm = dalloc<int16_t>(c->pcm_cap, c->owned);
    }
    if (n) HIPCHK(hipMemcpyAsync(c->pcm, pcm, (size_t)n * 2, hipMemcpyHostToDevice, c->stream));
    const int64_t h[6] = {0, n, cl.off, cl.off + (int64_t)cl.nframes * n_mels, cl.nframes, 0};
    HIPCHK(hipMemcpyAsync(cs.hdr, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    {
        Timed t(c, CL_MEL, (double)n * 2 + (double)cl.nframes * n_mels * 4);
        // (nframes as the low int of hdr[4]: little-endian)
        launch_mel(c->pcm, cs.hdr, cs.hdr + 2, (const int*)(cs.hdr + 4), 1, cl.nframes, c->tw400, c->hann, c->flo,
                   c->fcnt, c->foff, c->fw, n_mels, cs.arena, cs.maxv + cl.slot, c->stream);
        HIPCHK(hipGetLastError());
    }
    cs.clips[key] = cl;
}

void store_release(osw_ctx* c, int64_t key) {
    if (!c->cstore) return;
    ClipStore& cs = *c->cstore;
    auto it = cs.clips.find(key);
    if (it == cs.clips.end()) return;
    store_free(cs, it->second.off, (int64_t)it->second.nframes * c->d.n_mels);
    cs.free_slots.push_back(it->second.slot);
    cs.clips.erase(it);
}

void store_clear(osw_ctx* c) {
    if (!c->cstore) return;
    std::vector<int64_t> keys;
    for (auto& kv : c->cstore->clips) keys.push_back(kv.first);
    for (int64_t k : keys) store_release(c, k);
}

void session_begin(osw_ctx* c, const osw_decode_opts* o) {
    REQUIRE(o, "null decode options");
    REQUIRE(!c->sess, "a decode session is already open on this context");
    REQUIRE(!(o->temperature > 0.f), "decode sessions decode at temperature 0 (greedy or beam search)");
    REQUIRE(o->beam_size <= 5, "decode sessions hold beam_size <= 5 (5 decoder rows per window slot)");
    auto S = std::make_unique<Session>();
    S->plan = DecodePlan(DecodeMode::Session, o, c->d);
    S->W = c->B;
    bind_plan(c, S->plan, o);  // (osw_set_confidences is refused while the session is open)
    const int R = S->W * S->plan.beam;
    c->xsplit = false;
    park_rows(c, R);
    HIPCHK(hipMemsetAsync(c->budget, 0, (size_t)R * 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    S->slots = SlotTable(S->W);
    c->row_pos = true;
    c->kv_rows = c->R;
    c->xkv_windows = c->B;
    c->sess = S.release();
}


void session_end(osw_ctx* c) {
    store_clear(c);
    delete c->sess;
    c->sess = nullptr;
    c->row_pos = false;
    c->kv_rows = 0;
    c->xkv_windows = 0;
    c->n_encoded = 0;
    c->xsplit = false;
}

// osw_session_retries: from here on the session keeps max(beam, best_of) rows per slot and binds
// the rows' sampling state; nothing was admitted yet, so every row is re-parked under the new
// row count.  The buffers are the context's, allocated by its first retry session.
void session_retries(osw_ctx* c, int best_of) {
    Session* S = c->sess;
    if (!S) throw OswError(OSW_ESTATE, "osw_session_retries: no decode session open");
    if (!S->slots.hold || S->slots.added)
        throw OswError(OSW_ESTATE, "osw_session_retries: valid after osw_session_hold(1) and before the first osw_session_add");
    REQUIRE(best_of >= 1 && best_of <= 5, "osw_session_retries: 1 <= best_of <= 5");
    retry_reserve(c);
    S->plan.enable_retries(best_of);
    const int group = S->plan.group, R = S->W * group;
    REQUIRE(R <= c->R, "decoder rows");
    S->plan.bind(c->seed_d, c->budget, c->conf, c->lp_hist, c->best_lp, c->lang_probs, c->row_inv_temp, c->row_seed);
    S->win.assign(S->W, Session::SlotWin{});
    S->armed.assign(S->W, 0);
    std::vector<int> map(c->R);
    for (int r = 0; r < c->R; ++r) map[r] = std::min(r / group, c->B - 1);
    HIPCHK(hipMemcpyAsync(c->xrow_map, map.data(), map.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->row_inv_temp, 0, (size_t)c->R * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->row_seed, 0, (size_t)c->R * 8, c->stream));
    park_rows(c, R);
    HIPCHK(hipMemsetAsync(c->budget, 0, (size_t)R * 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->xsplit = S->plan.beam == 1 && group > 1;
}

// One pack entry of launch_session_retry_rows: `active` rows of `slot` start at step 0 of `prompt`,
// sampling at 1 / temperature `inv_temp` with `seed` (0: the temperature-0 mode)
void retry_pack_entry(int* e, int slot, const std::vector<int>& prompt, int budget, int active, float inv_temp,
                      uint64_t seed) {
    e[0] = slot;
    e[1] = (int)prompt.size();
    e[2] = budget;
    e[3] = active;
    e[4] = float_bits(inv_temp);
    e[5] = (int)(uint32_t)seed;
    e[6] = (int)(uint32_t)(seed >> 32);
    e[7] = 0;
    std::copy(prompt.begin(), prompt.end(), e + RETRY_PACK_HEAD);
}

void launch_retry_pack(osw_ctx* c, const Session* S, const std::vector<int>& pack, int k) {
    const int ctx = c->d.n_text_ctx, beam = S->plan.beam;
    HIPCHK(hipMemcpyAsync(c->retry_pack, pack.data(), pack.size() * 4, hipMemcpyHostToDevice, c->stream));
    launch_session_retry_rows(c->retry_pack, k, RETRY_PACK_HEAD + ctx, S->plan.group, ctx, ctx, c->prompt, c->budget,
                              c->cur_tok, c->pos, c->sel, beam > 1 ? c->anc : nullptr, beam > 1 ? c->bwin : nullptr,
                              c->row_inv_temp, c->row_seed, c->stream);
    HIPCHK(hipGetLastError());
}

// osw_session_retry: every check before any change or launch; then the slots go held -> decoding
// and their rows are reset and armed.  The cross-K/V stays and the encoder does not run.
void session_retry(osw_ctx* c, int n, const osw_retry_window* e) {
    Session* S = c->sess;
    REQUIRE(S, "no decode session open");
    if (S->plan.best_of <= 0) throw OswError(OSW_ESTATE, "osw_session_retry: the session has no retries (osw_session_retries)");
    REQUIRE(n >= 1 && e, "null retry argument");
    std::vector<int64_t> tags(n);
    for (int i = 0; i < n; ++i) {
        REQUIRE(std::isfinite(e[i].temperature) && e[i].temperature > 0.f, "osw_session_retry: temperature must be finite and > 0");
        REQUIRE(S->plan.ss.english || (e[i].language_token >= 0 && e[i].language_token < c->d.n_vocab),
                "osw_session_retry: language token outside the vocabulary");
        tags[i] = e[i].tag;
    }
    const std::vector<int> slots = S->slots.held_slots(n, tags.data());
    const int ctx = c->d.n_text_ctx, ps = RETRY_PACK_HEAD + ctx;
    std::vector<int> pack((size_t)n * ps, 0);
    for (int i = 0; i < n; ++i) {
        std::vector<int> prompt = S->win[slots[i]].prompt;
        // the language attempt 0 reported (nothing is detected again)
        if (!S->plan.ss.english) prompt[prompt.size() - S->plan.ss.tail + 1] = e[i].language_token;
        retry_pack_entry(&pack[(size_t)i * ps], slots[i], prompt, S->win[slots[i]].budget, S->plan.best_of,
                         1.f / e[i].temperature, e[i].seed);
    }
    S->slots.retry(slots);
    for (int s : slots) S->armed[s] = S->plan.best_of;
    launch_retry_pack(c, S, pack, n);
}

void session_add(osw_ctx* c, const int16_t* pcm, const int64_t* offsets, int n, const osw_session_window* w) {
    Session* S = c->sess;
    REQUIRE(S, "no decode session open");
    REQUIRE(pcm && offsets && w && n >= 0, "null argument");
    // every window is checked before any is queued or any clip registered
    ClipStore& cs = clip_store(c);
    std::map<int64_t, int64_t> fresh;  // caller keys registered by this call -> window index
    for (int i = 0; i < n && S->slots.hold; ++i) {  // held windows are named by tag: one window per tag
        REQUIRE(!S->slots.tag_in_use(w[i].tag), "hold: a window of this tag is still decoding or held");
        for (const SessionWin& q : S->queue) REQUIRE(q.w.tag != w[i].tag, "hold: a window of this tag is queued");
        for (int j = 0; j < i; ++j) REQUIRE(w[j].tag != w[i].tag, "hold: a tag appears twice");
    }
    for (int i = 0; i < n; ++i) {
        REQUIRE(offsets[i + 1] >= offsets[i], "offsets must not decrease");
        REQUIRE(w[i].segment_size >= 1 && w[i].seek >= 0, "empty window");
        REQUIRE(w[i].n_prefix >= 0 && (w[i].n_prefix == 0 || w[i].prefix), "bad prefix");
        REQUIRE(w[i].n_prefix + S->plan.P < S->plan.max_len, "prompt longer than max_length");
        int64_t samples = offsets[i + 1] - offsets[i];
        if (w[i].clip >= 0) {
            auto it = cs.clips.find(w[i].clip);
            if (it != cs.clips.end()) {
                samples = -1;
                REQUIRE(w[i].seek < it->second.nframes, "window seek out of range");
            } else if (fresh.count(w[i].clip)) {
                samples = offsets[fresh[w[i].clip] + 1] - offsets[fresh[w[i].clip]];
            } else {
                fresh[w[i].clip] = i;
            }
        }
        // (log_mel's frame count: one frame per 160 samples, plus one)
        if (samples >= 0) REQUIRE(w[i].seek < (int)((samples + 160) / 160), "window seek out of range");
    }
    S->slots.note_add();
    for (int i = 0; i < n; ++i) {
        SessionWin q;
        if (w[i].clip >= 0) {
            if (!cs.clips.count(w[i].clip)) store_add(c, w[i].clip, pcm + offsets[i], offsets[i + 1] - offsets[i], false);
            q.clip = w[i].clip;
        } else {
            q.clip = cs.next_priv--;
            store_add(c, q.clip, pcm + offsets[i], offsets[i + 1] - offsets[i], true);
        }
        q.prefix.assign(w[i].prefix, w[i].prefix + w[i].n_prefix);
        q.w = w[i];
        q.w.prefix = nullptr;
        S->queue.push_back(std::move(q));
    }
}

void session_admit(osw_ctx* c, int refill_min) {
    Session* S = c->sess;
    const std::vector<int> free_slots = S->slots.free_slots();  // (never a held one)
    const int queued = (int)S->queue.size();
    if (!queued || free_slots.empty()) return;
    if (S->slots.decoding > 0 && (int)free_slots.size() < std::min(std::max(1, refill_min), queued)) return;
    const int k = std::min((int)free_slots.size(), queued);
    // the admitted windows' frames, staged from their clips' resident log-mel as k "clips"
    // (window i = its frames [seek, seek + min(segment, frames - seek)) and its clip's max), so
    // encode() sees the layout log_mel() writes
    ClipStore& cs = clip_store(c);
    const int n_mels = c->d.n_mels;
    c->nframes.assign(k, 0);
    c->mel_off.assign(k + 1, 0);
    std::vector<int64_t> src_off(k);
    std::vector<int> src_slot(k);
    for (int i = 0; i < k; ++i) {
        const SessionWin& q = S->queue[i];
        const ClipStore::Clip& cl = cs.clips.at(q.clip);
        const int len = std::max(1, std::min(std::min(q.w.segment_size, c->NF), cl.nframes - q.w.seek));
        c->nframes[i] = len;
        c->mel_off[i + 1] = c->mel_off[i] + (int64_t)len * n_mels;
        src_off[i] = cl.off + (int64_t)q.w.seek * n_mels;
        src_slot[i] = cl.slot;
    }
    reserve_clips(c, k);
    for (int i = 0; i < k; ++i) {
        HIPCHK(hipMemcpyAsync(c->logmel + c->mel_off[i], cs.arena + src_off[i],
                              (size_t)(c->mel_off[i + 1] - c->mel_off[i]) * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->clip_max + i, cs.maxv + src_slot[i], 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(c->mel_off_d, c->mel_off.data(), (k + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->nframes_d, c->nframes.data(), k * 4, hipMemcpyHostToDevice, c->stream));
    c->n_clips = k;
    const int ctx = c->d.n_text_ctx, beam = S->plan.beam, ps = 3 + ctx;
    const bool retries = S->plan.best_of > 0;
    std::vector<int> rpack(retries ? (size_t)k * (RETRY_PACK_HEAD + ctx) : 0, 0);
    std::vector<osw_window> wins(k);
    std::vector<int> slots(k), pack((size_t)k * ps, 0);
    for (int i = 0; i < k; ++i) {
        const SessionWin& q = S->queue[i];
        const int slot = free_slots[i];
        wins[i] = osw_window{i, 0, q.w.segment_size};
        slots[i] = slot;
        int* e = &pack[(size_t)i * ps];
        const int np = (int)q.prefix.size();
        e[0] = slot;
        e[1] = np + S->plan.P;
        e[2] = q.w.token_budget;
        for (int j = 0; j < np; ++j) e[3 + j] = q.prefix[j];
        S->plan.ss.tokens(q.w.language_token, e + 3 + np);
        if (retries) {  // kept for the window's retries; its rows start in the temperature-0 mode
            Session::SlotWin& sw = S->win[slot];
            sw.prompt.assign(e + 3, e + 3 + e[1]);
            sw.budget = q.w.token_budget;
            S->armed[slot] = 0;
            retry_pack_entry(&rpack[(size_t)i * (RETRY_PACK_HEAD + ctx)], slot, sw.prompt, sw.budget, beam, 0.f, 0);
        }
    }
    encode(c, wins.data(), k, slots.data());
    for (int i = 0; i < k; ++i) S->slots.admit(free_slots[i], S->queue[i].w.tag);
    if (retries) {
        launch_retry_pack(c, S, rpack, k);
    } else {
        HIPCHK(hipMemcpyAsync(c->refill_pack, pack.data(), pack.size() * 4, hipMemcpyHostToDevice, c->stream));
        launch_session_rows(c->refill_pack, k, ps, beam, ctx, ctx, c->prompt, c->budget, c->cur_tok, c->pos, c->sel,
                            beam > 1 ? c->anc : nullptr, beam > 1 ? c->bwin : nullptr, c->stream);
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < k; ++i) {
        if (S->queue.front().clip < 0) store_release(c, S->queue.front().clip);  // (its frames were staged)
        S->queue.pop_front();
    }
}

// returns the number of finished windows written to r / tags
int session_step(osw_ctx* c, int max_chunks, int refill_min, osw_window_result* r, int64_t* tags, int cap) {
    Session* S = c->sess;
    REQUIRE(S, "no decode session open");
    REQUIRE(r && r->tokens && r->n_tokens && r->sum_logprob && r->no_speech_prob && r->language && tags,
            "null result argument");
    REQUIRE(cap >= S->W, "cap must hold every slot (max_batch)");
    // OSW_SESSION_CHUNK: decoder steps between admission points.  4 since round 6 (config 5
    // 177-179 vs 171-172 calls/s, REST mixed continuous 74-75 vs 73 calls/s with p50 117-122
    // vs 136-141 ms: profiles/r06_zcd_session_chunk_ab.txt); 8 before (decode()'s chunk)
    static const int CH = [] {
        const char* e = getenv("OSW_SESSION_CHUNK");
        return e ? std::max(1, std::min(64, atoi(e))) : 4;
    }();
    const DecodePlan& plan = S->plan;
    const int group = plan.group;  // (== beam unless the session has retries)
    const bool retries = plan.best_of > 0;
    int done = 0;
    c->conf_res.clear();
    c->conf_valid = c->conf;
    // every slot held and windows waiting: nothing to launch and nothing to wait for until the
    // caller aligns or releases (osw_session_align / osw_session_release)
    if (S->slots.stalled((int)S->queue.size())) return 0;
    if (max_chunks == 0) {  // admission only: the queued windows' encoder, waited for
        session_admit(c, refill_min);
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
    Readback rb;
    for (int chunk = 0; chunk < max_chunks && done == 0; ++chunk) {
        session_admit(c, refill_min);
        if (S->slots.decoding == 0) break;
        int hi = S->slots.decoding_end();
        if (hi > 4) hi = std::min(S->W, (hi + 3) / 4 * 4);  // (fewer graph shapes; idle slots' rows are finished)
        const int nb = hi * group;
        run_chunk(c, plan, nb, hi, CH, c->use_graph && !c->prof_eager);
        S->steps += CH;
        std::function<int(int)> armed;
        if (retries) armed = [&](int i) { return S->armed[i]; };
        for (int slot : finished_windows(c, plan, nb, hi, [&](int i) { return S->slots.is_decoding(i); }, rb, armed)) {
            // a sampling slot reports its best row (decode()'s best_of rule)
            const int n_armed = retries ? S->armed[slot] : 0;
            const size_t row = n_armed > 0 ? best_sample(rb, (size_t)slot * group, n_armed, plan.sp.length_penalty)
                                           : (size_t)slot * group;
            write_window(c, plan, r, done, rb, row, slot, n_armed > 0);
            tags[done] = S->slots.finish(slot);  // (hold: the slot and its cross-K/V stay)
            ++done;
        }
    }
    c->pf.decode_steps = S->steps;
    return done;
}
}  // namespace

namespace osw {
void retry_reserve(osw_ctx* c) {
    if (c->row_inv_temp) return;
    const int ctx = c->d.n_text_ctx, H = c->d.n_text_head;
    c->row_inv_temp = dalloc<float>(c->R, c->owned);
    c->row_seed = dalloc<unsigned long long>(c->R, c->owned);
    c->retry_pack = dalloc<int>((size_t)c->B * (RETRY_PACK_HEAD + ctx), c->owned);
    c->xdone_single = dalloc<SelState>(c->R, c->owned);
    c->xdone_group = dalloc<SelState>(c->R, c->owned);
    c->xrow_map = dalloc<int>(c->R, c->owned);
    c->xrow_ticket = dalloc<int>((size_t)c->R * H, c->owned);
    HIPCHK(hipMemsetAsync(c->xdone_single, 0, (size_t)c->R * sizeof(SelState), c->stream));
    HIPCHK(hipMemsetAsync(c->xdone_group, 0, (size_t)c->R * sizeof(SelState), c->stream));
    HIPCHK(hipMemsetAsync(c->xrow_ticket, 0, (size_t)c->R * H * 4, c->stream));
}

void session_destroy(osw_ctx* c) {
    delete c->sess;
    c->sess = nullptr;
    delete c->cstore;
    c->cstore = nullptr;
}
}  // namespace osw

extern "C" {

int osw_session_begin(osw_ctx* c, const osw_decode_opts* opts) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        session_begin(c, opts);
    });
}

int osw_session_add(osw_ctx* c, const int16_t* pcm, const int64_t* offsets, int32_t n,
                    const osw_session_window* windows) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        session_add(c, pcm, offsets, n, windows);
    });
}

int osw_session_step(osw_ctx* c, int32_t max_chunks, int32_t refill_min, osw_window_result* res, int64_t* tags_out,
                     int32_t cap, int32_t* n_done, int32_t* n_active, int32_t* n_queued) {
    return guard([&] {
        REQUIRE(c && n_done && n_active && n_queued, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        LaneCall call_(c);
        *n_done = session_step(c, std::max(0, max_chunks), refill_min, res, tags_out, cap);
        *n_active = c->sess->slots.decoding;
        *n_queued = (int32_t)c->sess->queue.size();
        resolve_events(c);
    });
}

int osw_session_hold(osw_ctx* c, int32_t enable) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->sess) throw OswError(OSW_ESTATE, "osw_session_hold: no decode session open");
        c->sess->slots.set_hold(enable != 0);
    });
}

int osw_session_retries(osw_ctx* c, int32_t best_of) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        session_retries(c, best_of);
    });
}

int osw_session_retry(osw_ctx* c, int32_t n, const osw_retry_window* entries) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        session_retry(c, n, entries);
    });
}

int osw_session_align(osw_ctx* c, int32_t n, const int64_t* tags, const osw_align_window* w, osw_align_result* res) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(c->sess, "no decode session open");
        REQUIRE(n >= 1 && tags && w && res, "null align argument");
        DeviceScope dev_scope_((c->device));
        LaneCall call_(c);
        // every check (tags here, the windows in align_held) comes before the first launch and
        // before any slot changes: a refused call leaves the session as it was
        const std::vector<int> slots = c->sess->slots.held_slots(n, tags);
        align_held(c, n, slots.data(), w, res);
        c->sess->slots.take_held(slots);
    });
}

int osw_session_release(osw_ctx* c, int32_t n, const int64_t* tags) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(c->sess, "no decode session open");
        c->sess->slots.take_held(c->sess->slots.held_slots(n, tags));
    });
}

int osw_session_release_clip(osw_ctx* c, int64_t clip) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        REQUIRE(c->sess, "no decode session open");
        REQUIRE(clip >= 0, "clip keys are >= 0");
        for (const SessionWin& q : c->sess->queue)
            REQUIRE(q.clip != clip, "a queued window still reads this clip");
        store_release(c, clip);
    });
}

int osw_session_end(osw_ctx* c) {
    return guard([&] {
        REQUIRE(c, "null ctx");
        std::lock_guard<std::mutex> lk(c->mu);
        DeviceScope dev_scope_((c->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        session_end(c);
    });
}

}  // extern "C"
