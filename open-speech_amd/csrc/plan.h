// The decode plan: everything the host side of token decoding derives from osw_decode_opts, in
// one place for the three decode paths (decode, decode_refill, decode sessions; decode_host.hip
// and session.hip).  Host only: no HIP call and nothing of osw_ctx, so a stand-alone program
// checks it (tests/cpp/decode_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "error.h"
#include "seltypes.h"

namespace osw {

enum class DecodeMode { Batch, Refill, Session };

// The start sequence.  osw_decode_opts::task_token < 0 selects an English-only model's:
// <|startoftranscript|> alone (faster-whisper's Tokenizer.sot_sequence for a model that is not
// multilingual), so a prompt is [prefix..., sot(, no_timestamps)] and the language fields of
// the options are ignored; otherwise [prefix..., sot, language, task(, no_timestamps)].
struct StartSeq {
    bool english = false;
    int tail = 3;     // prompt positions from <|startoftranscript|> to the end
    int n_langs = 0;  // language tokens the selection and the confidences see (0: English-only)
    int sot = 0, task = 0, no_ts = -1;  // its tokens (no_ts < 0: timestamps on, no <|notimestamps|>)
    // e[0 .. tail): the start sequence with `lang` as its language token (-1: detect)
    void tokens(int lang, int* e) const {
        *e++ = sot;
        if (!english) *e++ = lang, *e++ = task;
        if (no_ts >= 0) *e = no_ts;
    }
    StartSeq() = default;
    explicit StartSeq(const osw_decode_opts* o)
        : english(o->task_token < 0), tail((english ? 1 : 3) + (o->without_timestamps ? 1 : 0)),
          n_langs(english ? 0 : o->n_langs), sot(o->sot), task(o->task_token),
          no_ts(o->without_timestamps ? o->no_timestamps : -1) {}
};

inline int32_t float_bits(float f) {
    int32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// osw_decode_opts::repetition_penalty / no_repeat_ngram_size as the decode paths use them:
// off values normalised (penalty 1, size 0), so equal rules give equal decode-graph keys.
struct HistRules {
    bool on = false;
    float penalty = 1.f;
    int ngram = 0;
    HistRules() = default;
    HistRules(const osw_decode_opts* o, const osw_dims& d)
        : penalty((o->repetition_penalty > 0.f && o->repetition_penalty != 1.f) ? o->repetition_penalty : 1.f),
          ngram(std::max(0, o->no_repeat_ngram_size)) {
        on = history_rules_on(penalty, ngram);
        REQUIRE(!on || d.n_text_ctx <= 448, "the history rules hold at most 448 sampled tokens");
    }
};

// Built once per decode call (Batch, Refill) or once per session.  n_pre: the prefix tokens before
// <|startoftranscript|> (Batch only; sessions carry per-row prefixes in SelState::plen).
// n_encoded > 0: a mapped decode (osw_decode_window_list) over that many encoded windows.
// retries > 0 (Session only, osw_session_retries): the session's best_of; a slot then keeps
// max(beam, best_of) decoder rows, so a held window can decode again there with sampling.
struct DecodePlan {
    DecodeMode mode = DecodeMode::Batch;
    StartSeq ss;
    HistRules hr;
    bool sampling = false;
    int n_pre = 0, n_encoded = 0;
    int beam = 1;   // hypotheses per window
    int group = 1;  // decoder rows per window (beam hypotheses or best_of samples)
    int best_of = 0;  // retry sessions: sampled rows of a retried window (0: a session without retries)
    int P = 0, max_len = 0, max_tok = 0;
    SelParams sp{};
    std::vector<unsigned> mask;  // suppress_tokens as a bitmask over the vocabulary

    DecodePlan() = default;
    DecodePlan(DecodeMode m, const osw_decode_opts* o, const osw_dims& d, int n_prefix = 0, int mapped_n_encoded = 0,
               int retries = 0)
        : mode(m), n_encoded(mapped_n_encoded) {
        const int V = d.n_vocab, ctx = d.n_text_ctx;
        const int wide = std::max(1, o->beam_size);
        const float patience = o->patience > 0.f ? o->patience : 1.f;
        // what differs per mode.  Batch: temperature > 0 is faster-whisper's sampling branch (beam 1
        // and best_of independent sampled rows per window, the best one kept), else beam search
        // or greedy.  Refill is greedy whatever the options say; sessions decode at temperature 0.
        SelParams& s = sp;
        switch (mode) {
            case DecodeMode::Batch:
                sampling = o->temperature > 0.f;
                n_pre = n_prefix;
                REQUIRE(n_pre >= 0 && (n_pre == 0 || o->prefix_tokens), "bad prefix");
                beam = sampling ? 1 : wide;
                group = sampling ? std::max(1, o->best_of) : beam;
                REQUIRE(group <= MAX_BEAM, "beam_size / best_of > 8");
                s.num_hyp = std::max(1, o->num_hypotheses);
                s.max_cand = std::max(1, (int)std::lround(beam * patience));
                s.inv_temp = sampling ? 1.f / o->temperature : 0.f;
                s.pos_row = 0;
                break;
            case DecodeMode::Refill:
                beam = group = 1;
                s.num_hyp = s.max_cand = 1;
                s.inv_temp = 0.f;
                s.pos_row = 1;
                break;
            case DecodeMode::Session:
                beam = group = wide;
                s.num_hyp = std::max(1, o->num_hypotheses);
                s.max_cand = std::max(1, (int)std::lround(beam * patience));
                s.inv_temp = 0.f;
                s.pos_row = 1;
                break;
        }
        REQUIRE(V <= SEL_SPLIT * 4096, "vocabulary too large for the selection kernels");
        hr = HistRules(o, d);
        ss = StartSeq(o);
        P = n_pre + ss.tail;
        max_len = std::min(o->max_length > 0 ? o->max_length : ctx, ctx);
        REQUIRE(P < max_len, "prompt longer than max_length");
        max_tok = std::max(1, max_len - P);
        // the prompt buffer's row: the call's one prompt length, or room for any per-row prefix
        s.pstride = mode == DecodeMode::Session ? ctx : P;
        s.prompt_len = P; s.sot_pos = n_pre; s.lang_pos = n_pre + 1; s.max_length = max_len;
        // with timestamps an English-only row samples at <|startoftranscript|>
        s.tail = ss.tail; s.sot_last = ss.english && !o->without_timestamps;
        s.V = V; s.eot = o->eot; s.no_speech = o->no_speech; s.no_ts = o->no_timestamps; s.tb = o->timestamp_begin;
        s.blank = o->blank; s.first_lang = ss.english ? 0 : o->first_lang; s.n_langs = ss.n_langs;
        s.suppress_blank = o->suppress_blank; s.with_ts = o->without_timestamps ? 0 : 1;
        s.max_init_ts = o->max_initial_timestamp_index;
        s.beam = beam;
        s.length_penalty = o->length_penalty;
        s.lp_stride = ctx; s.lp_group = group;
        has_budget = mode == DecodeMode::Session || o->token_budget != nullptr;
        if (retries) enable_retries(retries);
        mask.assign((V + 31) / 32, 0u);
        for (int i = 0; i < o->n_suppress; ++i) {
            const int t = o->suppress_tokens[i];
            if (t >= 0 && t < V) mask[t >> 5] |= 1u << (t & 31);
        }
    }

    // osw_session_retries: the session keeps max(beam, best_of) rows per slot from here on
    void enable_retries(int n) {
        REQUIRE(mode == DecodeMode::Session, "only a decode session retries windows in place");
        REQUIRE(n >= 1 && n <= 5, "a retry session samples 1 to 5 rows per window (best_of)");
        best_of = n;
        group = std::max(beam, n);
        sp.lp_group = group;
    }

    // The device side: the seed word, the per-row budgets (kept only when the call has budgets;
    // a session always has them, per window) and, with confidences on, where they are recorded
    // (all null when off, so the kernels store nothing; English-only: no language distribution).
    // row_inv_temp / row_seed: a retry session's per-row sampling state (SelParams), else null.
    void bind(const unsigned long long* seed, const int* budget, bool conf, float* lp_hist, float* best_lp,
              float* lang_probs, const float* row_inv_temp = nullptr, const unsigned long long* row_seed = nullptr) {
        REQUIRE((best_of > 0) == (row_inv_temp != nullptr) && (best_of > 0) == (row_seed != nullptr),
                "row temperatures belong to a retry session");
        sp.row_inv_temp = row_inv_temp;
        sp.row_seed = row_seed;
        sp.seed = seed;
        sp.budget = has_budget ? budget : nullptr;
        if (!conf) return;
        REQUIRE(ss.english || (sp.n_langs >= 1 && sp.n_langs <= LANG_CAP), "confidences hold at most 128 languages");
        sp.lp_hist = lp_hist;
        sp.best_lp = best_lp;
        sp.lang_probs = ss.english ? nullptr : lang_probs;
    }

    // The decode-graph key of CH steps over `rows` decoder rows: the mode, every scalar of
    // SelParams in declaration order (floats by their bits), then what else shapes a captured
    // launch.  The seed, the mask's contents, language tokens, prefix contents, budget values and
    // the window map are data the launches read through fixed addresses: not in the key.  A retry
    // session's launches differ (the row-temperature selection): one more word, only there, so
    // every other key is what it was; which rows sample, at what temperature and seed is data.
    std::vector<int64_t> key(int rows, int CH) const {
        static_assert(sizeof(SelParams) == 168, "SelParams changed: put every new scalar field into the key below");
        const SelParams& s = sp;
        std::vector<int64_t> k{(int64_t)mode,
                s.prompt_len, s.sot_pos, s.lang_pos, s.max_length, s.pstride, s.tail, s.sot_last, s.V, s.eot,
                s.no_speech, s.no_ts, s.tb, s.blank, s.first_lang, s.n_langs, s.suppress_blank, s.with_ts,
                s.max_init_ts, s.beam, s.num_hyp, s.max_cand, float_bits(s.length_penalty), float_bits(s.inv_temp),
                s.pos_row, s.lp_stride, s.lp_group,
                rows, group, n_pre, CH, float_bits(hr.penalty), hr.ngram, s.budget != nullptr, s.lp_hist != nullptr,
                n_encoded};
        if (s.row_inv_temp) k.push_back(best_of);
        return k;
    }

private:
    bool has_budget = false;
};

}  // namespace osw
