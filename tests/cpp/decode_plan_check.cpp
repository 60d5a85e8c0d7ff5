// Host-only check of csrc/plan.h (the decode plan): walks a grid of decode options across the three
// decode modes and asserts (1) every SelParams field against a table written out here per mode,
// (2) that the graph key moves with every option that reaches SelParams or a launch argument and
// with nothing that is data, (3) that keys of different modes / mapped and unmapped / English-only
// and multilingual calls never meet, (4) the mask's capacity and the prompt-length check.
// No HIP call; built and run by tests/test_decode_plan_cpu.py with ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <tuple>

#include "plan.h"

using namespace osw;

static int g_checks = 0;
#define CHECK(c)                                                                \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case.c_str()); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)
static std::string g_case;

static const osw_dims DIMS = {80, 1500, 384, 6, 4, 51865, 448, 384, 6, 4};
static const int32_t SUPPRESS[] = {1, 2, 7, 50257, 51864};
static const int32_t PREFIX[] = {50361, 11, 12, 13, 14, 50361, 21, 22, 23, 24};  // 2 windows x 5
static const int32_t BUDGET[] = {9, 17};
// stand-ins for the context's device buffers: bound, never dereferenced
static unsigned long long SEED_WORD;
static int BUDGET_BUF[16];
static float LP_HIST[1], BEST_LP[1], LANG_PROBS[1];

struct Case {
    int kind;  // 0 greedy, 1 beam 2, 2 beam 5, 3 sampling best_of 1, 4 sampling best_of 3
    bool no_ts, english, hist, conf, budget;
    int n_pre, n_encoded;
    float patience, length_penalty;
    int max_length;
};

static osw_decode_opts opts_of(const Case& k) {
    osw_decode_opts o{};
    o.task_token = k.english ? -1 : 50359;
    o.language_token = 50259;
    o.suppress_blank = 1;
    o.without_timestamps = k.no_ts;
    o.max_initial_timestamp_index = 50;
    o.max_length = k.max_length;
    o.suppress_tokens = SUPPRESS;
    o.n_suppress = 5;
    o.eot = 50257; o.sot = 50258; o.sot_prev = 50361; o.no_speech = 50362; o.no_timestamps = 50363;
    o.timestamp_begin = 50364; o.blank = 220; o.first_lang = 50259; o.n_langs = 99;
    o.prefix_tokens = PREFIX;
    o.n_prefix = k.n_pre;
    o.beam_size = k.kind == 1 ? 2 : k.kind == 2 ? 5 : 1;
    o.patience = k.patience;
    o.length_penalty = k.length_penalty;
    o.num_hypotheses = 1;
    o.temperature = k.kind >= 3 ? 0.5f : 0.f;
    o.best_of = k.kind == 4 ? 3 : 1;
    o.seed = 1234;
    o.token_budget = k.budget ? BUDGET : nullptr;
    o.repetition_penalty = k.hist ? 1.25f : 0.f;
    o.no_repeat_ngram_size = k.hist ? 3 : 0;
    return o;
}

static bool admits(DecodeMode m, const Case& k) {
    if (m == DecodeMode::Batch) return true;
    if (k.n_pre || k.n_encoded || k.kind >= 3) return false;  // no call-wide prefix, no window map, no sampling
    return m == DecodeMode::Session || k.kind == 0;            // refill is greedy
}

static DecodePlan plan_of(DecodeMode m, const Case& k, const osw_decode_opts& o) {
    DecodePlan p(m, &o, DIMS, m == DecodeMode::Batch ? o.n_prefix : 0, k.n_encoded);
    p.bind(&SEED_WORD, BUDGET_BUF, k.conf, LP_HIST, BEST_LP, LANG_PROBS);
    return p;
}

static int lround_cand(int beam, float patience) { return std::max(1, (int)std::lround(beam * patience)); }

// (1) what decode(), decode_refill() and session_begin() set, field by field
static void check_params(DecodeMode m, const Case& k, const osw_decode_opts& o, const DecodePlan& p) {
    const SelParams& s = p.sp;
    const int ctx = DIMS.n_text_ctx;
    const int tail = k.english ? (k.no_ts ? 2 : 1) : (k.no_ts ? 4 : 3);
    const int max_len = k.max_length > 0 ? std::min(k.max_length, ctx) : ctx;
    const int wide = k.kind == 1 ? 2 : k.kind == 2 ? 5 : 1;
    // every mode
    CHECK(s.tail == tail && p.ss.tail == tail);
    CHECK(s.max_length == max_len && p.max_len == max_len);
    CHECK(s.sot_last == (k.english && !k.no_ts ? 1 : 0));
    CHECK(s.first_lang == (k.english ? 0 : 50259) && s.n_langs == (k.english ? 0 : 99));
    CHECK(s.V == 51865 && s.eot == 50257 && s.no_speech == 50362 && s.no_ts == 50363 && s.tb == 50364);
    CHECK(s.blank == 220 && s.suppress_blank == 1 && s.with_ts == (k.no_ts ? 0 : 1) && s.max_init_ts == 50);
    CHECK(s.length_penalty == k.length_penalty);
    CHECK(s.seed == &SEED_WORD);
    CHECK(s.lp_stride == ctx);
    CHECK(s.lp_hist == (k.conf ? LP_HIST : nullptr) && s.best_lp == (k.conf ? BEST_LP : nullptr));
    CHECK(s.lang_probs == (k.conf && !k.english ? LANG_PROBS : nullptr));
    CHECK(p.hr.on == k.hist && p.hr.penalty == (k.hist ? 1.25f : 1.f) && p.hr.ngram == (k.hist ? 3 : 0));
    CHECK(p.P == s.prompt_len && p.max_tok == std::max(1, max_len - p.P));
    CHECK(s.beam == p.beam && s.lp_group == p.group);
    switch (m) {
        case DecodeMode::Batch: {
            const bool sampling = k.kind >= 3;
            const int beam = sampling ? 1 : wide;
            CHECK(s.prompt_len == k.n_pre + tail && s.sot_pos == k.n_pre && s.lang_pos == k.n_pre + 1);
            CHECK(s.pstride == k.n_pre + tail && s.pos_row == 0);
            CHECK(s.beam == beam && s.num_hyp == 1 && s.max_cand == lround_cand(beam, k.patience));
            CHECK(p.group == (k.kind == 4 ? 3 : beam) && p.sampling == sampling);
            CHECK(s.inv_temp == (sampling ? 2.f : 0.f));
            CHECK(s.budget == (k.budget ? BUDGET_BUF : nullptr));
            break;
        }
        case DecodeMode::Refill:
            CHECK(s.prompt_len == tail && s.sot_pos == 0 && s.lang_pos == 1);
            CHECK(s.pstride == tail && s.pos_row == 1);
            CHECK(s.beam == 1 && s.num_hyp == 1 && s.max_cand == 1 && p.group == 1 && s.inv_temp == 0.f);
            CHECK(s.budget == (k.budget ? BUDGET_BUF : nullptr));
            break;
        case DecodeMode::Session:
            CHECK(s.prompt_len == tail && s.sot_pos == 0 && s.lang_pos == 1);
            CHECK(s.pstride == ctx && s.pos_row == 1);
            CHECK(s.beam == wide && s.num_hyp == 1 && s.max_cand == lround_cand(wide, k.patience));
            CHECK(p.group == wide && s.inv_temp == 0.f);
            CHECK(s.budget == BUDGET_BUF);  // always bound: budgets come per window
            break;
    }
    (void)o;
}

// (2) one option moved at a time
static void check_sensitivity(DecodeMode m, const Case& k, const osw_decode_opts& o, const DecodePlan& p) {
    const int rows = 2 * p.group, CH = 8;
    const std::vector<int64_t> key = p.key(rows, CH);
    auto moved = [&](const std::function<void(osw_decode_opts&, Case&)>& f) {
        osw_decode_opts o2 = o;
        Case k2 = k;
        f(o2, k2);
        return plan_of(m, k2, o2).key(rows, CH) != key;
    };
#define MOVES(stmt) CHECK(moved([](osw_decode_opts& o, Case& k) { (void)o; (void)k; stmt; }))
#define STAYS(stmt) CHECK(!moved([](osw_decode_opts& o, Case& k) { (void)o; (void)k; stmt; }))
    MOVES(o.eot += 1);
    MOVES(o.no_speech += 1);
    MOVES(o.no_timestamps += 1);
    MOVES(o.timestamp_begin += 1);
    MOVES(o.blank += 1);
    MOVES(o.suppress_blank = 0);
    MOVES(o.without_timestamps = !o.without_timestamps);
    MOVES(o.max_initial_timestamp_index = -1);
    MOVES(o.max_length = 200);
    MOVES(o.length_penalty += 0.5f);
    MOVES(o.repetition_penalty = 1.5f);
    MOVES(o.no_repeat_ngram_size = 2);
    MOVES(o.task_token = o.task_token < 0 ? 50359 : -1);
    MOVES(k.conf = !k.conf);
    if (!k.english) {
        MOVES(o.first_lang += 1);
        MOVES(o.n_langs += 1);
    }
    if (m != DecodeMode::Session) MOVES((o.token_budget = o.token_budget ? nullptr : BUDGET));
    if (m != DecodeMode::Refill) {  // (refill decodes greedily whatever these say)
        MOVES(o.num_hypotheses = 2);
        MOVES(o.patience = o.patience * 2 + 1.f);
        if (k.kind < 3) MOVES(o.beam_size += 1);
    }
    if (m == DecodeMode::Batch) {
        MOVES(o.n_prefix = o.n_prefix ? 0 : 5);
        MOVES(k.n_encoded = k.n_encoded ? k.n_encoded + 1 : 4);
        MOVES(o.temperature = o.temperature > 0.f ? o.temperature * 2 : 0.3f);
        if (k.kind >= 3) MOVES(o.best_of += 1);
    }
    CHECK(p.key(rows + p.group, CH) != key);
    CHECK(p.key(rows, CH / 2) != key);
    // data the launches read through fixed addresses
    static const int32_t suppress2[] = {3, 4, 5}, prefix2[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, budget2[] = {1, 2},
                         langs2[] = {50260, -1};
    STAYS(o.seed += 99);
    STAYS((o.suppress_tokens = suppress2, o.n_suppress = 3));
    STAYS(o.language_token = -1);
    STAYS(o.language_tokens = langs2);
    STAYS(o.prefix_tokens = prefix2);
    STAYS(o.sot += 1);
    if (o.token_budget) STAYS(o.token_budget = budget2);
#undef MOVES
#undef STAYS
}

int main() {
    // (3) every key of the grid, with who made it
    std::map<std::vector<int64_t>, std::tuple<int, bool, bool>> keys;
    int plans = 0;
    for (int mode = 0; mode < 3; ++mode)
    for (int kind = 0; kind < 5; ++kind)
    for (int bits = 0; bits < 1024; ++bits) {
        const DecodeMode m = (DecodeMode)mode;
        Case k;
        k.kind = kind;
        k.no_ts = bits & 1; k.english = bits & 2; k.hist = bits & 4; k.conf = bits & 8; k.budget = bits & 16;
        k.n_pre = bits & 32 ? 5 : 0;
        k.n_encoded = bits & 64 ? 4 : 0;
        k.patience = bits & 128 ? 2.f : 1.f;
        k.length_penalty = bits & 256 ? 1.f : 0.f;
        k.max_length = bits & 512 ? 100 : 0;
        if (!admits(m, k)) continue;
        g_case = "mode " + std::to_string(mode) + " kind " + std::to_string(kind) + " bits " + std::to_string(bits);
        const osw_decode_opts o = opts_of(k);
        const DecodePlan p = plan_of(m, k, o);
        ++plans;
        check_params(m, k, o, p);
        check_sensitivity(m, k, o, p);
        for (int rows : {p.group, 2 * p.group}) {
            const auto who = std::make_tuple(mode, k.n_encoded != 0, k.english);
            auto ins = keys.emplace(p.key(rows, 8), who);
            CHECK(ins.second || ins.first->second == who);
        }
        // (4) the mask: (V + 31) / 32 words, ids outside [0, V) ignored
        CHECK(p.mask.size() == (51865 + 31) / 32);
        size_t set = 0;
        for (unsigned w : p.mask) set += __builtin_popcount(w);
        CHECK(set == 5 && (p.mask[0] & 0x86u) == 0x86u && (p.mask[51864 >> 5] >> (51864 & 31) & 1u));
    }
    g_case = "capacity";
    {
        static const int32_t wild[] = {-1, -51865, 51865, 1 << 30, 51864, 0};
        Case k{};
        k.patience = 1.f;
        osw_decode_opts o = opts_of(k);
        o.suppress_tokens = wild;
        o.n_suppress = 6;
        const DecodePlan p(DecodeMode::Batch, &o, DIMS);
        size_t set = 0;
        for (unsigned w : p.mask) set += __builtin_popcount(w);
        CHECK(set == 2 && (p.mask[0] & 1u));
        // P < max_len, for each mode's P
        for (int mode = 0; mode < 3; ++mode) {
            o.max_length = 3;  // == the multilingual start sequence
            std::string msg;
            try {
                DecodePlan q((DecodeMode)mode, &o, DIMS);
            } catch (const OswError& e) {
                msg = e.what();
                CHECK(e.code == OSW_EINVAL);
            }
            CHECK(msg == "prompt longer than max_length");
            o.max_length = 4;
            CHECK(DecodePlan((DecodeMode)mode, &o, DIMS).max_tok == 1);
        }
        o.max_length = 8;
        o.n_prefix = 5;
        std::string msg;
        try {
            DecodePlan q(DecodeMode::Batch, &o, DIMS, 5);
        } catch (const OswError& e) {
            msg = e.what();
        }
        CHECK(msg == "prompt longer than max_length");
    }
    std::printf("decode plan ok: %d plans, %zu keys, %d checks\n", plans, keys.size(), g_checks);
    return 0;
}
