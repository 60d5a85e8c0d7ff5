// Host-only check of what a retry session (osw_session_retries / osw_session_retry) adds to
// csrc/slots.h and csrc/plan.h: (1) SlotTable::retry, held -> decoding, with the counters, and every
// refusal (a free, a decoding or an unknown tag, a tag or a slot twice) leaving the table exactly
// as it was, (2) stalled() / decoding_end() / free_slots() with retried slots, a retried slot held
// again by finish(), (3) a seeded random walk against a model written out here, (4) the session
// plan with retries: group = max(beam, best_of) for (1,1) (1,3) (1,5) (5,3) (5,5) (2,5), lp_group
// with it, beam and the stop rule untouched, best_of out of range refused, (5) the decode-graph
// key: a retry session's differs from the retry-free session's and from another best_of's, the
// retry-free key is the one a plan built without the new argument gives, word for word, and
// binding row temperatures to a plan without retries (or none to one with) is refused.
// No HIP call; built and run by tests/test_session_retry_cpu.py with ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "plan.h"
#include "slots.h"

using namespace osw;

static int g_checks = 0;
static std::string g_case;
#define CHECK(c)                                                                \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) {                                                             \
            std::fprintf(stderr, "FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case.c_str()); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

template <typename F>
static int refused(F&& f) {
    try {
        f();
    } catch (const OswError& e) {
        return e.code;
    }
    return 0;
}

static bool same(const SlotTable& a, const SlotTable& b) {
    return a.state == b.state && a.tag == b.tag && a.hold == b.hold && a.added == b.added && a.decoding == b.decoding &&
           a.held == b.held;
}

#define CHECK_REFUSED(t, code, ...)                    \
    do {                                               \
        const SlotTable before_ = (t);                 \
        CHECK(refused([&] { __VA_ARGS__; }) == code);  \
        CHECK(same(before_, (t)));                     \
    } while (0)

// what osw_session_retry does with the table: all tags checked, then the transition
static void retry_tags(SlotTable& t, std::vector<int64_t> tags) {
    t.retry(t.held_slots((int)tags.size(), tags.data()));
}

static void transitions() {
    g_case = "transitions";
    SlotTable t(4);
    t.set_hold(true);
    t.note_add();
    t.admit(0, 10);
    t.admit(1, 11);
    t.admit(2, 12);
    CHECK(t.finish(1) == 11 && t.finish(2) == 12);
    CHECK(t.decoding == 1 && t.held == 2);
    // refusals: unknown, decoding, free (no tag), twice, one bad among good
    CHECK_REFUSED(t, OSW_EINVAL, retry_tags(t, {99}));
    CHECK_REFUSED(t, OSW_EINVAL, retry_tags(t, {10}));
    CHECK_REFUSED(t, OSW_EINVAL, retry_tags(t, {-1}));
    CHECK_REFUSED(t, OSW_EINVAL, retry_tags(t, {11, 11}));
    CHECK_REFUSED(t, OSW_EINVAL, retry_tags(t, {11, 12, 10}));
    CHECK_REFUSED(t, OSW_EINVAL, t.retry({3}));        // a free slot
    CHECK_REFUSED(t, OSW_EINVAL, t.retry({0}));        // a decoding slot
    CHECK_REFUSED(t, OSW_EINVAL, t.retry({1, 1}));     // a slot twice
    CHECK_REFUSED(t, OSW_EINVAL, t.retry({1, 7}));     // out of range
    CHECK_REFUSED(t, OSW_EINVAL, t.retry({-1}));
    // held -> decoding: the tag stays, the slot is no admission target, it counts as decoding
    retry_tags(t, {12});
    CHECK(t.state[2] == SlotState::Decoding && t.tag[2] == 12 && t.decoding == 2 && t.held == 1);
    CHECK(t.is_decoding(2) && t.tag_in_use(12) && t.decoding_end() == 3);
    CHECK((t.free_slots() == std::vector<int>{3}));
    CHECK_REFUSED(t, OSW_EINVAL, retry_tags(t, {12}));  // decoding again: not held
    CHECK_REFUSED(t, OSW_EINVAL, t.take_held(t.held_slots(1, std::vector<int64_t>{12}.data())));
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(3, 12));       // its tag is in use
    // it finishes into held again, is retried again, then released
    CHECK(t.finish(2) == 12 && t.held == 2 && t.decoding == 1);
    retry_tags(t, {11, 12});
    CHECK(t.held == 0 && t.decoding == 3);
    CHECK(t.finish(1) == 11 && t.finish(2) == 12);
    t.take_held(t.held_slots(2, std::vector<int64_t>{12, 11}.data()));
    CHECK(t.held == 0 && t.decoding == 1 && (t.free_slots() == std::vector<int>{1, 2, 3}));
    retry_tags(t, {});                                   // n == 0: a no-op
    CHECK(t.decoding == 1);
}

static void stalled_with_retries() {
    g_case = "stalled";
    SlotTable t(2);
    t.set_hold(true);
    t.note_add();
    t.admit(0, 1);
    t.admit(1, 2);
    t.finish(0);
    t.finish(1);
    CHECK(t.stalled(1) && !t.stalled(0));   // every slot held, a window queued: nothing to launch
    retry_tags(t, {2});
    CHECK(!t.stalled(1) && t.decoding_end() == 2);   // the retried slot decodes: a step has work
    t.finish(1);
    CHECK(t.stalled(3));
    retry_tags(t, {1, 2});
    CHECK(!t.stalled(3) && t.decoding == 2 && t.held == 0 && t.free_slots().empty());
}

// a random walk against a model: tag -> 0 decoding / 1 held
static void random_walk() {
    g_case = "random walk";
    unsigned long long z = 12345;
    auto rnd = [&](int n) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((z >> 33) % (unsigned)n);
    };
    SlotTable t(5);
    t.set_hold(true);
    t.note_add();
    std::map<int64_t, int> model;
    int64_t next_tag = 100;
    for (int it = 0; it < 4000; ++it) {
        const int op = rnd(4);
        if (op == 0) {
            const std::vector<int> f = t.free_slots();
            if (!f.empty()) {
                t.admit(f[rnd((int)f.size())], next_tag);
                model[next_tag++] = 0;
            }
        } else if (op == 1) {
            for (int s = 0; s < t.size(); ++s)
                if (t.is_decoding(s) && rnd(2)) model[t.finish(s)] = 1;
        } else {
            std::vector<int64_t> tags;
            for (auto& kv : model)
                if (kv.second == 1 && rnd(2)) tags.push_back(kv.first);
            const std::vector<int> slots = t.held_slots((int)tags.size(), tags.data());
            if (op == 2) {
                t.retry(slots);
                for (int64_t g : tags) model[g] = 0;
            } else {
                t.take_held(slots);
                for (int64_t g : tags) model.erase(g);
            }
        }
        int dec = 0, held = 0;
        for (auto& kv : model) (kv.second ? held : dec) += 1;
        CHECK(t.decoding == dec && t.held == held && (int)t.free_slots().size() == t.size() - dec - held);
        for (auto& kv : model) {
            CHECK(t.tag_in_use(kv.first));
            const int64_t g = kv.first;
            CHECK((refused([&] { (void)t.held_slots(1, &g); }) == 0) == (kv.second == 1));
        }
    }
}

static const osw_dims DIMS = {80, 1500, 384, 6, 4, 51865, 448, 384, 6, 4};
static unsigned long long SEED_WORD, ROW_SEED[32];
static int BUDGET_BUF[32];
static float LP_HIST[1], BEST_LP[1], LANG_PROBS[1], ROW_INV_TEMP[32];

static osw_decode_opts opts_of(int beam) {
    osw_decode_opts o{};
    o.task_token = 50359;
    o.language_token = 50259;
    o.suppress_blank = 1;
    o.max_initial_timestamp_index = 50;
    o.max_length = 448;
    o.eot = 50257; o.sot = 50258; o.sot_prev = 50361; o.no_speech = 50362; o.no_timestamps = 50363;
    o.timestamp_begin = 50364; o.blank = 220; o.first_lang = 50259; o.n_langs = 99;
    o.beam_size = beam;
    o.patience = 1.f;
    o.length_penalty = 1.f;
    o.num_hypotheses = 1;
    o.best_of = 5;
    return o;
}

static void plans() {
    g_case = "plans";
    const int cases[][2] = {{1, 1}, {1, 3}, {1, 5}, {5, 3}, {5, 5}, {2, 5}};
    for (auto& bc : cases) {
        const int beam = bc[0], best_of = bc[1];
        const osw_decode_opts o = opts_of(beam);
        DecodePlan plain(DecodeMode::Session, &o, DIMS);          // as every caller before built it
        DecodePlan off(DecodeMode::Session, &o, DIMS, 0, 0, 0);
        DecodePlan on(DecodeMode::Session, &o, DIMS, 0, 0, best_of);
        DecodePlan later(DecodeMode::Session, &o, DIMS);          // osw_session_retries after osw_session_begin
        later.enable_retries(best_of);
        for (DecodePlan* p : {&plain, &off}) {
            CHECK(p->beam == beam && p->group == beam && p->best_of == 0 && p->sp.lp_group == beam);
            p->bind(&SEED_WORD, BUDGET_BUF, true, LP_HIST, BEST_LP, LANG_PROBS);
            CHECK(p->sp.row_inv_temp == nullptr && p->sp.row_seed == nullptr);
        }
        for (DecodePlan* p : {&on, &later}) {
            CHECK(p->beam == beam && p->sp.beam == beam && p->best_of == best_of);
            CHECK(p->group == std::max(beam, best_of) && p->sp.lp_group == p->group);
            CHECK(p->sp.max_cand == plain.sp.max_cand && p->sp.num_hyp == plain.sp.num_hyp && p->sp.inv_temp == 0.f);
            CHECK(p->sp.pos_row == 1 && p->sp.pstride == plain.sp.pstride && p->max_tok == plain.max_tok);
            p->bind(&SEED_WORD, BUDGET_BUF, true, LP_HIST, BEST_LP, LANG_PROBS, ROW_INV_TEMP, ROW_SEED);
            CHECK(p->sp.row_inv_temp == ROW_INV_TEMP && p->sp.row_seed == ROW_SEED);
        }
        // the keys: the retry-free one is unchanged (the same words whichever way the plan was built:
        // 36 of them, the count before retries existed); a retry session's is another
        const int rows = 4 * plain.group, rrows = 4 * on.group;
        CHECK(plain.key(rows, 4) == off.key(rows, 4) && plain.key(rows, 4).size() == 36);
        CHECK(on.key(rrows, 4) == later.key(rrows, 4) && on.key(rrows, 4).size() == 37);
        CHECK(on.key(rrows, 4) != plain.key(rows, 4) && on.key(rrows, 4) != plain.key(rrows, 4));
        if (best_of != 4) {
            DecodePlan other(DecodeMode::Session, &o, DIMS, 0, 0, 4);
            other.bind(&SEED_WORD, BUDGET_BUF, true, LP_HIST, BEST_LP, LANG_PROBS, ROW_INV_TEMP, ROW_SEED);
            CHECK(other.key(rrows, 4) != on.key(rrows, 4));
        }
        // row temperatures only with retries, and always with them
        CHECK(refused([&] { plain.bind(&SEED_WORD, BUDGET_BUF, false, LP_HIST, BEST_LP, LANG_PROBS, ROW_INV_TEMP, ROW_SEED); }) == OSW_EINVAL);
        CHECK(refused([&] { on.bind(&SEED_WORD, BUDGET_BUF, false, LP_HIST, BEST_LP, LANG_PROBS); }) == OSW_EINVAL);
        CHECK(refused([&] { on.bind(&SEED_WORD, BUDGET_BUF, false, LP_HIST, BEST_LP, LANG_PROBS, ROW_INV_TEMP, nullptr); }) == OSW_EINVAL);
    }
    g_case = "plan refusals";
    const osw_decode_opts o = opts_of(5);
    for (int bad : {-1, 6, 100})
        CHECK(refused([&] { DecodePlan p(DecodeMode::Session, &o, DIMS, 0, 0, bad); }) == OSW_EINVAL);
    for (int bad : {0, -1, 6}) {
        DecodePlan p(DecodeMode::Session, &o, DIMS);
        CHECK(refused([&] { p.enable_retries(bad); }) == OSW_EINVAL);
        CHECK(p.group == 5 && p.best_of == 0 && p.sp.lp_group == 5);
    }
    // only sessions retry in place
    osw_decode_opts g = opts_of(1);
    DecodePlan batch(DecodeMode::Batch, &g, DIMS), refill(DecodeMode::Refill, &g, DIMS);
    CHECK(refused([&] { batch.enable_retries(3); }) == OSW_EINVAL);
    CHECK(refused([&] { refill.enable_retries(3); }) == OSW_EINVAL);
    CHECK(refused([&] { DecodePlan p(DecodeMode::Batch, &g, DIMS, 0, 0, 3); }) == OSW_EINVAL);
}

int main() {
    transitions();
    stalled_with_retries();
    random_walk();
    plans();
    std::printf("session retry ok: %d checks\n", g_checks);
    return 0;
}
