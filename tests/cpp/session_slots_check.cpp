// Host-only check of csrc/slots.h (a decode session's window slots): (1) every transition of a
// slot (free -> decoding -> free without hold, -> held -> free with it) and the counters, (2) every
// refusal with its code and with the table left exactly as it was (align / release of a free, a
// decoding or an unknown tag, a tag twice in one call, a tag already in use at admission, hold
// after the first add), (3) admission never picks a held slot, (4) the all-held-and-queued case
// is recognised as a step without work, and only it, (5) a seeded random walk against a model
// written out here.  No HIP call; built and run by tests/test_session_slots_cpu.py with ASan + UBSan.
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <string>

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

// the code f() is refused with (0: it was not refused)
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

// the statement must be refused with `code` and leave t untouched
#define CHECK_REFUSED(t, code, ...)                    \
    do {                                               \
        const SlotTable before_ = (t);                 \
        CHECK(refused([&] { __VA_ARGS__; }) == code);  \
        CHECK(same(before_, (t)));                     \
    } while (0)

static void without_hold() {
    g_case = "no hold";
    SlotTable t(3);
    CHECK(t.size() == 3 && t.decoding == 0 && t.held == 0 && !t.hold);
    CHECK((t.free_slots() == std::vector<int>{0, 1, 2}));
    t.note_add();
    t.admit(0, 10);
    t.admit(2, 10);  // (without hold tags need not differ)
    CHECK(t.decoding == 2 && t.decoding_end() == 3 && t.is_decoding(0) && !t.is_decoding(1) && t.is_decoding(2));
    CHECK((t.free_slots() == std::vector<int>{1}));
    CHECK(t.finish(2) == 10);
    CHECK(t.decoding == 1 && t.held == 0 && t.decoding_end() == 1);
    CHECK((t.free_slots() == std::vector<int>{1, 2}));  // the slot is free at once
    const int64_t tag = 10;
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(1, &tag));  // nothing is ever held
    CHECK_REFUSED(t, OSW_EINVAL, t.finish(2));            // a free slot cannot finish
    CHECK_REFUSED(t, OSW_EINVAL, t.finish(5));
    CHECK_REFUSED(t, OSW_EINVAL, t.finish(-1));
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(0, 11));         // a decoding slot takes no window
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(3, 11));
    CHECK(!t.stalled(4) && !t.stalled(0));
}

static void hold_after_add() {
    g_case = "hold after add";
    SlotTable t(2);
    t.set_hold(true);
    t.set_hold(false);
    t.set_hold(true);  // any number of times before the first add
    CHECK(t.hold);
    t.note_add();
    CHECK_REFUSED(t, OSW_ESTATE, t.set_hold(false));
    CHECK_REFUSED(t, OSW_ESTATE, t.set_hold(true));
    SlotTable u(2);
    u.note_add();
    CHECK_REFUSED(u, OSW_ESTATE, u.set_hold(true));
    CHECK(!u.hold);
}

static void with_hold() {
    g_case = "hold";
    SlotTable t(4);
    t.set_hold(true);
    t.note_add();
    for (int i = 0; i < 4; ++i) t.admit(i, 100 + i);
    CHECK(t.decoding == 4 && t.free_slots().empty());
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(0, 7));
    // slots 1 and 3 finish: held, not free
    CHECK(t.finish(1) == 101 && t.finish(3) == 103);
    CHECK(t.decoding == 2 && t.held == 2 && t.free_slots().empty());
    CHECK(!t.is_decoding(1) && !t.is_decoding(3) && t.decoding_end() == 3);
    CHECK_REFUSED(t, OSW_EINVAL, t.finish(1));  // never reported twice
    CHECK(t.tag_in_use(101) && t.tag_in_use(100) && !t.tag_in_use(7));
    // refusals of align / release: decoding, unknown, twice, null
    const int64_t decoding[] = {103, 100}, unknown[] = {103, 55}, twice[] = {103, 101, 103};
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(2, decoding));
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(2, unknown));
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(3, twice));
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(1, nullptr));
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(-1, twice));
    CHECK_REFUSED(t, OSW_EINVAL, t.take_held({0}));      // decoding
    CHECK_REFUSED(t, OSW_EINVAL, t.take_held({3, 0}));   // nothing freed when one is refused
    CHECK_REFUSED(t, OSW_EINVAL, t.take_held({4}));
    CHECK(t.held_slots(0, nullptr).empty());
    // the order of the call is kept
    const int64_t both[] = {103, 101};
    CHECK((t.held_slots(2, both) == std::vector<int>{3, 1}));
    // one is aligned: its slot is free, its tag forgotten, the other still held
    const int64_t one = 103;
    t.take_held(t.held_slots(1, &one));
    CHECK(t.held == 1 && (t.free_slots() == std::vector<int>{3}) && !t.tag_in_use(103));
    CHECK_REFUSED(t, OSW_EINVAL, t.held_slots(1, &one));  // a second align / release of it
    // admission in hold mode: a tag in use is refused, a freed one is welcome again
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(3, 101));  // held
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(3, 100));  // decoding
    CHECK_REFUSED(t, OSW_EINVAL, t.admit(1, 9));    // a held slot takes no window
    t.admit(3, 103);
    CHECK(t.decoding == 3 && t.held == 1 && t.is_decoding(3));
}

static void stall() {
    g_case = "stall";
    SlotTable t(2);
    t.set_hold(true);
    t.note_add();
    t.admit(0, 1);
    t.admit(1, 2);
    CHECK(!t.stalled(1));  // both decode
    t.finish(0);
    CHECK(!t.stalled(1));  // one still decodes
    t.finish(1);
    CHECK(t.stalled(1) && t.stalled(7));
    CHECK(!t.stalled(0));  // nothing waits: the step just finds nothing to do
    CHECK(t.free_slots().empty() && t.decoding_end() == 0);
    const int64_t tag = 2;
    t.take_held(t.held_slots(1, &tag));
    CHECK(!t.stalled(1) && (t.free_slots() == std::vector<int>{1}));
    SlotTable e(0);  // (no slots: never "all held")
    CHECK(!e.stalled(0));
}

// a seeded walk of admissions, finishes, aligns and releases against a map-based model
static void walk(bool hold, uint64_t seed) {
    g_case = std::string("walk ") + (hold ? "hold" : "no hold");
    const int W = 5;
    SlotTable t(W);
    if (hold) t.set_hold(true);
    t.note_add();
    std::map<int, int64_t> dec, held;  // slot -> tag
    int64_t next_tag = 1;
    auto rnd = [&] {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(seed >> 33);
    };
    for (int it = 0; it < 4000; ++it) {
        const int op = rnd() % 4;
        if (op == 0) {
            const std::vector<int> f = t.free_slots();
            for (int s : f) CHECK(!dec.count(s) && !held.count(s));
            CHECK((int)f.size() == W - (int)dec.size() - (int)held.size());
            if (!f.empty()) {
                const int s = f[rnd() % f.size()];
                t.admit(s, next_tag);
                dec[s] = next_tag++;
            }
        } else if (op == 1 && !dec.empty()) {
            auto p = dec.begin();
            std::advance(p, rnd() % dec.size());
            CHECK(t.finish(p->first) == p->second);
            if (hold) held[p->first] = p->second;
            dec.erase(p);
        } else if (op >= 2 && !held.empty()) {
            std::vector<int64_t> tags;
            std::vector<int> want;
            for (auto& kv : held)
                if (rnd() % 2) tags.push_back(kv.second), want.push_back(kv.first);
            const std::vector<int> got = t.held_slots((int)tags.size(), tags.data());
            CHECK(got == want);
            t.take_held(got);
            for (int s : want) held.erase(s);
        }
        CHECK(t.decoding == (int)dec.size() && t.held == (int)held.size());
        for (int s = 0; s < W; ++s) CHECK(t.is_decoding(s) == (dec.count(s) == 1));
        CHECK(t.stalled(1) == (dec.empty() && (int)held.size() == W));
    }
}

int main() {
    without_hold();
    hold_after_add();
    with_hold();
    stall();
    walk(false, 1);
    walk(true, 2);
    walk(true, 3);
    std::printf("session slots ok: %d checks\n", g_checks);
    return 0;
}
