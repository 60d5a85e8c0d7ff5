// The window slots of a decode session (osw_session_*, session.hip): which slot is free, which
// decodes and which is held for word timing (osw_session_hold), the tag-to-slot lookup and every
// transition with its refusals.  Host only: no HIP call and nothing of osw_ctx, so a stand-alone
// program checks it (tests/cpp/session_slots_check.cpp).
//
//   free --admit--> decoding --finish--> free                      (no hold)
//                            --finish--> held --take_held--> free  (hold: osw_session_align /
//                                                                   osw_session_release)
//                                        held --retry--> decoding   (osw_session_retry: the window
//                                                                   decodes again in its own slot)
// A held slot keeps its cross-K/V: admission never picks it and finish never reports it again.
#pragma once
#include <cstdint>
#include <vector>

#include "error.h"

namespace osw {

enum class SlotState : uint8_t { Free, Decoding, Held };

struct SlotTable {
    std::vector<SlotState> state;
    std::vector<int64_t> tag;  // of a decoding or held slot
    bool hold = false;         // finished windows keep their slots
    bool added = false;        // a window was queued: the hold mode is fixed
    int decoding = 0, held = 0;

    SlotTable() = default;
    explicit SlotTable(int n) : state((size_t)n, SlotState::Free), tag((size_t)n, -1) {}
    int size() const { return (int)state.size(); }

    // osw_session_hold: before the session's first osw_session_add only
    void set_hold(bool enable) {
        if (added) throw OswError(OSW_ESTATE, "osw_session_hold: windows were already added to this session");
        hold = enable;
    }
    void note_add() { added = true; }

    // the slots admission may fill, in index order: never a held one
    std::vector<int> free_slots() const {
        std::vector<int> f;
        for (int i = 0; i < size(); ++i)
            if (state[i] == SlotState::Free) f.push_back(i);
        return f;
    }
    bool is_decoding(int slot) const { return slot >= 0 && slot < size() && state[slot] == SlotState::Decoding; }
    // one past the highest decoding slot: the slots a decoder chunk has to cover
    int decoding_end() const {
        int hi = 0;
        for (int i = 0; i < size(); ++i)
            if (state[i] == SlotState::Decoding) hi = i + 1;
        return hi;
    }
    // a decoding or held window carries this tag (hold mode keeps them distinct: session_add)
    bool tag_in_use(int64_t t) const {
        for (int i = 0; i < size(); ++i)
            if (state[i] != SlotState::Free && tag[i] == t) return true;
        return false;
    }

    void admit(int slot, int64_t t) {
        REQUIRE(slot >= 0 && slot < size() && state[slot] == SlotState::Free, "admission into a slot that is not free");
        REQUIRE(!hold || !tag_in_use(t), "a window of this tag is still decoding or held");
        state[slot] = SlotState::Decoding;
        tag[slot] = t;
        ++decoding;
    }
    // the window of `slot` finished: its tag; the slot is held (hold) or free
    int64_t finish(int slot) {
        REQUIRE(is_decoding(slot), "a slot that is not decoding cannot finish");
        --decoding;
        if (hold) {
            state[slot] = SlotState::Held;
            ++held;
        } else {
            state[slot] = SlotState::Free;
        }
        return tag[slot];
    }
    // The held slots of tags[0 .. n), in that order.  Every tag is checked before anything
    // changes: a tag that is not held (free, still decoding, unknown) or that appears twice
    // refuses the whole call (OSW_EINVAL), and the table is left as it was.
    std::vector<int> held_slots(int n, const int64_t* tags) const {
        REQUIRE(n >= 0 && (n == 0 || tags), "null tag list");
        std::vector<int> out;
        for (int i = 0; i < n; ++i) {
            int slot = -1;
            for (int s = 0; s < size(); ++s)
                if (state[s] == SlotState::Held && tag[s] == tags[i]) slot = s;
            REQUIRE(slot >= 0, "no held window has this tag");
            for (int s : out) REQUIRE(s != slot, "a tag appears twice");
            out.push_back(slot);
        }
        return out;
    }
    // frees slots held_slots() returned
    void take_held(const std::vector<int>& slots) {
        for (int s : slots) REQUIRE(s >= 0 && s < size() && state[s] == SlotState::Held, "slot is not held");
        for (int s : slots) {
            state[s] = SlotState::Free;
            tag[s] = -1;
            --held;
        }
    }
    // slots held_slots() returned decode again (osw_session_retry): they keep their tags and
    // their cross-K/V, finish() holds them again
    void retry(const std::vector<int>& slots) {
        for (int s : slots) REQUIRE(s >= 0 && s < size() && state[s] == SlotState::Held, "slot is not held");
        for (size_t i = 0; i < slots.size(); ++i)
            for (size_t j = 0; j < i; ++j) REQUIRE(slots[i] != slots[j], "a slot appears twice");
        for (int s : slots) {
            state[s] = SlotState::Decoding;
            --held;
            ++decoding;
        }
    }
    // Nothing decodes, no slot is free and windows wait: a step has nothing to launch until the
    // caller aligns or releases what it holds
    bool stalled(int queued) const { return queued > 0 && decoding == 0 && held == size(); }
};

}  // namespace osw
