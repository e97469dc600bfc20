// svo_named_slots.hpp — the slots a call of the ctx names: the caller's (seqs, n), where seqs == NULL stands for the
// slots 0 .. n-1 in order (an entry point that takes NULL for "every slot" sets n to the ctx's B first). Plain C++:
// no HIP, no error text; the entry points of svo_ctx*.hip format their own messages (svo_ctx_state.hpp).
#pragma once

#include <vector>

// One group's share of a naming, which a queued job of the ctx carries: its named slots as indices in the group, in
// named order (SlotList), and for a job that fills one segment per named slot the named position of each (SlotShare).
struct SlotList {
    std::vector<int> seqs;
};
struct SlotShare : SlotList {
    std::vector<int> seg;
};
inline void add_slot(SlotList& s, int, int local) { s.seqs.push_back(local); }
inline void add_slot(SlotShare& s, int i, int local) {
    s.seqs.push_back(local);
    s.seg.push_back(i);
}

struct NamedSlots {
    const int* seqs;
    int n;
    // the slot at named position i
    int at(int i) const { return seqs ? seqs[i] : i; }
    // the first named position whose slot is outside [0, B) or (once: also) was named before; -1: none
    int first_bad(int B, bool once) const {
        std::vector<char> named(once && B > 0 ? (size_t)B : 0, 0);
        for (int i = 0; i < n; i++) {
            const int s = at(i);
            if (s < 0 || s >= B || (once && named[(size_t)s])) return i;
            if (once) named[(size_t)s] = 1;
        }
        return -1;
    }
    // f(i, local) for every named position i whose slot is in [first, first + count), in named order; local: the
    // slot's index from `first`
    template <typename F>
    void each_in(int first, int count, F f) const {
        for (int i = 0; i < n; i++) {
            const int s = at(i);
            if (s >= first && s < first + count) f(i, s - first);
        }
    }
    // the share of the group [first, first + count) into `job` (a SlotList or SlotShare): keep(job, i, local) for
    // every named position of the group, in named order; it adds what the job keeps per slot besides the slot, or
    // returns false and the slot is left out. False: the group has no slot in the job.
    template <typename Share, typename Keep>
    bool share(int first, int count, Share& job, Keep keep) const {
        each_in(first, count, [&](int i, int local) {
            if (keep(job, i, local)) add_slot(job, i, local);
        });
        return !job.seqs.empty();
    }
};
