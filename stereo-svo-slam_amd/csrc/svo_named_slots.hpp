// svo_named_slots.hpp — the slots a call of the ctx names: the caller's (seqs, n), where seqs == NULL stands for the
// slots 0 .. n-1 in order (an entry point that takes NULL for "every slot" sets n to the ctx's B first). Plain C++:
// no HIP, no error text; the entry points of svo_ctx.hip format their own messages.
#pragma once

#include <vector>

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
};
