// named_slots_check.cpp — csrc/svo_named_slots.hpp without a GPU: the first bad named position, and the split of the
// named positions over the groups of a ctx of B = 6 slots, as groups of 2, 2, 2 and of 1, 5, by each_in and as the shares
// that the queued jobs carry (SlotList, SlotShare, NamedSlots::share). Prints "named slots ok".
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../stereo-svo-slam_amd/csrc/svo_named_slots.hpp"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

namespace {

constexpr int B = 6;
const std::vector<std::vector<int>> SPLITS = {{2, 2, 2}, {1, 5}};   // slots per group

// every named position is visited by exactly one group, in named order within it, with local = slot - first
void check_split(const NamedSlots& slots) {
    for (const std::vector<int>& counts : SPLITS) {
        std::vector<int> seen((size_t)slots.n, 0);
        int first = 0;
        for (int count : counts) {
            int last = -1;
            slots.each_in(first, count, [&](int i, int local) {
                CHECK(i >= 0 && i < slots.n && i > last);
                CHECK(local == slots.at(i) - first && local >= 0 && local < count);
                seen[(size_t)i]++;
                last = i;
            });
            first += count;
        }
        CHECK(first == B);
        for (int v : seen) CHECK(v == 1);
    }
}

// a job of the ctx: the share of its group and something of its own per slot
struct ListJob : SlotList {
    std::vector<int> item;
};
struct ShareJob : SlotShare {
    std::vector<int> item;
};

// share() fills a group's job like each_in visits it: the slots as indices in the group, the named positions as the
// segments, the hook once per position before the slot is added, in named order; a position the hook turns down is in
// no job; the result says whether the job has a slot at all
void check_shares(const NamedSlots& slots) {
    for (const std::vector<int>& counts : SPLITS) {
        std::vector<int> seen((size_t)slots.n, 0);
        int first = 0;
        for (int count : counts) {
            std::vector<int> want_seqs, want_seg;
            slots.each_in(first, count, [&](int i, int local) { want_seqs.push_back(local); want_seg.push_back(i); });
            ShareJob all;
            const bool any = slots.share(first, count, all, [&](ShareJob& j, int i, int local) {
                CHECK(j.seqs.size() == j.item.size() && j.seg.size() == j.item.size());   // (the slot is added after the hook)
                CHECK(local == slots.at(i) - first);
                j.item.push_back(10 * i);
                return true;
            });
            CHECK(any == !want_seqs.empty());
            CHECK(all.seqs == want_seqs && all.seg == want_seg && all.item.size() == want_seg.size());
            for (size_t k = 0; k < all.seg.size(); k++) {
                CHECK(all.item[k] == 10 * all.seg[k]);
                seen[(size_t)all.seg[k]]++;
            }
            // a list job keeps no segments; the hook leaves the odd positions out
            ListJob even;
            const bool any_even = slots.share(first, count, even, [](ListJob& j, int i, int) {
                if (i % 2) return false;
                j.item.push_back(i);
                return true;
            });
            std::vector<int> even_seqs, even_item;
            for (size_t k = 0; k < want_seg.size(); k++)
                if (want_seg[k] % 2 == 0) { even_seqs.push_back(want_seqs[k]); even_item.push_back(want_seg[k]); }
            CHECK(any_even == !even_seqs.empty() && even.seqs == even_seqs && even.item == even_item);
            // nobody kept: no job
            SlotShare none;
            CHECK(!slots.share(first, count, none, [](SlotShare&, int, int) { return false; }) && none.seqs.empty() && none.seg.empty());
            first += count;
        }
        for (int v : seen) CHECK(v == 1);
    }
}

// a naming with no bad position, either way of asking
void check_good(const int* seqs, int n) {
    const NamedSlots slots{seqs, n};
    CHECK(slots.first_bad(B, true) == -1 && slots.first_bad(B, false) == -1);
    check_split(slots);
    check_shares(slots);
}

// position `once` is the first bad one when a slot may be named once, `range` when only the range is checked
void check_bad(const std::vector<int>& seqs, int once, int range) {
    const NamedSlots slots{seqs.data(), (int)seqs.size()};
    CHECK(slots.first_bad(B, true) == once);
    CHECK(slots.first_bad(B, false) == range);
    if (range == -1) {                        // (a slot named twice is still split: restarts and rig assignments allow it)
        check_split(slots);
        check_shares(slots);
    }
}

}  // namespace

int main() {
    // seqs == NULL: the slots 0 .. B-1
    const NamedSlots all{nullptr, B};
    for (int i = 0; i < B; i++) CHECK(all.at(i) == i);
    check_good(nullptr, B);
    // nobody named: nothing is bad, nothing is visited
    check_good(nullptr, 0);
    const int none = 0;
    check_good(&none, 0);
    int visits = 0;
    NamedSlots{&none, 0}.each_in(0, B, [&](int, int) { visits++; });
    CHECK(visits == 0);
    // add_slot: a list keeps the slot, a share the slot and its named position
    SlotList list;
    SlotShare share;
    add_slot(list, 7, 3);
    add_slot(share, 7, 3);
    CHECK(list.seqs == std::vector<int>{3} && share.seqs == std::vector<int>{3} && share.seg == std::vector<int>{7});
    // a permutation, and namings that interleave the groups
    const int perm[B] = {3, 0, 5, 1, 4, 2};
    for (int i = 0; i < B; i++) CHECK((NamedSlots{perm, B}.at(i) == perm[i]));
    check_good(perm, B);
    const int inter[4] = {4, 0, 5, 2};
    check_good(inter, 4);
    const int one[1] = {5};
    check_good(one, 1);
    // one slot named twice: first and last, adjacent, and the first slot of the list
    check_bad({2, 0, 4, 2}, 3, -1);
    check_bad({1, 3, 3, 5}, 2, -1);
    check_bad({0, 0}, 1, -1);
    check_bad({5, 4, 3, 2, 1, 0, 5}, 6, -1);
    // out of range: -1 and B, alone, first, last, and before a repeat
    check_bad({-1}, 0, 0);
    check_bad({B}, 0, 0);
    check_bad({0, 1, B}, 2, 2);
    check_bad({-1, 0, 0}, 0, 0);
    check_bad({2, 2, -1}, 1, 2);
    check_bad({2, B, 2}, 1, 1);
    // NULL with more than B positions: position B names slot B
    CHECK((NamedSlots{nullptr, B + 1}.first_bad(B, true) == B));
    std::printf("named slots ok\n");
    return 0;
}
