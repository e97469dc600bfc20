// named_slots_check.cpp — csrc/svo_named_slots.hpp without a GPU: the first bad named position, and the split of the
// named positions over the groups of a ctx of B = 6 slots, as groups of 2, 2, 2 and of 1, 5. Prints "named slots ok".
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

// a naming with no bad position, either way of asking
void check_good(const int* seqs, int n) {
    const NamedSlots slots{seqs, n};
    CHECK(slots.first_bad(B, true) == -1 && slots.first_bad(B, false) == -1);
    check_split(slots);
}

// position `once` is the first bad one when a slot may be named once, `range` when only the range is checked
void check_bad(const std::vector<int>& seqs, int once, int range) {
    const NamedSlots slots{seqs.data(), (int)seqs.size()};
    CHECK(slots.first_bad(B, true) == once);
    CHECK(slots.first_bad(B, false) == range);
    if (range == -1) check_split(slots);      // (a slot named twice is still split: restarts and rig assignments allow it)
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
