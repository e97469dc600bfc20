// voxel_entries_plan_check.cpp — the entries' part of csrc/svo_voxel_plan.hpp without a GPU: what a span of entry
// records must look like, the tiles it is cut into (walked over a real array of 40-byte records, so that the
// sanitizers see an index past the end), the merge's load bound over several spans at and around its limit and at
// counts whose sum would wrap, the pack's fit rule, the rehash's admission rule for every capacity, the bitwise
// comparison of voxel edges and the overlap of two byte ranges. Prints "voxel entries plan ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../stereo-svo-slam_amd/csrc/svo_voxel_plan.hpp"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using namespace svo;

namespace {

struct Entry {                       // svo_voxel_entry
    uint64_t key;
    uint32_t acc[8];
};
static_assert(sizeof(Entry) == VOXEL_ENTRY_BYTES && alignof(Entry) == 8, "40 bytes, 8-byte aligned");

// every record of a span of n is visited exactly once by the lanes of its tiles, and no lane below n is left out
void check_tiles(int64_t n) {
    const int64_t tiles = voxel_entry_span_tiles(n);
    CHECK(tiles == voxel_span_tiles(n) && tiles * VOXEL_TILE >= n && (tiles == 0 || (tiles - 1) * VOXEL_TILE < n));
    std::vector<Entry> span((size_t)n);
    CHECK(voxel_entry_span_ok(n ? (uintptr_t)span.data() : 0, n));
    for (int64_t t = 0; t < tiles; t++)
        for (int lane = 0; lane < VOXEL_TILE; lane++) {
            const int64_t k = t * VOXEL_TILE + lane;
            if (k < n) span[(size_t)k].acc[0]++;
        }
    for (const Entry& e : span) CHECK(e.acc[0] == 1);
}

}  // namespace

int main() {
    // spans
    alignas(8) static unsigned char bytes[64];
    const uintptr_t at = (uintptr_t)bytes;
    CHECK(voxel_entry_span_ok(0, 0) && voxel_entry_span_ok(at + 3, 0) && voxel_entry_span_ok(at, 1) && voxel_entry_span_ok(at + 8, 1));
    CHECK(!voxel_entry_span_ok(0, 1) && !voxel_entry_span_ok(at, -1) && !voxel_entry_span_ok(0, -1));
    for (int off = 1; off < 8; off++) CHECK(!voxel_entry_span_ok(at + off, 1));
    CHECK(voxel_entry_span_ok(at + 8, std::numeric_limits<int64_t>::max()));
    for (int64_t n : {0, 1, 255, 256, 257, 511, 512, 513, 70001}) check_tiles(n);
    CHECK(voxel_entry_span_tiles(-5) == 0 && voxel_entry_span_tiles(std::numeric_limits<int64_t>::max()) == (std::numeric_limits<int64_t>::max() >> 8) + 1);

    // the load bound over several spans: on the bound, and sums that would wrap
    for (int log2 = VOXEL_LOG2_MIN; log2 <= VOXEL_LOG2_MAX; log2++) {
        const uint64_t limit = voxel_load_limit(log2);
        CHECK(limit == ((uint64_t)3 << log2) / 4);
        const int64_t a[3] = {(int64_t)(limit / 2), 0, (int64_t)(limit - limit / 2)};
        CHECK(voxel_merge_load_ok(0, a, 3, log2) && !voxel_merge_load_ok(1, a, 3, log2) && voxel_merge_load_ok(limit - limit / 2, a, 2, log2));
        const int64_t b[2] = {(int64_t)limit, 1};
        CHECK(voxel_merge_load_ok(0, b, 1, log2) && !voxel_merge_load_ok(0, b, 2, log2) && voxel_merge_load_ok(limit, b, 0, log2));
        CHECK(!voxel_merge_load_ok(limit + 1, b, 0, log2) && voxel_merge_load_ok(limit, nullptr, 0, log2));
    }
    const int64_t big = std::numeric_limits<int64_t>::max();
    const int64_t wrap[3] = {big, big, 2};                  // 2^64 exactly: the sum must not come back as 0
    CHECK(!voxel_merge_load_ok(0, wrap, 3, 26) && !voxel_merge_load_ok(0, wrap, 2, 26) && !voxel_merge_load_ok(0, wrap, 1, 26));
    const int64_t neg[2] = {5, -1};
    CHECK(!voxel_merge_load_ok(0, neg, 2, 10) && voxel_merge_load_ok(0, neg, 1, 10));
    CHECK(!voxel_merge_load_ok(std::numeric_limits<uint64_t>::max(), neg, 1, 26));

    // the pack's fit rule: the extraction's
    CHECK(voxel_pack_fits(0, 0) && voxel_pack_fits(48, 48) && !voxel_pack_fits(48, 47) && !voxel_pack_fits(1, 0) && !voxel_pack_fits(-1, 5) &&
          !voxel_pack_fits(0, -1));
    for (int64_t k : {0, 1, 47, 48, 49})
        for (int64_t c : {-1, 0, 47, 48, 49}) CHECK(voxel_pack_fits(k, c) == voxel_extract_fits(k, c));

    // the rehash's admission rule
    CHECK(voxel_rehash_ok(48, 6) && !voxel_rehash_ok(49, 6) && voxel_rehash_ok(0, 6) && voxel_rehash_ok(768, 10) && !voxel_rehash_ok(769, 10));
    CHECK(!voxel_rehash_ok(0, 5) && !voxel_rehash_ok(0, 27) && !voxel_rehash_ok(0, -1) && !voxel_rehash_ok(0, 64) && voxel_rehash_ok(0, 26));
    CHECK(voxel_rehash_ok(voxel_load_limit(26), 26) && !voxel_rehash_ok(voxel_load_limit(26) + 1, 26) &&
          !voxel_rehash_ok(std::numeric_limits<uint64_t>::max(), 26));

    // voxel edges: bit for bit
    float one = 1.0f, next;
    uint32_t u;
    std::memcpy(&u, &one, 4);
    u += 1;
    std::memcpy(&next, &u, 4);
    CHECK(voxel_edge_same(one, 1.0f) && !voxel_edge_same(one, next) && !voxel_edge_same(0.3f, 0.30000004f) && voxel_edge_same(0.05f, 0.05f));
    CHECK(!voxel_edge_same(0.0f, -0.0f));

    // byte ranges
    CHECK(voxel_ranges_overlap(100, 10, 100, 10) && voxel_ranges_overlap(100, 10, 109, 1) && !voxel_ranges_overlap(100, 10, 110, 1));
    CHECK(voxel_ranges_overlap(109, 5, 100, 10) && !voxel_ranges_overlap(110, 5, 100, 10) && !voxel_ranges_overlap(100, 0, 100, 10));
    CHECK(!voxel_ranges_overlap(std::numeric_limits<uintptr_t>::max() - 4, 4, 0, 16) && voxel_ranges_overlap(0, 16, 15, 1));
    CHECK(voxel_ranges_overlap(100, voxel_map_bytes(6), 100 + voxel_map_bytes(6) - 16, voxel_map_bytes(10)) &&
          !voxel_ranges_overlap(100, voxel_map_bytes(6), 100 + voxel_map_bytes(6), voxel_map_bytes(10)));
    std::printf("voxel entries plan ok\n");
    return 0;
}
