// voxel_plan_check.cpp — csrc/svo_voxel_plan.hpp without a GPU: the bytes of a map, the load bound at and around
// its limit and at values that would wrap, spans and regions an entry accepts, the tiles of a span and of a map, and
// the staging of an extraction (the blocks are carved out of a real array and written through, so that the sanitizers
// see an overlap or an index past the end). Prints the homes of the keys given as arguments in tables of 2^6 and
// 2^26 entries, then "voxel plan ok".
#include <cstdio>
#include <cstdlib>
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

// the blocks of a plan are disjoint, in order, 256-byte aligned and inside plan.bytes
void check_plan(uint64_t kept, size_t temp) {
    const VoxelExtractPlan p = voxel_extract_plan(kept, temp);
    std::vector<unsigned char> block(p.bytes, 0);
    const size_t off[5] = {p.keys_in, p.keys_out, p.index_in, p.index_out, p.sort_temp};
    const size_t len[5] = {8 * (size_t)kept, 8 * (size_t)kept, 4 * (size_t)kept, 4 * (size_t)kept, temp};
    for (int b = 0; b < 5; b++) {
        CHECK(off[b] % 256 == 0 && off[b] + len[b] <= p.bytes);
        for (size_t i = 0; i < len[b]; i++) block[off[b] + i]++;
    }
    for (unsigned char v : block) CHECK(v <= 1);
    CHECK(p.bytes % 256 == 0 && p.bytes < 24 * (size_t)kept + temp + 5 * 256);
}

}  // namespace

int main(int argc, char** argv) {
    // bytes: header + 40 per entry; nothing outside 6 .. 26
    CHECK(voxel_map_bytes(6) == 256 + 40 * 64 && voxel_map_bytes(10) == 256 + 40 * 1024 && voxel_map_bytes(26) == 256 + ((size_t)40 << 26));
    CHECK(voxel_map_bytes(5) == 0 && voxel_map_bytes(27) == 0 && voxel_map_bytes(-1) == 0 && voxel_map_bytes(64) == 0);
    CHECK(voxel_log2_ok(6, false) && !voxel_log2_ok(6, true) && !voxel_log2_ok(9, true) && voxel_log2_ok(10, true) && voxel_log2_ok(26, true));
    for (int l = VOXEL_LOG2_MIN; l <= VOXEL_LOG2_MAX; l++) CHECK(voxel_map_bytes(l) % 256 == 0 && ((size_t)8 << l) % 256 == 0);
    // the load bound: capacity - capacity / 4, on the bound, without wrapping
    CHECK(voxel_load_limit(6) == 48 && voxel_load_limit(10) == 768 && voxel_load_limit(26) == (uint64_t)3 << 24);
    CHECK(voxel_load_ok(0, 48, 6) && !voxel_load_ok(0, 49, 6) && voxel_load_ok(40, 8, 6) && !voxel_load_ok(40, 9, 6) && voxel_load_ok(48, 0, 6));
    CHECK(!voxel_load_ok(49, 0, 6) && !voxel_load_ok(1, UINT64_MAX, 6) && !voxel_load_ok(UINT64_MAX, 1, 6) && !voxel_load_ok(UINT64_MAX, UINT64_MAX, 26));
    uint64_t sum = 0;
    CHECK(voxel_add_records(sum, 5) && voxel_add_records(sum, 0) && sum == 5 && !voxel_add_records(sum, -1) && sum == 5);
    sum = UINT64_MAX - 3;
    CHECK(voxel_add_records(sum, 3) && sum == UINT64_MAX && !voxel_add_records(sum, 1) && sum == UINT64_MAX);
    sum = 0;
    CHECK(voxel_add_records(sum, INT64_MAX) && voxel_add_records(sum, INT64_MAX) && voxel_add_records(sum, 1) && !voxel_add_records(sum, 1));
    // spans and regions
    CHECK(voxel_span_ok(0, 0) && voxel_span_ok(8, 0) && voxel_span_ok(4096, 1) && voxel_span_ok(16, INT64_C(1) << 40));
    CHECK(!voxel_span_ok(4096, -1) && !voxel_span_ok(0, 1) && !voxel_span_ok(4104, 1) && !voxel_span_ok(4097, 7));
    CHECK(voxel_span_tiles(-5) == 0 && voxel_span_tiles(0) == 0 && voxel_span_tiles(1) == 1 && voxel_span_tiles(256) == 1 && voxel_span_tiles(257) == 2);
    CHECK(voxel_span_tiles((INT64_C(1) << 40) + 1) == (INT64_C(1) << 32) + 1 && voxel_span_tiles(INT64_MAX - 255) == (INT64_MAX - 255) / 256 && voxel_span_tiles(INT64_MAX) == INT64_MAX / 256 + 1);
    CHECK(voxel_map_tiles(6) == 1 && voxel_map_tiles(8) == 1 && voxel_map_tiles(9) == 2 && voxel_map_tiles(26) == 1 << 18);
    CHECK(voxel_region_ok(0, 0, 0) && voxel_region_ok(0, 10, 10) && voxel_region_ok(10, 0, 10) && voxel_region_ok(3, 7, 10));
    CHECK(!voxel_region_ok(3, 8, 10) && !voxel_region_ok(-1, 1, 10) && !voxel_region_ok(1, -1, 10) && !voxel_region_ok(11, 0, 10));
    CHECK(!voxel_region_ok(INT64_MAX, INT64_MAX, INT64_MAX - 1) && !voxel_region_ok(1, INT64_MAX, INT64_MAX) && voxel_region_ok(1, INT64_MAX - 1, INT64_MAX));
    CHECK(voxel_extract_fits(0, 0) && voxel_extract_fits(5, 5) && !voxel_extract_fits(6, 5) && !voxel_extract_fits(-1, 5) && !voxel_extract_fits(0, -1));
    // staging
    CHECK(voxel_offsets_bytes(6) == 256 && voxel_offsets_bytes(14) == 512 && voxel_offsets_bytes(26) == ((size_t)1 << 20) + 256);
    for (uint64_t kept : {(uint64_t)0, (uint64_t)1, (uint64_t)31, (uint64_t)32, (uint64_t)33, (uint64_t)48, (uint64_t)70000, (uint64_t)786432})
        for (size_t temp : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)100001}) check_plan(kept, temp);
    // placement
    CHECK(voxel_home(0, 6) == 0 && voxel_home(1, 6) == (VOXEL_HASH >> 58) && voxel_home(1, 26) == (VOXEL_HASH >> 38));
    for (uint64_t k : {(uint64_t)1, (uint64_t)12345, VOXEL_EMPTY - 1, (uint64_t)1 << 62})
        for (int l = VOXEL_LOG2_MIN; l <= VOXEL_LOG2_MAX; l++) CHECK(voxel_home(k, l) < ((uint64_t)1 << l));
    std::printf("homes:");
    for (int i = 1; i < argc; i++) {
        const uint64_t k = std::strtoull(argv[i], nullptr, 10);
        std::printf(" %llu %llu", (unsigned long long)voxel_home(k, 6), (unsigned long long)voxel_home(k, 26));
    }
    std::printf("\nvoxel plan ok\n");
    return 0;
}
