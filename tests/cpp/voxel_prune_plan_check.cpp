// voxel_prune_plan_check.cpp — the prune's part of csrc/svo_voxel_plan.hpp without a GPU: the staging block of a prune
// (its two planes carved out of a real array and written through, so that the sanitizers see an overlap or an index
// past the end), the 1 GiB bound at and around its limit and at values that would wrap, the reinsert pass's
// workgroups, and the centre's index by the key rule at its edges. Prints the index of every (coordinate, voxel) pair
// given as arguments (-1: outside), then "voxel prune plan ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// the planes of a plan are disjoint, the records 16-byte and the keys 8-byte aligned, all inside plan.bytes
void check_plan(uint64_t n) {
    VoxelPrunePlan p;
    CHECK(voxel_prune_plan(n, p));
    CHECK(p.bytes == voxel_up256(40 * (size_t)n) && p.bytes % 256 == 0 && p.acc % 16 == 0 && p.keys % 8 == 0);
    std::vector<unsigned char> block(p.bytes, 0);
    const size_t off[2] = {p.acc, p.keys}, len[2] = {32 * (size_t)n, 8 * (size_t)n};
    for (int b = 0; b < 2; b++) {
        CHECK(off[b] + len[b] <= p.bytes);
        for (size_t i = 0; i < len[b]; i++) block[off[b] + i]++;
    }
    for (unsigned char v : block) CHECK(v <= 1);
}

int index_of(float c, float voxel) {
    int32_t i = -7;
    if (!voxel_center_index(c, voxel, i)) {
        CHECK(i == -7);                                    // nothing is written for a centre outside
        return -1;
    }
    return i;
}

}  // namespace

int main(int argc, char** argv) {
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)6, (uint64_t)7, (uint64_t)31, (uint64_t)48, (uint64_t)768, (uint64_t)70001,
                       (uint64_t)786432})
        check_plan(n);
    // the bound: 40 n rounded up to 256 must not exceed 1 GiB
    VoxelPrunePlan p;
    const uint64_t most = VOXEL_PRUNE_STAGING_MAX / 40;    // 26843545: 1073741800 bytes, up256 -> 1073741824
    CHECK(VOXEL_PRUNE_STAGING_MAX == (size_t)1 << 30 && most == 26843545);
    CHECK(voxel_prune_plan(most, p) && p.bytes == VOXEL_PRUNE_STAGING_MAX && p.keys == 32 * (size_t)most);
    CHECK(!voxel_prune_plan(most + 1, p) && p.bytes == 0);
    CHECK(!voxel_prune_plan(voxel_load_limit(26), p) && voxel_prune_plan(voxel_load_limit(24), p) && voxel_prune_plan(voxel_load_limit(25), p));
    CHECK(!voxel_prune_plan(UINT64_MAX, p) && !voxel_prune_plan(UINT64_MAX / 40 + 1, p) && !voxel_prune_plan((uint64_t)1 << 62, p));
    CHECK(voxel_prune_tiles(0) == 0 && voxel_prune_tiles(1) == 1 && voxel_prune_tiles(256) == 1 && voxel_prune_tiles(257) == 2);
    CHECK(voxel_prune_tiles(most) == 104858 && voxel_prune_tiles(voxel_load_limit(26)) == 196608);
    // the centre's index: the key rule, in float32
    CHECK(index_of(0.f, 1.f) == 1048576 && index_of(-0.f, 1.f) == 1048576 && index_of(-1e-10f, 1.f) == 1048575 && index_of(2.f, 1.f) == 1048578);
    CHECK(index_of(-3.f, 1.f) == 1048573 && index_of(1048575.5f, 1.f) == 2097151 && index_of(-1048575.f, 1.f) == 1);
    CHECK(index_of(1048576.f, 1.f) == -1 && index_of(-1048575.5f, 1.f) == -1 && index_of(-1048576.f, 1.f) == -1 && index_of(3e38f, 0.3f) == -1);
    CHECK(index_of(std::numeric_limits<float>::quiet_NaN(), 1.f) == -1 && index_of(std::numeric_limits<float>::infinity(), 1.f) == -1);
    CHECK(index_of(-std::numeric_limits<float>::infinity(), 0.05f) == -1);
    std::printf("centres:");
    for (int i = 1; i + 1 < argc; i += 2) std::printf(" %d", index_of(std::strtof(argv[i], nullptr), std::strtof(argv[i + 1], nullptr)));
    std::printf("\nvoxel prune plan ok\n");
    return 0;
}
