// The host arithmetic of the carve (csrc/svo_voxel_plan.hpp, "voxel carve") as a program of its own: the scalar checks
// of the stage entry and the bytes a carving rebuild adds behind the prune's block. Arguments come in fives, "margin
// near ring width height": one line "ok" or "bad" each. Then one line per log2_capacity 6 .. 26: the offsets and bytes
// of the plan, checked here against the words a launch writes (four per tile of 256 entries).
#include <cstdio>
#include <cstdlib>

#include "../../stereo-svo-slam_amd/csrc/svo_voxel_plan.hpp"

int main(int argc, char** argv) {
    using namespace svo;
    for (int i = 1; i + 4 < argc; i += 5)
        printf("%s\n", voxel_carve_scalars_ok(strtof(argv[i], nullptr), strtof(argv[i + 1], nullptr), atoi(argv[i + 2]), atoi(argv[i + 3]),
                                              atoi(argv[i + 4])) ? "ok" : "bad");
    for (int log2 = VOXEL_LOG2_MIN; log2 <= VOXEL_LOG2_MAX; log2++) {
        const VoxelCarvePlan p = voxel_carve_plan(log2);
        const size_t words = (size_t)(VOXEL_TILE / 64) * (size_t)voxel_map_tiles(log2);
        if (p.ballots != 0 || p.counters < 8 * words || p.counters % 256 != 0 || p.bytes != p.counters + 256 || 64 * words < ((size_t)1 << log2)) {
            printf("plan %d is wrong\n", log2);
            return 1;
        }
        printf("plan %d %zu %zu %zu\n", log2, p.ballots, p.counters, p.bytes);
    }
    return 0;
}
