// map.hip — the keypoints of many keyframes, filtered and compacted into 16-byte map points (svo_map_point: kps3d bits,
// colour, flag bits), many regions in one call. The reference's viewer reply carries every keyframe's kps3d and
// colours (src/app/svo_slam_backend.cpp:18-110); a keyframe holds copies of earlier keyframes' points
// (merge_keypoints, src/lib/depth_calculator.cpp:88-130) that go stale, because the depth filter writes back to the
// origin keyframe only (src/lib/stereo_slam.cpp:205-226). Which points are current is in the device's planes (flags,
// keyframe_id, inlier_count), so the selection and the compaction run here.
//
// The host cuts every keyframe's set into tiles of at most MAP_TILE keypoints (MapTile) — it knows the counts — and
// numbers them; a region's tiles are consecutive. A workgroup takes one tile, a lane one keypoint. Two launches:
//
//  * map_count_kernel evaluates the predicate and writes the tile's kept count to tile_counts[index]: a 64-bit
//    __ballot per wave, popcount, the four waves through LDS.
//  * map_write_kernel sums tile_counts over the tiles of its region before it (a strided loop over the workgroup and
//    a reduction: a region can have more tiles than a workgroup has lanes), evaluates the predicate again, ranks the
//    kept lanes (mbcnt of the ballot inside a wave, the waves through LDS) and writes each kept point with one
//    16-byte store at first + before + rank. The last tile of a set also writes the set's kept count.
//
// The offsets are sums of what an earlier launch wrote: no workgroup waits for another, nothing is atomic, and the
// order (tile order, keypoint order) and so every byte is the same in every run. With a chunked table the count and
// write launches of a chunk follow those of the chunks before it on the stream; a tile reads only counts of tiles
// before it, so tile_counts (not part of the table) is all that has to survive a refill.
//
// Loads: the planes are 4-byte aligned only (keyframe slabs are carved at any offset), so lane i reads dword i of
// flags / keyframe_id / inlier_count / colour (coalesced dword loads). kps3d is 12-byte AoS: the tile's 3 n dwords
// are read as a contiguous stream into LDS and lane i picks dwords 3 i .. 3 i + 2 (odd stride: no bank conflict).
// 3 KB of LDS per workgroup; the kernels only move data (12 B per keypoint in the count launch, 28 B in and up to
// 16 B out in the write launch); their roof is HBM.
//
// Bounds: of a tile, keypoints [0, count) of the planes are read; of a region, records [first, first + kept) are
// written, and kept <= the region's keypoints, which the host has checked against the capacity.
#include "svo_tracker.hpp"

namespace svo {

constexpr int MAP_THREADS = 256;
constexpr int MAP_WAVES = MAP_THREADS / 64;
static_assert(MAP_TILE == MAP_THREADS, "one lane per keypoint of a tile");
static_assert(sizeof(svo_map_point) == 16 && sizeof(svo_kp3d) == 12, "record sizes of the C ABI");
constexpr uint32_t MAP_FLAG_BITS = SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY;

void map_tiles(const KpsDev& k, int n, int own_id, int set, int64_t first, int region_tile, std::vector<MapTile>& out) {
    const int set_tile = (int)out.size();
    int start = 0;
    do {
        MapTile t;
        t.kps3d = reinterpret_cast<const uint32_t*>(k.kps3d) + (size_t)start * 3;
        t.flags = k.flags + start;
        t.kf_id = k.kf_id + start;
        t.inl = k.inl + start;
        t.color = k.color + start;
        t.first = first;
        t.count = std::max(0, std::min(MAP_TILE, n - start));
        t.own_id = own_id;
        t.index = (int)out.size();
        t.region_tile = region_tile;
        t.set_tile = set_tile;
        start += MAP_TILE;
        t.set = start >= n ? set : -1;
        out.push_back(t);
    } while (start < n);
}

// is keypoint i of the tile kept? (flags: its flags word, 0 beyond the tile)
__device__ __forceinline__ bool map_keep(const MapTile& t, const svo_map_filter& f, int i, uint32_t& flags) {
    flags = 0;
    if (i >= t.count) return false;
    flags = G(t.flags)[i];
    bool keep = (flags & f.drop_flags) == 0;
    if (f.own_only) keep = keep && G(t.kf_id)[i] == t.own_id;
    return keep && G(t.inl)[i] >= f.min_inliers;
}

__global__ __launch_bounds__(MAP_THREADS) void map_count_kernel(const MapTile* __restrict__ tiles, svo_map_filter f,
                                                                int* __restrict__ tile_counts) {
    __shared__ int wave_n[MAP_WAVES];
    const MapTile t = G(tiles)[blockIdx.x];
    uint32_t flags;
    const bool keep = map_keep(t, f, threadIdx.x, flags);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < MAP_WAVES; w++) n += wave_n[w];
        G(tile_counts)[t.index] = n;
    }
}

__global__ __launch_bounds__(MAP_THREADS) void map_write_kernel(const MapTile* __restrict__ tiles, svo_map_filter f,
                                                                uint4* points, const int* tile_counts, int* set_counts) {
    __shared__ uint32_t xyz[MAP_TILE * 3];
    __shared__ long long wave_before[MAP_WAVES];
    __shared__ int wave_set[MAP_WAVES], wave_n[MAP_WAVES];
    const MapTile t = G(tiles)[blockIdx.x];
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    if (points)
        for (int k = i; k < t.count * 3; k += MAP_THREADS) xyz[k] = G(t.kps3d)[k];
    // kept points of the region's tiles before this one, and of those that belong to this tile's set
    long long before = 0;
    int in_set = 0;
    for (int j = t.region_tile + i; j < t.index; j += MAP_THREADS) {
        const int c = G(tile_counts)[j];
        before += c;
        if (j >= t.set_tile) in_set += c;
    }
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_down(before, o);
        in_set += __shfl_down(in_set, o);
    }
    uint32_t flags;
    const bool keep = map_keep(t, f, i, flags);
    const unsigned long long m = __ballot(keep);
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (lane == 0) {
        wave_before[wave] = before;
        wave_set[wave] = in_set;
        wave_n[wave] = __popcll(m);
    }
    __syncthreads();
    long long at = t.first;
    int set_n = 0;
    for (int w = 0; w < MAP_WAVES; w++) {
        at += wave_before[w];
        set_n += wave_set[w] + wave_n[w];
        if (w < wave) at += wave_n[w];
    }
    if (keep && points) {
        const uint32_t color = G(t.color)[i];
        uint4 r;
        r.x = xyz[3 * i]; r.y = xyz[3 * i + 1]; r.z = xyz[3 * i + 2];
        r.w = (color & 0xffffffu) | ((flags & MAP_FLAG_BITS) << 24);
        ((SVO_GP(uint4))points)[at + rank] = r;
    }
    if (i == 0 && set_counts && t.set >= 0) G(set_counts)[t.set] = set_n;
}

void launch_map(const MapTile* d_tiles, int n_tiles, const svo_map_filter& filter, svo_map_point* points, int* tile_counts,
                int* set_counts, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(map_count_kernel, dim3(n_tiles), dim3(MAP_THREADS), 0, stream, d_tiles, filter, tile_counts);
    hipLaunchKernelGGL(map_write_kernel, dim3(n_tiles), dim3(MAP_THREADS), 0, stream, d_tiles, filter,
                       reinterpret_cast<uint4*>(points), static_cast<const int*>(tile_counts), set_counts);
}

}  // namespace svo
