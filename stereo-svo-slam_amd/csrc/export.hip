// export.hip — SoA keypoint sets into the AoS records of the C ABI (svo_kp2d, svo_kp3d, svo_kp_info), many sets
// in one launch. The reference hands its state out one object at a time (StereoSlam::get_frame / get_keyframes,
// src/lib/stereo_slam.cpp:273-289: a Frame carries vector<KeyPoint2d>, vector<KeyPoint3d> and
// vector<KeyPointInformation>); the per-sequence getters of svo_ctx.hip restate that with twelve blocking
// copies per sequence and a host loop. This is the bulk form: the records are built on the GPU, byte for byte
// the getters' (a cleared record, then its fields: `_pad` is 0).
//
// The host cuts every set into tiles of at most EXPORT_TILE keypoints (ExportTile: the source arrays at the
// tile's first keypoint, the destination record, the count) — it knows the counts, no device scan. A workgroup
// takes one tile:
//
//  * kps2d / kps3d are AoS at the source already: the tile's 2 / 3 dwords per keypoint are copied as a stream,
//    16 bytes per lane where source and destination are 16-byte aligned (they are for the tracker: a segment
//    starts at a multiple of 4 records, a tile at a multiple of EXPORT_TILE), dword by dword otherwise;
//  * lane i reads keypoint i of the ten 4-byte planes (ten coalesced dword loads per wave: a plane only needs a
//    4-byte aligned base), builds the 11 dwords of its svo_kp_info and writes them to LDS at dword 11 i. The
//    stride is odd, so the 32 lanes of a ds_write_b32 group hit 32 different banks. After the barrier the tile's
//    records are one contiguous run of 11 n dwords in LDS and in the output: they leave as 16-byte stores
//    (contiguous ds_read_b128, contiguous global stores), the last 11 n mod 4 dwords as dword stores.
//
// 256 keypoints x 44 B = 11 KB of LDS per workgroup: 14 workgroups of four waves fit a CU's 160 KB, more than
// its wave slots hold, so LDS does not bound the occupancy. The kernel only moves data (64 B in, 64 B out per
// keypoint); its roof is HBM.
//
// Bounds: of a tile, keypoints 0 .. count-1 of every source array are read and records first .. first+count-1
// of every output array are written, nothing else (count = 0: nothing at all).
#include "svo_tracker.hpp"

namespace svo {

constexpr int EXPORT_THREADS = 256;
constexpr int INFO_DWORDS = sizeof(svo_kp_info) / 4;
static_assert(EXPORT_TILE == EXPORT_THREADS, "one lane per keypoint of a tile");
static_assert(sizeof(svo_kp_info) == 44 && sizeof(svo_kp2d) == 8 && sizeof(svo_kp3d) == 12, "record sizes of the C ABI");
static_assert(EXPORT_TILE * INFO_DWORDS % 4 == 0, "a full tile is whole 16-byte units");

ExportTile export_tile(const KpsDev& k, int start, int count, int64_t first) {
    ExportTile t;
    t.kps2d = reinterpret_cast<const uint32_t*>(k.kps2d + start);
    t.kps3d = reinterpret_cast<const uint32_t*>(k.kps3d + start);
    const void* planes[EXPORT_PLANES] = {k.flags, k.outl, k.inl, k.kf_id, k.kp_index, k.kfx, k.kfP, k.score, k.level_type, k.color};
    for (int i = 0; i < EXPORT_PLANES; i++) t.plane[i] = static_cast<const uint32_t*>(planes[i]) + start;
    t.first = first + start;
    t.count = count;
    t.pad_ = 0;
    return t;
}

// n dwords src -> dst by the whole workgroup
__device__ __forceinline__ void copy_dwords(SVO_GP(uint32_t) dst, SVO_GP(const uint32_t) src, int n) {
    int done = 0;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
        const int nv = n >> 2;
        for (int i = threadIdx.x; i < nv; i += EXPORT_THREADS) ((SVO_GP(uint4))dst)[i] = ((SVO_GP(const uint4))src)[i];
        done = nv << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += EXPORT_THREADS) dst[i] = src[i];
}

__global__ __launch_bounds__(EXPORT_THREADS) void export_pack_kernel(const ExportTile* __restrict__ tiles, uint32_t* out2d,
                                                                     uint32_t* out3d, uint32_t* out_info) {
    __shared__ uint4 rec4[EXPORT_TILE * INFO_DWORDS / 4];
    const ExportTile t = G(tiles)[blockIdx.x];
    const int n = t.count;
    if (out2d) copy_dwords(G(out2d) + t.first * 2, G(t.kps2d), n * 2);
    if (out3d) copy_dwords(G(out3d) + t.first * 3, G(t.kps3d), n * 3);
    if (!out_info) return;
    uint32_t* rec = reinterpret_cast<uint32_t*>(rec4);
    const int i = threadIdx.x;
    if (i < n) {
        const uint32_t flags = G(t.plane[0])[i], lt = G(t.plane[8])[i], color = G(t.plane[9])[i];
        uint32_t* r = rec + i * INFO_DWORDS;
        r[0] = G(t.plane[7])[i];                                   // score
        r[1] = lt & 0xffu;                                         // level
        r[2] = (lt >> 8) & 0xffu;                                  // type
        r[3] = G(t.plane[3])[i];                                   // keyframe_id
        r[4] = G(t.plane[4])[i];                                   // keypoint_index
        r[5] = (color & 0xffffffu) | ((flags & SVO_IGNORE_DURING_REFINEMENT) ? 1u << 24 : 0u);   // color[3], ignore_during_refinement
        r[6] = ((flags & SVO_IGNORE_COMPLETELY) ? 1u : 0u) | ((flags & SVO_IGNORE_TEMPORARY) ? 1u << 8 : 0u);   // ..., _pad = 0
        r[7] = G(t.plane[1])[i];                                   // outlier_count
        r[8] = G(t.plane[2])[i];                                   // inlier_count
        r[9] = G(t.plane[5])[i];                                   // kf_inv_depth
        r[10] = G(t.plane[6])[i];                                  // kf_variance
    }
    __syncthreads();
    SVO_GP(uint32_t) out = G(out_info) + t.first * INFO_DWORDS;
    const int nd = n * INFO_DWORDS;
    int done = 0;
    if (((uintptr_t)out & 15) == 0) {
        const int nv = nd >> 2;
        for (int k = i; k < nv; k += EXPORT_THREADS) ((SVO_GP(uint4))out)[k] = rec4[k];
        done = nv << 2;
    }
    for (int k = done + i; k < nd; k += EXPORT_THREADS) out[k] = rec[k];
}

void launch_export(const ExportTile* d_tiles, int n_tiles, svo_kp2d* kps2d, svo_kp3d* kps3d, svo_kp_info* info,
                   hipStream_t stream) {
    if (n_tiles <= 0 || (!kps2d && !kps3d && !info)) return;
    hipLaunchKernelGGL(export_pack_kernel, dim3(n_tiles), dim3(EXPORT_THREADS), 0, stream, d_tiles,
                       reinterpret_cast<uint32_t*>(kps2d), reinterpret_cast<uint32_t*>(kps3d), reinterpret_cast<uint32_t*>(info));
}

}  // namespace svo
