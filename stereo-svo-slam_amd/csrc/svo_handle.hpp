// svo_handle.hpp — what the five files of the stage-level C API share (svo_capi.hip, svo_capi_tables.hip,
// svo_capi_check.hip, svo_capi_voxel.hip, svo_capi_sgm.hip; nothing else includes it): the handle, its device ring for argument blocks, its grow-only
// workspaces and the check of a caller's keypoint planes.
#pragma once

#include <cstdint>
#include <vector>

#include "svo_host.hpp"
#include "svo_kernels.hpp"
#include "svo_tracker.hpp"

// A device block that only grows, for one entry's tables: exactly the bytes of the largest call so far.
struct svo_workspace {
    svo::DevPtr<uint8_t> ptr;
    size_t bytes = 0;
    // at least `need` bytes; a larger block replaces the old one once `stream` is idle (an earlier call may still
    // read it). On failure the workspace is empty.
    int reserve(size_t need, hipStream_t stream) {
        if (need <= bytes) return SVO_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        ptr.reset();
        bytes = 0;
        HIP_TRY(svo::dev_malloc(ptr, need));
        bytes = need;
        return SVO_OK;
    }
};

struct svo_handle {
    int device;
    hipStream_t stream = nullptr;   // the caller's (svo_handle_set_stream), not owned
    int max_kps;
    svo::DevPtr<uint8_t> ring;      // device ring for argument blocks
    size_t ring_cap = 1 << 20, ring_off = 0;
    svo::DevPtr<float> sia_kpws;    // [9][rec_cap] per-keypoint values of the BIG alignment path
    svo::DevPtr<float> sia_rec;     // [7][68][rec_cap] per-level alignment records
    int rec_cap;
    int exact_pinv = 1;             // reference-order Gauss-Newton by default
    svo_workspace remap_ws;         // svo_remap_linear{,_multi}: the maps in the kernels' form + the image and chunk tables
    svo_workspace rigcam_ws;        // svo_build_rectify_maps: the camera table
    svo_workspace ingest_ws;        // svo_convert_frames: the image table
    svo_workspace export_ws;        // svo_pack_keypoints: the tile table
    svo_workspace copy_ws;          // svo_copy_segments: the tile table
    svo_workspace map_ws;           // svo_pack_map_points: the tile counts of a call, then the tile table
    svo_workspace view_ws;          // svo_render_views: the tile table
    svo_workspace scene_ws;         // svo_render_scene: the sets and image records of a call, then the tile table
    svo_workspace scene_cloud_ws;   // svo_render_scene_clouds: the key planes of a call, the plane table, then the span table
    svo_workspace ar_ws;            // svo_render_ar: the draws, image records, work list and screen records of a call, then the tile table
    svo_workspace dense_ws;         // svo_dense_disparity: the image table
    svo_workspace sgm_ws;           // svo_sgm_aggregate, svo_dense_disparity_sgm: the two image tables of a chunk, then its sums, volumes and count planes
    svo_workspace cloud_ws;         // svo_cloud_points: the two image tables of a chunk, then its planes, tile counts and pose matrices
    svo_workspace voxel_ws;         // svo_voxel_fuse: the map table, the maps' headers, the span table; svo_voxel_extract: the tile offsets
    svo_workspace voxel_sort_ws;    // svo_voxel_extract: the (key, entry) pairs before and after the sort and the sort's temporary storage
};

#define CHECK_H(h)                                                   \
    do {                                                             \
        if (!(h)) return svo_set_error(SVO_ERR_INVALID, "null handle");       \
        HIP_TRY(hipSetDevice((h)->device));                          \
    } while (0)

// copy `count` host blocks into the device ring (stream ordered); returns the device address
template <typename T>
int stage(svo_handle* h, const T* host, size_t count, T** dev) {
    const size_t bytes = (sizeof(T) * count + 255) & ~(size_t)255;
    if (bytes > h->ring_cap) return svo_set_error(SVO_ERR_CAPACITY, "argument blocks do not fit the ring");
    if (h->ring_off + bytes > h->ring_cap) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->ring_off = 0;
    }
    T* d = reinterpret_cast<T*>(h->ring.get() + h->ring_off);
    h->ring_off += bytes;
    HIP_TRY(hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
    *dev = d;
    return SVO_OK;
}
template <typename T>
int stage(svo_handle* h, const T& host, T** dev) { return stage(h, &host, 1, dev); }
template <typename T>
int stage(svo_handle* h, const std::vector<T>& host, T** dev) { return stage(h, host.data(), host.size(), dev); }
inline int stage_n(svo_handle* h, int n, int** d_n) { return stage(h, &n, 1, d_n); }

// launch done: the first error of the launch or the wait
inline int finish_launch(svo_handle* h) {
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(launched);
    return SVO_OK;
}

// the twelve planes of a keypoint set as bits, in the order of svo_kps_planes
enum : unsigned {
    KP_KPS2D = 1 << 0, KP_KPS3D = 1 << 1, KP_FLAGS = 1 << 2, KP_KF_ID = 1 << 3, KP_KP_INDEX = 1 << 4, KP_OUTL = 1 << 5,
    KP_INL = 1 << 6, KP_KFX = 1 << 7, KP_KFP = 1 << 8, KP_SCORE = 1 << 9, KP_LEVEL_TYPE = 1 << 10, KP_COLOR = 1 << 11,
    KP_ALL = (1 << 12) - 1,
    KP_MAP = KP_KPS3D | KP_FLAGS | KP_KF_ID | KP_INL | KP_COLOR,          // what the map and scene kernels read
    KP_VIEW = KP_KPS2D | KP_FLAGS | KP_LEVEL_TYPE | KP_COLOR,             // what the view kernel's markers read
};

// d = the planes of `k` that `planes` names, every other one null. False: one of them is not 4-byte aligned, or is
// null although the set is `non_empty`.
inline bool take_planes(const svo_keypoints& k, unsigned planes, bool non_empty, svo::KpsDev& d) {
    bool ok = true;
    auto take = [&](unsigned bit, auto*& dst, auto* src) {
        if (!(planes & bit)) return;
        dst = src;
        ok = ok && (src || !non_empty) && !((uintptr_t)src & 3);
    };
    d = svo::KpsDev{};
    take(KP_KPS2D, d.kps2d, k.kps2d);
    take(KP_KPS3D, d.kps3d, k.kps3d);
    take(KP_FLAGS, d.flags, k.flags);
    take(KP_KF_ID, d.kf_id, k.keyframe_id);
    take(KP_KP_INDEX, d.kp_index, k.keypoint_index);
    take(KP_OUTL, d.outl, k.outlier_count);
    take(KP_INL, d.inl, k.inlier_count);
    take(KP_KFX, d.kfx, k.kf_inv_depth);
    take(KP_KFP, d.kfP, k.kf_variance);
    take(KP_SCORE, d.score, k.score);
    take(KP_LEVEL_TYPE, d.level_type, k.level_type);
    take(KP_COLOR, d.color, k.color);
    return ok;
}
