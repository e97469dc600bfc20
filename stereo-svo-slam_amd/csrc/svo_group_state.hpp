// svo_group_state.hpp — the state of one sequence group, internal to the group: only its translation units
// (svo_group.hip: storage, creation, settings, the end of a sequence; svo_group_step.hip: the step;
// svo_group_export.hip: the bulk export; svo_group_map.hip: the map export; svo_group_view.hip: the views;
// svo_group_scene.hip: the scenes; svo_group_ar.hip: the ar pictures;
// svo_group_snapshot.hip: save and load;
// svo_group_pose.hip: the batched pose-filter updates) and the per-sequence getters of
// svo_ctx_get.hip include it. Everyone else drives a group through the opaque interface of svo_group.hpp.
//
// Host side = bookkeeping only: image-set pool, argument blocks, the 12-state
// pose Kalman filter (stereo_slam.cpp:296-359) and the keyframe decision. All
// image and keypoint work runs in the kernels of pyramid/sia/klt/reproj/depth/
// keyframe.hip.
//
// HBM layout per sequence:
//   image sets  : left halfSample pyramid | right level 0 | Gaussian levels 1,2
//                 (rows padded to 64 B). The current, the previous and every
//                 keyframe's set stay resident (288 GB: ~1 MB per 752x480 set).
//   keypoints   : two SoA sets (KpsDev) ping-ponged by the order-preserving
//                 compactions; per-point scratch (tracked, err, disparity).
//   keyframes   : table of KfDev records (a ring over the resident ids) + per-keyframe SoA copies.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "svo_group.hpp"
#include "svo_host.hpp"
#include "svo_tracker.hpp"
namespace svo {

// ------------------------------------------------------ 12-state pose filter
// cv::KalmanFilter(12,12) as configured in the StereoSlam ctor
// (src/lib/stereo_slam.cpp:29-41) and driven by update_pose (:296-359).
// cv::gemm on float data: double accumulation, float store; the gain comes
// out of cv::solve(DECOMP_SVD) (Jacobi SVD, svo_device.hpp).
struct PoseFilter {
    static constexpr int N = 12;
    float statePre[N], statePost[N];
    float A[N * N], Hm[N * N], Q[N * N], R[N * N];
    float errorCovPre[N * N], errorCovPost[N * N], gain[N * N];

    static void identity(float* m, float v) {
        std::memset(m, 0, sizeof(float) * N * N);
        for (int i = 0; i < N; i++) m[i * N + i] = v;
    }
    void init() {
        std::memset(this, 0, sizeof(*this));
        identity(A, 1.f); identity(Hm, 1.f); identity(Q, 100.f); identity(R, 1.f);
        identity(errorCovPost, 1.f);
    }
    static void gemm(const float* a, const float* b, bool bt, double alpha, const float* c,
                     double beta, float* d, int m, int k, int n) {
        float tmp[N * N];
        for (int i = 0; i < m; i++)
            for (int j = 0; j < n; j++) {
                double s = 0;
                for (int p = 0; p < k; p++)
                    s += (double)a[i * k + p] * (double)(bt ? b[j * k + p] : b[p * n + j]);
                s *= alpha;
                if (c) s += (double)c[i * n + j] * beta;
                tmp[i * n + j] = (float)s;
            }
        std::memcpy(d, tmp, sizeof(float) * m * n);
    }
    static void solve_svd(const float* Am, const float* B, float* X) {
        float At[N][N], Vt[N][N], W[N];
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) At[i][j] = Am[j * N + i];
        jacobi_svd<N, N>(At, W, Vt);
        for (int i = 0; i < N * N; i++) X[i] = 0;
        double threshold = 0;
        for (int i = 0; i < N; i++) threshold += W[i];
        threshold *= (float)(DBL_EPSILON * 2);
        for (int i = 0; i < N; i++) {
            double wi = W[i];
            if (std::fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            double buffer[N];
            for (int j = 0; j < N; j++) buffer[j] = 0;
            for (int r = 0; r < N; r++) {
                const float s = At[i][r];
                for (int j = 0; j < N; j++) buffer[j] = buffer[j] + (double)(s * B[r * N + j]);
            }
            for (int j = 0; j < N; j++) buffer[j] *= wi;
            for (int r = 0; r < N; r++) {
                const float s = Vt[i][r];
                for (int j = 0; j < N; j++) X[r * N + j] = (float)(X[r * N + j] + s * buffer[j]);
            }
        }
    }
    void predict() {
        float temp1[N * N];
        gemm(A, statePost, false, 1, nullptr, 0, statePre, N, N, 1);
        gemm(A, errorCovPost, false, 1, nullptr, 0, temp1, N, N, N);
        gemm(temp1, A, true, 1, Q, 1, errorCovPre, N, N, N);
        std::memcpy(statePost, statePre, sizeof(statePre));
        std::memcpy(errorCovPost, errorCovPre, sizeof(errorCovPre));
    }
    void correct(const float* z) {
        float temp2[N * N], temp3[N * N], temp4[N * N], temp5[N], hx[N];
        gemm(Hm, errorCovPre, false, 1, nullptr, 0, temp2, N, N, N);
        gemm(temp2, Hm, true, 1, R, 1, temp3, N, N, N);
        solve_svd(temp3, temp2, temp4);
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) gain[i * N + j] = temp4[j * N + i];
        gemm(Hm, statePre, false, 1, nullptr, 0, hx, N, N, 1);
        for (int i = 0; i < N; i++) temp5[i] = z[i] - hx[i];
        gemm(gain, temp5, false, 1, statePre, 1, statePost, N, N, 1);
        gemm(gain, temp2, false, -1, errorCovPre, 1, errorCovPost, N, N, N);
    }
    // StereoSlam::update_pose
    void update(const float pose[6], const float speed[6], const float pv[6], const float sv[6],
                double dt, float filtered[6]) {
        for (int i = 0; i < 6; i++) A[i * N + 6 + i] = (float)dt;
        predict();
        for (int i = 0; i < 6; i++) { R[i * N + i] = pv[i]; R[(6 + i) * N + 6 + i] = sv[i]; }
        float z[N];
        for (int i = 0; i < 6; i++) { z[i] = pose[i]; z[6 + i] = speed[i]; }
        correct(z);
        for (int i = 0; i < 6; i++) filtered[i] = statePost[i];
    }
};

struct ImageSet {
    uint8_t* base = nullptr;
    ImgView left[SVO_MAX_PYRAMID_LEVELS];
    ImgView right;
    ImgView lk[SVO_LK_LEVELS];
    ImgView own_left0, own_right;     // the set's own level-0 storage (left[0] / right alias the caller's
                                      // images instead with SVO_MEM_DEVICE_BORROW)
    int refs = 0;
};

// where the views of an image set lie in its storage (computed once per group)
struct SetLayout {
    ImageSet views;                   // sizes and strides; data: null
    size_t left[SVO_MAX_PYRAMID_LEVELS], right, lk[SVO_LK_LEVELS];   // byte offsets
    size_t bytes;
};

struct FrameResult {            // device -> host, one per sequence and frame
    float pose_sia[6];
    float pose_refined[6];
    float sia_cost, reproj_cost;
    int inside, overflow, kf_n, old_count;
    int min_kf;                 // smallest origin-keyframe id of the frame's keypoints (compact_kernel) ...
    unsigned live_kf[2];        // ... and which of the 64 keyframes from there on still have keypoints in the frame
    svo_gn_trace sia_trace[SVO_MAX_PYRAMID_LEVELS];
    svo_gn_trace reproj_trace;
};

struct KfHost {
    ImageSet* set;              // null once the keyframe has given its image set back
    float pose[6];
    int n;
    KpsDev kps;                 // device arrays, carved out of one slab (kps.n: unused)
};

// The keyframes of a sequence by id. Ids keep counting up over the whole run; [first(), size()) are resident and
// the ones below were trimmed (drop_below). Every host index by id goes through here, so nothing else knows the
// offset; a range-for visits the resident ones, oldest first.
class KfList {
  public:
    int first() const { return first_; }
    size_t size() const { return (size_t)first_ + v_.size(); }       // ids given out so far (not: resident keyframes)
    int resident() const { return (int)v_.size(); }
    bool empty() const { return v_.empty(); }                        // (a run with keyframes has a resident one: the newest)
    KfHost& operator[](size_t id) { return v_[id - (size_t)first_]; }
    const KfHost& operator[](size_t id) const { return v_[id - (size_t)first_]; }
    KfHost& back() { return v_.back(); }
    const KfHost& back() const { return v_.back(); }
    void push_back(const KfHost& k) { v_.push_back(k); }
    std::vector<KfHost>::iterator begin() { return v_.begin(); }
    std::vector<KfHost>::iterator end() { return v_.end(); }
    std::vector<KfHost>::const_iterator begin() const { return v_.begin(); }
    std::vector<KfHost>::const_iterator end() const { return v_.end(); }
    void drop_below(int id) {                                        // first() <= id <= size()
        v_.erase(v_.begin(), v_.begin() + (id - first_));
        first_ = id;
    }
    void clear(int first = 0) { v_.clear(); first_ = first; }        // no keyframes; the next one gets id `first`
  private:
    std::vector<KfHost> v_;
    int first_ = 0;
};

struct Seq {
    KpsDev kps[2];
    int cur = 0;
    int* d_n = nullptr;          // [2] keypoint counts of the two sets
    svo_kp2d* tracked = nullptr;
    float* klt_err = nullptr;
    uint8_t* klt_status = nullptr;
    float* disparity = nullptr;
    float* sia_rec = nullptr;        // per-level alignment records (sia_prep_kernel)
    float* sia_kpws = nullptr;
    PoseMats* sia_mats = nullptr;    // rotation matrices of the aligned pose (sia_gn_kernel -> klt_track_kernel)
    uint8_t* tmpl_base = nullptr;    // KLT template cache: tmpl_kf blocks (a ring over the sequence's keyframes)
    uint8_t* tmpl_valid = nullptr;   // their "stored" flags
    KfDev* d_kfs = nullptr;          // the keyframe table: a ring of svo_group::max_kf records, keyframe id in slot id & (max_kf - 1)
    KfList kfs;                      // kfs.first() <= kfs_retired <= kfs.size() - 1 (while there is a keyframe)
    int kfs_retired = 0;             // keyframes [0, kfs_retired) have given their image sets back
    DetCell* det = nullptr; int* n_det = nullptr;
    DetCell* sel = nullptr; int* sel_level = nullptr; int* sel_cell = nullptr; int* occupied = nullptr;
    uint32_t* color_lcg = nullptr;
    std::vector<std::unique_ptr<ImageSet>> sets;   // every image set of the sequence; the rest point into these
    std::vector<ImageSet*> free_sets;
    ImageSet* cur_set = nullptr;
    ImageSet* prev_set = nullptr;
    // the camera rig the slot is bound to (grp_assign_rigs; 0: the ctx's own), the settings its sequences track with
    // (the ctx's integer settings, the rig's floats), and for rig >= 1 the storage of its left and right
    // rectification maps (owned by the ctx; null: the rig has none). Rig 0 rectifies through svo_group::rect.
    int rig = 0;
    svo_camera_settings cam{};
    const uint8_t* rig_maps[2] = {nullptr, nullptr};
    // host state
    PoseFilter kf;
    int frame_id = -1;               // -1: the slot is EMPTY (no sequence yet, or ended: end_sequence); its next frame is frame 0
    int run = 0;                     // ordinal of the slot's current (or next) sequence
    double ts = 0;
    float pose[6] = {0, 0, 0, 0, 0, 0};
    std::vector<svo_pose> trajectory;
    svo_frame_stats stats;
    int n_host = 0;
    // pose-filter update of the last frame, deferred so that it overlaps the next frame's kernels
    bool pending = false;
    float pending_pose[6] = {0, 0, 0, 0, 0, 0};
    double pending_ts = 0;
};

// what stays of a sequence that svo_ctx_restart_sequences ended (host memory only)
struct FinishedRun {
    svo_run_info info;               // (info.seq: index in the group)
    std::vector<svo_pose> trajectory;
};

// one kernel's argument blocks: slot i of the pinned array `h` goes up to slot i of the device array `d`
template <typename T>
struct ArgArray {
    using type = T;
    T* h = nullptr;
    T* d = nullptr;
};

// every kernel's argument array, carved in this order out of one pinned block and one device block: the
// tracked-frame arrays first, so that a tracked frame uploads them as one prefix copy (frame_bytes), and right behind
// them the chunk table of a multi-map remap, which a step that has one uploads in the same copy (frame_rig_bytes)
struct ArgBlocks {
    ArgArray<PyrArgs> pyr;
    ArgArray<CompactArgs> compact;
    ArgArray<SiaArgs> sia;
    ArgArray<KltArgs> klt;
    ArgArray<ReprojArgs> reproj;
    ArgArray<SsdArgs> ssd;
    ArgArray<FilterArgs> filter;
    ArgArray<float[8]> guess;        // per sequence: the predicted pose
    ArgArray<RemapChunk> remap_chunk;    // the chunks of a step's multi-map remap (slots on different rigs)
    ArgArray<DetectArgs> detect;
    ArgArray<MergeArgs> merge;
    ArgArray<KfInitArgs> kf_init;
    ArgArray<int> enable;            // (reserved)
    ArgArray<KfDev> kf_record;       // per sequence: staging of its newest keyframe's record
    template <typename F> void frame_arrays(F f) { f(pyr); f(compact); f(sia); f(klt); f(reproj); f(ssd); f(filter); f(guess); }
    template <typename F> void rig_arrays(F f) { f(remap_chunk); }
    template <typename F> void keyframe_arrays(F f) { f(detect); f(merge); f(kf_init); f(enable); f(kf_record); }
    PinnedPtr<uint8_t> host;
    uint8_t* dev = nullptr;
    size_t frame_bytes = 0, frame_rig_bytes = 0, bytes = 0;
};

// A device block of the group that is made by the first job that needs it and replaced when outgrown: `bytes` is
// what dev_alloc booked and what dev_release gives back. Mirror: a pinned block of the same size goes with it.
template <typename T, bool Mirror = false>
struct GrowBlock {
    T* p = nullptr;
    size_t bytes = 0;
    PinnedPtr<T> host;               // (Mirror only)
    int reserve(svo_group* c, size_t want);   // the block holds `want` bytes; a grown one replaces the old
};

}  // namespace svo

struct svo_group {
    svo::Stream stream;                   // (declared first: destroyed after everything that uses it)
    int device, B, width, height, cap, rec_cap, max_kf, n_lk, det_levels, max_cells, merge_cells;
    svo_camera_settings cam;
    std::vector<svo::DevPtr<void>> dev_mem;   // every device allocation of the group (dev_alloc)
    std::vector<svo::Seq> seqs;
    svo::ArgBlocks args;
    // d_res | d_n_all | d_inside are one device block mirrored by one pinned block: the end-of-frame
    // read-back is a single copy, the keyframe decision reads back only the B inside-counters
    svo::PinnedPtr<uint8_t> readback_host;
    svo::FrameResult* d_res = nullptr; svo::FrameResult* h_res = nullptr;
    int* h_n = nullptr;          // pinned [B*2]
    int* d_n_all = nullptr;      // [B*2]
    int* d_inside = nullptr; int* h_inside = nullptr;
    size_t readback_bytes = 0;
    // host-resident input frames land here first (2 x B frames; runs of contiguous frames as one
    // copy) and are then ingested like device-resident ones
    uint8_t* d_stage_in = nullptr; size_t stage_frame_bytes = 0;
    // rectification (svo_ctx_set_rectification): the two maps of rig 0, or null (a slot on another rig: Seq::rig_maps);
    // the image table of the remap launch (left images of the active sequences that remap, then their right images:
    // in slot order while they share their maps, else sorted by map) in a pinned block and its device mirror
    const svo::RemapMap* rect = nullptr;
    svo::ArgArray<svo::RemapImg> remap_img;
    svo::PinnedPtr<svo::RemapImg> remap_img_host;
    // input format (svo_ctx_set_input_format). fmt: its row of ingest.hip's table. A format that converts launches
    // ingest_kernel over ingest_img (left images of the active sequences, then their right images: pinned block and
    // device mirror, made when the first such format is set); with rectification on too it writes the raw gray
    // planes d_raw_gray (2 x B of raw_plane_bytes, made on first use) that the remap reads.
    int input_format = SVO_INPUT_GRAY_PAIR;
    const svo::IngestFormat* fmt = nullptr;
    svo::ArgArray<svo::IngestImg> ingest_img;
    svo::PinnedPtr<svo::IngestImg> ingest_img_host;
    uint8_t* d_raw_gray = nullptr; size_t raw_plane_bytes = 0;
    // bulk export (grp_export) in host mode: B * cap records of each of the three arrays (kps2d | kps3d | info),
    // made by the first such export
    uint8_t* d_export = nullptr;
    // snapshots (grp_save / grp_load) in host mode: the data parts of one call, made by the first such call and
    // replaced when outgrown
    svo::GrowBlock<uint8_t> d_snap;
    // map export (grp_export_map): the kept counts of one job (per exported keyframe, then per tile) and the pinned
    // mirror that its per-keyframe part comes back into, made by the group's first map export; in host mode the
    // staging block of points, made by the first host-mode one. Replaced when outgrown.
    svo::GrowBlock<int, true> d_map_counts;
    svo::GrowBlock<svo_map_point> d_map_points;
    // views (grp_export_views) in host mode: the images of one job, made by the first such job and replaced when
    // outgrown
    svo::GrowBlock<uint8_t> d_view;
    // scenes (grp_export_scenes): the input block of one job (lines | keyframe sets | image records) and its pinned
    // mirror, made by the group's first scene job; in host mode the images of one job, made by the first host-mode
    // one. Replaced when outgrown.
    svo::GrowBlock<uint8_t, true> d_scene_in;
    svo::GrowBlock<uint8_t> d_scene;
    // scene clouds (grp_export_scenes_clouds): the key planes of one chunk of a job, then the records of its live layer,
    // made by the first such job and replaced when outgrown
    svo::GrowBlock<uint8_t> d_scene_cloud;
    // ar pictures (grp_export_ar): the input block of one job (meshes | draws | image records | work list) and its
    // pinned mirror and the screen records of one job, made by the group's first ar job; in host mode the images of
    // one job, made by the first host-mode one. Replaced when outgrown.
    svo::GrowBlock<uint8_t, true> d_ar_in;
    svo::GrowBlock<uint8_t> d_ar_rec;
    svo::GrowBlock<uint8_t> d_ar;
    // ar occlusion (grp_export_ar_occluded): the organized records of one chunk of a job, made by the first occluded
    // job and replaced when outgrown
    svo::GrowBlock<uint8_t> d_ar_occ;
    // disparity maps (grp_export_disparity) in host mode: the planes of one job, made by the first such job and
    // replaced when outgrown
    svo::GrowBlock<uint8_t> d_dense;
    // point clouds (grp_export_cloud): the staging block of one chunk of a job (planes | tile counts and pose matrices |
    // in host mode records | kept counts) and the pinned mirror of the kept counts, made by the first such job and
    // replaced when outgrown
    svo::GrowBlock<uint8_t> d_cloud;
    svo::PinnedPtr<int> cloud_counts_host; size_t cloud_counts_cap = 0;
    // cross-check (a checked grp_export_disparity or grp_export_cloud): the reverse planes of one chunk of a job, made
    // by the first checked job and replaced when outgrown
    svo::GrowBlock<uint8_t> d_lr;
    // semi-global aggregation (an SGM grp_export_disparity or grp_export_cloud): the sums, volumes and count planes of
    // one chunk of a job, with a check also those of the mirrored pairs and their disparity planes, made by the first
    // SGM job and replaced when outgrown
    svo::GrowBlock<uint8_t> d_sgm;
    // voxel maps (svo_group_voxel.hip): a map per slot that has one (svo_ctx_set_voxel_maps; empty until then) with
    // the host mirror of its header; the records of one chunk of a fuse job and its tables (maps | headers | spans,
    // mirrored); the tile offsets, the sort staging and in host mode the records of an export. Each block is made by
    // the first job that needs it and replaced when outgrown.
    struct VoxelSlot {
        uint8_t* p = nullptr;
        uint8_t* next = nullptr;         // (inside svo_ctx_resize_voxel_maps only: the map it moves into)
        svo_voxel_params params{};
        svo::VoxelHeader head{};         // as of the last job that changed the map
    };
    std::vector<VoxelSlot> voxel_maps;
    svo::GrowBlock<uint8_t> d_voxel_records;
    svo::GrowBlock<uint8_t, true> d_voxel_tables;
    svo::GrowBlock<uint8_t> d_voxel_offsets, d_voxel_sort, d_voxel_out;
    svo::GrowBlock<uint8_t> d_voxel_prune;   // a prune job: the tile offsets and the staging of one slot at a time
    svo::GrowBlock<uint8_t> d_voxel_in;      // a load job in host mode: the entry records of the group's share
    // batched pose-filter updates (grp_pose_updates): the upload block (samples | filter states | start poses |
    // sample offsets) and behind it the download block (filter states | filtered poses) of one job, device and pinned,
    // made by the first such job and replaced when outgrown
    uint8_t* d_pose = nullptr; size_t pose_up_bytes = 0, pose_down_bytes = 0;
    svo::PinnedPtr<uint8_t> pose_host;
    bool timing = false;
    bool failed = false;
    int exact_pinv = 1;          // reference-order Gauss-Newton unless svo_ctx_set_fast_solver(ctx, 1)
    svo::Event ev[10];
    svo::SetLayout set_layout;
    std::vector<uint8_t*> kf_slabs;   // free per-keyframe keypoint storage (allocated in chunks)
    int kf_slab_count = 0;            // ... of so many slabs allocated so far
    size_t device_bytes = 0;          // sum of dev_mem
    std::vector<svo::FinishedRun> finished;   // ended sequences, oldest first (svo_get_finished_run)
    std::vector<uint8_t*> set_slabs;  // free image-set storage (allocated in chunks)
    // KLT template cache (klt.hip): the templates of a keyframe's keypoints stay in HBM while the keyframe is one
    // of the last tmpl_kf of its sequence (0: off)
    int tmpl_kf = 0, tmpl_cap = 0;
    size_t tmpl_block_bytes = 0, tmpl_valid_bytes = 0;
    svo_totals totals;
    std::vector<svo_launch_shape> launch_shapes;   // distinct shapes of launch_sia / launch_reproj and their launches
    bool retire_kf_images = true;    // SVO_KEEP_KEYFRAME_IMAGES=1: keep every keyframe's image set (the reference's behaviour)
    int kf_window = -1;              // svo_ctx_set_keyframe_window: retired keyframes a slot keeps after a step (-1: all of them)
    int image_sets = 0;              // image sets allocated so far
    double host_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // SVO_HOST_TIMING diagnostic: host phases of a step
    long host_steps = 0;
};

namespace svo {

template <typename T>
T& clear(T& x) {
    std::memset(&x, 0, sizeof(x));
    return x;
}

// `count` elements of T (at least one byte's worth), owned by the group; `zero`: cleared first. The clearing is
// complete on return: hipMemset of device memory only enqueues on the null stream, which the group's
// non-blocking stream does not wait for, and the staging buffer of host frames is allocated and filled in
// the same step (a first host frame arrived with patches of it zeroed, about once in a hundred ctxs).
template <typename T>
int dev_alloc(svo_group* c, T** p, size_t count, bool zero = true) {
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    DevPtr<void> q;
    HIP_TRY(dev_malloc(q, bytes));
    if (zero) {
        HIP_TRY(hipMemsetAsync(q.get(), 0, bytes, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    *p = static_cast<T*>(q.get());
    c->dev_mem.push_back(std::move(q));
    c->device_bytes += bytes;
    return SVO_OK;
}

// does the format need ingest_kernel? GRAY_PAIR is the tracker's own input; SBS_GRAY is GRAY_PAIR at base + W and base
inline bool converts(int format) { return format != SVO_INPUT_GRAY_PAIR && format != SVO_INPUT_SBS_GRAY; }

constexpr int MAX_KEYFRAMES = 4096;   // resident ones of one sequence (the keyframe table's default and largest size)

// The tile table of an export, a save or a load (TileTable, svo_host.hpp) goes up through the group's argument
// blocks, pinned and device: between two steps the stream is idle and nothing in them is live (every step fills and
// uploads what its launches read), so none of them allocates a table of its own. One launch unless the table
// outgrows the blocks, or the diagnostic `env` (a *_TABLE_TILES) makes it smaller.
template <typename Tile, typename Launch>
TileTable<Tile, Launch> group_tile_table(svo_group* c, const char* env, Launch run) {
    return {reinterpret_cast<Tile*>(c->args.host.get()), reinterpret_cast<Tile*>(c->args.dev),
            table_tiles(env, c->args.bytes / sizeof(Tile)), c->stream.get(), run};
}

// what one unit of the group implements for the others (svo_group.hip all of it but the last)
size_t align_up(size_t v, size_t a);
void dev_release(svo_group* c, void* p, size_t bytes);                 // gives an allocation of dev_alloc back
// Host-mode delivery of a job whose named slot seg[i] owns image_bytes at seg[i] * image_bytes of the caller's `to` and
// whose i-th slot was staged at i * image_bytes of `from`, `used` bytes of it: every run of delivered slots (shown[i])
// that are consecutive in both goes out with one copy, so that the bytes between two slots stay untouched. Enqueued
// on `st`; the caller synchronises.
int copy_out_slots(hipStream_t st, uint8_t* to, const uint8_t* from, const int* seg, const char* shown, int n, int64_t image_bytes,
                   int64_t used);
// a failed group rejects the job of entry point `who` (SVO_OK: it has not failed)
int reject_if_failed(const svo_group* c, const char* who);
// how a job that reads the slots' poses begins: reject_if_failed, the group's device, the deferred pose-filter updates
int job_begin(svo_group* c, const char* who);
int acquire_set(svo_group* c, Seq& q, ImageSet** out);
// The SGM planes of `images` (svo_group_dense.hip): value [, cost] at each image's out, computed through the group's
// d_sgm block and argument blocks, enqueued on the group's stream. sp: the checked params with the value and cost of
// the planes. check: the lattice check of "sgm cross-check" behind them (sp.value is SVO_DENSE_DISPARITY then), which
// writes the lr plane at out + lr_plane floats (< 0: none) and masks and converts the value plane; null: none.
// args_reused: the caller fills the argument blocks again, so the uploads are over on return.
int grp_sgm_planes(svo_group* c, const std::vector<DenseImage>& images, const DenseParams& params, SgmParams sp, int cols, int rows,
                   const LrParams* check, int64_t lr_plane, bool args_reused);
void release_set(Seq& q, ImageSet*& s);
int take_kf_slab(svo_group* c, KpsDev* out);
void fill_kf_record(const svo_group* c, const Seq& q, int id, const KfHost& k, KfDev& d);
void flush_one(Seq& q);
void flush_pending(svo_group* c);
void end_sequence(svo_group* c, int s);
void trim_keyframes(svo_group* c, Seq& q, int below);                  // drops the slot's keyframes below min(below, kfs_retired)
int check_settings(const svo_camera_settings* cam, int width, int height, int n_sequences);
int keypoint_capacity(const svo_camera_settings& cam, int width, int height);
int usable_lk_levels(const svo_camera_settings& cam, int width, int height);

template <typename T, bool Mirror>
int GrowBlock<T, Mirror>::reserve(svo_group* c, size_t want) {
    if (want <= bytes) return SVO_OK;
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    if (p) dev_release(c, p, bytes);
    p = nullptr; bytes = 0;
    if (Mirror) {
        host.reset();
        HIP_TRY(pinned_malloc(host, want));
    }
    uint8_t* q = nullptr;
    if (const int rc = dev_alloc(c, &q, want, false)) return rc;
    p = reinterpret_cast<T*>(q);
    bytes = want;
    return SVO_OK;
}
}  // namespace svo
