// svo_group.hip — one group of the tracker behind the C ABI: StereoSlam::new_image
// (src/lib/stereo_slam.cpp:123-271) for B sequences together, one kernel launch per stage, on the
// group's own stream: creation, the step as its phases, the bulk export, snapshots (save / load of a slot's sequence
// state), and the per-sequence getters of the C ABI.
// svo_ctx.hip spreads a ctx's sequences over groups.
//
// Host side = bookkeeping only: image-set pool, argument blocks, the 12-state
// pose Kalman filter (stereo_slam.cpp:296-359) and the keyframe decision. All
// image and keypoint work runs in the kernels of pyramid/sia/klt/reproj/depth/
// keyframe.hip; a tracked frame is nine launches on one stream, one blocking
// read-back of the result block, and (only when a keyframe is due) a second
// batch of five launches.
//
// HBM layout per sequence:
//   image sets  : left halfSample pyramid | right level 0 | Gaussian levels 1,2
//                 (rows padded to 64 B). The current, the previous and every
//                 keyframe's set stay resident (288 GB: ~1 MB per 752x480 set).
//   keypoints   : two SoA sets (KpsDev) ping-ponged by the order-preserving
//                 compactions; per-point scratch (tracked, err, disparity).
//   keyframes   : table of KfDev records + per-keyframe SoA copies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "svo_group.hpp"
#include "svo_host.hpp"
#include "svo_tracker.hpp"

using namespace svo;

namespace {

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
    KfDev* d_kfs = nullptr;
    std::vector<KfHost> kfs;
    int kfs_retired = 0;             // keyframes [0, kfs_retired) have given their image sets back
    DetCell* det = nullptr; int* n_det = nullptr;
    DetCell* sel = nullptr; int* sel_level = nullptr; int* sel_cell = nullptr; int* occupied = nullptr;
    uint32_t* color_lcg = nullptr;
    std::vector<std::unique_ptr<ImageSet>> sets;   // every image set of the sequence; the rest point into these
    std::vector<ImageSet*> free_sets;
    ImageSet* cur_set = nullptr;
    ImageSet* prev_set = nullptr;
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
// tracked-frame arrays first, so that a tracked frame uploads them as one prefix copy (frame_bytes)
struct ArgBlocks {
    ArgArray<PyrArgs> pyr;
    ArgArray<CompactArgs> compact;
    ArgArray<SiaArgs> sia;
    ArgArray<KltArgs> klt;
    ArgArray<ReprojArgs> reproj;
    ArgArray<SsdArgs> ssd;
    ArgArray<FilterArgs> filter;
    ArgArray<float[8]> guess;        // per sequence: the predicted pose
    ArgArray<DetectArgs> detect;
    ArgArray<MergeArgs> merge;
    ArgArray<KfInitArgs> kf_init;
    ArgArray<int> enable;            // (reserved)
    ArgArray<KfDev> kf_record;       // per sequence: staging of its newest keyframe's record
    template <typename F> void frame_arrays(F f) { f(pyr); f(compact); f(sia); f(klt); f(reproj); f(ssd); f(filter); f(guess); }
    template <typename F> void keyframe_arrays(F f) { f(detect); f(merge); f(kf_init); f(enable); f(kf_record); }
    PinnedPtr<uint8_t> host;
    uint8_t* dev = nullptr;
    size_t frame_bytes = 0, bytes = 0;
};

}  // namespace

struct svo_group {
    Stream stream;                   // (declared first: destroyed after everything that uses it)
    int device, B, width, height, cap, rec_cap, max_kf, n_lk, det_levels, max_cells, merge_cells;
    svo_camera_settings cam;
    std::vector<DevPtr<void>> dev_mem;   // every device allocation of the group (dev_alloc)
    std::vector<Seq> seqs;
    ArgBlocks args;
    // d_res | d_n_all | d_inside are one device block mirrored by one pinned block: the end-of-frame
    // read-back is a single copy, the keyframe decision reads back only the B inside-counters
    PinnedPtr<uint8_t> readback_host;
    FrameResult* d_res = nullptr; FrameResult* h_res = nullptr;
    int* h_n = nullptr;          // pinned [B*2]
    int* d_n_all = nullptr;      // [B*2]
    int* d_inside = nullptr; int* h_inside = nullptr;
    size_t readback_bytes = 0;
    // host-resident input frames land here first (2 x B frames; runs of contiguous frames as one
    // copy) and are then ingested like device-resident ones
    uint8_t* d_stage_in = nullptr; size_t stage_frame_bytes = 0;
    // rectification (svo_ctx_set_rectification): the ctx's two maps, or null; the image table of its launch
    // (left images of the active sequences, then their right images) in a pinned block and its device mirror
    const RemapMap* rect = nullptr;
    ArgArray<RemapImg> remap_img;
    PinnedPtr<RemapImg> remap_img_host;
    // input format (svo_ctx_set_input_format). fmt: its row of ingest.hip's table. A format that converts launches
    // ingest_kernel over ingest_img (left images of the active sequences, then their right images: pinned block and
    // device mirror, made when the first such format is set); with rectification on too it writes the raw gray
    // planes d_raw_gray (2 x B of raw_plane_bytes, made on first use) that the remap reads.
    int input_format = SVO_INPUT_GRAY_PAIR;
    const IngestFormat* fmt = nullptr;
    ArgArray<IngestImg> ingest_img;
    PinnedPtr<IngestImg> ingest_img_host;
    uint8_t* d_raw_gray = nullptr; size_t raw_plane_bytes = 0;
    // bulk export (grp_export) in host mode: B * cap records of each of the three arrays (kps2d | kps3d | info),
    // made by the first such export
    uint8_t* d_export = nullptr;
    // snapshots (grp_save / grp_load) in host mode: the data parts of one call, made by the first such call and
    // replaced when outgrown
    uint8_t* d_snap = nullptr; size_t snap_bytes = 0;
    bool timing = false;
    bool failed = false;
    int exact_pinv = 1;          // reference-order Gauss-Newton unless svo_ctx_set_fast_solver(ctx, 1)
    Event ev[10];
    SetLayout set_layout;
    std::vector<uint8_t*> kf_slabs;   // free per-keyframe keypoint storage (allocated in chunks)
    int kf_slab_count = 0;            // ... of so many slabs allocated so far
    size_t device_bytes = 0;          // sum of dev_mem
    std::vector<FinishedRun> finished;   // ended sequences, oldest first (svo_get_finished_run)
    std::vector<uint8_t*> set_slabs;  // free image-set storage (allocated in chunks)
    // KLT template cache (klt.hip): the templates of a keyframe's keypoints stay in HBM while the keyframe is one
    // of the last tmpl_kf of its sequence (0: off)
    int tmpl_kf = 0, tmpl_cap = 0;
    size_t tmpl_block_bytes = 0, tmpl_valid_bytes = 0;
    svo_totals totals;
    std::vector<svo_launch_shape> launch_shapes;   // distinct shapes of launch_sia / launch_reproj and their launches
    bool retire_kf_images = true;    // SVO_KEEP_KEYFRAME_IMAGES=1: keep every keyframe's image set (the reference's behaviour)
    int image_sets = 0;              // image sets allocated so far
    double host_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // SVO_HOST_TIMING diagnostic: host phases of a step
    long host_steps = 0;
};

void GroupDelete::operator()(svo_group* c) const {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream.get());
    if (std::getenv("SVO_HOST_TIMING") && c->host_steps > 0) {
        static const char* names[7] = {"args", "launch", "pose_filter", "wait_frame", "kf_enqueue", "wait_kf", "bookkeeping"};
        std::fprintf(stderr, "[svo host ms/step over %ld steps]", c->host_steps);
        for (int i = 0; i < 7; i++) std::fprintf(stderr, " %s=%.3f", names[i], c->host_ms[i] / c->host_steps);
        std::fprintf(stderr, "\n");
    }
    delete c;
}

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

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

// gives an allocation of dev_alloc back
void dev_release(svo_group* c, void* p, size_t bytes) {
    for (auto it = c->dev_mem.begin(); it != c->dev_mem.end(); ++it)
        if (it->get() == p) {
            c->dev_mem.erase(it);
            c->device_bytes -= bytes;
            return;
        }
}

// ------------------------------------------------------------------------------------ storage

// Image-set storage comes from slabs allocated in chunks: one hipMalloc (a device-wide
// synchronising call) per chunk of sets, not per set — every keyframe keeps its set for good, so a
// long run asks for one per keyframe.
int grow_set_slabs(svo_group* c, int count) {
    uint8_t* base = nullptr;
    const int rc = dev_alloc(c, &base, c->set_layout.bytes * (size_t)count, false);
    if (rc) return rc;
    for (int i = count - 1; i >= 0; i--) c->set_slabs.push_back(base + c->set_layout.bytes * (size_t)i);
    return SVO_OK;
}

SetLayout image_set_layout(const svo_group* c) {
    SetLayout t{};
    size_t off = 0;
    auto place = [&off](ImgView& v, size_t& at, int w, int h) {
        v = ImgView{nullptr, w, h, (int)align_up((size_t)std::max(w, 1), 64)};
        at = off;
        off += align_up((size_t)v.stride * std::max(h, 1), 256);
    };
    int w = c->width, h = c->height;
    for (int l = 0; l < c->cam.max_pyramid_levels; l++, w /= 2, h /= 2) place(t.views.left[l], t.left[l], w, h);
    place(t.views.right, t.right, c->width, c->height);
    w = c->width; h = c->height;
    for (int l = 1; l < c->n_lk; l++) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        place(t.views.lk[l], t.lk[l], w, h);
    }
    t.bytes = off;
    return t;
}

// a new image set of the sequence, on the free list
int new_image_set(svo_group* c, Seq& q) {
    if (c->set_slabs.empty()) {
        const int rc = grow_set_slabs(c, std::max(c->B, 16));
        if (rc) return rc;
    }
    const SetLayout& t = c->set_layout;
    auto s = std::make_unique<ImageSet>(t.views);
    s->base = c->set_slabs.back();
    c->set_slabs.pop_back();
    for (int l = 0; l < c->cam.max_pyramid_levels; l++) s->left[l].data = s->base + t.left[l];
    s->right.data = s->base + t.right;
    s->lk[0] = s->left[0];
    s->own_left0 = s->left[0];
    s->own_right = s->right;
    for (int l = 1; l < c->n_lk; l++) s->lk[l].data = s->base + t.lk[l];
    q.free_sets.push_back(s.get());
    q.sets.push_back(std::move(s));
    c->image_sets++;
    return SVO_OK;
}

int acquire_set(svo_group* c, Seq& q, ImageSet** out) {
    if (q.free_sets.empty()) {
        const int rc = new_image_set(c, q);
        if (rc) return rc;
    }
    *out = q.free_sets.back();
    q.free_sets.pop_back();
    (*out)->refs = 1;
    return SVO_OK;
}

void release_set(Seq& q, ImageSet*& s) {
    if (s && --s->refs <= 0) q.free_sets.push_back(s);
    s = nullptr;
}

// the separate arrays of a frame keypoint set, in the order of KpsDev
int alloc_kps(svo_group* c, KpsDev& k, int* n_ptr) {
    int rc = SVO_OK;
    auto alloc = [&](auto** p) { if (!rc) rc = dev_alloc(c, p, (size_t)c->cap); };
    alloc(&k.kps2d); alloc(&k.kps3d); alloc(&k.flags); alloc(&k.kf_id); alloc(&k.kp_index); alloc(&k.outl);
    alloc(&k.inl); alloc(&k.kfx); alloc(&k.kfP); alloc(&k.score); alloc(&k.level_type); alloc(&k.color);
    k.n = n_ptr;
    return rc;
}

// per-keyframe keypoint storage: 15 dwords per keypoint. Slabs come from chunks of `count`
// (one hipMalloc — a device-wide synchronising call — per chunk, not per keyframe).
size_t kf_slab_bytes(const svo_group* c) { return align_up((size_t)c->cap * 15 * 4, 256); }

int grow_kf_slabs(svo_group* c, int count) {
    const size_t sb = kf_slab_bytes(c);
    uint8_t* base = nullptr;
    const int rc = dev_alloc(c, &base, sb * count, false);
    if (rc) return rc;
    for (int i = count - 1; i >= 0; i--) c->kf_slabs.push_back(base + sb * i);
    c->kf_slab_count += count;
    return SVO_OK;
}

// the keypoint arrays of a keyframe in one slab of kf_slab_bytes (kps3d is the slab's first array: its address
// is the slab's, which end_sequence gives back)
KpsDev carve_kps(uint8_t* base, size_t cap) {
    KpsDev k;
    std::memset(&k, 0, sizeof(k));
    k.kps3d = reinterpret_cast<svo_kp3d*>(base);
    k.kps2d = reinterpret_cast<svo_kp2d*>(base + cap * sizeof(svo_kp3d));
    k.flags = reinterpret_cast<uint32_t*>(base + cap * (sizeof(svo_kp3d) + sizeof(svo_kp2d)));
    k.outl = reinterpret_cast<int*>(k.flags + cap);
    k.inl = k.outl + cap;
    k.kf_id = k.inl + cap;
    k.kp_index = k.kf_id + cap;
    k.score = reinterpret_cast<float*>(k.kp_index + cap);
    k.level_type = reinterpret_cast<int*>(k.score + cap);
    k.color = reinterpret_cast<uint32_t*>(k.level_type + cap);
    k.kfx = reinterpret_cast<float*>(k.color + cap);
    k.kfP = k.kfx + cap;
    return k;
}

// the device record of keyframe `id` of the sequence: its image set, keypoint arrays and template-cache block
void fill_kf_record(const svo_group* c, const Seq& q, int id, const KfHost& k, KfDev& d) {
    clear(d);
    if (k.set)                               // (a retired keyframe of a loaded snapshot has no images: nothing tracks from it)
        for (int l = 0; l < c->n_lk; l++) d.lk[l] = k.set->lk[l];
    d.n_lk = c->n_lk;
    d.kps2d = k.kps.kps2d; d.kps3d = k.kps.kps3d; d.flags = k.kps.flags;
    d.outlier_count = k.kps.outl; d.inlier_count = k.kps.inl;
    d.kf_id = k.kps.kf_id; d.kp_index = k.kps.kp_index; d.score = k.kps.score; d.level_type = k.kps.level_type;
    d.color = k.kps.color; d.kfx = k.kps.kfx; d.kfP = k.kps.kfP;
    if (c->tmpl_kf > 0) {
        // the keyframe takes the oldest block of the sequence's ring; kf_init_kernel clears the flags and
        // takes the cache away from the keyframe that held the block (id - tmpl_kf: its points are tracked
        // from the images again)
        const int r = id % c->tmpl_kf;
        d.tmpl = q.tmpl_base + (size_t)r * c->tmpl_block_bytes;
        d.tmpl_valid = q.tmpl_valid + (size_t)r * c->tmpl_valid_bytes;
        d.tmpl_cap = c->tmpl_cap;
        d.tmpl_win = c->cam.window_size_opt_flow;
    }
}

// keyframe `id` of sequence s on its current image set; its record goes to the pinned staging slot of s
// (it reaches the device inside the KfInitArgs block: no copy per keyframe)
int new_keyframe_storage(svo_group* c, Seq& q, int s, int id) {
    if (id >= c->max_kf) return svo_set_error(SVO_ERR_CAPACITY, "more than %d keyframes", c->max_kf);
    if (c->kf_slabs.empty()) {
        const int rc = grow_kf_slabs(c, std::max(c->B, 32));
        if (rc) return rc;
    }
    KfHost k{};
    k.kps = carve_kps(c->kf_slabs.back(), c->cap);
    c->kf_slabs.pop_back();
    k.set = q.cur_set;
    q.cur_set->refs++;
    q.kfs.push_back(k);
    fill_kf_record(c, q, id, k, c->args.kf_record.h[s]);
    return SVO_OK;
}

// ------------------------------------------------------------------------------------ creation

int check_settings(const svo_camera_settings* cam, int width, int height, int n_sequences) {
    if (!cam || width < 16 || height < 16 || n_sequences < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_create: bad arguments");
    if (cam->max_pyramid_levels < 1 || cam->max_pyramid_levels > 7 ||
        cam->min_pyramid_level_pose_estimation < 0 ||
        cam->min_pyramid_level_pose_estimation >= cam->max_pyramid_levels)
        return svo_set_error(SVO_ERR_INVALID, "max_pyramid_levels must be 1..7 and > min level");
    if (cam->window_size_opt_flow < 3 || cam->window_size_opt_flow > 35 ||
        cam->window_size_depth_calculator < 1 || cam->window_size_depth_calculator > 35 ||
        cam->search_x < 0 || cam->search_x > 64 || cam->search_y < 0 || cam->search_y > 8)
        return svo_set_error(SVO_ERR_INVALID, "windows <= 35, search_x <= 64, search_y <= 8 supported");
    if (cam->window_size_pose_estimator != 4)   // PATCH_SIZE, src/lib/pose_estimator.cpp:68
        return svo_set_error(SVO_ERR_INVALID, "window_size_pose_estimator must be 4");
    if (cam->grid_width < 4 || cam->grid_height < 4 || cam->grid_width > 96 || cam->grid_height > 64)
        return svo_set_error(SVO_ERR_INVALID, "grid cell must be within 4..96 x 4..64");
    return SVO_OK;
}

// keypoints a sequence can hold: the frame's plus a keyframe's new ones, and some room
int keypoint_capacity(const svo_camera_settings& cam, int width, int height) {
    const int cells = (width / cam.grid_width) * (height / cam.grid_height);
    return (int)align_up((size_t)(2 * cells + 128), 64);
}

// usable LK levels (cv::buildOpticalFlowPyramid stops at levels not larger than the window)
int usable_lk_levels(const svo_camera_settings& cam, int width, int height) {
    for (int l = 0, w = width, h = height; l < SVO_LK_LEVELS; l++) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= cam.window_size_opt_flow || h <= cam.window_size_opt_flow) return l + 1;
    }
    return SVO_LK_LEVELS;
}

constexpr int MAX_KEYFRAMES = 4096;   // of one sequence (the keyframe table)

// capacities and level counts that follow from the settings
void size_group(svo_group* c) {
    const svo_camera_settings& cam = c->cam;
    const int width = c->width, height = c->height;
    c->cap = keypoint_capacity(cam, width, height);
    c->rec_cap = (int)align_up((size_t)c->cap, 512);   // whole passes of the widest alignment workgroup
    c->max_kf = MAX_KEYFRAMES;
    if (const char* e = std::getenv("SVO_KEEP_KEYFRAME_IMAGES")) c->retire_kf_images = std::atoi(e) == 0;
    c->n_lk = usable_lk_levels(cam, width, height);
    c->det_levels = cam.max_pyramid_levels / 2;
    c->max_cells = 1;
    for (int l = 0; l < c->det_levels; l++) {
        const int gw = cam.grid_width >> l, gh = cam.grid_height >> l;
        if (gw <= 0 || gh <= 0) { c->det_levels = l; break; }
        const int nc = ((width >> l) / gw) * std::max((height >> l) / gh, 1);
        c->max_cells = std::max(c->max_cells, nc);
    }
    c->merge_cells = ((width + cam.grid_height - 1) / cam.grid_height) *
                     ((height + cam.grid_width - 1) / cam.grid_width);
    c->set_layout = image_set_layout(c);
}

// the argument blocks (one pinned, one device) and the result block with its pinned mirror
int alloc_blocks(svo_group* c) {
    ArgBlocks& a = c->args;
    const size_t B = c->B;
    size_t off = 0;
    auto size = [&](auto& arr) { off += align_up(sizeof(typename std::decay_t<decltype(arr)>::type) * B, 256); };
    a.frame_arrays(size);
    a.frame_bytes = off;                  // everything a tracked frame uploads; the rest is keyframe-only
    a.keyframe_arrays(size);
    a.bytes = off;
    HIP_TRY(pinned_malloc(a.host, a.bytes));
    std::memset(a.host.get(), 0, a.bytes);
    int rc;
    if ((rc = dev_alloc(c, &a.dev, a.bytes))) return rc;
    off = 0;
    auto place = [&](auto& arr) {
        using T = typename std::decay_t<decltype(arr)>::type;
        arr.h = reinterpret_cast<T*>(a.host.get() + off);
        arr.d = reinterpret_cast<T*>(a.dev + off);
        off += align_up(sizeof(T) * B, 256);
    };
    a.frame_arrays(place);
    a.keyframe_arrays(place);

    const size_t res_bytes = sizeof(FrameResult) * B, n_bytes = sizeof(int) * 2 * B, in_bytes = sizeof(int) * B;
    c->readback_bytes = res_bytes + n_bytes;
    uint8_t* db = nullptr;
    HIP_TRY(pinned_malloc(c->readback_host, res_bytes + n_bytes + in_bytes));
    uint8_t* hb = c->readback_host.get();
    std::memset(hb, 0, res_bytes + n_bytes + in_bytes);
    if ((rc = dev_alloc(c, &db, res_bytes + n_bytes + in_bytes))) return rc;
    c->h_res = reinterpret_cast<FrameResult*>(hb); c->d_res = reinterpret_cast<FrameResult*>(db);
    c->h_n = reinterpret_cast<int*>(hb + res_bytes); c->d_n_all = reinterpret_cast<int*>(db + res_bytes);
    c->h_inside = reinterpret_cast<int*>(hb + res_bytes + n_bytes);
    c->d_inside = reinterpret_cast<int*>(db + res_bytes + n_bytes);
    return SVO_OK;
}

int alloc_sequence(svo_group* c, Seq& q, int s) {
    q.d_n = c->d_n_all + 2 * s;
    int rc = alloc_kps(c, q.kps[0], q.d_n);
    if (!rc) rc = alloc_kps(c, q.kps[1], q.d_n + 1);
    auto alloc = [&](auto** p, size_t count) { if (!rc) rc = dev_alloc(c, p, count); };
    const size_t cap = c->cap, cells = c->max_cells;
    alloc(&q.tracked, cap); alloc(&q.klt_err, cap); alloc(&q.klt_status, cap); alloc(&q.disparity, cap);
    alloc(&q.sia_rec, sia_rec_ws_floats(c->cam, c->rec_cap)); alloc(&q.sia_kpws, (size_t)9 * c->rec_cap);
    alloc(&q.sia_mats, 1); alloc(&q.d_kfs, c->max_kf);
    alloc(&q.det, SVO_MAX_PYRAMID_LEVELS * cells); alloc(&q.n_det, SVO_MAX_PYRAMID_LEVELS);
    alloc(&q.sel, cells); alloc(&q.sel_level, cells); alloc(&q.sel_cell, cells); alloc(&q.occupied, c->merge_cells);
    alloc(&q.color_lcg, 1);
    if (rc) return rc;
    q.kf.init();
    std::memset(&q.stats, 0, sizeof(q.stats));
    for (int i = 0; i < 4; i++)         // pre-allocate a few image sets
        if ((rc = new_image_set(c, q))) return rc;
    return SVO_OK;
}

// KLT template cache: SVO_KLT_CACHE_KF keyframes per sequence (default 8 while a keyframe's block stays below
// 8 MB, else 4; 0 = off), as many as fit a third of the free device memory. On closed camera loops every
// keyframe keeps keypoints in view, and those of keyframes that have left the ring build their templates
// on every frame: 8 instead of 4 blocks per sequence are +0.8 % frames/s at C2 (profiles/r03_ab_steps.txt).
// A keypoint index beyond tmpl_cap (more points than grid cells + 64 in the frame that made the keyframe)
// is tracked without the cache.
int alloc_template_cache(svo_group* c) {
    const int B = c->B;
    const int cells = (c->width / c->cam.grid_width) * (c->height / c->cam.grid_height);
    c->tmpl_cap = std::min(c->cap, cells + 64);
    c->tmpl_block_bytes = align_up((size_t)c->tmpl_cap * SVO_LK_LEVELS * klt_template_bytes(c->cam.window_size_opt_flow), 256);
    int K = c->tmpl_block_bytes <= ((size_t)8 << 20) ? 8 : 4;
    if (const char* e = std::getenv("SVO_KLT_CACHE_KF")) K = std::max(0, std::min(std::atoi(e), 64));
    c->tmpl_valid_bytes = align_up((size_t)c->tmpl_cap * SVO_LK_LEVELS, 256);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    while (K > 0 && (size_t)B * K * c->tmpl_block_bytes > free_b / 3) K--;
    c->tmpl_kf = K;
    if (K == 0) return SVO_OK;
    uint8_t* base = nullptr; uint8_t* vbase = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &base, (size_t)B * K * c->tmpl_block_bytes, false))) return rc;
    if ((rc = dev_alloc(c, &vbase, (size_t)B * K * c->tmpl_valid_bytes))) return rc;
    for (int s = 0; s < B; s++) {
        c->seqs[s].tmpl_base = base + (size_t)s * K * c->tmpl_block_bytes;
        c->seqs[s].tmpl_valid = vbase + (size_t)s * K * c->tmpl_valid_bytes;
    }
    return SVO_OK;
}

}  // namespace

int grp_create(const svo_camera_settings* cam, int width, int height, int n_sequences, int device, Group* out) {
    int rc = check_settings(cam, width, height, n_sequences);
    if (rc) return rc;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return svo_set_error(SVO_ERR_NO_DEVICE, "no HIP device visible: libsvo_hip has no CPU fallback");
    if (device < 0 || device >= count) return svo_set_error(SVO_ERR_INVALID, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));
    Group g(new (std::nothrow) svo_group());
    svo_group* c = g.get();
    if (!c) return svo_set_error(SVO_ERR_INVALID, "out of host memory");
    c->fmt = ingest_format(SVO_INPUT_GRAY_PAIR);
    c->device = device; c->B = n_sequences; c->width = width; c->height = height; c->cam = *cam;
    std::memset(&c->totals, 0, sizeof(c->totals));
    HIP_TRY(make_stream(c->stream));
    size_group(c);
    if ((rc = alloc_blocks(c))) return rc;
    for (Event& e : c->ev) HIP_TRY(make_event(e));
    c->seqs.resize(n_sequences);
    if ((rc = grow_set_slabs(c, 4 * n_sequences))) return rc;   // the first four image sets of every sequence: one allocation
    for (int s = 0; s < n_sequences; s++)
        if ((rc = alloc_sequence(c, c->seqs[s], s))) return rc;
    if ((rc = grow_kf_slabs(c, std::max(2 * n_sequences, 32)))) return rc;   // the first keyframes never allocate
    if ((rc = alloc_template_cache(c))) return rc;
    HIP_TRY(pinned_malloc(c->remap_img_host, sizeof(RemapImg) * 2 * (size_t)n_sequences));
    c->remap_img.h = c->remap_img_host.get();
    if ((rc = dev_alloc(c, &c->remap_img.d, 2 * (size_t)n_sequences))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = std::move(g);
    return SVO_OK;
}

void grp_set_exact_pinv(svo_group* c, int on) { c->exact_pinv = on != 0; }
void grp_set_rectification(svo_group* c, const RemapMap* maps) { c->rect = maps; }
void grp_enable_timing(svo_group* c, int on) { c->timing = on != 0; }

namespace {
// does the format need ingest_kernel? GRAY_PAIR is the tracker's own input; SBS_GRAY is GRAY_PAIR at base + W and base
bool converts(int format) { return format != SVO_INPUT_GRAY_PAIR && format != SVO_INPUT_SBS_GRAY; }
}  // namespace

int grp_set_input_format(svo_group* c, int format) {
    if (converts(format) && !c->ingest_img.d) {
        HIP_TRY(hipSetDevice(c->device));
        PinnedPtr<IngestImg> host;
        HIP_TRY(pinned_malloc(host, sizeof(IngestImg) * 2 * (size_t)c->B));
        IngestImg* dev = nullptr;
        if (const int rc = dev_alloc(c, &dev, 2 * (size_t)c->B)) return rc;
        c->ingest_img_host = std::move(host);
        c->ingest_img.h = c->ingest_img_host.get();
        c->ingest_img.d = dev;
    }
    c->input_format = format;
    c->fmt = ingest_format(format);
    return SVO_OK;
}

svo_totals grp_totals(const svo_group* c) {
    svo_totals t = c->totals;
    t.image_sets = c->image_sets;
    return t;
}

const std::vector<svo_launch_shape>& grp_launch_shapes(const svo_group* c) { return c->launch_shapes; }

namespace {

// motion + 12-state filter + trajectory of the last frame (stereo_slam.cpp:250-270).
// Deferred: the next frame's pose guess only needs the state BEFORE this update
// (kf.statePre after its predict() equals the current statePost, dt = 0), so the
// host runs it while the GPU already works on the next frame.
void flush_one(Seq& q) {
    if (!q.pending) return;
    q.pending = false;
    float prev_pose[6];
    std::memcpy(prev_pose, q.pose, sizeof(prev_pose));
    std::memcpy(q.pose, q.pending_pose, sizeof(q.pose));
    const double dt = q.pending_ts - q.ts;
    const double inv = 1. / dt;
    float motion[6];
    for (int i = 0; i < 6; i++) motion[i] = (float)((q.pose[i] - prev_pose[i]) * inv);
    const float pv[6] = {0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f};
    const float mv[6] = {1, 1, 1, 1, 1, 1};
    float filtered[6];
    q.kf.update(q.pose, motion, pv, mv, 0.0, filtered);
    std::memcpy(q.pose, filtered, sizeof(q.pose));
    q.ts = q.pending_ts;
    svo_pose p;
    std::memcpy(&p, q.pose, sizeof(p));
    q.trajectory.push_back(p);
}

void flush_pending(svo_group* c) {
    for (Seq& q : c->seqs) flush_one(q);
}

// ------------------------------------------------------------------------------------ the step

// one call of the step: its input and what its phases hand on
struct Step {
    const uint8_t* const* left;
    const uint8_t* const* right;
    int stride, mem;
    const float* time_stamps;
    std::vector<int> act;        // the sequences that take part, in slot order: they get pyramids
    std::vector<int> trk;        // of these, the ones with a previous frame: they run the tracked frame's kernels
    std::vector<int> start;      // [B] 1: this is frame 0 of the sequence (the slot was empty): no tracking, a keyframe
    std::vector<int> need;       // [B] 1: the sequence makes a keyframe in this step
    int pyr_stream = -1;         // row block of the row-streaming pyramid kernel, 0: some frame does not fit it
    float stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t0, lap_start;
};

hipError_t mark(svo_group* c, int i) {
    return c->timing ? hipEventRecord(c->ev[i].get(), c->stream.get()) : hipSuccess;
}

void lap(svo_group* c, Step& s, int phase) {
    const auto now = std::chrono::steady_clock::now();
    c->host_ms[phase] += std::chrono::duration<double, std::milli>(now - s.lap_start).count();
    s.lap_start = now;
}

// Sequences whose image pointers are NULL sit this step out (their state is untouched; an empty slot stays
// empty): a ctx can hold sequences of different lengths. An empty slot that gets a frame starts a sequence
// with it. The sequences of a launch are packed into the first slots of its argument arrays, so every
// launch covers exactly the sequences it is for.
int select_sequences(svo_group* c, Step& s) {
    s.act.reserve(c->B);
    s.trk.reserve(c->B);
    s.start.assign(c->B, 0);
    s.need.assign(c->B, 0);
    const bool one_buffer = c->fmt->buffers == 1;
    for (int q = 0; q < c->B; q++)
        if (s.left[q] && (one_buffer || s.right[q])) {
            s.act.push_back(q);
            if (c->seqs[q].frame_id < 0) s.start[q] = 1;
            else s.trk.push_back(q);
        } else if (!one_buffer && (s.left[q] != nullptr) != (s.right[q] != nullptr)) {
            return svo_set_error(SVO_ERR_INVALID, "svo_new_images: sequence %d has only one image", q);
        }
    return SVO_OK;
}

// host-resident frames into the staging buffer: slots 0..B-1 left frames, B..2B-1 right frames (a one-buffer
// input format: slots 0..B-1, one side only)
int stage_host_frames(svo_group* c, const Step& s) {
    const int B = c->B;
    const size_t row_bytes = (size_t)ingest_row_pixels(*c->fmt, c->width) * c->fmt->channels;
    const size_t used = (size_t)(c->height - 1) * s.stride + row_bytes;     // bytes of one frame that are read
    const size_t fb = align_up((size_t)c->height * s.stride, 256);
    if (fb > c->stage_frame_bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        const int rc = dev_alloc(c, &c->d_stage_in, fb * 2 * B);    // (an outgrown buffer is freed with the group)
        if (rc) return rc;
        c->stage_frame_bytes = fb;
    }
    // host frames that follow each other at exactly one frame's distance (one [B][H][stride] block per
    // side) go as ONE 2D copy: a "row" is a whole frame
    const size_t spacing = (size_t)c->height * s.stride;
    for (int side = 0; side < c->fmt->buffers; side++) {
        const uint8_t* const* src = side ? s.right : s.left;
        int s0 = 0;
        while (s0 < B) {
            if (!src[s0]) { s0++; continue; }
            int s1 = s0 + 1;
            while (s1 < B && src[s1] && src[s1] == src[s1 - 1] + spacing) s1++;
            uint8_t* dst = c->d_stage_in + (size_t)(side * B + s0) * c->stage_frame_bytes;
            if (s1 - s0 > 1) {
                HIP_TRY(hipMemcpy2DAsync(dst, c->stage_frame_bytes, src[s0], spacing, spacing, s1 - s0,
                                         hipMemcpyHostToDevice, c->stream.get()));
            } else {
                HIP_TRY(hipMemcpyAsync(dst, src[s0], used, hipMemcpyHostToDevice, c->stream.get()));
            }
            s0 = s1;
        }
    }
    return SVO_OK;
}

// every active sequence takes a fresh image set; its pyramid arguments
int pack_pyramids(svo_group* c, Step& s) {
    if (converts(c->input_format) && c->rect && !c->d_raw_gray) {
        c->raw_plane_bytes = align_up(align_up((size_t)c->width, 64) * c->height, 256);
        const int rc = dev_alloc(c, &c->d_raw_gray, c->raw_plane_bytes * 2 * c->B, false);
        if (rc) return rc;
    }
    for (int j = 0; j < (int)s.act.size(); j++) {
        const int seq = s.act[j];
        Seq& q = c->seqs[seq];
        release_set(q, q.prev_set);
        q.prev_set = q.cur_set;
        const int rc = acquire_set(c, q, &q.cur_set);
        if (rc) return rc;
        ImageSet* is = q.cur_set;
        PyrArgs& hs = clear(c->args.pyr.h[j]);
        hs.n_levels = c->cam.max_pyramid_levels;
        // the sequence's buffers on the device (in place, or in the staging buffer), and its two gray images in them
        const bool host = s.mem == SVO_MEM_HOST;
        const uint8_t* buf[2];
        buf[0] = host ? c->d_stage_in + (size_t)seq * c->stage_frame_bytes : s.left[seq];
        buf[1] = c->fmt->buffers == 1 ? buf[0] : host ? c->d_stage_in + (size_t)(c->B + seq) * c->stage_frame_bytes : s.right[seq];
        const uint8_t* src_l = buf[c->fmt->left.buffer] + (size_t)c->fmt->left.start * c->width;    // (gray formats; unused
        const uint8_t* src_r = buf[c->fmt->right.buffer] + (size_t)c->fmt->right.start * c->width;  //  when the format converts)
        const int M = (int)s.act.size();
        if (converts(c->input_format)) {
            // the ingest launch makes the gray images: straight into the set's own level 0 and right image, or,
            // with rectification on, into the group's raw planes, which the remap then reads (dense rows of the
            // aligned width). The pyramids are built from the set's own images (no ingest of theirs).
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            ImgView gray_l = is->own_left0, gray_r = is->own_right;
            if (c->rect) {
                const int pitch = (int)align_up((size_t)c->width, 64);
                gray_l = ImgView{c->d_raw_gray + (size_t)seq * c->raw_plane_bytes, c->width, c->height, pitch};
                gray_r = ImgView{c->d_raw_gray + (size_t)(c->B + seq) * c->raw_plane_bytes, c->width, c->height, pitch};
                c->remap_img.h[j] = RemapImg{gray_l, is->own_left0};
                c->remap_img.h[M + j] = RemapImg{gray_r, is->own_right};
            }
            c->ingest_img.h[j] = ingest_image(*c->fmt, 0, buf[c->fmt->left.buffer], s.stride, gray_l);
            c->ingest_img.h[M + j] = ingest_image(*c->fmt, 1, buf[c->fmt->right.buffer], s.stride, gray_r);
            hs.src_left = is->left[0];
        } else if (c->rect) {
            // rectification: the raw frames (in place, or from the staging buffer) are remapped into the
            // set's own level 0 and right image, then the pyramids are built from there (no ingest)
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            c->remap_img.h[j] = RemapImg{ImgView{src_l, c->width, c->height, s.stride}, is->own_left0};
            c->remap_img.h[M + j] = RemapImg{ImgView{src_r, c->width, c->height, s.stride}, is->own_right};
            hs.src_left = is->left[0];
        } else if (s.mem == SVO_MEM_DEVICE_BORROW) {
            // level 0 of both pyramids and the right image ARE the caller's images (like the
            // reference's shallow cv::Mat alias, stereo_slam.cpp:115): nothing is copied
            is->left[0] = ImgView{src_l, c->width, c->height, s.stride};
            is->right = ImgView{src_r, c->width, c->height, s.stride};
            hs.src_left = is->left[0];
        } else {
            // frames are ingested by the pyramid kernel itself (one launch for all sequences instead of
            // 2 copies per sequence); host-resident ones come through the staging buffer
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            hs.src_left = ImgView{src_l, c->width, c->height, s.stride};
            hs.src_right = ImgView{src_r, c->width, c->height, s.stride};
            hs.dst_right = is->right;
        }
        is->lk[0] = is->left[0];
        for (int l = 0; l < hs.n_levels; l++) hs.level[l] = is->left[l];
        hs.n_lk = c->n_lk;
        for (int l = 0; l < c->n_lk; l++) hs.lk[l] = is->lk[l];
        const int rows = pyr_stream_rows(hs);
        s.pyr_stream = (s.pyr_stream == 0 || rows == 0) ? 0 : std::max(s.pyr_stream, rows);
    }
    return SVO_OK;
}

// compaction of the sequence's current keypoint set into the other one, which becomes current
// (mode 0: remove_outliers, 1: find_bad_keypoints)
CompactArgs& pack_compact(svo_group* c, Seq& q, int slot, int mode) {
    CompactArgs& ca = clear(c->args.compact.h[slot]);
    ca.src = q.kps[q.cur]; ca.dst = q.kps[q.cur ^ 1]; ca.mode = mode;
    q.cur ^= 1;
    return ca;
}

// disparity search on the current keypoints: tracked frames clamp to half the window, keyframes
// search from the first new keypoint on (first_ptr)
void pack_ssd(svo_group* c, const Seq& q, int slot, int clamp_half, const int* first_ptr) {
    SsdArgs& sa = clear(c->args.ssd.h[slot]);
    const KpsDev& k = q.kps[q.cur];
    sa.left = q.cur_set->left[0]; sa.right = q.cur_set->right;
    sa.n_ptr = k.n; sa.kps2d = k.kps2d; sa.disparity = q.disparity;
    sa.win = c->cam.window_size_depth_calculator; sa.search_x = c->cam.search_x;
    sa.search_y = c->cam.search_y; sa.clamp_half = clamp_half;
    sa.first = 0; sa.first_ptr = first_ptr;
}

// arguments of the tracked frame's kernels: tracked sequence j in slot j
void pack_tracking_args(svo_group* c, const Step& st) {
    ArgBlocks& a = c->args;
    for (int slot = 0; slot < (int)st.trk.size(); slot++) {
        const int s = st.trk[slot];
        Seq& q = c->seqs[s];
        FrameResult* dr = c->d_res + s;
        // predicted pose = kf.statePre (stereo_slam.cpp:183-192)
        // (== statePost while the previous frame's filter update is still pending, dt = 0)
        for (int i = 0; i < 6; i++) a.guess.h[s][i] = q.pending ? q.kf.statePost[i] : q.kf.statePre[i];
        pack_compact(c, q, slot, 0).min_kf = &dr->min_kf;     // remove_outliers: the result is the frame's keypoints
        const KpsDev& k = q.kps[q.cur];
        SiaArgs& sa = clear(a.sia.h[slot]);
        for (int l = 0; l < c->cam.max_pyramid_levels; l++) {
            sa.prev[l] = q.prev_set->left[l];
            sa.cur[l] = q.cur_set->left[l];
        }
        sa.cam = c->cam; sa.n_ptr = k.n; sa.kps2d = k.kps2d; sa.kps3d = k.kps3d; sa.flags = k.flags;
        sa.pose_guess = a.guess.d[s]; sa.pose_out = dr->pose_sia; sa.cost_out = &dr->sia_cost;
        sa.trace = dr->sia_trace; sa.kp_ws = q.sia_kpws;
        sa.rec_ws = q.sia_rec; sa.rec_cap = c->rec_cap;
        sa.mats_out = q.sia_mats;
        sa.dbg_H = nullptr; sa.dbg_level = -1; sa.cap = c->cap; sa.exact_pinv = c->exact_pinv;
        KltArgs& ka = clear(a.klt.h[slot]);
        ka.kfs = q.d_kfs; ka.kf_id = k.kf_id; ka.n_cur = c->n_lk;
        for (int l = 0; l < c->n_lk; l++) ka.cur[l] = q.cur_set->lk[l];
        ka.n_ptr = k.n; ka.prev_pts = nullptr; ka.cur_pts = q.tracked; ka.status = q.klt_status;
        ka.err = q.klt_err; ka.win = c->cam.window_size_opt_flow;
        ka.proj_pose = dr->pose_sia; ka.proj_mats = q.sia_mats; ka.kps3d = k.kps3d; ka.proj_out = k.kps2d;
        ka.kp_index = k.kp_index; ka.ref_out = nullptr; ka.cam = c->cam;
        ReprojArgs& ra = clear(a.reproj.h[slot]);
        ra.cam = c->cam; ra.n_ptr = k.n; ra.kps2d = k.kps2d; ra.kps3d = k.kps3d; ra.flags = k.flags;
        ra.tracked = q.tracked; ra.err = q.klt_err; ra.pose_in = dr->pose_sia;
        ra.pose_out = dr->pose_refined; ra.cost_out = &dr->reproj_cost; ra.trace = &dr->reproj_trace;
        ra.exact_pinv = c->exact_pinv;
        ra.zero_out = c->d_inside + s;      // filter_update_kernel adds to it
        pack_ssd(c, q, slot, 1, nullptr);
        FilterArgs& fa = clear(a.filter.h[slot]);
        fa.cam = c->cam; fa.n_ptr = k.n; fa.frame_pose = dr->pose_refined;
        fa.kps2d = k.kps2d; fa.kps3d = k.kps3d; fa.flags = k.flags;
        fa.outlier_count = k.outl; fa.inlier_count = k.inl; fa.kf_inv_depth = k.kfx;
        fa.kf_variance = k.kfP; fa.disparity = q.disparity;
        fa.kfs = q.d_kfs; fa.kf_id = k.kf_id; fa.kp_index = k.kp_index;
        fa.do_outlier_check = 1; fa.do_update = 1; fa.do_flags = 1; fa.do_reproject = 1;
        fa.width = c->width; fa.height = c->height; fa.inside_count = c->d_inside + s;
    }
}

// one more launch of `kernel` (SVO_KERNEL_*) in shape `sh`
void count_launch(svo_group* c, int kernel, const LaunchShape& sh) {
    for (svo_launch_shape& e : c->launch_shapes)
        if (e.kernel == kernel && e.waves == sh.waves && e.mode == sh.mode && e.cap == sh.cap) {
            e.launches++;
            return;
        }
    c->launch_shapes.push_back({kernel, sh.waves, sh.mode, sh.cap, 1});
}

// the arguments upload, the pyramids of every sequence with a frame and the tracked frame's kernels for those
// that have a previous one; their inside-counters go back to the host for the keyframe decision
int launch_tracking(svo_group* c, const Step& s) {
    const ArgBlocks& a = c->args;
    hipStream_t st = c->stream.get();
    const int M = (int)s.act.size(), T = (int)s.trk.size();
    HIP_TRY(hipMemcpyAsync(a.dev, a.host.get(), a.frame_bytes, hipMemcpyHostToDevice, st));
    const bool ingest = converts(c->input_format);
    if (ingest) {
        // both sides of every active sequence in one launch (chunks of the grid's z limit)
        HIP_TRY(hipMemcpyAsync(c->ingest_img.d, c->ingest_img.h, sizeof(IngestImg) * 2 * M, hipMemcpyHostToDevice, st));
        for (int i0 = 0; i0 < 2 * M; i0 += 32768) {
            launch_ingest(c->ingest_img.d + i0, std::min(32768, 2 * M - i0), c->width, c->height, st);
            HIP_TRY(hipGetLastError());
        }
    }
    if (c->rect) {
        HIP_TRY(hipMemcpyAsync(c->remap_img.d, c->remap_img.h, sizeof(RemapImg) * 2 * M, hipMemcpyHostToDevice, st));
        RemapLaunch ra;
        ra.map[0] = c->rect[0]; ra.map[1] = c->rect[1];
        ra.img = c->remap_img.d; ra.n = M;
        launch_remap(ra, 2, st);
        HIP_TRY(hipGetLastError());
    }
    launch_pyr_fused(a.pyr.d, M, c->width, c->height, !c->rect && !ingest && s.mem != SVO_MEM_DEVICE_BORROW,
                     std::max(s.pyr_stream, 0), st);
    HIP_TRY(hipGetLastError());   // (every launch is checked on its own: a later success must not mask a failure)
    HIP_TRY(mark(c, 1));
    if (T == 0) {                 // only starting sequences: the stages of a tracked frame are empty
        for (int i = 2; i <= 7; i++) HIP_TRY(mark(c, i));
        return SVO_OK;
    }
    launch_compact(a.compact.d, T, c->cap, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 2));
    // the compaction can only shrink a sequence's keypoint set, so last frame's counts bound the
    // grids and the alignment kernel's LDS working set
    int grid_n = 1;
    for (int seq : s.trk) grid_n = std::max(grid_n, c->seqs[seq].n_host);
    grid_n = std::min(grid_n, c->cap);
    const LaunchStatus sia_launch =
        launch_sia(a.sia.d, T, c->cam, c->width, c->height, grid_n, c->rec_cap, c->exact_pinv, st);
    HIP_TRY(sia_launch.err);
    if (!sia_launch.shape.fits)
        return svo_set_error(SVO_ERR_CAPACITY, "sparse alignment: %d keypoints exceed the workspaces", grid_n);
    count_launch(c, SVO_KERNEL_SIA_GN, sia_launch.shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 3));
    launch_klt(a.klt.d, T, grid_n, c->cam.window_size_opt_flow, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 4));
    const LaunchStatus reproj_launch = launch_reproj(a.reproj.d, T, grid_n, st);
    HIP_TRY(reproj_launch.err);
    if (!reproj_launch.shape.fits)
        return svo_set_error(SVO_ERR_CAPACITY, "reprojection GN: %d keypoints do not fit LDS", grid_n);
    count_launch(c, SVO_KERNEL_REPROJ_GN, reproj_launch.shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 5));
    launch_ssd(a.ssd.d, T, grid_n, c->cam.window_size_depth_calculator, c->cam.search_y, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 6));
    launch_filter(a.filter.d, T, grid_n, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 7));
    HIP_TRY(hipMemcpyAsync(c->h_inside, c->d_inside, sizeof(int) * c->B, hipMemcpyDeviceToHost, st));
    return SVO_OK;
}

// arguments of the keyframe kernels for sequence s in `slot`: a new keyframe `id`
int pack_keyframe_args(svo_group* c, int slot, int s, bool first_frame) {
    ArgBlocks& a = c->args;
    Seq& q = c->seqs[s];
    FrameResult* dr = c->d_res + s;
    const int id = (int)q.kfs.size();
    const int rc = new_keyframe_storage(c, q, s, id);
    if (rc) return rc;
    // find_bad_keypoints: cur -> other, then the other set is current
    CompactArgs& ca = pack_compact(c, q, slot, 1);
    ca.width = c->width; ca.height = c->height;
    ca.zero = q.n_det; ca.zero_count = SVO_MAX_PYRAMID_LEVELS;      // (detection counters: cleared by the compaction kernel)
    if (first_frame) {
        // a sequence starts: no keypoints, and the slot's result block as a fresh ctx has it (no stream
        // operation of its own per starting sequence)
        ca.start = 1;
        ca.zero_res = reinterpret_cast<int*>(dr); ca.zero_res_count = (int)(sizeof(FrameResult) / sizeof(int));
    }
    DetectArgs& da = clear(a.detect.h[slot]);
    for (int l = 0; l < c->cam.max_pyramid_levels; l++) da.level[l] = q.cur_set->left[l];
    da.n_levels = c->det_levels; da.grid_w = c->cam.grid_width; da.grid_h = c->cam.grid_height;
    da.out = q.det; da.n_out = q.n_det; da.max_cells = c->max_cells;
    MergeArgs& ma = clear(a.merge.h[slot]);
    ma.cam = c->cam; ma.width = c->width; ma.height = c->height;
    ma.det = q.det; ma.n_det = q.n_det; ma.n_levels = c->det_levels; ma.max_cells = c->max_cells;
    ma.kps = q.kps[q.cur]; ma.cap = c->cap;
    ma.sel = q.sel; ma.sel_level = q.sel_level; ma.sel_cell = q.sel_cell; ma.occupied = q.occupied;
    ma.old_count = &dr->old_count; ma.overflow = &dr->overflow;
    pack_ssd(c, q, slot, 0, &dr->old_count);
    KfInitArgs& ia = clear(a.kf_init.h[slot]);
    ia.cam = c->cam; ia.kps = q.kps[q.cur]; ia.old_count = &dr->old_count;
    ia.disparity = q.disparity; ia.frame_pose = dr->pose_refined;
    ia.first_frame = first_frame ? 1 : 0; ia.new_kf_id = id; ia.kfs = q.d_kfs;
    ia.color_lcg = q.color_lcg; ia.n_out = &dr->kf_n;
    ia.record = a.kf_record.h[s];
    ia.tmpl_valid_bytes = (int)c->tmpl_valid_bytes;
    ia.evict_id = (c->tmpl_kf > 0 && id >= c->tmpl_kf) ? id - c->tmpl_kf : -1;
    return SVO_OK;
}

// keyframe creation for the sequences flagged in s.need: their argument blocks are
// packed into the first m slots, so the five launches cover exactly those sequences
int enqueue_keyframes(svo_group* c, const Step& s) {
    const ArgBlocks& a = c->args;
    hipStream_t st = c->stream.get();
    int m = 0;
    for (int seq = 0; seq < c->B; seq++) {
        if (!s.need[seq]) continue;
        const int rc = pack_keyframe_args(c, m++, seq, s.start[seq] != 0);
        if (rc) return rc;
    }
    if (m == 0) return SVO_OK;
    HIP_TRY(hipMemcpyAsync(a.dev, a.host.get(), a.bytes, hipMemcpyHostToDevice, st));
    // (a launch that fails must not be masked by the next one that succeeds: checked one by one)
    launch_compact(a.compact.d, m, c->cap, st);
    HIP_TRY(hipGetLastError());
    if (c->det_levels > 0) {
        launch_detect(a.detect.d, m, c->max_cells, c->det_levels, c->cam.grid_width, c->cam.grid_height, st);
        HIP_TRY(hipGetLastError());
    }
    launch_select_merge(a.merge.d, m, c->max_cells, st);
    HIP_TRY(hipGetLastError());
    launch_ssd(a.ssd.d, m, c->cap, c->cam.window_size_depth_calculator, c->cam.search_y, st);
    HIP_TRY(hipGetLastError());
    launch_kf_init(a.kf_init.d, m, st);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

// which sequences make a keyframe (every one that starts, stereo_slam.cpp:141-160) and their launches
int decide_keyframes(svo_group* c, Step& s) {
    // KeyFrameManager::keyframe_needed (keyframe_manager.cpp:66-72)
    const int max_keypoints = (c->width / c->cam.grid_width) * (c->height / c->cam.grid_height);
    bool any = false;
    for (int seq : s.act) {
        s.need[seq] = s.start[seq] || (double)c->h_inside[seq] < 0.66 * max_keypoints ? 1 : 0;
        any = any || s.need[seq];
    }
    return any ? enqueue_keyframes(c, s) : SVO_OK;
}

int read_stage_times(svo_group* c, Step& s) {
    HIP_TRY(mark(c, 8));
    if (!c->timing) return SVO_OK;
    HIP_TRY(hipEventSynchronize(c->ev[8].get()));
    for (int i = 0; i < 8; i++) (void)hipEventElapsedTime(&s.stage_ms[i], c->ev[i].get(), c->ev[i + 1].get());
    return SVO_OK;
}

// Keyframe images are only read for keypoints that came from that keyframe (KLT builds a template from
// them when the cache has none). The frame's keypoints — kept by the compaction at its start, plus what a
// keyframe created in this frame adds — refer to keyframes r.min_kf and younger and, of the next 64, to
// those whose bit is set in r.live_kf: the others hand their image sets back to the sequence's free
// list, so memory stays bounded by the keyframes still in use
// instead of growing with every keyframe (the reference keeps them all). Nothing else of a keyframe goes:
// its keypoint arrays, pose and table record stay for the depth filter and the getters.
void retire_keyframe_images(svo_group* c, const Step& s) {
    for (int seq : s.trk) {
        Seq& q = c->seqs[seq];
        const FrameResult& r = c->h_res[seq];
        const int newest = (int)q.kfs.size() - 1;                  // (never the newest: a keyframe made in this frame)
        for (; q.kfs_retired < std::min(r.min_kf, newest); q.kfs_retired++) release_set(q, q.kfs[q.kfs_retired].set);
        for (int i = 0; i < 64 && r.min_kf < newest && r.min_kf + i < newest; i++) {
            KfHost& old = q.kfs[r.min_kf + i];
            if (old.set && !((r.live_kf[i >> 5] >> (i & 31)) & 1u)) release_set(q, old.set);
        }
    }
}

// host bookkeeping (stereo_slam.cpp:250-270); the pose filter itself is deferred
int book_frame(svo_group* c, Step& s) {
    int overflow_seq = -1;
    for (int seq : s.act) {
        Seq& q = c->seqs[seq];
        const FrameResult& r = c->h_res[seq];
        const double ts = (double)s.time_stamps[seq];
        const bool first = s.start[seq] != 0;
        q.frame_id++;
        if (first) {
            std::memset(q.pose, 0, sizeof(q.pose));
            q.ts = ts;
            q.trajectory.push_back(svo_pose{});         // (the zero pose)
        } else {
            q.pending = true;
            std::memcpy(q.pending_pose, r.pose_refined, sizeof(q.pending_pose));
            q.pending_ts = ts;
        }
        if (s.need[seq]) {
            KfHost& k = q.kfs.back();
            k.n = r.kf_n;
            if (first) std::memset(k.pose, 0, sizeof(k.pose));
            else std::memcpy(k.pose, r.pose_refined, sizeof(k.pose));
        }
        q.n_host = c->h_n[2 * seq + q.cur];
        svo_frame_stats& st = clear(q.stats);
        st.frame_id = q.frame_id; st.is_keyframe = s.need[seq]; st.n_keypoints = q.n_host;
        st.n_keyframes = (int)q.kfs.size(); st.inside_count = first ? 0 : c->h_inside[seq]; st.overflow = r.overflow;
        std::memcpy(st.pose_sia, r.pose_sia, sizeof(st.pose_sia));
        std::memcpy(st.pose_refined, r.pose_refined, sizeof(st.pose_refined));
        st.sia_cost = r.sia_cost; st.reproj_cost = r.reproj_cost; st.sia_ms = s.stage_ms[2];
        std::memcpy(st.stage_ms, s.stage_ms, sizeof(s.stage_ms));
        std::memcpy(st.sia_trace, r.sia_trace, sizeof(st.sia_trace));
        st.reproj_trace = r.reproj_trace;
        c->totals.frames++;
        c->totals.keyframes += s.need[seq];
        c->totals.keypoints += q.n_host;
        if (!first)
            for (int l = 0; l < SVO_MAX_PYRAMID_LEVELS; l++) {
                c->totals.gn_gradient_calls += r.sia_trace[l].n_gradient;
                c->totals.gn_cost_calls += r.sia_trace[l].n_cost;
            }
        if (r.overflow && overflow_seq < 0) overflow_seq = seq;     // reported after every sequence is booked
    }
    lap(c, s, 6);   // bookkeeping
    c->host_steps++;
    c->totals.launches++;
    for (int i = 0; i < 8; i++) c->totals.stage_ms[i] += s.stage_ms[i];
    c->totals.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - s.t0).count();
    if (overflow_seq >= 0)
        return svo_set_error(SVO_ERR_CAPACITY, "sequence %d: more than %d keypoints", overflow_seq, c->cap);
    return SVO_OK;
}

// One frame of the group, as its phases. SVO_HOST_TIMING laps: args, launch, pose_filter, wait_frame,
// kf_enqueue, wait_kf, bookkeeping.
int step(svo_group* c, Step& s) {
    HIP_TRY(hipSetDevice(c->device));
    s.t0 = s.lap_start = std::chrono::steady_clock::now();
    int rc = select_sequences(c, s);
    if (rc || s.act.empty()) return rc;
    HIP_TRY(mark(c, 0));
    if (s.mem == SVO_MEM_HOST && (rc = stage_host_frames(c, s))) return rc;
    if ((rc = pack_pyramids(c, s))) return rc;
    pack_tracking_args(c, s);
    lap(c, s, 0);
    if ((rc = launch_tracking(c, s))) return rc;
    lap(c, s, 1);
    flush_pending(c);                     // previous frame's pose filter, overlapped with the kernels
    lap(c, s, 2);
    if (!s.trk.empty()) HIP_TRY(hipStreamSynchronize(c->stream.get()));   // the inside-counters
    lap(c, s, 3);
    if ((rc = decide_keyframes(c, s))) return rc;
    lap(c, s, 4);
    HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, c->readback_bytes, hipMemcpyDeviceToHost, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));   // results + counts
    lap(c, s, 5);
    if ((rc = read_stage_times(c, s))) return rc;
    if (c->retire_kf_images) retire_keyframe_images(c, s);
    return book_frame(c, s);
}

}  // namespace

// A frame that fails half way (HIP error, capacity) leaves the sequences of the group at mixed
// frame ids: the group is marked failed and rejects further frames instead of tracking on.
int grp_new_images(svo_group* c, const uint8_t* const* left, const uint8_t* const* right, int stride,
                   const float* time_stamps, int mem) {
    if (!c || !left || (!right && c->fmt->buffers == 2) || !time_stamps ||
        (long long)stride < (long long)ingest_row_pixels(*c->fmt, c->width) * c->fmt->channels)
        return svo_set_error(SVO_ERR_INVALID, "svo_new_images: bad arguments");
    if (c->failed)
        return svo_set_error(SVO_ERR_INVALID, "svo_new_images: an earlier frame of this ctx failed; create a new ctx");
    Step s;
    s.left = left; s.right = right; s.stride = stride; s.mem = mem; s.time_stamps = time_stamps;
    const int rc = step(c, s);
    if (rc != SVO_OK) c->failed = true;
    return rc;
}

// ------------------------------------------------------------------ the end of a sequence

namespace {

// The sequence of the slot ends (between two steps of the group: its stream is idle). Its image sets and
// keyframe keypoint slabs go back to their free lists, its host state becomes that of a fresh ctx, and a host
// record of the run stays. Nothing is cleared on the device: the slot's next frame is frame 0 of a new
// sequence, whose kernels reset what they read (compact_kernel: keypoint counts and result block,
// kf_init_kernel: colour generator, table record and "stored" flags of keyframe 0). Records and template-cache
// blocks of the old run's keyframes stay behind in the table, but a keypoint only refers to a keyframe id that
// its own run has created, and creating it rewrites both.
void end_sequence(svo_group* c, int s) {
    Seq& q = c->seqs[s];
    if (q.frame_id < 0) return;              // empty: nothing to end
    flush_one(q);
    FinishedRun f;
    clear(f.info);
    f.info.seq = s; f.info.run = q.run; f.info.frames = q.frame_id + 1; f.info.keyframes = (int)q.kfs.size();
    f.info.last_time_stamp = (float)q.ts;
    std::memcpy(f.info.pose, q.pose, sizeof(f.info.pose));
    f.trajectory = std::move(q.trajectory);
    c->finished.push_back(std::move(f));
    for (KfHost& k : q.kfs) {
        release_set(q, k.set);
        c->kf_slabs.push_back(reinterpret_cast<uint8_t*>(k.kps.kps3d));
    }
    release_set(q, q.cur_set);
    release_set(q, q.prev_set);
    q.kfs.clear();
    q.kfs_retired = 0;
    q.trajectory.clear();
    q.cur = 0; q.n_host = 0; q.frame_id = -1; q.ts = 0; q.run++;
    std::memset(q.pose, 0, sizeof(q.pose));
    q.kf.init();
    clear(q.stats);
}

}  // namespace

int grp_restart_sequences(svo_group* c, const int* seqs, int n) {
    if (c->failed)
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_restart_sequences: an earlier frame of this ctx failed; create a new ctx");
    for (int i = 0; i < n; i++) end_sequence(c, seqs[i]);
    return SVO_OK;
}

void grp_drop_finished_runs(svo_group* c, int seq) {
    if (seq < 0) { c->finished.clear(); return; }
    c->finished.erase(std::remove_if(c->finished.begin(), c->finished.end(),
                                     [seq](const FinishedRun& f) { return f.info.seq == seq; }),
                      c->finished.end());
}

svo_memory grp_memory(const svo_group* c) {
    svo_memory m;
    clear(m);
    m.device_bytes = (int64_t)c->device_bytes;
    m.klt_cache_bytes = (int64_t)((size_t)c->B * c->tmpl_kf * (c->tmpl_block_bytes + c->tmpl_valid_bytes));
    m.image_sets = c->image_sets;
    for (const Seq& q : c->seqs) m.image_sets_free += (int)q.free_sets.size();
    m.keyframe_slabs = c->kf_slab_count;
    m.keyframe_slabs_free = (int)c->kf_slabs.size();
    return m;
}

// ------------------------------------------------------------------ bulk export

extern "C" int svo_export_capacity(const svo_camera_settings* cam, int width, int height, int* records_per_sequence) {
    if (!records_per_sequence) return svo_set_error(SVO_ERR_INVALID, "svo_export_capacity: bad arguments");
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    *records_per_sequence = keypoint_capacity(*cam, width, height);
    return SVO_OK;
}

int grp_capacity(const svo_group* c) { return c->cap; }

// The named slots of the group as segments and records (svo_submit_export). The counts are the host's own
// (Seq::n_host, KfHost::n), so the tile table is built here; it goes up through the group's argument blocks, pinned
// and device: between two steps the stream is idle and nothing in them is live (every step fills and uploads what
// its launches read), so an export allocates no table of its own. One launch unless the table outgrows the
// blocks. Host mode packs into the staging block and copies the used prefix of each array out.
int grp_export(svo_group* c, int what, int mem, const int* seqs, const int* seg, int n, int seq0, int64_t base,
               const svo_export_dst* dst) {
    if (c->failed)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export: an earlier frame of this ctx failed; create a new ctx");
    HIP_TRY(hipSetDevice(c->device));
    flush_pending(c);
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    svo_kp2d* o2 = dst->kps2d ? dst->kps2d + base : nullptr;
    svo_kp3d* o3 = dst->kps3d ? dst->kps3d + base : nullptr;
    svo_kp_info* oi = dst->info ? dst->info + base : nullptr;
    const bool any = o2 || o3 || oi;
    if (host && any) {
        const size_t records = (size_t)c->B * c->cap;
        if (!c->d_export)
            if (const int rc = dev_alloc(c, &c->d_export, records * (sizeof(svo_kp2d) + sizeof(svo_kp3d) + sizeof(svo_kp_info)))) return rc;
        if (o2) o2 = reinterpret_cast<svo_kp2d*>(c->d_export);
        if (o3) o3 = reinterpret_cast<svo_kp3d*>(c->d_export + records * sizeof(svo_kp2d));
        if (oi) oi = reinterpret_cast<svo_kp_info*>(c->d_export + records * (sizeof(svo_kp2d) + sizeof(svo_kp3d)));
    }
    ExportTile* h_tiles = reinterpret_cast<ExportTile*>(c->args.host.get());
    ExportTile* d_tiles = reinterpret_cast<ExportTile*>(c->args.dev);
    size_t table_cap = c->args.bytes / sizeof(ExportTile);
    if (const char* e = std::getenv("SVO_EXPORT_TABLE_TILES"))     // diagnostic: a smaller table (tests reach the chunked launches)
        table_cap = std::max<size_t>(1, std::min<size_t>(table_cap, (size_t)std::atoll(e)));
    size_t m = 0;
    // the tiles so far; `more`: the pinned table is filled again, so the upload must be over
    auto launch = [&](bool more) -> int {
        if (m == 0) return SVO_OK;
        HIP_TRY(hipMemcpyAsync(d_tiles, h_tiles, sizeof(ExportTile) * m, hipMemcpyHostToDevice, st));
        launch_export(d_tiles, (int)m, o2, o3, oi, st);
        HIP_TRY(hipGetLastError());
        if (more) HIP_TRY(hipStreamSynchronize(st));
        m = 0;
        return SVO_OK;
    };
    int64_t used = 0;                        // records of the group so far
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_export_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.keyframe_id = -1;
        e.is_keyframe = q.stats.is_keyframe; e.time_stamp = (float)q.ts;
        const KpsDev* src = &q.kps[q.cur];
        if (what == SVO_EXPORT_FRAMES) {
            e.n = q.n_host;
            std::memcpy(e.pose, q.pose, sizeof(e.pose));
        } else if (!q.kfs.empty()) {
            const KfHost& k = q.kfs.back();
            e.keyframe_id = (int)q.kfs.size() - 1;
            e.n = k.n;
            std::memcpy(e.pose, k.pose, sizeof(e.pose));
            src = &k.kps;
        }
        used = (int64_t)align_up((size_t)used, 4);
        e.first = base + used;
        for (int start = 0; any && start < e.n; start += EXPORT_TILE) {
            if (m == table_cap)
                if (const int rc = launch(true)) return rc;
            h_tiles[m++] = export_tile(*src, start, std::min(EXPORT_TILE, e.n - start), used);
        }
        used += e.n;
    }
    if (const int rc = launch(false)) return rc;
    if (host && used > 0) {
        if (o2) HIP_TRY(hipMemcpyAsync(dst->kps2d + base, o2, sizeof(svo_kp2d) * used, hipMemcpyDeviceToHost, st));
        if (o3) HIP_TRY(hipMemcpyAsync(dst->kps3d + base, o3, sizeof(svo_kp3d) * used, hipMemcpyDeviceToHost, st));
        if (oi) HIP_TRY(hipMemcpyAsync(dst->info + base, oi, sizeof(svo_kp_info) * used, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}

// ------------------------------------------------------------------ snapshots (svo_submit_save / svo_submit_load)

namespace {

using SnapHeader = struct svo_snapshot_info;    // (the tag: svo_snapshot_info alone names the function)
constexpr int KP_PLANES = 12;
constexpr int KP_PLANE_ELEM[KP_PLANES] = {sizeof(svo_kp2d), sizeof(svo_kp3d), 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
constexpr int FIXED_PLANES = KP_PLANES + 2;     // the current keypoint set, the colour generator's word, the device count
constexpr size_t SNAP_FRAME_BYTES = sizeof(double) + sizeof(float) * 6 + sizeof(svo_frame_stats);
static_assert(sizeof(SnapHeader) == 160 && sizeof(PoseFilter) == 4128 && SNAP_FRAME_BYTES == 616 &&
              sizeof(svo_snapshot_keyframe) == 32 && sizeof(svo_snapshot_plane) == 16 && sizeof(svo_pose) == 24,
              "the snapshot format of include/svo_hip.h");

// the arrays of a keypoint set in directory order
void kps_planes(const KpsDev& k, uint8_t* out[KP_PLANES]) {
    void* p[KP_PLANES] = {k.kps2d, k.kps3d, k.flags, k.kf_id, k.kp_index, k.outl, k.inl, k.kfx, k.kfP, k.score, k.level_type, k.color};
    for (int i = 0; i < KP_PLANES; i++) out[i] = static_cast<uint8_t*>(p[i]);
}

struct PlaneDim { int row_bytes, rows; };

// the extent every plane of a snapshot has, in directory order (the header's counts are checked already)
std::vector<PlaneDim> snapshot_plane_dims(const SnapHeader& h, const svo_snapshot_keyframe* kfs) {
    std::vector<PlaneDim> v;
    v.reserve((size_t)h.n_planes);
    for (int i = 0; i < KP_PLANES; i++) v.push_back({KP_PLANE_ELEM[i] * h.n_keypoints, 1});
    v.push_back({4, 1});
    v.push_back({4, 1});
    for (int k = 0; k < h.n_keyframes; k++)
        for (int i = 0; i < KP_PLANES; i++) v.push_back({KP_PLANE_ELEM[i] * kfs[k].n, 1});
    for (int s = 0; s < h.n_image_sets; s++) {
        for (int l = 0; l < h.pyramid_levels; l++) v.push_back({h.width >> l, h.height >> l});
        v.push_back({h.width, h.height});
        for (int l = 1, w = h.width, ht = h.height; l < h.lk_levels; l++) {
            w = (w + 1) / 2; ht = (ht + 1) / 2;
            v.push_back({w, ht});
        }
    }
    return v;
}

int64_t snapshot_plane_count(const SnapHeader& h) {
    return FIXED_PLANES + (int64_t)KP_PLANES * h.n_keyframes + (int64_t)h.n_image_sets * (h.pyramid_levels + h.lk_levels);
}

int64_t snapshot_host_bytes(const SnapHeader& h) {
    return (int64_t)(sizeof(SnapHeader) + sizeof(PoseFilter) + SNAP_FRAME_BYTES) + (int64_t)sizeof(svo_pose) * h.n_trajectory +
           (int64_t)sizeof(svo_snapshot_keyframe) * h.n_keyframes + (int64_t)sizeof(svo_snapshot_plane) * h.n_planes;
}

// the sections of a checked host part (an aligned private copy)
struct SnapView {
    const SnapHeader* h;
    const PoseFilter* filter;
    const uint8_t* frame;
    const svo_pose* trajectory;
    const svo_snapshot_keyframe* kfs;
    const svo_snapshot_plane* dir;
};

SnapView snapshot_view(const uint8_t* p) {
    SnapView v;
    v.h = reinterpret_cast<const SnapHeader*>(p);
    p += sizeof(SnapHeader);
    v.filter = reinterpret_cast<const PoseFilter*>(p);
    p += sizeof(PoseFilter);
    v.frame = p;
    p += SNAP_FRAME_BYTES;
    v.trajectory = reinterpret_cast<const svo_pose*>(p);
    p += sizeof(svo_pose) * (size_t)v.h->n_trajectory;
    v.kfs = reinterpret_cast<const svo_snapshot_keyframe*>(p);
    p += sizeof(svo_snapshot_keyframe) * (size_t)v.h->n_keyframes;
    v.dir = reinterpret_cast<const svo_snapshot_plane*>(p);
    return v;
}

#define SNAP_BAD(...) return svo_set_error(SVO_ERR_INVALID, "snapshot: " __VA_ARGS__)

// Checks a host part completely and copies it (header only for a header-only part) into `copy`, aligned.
int check_snapshot(const void* host_part, int64_t bytes, std::vector<uint8_t>& copy) {
    if (!host_part || bytes < (int64_t)sizeof(SnapHeader)) SNAP_BAD("the host part is shorter than its header");
    SnapHeader h;
    std::memcpy(&h, host_part, sizeof(h));
    if (h.magic != SVO_SNAPSHOT_MAGIC) SNAP_BAD("bad magic");
    if (h.version != SVO_SNAPSHOT_VERSION) SNAP_BAD("version %u, this library reads version %d", h.version, SVO_SNAPSHOT_VERSION);
    if (h.byte_order != SVO_SNAPSHOT_BYTE_ORDER) SNAP_BAD("not little endian");
    if (h.status != SVO_SNAPSHOT_COMPLETE && h.status != SVO_SNAPSHOT_TOO_SMALL) SNAP_BAD("bad status %u", h.status);
    if (h._reserved != 0) SNAP_BAD("reserved field is not 0");
    if (h.width < 16 || h.height < 16 || check_settings(&h.cam, h.width, h.height, 1) != SVO_OK) SNAP_BAD("bad camera settings or size");
    if (h.capacity != keypoint_capacity(h.cam, h.width, h.height)) SNAP_BAD("capacity %d does not follow from the settings", h.capacity);
    if (h.pyramid_levels != h.cam.max_pyramid_levels || h.lk_levels != usable_lk_levels(h.cam, h.width, h.height))
        SNAP_BAD("level counts do not follow from the settings");
    if (h.frame_id < -1 || h.n_trajectory != h.frame_id + 1) SNAP_BAD("frame id %d with %d poses", h.frame_id, h.n_trajectory);
    if (h.n_keypoints < 0 || h.n_keypoints > h.capacity) SNAP_BAD("%d keypoints, capacity %d", h.n_keypoints, h.capacity);
    if (h.n_keyframes < 0 || h.n_keyframes > MAX_KEYFRAMES) SNAP_BAD("%d keyframes", h.n_keyframes);
    if (h.n_image_sets < 0 || h.n_image_sets > h.n_keyframes + 1) SNAP_BAD("%d image sets for %d keyframes", h.n_image_sets, h.n_keyframes);
    if (h.keyframes_retired < 0 || h.keyframes_retired > std::max(h.n_keyframes - 1, 0)) SNAP_BAD("%d keyframes retired of %d", h.keyframes_retired, h.n_keyframes);
    if (h.frame_id < 0 ? (h.n_keypoints || h.n_keyframes || h.n_image_sets) : (h.n_keyframes < 1 || h.n_image_sets < 1))
        SNAP_BAD("counts do not fit frame id %d", h.frame_id);
    if ((int64_t)h.n_planes != snapshot_plane_count(h)) SNAP_BAD("%d planes", h.n_planes);
    if (h.host_bytes != snapshot_host_bytes(h) || h.data_bytes < 0) SNAP_BAD("sizes do not fit the counts");
    if (h.status == SVO_SNAPSHOT_TOO_SMALL) {
        copy.assign(reinterpret_cast<const uint8_t*>(&h), reinterpret_cast<const uint8_t*>(&h) + sizeof(h));
        return SVO_OK;
    }
    if (bytes < h.host_bytes) SNAP_BAD("the host part has %lld bytes of %lld", (long long)bytes, (long long)h.host_bytes);
    copy.assign(static_cast<const uint8_t*>(host_part), static_cast<const uint8_t*>(host_part) + h.host_bytes);
    const SnapView v = snapshot_view(copy.data());
    std::vector<int> refs((size_t)h.n_image_sets, 0);
    for (int k = 0; k < h.n_keyframes; k++) {
        const svo_snapshot_keyframe& kf = v.kfs[k];
        if (kf.n < 0 || kf.n > h.capacity) SNAP_BAD("keyframe %d: %d keypoints, capacity %d", k, kf.n, h.capacity);
        if (kf.image_set < -1 || kf.image_set >= h.n_image_sets || (k < h.keyframes_retired && kf.image_set != -1))
            SNAP_BAD("keyframe %d: image set %d", k, kf.image_set);
        if (kf.image_set >= 0) refs[kf.image_set]++;
    }
    for (int s = 1; s < h.n_image_sets; s++)
        if (!refs[s]) SNAP_BAD("image set %d belongs to no keyframe", s);
    const std::vector<PlaneDim> dims = snapshot_plane_dims(h, v.kfs);
    for (int i = 0; i < h.n_planes; i++) {
        const svo_snapshot_plane& p = v.dir[i];
        if (p.row_bytes != dims[i].row_bytes || p.rows != dims[i].rows)
            SNAP_BAD("plane %d: %d x %d bytes, must be %d x %d", i, p.rows, p.row_bytes, dims[i].rows, dims[i].row_bytes);
        if (p.offset < 0 || p.offset > h.data_bytes || (int64_t)p.row_bytes * p.rows > h.data_bytes - p.offset)
            SNAP_BAD("plane %d lies outside the data part", i);
    }
    return SVO_OK;
}

// what a save of the slot writes: header, keyframe records, directory, and the image sets in saved order
struct SavePlan {
    SnapHeader h;
    std::vector<svo_snapshot_keyframe> kfs;
    std::vector<svo_snapshot_plane> dir;
    std::vector<ImageSet*> sets;
};

void plan_snapshot(const svo_group* c, const Seq& q, SavePlan& p) {
    SnapHeader& h = clear(p.h);
    h.magic = SVO_SNAPSHOT_MAGIC; h.version = SVO_SNAPSHOT_VERSION; h.byte_order = SVO_SNAPSHOT_BYTE_ORDER;
    h.cam = c->cam; h.width = c->width; h.height = c->height; h.capacity = c->cap;
    h.pyramid_levels = c->cam.max_pyramid_levels; h.lk_levels = c->n_lk;
    h.frame_id = q.frame_id;
    if (q.frame_id >= 0) {
        h.n_keypoints = q.n_host; h.n_trajectory = (int)q.trajectory.size();
        h.n_keyframes = (int)q.kfs.size(); h.keyframes_retired = q.kfs_retired;
        p.sets.push_back(q.cur_set);
        for (const KfHost& k : q.kfs) {
            svo_snapshot_keyframe r;
            std::memcpy(r.pose, k.pose, sizeof(r.pose));
            r.n = k.n; r.image_set = -1;
            if (k.set) {
                const auto it = std::find(p.sets.begin(), p.sets.end(), k.set);
                r.image_set = (int)(it - p.sets.begin());
                if (it == p.sets.end()) p.sets.push_back(k.set);
            }
            p.kfs.push_back(r);
        }
    }
    h.n_image_sets = (int)p.sets.size();
    h.n_planes = (int)snapshot_plane_count(h);
    int64_t off = 0;
    for (const PlaneDim& d : snapshot_plane_dims(h, p.kfs.data())) {
        p.dir.push_back({off, d.row_bytes, d.rows});
        off += (int64_t)align_up((size_t)d.row_bytes * d.rows, 16);
    }
    h.host_bytes = snapshot_host_bytes(h);
    h.data_bytes = off;
}

// where the planes of a slot's state lie on the device, in directory order: the address and the row pitch
struct DevPlane { uint8_t* p; int64_t pitch; };

std::vector<DevPlane> device_planes(const svo_group* c, const Seq& q, const std::vector<ImageSet*>& sets) {
    std::vector<DevPlane> v;
    uint8_t* a[KP_PLANES];
    kps_planes(q.kps[q.cur], a);
    for (uint8_t* p : a) v.push_back({p, 0});
    v.push_back({reinterpret_cast<uint8_t*>(q.color_lcg), 0});
    v.push_back({reinterpret_cast<uint8_t*>(q.d_n + q.cur), 0});
    for (const KfHost& k : q.kfs) {
        kps_planes(k.kps, a);
        for (uint8_t* p : a) v.push_back({p, 0});
    }
    auto image = [&v](const ImgView& im) { v.push_back({const_cast<uint8_t*>(im.data), im.stride}); };
    for (const ImageSet* s : sets) {
        for (int l = 0; l < c->cam.max_pyramid_levels; l++) image(s->left[l]);
        image(s->right);
        for (int l = 1; l < c->n_lk; l++) image(s->lk[l]);
    }
    return v;
}

// The tile table of a save or a load. Like grp_export's it goes up through the group's argument blocks, pinned
// and device: between two steps the stream is idle and nothing in them is live. One launch unless the table
// outgrows the blocks (SVO_SNAPSHOT_TABLE_TILES: a smaller table, so that tests reach the chunked launches).
struct TileTable {
    svo_group* c;
    CopyTile* h;
    CopyTile* d;
    size_t cap, m = 0;
    std::vector<CopyTile> cut;
    explicit TileTable(svo_group* g) : c(g) {
        h = reinterpret_cast<CopyTile*>(c->args.host.get());
        d = reinterpret_cast<CopyTile*>(c->args.dev);
        cap = c->args.bytes / sizeof(CopyTile);
        if (const char* e = std::getenv("SVO_SNAPSHOT_TABLE_TILES"))
            cap = std::max<size_t>(1, std::min<size_t>(cap, (size_t)std::atoll(e)));
    }
    // the tiles so far; `more`: the pinned table is filled again, so the upload must be over
    int launch(bool more) {
        if (m == 0) return SVO_OK;
        hipStream_t st = c->stream.get();
        HIP_TRY(hipMemcpyAsync(d, h, sizeof(CopyTile) * m, hipMemcpyHostToDevice, st));
        launch_copy_tiles(d, (int)m, st);
        HIP_TRY(hipGetLastError());
        if (more) HIP_TRY(hipStreamSynchronize(st));
        m = 0;
        return SVO_OK;
    }
    int add(const void* src, void* dst, int64_t row_bytes, int64_t rows, int64_t src_pitch, int64_t dst_pitch) {
        cut.clear();
        cut_copy_tiles(src, dst, row_bytes, rows, src_pitch, dst_pitch, cut);
        for (const CopyTile& t : cut) {
            if (m == cap)
                if (const int rc = launch(true)) return rc;
            h[m++] = t;
        }
        return SVO_OK;
    }
};

// the host-mode staging block holds `bytes`
int reserve_snap_stage(svo_group* c, size_t bytes) {
    if (bytes <= c->snap_bytes) return SVO_OK;
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    if (c->d_snap) dev_release(c, c->d_snap, c->snap_bytes);
    c->d_snap = nullptr; c->snap_bytes = 0;
    if (const int rc = dev_alloc(c, &c->d_snap, bytes, false)) return rc;
    c->snap_bytes = bytes;
    return SVO_OK;
}

}  // namespace

int grp_snapshot_size(svo_group* c, int s, int64_t* host_bytes, int64_t* data_bytes) {
    flush_one(c->seqs[s]);
    SavePlan p;
    plan_snapshot(c, c->seqs[s], p);
    if (host_bytes) *host_bytes = p.h.host_bytes;
    if (data_bytes) *data_bytes = p.h.data_bytes;
    return SVO_OK;
}

int grp_check_snapshot(const svo_group* c, const svo_snapshot* snap, std::vector<uint8_t>* host_copy) {
    if (const int rc = check_snapshot(snap->host, snap->host_capacity, *host_copy)) return rc;
    const SnapHeader& h = *reinterpret_cast<const SnapHeader*>(host_copy->data());
    if (h.status != SVO_SNAPSHOT_COMPLETE) SNAP_BAD("only the header was saved (a capacity was too small)");
    if (std::memcmp(&h.cam, &c->cam, sizeof(h.cam)) != 0 || h.width != c->width || h.height != c->height || h.capacity != c->cap)
        SNAP_BAD("camera settings, size or capacity differ from the ctx's");
    if (snap->data_capacity < h.data_bytes || (h.data_bytes > 0 && !snap->data))
        SNAP_BAD("the data part has %lld bytes of %lld", (long long)snap->data_capacity, (long long)h.data_bytes);
    return SVO_OK;
}

// One group's share of svo_submit_save, between two steps of the group: slot seqs[i] into snaps[i].
int grp_save(svo_group* c, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    if (c->failed)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_save: an earlier frame of this ctx failed; create a new ctx");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    std::vector<SavePlan> plans((size_t)n);
    std::vector<size_t> stage_off((size_t)n, 0);
    size_t stage = 0;
    for (int i = 0; i < n; i++) {
        Seq& q = c->seqs[seqs[i]];
        flush_one(q);
        SavePlan& p = plans[i];
        plan_snapshot(c, q, p);
        const svo_snapshot& out = snaps[i];
        if (out.host_capacity < p.h.host_bytes || out.data_capacity < p.h.data_bytes) {
            p.h.status = SVO_SNAPSHOT_TOO_SMALL;
            std::memcpy(out.host, &p.h, sizeof(p.h));
            continue;
        }
        std::vector<uint8_t> part((size_t)p.h.host_bytes);
        uint8_t* w = part.data();
        auto put = [&w](const void* src, size_t bytes) { if (bytes) std::memcpy(w, src, bytes); w += bytes; };
        put(&p.h, sizeof(p.h));
        put(&q.kf, sizeof(PoseFilter));
        put(&q.ts, sizeof(double));
        put(q.pose, sizeof(q.pose));
        put(&q.stats, sizeof(q.stats));
        put(q.trajectory.data(), sizeof(svo_pose) * q.trajectory.size());
        put(p.kfs.data(), sizeof(svo_snapshot_keyframe) * p.kfs.size());
        put(p.dir.data(), sizeof(svo_snapshot_plane) * p.dir.size());
        std::memcpy(out.host, part.data(), part.size());
        stage_off[i] = stage;
        stage += align_up((size_t)p.h.data_bytes, 256);
    }
    if (host && stage > 0) {
        if (const int rc = reserve_snap_stage(c, stage)) return rc;
        HIP_TRY(hipMemsetAsync(c->d_snap, 0, stage, st));     // (the bytes between planes: a host-mode snapshot is all defined)
    }
    TileTable table(c);
    for (int i = 0; i < n; i++) {
        const SavePlan& p = plans[i];
        if (p.h.status != SVO_SNAPSHOT_COMPLETE) continue;
        const Seq& q = c->seqs[seqs[i]];
        uint8_t* base = host ? c->d_snap + stage_off[i] : static_cast<uint8_t*>(snaps[i].data);
        const std::vector<DevPlane> dev = device_planes(c, q, p.sets);
        for (size_t j = 0; j < dev.size(); j++) {
            const svo_snapshot_plane& e = p.dir[j];
            if (const int rc = table.add(dev[j].p, base + e.offset, e.row_bytes, e.rows, dev[j].pitch, e.row_bytes)) return rc;
        }
    }
    if (const int rc = table.launch(false)) return rc;
    if (host)
        for (int i = 0; i < n; i++)
            if (plans[i].h.status == SVO_SNAPSHOT_COMPLETE && plans[i].h.data_bytes > 0)
                HIP_TRY(hipMemcpyAsync(snaps[i].data, c->d_snap + stage_off[i], (size_t)plans[i].h.data_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}

// One group's share of svo_submit_load, between two steps of the group. The host parts are checked copies
// (grp_check_snapshot); the data parts are trusted.
int grp_load(svo_group* c, const SnapshotLoad* loads, int n, int mem) {
    if (c->failed)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_load: an earlier frame of this ctx failed; create a new ctx");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    std::vector<size_t> stage_off((size_t)n, 0);
    size_t stage = 0;
    for (int i = 0; i < n; i++) {
        stage_off[i] = stage;
        stage += align_up((size_t)reinterpret_cast<const SnapHeader*>(loads[i].host.data())->data_bytes, 256);
    }
    if (host && stage > 0)
        if (const int rc = reserve_snap_stage(c, stage)) return rc;
    TileTable table(c);
    std::vector<std::vector<KfDev>> records((size_t)n);      // (read by their uploads until the stream is idle)
    for (int i = 0; i < n; i++) {
        const int s = loads[i].seq;
        end_sequence(c, s);
        const SnapView v = snapshot_view(loads[i].host.data());
        const SnapHeader& h = *v.h;
        if (h.frame_id < 0) continue;            // an empty snapshot: a restart
        Seq& q = c->seqs[s];
        // storage from the free lists: image sets (their own level 0 and right image) and keyframe slabs
        std::vector<ImageSet*> sets((size_t)h.n_image_sets, nullptr);
        for (ImageSet*& is : sets) {
            if (const int rc = acquire_set(c, q, &is)) return rc;
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            is->lk[0] = is->left[0];
            is->refs = 0;
        }
        q.cur_set = sets[0];
        q.cur_set->refs = 1;
        for (int k = 0; k < h.n_keyframes; k++) {
            if (c->kf_slabs.empty())
                if (const int rc = grow_kf_slabs(c, std::max(c->B, 32))) return rc;
            KfHost kf{};
            kf.kps = carve_kps(c->kf_slabs.back(), c->cap);
            c->kf_slabs.pop_back();
            std::memcpy(kf.pose, v.kfs[k].pose, sizeof(kf.pose));
            kf.n = v.kfs[k].n;
            if (v.kfs[k].image_set >= 0) {
                kf.set = sets[v.kfs[k].image_set];
                kf.set->refs++;
            }
            q.kfs.push_back(kf);
        }
        q.kfs_retired = h.keyframes_retired;
        // host state
        std::memcpy(&q.kf, v.filter, sizeof(PoseFilter));
        std::memcpy(&q.ts, v.frame, sizeof(double));
        std::memcpy(q.pose, v.frame + sizeof(double), sizeof(q.pose));
        std::memcpy(&q.stats, v.frame + sizeof(double) + sizeof(q.pose), sizeof(q.stats));
        q.trajectory.assign(v.trajectory, v.trajectory + h.n_trajectory);
        q.frame_id = h.frame_id; q.n_host = h.n_keypoints; q.pending = false;
        // the keyframe table. Template cache: the keyframes a fresh run would hold ring blocks for get theirs with
        // the "stored" flags cleared, the others have none (as after their eviction)
        std::vector<KfDev>& rec = records[i];
        rec.resize((size_t)h.n_keyframes);
        for (int k = 0; k < h.n_keyframes; k++) {
            fill_kf_record(c, q, k, q.kfs[k], rec[k]);
            std::memcpy(rec[k].pose, q.kfs[k].pose, sizeof(rec[k].pose));
            rec[k].n = q.kfs[k].n;
            if (c->tmpl_kf > 0) {
                if (k < h.n_keyframes - c->tmpl_kf) rec[k].tmpl = nullptr;
                else HIP_TRY(hipMemsetAsync(rec[k].tmpl_valid, 0, c->tmpl_valid_bytes, st));
            }
        }
        HIP_TRY(hipMemcpyAsync(q.d_kfs, rec.data(), sizeof(KfDev) * rec.size(), hipMemcpyHostToDevice, st));
        // the data part -> device
        const uint8_t* base = static_cast<const uint8_t*>(loads[i].data);
        if (host && h.data_bytes > 0) {
            HIP_TRY(hipMemcpyAsync(c->d_snap + stage_off[i], loads[i].data, (size_t)h.data_bytes, hipMemcpyHostToDevice, st));
            base = c->d_snap + stage_off[i];
        }
        const std::vector<DevPlane> dev = device_planes(c, q, sets);
        for (size_t j = 0; j < dev.size(); j++) {
            const svo_snapshot_plane& e = v.dir[j];
            if (const int rc = table.add(base + e.offset, dev[j].p, e.row_bytes, e.rows, e.row_bytes, dev[j].pitch)) return rc;
        }
    }
    if (const int rc = table.launch(false)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // loaded: svo_wait means that
    return SVO_OK;
}

extern "C" int svo_snapshot_info(const void* host_part, int64_t bytes, struct svo_snapshot_info* out) {
    std::vector<uint8_t> copy;
    if (const int rc = check_snapshot(host_part, bytes, copy)) return rc;
    if (out) std::memcpy(out, copy.data(), sizeof(*out));
    return SVO_OK;
}

// ------------------------------------------------------------------ per-sequence getters of the C ABI

static int fetch_info(int n, const KpsDev& k, svo_kp2d* kps2d, svo_kp3d* kps3d, svo_kp_info* info) {
    if (n <= 0) return SVO_OK;
    if (kps2d) HIP_TRY(hipMemcpy(kps2d, k.kps2d, sizeof(svo_kp2d) * n, hipMemcpyDeviceToHost));
    if (kps3d) HIP_TRY(hipMemcpy(kps3d, k.kps3d, sizeof(svo_kp3d) * n, hipMemcpyDeviceToHost));
    if (!info) return SVO_OK;
    std::vector<uint32_t> fl(n), col(n);
    std::vector<int> kf(n), ki(n), ou(n), in(n), lt(n);
    std::vector<float> kx(n), kP(n), sc(n);
    const struct { void* dst; const void* src; } arrays[] = {
        {fl.data(), k.flags}, {ou.data(), k.outl}, {in.data(), k.inl}, {kf.data(), k.kf_id}, {ki.data(), k.kp_index},
        {kx.data(), k.kfx}, {kP.data(), k.kfP}, {sc.data(), k.score}, {lt.data(), k.level_type}, {col.data(), k.color}};
    for (const auto& a : arrays) HIP_TRY(hipMemcpy(a.dst, a.src, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));   // (all 4-byte)
    for (int i = 0; i < n; i++) {
        svo_kp_info& o = clear(info[i]);
        o.score = sc[i]; o.level = lt[i] & 0xff; o.type = (lt[i] >> 8) & 0xff;
        o.keyframe_id = kf[i]; o.keypoint_index = ki[i];
        o.color[0] = col[i] & 0xff; o.color[1] = (col[i] >> 8) & 0xff; o.color[2] = (col[i] >> 16) & 0xff;
        o.ignore_during_refinement = (fl[i] & SVO_IGNORE_DURING_REFINEMENT) != 0;
        o.ignore_completely = (fl[i] & SVO_IGNORE_COMPLETELY) != 0;
        o.ignore_temporary = (fl[i] & SVO_IGNORE_TEMPORARY) != 0;
        o.outlier_count = ou[i]; o.inlier_count = in[i];
        o.kf_inv_depth = kx[i]; o.kf_variance = kP[i];
    }
    return SVO_OK;
}

extern "C" int svo_get_pose(svo_ctx* ctx, int seq, float pose[6]) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    flush_pending(c);
    std::memcpy(pose, c->seqs[s].pose, sizeof(float) * 6);
    return SVO_OK;
}

extern "C" int svo_get_frame_keypoints(svo_ctx* ctx, int seq, svo_kp2d* kps2d, svo_kp3d* kps3d,
                                       svo_kp_info* info, int cap, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    const Seq& q = c->seqs[s];
    if (n) *n = q.n_host;
    return fetch_info(std::min(cap, q.n_host), q.kps[q.cur], kps2d, kps3d, info);
}

extern "C" int svo_get_keyframe_count(svo_ctx* ctx, int seq, int* count) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    if (count) *count = (int)c->seqs[s].kfs.size();
    return SVO_OK;
}

extern "C" int svo_get_keyframe(svo_ctx* ctx, int seq, int id, svo_kp2d* kps2d, svo_kp3d* kps3d,
                                svo_kp_info* info, float pose[6], int cap, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    const Seq& q = c->seqs[s];
    if (id < 0 || id >= (int)q.kfs.size()) return svo_set_error(SVO_ERR_INVALID, "keyframe %d does not exist", id);
    const KfHost& k = q.kfs[id];
    if (n) *n = k.n;
    if (pose) std::memcpy(pose, k.pose, sizeof(float) * 6);
    return fetch_info(std::min(cap, k.n), k.kps, kps2d, kps3d, info);
}

extern "C" int svo_get_trajectory(svo_ctx* ctx, int seq, svo_pose* out, int cap, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    flush_pending(c);
    const Seq& q = c->seqs[s];
    if (n) *n = (int)q.trajectory.size();
    const int m = std::min<int>(cap, (int)q.trajectory.size());
    if (out && m > 0) std::memcpy(out, q.trajectory.data(), sizeof(svo_pose) * m);
    return SVO_OK;
}

extern "C" int svo_update_pose(svo_ctx* ctx, int seq, const float pose[6], const float speed[6],
                               const float pose_var[6], const float speed_var[6], double dt,
                               float filtered[6]) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    flush_pending(c);
    c->seqs[s].kf.update(pose, speed, pose_var, speed_var, dt, filtered);
    return SVO_OK;
}

extern "C" int svo_get_frame_stats(svo_ctx* ctx, int seq, svo_frame_stats* out) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    if (out) *out = c->seqs[s].stats;
    return SVO_OK;
}

extern "C" int svo_get_finished_runs(svo_ctx* ctx, int seq, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    if (n) *n = (int)std::count_if(c->finished.begin(), c->finished.end(), [s](const FinishedRun& f) { return f.info.seq == s; });
    return SVO_OK;
}

extern "C" int svo_get_finished_run(svo_ctx* ctx, int seq, int i, svo_run_info* info, svo_pose* trajectory,
                                    int cap, int* n_poses) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    int k = 0;
    for (const FinishedRun& f : c->finished) {
        if (f.info.seq != s || k++ != i) continue;
        if (info) { *info = f.info; info->seq = seq; }
        if (n_poses) *n_poses = (int)f.trajectory.size();
        const int m = std::min<int>(cap, (int)f.trajectory.size());
        if (trajectory && m > 0) std::memcpy(trajectory, f.trajectory.data(), sizeof(svo_pose) * m);
        return SVO_OK;
    }
    return svo_set_error(SVO_ERR_INVALID, "sequence %d has no finished run %d", seq, i);
}
