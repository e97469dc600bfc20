// svo_group.hip — one group of the tracker behind the C ABI: StereoSlam::new_image
// (src/lib/stereo_slam.cpp:123-271) for B sequences together, one kernel launch per stage, on the
// group's own stream. This unit owns the group's storage (device allocations, image-set and keyframe-slab pools),
// its sizing and creation, its settings, the deferred pose-filter update and the end of a sequence. The step is in
// svo_group_step.hip, the bulk export in svo_group_export.hip, snapshots in svo_group_snapshot.hip; the state they
// share is svo_group_state.hpp. The layer above spreads a ctx's sequences over groups, through svo_group.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "svo_group_state.hpp"

using namespace svo;

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

// (static: local to this unit; the rest is declared in svo_group_state.hpp)
namespace svo {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// gives an allocation of dev_alloc back
void dev_release(svo_group* c, void* p, size_t bytes) {
    for (auto it = c->dev_mem.begin(); it != c->dev_mem.end(); ++it)
        if (it->get() == p) {
            c->dev_mem.erase(it);
            c->device_bytes -= bytes;
            return;
        }
}

// a plain copy where a slot fills its image_bytes, a short one for a lone slot, else a 2-D one of `used` bytes per slot
int copy_out_slots(hipStream_t st, uint8_t* to, const uint8_t* from, const int* seg, const char* shown, int n, int64_t image_bytes,
                   int64_t used) {
    for (int i = 0; i < n;) {
        if (!shown[i]) { i++; continue; }
        int j = i + 1;
        while (j < n && shown[j] && seg[j] == seg[j - 1] + 1) j++;
        uint8_t* dst = to + (int64_t)seg[i] * image_bytes;
        const uint8_t* src = from + (int64_t)i * image_bytes;
        if (used == image_bytes)
            HIP_TRY(hipMemcpyAsync(dst, src, (size_t)((j - i) * image_bytes), hipMemcpyDeviceToHost, st));
        else if (j - i == 1)
            HIP_TRY(hipMemcpyAsync(dst, src, (size_t)used, hipMemcpyDeviceToHost, st));
        else
            HIP_TRY(hipMemcpy2DAsync(dst, (size_t)image_bytes, src, (size_t)image_bytes, (size_t)used, (size_t)(j - i), hipMemcpyDeviceToHost, st));
        i = j;
    }
    return SVO_OK;
}

int reject_if_failed(const svo_group* c, const char* who) {
    return c->failed ? svo_set_error(SVO_ERR_INVALID, "%s: an earlier frame of this ctx failed; create a new ctx", who) : SVO_OK;
}

int job_begin(svo_group* c, const char* who) {
    if (const int rc = reject_if_failed(c, who)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    flush_pending(c);
    return SVO_OK;
}

// ------------------------------------------------------------------------------------ storage

// Image-set storage comes from slabs allocated in chunks: one hipMalloc (a device-wide
// synchronising call) per chunk of sets, not per set — every keyframe keeps its set for good, so a
// long run asks for one per keyframe.
static int grow_set_slabs(svo_group* c, int count) {
    uint8_t* base = nullptr;
    const int rc = dev_alloc(c, &base, c->set_layout.bytes * (size_t)count, false);
    if (rc) return rc;
    for (int i = count - 1; i >= 0; i--) c->set_slabs.push_back(base + c->set_layout.bytes * (size_t)i);
    return SVO_OK;
}

static SetLayout image_set_layout(const svo_group* c) {
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
static int new_image_set(svo_group* c, Seq& q) {
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
static int alloc_kps(svo_group* c, KpsDev& k, int* n_ptr) {
    int rc = SVO_OK;
    auto alloc = [&](auto** p) { if (!rc) rc = dev_alloc(c, p, (size_t)c->cap); };
    alloc(&k.kps2d); alloc(&k.kps3d); alloc(&k.flags); alloc(&k.kf_id); alloc(&k.kp_index); alloc(&k.outl);
    alloc(&k.inl); alloc(&k.kfx); alloc(&k.kfP); alloc(&k.score); alloc(&k.level_type); alloc(&k.color);
    k.n = n_ptr;
    return rc;
}

// per-keyframe keypoint storage: 15 dwords per keypoint. Slabs come from chunks of `count`
// (one hipMalloc — a device-wide synchronising call — per chunk, not per keyframe).
static size_t kf_slab_bytes(const svo_group* c) { return align_up((size_t)c->cap * 15 * 4, 256); }

static int grow_kf_slabs(svo_group* c, int count) {
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
static KpsDev carve_kps(uint8_t* base, size_t cap) {
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

// the keypoint arrays of one more keyframe: a slab off the free list, which grows by a chunk when it is empty
int take_kf_slab(svo_group* c, KpsDev* out) {
    if (c->kf_slabs.empty()) {
        const int rc = grow_kf_slabs(c, std::max(c->B, 32));
        if (rc) return rc;
    }
    *out = carve_kps(c->kf_slabs.back(), c->cap);
    c->kf_slabs.pop_back();
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


// capacities and level counts that follow from the settings
static void size_group(svo_group* c) {
    const svo_camera_settings& cam = c->cam;
    const int width = c->width, height = c->height;
    c->cap = keypoint_capacity(cam, width, height);
    c->rec_cap = (int)align_up((size_t)c->cap, 512);   // whole passes of the widest alignment workgroup
    // the keyframe table of a sequence: a ring, so a power of two. SVO_KEYFRAME_TABLE (4 .. MAX_KEYFRAMES) is a
    // diagnostic: tests reach the table's end in seconds with it. Anything else: the default.
    c->max_kf = MAX_KEYFRAMES;
    if (const char* e = std::getenv("SVO_KEYFRAME_TABLE")) {
        const int t = std::atoi(e);
        if (t >= 4 && t <= MAX_KEYFRAMES && (t & (t - 1)) == 0) c->max_kf = t;
    }
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
static int alloc_blocks(svo_group* c) {
    ArgBlocks& a = c->args;
    const size_t B = c->B;
    size_t off = 0;
    auto size = [&](auto& arr) { off += align_up(sizeof(typename std::decay_t<decltype(arr)>::type) * B, 256); };
    a.frame_arrays(size);
    a.frame_bytes = off;                  // everything a tracked frame uploads; the rest is keyframe-only ...
    a.rig_arrays(size);
    a.frame_rig_bytes = off;              // ... but for the chunk table of a step whose slots remap through different maps
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
    a.rig_arrays(place);
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

static int alloc_sequence(svo_group* c, Seq& q, int s) {
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
static int alloc_template_cache(svo_group* c) {
    const int B = c->B;
    const int cells = (c->width / c->cam.grid_width) * (c->height / c->cam.grid_height);
    c->tmpl_cap = std::min(c->cap, cells + 64);
    c->tmpl_block_bytes = align_up((size_t)c->tmpl_cap * SVO_LK_LEVELS * klt_template_bytes(c->cam.window_size_opt_flow), 256);
    int K = c->tmpl_block_bytes <= ((size_t)8 << 20) ? 8 : 4;
    if (const char* e = std::getenv("SVO_KLT_CACHE_KF")) K = std::max(0, std::min(std::atoi(e), 64));
    c->tmpl_valid_bytes = kf_tmpl_valid_bytes(c->tmpl_cap);
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

// a pinned table of n entries and its device mirror; a failure leaves `table` and `host` as they were
template <typename T>
static int alloc_mirrored_table(svo_group* c, ArgArray<T>& table, PinnedPtr<T>& host, size_t n) {
    PinnedPtr<T> pinned;
    HIP_TRY(pinned_malloc(pinned, sizeof(T) * n));
    T* dev = nullptr;
    if (const int rc = dev_alloc(c, &dev, n)) return rc;
    host = std::move(pinned);
    table.h = host.get();
    table.d = dev;
    return SVO_OK;
}

}  // namespace svo

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
    for (Seq& q : c->seqs) q.cam = c->cam;                      // (rig 0)
    if ((rc = grow_set_slabs(c, 4 * n_sequences))) return rc;   // the first four image sets of every sequence: one allocation
    for (int s = 0; s < n_sequences; s++)
        if ((rc = alloc_sequence(c, c->seqs[s], s))) return rc;
    if ((rc = grow_kf_slabs(c, std::max(2 * n_sequences, 32)))) return rc;   // the first keyframes never allocate
    if ((rc = alloc_template_cache(c))) return rc;
    if ((rc = alloc_mirrored_table(c, c->remap_img, c->remap_img_host, 2 * (size_t)n_sequences))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = std::move(g);
    return SVO_OK;
}

void grp_set_exact_pinv(svo_group* c, int on) { c->exact_pinv = on != 0; }
void grp_set_rectification(svo_group* c, const RemapMap* maps) { c->rect = maps; }
void grp_enable_timing(svo_group* c, int on) { c->timing = on != 0; }

int grp_set_input_format(svo_group* c, int format) {
    if (converts(format) && !c->ingest_img.d) {
        HIP_TRY(hipSetDevice(c->device));
        if (const int rc = alloc_mirrored_table(c, c->ingest_img, c->ingest_img_host, 2 * (size_t)c->B)) return rc;
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

namespace svo {

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

// ------------------------------------------------------------------ the end of a sequence

// The sequence of the slot ends (between two steps of the group: its stream is idle). Its image sets and
// keyframe keypoint slabs go back to their free lists, its host state becomes that of a fresh ctx, and a host
// record of the run stays. Nothing is cleared on the device: the slot's next frame is frame 0 of a new
// sequence, whose kernels reset what they read (compact_kernel: keypoint counts and result block,
// kf_init_kernel: colour generator, table record and "stored" flags of keyframe 0). Records and template-cache
// blocks of the old run's keyframes stay behind in the table, but a keypoint only refers to a keyframe id that
// its own run has created, and creating it rewrites both.
// (Trimmed keyframes gave their slabs back when they went: the resident ones are all that is left to free.)
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

// The slot's keyframes below min(below, kfs_retired) go (between two steps of the group): host bookkeeping only. Such
// a keyframe is retired, so no keypoint of the frame originates from it, neither the tracker nor the depth filter reads
// or writes it again and its image set is back already; its keypoint slab returns to the free list, its host entry
// goes, and its record stays behind in the table ring until a new keyframe takes the slot.
void trim_keyframes(svo_group* c, Seq& q, int below) {
    const int to = std::min(below, q.kfs_retired);
    if (to <= q.kfs.first()) return;
    for (int id = q.kfs.first(); id < to; id++) {
        KfHost& k = q.kfs[(size_t)id];
        release_set(q, k.set);               // (null already)
        c->kf_slabs.push_back(reinterpret_cast<uint8_t*>(k.kps.kps3d));
    }
    q.kfs.drop_below(to);
}

}  // namespace svo

int grp_trim_keyframes(svo_group* c, const int* seqs, const int* below, int n) {
    if (const int rc = reject_if_failed(c, "svo_submit_trim_keyframes")) return rc;
    for (int i = 0; i < n; i++) trim_keyframes(c, c->seqs[seqs[i]], below[i]);
    return SVO_OK;
}

void grp_set_keyframe_window(svo_group* c, int keep) { c->kf_window = keep; }

svo_keyframe_range grp_keyframe_range(const svo_group* c, int seq) {
    const Seq& q = c->seqs[seq];
    return svo_keyframe_range{q.kfs.first(), q.kfs_retired, (int)q.kfs.size(), c->max_kf};
}

int grp_restart_sequences(svo_group* c, const int* seqs, int n) {
    if (const int rc = reject_if_failed(c, "svo_ctx_restart_sequences")) return rc;
    for (int i = 0; i < n; i++) end_sequence(c, seqs[i]);
    return SVO_OK;
}

int grp_assign_rigs(svo_group* c, const int* seqs, const RigBinding* b, int n) {
    if (const int rc = reject_if_failed(c, "svo_ctx_assign_rigs")) return rc;
    for (int i = 0; i < n; i++) {
        end_sequence(c, seqs[i]);
        Seq& q = c->seqs[seqs[i]];
        q.rig = b[i].rig; q.cam = b[i].cam;
        q.rig_maps[0] = b[i].rig ? b[i].maps[0] : nullptr;
        q.rig_maps[1] = b[i].rig ? b[i].maps[1] : nullptr;
    }
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
