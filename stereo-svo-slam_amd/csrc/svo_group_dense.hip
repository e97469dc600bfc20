// svo_group_dense.hip — the disparity job of a sequence group (svo_submit_export_disparity): dense disparity or depth
// maps of the frames or newest keyframes of its named slots, computed by dense.hip's kernel from the left level-0
// plane and the right image of each slot, as segments and float planes; and svo_disparity_size. The state is
// svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

// the style is checked and the ctx's size has a lattice point at its step
int check_style(const svo_camera_settings* cam, int width, int height, const svo_disparity_style* style, const char* who, DenseParams* out) {
    DenseParams p;
    if (const int rc = dense_check_style(style, cam, who, &p)) return rc;
    if (width / p.step < 1 || height / p.step < 1)
        return svo_set_error(SVO_ERR_INVALID, "%s: %d x %d has no lattice point at step %d", who, width, height, p.step);
    if (out) *out = p;
    return SVO_OK;
}

}  // namespace

extern "C" int svo_disparity_size(const svo_camera_settings* cam, int width, int height, const svo_disparity_style* style,
                                  int* cols, int* rows, int* planes, int64_t* image_bytes) {
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    DenseParams p;
    if (const int rc = check_style(cam, width, height, style, "svo_disparity_size", &p)) return rc;
    dense_shape(p, width, height, cols, rows, planes, image_bytes);
    return SVO_OK;
}

int grp_check_disparity_style(const svo_group* c, const svo_disparity_style* style) {
    return check_style(&c->cam, c->width, c->height, style, "svo_submit_export_disparity", nullptr);
}

int64_t grp_disparity_bytes(const svo_group* c, const svo_disparity_style* style) {
    DenseParams p;
    int64_t bytes = 0;
    if (dense_check_style(style, &c->cam, "svo_submit_export_disparity", &p) == SVO_OK) dense_shape(p, c->width, c->height, nullptr, nullptr, nullptr, &bytes);
    return bytes;
}

// The named slots of the group as segments and planes (svo_submit_export_disparity). Named slot seg[i] of the job goes
// to byte seg[i] * image_bytes of the caller's values; in host mode the group computes its i-th named slot at byte
// i * image_bytes of its staging block and copies every run of slots that are consecutive in both (and delivered) out
// with one copy: a plain one where the planes fill their image_bytes, else a 2-D one of the planes' bytes per slot, so
// that the bytes between two slots stay untouched. The image table (one entry per delivered slot) goes through the
// group's argument blocks, one launch unless it outgrows them.
int grp_export_disparity(svo_group* c, int what, int mem, const int* seqs, const int* seg, int n, int seq0,
                         const svo_disparity_style* style, const svo_disparity_dst* dst) {
    if (const int rc = job_begin(c, "svo_submit_export_disparity")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    DenseParams params;
    if (const int rc = dense_check_style(style, &c->cam, "svo_submit_export_disparity", &params)) return rc;
    int cols, rows, planes; int64_t image_bytes;
    dense_shape(params, c->width, c->height, &cols, &rows, &planes, &image_bytes);
    const int64_t used = (int64_t)planes * cols * rows * 4;   // bytes of a slot's planes
    int tiles = dense_tiles(params, c->width, c->height);
    if (host)
        if (const int rc = c->d_dense.reserve(c, (size_t)n * (size_t)image_bytes)) return rc;
    // (SVO_DENSE_TABLE_IMAGES: a smaller table, so that tests reach the chunked launches)
    auto table = group_tile_table<DenseImage>(c, "SVO_DENSE_TABLE_IMAGES",
                                              [&](const DenseImage* d, int m, hipStream_t s) { launch_dense(d, m, tiles, params, s); });
    table.cap = std::min(table.cap, DENSE_MAX_IMAGES);
    std::vector<char> shown((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_disparity_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.keyframe_id = -1;
        e.time_stamp = (float)q.ts; e.offset = (int64_t)seg[i] * image_bytes; e.status = SVO_DISPARITY_NONE;
        e.baseline = q.cam.baseline;
        const ImageSet* set = nullptr;
        if (what == SVO_EXPORT_FRAMES) {
            std::memcpy(e.pose, q.pose, sizeof(e.pose));
            if (q.frame_id >= 0) set = q.cur_set;
        } else if (!q.kfs.empty()) {
            const KfHost& k = q.kfs.back();
            e.keyframe_id = (int)q.kfs.size() - 1;
            std::memcpy(e.pose, k.pose, sizeof(e.pose));
            set = k.set;
        }
        if (!set) continue;
        const ImgView& l = set->left[0];
        const ImgView& r = set->right;
        if (l.w != c->width || l.h != c->height || r.w != l.w || r.h != l.h)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: the planes are %d x %d and %d x %d, not %d x %d", l.w, l.h, r.w, r.h,
                                 c->width, c->height);
        e.status = SVO_DISPARITY_OK;
        shown[i] = 1;
        uint8_t* out = host ? c->d_dense.p + (int64_t)i * image_bytes : reinterpret_cast<uint8_t*>(dst->values) + e.offset;
        if (const int rc = table.add(DenseImage{l.data, r.data, reinterpret_cast<float*>(out), l.stride, r.stride, l.w, l.h, q.cam.baseline, 0}))
            return rc;
    }
    if (table.m == (size_t)std::count(shown.begin(), shown.end(), 1)) {   // (one launch: sized by what it holds)
        dense_plan(params, (long long)tiles * (long long)table.m);
        tiles = dense_tiles(params, c->width, c->height);
    }
    if (const int rc = table.launch(false)) return rc;
    if (host)
        if (const int rc = copy_out_slots(st, reinterpret_cast<uint8_t*>(dst->values), c->d_dense.p, seg, shown.data(), n, image_bytes, used)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}
