// svo_group_view.hip — the view job of a sequence group (svo_submit_export_views): the images of the frames or
// newest keyframes of its named slots, as gray planes or as RGB with a marker per keypoint, rendered by view.hip's
// kernel, as segments and pixels; and svo_view_size. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

// cols, rows, pitch and image_bytes of an image of a checked style in a ctx of width x height
void view_shape(int width, int height, const svo_view_style& s, int* cols, int* rows, int64_t* pitch, int64_t* image_bytes) {
    const int level = s.plane == SVO_PLANE_LEFT ? s.level : 0;
    const int w = width >> level, h = height >> level;
    const int64_t p = (int64_t)w * view_params(s).bpp;
    if (cols) *cols = w;
    if (rows) *rows = h;
    if (pitch) *pitch = p;
    if (image_bytes) *image_bytes = (int64_t)align_up((size_t)(p * h), 256);
}

}  // namespace

extern "C" int svo_view_size(const svo_camera_settings* cam, int width, int height, const svo_view_style* style, int* cols,
                             int* rows, int64_t* pitch, int64_t* image_bytes) {
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    if (const int rc = view_check_style(style, cam->max_pyramid_levels, "svo_view_size")) return rc;
    view_shape(width, height, *style, cols, rows, pitch, image_bytes);
    return SVO_OK;
}

int64_t grp_view_bytes(const svo_group* c, const svo_view_style* style) {
    int64_t bytes = 0;
    view_shape(c->width, c->height, *style, nullptr, nullptr, nullptr, &bytes);
    return bytes;
}

int grp_check_view_style(const svo_group* c, const svo_view_style* style) {
    return view_check_style(style, c->cam.max_pyramid_levels, "svo_submit_export_views");
}

// The named slots of the group as segments and images (svo_submit_export_views). Named slot seg[i] of the job goes to
// byte seg[i] * image_bytes of the caller's pixels; in host mode the group renders its i-th named slot at byte
// i * image_bytes of its staging block and copies every run of slots that are consecutive in both (and delivered) out
// with one copy: a plain one where an image fills its image_bytes, else a 2-D one of rows * pitch bytes per slot, so
// that the bytes between two images stay untouched. The tile table goes through the group's argument blocks
// (group_tile_table), one launch unless it outgrows them.
int grp_export_views(svo_group* c, int what, int mem, const int* seqs, const int* seg, int n, int seq0,
                     const svo_view_style* style, const svo_view_dst* dst) {
    if (const int rc = job_begin(c, "svo_submit_export_views")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    int cols, rows; int64_t pitch, image_bytes;
    view_shape(c->width, c->height, *style, &cols, &rows, &pitch, &image_bytes);
    const int64_t used = (int64_t)rows * pitch;          // bytes of an image
    if (host)
        if (const int rc = c->d_view.reserve(c, (size_t)n * (size_t)image_bytes)) return rc;
    const ViewParams params = view_params(*style);
    // (SVO_VIEW_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    auto table = group_tile_table<ViewTile>(c, "SVO_VIEW_TABLE_TILES",
                                            [&](const ViewTile* d, int m, hipStream_t s) { launch_view(d, m, params, s); });
    std::vector<ViewTile> tiles;
    std::vector<char> shown((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_view_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.keyframe_id = -1;
        e.time_stamp = (float)q.ts; e.offset = (int64_t)seg[i] * image_bytes; e.status = SVO_VIEW_NONE;
        const ImageSet* set = nullptr;
        const KpsDev* kps = nullptr;
        if (what == SVO_EXPORT_FRAMES) {
            e.n = q.n_host;
            std::memcpy(e.pose, q.pose, sizeof(e.pose));
            if (q.frame_id >= 0) { set = q.cur_set; kps = &q.kps[q.cur]; }
        } else if (!q.kfs.empty()) {
            const KfHost& k = q.kfs.back();
            e.keyframe_id = (int)q.kfs.size() - 1;
            e.n = k.n;
            std::memcpy(e.pose, k.pose, sizeof(e.pose));
            set = k.set; kps = &k.kps;
        }
        if (!set) continue;
        const ImgView& src = style->plane == SVO_PLANE_LEFT ? set->left[style->level] : set->right;
        if (src.w != cols || src.h != rows)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_views: level %d is %d x %d, not %d x %d", style->level, src.w, src.h, cols, rows);
        e.status = SVO_VIEW_OK;
        shown[i] = 1;
        uint8_t* out = host ? c->d_view.p + (int64_t)i * image_bytes : dst->pixels + e.offset;
        tiles.clear();
        view_tiles(src, out, style->markers ? kps : nullptr, e.n, tiles);
        for (const ViewTile& t : tiles)
            if (const int rc = table.add(t)) return rc;
    }
    if (const int rc = table.launch(false)) return rc;
    if (host)
        if (const int rc = copy_out_slots(st, dst->pixels, c->d_view.p, seg, shown.data(), n, image_bytes, used)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}
