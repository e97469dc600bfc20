// svo_capi_tables.hip — the stage-level entries that take many images, sets or segments and build a table for one
// launch: rectification and remap, frame ingest, keypoint and map export, the viewer's images and scenes, the AR picture,
// dense disparity maps and point clouds, segment copies, the pose filter. Every entry keeps a grow-only workspace of its own in the handle (svo_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "svo_handle.hpp"

using namespace svo;

// Every tile through a table of `chunk` tiles at `dev`, run(dev, tiles, stream) per chunk. Waits for the stream on
// every path (the uploads read host memory of this call); the first error.
template <typename Tile, typename Launch>
static int launch_tiles(svo_handle* h, const std::vector<Tile>& tiles, Tile* dev, size_t chunk, Launch run) {
    std::vector<Tile> host(chunk);
    TileTable table{host.data(), dev, chunk, h->stream, run};
    int rc = SVO_OK;
    for (const Tile& t : tiles)
        if ((rc = table.add(t))) break;
    if (!rc) rc = table.launch(false);
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    HIP_TRY(e);
    return SVO_OK;
}

extern "C" int svo_remap_linear(svo_handle* h, int n, const svo_image* src, svo_image* dst, const float* map_x,
                                const float* map_y) {
    CHECK_H(h);
    if (n < 1 || !src || !dst || !map_x || !map_y)
        return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear: bad arguments");
    const int w = dst[0].width, hgt = dst[0].height;
    if (w < 1 || hgt < 1) return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear: empty map");
    for (int i = 0; i < n; i++) {
        if (!src[i].data || !dst[i].data || dst[i].width != w || dst[i].height != hgt || dst[i].stride < w)
            return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear: image %d: every dst is the map's size", i);
        if (src[i].width < 1 || src[i].height < 1 || src[i].width > REMAP_MAX_SRC || src[i].height > REMAP_MAX_SRC ||
            src[i].stride < src[i].width)
            return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear: image %d: source of 1..%d pixels a side", i, REMAP_MAX_SRC);
    }
    const size_t map_bytes = remap_map_bytes(w, hgt);
    const size_t need = map_bytes + sizeof(RemapImg) * (size_t)n;
    if (const int rc = h->remap_ws.reserve(need, h->stream)) return rc;
    std::vector<RemapImg> imgs(n);
    for (int i = 0; i < n; i++) imgs[i] = RemapImg{make_view(src[i]), make_view(dst[i])};
    RemapImg* d_img = reinterpret_cast<RemapImg*>(h->remap_ws.ptr.get() + map_bytes);
    HIP_TRY(hipMemcpyAsync(d_img, imgs.data(), sizeof(RemapImg) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    RemapLaunch a;
    std::memset(&a, 0, sizeof(a));
    a.map[0] = a.map[1] = remap_map_view(h->remap_ws.ptr.get(), w, hgt);
    launch_remap_prep(map_x, map_y, a.map[0], h->stream);
    HIP_TRY(hipGetLastError());
    a.img = d_img;
    a.n = n;
    launch_remap(a, 1, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_rectify_inverse(const svo_camera_calibration* cal, double ir[9]) {
    if (!cal || !ir) return svo_set_error(SVO_ERR_INVALID, "svo_rectify_inverse: bad arguments");
    if (!rectify_inverse(*cal, ir))
        return svo_set_error(SVO_ERR_INVALID, "svo_rectify_inverse: a value is not finite, or P R has no inverse");
    return SVO_OK;
}

extern "C" int svo_build_rectify_maps(svo_handle* h, int n, const svo_camera_calibration* cal, int width, int height,
                                      float* const* map_x, float* const* map_y) {
    CHECK_H(h);
    if (n < 0 || width < 1 || height < 1 || (n > 0 && (!cal || !map_x || !map_y)))
        return svo_set_error(SVO_ERR_INVALID, "svo_build_rectify_maps: bad arguments");
    const long long tiles = (long long)((width + REMAP_TILE - 1) / REMAP_TILE) * ((height + REMAP_TILE - 1) / REMAP_TILE);
    if (tiles * n >= RIG_MAX_WORKGROUPS)
        return svo_set_error(SVO_ERR_INVALID, "svo_build_rectify_maps: %d cameras of %d x %d are too many for one call", n, width, height);
    std::vector<RigCam> cams((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!map_x[i] || !map_y[i]) return svo_set_error(SVO_ERR_INVALID, "svo_build_rectify_maps: camera %d: a plane is NULL", i);
        if (!rig_camera(cal[i], cams[i]))
            return svo_set_error(SVO_ERR_INVALID, "svo_build_rectify_maps: camera %d: a value is not finite, or P R has no inverse", i);
        cams[i].map_x = map_x[i];
        cams[i].map_y = map_y[i];
    }
    if (n == 0) return SVO_OK;
    if (const int rc = h->rigcam_ws.reserve(sizeof(RigCam) * (size_t)n, h->stream)) return rc;
    RigCam* d_cams = reinterpret_cast<RigCam*>(h->rigcam_ws.ptr.get());
    HIP_TRY(hipMemcpyAsync(d_cams, cams.data(), sizeof(RigCam) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    launch_rig_maps(d_cams, n, width, height, false, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_remap_linear_multi(svo_handle* h, int n, const svo_image* src, svo_image* dst, int n_maps,
                                      const float* const* map_x, const float* const* map_y, const int* map_of_image) {
    CHECK_H(h);
    if (n < 1 || n_maps < 1 || !src || !dst || !map_x || !map_y || !map_of_image)
        return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: bad arguments");
    const int w = dst[0].width, hgt = dst[0].height;
    if (w < 1 || hgt < 1) return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: empty map");
    for (int m = 0; m < n_maps; m++)
        if (!map_x[m] || !map_y[m]) return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: map %d is NULL", m);
    for (int i = 0; i < n; i++) {
        if (map_of_image[i] < 0 || map_of_image[i] >= n_maps)
            return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: image %d: map %d of %d", i, map_of_image[i], n_maps);
        if (!src[i].data || !dst[i].data || dst[i].width != w || dst[i].height != hgt || dst[i].stride < w)
            return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: image %d: every dst is the maps' size", i);
        if (src[i].width < 1 || src[i].height < 1 || src[i].width > REMAP_MAX_SRC || src[i].height > REMAP_MAX_SRC ||
            src[i].stride < src[i].width)
            return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: image %d: source of 1..%d pixels a side", i, REMAP_MAX_SRC);
    }
    // the images in map order, and the chunks of that order
    std::vector<int> order;
    std::vector<RemapChunkSpan> spans;
    const int longest = remap_chunks(map_of_image, n, order, spans);
    if (spans.size() > 65535) return svo_set_error(SVO_ERR_INVALID, "svo_remap_linear_multi: more than 65535 chunks in one call");
    // workspace: the maps that have an image, in the kernels' form | image table | chunk table
    std::vector<int> slot_of_map((size_t)n_maps, -1);
    int used = 0;
    for (const RemapChunkSpan& c : spans)
        if (slot_of_map[c.map] < 0) slot_of_map[c.map] = used++;
    const size_t map_bytes = remap_map_bytes(w, hgt);
    const size_t img_bytes = (sizeof(RemapImg) * (size_t)n + 255) / 256 * 256;
    const size_t need = map_bytes * used + img_bytes + sizeof(RemapChunk) * spans.size();
    if (const int rc = h->remap_ws.reserve(need, h->stream)) return rc;
    uint8_t* ws = h->remap_ws.ptr.get();
    std::vector<RemapImg> imgs((size_t)n);
    for (int k = 0; k < n; k++) imgs[k] = RemapImg{make_view(src[order[k]]), make_view(dst[order[k]])};
    std::vector<RemapChunk> chunks(spans.size());
    for (size_t k = 0; k < spans.size(); k++) {
        const uint8_t* base = ws + map_bytes * slot_of_map[spans[k].map];
        chunks[k] = RemapChunk{{base, base}, spans[k].first, spans[k].count};
    }
    RemapImg* d_img = reinterpret_cast<RemapImg*>(ws + map_bytes * used);
    RemapChunk* d_chunks = reinterpret_cast<RemapChunk*>(ws + map_bytes * used + img_bytes);
    HIP_TRY(hipMemcpyAsync(d_img, imgs.data(), sizeof(RemapImg) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(RemapChunk) * chunks.size(), hipMemcpyHostToDevice, h->stream));
    for (int m = 0; m < n_maps; m++) {
        if (slot_of_map[m] < 0) continue;
        launch_remap_prep(map_x[m], map_y[m], remap_map_view(ws + map_bytes * slot_of_map[m], w, hgt), h->stream);
        HIP_TRY(hipGetLastError());
    }
    RemapMultiLaunch a;
    std::memset(&a, 0, sizeof(a));
    a.chunks = d_chunks; a.img = d_img; a.n = n;
    launch_remap_multi(a, w, hgt, (int)chunks.size(), longest == 1, 1, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_input_format_info(int format, int width, svo_input_layout* out) {
    const IngestFormat* f = ingest_format(format);
    if (!f || width < 1 || !out) return svo_set_error(SVO_ERR_INVALID, "svo_input_format_info: unknown format %d, width %d", format, width);
    std::memset(out, 0, sizeof(*out));
    out->buffers = f->buffers; out->channels = f->channels; out->min_row_pixels = ingest_row_pixels(*f, width);
    const IngestSide* sides[2] = {&f->left, &f->right};
    svo_input_side* outs[2] = {&out->left, &out->right};
    for (int i = 0; i < 2; i++) {
        outs[i]->buffer = sides[i]->buffer; outs[i]->start_column = sides[i]->start * width;
        outs[i]->op = sides[i]->op; outs[i]->channel = sides[i]->channel;
        for (int k = 0; k < 3; k++) outs[i]->weight[k] = sides[i]->weight[k];
    }
    return SVO_OK;
}

extern "C" int svo_convert_frames(svo_handle* h, int format, int n, const svo_image* src_a, const svo_image* src_b,
                                  svo_image* left, svo_image* right) {
    CHECK_H(h);
    const IngestFormat* f = ingest_format(format);
    if (!f || n < 1 || !src_a || !left || !right || (f->buffers == 2 && !src_b))
        return svo_set_error(SVO_ERR_INVALID, "svo_convert_frames: bad arguments");
    const int w = left[0].width, hgt = left[0].height;
    if (w < 1 || hgt < 1) return svo_set_error(SVO_ERR_INVALID, "svo_convert_frames: empty output");
    const int row_px = ingest_row_pixels(*f, w);
    if ((long long)row_px * f->channels > INT_MAX) return svo_set_error(SVO_ERR_INVALID, "svo_convert_frames: row too long");
    for (int i = 0; i < n; i++) {
        for (const svo_image* d : {&left[i], &right[i]})
            if (!d->data || d->width != w || d->height != hgt || d->stride < w)
                return svo_set_error(SVO_ERR_INVALID, "svo_convert_frames: image %d: every output has the size of left[0]", i);
        for (int b = 0; b < f->buffers; b++) {
            const svo_image& s = b ? src_b[i] : src_a[i];
            if (!s.data || s.width < row_px || s.height < hgt || (long long)s.stride < (long long)s.width * f->channels)
                return svo_set_error(SVO_ERR_INVALID, "svo_convert_frames: image %d: a source of at least %d x %d pixels, stride >= its row", i, row_px, hgt);
        }
    }
    if (const int rc = h->ingest_ws.reserve(sizeof(IngestImg) * 2 * (size_t)n, h->stream)) return rc;
    IngestImg* d_imgs = reinterpret_cast<IngestImg*>(h->ingest_ws.ptr.get());
    std::vector<IngestImg> imgs((size_t)2 * n);
    for (int i = 0; i < n; i++)
        for (int side = 0; side < 2; side++) {
            const svo_image& s = (side ? f->right : f->left).buffer ? src_b[i] : src_a[i];
            imgs[(size_t)side * n + i] = ingest_image(*f, side, s.data, s.stride, make_view(side ? right[i] : left[i]));
        }
    HIP_TRY(hipMemcpyAsync(d_imgs, imgs.data(), sizeof(IngestImg) * imgs.size(), hipMemcpyHostToDevice, h->stream));
    const int total = 2 * n, per_launch = 32768;
    for (int i0 = 0; i0 < total; i0 += per_launch) {
        launch_ingest(d_imgs + i0, std::min(per_launch, total - i0), w, hgt, h->stream);
        HIP_TRY(hipGetLastError());
    }
    return SVO_OK;
}

extern "C" int svo_pack_keypoints(svo_handle* h, int n_sets, const svo_keypoints* sets, const int64_t* first,
                                  svo_kp2d* kps2d, svo_kp3d* kps3d, svo_kp_info* info) {
    CHECK_H(h);
    if (n_sets < 0 || (n_sets > 0 && (!sets || !first)))
        return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: bad arguments");
    for (const void* p : {(const void*)kps2d, (const void*)kps3d, (const void*)info})
        if ((uintptr_t)p & 3) return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: an output array is not 4-byte aligned");
    std::vector<ExportTile> tiles;
    for (int i = 0; i < n_sets; i++) {
        const svo_keypoints& k = sets[i];
        if (k.n < 0 || first[i] < 0) return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: set %d: n and first must be >= 0", i);
        if (k.n == 0) continue;
        KpsDev d;
        if (!take_planes(k, KP_ALL, true, d))
            return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: set %d: every array is device memory, 4-byte aligned", i);
        for (int start = 0; start < k.n; start += EXPORT_TILE)
            tiles.push_back(export_tile(d, start, std::min(EXPORT_TILE, k.n - start), first[i]));
    }
    if (tiles.empty() || (!kps2d && !kps3d && !info)) return SVO_OK;
    if (tiles.size() > (size_t)INT_MAX) return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: too many keypoints");
    if (const int rc = h->export_ws.reserve(sizeof(ExportTile) * tiles.size(), h->stream)) return rc;
    ExportTile* d_tiles = reinterpret_cast<ExportTile*>(h->export_ws.ptr.get());
    HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(ExportTile) * tiles.size(), hipMemcpyHostToDevice, h->stream));
    launch_export(d_tiles, (int)tiles.size(), kps2d, kps3d, info, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_pack_map_points(svo_handle* h, int n_regions, const int32_t* set_begin, const svo_keypoints* sets,
                                   const int32_t* own_id, const int64_t* first, const svo_map_filter* filter,
                                   svo_map_point* points, int32_t* counts) {
    CHECK_H(h);
    if (n_regions < 0 || (n_regions > 0 && (!set_begin || !first || set_begin[0] != 0)))
        return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: bad arguments");
    const svo_map_filter f = filter ? *filter : svo_map_filter{0, 0, 0, 0};
    if ((f.drop_flags & ~(uint32_t)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY)) || f._reserved != 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: drop_flags 0x%x has unknown bits, or _reserved is not 0", f.drop_flags);
    if (((uintptr_t)points & 15) || ((uintptr_t)counts & 3))
        return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: points must be 16-byte aligned, counts 4-byte");
    std::vector<MapTile> tiles;
    for (int r = 0; r < n_regions; r++) {
        if (set_begin[r + 1] < set_begin[r] || first[r] < 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: region %d: set_begin must ascend, first must be >= 0", r);
        if (set_begin[r + 1] > set_begin[r] && (!sets || !own_id)) return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: no sets");
        const int region_tile = (int)tiles.size();
        for (int s = set_begin[r]; s < set_begin[r + 1]; s++) {
            const svo_keypoints& k = sets[s];
            if (k.n < 0) return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: set %d: n must be >= 0", s);
            KpsDev d;
            if (!take_planes(k, KP_MAP, k.n > 0, d))
                return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: set %d: kps3d, flags, keyframe_id, inlier_count and color are device memory, 4-byte aligned", s);
            map_tiles(d, k.n, own_id[s], s, first[r], region_tile, tiles);
            if (tiles.size() > (size_t)INT_MAX / 2) return svo_set_error(SVO_ERR_INVALID, "svo_pack_map_points: too many keypoints");
        }
    }
    if (tiles.empty() || (!points && !counts)) return SVO_OK;
    // (SVO_MAP_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_MAP_TABLE_TILES", tiles.size());
    const size_t counts_bytes = (sizeof(int) * tiles.size() + 15) / 16 * 16;
    const size_t bytes = counts_bytes + sizeof(MapTile) * chunk;
    if (const int rc = h->map_ws.reserve(bytes, h->stream)) return rc;
    int* tile_counts = reinterpret_cast<int*>(h->map_ws.ptr.get());
    return launch_tiles(h, tiles, reinterpret_cast<MapTile*>(h->map_ws.ptr.get() + counts_bytes), chunk,
                        [&](const MapTile* d, int m, hipStream_t s) { launch_map(d, m, f, points, tile_counts, counts, s); });
}

extern "C" int svo_render_views(svo_handle* h, int n, const svo_view_src* src, const int64_t* offset, const svo_view_style* style,
                                uint8_t* pixels) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !offset))) return svo_set_error(SVO_ERR_INVALID, "svo_render_views: bad arguments");
    if (const int rc = view_check_style(style, SVO_MAX_PYRAMID_LEVELS, "svo_render_views")) return rc;
    if (!pixels || ((uintptr_t)pixels & 3)) return svo_set_error(SVO_ERR_INVALID, "svo_render_views: pixels is NULL or not 4-byte aligned");
    std::vector<ViewTile> tiles;
    for (int i = 0; i < n; i++) {
        const svo_image& im = src[i].image;
        const svo_keypoints& k = src[i].kps;
        if (!im.data || im.width < 1 || im.height < 1 || im.stride < im.width || im.width > (1 << 15) || im.height > (1 << 15))
            return svo_set_error(SVO_ERR_INVALID, "svo_render_views: image %d: a device plane of 1 .. 32768 pixels a side, stride >= width", i);
        if (offset[i] < 0 || (offset[i] & 3)) return svo_set_error(SVO_ERR_INVALID, "svo_render_views: image %d: offset must be >= 0 and a multiple of 4", i);
        KpsDev d{};
        if (style->markers) {
            if (k.n < 0) return svo_set_error(SVO_ERR_INVALID, "svo_render_views: image %d: n must be >= 0", i);
            if (!take_planes(k, KP_VIEW, k.n > 0, d))
                return svo_set_error(SVO_ERR_INVALID, "svo_render_views: image %d: kps2d, flags, level_type and color are device memory, 4-byte aligned", i);
        }
        view_tiles(make_view(im), pixels + offset[i], style->markers ? &d : nullptr, k.n, tiles);
    }
    if (tiles.empty()) return SVO_OK;
    // (SVO_VIEW_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_VIEW_TABLE_TILES", std::min<size_t>(tiles.size(), (size_t)INT_MAX));
    if (const int rc = h->view_ws.reserve(sizeof(ViewTile) * chunk, h->stream)) return rc;
    const ViewParams params = view_params(*style);
    return launch_tiles(h, tiles, reinterpret_cast<ViewTile*>(h->view_ws.ptr.get()), chunk,
                        [&](const ViewTile* d, int m, hipStream_t s) { launch_view(d, m, params, s); });
}

extern "C" int svo_render_scene(svo_handle* h, int n, const svo_scene_src* src, const svo_scene_camera* cameras,
                                const int64_t* offset, const svo_scene_style* style, uint8_t* pixels) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !cameras || !offset))) return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: bad arguments");
    if (const int rc = scene_check_style(style, "svo_render_scene")) return rc;
    if (!pixels || ((uintptr_t)pixels & 3)) return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: pixels is NULL or not 4-byte aligned");
    std::vector<SceneSet> sets;
    std::vector<SceneImage> images;
    std::vector<size_t> set0;
    std::vector<SceneTile> tiles;
    for (int i = 0; i < n; i++) {
        const svo_scene_src& s = src[i];
        if (s.cols < 1 || s.cols > 4096 || s.rows < 1 || s.rows > 4096)
            return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: image %d: %d x %d is not within 1 .. 4096 a side", i, s.cols, s.rows);
        if (offset[i] < 0 || (offset[i] & 3)) return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: image %d: offset must be >= 0 and a multiple of 4", i);
        if (const int rc = scene_check_camera(&cameras[i], "svo_render_scene", i)) return rc;
        if (s.n_sets < 0 || s.n_lines < 0 || (s.n_sets > 0 && (!s.sets || !s.own_id)) || (s.n_lines > 0 && !s.lines) || ((uintptr_t)s.lines & 15))
            return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: image %d: sets, own_id or lines missing, or lines not 16-byte aligned", i);
        set0.push_back(sets.size());
        for (int j = 0; j < s.n_sets; j++) {
            const svo_keypoints& k = s.sets[j];
            if (k.n < 0) return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: image %d: set %d: n must be >= 0", i, j);
            KpsDev d;
            if (!take_planes(k, KP_MAP, k.n > 0, d))
                return svo_set_error(SVO_ERR_INVALID, "svo_render_scene: image %d: set %d: kps3d, flags, keyframe_id, inlier_count and color are device memory, 4-byte aligned", i, j);
            sets.push_back(scene_set(d, k.n, s.own_id[j]));
        }
        SceneImage im;
        im.cam = cameras[i];
        im.dst = pixels + offset[i];
        im.sets = nullptr; im.lines = s.lines;             // (the sets are placed below, once the block is there)
        im.n_sets = s.n_sets; im.n_lines = s.n_lines;
        im.w = s.cols; im.h = s.rows;
        scene_tiles(i, s.cols, s.rows, tiles);
        images.push_back(im);
    }
    if (tiles.empty()) return SVO_OK;
    // (SVO_SCENE_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_SCENE_TABLE_TILES", std::min<size_t>(tiles.size(), (size_t)INT_MAX));
    const size_t sets_bytes = (sizeof(SceneSet) * sets.size() + 15) / 16 * 16;
    const size_t images_bytes = (sizeof(SceneImage) * images.size() + 15) / 16 * 16;
    const size_t bytes = sets_bytes + images_bytes + sizeof(SceneTile) * chunk;
    if (const int rc = h->scene_ws.reserve(bytes, h->stream)) return rc;
    const SceneSet* d_sets = reinterpret_cast<const SceneSet*>(h->scene_ws.ptr.get());
    const SceneImage* d_images = reinterpret_cast<const SceneImage*>(h->scene_ws.ptr.get() + sets_bytes);
    for (size_t i = 0; i < images.size(); i++) images[i].sets = d_sets + set0[i];
    if (!sets.empty()) HIP_TRY(hipMemcpyAsync(h->scene_ws.ptr.get(), sets.data(), sizeof(SceneSet) * sets.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->scene_ws.ptr.get() + sets_bytes, images.data(), sizeof(SceneImage) * images.size(), hipMemcpyHostToDevice, h->stream));
    const SceneParams params = scene_params(*style);
    return launch_tiles(h, tiles, reinterpret_cast<SceneTile*>(h->scene_ws.ptr.get() + sets_bytes + images_bytes), chunk,
                        [&](const SceneTile* d, int m, hipStream_t s) { launch_scene(d, m, d_images, params, s); });
}

// svo_render_scene with cloud points: the key planes of the images that have a record are cleared, the pieces of
// every span go through the splat pass (a table of its own, chunked like the tile table), then the tile kernel starts
// from the planes. Without a record it is svo_render_scene itself.
extern "C" int svo_render_scene_clouds(svo_handle* h, int n, const svo_scene_src* src, const svo_scene_span* spans, const int32_t* n_spans,
                                       const svo_scene_camera* cameras, const int64_t* offset, const svo_scene_style* style,
                                       int32_t point_size, uint8_t* pixels) {
    const char* who = "svo_render_scene_clouds";
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !cameras || !offset || !n_spans))) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments", who);
    if (point_size < 1 || point_size > 16) return svo_set_error(SVO_ERR_INVALID, "%s: point_size %d is not within 1 .. 16", who, point_size);
    int64_t records = 0, pieces = 0;
    size_t n_all = 0;
    for (int i = 0; i < n; i++) {
        if (n_spans[i] < 0 || (n_spans[i] > 0 && !spans)) return svo_set_error(SVO_ERR_INVALID, "%s: image %d: %d spans, or no span array", who, i, n_spans[i]);
        for (int j = 0; j < n_spans[i]; j++, n_all++) {
            const svo_scene_span& sp = spans[n_all];
            if (!scene_span_ok((uintptr_t)sp.points, sp.n))
                return svo_set_error(SVO_ERR_INVALID, "%s: image %d: span %d: n %lld must be >= 0 and its records device memory, 16-byte aligned", who, i, j,
                                     (long long)sp.n);
            records += sp.n;
            pieces += scene_span_pieces(sp.n);
        }
    }
    if (records == 0) return svo_render_scene(h, n, src, cameras, offset, style, pixels);
    if (pieces > INT_MAX) return svo_set_error(SVO_ERR_INVALID, "%s: %lld records are too many for one call", who, (long long)records);
    if (const int rc = scene_check_style(style, who)) return rc;
    if (!pixels || ((uintptr_t)pixels & 3)) return svo_set_error(SVO_ERR_INVALID, "%s: pixels is NULL or not 4-byte aligned", who);
    std::vector<SceneSet> sets;
    std::vector<SceneImage> images;
    std::vector<size_t> set0, plane_at((size_t)n, SIZE_MAX);
    std::vector<SceneTile> tiles;
    std::vector<SceneSpan> table;
    size_t planes_bytes = 0;
    n_all = 0;
    for (int i = 0; i < n; i++) {
        const svo_scene_src& s = src[i];
        if (s.cols < 1 || s.cols > 4096 || s.rows < 1 || s.rows > 4096)
            return svo_set_error(SVO_ERR_INVALID, "%s: image %d: %d x %d is not within 1 .. 4096 a side", who, i, s.cols, s.rows);
        if (offset[i] < 0 || (offset[i] & 3)) return svo_set_error(SVO_ERR_INVALID, "%s: image %d: offset must be >= 0 and a multiple of 4", who, i);
        if (const int rc = scene_check_camera(&cameras[i], who, i)) return rc;
        if (s.n_sets < 0 || s.n_lines < 0 || (s.n_sets > 0 && (!s.sets || !s.own_id)) || (s.n_lines > 0 && !s.lines) || ((uintptr_t)s.lines & 15))
            return svo_set_error(SVO_ERR_INVALID, "%s: image %d: sets, own_id or lines missing, or lines not 16-byte aligned", who, i);
        set0.push_back(sets.size());
        for (int j = 0; j < s.n_sets; j++) {
            const svo_keypoints& k = s.sets[j];
            if (k.n < 0) return svo_set_error(SVO_ERR_INVALID, "%s: image %d: set %d: n must be >= 0", who, i, j);
            KpsDev d;
            if (!take_planes(k, KP_MAP, k.n > 0, d))
                return svo_set_error(SVO_ERR_INVALID, "%s: image %d: set %d: kps3d, flags, keyframe_id, inlier_count and color are device memory, 4-byte aligned", who, i, j);
            sets.push_back(scene_set(d, k.n, s.own_id[j]));
        }
        for (int j = 0; j < n_spans[i]; j++, n_all++) {
            const svo_scene_span& sp = spans[n_all];
            if (sp.n > 0 && plane_at[(size_t)i] == SIZE_MAX) {
                plane_at[(size_t)i] = planes_bytes;
                planes_bytes += scene_key_bytes(s.cols, s.rows);
            }
            scene_each_piece(sp.n, [&](int64_t first, int count) { table.push_back(SceneSpan{sp.points + first, i, count}); });
        }
        SceneImage im;
        im.cam = cameras[i];
        im.dst = pixels + offset[i];
        im.sets = nullptr; im.lines = s.lines;             // (the sets are placed below, once the block is there)
        im.n_sets = s.n_sets; im.n_lines = s.n_lines;
        im.w = s.cols; im.h = s.rows;
        scene_tiles(i, s.cols, s.rows, tiles);
        images.push_back(im);
    }
    const size_t chunk = table_tiles("SVO_SCENE_TABLE_TILES", std::min<size_t>(tiles.size(), (size_t)INT_MAX));
    const size_t sets_bytes = (sizeof(SceneSet) * sets.size() + 15) / 16 * 16;
    const size_t images_bytes = (sizeof(SceneImage) * images.size() + 15) / 16 * 16;
    if (const int rc = h->scene_ws.reserve(sets_bytes + images_bytes + sizeof(SceneTile) * chunk, h->stream)) return rc;
    // (SVO_SCENE_TABLE_SPANS: a smaller span table, so that tests reach the chunked splat launches)
    const size_t span_chunk = table_tiles("SVO_SCENE_TABLE_SPANS", table.size());
    const size_t ptrs_bytes = (sizeof(unsigned long long*) * (size_t)n + 255) / 256 * 256;
    if (const int rc = h->scene_cloud_ws.reserve(planes_bytes + ptrs_bytes + sizeof(SceneSpan) * span_chunk, h->stream)) return rc;
    uint8_t* const d_planes = h->scene_cloud_ws.ptr.get();
    unsigned long long** const d_ptrs = reinterpret_cast<unsigned long long**>(d_planes + planes_bytes);
    std::vector<unsigned long long*> ptrs((size_t)n, nullptr);
    for (int i = 0; i < n; i++)
        if (plane_at[(size_t)i] != SIZE_MAX) ptrs[(size_t)i] = reinterpret_cast<unsigned long long*>(d_planes + plane_at[(size_t)i]);
    const SceneSet* d_sets = reinterpret_cast<const SceneSet*>(h->scene_ws.ptr.get());
    const SceneImage* d_images = reinterpret_cast<const SceneImage*>(h->scene_ws.ptr.get() + sets_bytes);
    for (size_t i = 0; i < images.size(); i++) images[i].sets = d_sets + set0[i];
    if (!sets.empty()) HIP_TRY(hipMemcpyAsync(h->scene_ws.ptr.get(), sets.data(), sizeof(SceneSet) * sets.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->scene_ws.ptr.get() + sets_bytes, images.data(), sizeof(SceneImage) * images.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_ptrs, ptrs.data(), sizeof(unsigned long long*) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(d_planes, 0xff, planes_bytes, h->stream));
    const SceneParams params = scene_params(*style);
    if (const int rc = launch_tiles(h, table, reinterpret_cast<SceneSpan*>(d_planes + planes_bytes + ptrs_bytes), span_chunk,
                                    [&](const SceneSpan* d, int m, hipStream_t s) { launch_scene_splat(d, m, d_images, d_ptrs, params, point_size, s); }))
        return rc;
    return launch_tiles(h, tiles, reinterpret_cast<SceneTile*>(h->scene_ws.ptr.get() + sets_bytes + images_bytes), chunk,
                        [&](const SceneTile* d, int m, hipStream_t s) { launch_scene_clouds(d, m, d_images, d_ptrs, params, s); });
}

// svo_render_ar (occlusion == null) and svo_render_ar_occluded. `occluded` (occlusion->on == 1): the occluder table and
// the images' counters follow the records in the workspace, the tile table comes last as before; the counters come
// back in one copy after the last tile launch.
static int render_ar(svo_handle* h, int n, const svo_ar_src* src, const svo_ar_camera* cameras, const int64_t* offset, const svo_ar_style* style,
                     const svo_ar_occlusion* occlusion, const svo_ar_occluder* occluders, uint8_t* pixels, svo_ar_visibility* visibility) {
    CHECK_H(h);
    const bool occluded = occlusion && occlusion->on == 1;
    if (occluded && n > 0 && !occluders) return svo_set_error(SVO_ERR_INVALID, "svo_render_ar_occluded: no occluders");
    if (n < 0 || (n > 0 && (!src || !cameras || !offset))) return svo_set_error(SVO_ERR_INVALID, "svo_render_ar: bad arguments");
    if (const int rc = ar_check_style(style, "svo_render_ar")) return rc;
    if (!pixels || ((uintptr_t)pixels & 3)) return svo_set_error(SVO_ERR_INVALID, "svo_render_ar: pixels is NULL or not 4-byte aligned");
    std::vector<svo_ar_draw> draws;
    std::vector<ArImage> images;
    std::vector<size_t> draw0, rec0;
    std::vector<ArSetup> setup;
    std::vector<ArTile> tiles;
    size_t records = 0;
    for (int i = 0; i < n; i++) {
        const svo_ar_src& s = src[i];
        const svo_image& im = s.image;
        if (!im.data || im.width < 1 || im.height < 1 || im.stride < im.width || im.width > (1 << 15) || im.height > (1 << 15))
            return svo_set_error(SVO_ERR_INVALID, "svo_render_ar: image %d: a device plane of 1 .. 32768 pixels a side, stride >= width", i);
        if (offset[i] < 0 || (offset[i] & 3)) return svo_set_error(SVO_ERR_INVALID, "svo_render_ar: image %d: offset must be >= 0 and a multiple of 4", i);
        if (const int rc = ar_check_camera(&cameras[i], "svo_render_ar", i)) return rc;
        if (s.n_draws < 0 || (s.n_draws > 0 && !s.draws) || s._reserved != 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_render_ar: image %d: draws missing, or _reserved is not 0", i);
        int64_t tri = 0;
        for (int j = 0; j < s.n_draws; j++) {
            const svo_ar_draw& d = s.draws[j];
            bool finite = true;
            for (float v : d.model) finite = finite && std::isfinite(v);
            if (!finite || d.n_vertices < 0 || d.n_triangles < 0 || (d.n_triangles > 0 && (!d.triangles || (d.n_vertices > 0 && !d.vertices))) ||
                (((uintptr_t)d.vertices | (uintptr_t)d.triangles | (uintptr_t)d.rgb) & 3) || (d.rgb_all >> 24) || d._reserved != 0)
                return svo_set_error(SVO_ERR_INVALID, "svo_render_ar: image %d: draw %d: a model entry that is not finite, a negative count, arrays missing or not 4-byte aligned, a colour with a top byte, or _reserved is not 0", i, j);
            tri += d.n_triangles;
        }
        if (tri > SVO_AR_MAX_TRIANGLES)
            return svo_set_error(SVO_ERR_CAPACITY, "svo_render_ar: image %d: %lld triangles, at most %d", i, (long long)tri, (int)SVO_AR_MAX_TRIANGLES);
        if (occluded) {
            if (const int rc = ar_check_occluder(&occluders[i], "svo_render_ar_occluded", i)) return rc;
        }
        draw0.push_back(draws.size());
        rec0.push_back(records);
        draws.insert(draws.end(), s.draws, s.draws + s.n_draws);
        ArImage a;
        a.cam = cameras[i];
        a.src = im.data; a.dst = pixels + offset[i];
        a.draws = nullptr; a.records = nullptr;            // (placed below, once the block is there)
        a.src_stride = im.stride; a.w = im.width; a.h = im.height;
        a.n_records = ar_work(i, im.width, im.height, s.draws, s.n_draws, setup, tiles);
        records += (size_t)a.n_records;
        images.push_back(a);
    }
    for (int i = 0; visibility && i < n; i++) {
        visibility[i] = svo_ar_visibility{};
        visibility[i].status = occluded && occluders[i].records ? SVO_CLOUD_OK : SVO_CLOUD_NONE;
    }
    if (tiles.empty()) return SVO_OK;
    // (SVO_AR_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_AR_TABLE_TILES", std::min<size_t>(tiles.size(), (size_t)INT_MAX));
    auto pad = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t draws_bytes = pad(sizeof(svo_ar_draw) * draws.size()), images_bytes = pad(sizeof(ArImage) * images.size());
    const size_t setup_bytes = pad(sizeof(ArSetup) * setup.size()), records_bytes = sizeof(ArRecord) * records;
    const size_t occl_bytes = occluded ? sizeof(ArOccluder) * (size_t)n : 0, counts_bytes = occluded ? 16 * (size_t)n : 0;
    const size_t tiles_at = draws_bytes + images_bytes + setup_bytes + records_bytes + occl_bytes + counts_bytes;
    const size_t bytes = tiles_at + sizeof(ArTile) * chunk;
    if (const int rc = h->ar_ws.reserve(bytes, h->stream)) return rc;
    uint8_t* base = h->ar_ws.ptr.get();
    const svo_ar_draw* d_draws = reinterpret_cast<const svo_ar_draw*>(base);
    const ArImage* d_images = reinterpret_cast<const ArImage*>(base + draws_bytes);
    const ArSetup* d_setup = reinterpret_cast<const ArSetup*>(base + draws_bytes + images_bytes);
    ArRecord* d_records = reinterpret_cast<ArRecord*>(base + draws_bytes + images_bytes + setup_bytes);
    for (size_t i = 0; i < images.size(); i++) { images[i].draws = d_draws + draw0[i]; images[i].records = d_records + rec0[i]; }
    const ArOccluder* d_occluders = reinterpret_cast<const ArOccluder*>(base + draws_bytes + images_bytes + setup_bytes + records_bytes);
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(base + draws_bytes + images_bytes + setup_bytes + records_bytes + occl_bytes);
    std::vector<ArOccluder> occl;
    for (int i = 0; occluded && i < n; i++) {
        const svo_ar_occluder& o = occluders[i];
        occl.push_back(ArOccluder{o.records, d_counts + 2 * (size_t)i, o.records ? o.cols : 0, o.records ? o.rows : 0, o.records ? o.step : 1, 0});
    }
    const ArParams params = ar_params(*style);
    int rc = SVO_OK;
    auto up = [&](const void* dst, const void* from, size_t b) {
        if (rc == SVO_OK && b > 0 && hipMemcpyAsync(const_cast<void*>(dst), from, b, hipMemcpyHostToDevice, h->stream) != hipSuccess)
            rc = svo_set_error(SVO_ERR_HIP, "svo_render_ar: an upload failed");
    };
    up(d_draws, draws.data(), sizeof(svo_ar_draw) * draws.size());
    up(d_images, images.data(), sizeof(ArImage) * images.size());
    up(d_setup, setup.data(), sizeof(ArSetup) * setup.size());
    up(d_occluders, occl.data(), sizeof(ArOccluder) * occl.size());
    if (rc == SVO_OK && occluded && hipMemsetAsync(d_counts, 0, counts_bytes, h->stream) != hipSuccess)
        rc = svo_set_error(SVO_ERR_HIP, "svo_render_ar_occluded: clearing the counters failed");
    if (rc == SVO_OK) {
        launch_ar_setup(d_setup, (int)setup.size(), d_images, params, h->stream);
        if (hipGetLastError() != hipSuccess) rc = svo_set_error(SVO_ERR_HIP, "svo_render_ar: the first launch failed");
    }
    if (rc != SVO_OK) {                                    // (the uploads read host memory of this call)
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    if (!occluded)
        return launch_tiles(h, tiles, reinterpret_cast<ArTile*>(base + tiles_at), chunk,
                            [&](const ArTile* d, int m, hipStream_t s) { launch_ar(d, m, d_images, params, s); });
    const ArOcclusion occlusion_params = ar_occlusion(*occlusion);
    if (const int rc2 = launch_tiles(h, tiles, reinterpret_cast<ArTile*>(base + tiles_at), chunk, [&](const ArTile* d, int m, hipStream_t s) {
            launch_ar_occluded(d, m, d_images, d_occluders, params, occlusion_params, s);
        }))
        return rc2;
    if (visibility) {
        std::vector<unsigned long long> counts(2 * (size_t)n);
        HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, counts_bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int i = 0; i < n; i++) {
            visibility[i].covered = (int64_t)counts[2 * (size_t)i];
            visibility[i].hidden = (int64_t)counts[2 * (size_t)i + 1];
        }
    }
    return SVO_OK;
}

extern "C" int svo_render_ar(svo_handle* h, int n, const svo_ar_src* src, const svo_ar_camera* cameras, const int64_t* offset,
                             const svo_ar_style* style, uint8_t* pixels) {
    return render_ar(h, n, src, cameras, offset, style, nullptr, nullptr, pixels, nullptr);
}

extern "C" int svo_render_ar_occluded(svo_handle* h, int n, const svo_ar_src* src, const svo_ar_camera* cameras, const int64_t* offset,
                                      const svo_ar_style* style, const svo_ar_occlusion* occlusion, const svo_ar_occluder* occluders,
                                      uint8_t* pixels, svo_ar_visibility* visibility) {
    if (const int rc = ar_check_occlusion(occlusion, "svo_render_ar_occluded")) return rc;
    return render_ar(h, n, src, cameras, offset, style, occlusion, occluders, pixels, visibility);
}


// With a check that is on, a chunk of the image table is followed by its LrImage table and the reverse planes of its
// images (each a multiple of 256 bytes) in the workspace: the search writes disparities whatever the style's value, the
// reverse search and the check follow it in the stream.
extern "C" int svo_dense_disparity_checked(svo_handle* h, int n, const svo_dense_src* src, const int64_t* offset,
                                           const svo_disparity_style* style, const svo_stereo_check* check, float* values) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !offset))) return svo_set_error(SVO_ERR_INVALID, "svo_dense_disparity: bad arguments");
    DenseParams params;
    if (const int rc = dense_check_style(style, nullptr, "svo_dense_disparity", &params)) return rc;
    LrCheck lr;
    if (const int rc = lr_check_parse(check, false, "svo_dense_disparity_checked", &lr)) return rc;
    const LrParams lr_params{params.value, params.step, lr.max_lr_diff};
    if (lr.on) params.value = SVO_DENSE_DISPARITY;
    std::vector<LrImage> checks(lr.on ? (size_t)n : 0);
    std::vector<size_t> reverse(lr.on ? (size_t)n : 0);
    if (!values || ((uintptr_t)values & 15)) return svo_set_error(SVO_ERR_INVALID, "svo_dense_disparity: values is NULL or not 16-byte aligned");
    std::vector<DenseImage> images((size_t)n);
    std::vector<int> tiles((size_t)n);
    for (int i = 0; i < n; i++) {
        const svo_image& l = src[i].left;
        const svo_image& r = src[i].right;
        if (!l.data || !r.data || l.width < 1 || l.height < 1 || l.width > (1 << 15) || l.height > (1 << 15) || r.width != l.width ||
            r.height != l.height || l.stride < l.width || r.stride < r.width || src[i]._reserved != 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_dense_disparity: image %d: two device planes of one size, 1 .. 32768 pixels a side, stride >= width, _reserved 0", i);
        if (l.width / params.step < 1 || l.height / params.step < 1)
            return svo_set_error(SVO_ERR_INVALID, "svo_dense_disparity: image %d: %d x %d has no lattice point at step %d", i, l.width, l.height, params.step);
        if (offset[i] < 0 || (offset[i] & 15)) return svo_set_error(SVO_ERR_INVALID, "svo_dense_disparity: image %d: offset must be >= 0 and a multiple of 16", i);
        images[(size_t)i] = DenseImage{l.data, r.data, reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(values) + offset[i]),
                                       l.stride, r.stride, l.width, l.height, src[i].baseline, 0};
        tiles[(size_t)i] = dense_tiles(params, l.width, l.height);
        if (lr.on) {
            float* value = images[(size_t)i].out;
            const int64_t plane = (int64_t)(l.width / params.step) * (l.height / params.step);
            checks[(size_t)i] = LrImage{l.data, r.data, nullptr, value, value + (1 + params.cost) * plane, l.stride, r.stride, l.width, l.height,
                                        src[i].baseline, 0};
            reverse[(size_t)i] = lr_reverse_bytes(l.width, l.height, params.step);
        }
    }
    if (n == 0) return SVO_OK;
    long long workgroups = 0;
    for (int t : tiles) workgroups += t;
    dense_plan(params, workgroups);
    for (int i = 0; i < n; i++) tiles[(size_t)i] = dense_tiles(params, images[(size_t)i].w, images[(size_t)i].h);
    // (SVO_DENSE_TABLE_IMAGES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_DENSE_TABLE_IMAGES", std::min<size_t>((size_t)n, DENSE_MAX_IMAGES));
    const size_t tables = lr.on ? ((sizeof(DenseImage) + sizeof(LrImage)) * chunk + 255) / 256 * 256 : sizeof(DenseImage) * chunk;
    size_t block = 0;
    for (size_t i0 = 0; lr.on && i0 < (size_t)n; i0 += chunk) {
        size_t b = 0;
        for (size_t i = i0; i < std::min(i0 + chunk, (size_t)n); i++) b += reverse[i];
        block = std::max(block, b);
    }
    if (const int rc = h->dense_ws.reserve(tables + block, h->stream)) return rc;
    DenseImage* d_images = reinterpret_cast<DenseImage*>(h->dense_ws.ptr.get());
    LrImage* d_checks = reinterpret_cast<LrImage*>(d_images + chunk);
    int rc = SVO_OK;
    for (size_t i0 = 0; i0 < (size_t)n && rc == SVO_OK; i0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - i0);
        if (i0 > 0 && hipStreamSynchronize(h->stream) != hipSuccess) { rc = svo_set_error(SVO_ERR_HIP, "svo_dense_disparity: a launch failed"); break; }
        if (hipMemcpyAsync(d_images, images.data() + i0, sizeof(DenseImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            rc = svo_set_error(SVO_ERR_HIP, "svo_dense_disparity: an upload failed");
            break;
        }
        const int grid = *std::max_element(tiles.begin() + (ptrdiff_t)i0, tiles.begin() + (ptrdiff_t)(i0 + m));
        launch_dense(d_images, (int)m, grid, params, h->stream);
        if (lr.on) {
            uint8_t* at = h->dense_ws.ptr.get() + tables;
            int lr_grid = 0;
            for (size_t i = i0; i < i0 + m; i++) {
                checks[i].out = reinterpret_cast<float*>(at);
                at += reverse[i];
                lr_grid = std::max(lr_grid, lr_tiles((int64_t)(checks[i].w / params.step) * (checks[i].h / params.step)));
            }
            if (hipMemcpyAsync(d_checks, checks.data() + i0, sizeof(LrImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
                rc = svo_set_error(SVO_ERR_HIP, "svo_dense_disparity: an upload failed");
                break;
            }
            launch_dense_reverse(d_checks, (int)m, grid, params, h->stream);
            launch_lr_check(d_checks, (int)m, lr_grid, lr_params, h->stream);
        }
        if (hipGetLastError() != hipSuccess) rc = svo_set_error(SVO_ERR_HIP, "svo_dense_disparity: a launch failed");
    }
    const hipError_t e = hipStreamSynchronize(h->stream);    // (the uploads read host memory of this call)
    if (rc) return rc;
    HIP_TRY(e);
    return SVO_OK;
}

extern "C" int svo_dense_disparity(svo_handle* h, int n, const svo_dense_src* src, const int64_t* offset,
                                   const svo_disparity_style* style, float* values) {
    return svo_dense_disparity_checked(h, n, src, offset, style, nullptr, values);
}

// With a check that is on, an image's block of the workspace ends with its reverse plane, the LrImage table follows
// the other two, and the reverse search and the check (a mask on the staged disparity plane) run between the search
// and the count launch.
extern "C" int svo_cloud_points_checked(svo_handle* h, int n, const svo_cloud_src* src, const int64_t* first, const svo_cloud_style* style,
                                        const svo_stereo_check* check, svo_map_point* points, int32_t* counts) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !first))) return svo_set_error(SVO_ERR_INVALID, "svo_cloud_points: bad arguments");
    DenseParams search;
    CloudParams params;
    if (const int rc = cloud_check_style(style, nullptr, "svo_cloud_points", &search, &params)) return rc;
    LrCheck lr;
    if (const int rc = lr_check_parse(check, true, "svo_cloud_points_checked", &lr)) return rc;
    const LrParams lr_params{SVO_DENSE_DISPARITY, search.step, lr.max_lr_diff};
    if (!points || ((uintptr_t)points & 15)) return svo_set_error(SVO_ERR_INVALID, "svo_cloud_points: points is NULL or not 16-byte aligned");
    if ((uintptr_t)counts & 3) return svo_set_error(SVO_ERR_INVALID, "svo_cloud_points: counts is not 4-byte aligned");
    // per image of a chunk: its two planes, its tile counts and its pose matrices, each rounded up to 256 bytes
    std::vector<size_t> image_block((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
        const svo_image& l = src[i].left;
        const svo_image& r = src[i].right;
        if (!l.data || !r.data || l.width < 1 || l.height < 1 || l.width > (1 << 15) || l.height > (1 << 15) || r.width != l.width ||
            r.height != l.height || l.stride < l.width || r.stride < r.width || src[i]._reserved != 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_cloud_points: image %d: two device planes of one size, 1 .. 32768 pixels a side, stride >= width, _reserved 0", i);
        if (l.width / params.step < 1 || l.height / params.step < 1)
            return svo_set_error(SVO_ERR_INVALID, "svo_cloud_points: image %d: %d x %d has no lattice point at step %d", i, l.width, l.height, params.step);
        if (first[i] < 0) return svo_set_error(SVO_ERR_INVALID, "svo_cloud_points: image %d: first must be >= 0", i);
        const size_t pts = (size_t)(l.width / params.step) * (size_t)(l.height / params.step);
        image_block[(size_t)i + 1] = (pts * 8 + 255) / 256 * 256 + ((size_t)cloud_tiles((int64_t)pts) * 4 + 255) / 256 * 256 + 256 +
                                     (lr.on ? lr_reverse_bytes(l.width, l.height, params.step) : 0);
    }
    if (n == 0) return SVO_OK;
    // (SVO_CLOUD_TABLE_IMAGES: a smaller table, so that tests reach the chunked launches. SVO_CLOUD_SKIP_SEARCH=1: a
    // measurement's switch, tools/cloud_bench.py: the search is not launched and the count and write launches run on the
    // planes the workspace holds from the call before, so that their time can be taken alone)
    const size_t chunk = table_tiles("SVO_CLOUD_TABLE_IMAGES", std::min<size_t>((size_t)n, DENSE_MAX_IMAGES));
    const char* skip_env = std::getenv("SVO_CLOUD_SKIP_SEARCH");
    const bool skip_search = skip_env && std::atoi(skip_env) == 1;
    const size_t tables = ((sizeof(CloudImage) + sizeof(DenseImage) + (lr.on ? sizeof(LrImage) : 0)) * chunk + 255) / 256 * 256;
    size_t block = 0;
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        size_t b = 0;
        for (size_t i = i0; i < std::min(i0 + chunk, (size_t)n); i++) b += image_block[i + 1];
        block = std::max(block, b);
    }
    if (const int rc = h->cloud_ws.reserve(tables + block, h->stream)) return rc;
    CloudImage* d_cloud = reinterpret_cast<CloudImage*>(h->cloud_ws.ptr.get());
    DenseImage* d_dense = reinterpret_cast<DenseImage*>(d_cloud + chunk);
    LrImage* d_checks = reinterpret_cast<LrImage*>(d_dense + chunk);
    std::vector<CloudImage> cloud(chunk);
    std::vector<DenseImage> dense(chunk);
    std::vector<LrImage> checks(lr.on ? chunk : 0);
    int rc = SVO_OK;
    for (size_t i0 = 0; i0 < (size_t)n && rc == SVO_OK; i0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - i0);
        if (i0 > 0 && hipStreamSynchronize(h->stream) != hipSuccess) { rc = svo_set_error(SVO_ERR_HIP, "svo_cloud_points: a launch failed"); break; }
        uint8_t* at = h->cloud_ws.ptr.get() + tables;
        long long workgroups = 0;
        int cloud_grid = 0;
        for (size_t j = 0; j < m; j++) {
            const svo_cloud_src& s = src[i0 + j];
            const size_t pts = (size_t)(s.left.width / params.step) * (size_t)(s.left.height / params.step);
            float* planes = reinterpret_cast<float*>(at);
            int* tile_counts = reinterpret_cast<int*>(at + (pts * 8 + 255) / 256 * 256);
            const size_t reverse = lr.on ? lr_reverse_bytes(s.left.width, s.left.height, params.step) : 0;
            float* mats = reinterpret_cast<float*>(at + image_block[i0 + j + 1] - reverse - 256);
            if (lr.on)
                checks[j] = LrImage{s.left.data, s.right.data, reinterpret_cast<float*>(at + image_block[i0 + j + 1] - reverse), planes, nullptr,
                                    s.left.stride, s.right.stride, s.left.width, s.left.height, s.baseline, 0};
            at += image_block[i0 + j + 1];
            dense[j] = DenseImage{s.left.data, s.right.data, planes, s.left.stride, s.right.stride, s.left.width, s.left.height, s.baseline, 0};
            CloudImage& c = cloud[j];
            c = CloudImage{s.left.data, planes, planes + pts, points + first[i0 + j], tile_counts, counts ? counts + (i0 + j) : nullptr,
                           s.left.stride, s.left.width, s.left.height, s.baseline, s.fx, s.fy, s.cx, s.cy, {}, mats};
            std::memcpy(c.pose, s.pose, sizeof(c.pose));
            workgroups += dense_tiles(search, s.left.width, s.left.height);
            cloud_grid = std::max(cloud_grid, cloud_tiles((int64_t)pts));
        }
        DenseParams sp = search;
        dense_plan(sp, workgroups);
        int dense_grid = 0;
        for (size_t j = 0; j < m; j++) dense_grid = std::max(dense_grid, dense_tiles(sp, dense[j].w, dense[j].h));
        if (hipMemcpyAsync(d_cloud, cloud.data(), sizeof(CloudImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(d_dense, dense.data(), sizeof(DenseImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            rc = svo_set_error(SVO_ERR_HIP, "svo_cloud_points: an upload failed");
            break;
        }
        if (!skip_search) launch_dense(d_dense, (int)m, dense_grid, sp, h->stream);
        if (lr.on) {
            if (hipMemcpyAsync(d_checks, checks.data(), sizeof(LrImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
                rc = svo_set_error(SVO_ERR_HIP, "svo_cloud_points: an upload failed");
                break;
            }
            launch_dense_reverse(d_checks, (int)m, dense_grid, sp, h->stream);
            launch_lr_check(d_checks, (int)m, lr_tiles((int64_t)cloud_grid * CLOUD_TILE), lr_params, h->stream);
        }
        launch_cloud(d_cloud, (int)m, cloud_grid, params, h->stream);
        if (hipGetLastError() != hipSuccess) rc = svo_set_error(SVO_ERR_HIP, "svo_cloud_points: a launch failed");
    }
    const hipError_t e = hipStreamSynchronize(h->stream);    // (the uploads read host memory of this call)
    if (rc) return rc;
    HIP_TRY(e);
    return SVO_OK;
}

extern "C" int svo_cloud_points(svo_handle* h, int n, const svo_cloud_src* src, const int64_t* first, const svo_cloud_style* style,
                                svo_map_point* points, int32_t* counts) {
    return svo_cloud_points_checked(h, n, src, first, style, nullptr, points, counts);
}

extern "C" int svo_copy_segments(svo_handle* h, int n, const svo_copy_segment* segs) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && !segs)) return svo_set_error(SVO_ERR_INVALID, "svo_copy_segments: bad arguments");
    std::vector<CopyTile> tiles;
    for (int i = 0; i < n; i++) {
        const svo_copy_segment& g = segs[i];
        if (g.row_bytes < 0 || g.rows < 0 || g.src_pitch < 0 || g.dst_pitch < 0 || (g.rows > 1 && g.dst_pitch < g.row_bytes))
            return svo_set_error(SVO_ERR_INVALID, "svo_copy_segments: segment %d: negative size or pitch, or destination rows that overlap", i);
        if (g.row_bytes == 0 || g.rows == 0) continue;
        if (!g.src || !g.dst) return svo_set_error(SVO_ERR_INVALID, "svo_copy_segments: segment %d: null pointer", i);
        cut_copy_tiles(g.src, g.dst, g.row_bytes, g.rows, g.src_pitch, g.dst_pitch, tiles);
    }
    if (tiles.empty()) return SVO_OK;
    // (SVO_SNAPSHOT_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_SNAPSHOT_TABLE_TILES", std::min<size_t>(tiles.size(), (size_t)INT_MAX));
    if (const int rc = h->copy_ws.reserve(sizeof(CopyTile) * chunk, h->stream)) return rc;
    return launch_tiles(h, tiles, reinterpret_cast<CopyTile*>(h->copy_ws.ptr.get()), chunk, &launch_copy_tiles);
}

extern "C" int svo_pose_filter_batch(svo_handle* h, int n_states, const float* state_in, const float* start_pose,
                                     const int* first, int n_samples, const svo_pose_sample* samples, float* state_out,
                                     float* filtered) {
    CHECK_H(h);
    if (n_states < 0 || n_samples < 0 || (n_states > 0 && (!state_in || !start_pose || !first || !state_out)) ||
        (n_samples > 0 && !samples))
        return svo_set_error(SVO_ERR_INVALID, "svo_pose_filter_batch: bad arguments");
    if (((uintptr_t)samples & 7) || (((uintptr_t)state_in | (uintptr_t)start_pose | (uintptr_t)first | (uintptr_t)state_out | (uintptr_t)filtered) & 3))
        return svo_set_error(SVO_ERR_INVALID, "svo_pose_filter_batch: the samples are 8-byte aligned, every other array 4-byte aligned");
    if (n_states == 0 || n_samples == 0) return SVO_OK;
    launch_pose_filter(PoseFilterArgs{n_states, n_samples, state_in, start_pose, first, samples, state_out, filtered}, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}
