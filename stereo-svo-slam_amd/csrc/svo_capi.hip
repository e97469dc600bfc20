// svo_capi.hip — the C ABI of include/svo_hip.h: handle management and the
// stage-level entry points. Each entry fills the per-sequence argument block
// of one kernel (batch = 1), stages it in the handle's device ring and
// launches on the handle's stream. There is NO CPU fallback: without a HIP
// device every call fails with SVO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "svo_host.hpp"
#include "svo_kernels.hpp"
#include "svo_tracker.hpp"

using namespace svo;

struct svo_handle {
    int device;
    hipStream_t stream = nullptr;   // the caller's (svo_handle_set_stream), not owned
    int max_kps;
    DevPtr<uint8_t> ring;           // device ring for argument blocks
    size_t ring_cap = 1 << 20, ring_off = 0;
    DevPtr<float> sia_kpws;         // [9][rec_cap] per-keypoint values of the BIG alignment path
    DevPtr<float> sia_rec;          // [7][68][rec_cap] per-level alignment records
    int rec_cap;
    DevPtr<KfDev> kf_one;           // 1-entry keyframe table for svo_klt_track
    int exact_pinv = 1;             // reference-order Gauss-Newton by default
    DevPtr<uint8_t> remap_ws;       // svo_remap_linear: the map in the kernel's form + the image table
    size_t remap_ws_bytes = 0;
    DevPtr<RigCam> rigcam_ws;       // svo_build_rectify_maps: the camera table
    size_t rigcam_ws_count = 0;
    DevPtr<IngestImg> ingest_ws;    // svo_convert_frames: the image table
    size_t ingest_ws_count = 0;
    DevPtr<ExportTile> export_ws;   // svo_pack_keypoints: the tile table
    size_t export_ws_count = 0;
    DevPtr<CopyTile> copy_ws;       // svo_copy_segments: the tile table
    size_t copy_ws_count = 0;
    DevPtr<uint8_t> map_ws;         // svo_pack_map_points: the tile counts of a call, then the tile table
    size_t map_ws_bytes = 0;
    DevPtr<ViewTile> view_ws;       // svo_render_views: the tile table
    size_t view_ws_count = 0;
    DevPtr<uint8_t> scene_ws;       // svo_render_scene: the sets and image records of a call, then the tile table
    size_t scene_ws_bytes = 0;
};

extern "C" const char* svo_last_error(void) { return svo_error_text; }
extern "C" int svo_version(void) { return 100; }

extern "C" int svo_handle_create(int device, int max_keypoints, svo_handle** out) {
    if (!out || max_keypoints <= 0) return svo_set_error(SVO_ERR_INVALID, "svo_handle_create: bad arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return svo_set_error(SVO_ERR_NO_DEVICE, "no HIP device visible: libsvo_hip has no CPU fallback");
    if (device < 0 || device >= count) return svo_set_error(SVO_ERR_INVALID, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<svo_handle> h(new (std::nothrow) svo_handle());
    if (!h) return svo_set_error(SVO_ERR_INVALID, "out of host memory");
    h->device = device;
    h->max_kps = max_keypoints;
    HIP_TRY(dev_malloc(h->ring, h->ring_cap));
    HIP_TRY(dev_malloc(h->kf_one, sizeof(KfDev)));
    h->rec_cap = (max_keypoints + 511) / 512 * 512;
    HIP_TRY(dev_malloc(h->sia_rec, sizeof(float) * 7 * 68 * (size_t)h->rec_cap));
    HIP_TRY(dev_malloc(h->sia_kpws, sizeof(float) * 9 * (size_t)h->rec_cap));
    *out = h.release();
    return SVO_OK;
}

extern "C" int svo_handle_destroy(svo_handle* h) {
    if (!h) return SVO_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return SVO_OK;
}

extern "C" int svo_handle_set_stream(svo_handle* h, void* s) {
    if (!h) return svo_set_error(SVO_ERR_INVALID, "null handle");
    h->stream = reinterpret_cast<hipStream_t>(s);
    return SVO_OK;
}

extern "C" int svo_handle_set_fast_solver(svo_handle* h, int on) {
    if (!h) return svo_set_error(SVO_ERR_INVALID, "null handle");
    h->exact_pinv = on == 0;
    return SVO_OK;
}

extern "C" int svo_handle_set_exact_pinv(svo_handle* h, int on) {
    if (!h) return svo_set_error(SVO_ERR_INVALID, "null handle");
    h->exact_pinv = on != 0;
    return SVO_OK;
}

extern "C" int svo_handle_synchronize(svo_handle* h) {
    if (!h) return svo_set_error(SVO_ERR_INVALID, "null handle");
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;
}

// copy a host block into the device ring (stream ordered); returns device address
template <typename T>
static int stage(svo_handle* h, const T& host, T** dev) {
    const size_t bytes = (sizeof(T) + 255) & ~(size_t)255;
    if (h->ring_off + bytes > h->ring_cap) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->ring_off = 0;
    }
    T* d = reinterpret_cast<T*>(h->ring.get() + h->ring_off);
    h->ring_off += bytes;
    HIP_TRY(hipMemcpyAsync(d, &host, sizeof(T), hipMemcpyHostToDevice, h->stream));
    *dev = d;
    return SVO_OK;
}

static int stage_n(svo_handle* h, int n, int** d_n) { return stage<int>(h, n, d_n); }

#define CHECK_H(h)                                                   \
    do {                                                             \
        if (!(h)) return svo_set_error(SVO_ERR_INVALID, "null handle");       \
        HIP_TRY(hipSetDevice((h)->device));                          \
    } while (0)

extern "C" int svo_device_malloc(size_t bytes, void** out) {
    if (!out) return svo_set_error(SVO_ERR_INVALID, "svo_device_malloc: null out");
    DevPtr<void> p;
    HIP_TRY(dev_malloc(p, bytes ? bytes : 1));
    *out = p.release();
    return SVO_OK;
}
extern "C" int svo_device_free(void* p) {
    if (p) HIP_TRY(dev_free(p));
    return SVO_OK;
}
extern "C" int svo_copy_to_device(svo_handle* h, void* dst, const void* src, size_t bytes) {
    CHECK_H(h);
    if (bytes == 0) return SVO_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;
}
extern "C" int svo_copy_to_host(svo_handle* h, void* dst, const void* src, size_t bytes) {
    CHECK_H(h);
    if (bytes == 0) return SVO_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;
}
extern "C" int svo_copy_image_to_device(svo_handle* h, void* dst, size_t dst_stride, const void* src,
                                        size_t src_stride, size_t width, size_t height) {
    CHECK_H(h);
    HIP_TRY(hipMemcpy2DAsync(dst, dst_stride, src, src_stride, width, height, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;
}

extern "C" int svo_project_keypoints(svo_handle* h, const float* pose, const svo_kp3d* kps3d, int n,
                                     const svo_camera_settings* cam, svo_kp2d* out) {
    CHECK_H(h);
    if (!pose || !cam || n < 0 || (n > 0 && (!kps3d || !out)))
        return svo_set_error(SVO_ERR_INVALID, "svo_project_keypoints: bad arguments");
    if (n > 0) launch_project(pose, kps3d, n, *cam, out, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_build_pyramid(svo_handle* h, int n_levels, svo_image* levels) {
    CHECK_H(h);
    if (!levels || n_levels < 1 || n_levels > 7)
        return svo_set_error(SVO_ERR_INVALID, "svo_build_pyramid: n_levels must be 1..7");
    PyrArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.n_levels = n_levels;
    for (int l = 1; l < n_levels; l++) {
        levels[l].width = levels[l - 1].width / 2;
        levels[l].height = levels[l - 1].height / 2;
        levels[l].stride = levels[l].width;
    }
    for (int l = 0; l < n_levels; l++) pa.level[l] = make_view(levels[l]);
    PyrArgs* d;
    int rc = stage(h, pa, &d);
    if (rc) return rc;
    if (n_levels > 1) launch_pyr_fused(d, 1, levels[0].width, levels[0].height, false, pyr_stream_rows(pa), h->stream);
    HIP_TRY(hipGetLastError());
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
    if (need > h->remap_ws_bytes) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old workspace may still be read)
        h->remap_ws.reset();
        h->remap_ws_bytes = 0;
        HIP_TRY(dev_malloc(h->remap_ws, need));
        h->remap_ws_bytes = need;
    }
    std::vector<RemapImg> imgs(n);
    for (int i = 0; i < n; i++) imgs[i] = RemapImg{make_view(src[i]), make_view(dst[i])};
    RemapImg* d_img = reinterpret_cast<RemapImg*>(h->remap_ws.get() + map_bytes);
    HIP_TRY(hipMemcpyAsync(d_img, imgs.data(), sizeof(RemapImg) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    RemapLaunch a;
    std::memset(&a, 0, sizeof(a));
    a.map[0] = a.map[1] = remap_map_view(h->remap_ws.get(), w, hgt);
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
    if ((size_t)n > h->rigcam_ws_count) {
        HIP_TRY(hipStreamSynchronize(h->stream));     // (an earlier call may still read the table)
        h->rigcam_ws.reset();
        h->rigcam_ws_count = 0;
        HIP_TRY(dev_malloc(h->rigcam_ws, sizeof(RigCam) * (size_t)n));
        h->rigcam_ws_count = (size_t)n;
    }
    HIP_TRY(hipMemcpyAsync(h->rigcam_ws.get(), cams.data(), sizeof(RigCam) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    launch_rig_maps(h->rigcam_ws.get(), n, width, height, false, h->stream);
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
    if (need > h->remap_ws_bytes) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old workspace may still be read)
        h->remap_ws.reset();
        h->remap_ws_bytes = 0;
        HIP_TRY(dev_malloc(h->remap_ws, need));
        h->remap_ws_bytes = need;
    }
    uint8_t* ws = h->remap_ws.get();
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
    if ((size_t)2 * n > h->ingest_ws_count) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old table may still be read)
        h->ingest_ws.reset();
        h->ingest_ws_count = 0;
        HIP_TRY(dev_malloc(h->ingest_ws, sizeof(IngestImg) * 2 * (size_t)n));
        h->ingest_ws_count = (size_t)2 * n;
    }
    std::vector<IngestImg> imgs((size_t)2 * n);
    for (int i = 0; i < n; i++)
        for (int side = 0; side < 2; side++) {
            const svo_image& s = (side ? f->right : f->left).buffer ? src_b[i] : src_a[i];
            imgs[(size_t)side * n + i] = ingest_image(*f, side, s.data, s.stride, make_view(side ? right[i] : left[i]));
        }
    HIP_TRY(hipMemcpyAsync(h->ingest_ws.get(), imgs.data(), sizeof(IngestImg) * imgs.size(), hipMemcpyHostToDevice, h->stream));
    const int total = 2 * n, per_launch = 32768;
    for (int i0 = 0; i0 < total; i0 += per_launch) {
        launch_ingest(h->ingest_ws.get() + i0, std::min(per_launch, total - i0), w, hgt, h->stream);
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
        d.kps2d = k.kps2d; d.kps3d = k.kps3d; d.flags = k.flags; d.kf_id = k.keyframe_id; d.kp_index = k.keypoint_index;
        d.outl = k.outlier_count; d.inl = k.inlier_count; d.kfx = k.kf_inv_depth; d.kfP = k.kf_variance;
        d.score = k.score; d.level_type = k.level_type; d.color = k.color; d.n = nullptr;
        for (const void* p : {(const void*)d.kps2d, (const void*)d.kps3d, (const void*)d.flags, (const void*)d.kf_id,
                              (const void*)d.kp_index, (const void*)d.outl, (const void*)d.inl, (const void*)d.kfx,
                              (const void*)d.kfP, (const void*)d.score, (const void*)d.level_type, (const void*)d.color})
            if (!p || ((uintptr_t)p & 3))
                return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: set %d: every array is device memory, 4-byte aligned", i);
        for (int start = 0; start < k.n; start += EXPORT_TILE)
            tiles.push_back(export_tile(d, start, std::min(EXPORT_TILE, k.n - start), first[i]));
    }
    if (tiles.empty() || (!kps2d && !kps3d && !info)) return SVO_OK;
    if (tiles.size() > (size_t)INT_MAX) return svo_set_error(SVO_ERR_INVALID, "svo_pack_keypoints: too many keypoints");
    if (tiles.size() > h->export_ws_count) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old table may still be read)
        h->export_ws.reset();
        h->export_ws_count = 0;
        HIP_TRY(dev_malloc(h->export_ws, sizeof(ExportTile) * tiles.size()));
        h->export_ws_count = tiles.size();
    }
    HIP_TRY(hipMemcpyAsync(h->export_ws.get(), tiles.data(), sizeof(ExportTile) * tiles.size(), hipMemcpyHostToDevice, h->stream));
    launch_export(h->export_ws.get(), (int)tiles.size(), kps2d, kps3d, info, h->stream);
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
            KpsDev d{};
            d.kps3d = k.kps3d; d.flags = k.flags; d.kf_id = k.keyframe_id; d.inl = k.inlier_count; d.color = k.color;
            for (const void* p : {(const void*)d.kps3d, (const void*)d.flags, (const void*)d.kf_id, (const void*)d.inl, (const void*)d.color})
                if ((k.n > 0 && !p) || ((uintptr_t)p & 3))
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
    if (bytes > h->map_ws_bytes) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old block may still be read)
        h->map_ws.reset();
        h->map_ws_bytes = 0;
        HIP_TRY(dev_malloc(h->map_ws, bytes));
        h->map_ws_bytes = bytes;
    }
    int* tile_counts = reinterpret_cast<int*>(h->map_ws.get());
    std::vector<MapTile> host(chunk);
    TileTable table{host.data(), reinterpret_cast<MapTile*>(h->map_ws.get() + counts_bytes), chunk, h->stream,
                    [&](const MapTile* d, int m, hipStream_t s) { launch_map(d, m, f, points, tile_counts, counts, s); }};
    for (const MapTile& t : tiles)
        if (const int rc = table.add(t)) return rc;
    if (const int rc = table.launch(false)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));          // (the table's upload read `host`)
    return SVO_OK;
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
            d.kps2d = k.kps2d; d.flags = k.flags; d.level_type = k.level_type; d.color = k.color;
            for (const void* p : {(const void*)d.kps2d, (const void*)d.flags, (const void*)d.level_type, (const void*)d.color})
                if ((k.n > 0 && !p) || ((uintptr_t)p & 3))
                    return svo_set_error(SVO_ERR_INVALID, "svo_render_views: image %d: kps2d, flags, level_type and color are device memory, 4-byte aligned", i);
        }
        view_tiles(make_view(im), pixels + offset[i], style->markers ? &d : nullptr, k.n, tiles);
    }
    if (tiles.empty()) return SVO_OK;
    // (SVO_VIEW_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    const size_t chunk = table_tiles("SVO_VIEW_TABLE_TILES", std::min<size_t>(tiles.size(), (size_t)INT_MAX));
    if (chunk > h->view_ws_count) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old table may still be read)
        h->view_ws.reset();
        h->view_ws_count = 0;
        HIP_TRY(dev_malloc(h->view_ws, sizeof(ViewTile) * chunk));
        h->view_ws_count = chunk;
    }
    const ViewParams params = view_params(*style);
    std::vector<ViewTile> host(chunk);
    TileTable table{host.data(), h->view_ws.get(), chunk, h->stream,
                    [&](const ViewTile* d, int m, hipStream_t s) { launch_view(d, m, params, s); }};
    for (const ViewTile& t : tiles)
        if (const int rc = table.add(t)) return rc;
    if (const int rc = table.launch(false)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));          // (the table's upload read `host`)
    return SVO_OK;
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
            KpsDev d{};
            d.kps3d = k.kps3d; d.flags = k.flags; d.kf_id = k.keyframe_id; d.inl = k.inlier_count; d.color = k.color;
            for (const void* p : {(const void*)d.kps3d, (const void*)d.flags, (const void*)d.kf_id, (const void*)d.inl, (const void*)d.color})
                if ((k.n > 0 && !p) || ((uintptr_t)p & 3))
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
    if (bytes > h->scene_ws_bytes) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old block may still be read)
        h->scene_ws.reset();
        h->scene_ws_bytes = 0;
        HIP_TRY(dev_malloc(h->scene_ws, bytes));
        h->scene_ws_bytes = bytes;
    }
    const SceneSet* d_sets = reinterpret_cast<const SceneSet*>(h->scene_ws.get());
    const SceneImage* d_images = reinterpret_cast<const SceneImage*>(h->scene_ws.get() + sets_bytes);
    for (size_t i = 0; i < images.size(); i++) images[i].sets = d_sets + set0[i];
    if (!sets.empty()) HIP_TRY(hipMemcpyAsync(h->scene_ws.get(), sets.data(), sizeof(SceneSet) * sets.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->scene_ws.get() + sets_bytes, images.data(), sizeof(SceneImage) * images.size(), hipMemcpyHostToDevice, h->stream));
    const SceneParams params = scene_params(*style);
    std::vector<SceneTile> host(chunk);
    TileTable table{host.data(), reinterpret_cast<SceneTile*>(h->scene_ws.get() + sets_bytes + images_bytes), chunk, h->stream,
                    [&](const SceneTile* d, int m, hipStream_t s) { launch_scene(d, m, d_images, params, s); }};
    int rc = SVO_OK;
    for (size_t i = 0; i < tiles.size() && !rc; i++) rc = table.add(tiles[i]);
    if (!rc) rc = table.launch(false);
    const hipError_t e = hipStreamSynchronize(h->stream);   // (on every path: the uploads read host memory of this call)
    if (rc) return rc;
    HIP_TRY(e);
    return SVO_OK;
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
    if (chunk > h->copy_ws_count) {
        HIP_TRY(hipStreamSynchronize(h->stream));      // (the old table may still be read)
        h->copy_ws.reset();
        h->copy_ws_count = 0;
        HIP_TRY(dev_malloc(h->copy_ws, sizeof(CopyTile) * chunk));
        h->copy_ws_count = chunk;
    }
    std::vector<CopyTile> host(chunk);
    TileTable table{host.data(), h->copy_ws.get(), chunk, h->stream, &launch_copy_tiles};
    for (const CopyTile& t : tiles)
        if (const int rc = table.add(t)) return rc;
    if (const int rc = table.launch(false)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));          // (the table's upload read `host`)
    return SVO_OK;
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

extern "C" int svo_build_lk_pyramid(svo_handle* h, int max_levels, int win, svo_image* levels,
                                    int* n_out) {
    CHECK_H(h);
    if (!levels || max_levels < 1 || max_levels > SVO_LK_LEVELS)
        return svo_set_error(SVO_ERR_INVALID, "svo_build_lk_pyramid: max_levels must be 1..%d", SVO_LK_LEVELS);
    // cv::buildOpticalFlowPyramid stops when the next level is not larger than the window
    int n = max_levels, w = levels[0].width, hgt = levels[0].height;
    for (int l = 0; l < max_levels; l++) {
        if (l) { levels[l].width = w; levels[l].height = hgt; levels[l].stride = w; }
        w = (w + 1) / 2; hgt = (hgt + 1) / 2;
        if (w <= win || hgt <= win) { n = l + 1; break; }
    }
    PyrArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.n_levels = 1;
    pa.level[0] = make_view(levels[0]);
    pa.n_lk = n;
    for (int l = 0; l < n; l++) pa.lk[l] = make_view(levels[l]);
    PyrArgs* d;
    int rc = stage(h, pa, &d);
    if (rc) return rc;
    if (n > 1) launch_pyr_fused(d, 1, levels[0].width, levels[0].height, false, pyr_stream_rows(pa), h->stream);
    HIP_TRY(hipGetLastError());
    if (n_out) *n_out = n;
    return SVO_OK;
}

extern "C" int svo_sparse_align(svo_handle* h, const svo_image* prev_pyr, const svo_image* cur_pyr,
                                const svo_kp2d* kps2d, const svo_kp3d* kps3d, const uint32_t* flags,
                                int n, const svo_camera_settings* cam, const float* pose_guess,
                                float* pose_out, float* cost, svo_gn_trace* trace, float* dbg,
                                int dbg_level) {
    CHECK_H(h);
    if (!prev_pyr || !cur_pyr || !cam || !pose_guess || !pose_out || n < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align: bad arguments");
    if (n > h->max_kps) return svo_set_error(SVO_ERR_CAPACITY, "n=%d exceeds handle capacity %d", n, h->max_kps);
    if (cam->max_pyramid_levels < 1 || cam->max_pyramid_levels > 7 ||
        cam->min_pyramid_level_pose_estimation < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align: max_pyramid_levels must be 1..7");
    if (cam->window_size_pose_estimator != 4)   // PATCH_SIZE, src/lib/pose_estimator.cpp:68
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align: window_size_pose_estimator must be 4");
    SiaArgs sa;
    memset(&sa, 0, sizeof(sa));
    for (int l = 0; l < cam->max_pyramid_levels; l++) {
        sa.prev[l] = make_view(prev_pyr[l]);
        sa.cur[l] = make_view(cur_pyr[l]);
    }
    sa.cam = *cam;
    int* d_n;
    int rc = stage_n(h, n, &d_n);
    if (rc) return rc;
    sa.n_ptr = d_n;
    sa.kps2d = kps2d; sa.kps3d = kps3d; sa.flags = flags;
    sa.pose_guess = pose_guess; sa.pose_out = pose_out; sa.cost_out = cost; sa.trace = trace;
    sa.kp_ws = h->sia_kpws.get();
    sa.rec_ws = h->sia_rec.get(); sa.rec_cap = h->rec_cap;
    sa.dbg_H = dbg; sa.dbg_level = dbg_level;
    sa.cap = h->max_kps;
    sa.exact_pinv = h->exact_pinv;
    SiaArgs* d;
    rc = stage(h, sa, &d);
    if (rc) return rc;
    const LaunchStatus sia_launch =
        launch_sia(d, 1, *cam, cur_pyr[0].width, cur_pyr[0].height, n, h->rec_cap, h->exact_pinv, h->stream);
    HIP_TRY(sia_launch.err);
    if (!sia_launch.shape.fits) return svo_set_error(SVO_ERR_CAPACITY, "svo_sparse_align: %d keypoints exceed the workspaces", n);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_klt_track(svo_handle* h, const svo_image* prev_lk, const svo_image* cur_lk,
                             int n_levels, const svo_kp2d* prev_pts, svo_kp2d* cur_pts, int n, int win,
                             uint8_t* status, float* err) {
    CHECK_H(h);
    if (!prev_lk || !cur_lk || n_levels < 1 || n_levels > SVO_LK_LEVELS || n < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_klt_track: bad arguments");
    if (win < 3 || win > 35) return svo_set_error(SVO_ERR_INVALID, "svo_klt_track: window must be 3..35");
    KfDev kf;
    memset(&kf, 0, sizeof(kf));
    kf.n_lk = n_levels;
    for (int l = 0; l < n_levels; l++) kf.lk[l] = make_view(prev_lk[l]);
    KfDev* d_kf;
    int rc = stage(h, kf, &d_kf);
    if (rc) return rc;
    KltArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.kfs = d_kf; ka.kf_mask = -1;
    ka.n_cur = n_levels;
    for (int l = 0; l < n_levels; l++) ka.cur[l] = make_view(cur_lk[l]);
    int* d_n;
    rc = stage_n(h, n, &d_n);
    if (rc) return rc;
    ka.n_ptr = d_n;
    ka.prev_pts = prev_pts; ka.cur_pts = cur_pts; ka.status = status; ka.err = err; ka.win = win;
    KltArgs* d;
    rc = stage(h, ka, &d);
    if (rc) return rc;
    launch_klt(d, 1, n, win, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_reproj_gn(svo_handle* h, svo_kp2d* kps2d, const svo_kp3d* kps3d, uint32_t* flags,
                             int n, const svo_camera_settings* cam, const svo_kp2d* tracked,
                             const float* err, const float* pose_in, float* pose_out, float* cost,
                             svo_gn_trace* trace) {
    CHECK_H(h);
    if (!cam || !pose_in || !pose_out || n < 0) return svo_set_error(SVO_ERR_INVALID, "svo_reproj_gn: bad arguments");
    ReprojArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.cam = *cam;
    int* d_n;
    int rc = stage_n(h, n, &d_n);
    if (rc) return rc;
    ra.n_ptr = d_n;
    ra.kps2d = kps2d; ra.kps3d = kps3d; ra.flags = flags; ra.tracked = tracked; ra.err = err;
    ra.pose_in = pose_in; ra.pose_out = pose_out; ra.cost_out = cost; ra.trace = trace;
    ra.exact_pinv = h->exact_pinv;
    ReprojArgs* d;
    rc = stage(h, ra, &d);
    if (rc) return rc;
    const LaunchStatus reproj_launch = launch_reproj(d, 1, n, h->stream);
    HIP_TRY(reproj_launch.err);
    if (!reproj_launch.shape.fits) return svo_set_error(SVO_ERR_CAPACITY, "svo_reproj_gn: %d keypoints do not fit LDS", n);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_ssd_disparity(svo_handle* h, const svo_image* left, const svo_image* right,
                                 const svo_kp2d* kps2d, int n, int win, int search_x, int search_y,
                                 int clamp_half, float* disparity) {
    CHECK_H(h);
    if (!left || !right || n < 0) return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity: bad arguments");
    if (win < 1 || win > 35 || search_x < 0 || search_x > 64 || search_y < 0 || search_y > 8)
        return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity: win<=35, search_x<=64, search_y<=8 supported");
    SsdArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.left = make_view(*left); sa.right = make_view(*right);
    int* d_n;
    int rc = stage_n(h, n, &d_n);
    if (rc) return rc;
    sa.n_ptr = d_n; sa.kps2d = kps2d; sa.disparity = disparity;
    sa.win = win; sa.search_x = search_x; sa.search_y = search_y; sa.clamp_half = clamp_half;
    sa.first = 0;
    SsdArgs* d;
    rc = stage(h, sa, &d);
    if (rc) return rc;
    launch_ssd(d, 1, n, win, search_y, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_depth_filter_update(svo_handle* h, const svo_kp2d* kps2d, svo_kp3d* kps3d,
                                       const uint32_t* flags, int n, const svo_camera_settings* cam,
                                       const float* frame_pose, const float* disparity,
                                       const svo_kp3d* ref3d, const svo_kp2d* ref2d,
                                       const float* kf_pose, int32_t* outlier_count,
                                       int32_t* inlier_count, float* kf_inv_depth, float* kf_variance,
                                       int do_outlier_check, int do_update) {
    CHECK_H(h);
    if (!cam || !frame_pose || !kf_pose || n < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_depth_filter_update: bad arguments");
    FilterArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.cam = *cam;
    int* d_n;
    int rc = stage_n(h, n, &d_n);
    if (rc) return rc;
    fa.n_ptr = d_n;
    fa.frame_pose = frame_pose;
    fa.kps2d = const_cast<svo_kp2d*>(kps2d);
    fa.kps3d = kps3d;
    fa.flags = const_cast<uint32_t*>(flags);
    fa.outlier_count = outlier_count; fa.inlier_count = inlier_count;
    fa.kf_inv_depth = kf_inv_depth; fa.kf_variance = kf_variance;
    fa.disparity = disparity; fa.ref3d = ref3d; fa.ref2d = ref2d; fa.kf_pose = kf_pose;
    fa.do_outlier_check = do_outlier_check; fa.do_update = do_update;
    FilterArgs* d;
    rc = stage(h, fa, &d);
    if (rc) return rc;
    launch_filter(d, 1, n, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

// what CornerDetector::detect_keypoints has no value for: see include/svo_hip.h
static int check_detect_levels(const char* who, int n_levels, int grid_width, int grid_height) {
    if (n_levels < 1 || n_levels > SVO_MAX_PYRAMID_LEVELS)
        return svo_set_error(SVO_ERR_INVALID, "%s: n_levels must be 1..%d", who, SVO_MAX_PYRAMID_LEVELS);
    if (grid_width < 4 || grid_height < 4 || grid_width > 96 || grid_height > 64)
        return svo_set_error(SVO_ERR_INVALID, "%s: grid cell must be within 4..96 x 4..64", who);
    if ((grid_width >> (n_levels - 1)) == 0 || (grid_height >> (n_levels - 1)) == 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: the cell of level %d is empty", who, n_levels - 1);
    return SVO_OK;
}
static int detect_level_cells(const char* who, int l, int width, int height, int grid_width, int grid_height, int* cells) {
    const int gw = grid_width >> l, gh = grid_height >> l;
    if (width < 1 || height < gh)
        return svo_set_error(SVO_ERR_INVALID, "%s: level %d (%d x %d) is lower than its cell (%d x %d)", who, l, width, height, gw, gh);
    *cells = (width / gw) * (height / gh);
    return SVO_OK;
}

extern "C" int svo_detect_shape(int width, int height, int n_levels, int grid_width, int grid_height, int* max_cells,
                                int* cell_width, int* cell_height, int* list_capacity) {
    int rc = check_detect_levels("svo_detect_shape", n_levels, grid_width, grid_height);
    if (rc) return rc;
    int most = 1;
    for (int l = 0; l < n_levels; l++) {
        int nc;
        if ((rc = detect_level_cells("svo_detect_shape", l, width >> l, height >> l, grid_width, grid_height, &nc))) return rc;
        most = std::max(most, nc);
    }
    const DetectShape s = detect_pick_shape(grid_width, grid_height);
    if (max_cells) *max_cells = most;
    if (cell_width) *cell_width = s.cell_w;
    if (cell_height) *cell_height = s.cell_h;
    if (list_capacity) *list_capacity = s.list;
    return SVO_OK;
}

static_assert(sizeof(svo_det_cell) == sizeof(DetCell) && offsetof(svo_det_cell, score) == offsetof(DetCell, score) &&
              offsetof(svo_det_cell, type) == offsetof(DetCell, type), "svo_det_cell is the kernel's DetCell");

extern "C" int svo_detect_keypoints(svo_handle* h, int n_levels, const svo_image* levels, int grid_width, int grid_height,
                                    int max_cells, svo_det_cell* cells, int32_t* counts) {
    CHECK_H(h);
    if (!levels || !cells || !counts || max_cells < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_detect_keypoints: bad arguments");
    int rc = check_detect_levels("svo_detect_keypoints", n_levels, grid_width, grid_height);
    if (rc) return rc;
    DetectArgs da;
    memset(&da, 0, sizeof(da));
    for (int l = 0; l < n_levels; l++) {
        if (!levels[l].data || levels[l].stride < levels[l].width)
            return svo_set_error(SVO_ERR_INVALID, "svo_detect_keypoints: level %d: no data or stride < width", l);
        int nc;
        if ((rc = detect_level_cells("svo_detect_keypoints", l, levels[l].width, levels[l].height, grid_width, grid_height, &nc)))
            return rc;
        if (nc > max_cells)
            return svo_set_error(SVO_ERR_CAPACITY, "svo_detect_keypoints: level %d has %d cells, max_cells = %d", l, nc, max_cells);
        da.level[l] = make_view(levels[l]);
    }
    da.n_levels = n_levels; da.grid_w = grid_width; da.grid_h = grid_height;
    da.out = reinterpret_cast<DetCell*>(cells); da.n_out = counts; da.max_cells = max_cells;
    // (a level narrower than its cell has no cells and no workgroup that writes its count: the tracker clears the
    // counters in the compaction kernel that precedes the detection)
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_levels, h->stream));
    DetectArgs* d;
    rc = stage(h, da, &d);
    if (rc) return rc;
    launch_detect(d, 1, max_cells, n_levels, grid_width, grid_height, h->stream);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_pick_launch_shapes(const svo_camera_settings* cam, int width, int height, int batch, int n_bound,
                                      int rec_cap, int exact, svo_launch_shape out[2]) {
    if (!cam || !out || width < 1 || height < 1 || batch < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_pick_launch_shapes: bad arguments");
    const LaunchShape s = sia_pick_shape(batch, *cam, width, height, n_bound, rec_cap, exact);
    const LaunchShape r = reproj_pick_shape(batch, n_bound);
    out[0] = {SVO_KERNEL_SIA_GN, s.waves, s.mode, s.cap, s.fits ? 1 : 0};
    out[1] = {SVO_KERNEL_REPROJ_GN, r.waves, r.mode, r.cap, r.fits ? 1 : 0};
    return SVO_OK;
}

extern "C" int svo_pick_sia_lds_bytes(const svo_camera_settings* cam, int width, int height, int batch, int n_bound,
                                      int rec_cap, int exact, int64_t* lds_bytes) {
    if (!cam || !lds_bytes || width < 1 || height < 1 || batch < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_pick_sia_lds_bytes: bad arguments");
    *lds_bytes = (int64_t)sia_pick_shape(batch, *cam, width, height, n_bound, rec_cap, exact).lds;
    return SVO_OK;
}

// ------------------------------------------------------------------ diagnostics
// svo_pinv6_check: IMPL 0 runs jacobi_svd6_reg on one system per lane, IMPL 1 jacobi_svd6_lanes on one
// system per wavefront (H loaded alike by all 64 lanes: the wave-uniform input of the kernels' solves).
template <int IMPL>
__global__ void __launch_bounds__(64) pinv6_check_kernel(const float* H, int n, float* out, int32_t* sweeps) {
    const long sys = IMPL == 0 ? (long)blockIdx.x * 64 + threadIdx.x : (long)blockIdx.x;
    if (sys >= n) return;   // IMPL 1: never taken (one workgroup per system), the wave stays converged
    const float* h = H + sys * 36;
    float At[6][6], W[6], Vt[6][6], Hinv[36];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) At[i][j] = h[j * 6 + i];
    const int sw = IMPL == 0 ? jacobi_svd6_reg(At, W, Vt) : jacobi_svd6_lanes(At, W, Vt);
    svd6_pinv(At, W, Vt, Hinv);
    if (IMPL == 1 && threadIdx.x != 0) return;
    float* o = out + sys * 114;
#pragma unroll
    for (int i = 0; i < 36; i++) o[i] = Hinv[i];
#pragma unroll
    for (int i = 0; i < 6; i++) o[36 + i] = W[i];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k < 6; k++) { o[42 + i * 6 + k] = Vt[i][k]; o[78 + i * 6 + k] = At[i][k]; }
    sweeps[sys] = sw;
}

extern "C" int svo_pinv6_check(svo_handle* h, const float* H_dev, int n, float* out_dev, int32_t* sweeps_dev,
                               int impl) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!H_dev || !out_dev || !sweeps_dev)) || (impl != 0 && impl != 1))
        return svo_set_error(SVO_ERR_INVALID, "svo_pinv6_check: bad arguments");
    if (n == 0) return SVO_OK;
    if (impl == 0)
        pinv6_check_kernel<0><<<(n + 63) / 64, 64, 0, h->stream>>>(H_dev, n, out_dev, sweeps_dev);
    else
        pinv6_check_kernel<1><<<n, 64, 0, h->stream>>>(H_dev, n, out_dev, sweeps_dev);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

// svo_reproj_gn_batch / svo_filter_update_batch: launch_reproj and launch_filter with a batch of sequences, the way
// the tracker calls them, on caller-made arrays. The counts are read back and checked before the launch (a
// diagnostic may wait): a count beyond n_bound or the stride would make a block read its neighbour's arrays.
static int check_batch_counts(const char* who, int batch, int stride, const int32_t* n_dev, int n_bound) {
    if (batch < 1 || batch > 4096 || !n_dev || n_bound < 0 || stride < n_bound)
        return svo_set_error(SVO_ERR_INVALID, "%s: need 1 <= batch <= 4096, n_dev and 0 <= n_bound <= stride", who);
    std::vector<int32_t> n((size_t)batch);
    HIP_TRY(hipMemcpy(n.data(), n_dev, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; b++)
        if (n[(size_t)b] < 0 || n[(size_t)b] > n_bound)
            return svo_set_error(SVO_ERR_INVALID, "%s: n_dev[%d] = %d is outside 0..n_bound = %d", who, b, n[(size_t)b], n_bound);
    return SVO_OK;
}

template <typename T>
static int stage_blocks(svo_handle* h, const std::vector<T>& host, T** dev) {
    const size_t bytes = (sizeof(T) * host.size() + 255) & ~(size_t)255;
    if (bytes > h->ring_cap) return svo_set_error(SVO_ERR_CAPACITY, "argument blocks do not fit the ring");
    if (h->ring_off + bytes > h->ring_cap) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->ring_off = 0;
    }
    T* d = reinterpret_cast<T*>(h->ring.get() + h->ring_off);
    h->ring_off += bytes;
    HIP_TRY(hipMemcpyAsync(d, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice, h->stream));
    *dev = d;
    return SVO_OK;
}

extern "C" int svo_reproj_gn_batch(svo_handle* h, int batch, int stride, const int32_t* n_dev, int n_bound, svo_kp2d* kps2d,
                                   const svo_kp3d* kps3d, uint32_t* flags, const svo_camera_settings* cam,
                                   const svo_kp2d* tracked, const float* err, const float* pose_in, float* pose_out,
                                   float* cost, svo_gn_trace* trace, int32_t* zero_out, int* waves, int* cap) {
    CHECK_H(h);
    if (!cam || !pose_in || !pose_out || (n_bound > 0 && (!kps2d || !kps3d || !flags)) || (!tracked != !err))
        return svo_set_error(SVO_ERR_INVALID, "svo_reproj_gn_batch: bad arguments");
    int rc = check_batch_counts("svo_reproj_gn_batch", batch, stride, n_dev, n_bound);
    if (rc) return rc;
    std::vector<ReprojArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        ReprojArgs& ra = blocks[(size_t)b];
        const size_t o = (size_t)b * (size_t)stride;
        memset(&ra, 0, sizeof(ra));
        ra.cam = *cam;
        ra.n_ptr = n_dev + b;
        ra.kps2d = kps2d + o; ra.kps3d = kps3d + o; ra.flags = flags + o;
        ra.tracked = tracked ? tracked + o : nullptr; ra.err = err ? err + o : nullptr;
        ra.pose_in = pose_in + 6 * (size_t)b; ra.pose_out = pose_out + 6 * (size_t)b;
        ra.cost_out = cost ? cost + b : nullptr; ra.trace = trace ? trace + b : nullptr;
        ra.exact_pinv = h->exact_pinv;
        ra.zero_out = zero_out ? zero_out + b : nullptr;
    }
    ReprojArgs* d;
    rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    const LaunchStatus st = launch_reproj(d, batch, n_bound, h->stream);
    HIP_TRY(st.err);
    if (waves) *waves = st.shape.waves;
    if (cap) *cap = st.shape.cap;
    if (!st.shape.fits) return svo_set_error(SVO_ERR_CAPACITY, "svo_reproj_gn_batch: %d keypoints do not fit LDS", n_bound);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;
}

// svo_sparse_align_batch: launch_sia with a batch of sequences, the way the tracker calls it, on caller-made
// arrays. Every sequence gets record and per-keypoint workspaces of its own for the call ([levels used][68][rec_cap]
// and [9][rec_cap] floats, rec_cap the multiple of 256 that covers the launch's cap), filled with ws_fill first: what
// a kernel reads of a slot that nothing wrote is the caller's pattern.
// mats_out: null, or [batch] blocks of sizeof(PoseMats) (svo_pose_mats_layout), SiaArgs::mats_out of every sequence:
// what the tracker's KLT launch projects with (svo_sparse_align_batch_mats)
static int sparse_align_batch(svo_handle* h, int batch, int stride, const int32_t* n_dev, int n_bound,
                              const svo_kp2d* kps2d, const svo_kp3d* kps3d, const uint32_t* flags,
                              const svo_image* prev_pyr, const svo_image* cur_pyr,
                              const svo_camera_settings* cam, const float* pose_guess, int dbg_level,
                              uint32_t ws_fill, float* pose_out, float* cost, svo_gn_trace* trace, float* dbg,
                              int* waves, int* mode, int* cap, PoseMats* mats_out) {
    CHECK_H(h);
    if (!cam || !prev_pyr || !cur_pyr || !pose_guess || !pose_out || (n_bound > 0 && (!kps2d || !kps3d)))
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align_batch: bad arguments");
    if (cam->max_pyramid_levels < 1 || cam->max_pyramid_levels > 7 || cam->min_pyramid_level_pose_estimation < 0 ||
        cam->min_pyramid_level_pose_estimation >= cam->max_pyramid_levels)
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align_batch: max_pyramid_levels must be 1..7, min below it");
    if (cam->window_size_pose_estimator != 4)
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align_batch: window_size_pose_estimator must be 4");
    int rc = check_batch_counts("svo_sparse_align_batch", batch, stride, n_dev, n_bound);
    if (rc) return rc;
    const int levels = cam->max_pyramid_levels;
    const int width = cur_pyr[0].width, height = cur_pyr[0].height;      // (level 0 gives the size even where it is not used)
    if (width < 1 || height < 1) return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align_batch: cur_pyr[0] has no size");
    for (int b = 0; b < batch; b++)
        for (int l = cam->min_pyramid_level_pose_estimation; l < levels; l++) {
            const svo_image& p = prev_pyr[(size_t)b * levels + l];
            const svo_image& c = cur_pyr[(size_t)b * levels + l];
            if (!p.data || !c.data || p.width != (width >> l) || c.width != (width >> l) || p.height != (height >> l) ||
                c.height != (height >> l) || p.stride < p.width || c.stride < c.width)
                return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align_batch: sequence %d level %d: every sequence needs "
                                     "images of one size, %d x %d at level 0", b, l, width, height);
        }
    const LaunchShape want = sia_pick_shape(batch, *cam, width, height, n_bound, INT_MAX, h->exact_pinv);
    if (waves) *waves = want.waves;
    if (mode) *mode = want.mode;
    if (cap) *cap = want.cap;
    if (!want.fits || want.cap > INT_MAX - 255)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_sparse_align_batch: %d keypoints exceed the kernel's LDS", n_bound);
    const int rec_cap = (want.cap + 255) / 256 * 256;
    const size_t rec_floats = sia_rec_ws_floats(*cam, rec_cap), kp_floats = (size_t)9 * rec_cap;
    DevPtr<float> ws;
    HIP_TRY(dev_malloc(ws, sizeof(float) * (rec_floats + kp_floats) * (size_t)batch));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws.get()), (int)ws_fill,
                              (rec_floats + kp_floats) * (size_t)batch, h->stream));
    std::vector<SiaArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        SiaArgs& sa = blocks[(size_t)b];
        const size_t o = (size_t)b * (size_t)stride;
        memset(&sa, 0, sizeof(sa));
        for (int l = cam->min_pyramid_level_pose_estimation; l < levels; l++) {      // (the levels checked above: the others are not read)
            sa.prev[l] = make_view(prev_pyr[(size_t)b * levels + l]);
            sa.cur[l] = make_view(cur_pyr[(size_t)b * levels + l]);
        }
        sa.cam = *cam;
        sa.n_ptr = n_dev + b;
        sa.kps2d = kps2d ? kps2d + o : nullptr; sa.kps3d = kps3d ? kps3d + o : nullptr;
        sa.flags = flags ? flags + o : nullptr;
        sa.pose_guess = pose_guess + 6 * (size_t)b; sa.pose_out = pose_out + 6 * (size_t)b;
        sa.cost_out = cost ? cost + b : nullptr;
        sa.trace = trace ? trace + (size_t)b * SVO_MAX_PYRAMID_LEVELS : nullptr;
        sa.rec_ws = ws.get() + (size_t)b * (rec_floats + kp_floats);
        sa.kp_ws = sa.rec_ws + rec_floats;
        sa.rec_cap = rec_cap;
        sa.dbg_H = dbg ? dbg + 48 * (size_t)b : nullptr; sa.dbg_level = dbg_level;
        sa.cap = stride;
        sa.exact_pinv = h->exact_pinv;
        sa.mats_out = mats_out ? mats_out + b : nullptr;
    }
    SiaArgs* d;
    rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    const LaunchStatus st = launch_sia(d, batch, *cam, width, height, n_bound, rec_cap, h->exact_pinv, h->stream);
    HIP_TRY(st.err);
    if (!st.shape.fits) {
        (void)hipStreamSynchronize(h->stream);
        return svo_set_error(SVO_ERR_CAPACITY, "svo_sparse_align_batch: %d keypoints exceed the kernel's LDS or registers", n_bound);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;            // (ws is freed here: the launch is complete)
}

extern "C" int svo_sparse_align_batch(svo_handle* h, int batch, int stride, const int32_t* n_dev, int n_bound,
                                      const svo_kp2d* kps2d, const svo_kp3d* kps3d, const uint32_t* flags,
                                      const svo_image* prev_pyr, const svo_image* cur_pyr,
                                      const svo_camera_settings* cam, const float* pose_guess, int dbg_level,
                                      uint32_t ws_fill, float* pose_out, float* cost, svo_gn_trace* trace, float* dbg,
                                      int* waves, int* mode, int* cap) {
    return sparse_align_batch(h, batch, stride, n_dev, n_bound, kps2d, kps3d, flags, prev_pyr, cur_pyr, cam, pose_guess,
                              dbg_level, ws_fill, pose_out, cost, trace, dbg, waves, mode, cap, nullptr);
}

extern "C" int svo_sparse_align_batch_mats(svo_handle* h, int batch, int stride, const int32_t* n_dev, int n_bound,
                                           const svo_kp2d* kps2d, const svo_kp3d* kps3d, const uint32_t* flags,
                                           const svo_image* prev_pyr, const svo_image* cur_pyr,
                                           const svo_camera_settings* cam, const float* pose_guess, int dbg_level,
                                           uint32_t ws_fill, float* pose_out, float* cost, svo_gn_trace* trace, float* dbg,
                                           int* waves, int* mode, int* cap, void* mats_out) {
    if (!mats_out || (reinterpret_cast<uintptr_t>(mats_out) & (alignof(PoseMats) - 1)))
        return svo_set_error(SVO_ERR_INVALID, "svo_sparse_align_batch_mats: mats_out must be %zu-byte aligned device memory",
                             alignof(PoseMats));
    return sparse_align_batch(h, batch, stride, n_dev, n_bound, kps2d, kps3d, flags, prev_pyr, cur_pyr, cam, pose_guess,
                              dbg_level, ws_fill, pose_out, cost, trace, dbg, waves, mode, cap, static_cast<PoseMats*>(mats_out));
}

extern "C" int svo_pose_mats_layout(int64_t* block_bytes, int64_t* rd_offset, int64_t* r_offset, int64_t* ri_offset,
                                    int64_t* t_offset) {
    if (block_bytes) *block_bytes = (int64_t)sizeof(PoseMats);
    if (rd_offset) *rd_offset = (int64_t)offsetof(PoseMats, Rd);
    if (r_offset) *r_offset = (int64_t)offsetof(PoseMats, R);
    if (ri_offset) *ri_offset = (int64_t)offsetof(PoseMats, Ri);
    if (t_offset) *t_offset = (int64_t)offsetof(PoseMats, t);
    return SVO_OK;
}

extern "C" int svo_filter_update_batch(svo_handle* h, int batch, int stride, const int32_t* n_dev, int n_bound, svo_kp2d* kps2d,
                                       svo_kp3d* kps3d, uint32_t* flags, const svo_camera_settings* cam,
                                       const float* frame_pose, const float* disparity, const svo_kp3d* ref3d,
                                       const svo_kp2d* ref2d, const float* kf_pose, int32_t* outlier_count,
                                       int32_t* inlier_count, float* kf_inv_depth, float* kf_variance,
                                       int do_outlier_check, int do_update, int do_flags, int do_reproject, int width,
                                       int height, int32_t* inside_count) {
    CHECK_H(h);
    if (!cam || !frame_pose || !kf_pose || !kps2d || !kps3d || !flags || !outlier_count || !inlier_count ||
        !kf_inv_depth || !kf_variance || (do_outlier_check && !disparity))
        return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_batch: bad arguments");
    int rc = check_batch_counts("svo_filter_update_batch", batch, stride, n_dev, n_bound);
    if (rc) return rc;
    std::vector<FilterArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        FilterArgs& fa = blocks[(size_t)b];
        const size_t o = (size_t)b * (size_t)stride;
        memset(&fa, 0, sizeof(fa));
        fa.cam = *cam;
        fa.n_ptr = n_dev + b;
        fa.frame_pose = frame_pose + 6 * (size_t)b;
        fa.kps2d = kps2d + o; fa.kps3d = kps3d + o; fa.flags = flags + o;
        fa.outlier_count = outlier_count + o; fa.inlier_count = inlier_count + o;
        fa.kf_inv_depth = kf_inv_depth + o; fa.kf_variance = kf_variance + o;
        fa.disparity = disparity ? disparity + o : nullptr;
        fa.ref3d = ref3d ? ref3d + o : nullptr; fa.ref2d = ref2d ? ref2d + o : nullptr;
        fa.kf_pose = kf_pose + 6 * o;
        fa.do_outlier_check = do_outlier_check; fa.do_update = do_update;
        fa.do_flags = do_flags; fa.do_reproject = do_reproject;
        fa.width = width; fa.height = height;
        fa.inside_count = inside_count ? inside_count + b : nullptr;
    }
    FilterArgs* d;
    rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    launch_filter(d, batch, n_bound, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SVO_OK;
}

// svo_solve6_check: the exact Gauss-Newton solve delta = pinv(H) b, one system per wavefront (H and b loaded
// alike by all 64 lanes). IMPL 0 is the round-4 solve: jacobi_svd6_lanes, then svd6_pinv and delta = Hinv b
// on wave-uniform values. IMPL 1 is the kernels' solve: svd6_sweeps_lanes + svd6_tail_lanes, every element
// in its own lane. Output per system (120 floats): Hinv, W, Vt, U^T, delta.
template <int IMPL>
__global__ void __launch_bounds__(64) solve6_check_kernel(const float* H, const float* B, int n, float* out,
                                                          int32_t* sweeps) {
    const long sys = (long)blockIdx.x;
    if (sys >= n) return;   // never taken (one workgroup per system): the wave stays converged
    const float* h = H + sys * 36;
    const float* b = B + sys * 6;
    float* o = out + sys * 120;
    const int lane = threadIdx.x;
    if constexpr (IMPL == 0) {
        float At[6][6], W[6], Vt[6][6], Hinv[36], delta[6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) At[i][j] = h[j * 6 + i];
        const int sw = jacobi_svd6_lanes(At, W, Vt);
        svd6_pinv(At, W, Vt, Hinv);
#pragma unroll
        for (int r = 0; r < 6; r++) {
            float sacc = 0;
#pragma unroll
            for (int c = 0; c < 6; c++) sacc += Hinv[r * 6 + c] * b[c];
            delta[r] = sacc;
        }
        if (lane != 0) return;
#pragma unroll
        for (int i = 0; i < 36; i++) o[i] = Hinv[i];
#pragma unroll
        for (int i = 0; i < 6; i++) o[36 + i] = W[i];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) { o[42 + i * 6 + k] = Vt[i][k]; o[78 + i * 6 + k] = At[i][k]; }
#pragma unroll
        for (int i = 0; i < 6; i++) o[114 + i] = delta[i];
        sweeps[sys] = sw;
    } else {
        const int r = lane & 7;
        float a[6], v[6], delta[6];
#pragma unroll
        for (int k = 0; k < 6; k++) a[k] = r < 6 ? h[k * 6 + r] : 0.f;
        const float b_j = b[(lane < 36 ? lane : 35) % 6];
        const int sw = svd6_sweeps_lanes(a, v);
        Solve6Lane e;
        svd6_tail_lanes(a, v, b_j, delta, &e);
        if (lane < 36) {
            o[lane] = e.hinv;
            o[42 + lane] = e.vt;
            o[78 + lane] = e.ut;
            if (lane % 6 == 0) o[36 + lane / 6] = e.w;
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 6; i++) o[114 + i] = delta[i];
            sweeps[sys] = sw;
        }
    }
}

extern "C" int svo_solve6_check(svo_handle* h, const float* H_dev, const float* b_dev, int n, float* out_dev,
                                int32_t* sweeps_dev, int impl) {
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!H_dev || !b_dev || !out_dev || !sweeps_dev)) || (impl != 0 && impl != 1))
        return svo_set_error(SVO_ERR_INVALID, "svo_solve6_check: bad arguments");
    if (n == 0) return SVO_OK;
    if (impl == 0)
        solve6_check_kernel<0><<<n, 64, 0, h->stream>>>(H_dev, b_dev, n, out_dev, sweeps_dev);
    else
        solve6_check_kernel<1><<<n, 64, 0, h->stream>>>(H_dev, b_dev, n, out_dev, sweeps_dev);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

// svo_klt_track_batch: launch_klt with a batch of sequences, its argument blocks filled the way pack_tracking_args
// (svo_group_step.hip) fills them: the fused projection through proj_mats or proj_pose, the reference position
// gathered from the keyframe table, the keyframe's template cache. The table, the cache blocks and every array are
// the caller's; the counts and the two index arrays are read back and checked before the launch (a diagnostic may
// wait): an index beyond a keyframe's arrays would make a workgroup read or write a neighbour's memory.
__global__ void klt_pose_mats_kernel(const float* const* poses, PoseMats* out) {
    pose_mats(poses[blockIdx.x], out[blockIdx.x]);
}

static_assert(sizeof(svo_klt_keyframe) == 128 && sizeof(svo_klt_sequence) == 248, "the layouts the Python binding restates");
static bool klt_bad_view(const svo_image& v) { return !v.data || v.width < 1 || v.height < 1 || v.stride < v.width; }

extern "C" int svo_klt_track_batch(svo_handle* h, int batch, const svo_klt_sequence* seqs, int n_bound, int win,
                                   int use_mats) {
    CHECK_H(h);
    if (batch < 1 || batch > 4096 || !seqs || n_bound < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: need 1 <= batch <= 4096, seqs and n_bound >= 0");
    if (win < 3 || win > 35) return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: window must be 3..35");
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the caller's arrays are read back below)
    const size_t rec_bytes = klt_template_bytes(win);
    std::vector<KfDev> table;
    std::vector<size_t> first_kf((size_t)batch);
    std::vector<int32_t> idx, ids;
    for (int b = 0; b < batch; b++) {
        const svo_klt_sequence& s = seqs[b];
        if (!s.kfs || s.n_kfs < 1 || s.n_kfs > 8 || s.n_cur < 1 || s.n_cur > SVO_LK_LEVELS || !s.n || !s.pose ||
            (n_bound > 0 && (!s.kp_index || !s.kps3d || !s.tracked || !s.status || !s.err || !s.proj_out)))
            return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d: bad arguments", b);
        for (int l = 0; l < s.n_cur; l++)
            if (klt_bad_view(s.cur[l])) return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d: current level %d", b, l);
        first_kf[(size_t)b] = table.size();
        for (int k = 0; k < s.n_kfs; k++) {
            const svo_klt_keyframe& f = s.kfs[k];
            if (f.n_lk < 1 || f.n_lk > SVO_LK_LEVELS || f.n_kps < 0 || (f.n_kps > 0 && !f.kps2d))
                return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d keyframe %d: bad arguments", b, k);
            for (int l = 0; l < f.n_lk; l++)
                if (klt_bad_view(f.lk[l]))
                    return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d keyframe %d: level %d", b, k, l);
            if (f.tmpl && f.tmpl_win == win) {       // a cache that the kernel will use
                const int64_t recs = (int64_t)f.tmpl_cap * SVO_LK_LEVELS;
                if (f.tmpl_cap < 0 || !f.tmpl_valid || f.tmpl_valid_bytes < recs || f.tmpl_bytes < recs * (int64_t)rec_bytes ||
                    (reinterpret_cast<uintptr_t>(f.tmpl) & 15))
                    return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d keyframe %d: the cache needs %lld "
                                         "records of %zu bytes, 16-byte aligned, and as many flags", b, k, (long long)recs, rec_bytes);
            }
            KfDev kf;
            memset(&kf, 0, sizeof(kf));
            kf.n_lk = f.n_lk;
            for (int l = 0; l < f.n_lk; l++) kf.lk[l] = make_view(f.lk[l]);
            kf.kps2d = const_cast<svo_kp2d*>(f.kps2d);
            kf.n = f.n_kps;
            kf.tmpl = f.tmpl; kf.tmpl_valid = f.tmpl_valid; kf.tmpl_cap = f.tmpl_cap; kf.tmpl_win = f.tmpl_win;
            table.push_back(kf);
        }
        int32_t n = 0;
        HIP_TRY(hipMemcpy(&n, s.n, sizeof(n), hipMemcpyDeviceToHost));
        if (n < 0 || n > n_bound)
            return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d: n = %d is outside 0..n_bound = %d", b, n, n_bound);
        idx.resize((size_t)n); ids.assign((size_t)n, 0);
        if (n > 0) {
            HIP_TRY(hipMemcpy(idx.data(), s.kp_index, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
            if (s.kf_id) HIP_TRY(hipMemcpy(ids.data(), s.kf_id, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        }
        for (int i = 0; i < n; i++)
            if (ids[(size_t)i] < 0 || ids[(size_t)i] >= s.n_kfs || idx[(size_t)i] < 0 || idx[(size_t)i] >= s.kfs[ids[(size_t)i]].n_kps)
                return svo_set_error(SVO_ERR_INVALID, "svo_klt_track_batch: sequence %d point %d: keyframe %d, index %d", b, i,
                                     ids[(size_t)i], idx[(size_t)i]);
    }
    KfDev* d_table;
    int rc = stage_blocks(h, table, &d_table);
    if (rc) return rc;
    DevPtr<PoseMats> mats;
    if (use_mats) {
        std::vector<const float*> poses((size_t)batch);
        for (int b = 0; b < batch; b++) poses[(size_t)b] = seqs[b].pose;
        const float** d_poses;
        rc = stage_blocks(h, poses, &d_poses);
        if (rc) return rc;
        HIP_TRY(dev_malloc(mats, sizeof(PoseMats) * (size_t)batch));
        klt_pose_mats_kernel<<<batch, 1, 0, h->stream>>>(d_poses, mats.get());
        HIP_TRY(hipGetLastError());
    }
    std::vector<KltArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_klt_sequence& s = seqs[b];
        KltArgs& ka = blocks[(size_t)b];
        memset(&ka, 0, sizeof(ka));
        ka.kfs = d_table + first_kf[(size_t)b]; ka.kf_mask = -1; ka.kf_id = s.kf_id; ka.n_cur = s.n_cur;
        for (int l = 0; l < s.n_cur; l++) ka.cur[l] = make_view(s.cur[l]);
        ka.n_ptr = s.n; ka.prev_pts = nullptr; ka.cur_pts = s.tracked; ka.status = s.status;
        ka.err = s.err; ka.win = win;
        ka.proj_pose = s.pose; ka.proj_mats = use_mats ? mats.get() + b : nullptr; ka.kps3d = s.kps3d; ka.proj_out = s.proj_out;
        ka.kp_index = s.kp_index; ka.ref_out = s.ref_out; ka.cam = s.cam;
    }
    KltArgs* d;
    rc = stage_blocks(h, blocks, &d);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    launch_klt(d, batch, n_bound, win, h->stream);
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipStreamSynchronize(h->stream));      // (mats is freed on return: the launch is complete)
    HIP_TRY(launched);
    return SVO_OK;
}

extern "C" int svo_klt_cache_layout(int win, int64_t* record_bytes, int64_t* header_offset, int64_t* header_bytes, int* levels) {
    if (win < 3 || win > 35) return svo_set_error(SVO_ERR_INVALID, "svo_klt_cache_layout: window must be 3..35");
    if (record_bytes) *record_bytes = (int64_t)klt_template_bytes(win);
    if (header_offset) *header_offset = (int64_t)klt_template_header_offset(win);
    if (header_bytes) *header_bytes = (int64_t)klt_template_header_bytes();
    if (levels) *levels = SVO_LK_LEVELS;
    return SVO_OK;
}

// svo_compact_batch, svo_keyframe_merge_batch, svo_keyframe_init_batch, svo_ssd_disparity_batch: the four bookkeeping
// launches of the keyframe path with their argument blocks filled the way pack_compact, pack_keyframe_args and
// pack_ssd (svo_group_step.hip) fill them, through the tracker's launchers, over the caller's memory. What a kernel
// indexes with is read back and checked first (a diagnostic may wait): a count beyond the capacity would make a
// workgroup read or write a neighbour's memory.
static_assert(sizeof(svo_kps_planes) == 104 && sizeof(svo_compact_sequence) == 264 && sizeof(svo_merge_sequence) == 272 &&
              sizeof(svo_kf_init_sequence) == 400 && sizeof(svo_ssd_sequence) == 112, "the layouts the Python binding restates");

static KpsDev kps_dev(const svo_kps_planes& p) {
    KpsDev k;
    k.kps2d = p.kps2d; k.kps3d = p.kps3d; k.flags = p.flags; k.kf_id = p.kf_id; k.kp_index = p.kp_index;
    k.outl = p.outlier_count; k.inl = p.inlier_count; k.kfx = p.kf_inv_depth; k.kfP = p.kf_variance;
    k.score = p.score; k.level_type = p.level_type; k.color = p.color; k.n = p.n;
    return k;
}
static bool planes_missing(const svo_kps_planes& p, bool need_n) {
    return !p.kps2d || !p.kps3d || !p.flags || !p.kf_id || !p.kp_index || !p.outlier_count || !p.inlier_count ||
           !p.kf_inv_depth || !p.kf_variance || !p.score || !p.level_type || !p.color || (need_n && !p.n);
}
static int read_i32(const int32_t* dev, int count, int32_t* out) {
    HIP_TRY(hipMemcpy(out, dev, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost));
    return SVO_OK;
}
// launch done: the first error of the launch or the wait
static int finish_launch(svo_handle* h) {
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(launched);
    return SVO_OK;
}

extern "C" int svo_keyframe_launch_info(int cap, int max_cells, int tmpl_cap, int* compact_threads, int* merge_threads,
                                        int64_t* tmpl_valid_bytes) {
    if (cap < 1 || max_cells < 1 || tmpl_cap < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_launch_info: need cap >= 1, max_cells >= 1, tmpl_cap >= 0");
    if (compact_threads) *compact_threads = compact_pick_threads(cap);
    if (merge_threads) *merge_threads = select_merge_pick_threads(max_cells);
    if (tmpl_valid_bytes) *tmpl_valid_bytes = (int64_t)kf_tmpl_valid_bytes(tmpl_cap);
    return SVO_OK;
}

extern "C" int svo_compact_batch(svo_handle* h, int batch, const svo_compact_sequence* seqs, int cap, int* threads) {
    CHECK_H(h);
    if (batch < 1 || batch > 4096 || !seqs || cap < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_compact_batch: need 1 <= batch <= 4096, seqs and cap >= 1");
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the caller's counts are read back below)
    std::vector<CompactArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_compact_sequence& s = seqs[b];
        if (planes_missing(s.src, true) || planes_missing(s.dst, true) || (s.mode != 0 && s.mode != 1) ||
            (s.start != 0 && s.start != 1) || s.zero_count < 0 || s.zero_res_count < 0 || (s.zero_count > 0 && !s.zero) ||
            (s.zero_res_count > 0 && !s.zero_res))
            return svo_set_error(SVO_ERR_INVALID, "svo_compact_batch: sequence %d: bad arguments", b);
        if (s.min_kf && s.mode != 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_compact_batch: sequence %d: min_kf is defined for mode 0 only", b);
        if (!s.start) {
            int32_t n = 0;
            if (const int rc = read_i32(s.src.n, 1, &n)) return rc;
            if (n < 0 || n > cap)
                return svo_set_error(SVO_ERR_INVALID, "svo_compact_batch: sequence %d: n = %d is outside 0..cap = %d", b, n, cap);
        }
        CompactArgs& ca = blocks[(size_t)b];
        memset(&ca, 0, sizeof(ca));
        ca.src = kps_dev(s.src); ca.dst = kps_dev(s.dst); ca.mode = s.mode;
        ca.width = s.width; ca.height = s.height;
        ca.enable = s.enable;
        ca.zero = s.zero; ca.zero_count = s.zero_count;
        ca.start = s.start;
        ca.zero_res = s.zero_res; ca.zero_res_count = s.zero_res_count;
        ca.min_kf = s.min_kf;
    }
    CompactArgs* d;
    const int rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    if (threads) *threads = compact_pick_threads(cap);
    launch_compact(d, batch, cap, h->stream);
    return finish_launch(h);
}

extern "C" int svo_keyframe_merge_batch(svo_handle* h, int batch, const svo_merge_sequence* seqs, int n_levels,
                                        int max_cells, int cap, int* threads) {
    CHECK_H(h);
    if (batch < 1 || batch > 4096 || !seqs || n_levels < 1 || n_levels > SVO_MAX_PYRAMID_LEVELS || max_cells < 1 || cap < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_merge_batch: need 1 <= batch <= 4096, seqs, n_levels 1..%d, "
                             "max_cells >= 1 and cap >= 1", SVO_MAX_PYRAMID_LEVELS);
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<MergeArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_merge_sequence& s = seqs[b];
        if (planes_missing(s.kps, true) || !s.det || !s.n_det || !s.sel || !s.sel_level || !s.sel_cell || !s.occupied ||
            !s.old_count || !s.overflow || s.width < 1 || s.height < 1 || s.cam.grid_width < 1 || s.cam.grid_height < 1)
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_merge_batch: sequence %d: bad arguments", b);
        // (the kernel's grid: cells of grid_height x grid_width, the swap of depth_calculator.cpp:179-180)
        const int64_t cells = ((int64_t)(s.width + s.cam.grid_height - 1) / s.cam.grid_height) *
                              ((int64_t)(s.height + s.cam.grid_width - 1) / s.cam.grid_width);
        if (cells > s.occupied_count)
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_merge_batch: sequence %d: %lld merge cells, occupied holds %d", b,
                                 (long long)cells, s.occupied_count);
        int32_t nd[SVO_MAX_PYRAMID_LEVELS], n = 0;
        if (const int rc = read_i32(s.n_det, n_levels, nd)) return rc;
        if (const int rc = read_i32(s.kps.n, 1, &n)) return rc;
        for (int l = 0; l < n_levels; l++)
            if (nd[l] < 0 || nd[l] > max_cells)
                return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_merge_batch: sequence %d: n_det[%d] = %d is outside "
                                     "0..max_cells = %d", b, l, nd[l], max_cells);
        if (n < 0 || n > cap)
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_merge_batch: sequence %d: n = %d is outside 0..cap = %d", b, n, cap);
        MergeArgs& ma = blocks[(size_t)b];
        memset(&ma, 0, sizeof(ma));
        ma.cam = s.cam; ma.width = s.width; ma.height = s.height;
        ma.det = reinterpret_cast<const DetCell*>(s.det); ma.n_det = s.n_det; ma.n_levels = n_levels; ma.max_cells = max_cells;
        ma.kps = kps_dev(s.kps); ma.cap = cap;
        ma.sel = reinterpret_cast<DetCell*>(s.sel); ma.sel_level = s.sel_level; ma.sel_cell = s.sel_cell; ma.occupied = s.occupied;
        ma.old_count = s.old_count; ma.overflow = s.overflow;
        ma.enable = s.enable;
    }
    MergeArgs* d;
    const int rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    if (threads) *threads = select_merge_pick_threads(max_cells);
    launch_select_merge(d, batch, max_cells, h->stream);
    return finish_launch(h);
}

extern "C" int svo_keyframe_record_layout(int64_t* record_bytes, int64_t* n_offset, int64_t* pose_offset, int64_t* tmpl_offset,
                                          int64_t* tmpl_valid_offset, int64_t* tmpl_cap_offset, int64_t* tmpl_win_offset,
                                          int64_t plane_offsets[12]) {
    if (record_bytes) *record_bytes = (int64_t)sizeof(KfDev);
    if (n_offset) *n_offset = (int64_t)offsetof(KfDev, n);
    if (pose_offset) *pose_offset = (int64_t)offsetof(KfDev, pose);
    if (tmpl_offset) *tmpl_offset = (int64_t)offsetof(KfDev, tmpl);
    if (tmpl_valid_offset) *tmpl_valid_offset = (int64_t)offsetof(KfDev, tmpl_valid);
    if (tmpl_cap_offset) *tmpl_cap_offset = (int64_t)offsetof(KfDev, tmpl_cap);
    if (tmpl_win_offset) *tmpl_win_offset = (int64_t)offsetof(KfDev, tmpl_win);
    if (plane_offsets) {       // in the order of svo_kps_planes
        const size_t o[12] = {offsetof(KfDev, kps2d), offsetof(KfDev, kps3d), offsetof(KfDev, flags), offsetof(KfDev, kf_id),
                              offsetof(KfDev, kp_index), offsetof(KfDev, outlier_count), offsetof(KfDev, inlier_count),
                              offsetof(KfDev, kfx), offsetof(KfDev, kfP), offsetof(KfDev, score), offsetof(KfDev, level_type),
                              offsetof(KfDev, color)};
        for (int i = 0; i < 12; i++) plane_offsets[i] = (int64_t)o[i];
    }
    return SVO_OK;
}

extern "C" int svo_keyframe_init_batch(svo_handle* h, int batch, const svo_kf_init_sequence* seqs, int cap) {
    CHECK_H(h);
    if (batch < 1 || batch > 4096 || !seqs || cap < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_init_batch: need 1 <= batch <= 4096, seqs and cap >= 1");
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<KfInitArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_kf_init_sequence& s = seqs[b];
        if (planes_missing(s.kps, true) || planes_missing(s.record, false) || !s.old_count || !s.disparity || !s.kfs ||
            !s.color_lcg || !s.n_out || (!s.first_frame && !s.frame_pose) || (s.first_frame != 0 && s.first_frame != 1) ||
            s.new_kf_id < 0 || s.evict_id < -1)
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_init_batch: sequence %d: bad arguments", b);
        if (s.kf_mask < 0 || s.kf_mask > (1 << 20) || ((s.kf_mask + 1) & s.kf_mask) != 0 ||
            (int64_t)(s.kf_mask + 1) * (int64_t)sizeof(KfDev) > s.kfs_bytes || (reinterpret_cast<uintptr_t>(s.kfs) & 7))
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_init_batch: sequence %d: the table needs kf_mask + 1 = a power "
                                 "of two records of %zu bytes, 8-byte aligned", b, sizeof(KfDev));
        if (s.tmpl_valid_bytes < 0 || s.tmpl_valid_bytes % 4 != 0 || (s.tmpl_valid_bytes > 0 && !s.tmpl_valid) ||
            (reinterpret_cast<uintptr_t>(s.tmpl_valid) & 3))
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_init_batch: sequence %d: tmpl_valid must be 4-byte aligned and "
                                 "tmpl_valid_bytes a multiple of 4", b);
        int32_t n = 0, old_count = 0;
        if (const int rc = read_i32(s.kps.n, 1, &n)) return rc;
        if (const int rc = read_i32(s.old_count, 1, &old_count)) return rc;
        if (n < 0 || n > cap || old_count < 0 || old_count > n)
            return svo_set_error(SVO_ERR_INVALID, "svo_keyframe_init_batch: sequence %d: need 0 <= old_count = %d <= n = %d <= "
                                 "cap = %d", b, old_count, n, cap);
        KfInitArgs& ia = blocks[(size_t)b];
        memset(&ia, 0, sizeof(ia));
        ia.cam = s.cam; ia.kps = kps_dev(s.kps); ia.old_count = s.old_count;
        ia.disparity = s.disparity; ia.frame_pose = s.frame_pose;
        ia.first_frame = s.first_frame; ia.new_kf_id = s.new_kf_id; ia.kfs = static_cast<KfDev*>(s.kfs); ia.kf_mask = s.kf_mask;
        ia.color_lcg = s.color_lcg; ia.n_out = s.n_out;
        ia.enable = s.enable;
        KfDev& r = ia.record;          // (as fill_kf_record makes it, without images: no kernel of this entry reads them)
        r.kps2d = s.record.kps2d; r.kps3d = s.record.kps3d; r.flags = s.record.flags;
        r.outlier_count = s.record.outlier_count; r.inlier_count = s.record.inlier_count;
        r.kf_id = s.record.kf_id; r.kp_index = s.record.kp_index; r.score = s.record.score;
        r.level_type = s.record.level_type; r.color = s.record.color; r.kfx = s.record.kf_inv_depth; r.kfP = s.record.kf_variance;
        r.tmpl = s.tmpl; r.tmpl_valid = s.tmpl_valid; r.tmpl_cap = s.tmpl_cap; r.tmpl_win = s.tmpl_win;
        ia.tmpl_valid_bytes = s.tmpl_valid_bytes;
        ia.evict_id = s.evict_id;
    }
    KfInitArgs* d;
    const int rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    launch_kf_init(d, batch, h->stream);
    return finish_launch(h);
}

extern "C" int svo_ssd_disparity_batch(svo_handle* h, int batch, const svo_ssd_sequence* seqs, int n_bound, int win,
                                       int search_y, int* max_win) {
    CHECK_H(h);
    constexpr int kMaxIndex = 1 << 29;             // first, *first_ptr and n_bound: their sum stays an int
    if (batch < 1 || batch > 4096 || !seqs || n_bound < 0 || n_bound > kMaxIndex)
        return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_batch: need 1 <= batch <= 4096, seqs and 0 <= n_bound <= 2^29");
    if (win < 1 || win > 35 || search_y < 0 || search_y > 8)
        return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_batch: win<=35, search_y<=8 supported");
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<SsdArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_ssd_sequence& s = seqs[b];
        if (klt_bad_view(s.left) || klt_bad_view(s.right) || !s.n || s.cap < 0 || (s.cap > 0 && (!s.kps2d || !s.disparity)) ||
            s.first < 0 || s.first > kMaxIndex)
            return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_batch: sequence %d: bad arguments", b);
        if (s.win < 1 || s.win > win || s.search_x < 0 || s.search_x > 64 || s.search_y < 0 || s.search_y > search_y)
            return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_batch: sequence %d: win %d, search_x %d, search_y %d exceed "
                                 "the launch's %d, 64, %d", b, s.win, s.search_x, s.search_y, win, search_y);
        int32_t n = 0, first = 0;
        if (const int rc = read_i32(s.n, 1, &n)) return rc;
        if (s.first_ptr)
            if (const int rc = read_i32(s.first_ptr, 1, &first)) return rc;
        if (n < 0 || n > s.cap || first < 0 || first > kMaxIndex)
            return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_batch: sequence %d: n = %d is outside 0..cap = %d, or "
                                 "*first_ptr = %d is outside 0..2^29", b, n, s.cap, first);
        SsdArgs& sa = blocks[(size_t)b];
        memset(&sa, 0, sizeof(sa));
        sa.left = make_view(s.left); sa.right = make_view(s.right);
        sa.n_ptr = s.n; sa.kps2d = s.kps2d; sa.disparity = s.disparity;
        sa.win = s.win; sa.search_x = s.search_x; sa.search_y = s.search_y; sa.clamp_half = s.clamp_half;
        sa.first = s.first; sa.first_ptr = s.first_ptr;
        sa.enable = s.enable;
    }
    SsdArgs* d;
    const int rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    if (max_win) *max_win = ssd_pick_max_win(win, search_y);
    launch_ssd(d, batch, n_bound, win, search_y, h->stream);
    return finish_launch(h);
}

// svo_filter_update_table_batch: launch_filter in the form the tracker makes it (FilterArgs::kfs set: references
// gathered from the keyframe table, results written back into the keyframes), the argument blocks filled by the
// filling of pack_tracking_args itself (fill_filter_table_args). The entry makes the table's records from the
// caller's per-keyframe arrays and puts them into the caller's device memory; everything a lane would index with is
// read back and checked first (a diagnostic may wait).
static_assert(sizeof(svo_filter_keyframe) == 72 && sizeof(svo_filter_table_sequence) == 248, "the layouts the Python binding restates");

extern "C" int svo_filter_update_table_batch(svo_handle* h, int batch, const svo_filter_table_sequence* seqs, int n_bound,
                                             int do_outlier_check, int do_update, int do_flags, int do_reproject) {
    CHECK_H(h);
    if (batch < 1 || batch > 4096 || !seqs || n_bound < 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_table_batch: need 1 <= batch <= 4096, seqs and n_bound >= 0");
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the caller's counts and indices are read back below)
    std::vector<std::vector<KfDev>> tables((size_t)batch);
    std::vector<int32_t> ids, idx;
    for (int b = 0; b < batch; b++) {
        const svo_filter_table_sequence& s = seqs[b];
        const svo_kps_planes& p = s.kps;
        if (!s.kfs || !s.records || !s.frame_pose || !p.n || !p.kps2d || !p.kps3d || !p.flags || !p.kf_id || !p.kp_index ||
            !p.outlier_count || !p.inlier_count || !p.kf_inv_depth || !p.kf_variance || (do_outlier_check && !s.disparity))
            return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_table_batch: sequence %d: bad arguments", b);
        const bool ring = s.kf_mask != -1;
        if (s.table < 1 || s.table > 4096 || (ring && ((s.table & (s.table - 1)) != 0 || s.kf_mask != s.table - 1)) ||
            (int64_t)s.table * (int64_t)sizeof(KfDev) > s.records_bytes || (reinterpret_cast<uintptr_t>(s.records) & 7))
            return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_table_batch: sequence %d: the table needs 1..4096 records "
                                 "of %zu bytes, 8-byte aligned; a ring (kf_mask != -1) a power of two of them and kf_mask = "
                                 "table - 1", b, sizeof(KfDev));
        std::vector<KfDev>& rec = tables[(size_t)b];
        rec.resize((size_t)s.table);
        for (int k = 0; k < s.table; k++) {
            const svo_filter_keyframe& f = s.kfs[k];
            if (f.n < 0 || (f.n > 0 && (!f.kps2d || !f.kps3d || !f.flags || !f.outlier_count || !f.inlier_count)))
                return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_table_batch: sequence %d keyframe %d: bad arguments", b, k);
            KfDev& d = rec[(size_t)k];          // (as fill_kf_record makes it, without images and cache: this kernel reads neither)
            memset(&d, 0, sizeof(d));
            memcpy(d.pose, f.pose, sizeof(d.pose));
            d.kps2d = f.kps2d; d.kps3d = f.kps3d; d.flags = f.flags;
            d.outlier_count = f.outlier_count; d.inlier_count = f.inlier_count;
            d.n = f.n;
        }
        int32_t n = 0;
        if (const int rc = read_i32(p.n, 1, &n)) return rc;
        if (n < 0 || n > n_bound)
            return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_table_batch: sequence %d: n = %d is outside 0..n_bound = %d",
                                 b, n, n_bound);
        ids.resize((size_t)n); idx.resize((size_t)n);
        if (n > 0) {
            if (const int rc = read_i32(p.kf_id, n, ids.data())) return rc;
            if (const int rc = read_i32(p.kp_index, n, idx.data())) return rc;
        }
        for (int i = 0; i < n; i++) {
            const int slot = ids[(size_t)i] & s.kf_mask;
            if (ids[(size_t)i] < 0 || slot >= s.table || idx[(size_t)i] < 0 || idx[(size_t)i] >= s.kfs[slot].n)
                return svo_set_error(SVO_ERR_INVALID, "svo_filter_update_table_batch: sequence %d point %d: keyframe %d, index %d",
                                     b, i, ids[(size_t)i], idx[(size_t)i]);
        }
    }
    std::vector<FilterArgs> blocks((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_filter_table_sequence& s = seqs[b];
        HIP_TRY(hipMemcpy(s.records, tables[(size_t)b].data(), sizeof(KfDev) * (size_t)s.table, hipMemcpyHostToDevice));
        FilterArgs& fa = blocks[(size_t)b];
        memset(&fa, 0, sizeof(fa));
        fill_filter_table_args(fa, s.cam, kps_dev(s.kps), s.frame_pose, s.disparity, static_cast<KfDev*>(s.records), s.kf_mask,
                               s.width, s.height, s.inside_count);
        fa.do_outlier_check = do_outlier_check; fa.do_update = do_update; fa.do_flags = do_flags; fa.do_reproject = do_reproject;
    }
    FilterArgs* d;
    const int rc = stage_blocks(h, blocks, &d);
    if (rc) return rc;
    launch_filter(d, batch, n_bound, h->stream);
    return finish_launch(h);
}
