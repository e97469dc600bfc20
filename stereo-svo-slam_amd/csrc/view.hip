// view.hip — gray image planes as GRAY8 / RGB8 / RGBA8 images with one marker per keypoint, many images in one
// launch. The reference shows its state as images: draw_frame (src/app/main.cpp:40-118) converts
// frame.stereo_image.left[0] with GRAY2RGB and calls cv::drawMarker(img, p, color, type, size) at thickness 1 per
// keypoint (MARKER_CROSS for a FAST corner, MARKER_SQUARE otherwise). Both marker types are axis-aligned runs, so
// the picture is stated exactly here (include/svo_hip.h, "views"); putText and the x2 resize are not restated.
//
// The host cuts every output image into tiles of VIEW_TILE_W x VIEW_TILE_H pixels (ViewTile); a workgroup of 256
// lanes takes one tile, lane i the 4 pixels (4 (i % 16) .. + 3, i / 16) of it:
//
//  1. the lane's 4 gray bytes: one dword load where the address is 4-byte aligned and the 4 pixels lie inside the
//     row, bytes otherwise (any base, any stride: a borrowed frame, a pyramid level of odd width);
//  2. with markers: a per-pixel owner plane of the tile in LDS (64 x 16 dwords = 4 KB) is cleared, then the set's
//     keypoints are walked 256 at a time: a lane whose marker's bounding box meets the tile writes index + 1 into
//     the owner plane along the marker's <= 4 runs, clipped to the tile, with an LDS atomic max. The reference
//     draws in ascending index and a later marker overwrites: a pixel shows the highest index that covers it, and
//     the max does not depend on the order the lanes arrive in;
//  3. after the barrier a lane composes its 4 pixels, (g, g, g) or the colour of keypoint owner - 1, and stores
//     them: RGBA as one 16-byte store, RGB as three dwords, gray as one dword where the address allows, else
//     pixel by pixel (RGBA) or byte by byte.
//
// A tile's rows are 64 consecutive pixels: a wave's RGBA store instruction writes 4 rows of 256 contiguous bytes,
// its gray load reads 4 rows of 64. The kernel only moves data, 1 byte in and 1 - 4 out per pixel plus 16 bytes
// per keypoint candidate and tile; its roof is HBM. LDS: 4 KB per workgroup, far from bounding the occupancy. In
// the owner plane the 32 lanes of a ds_read_b128 group read 4 consecutive dwords each from 2 rows of 64 dwords:
// every bank once per 16 lanes.
//
// Bounds: every address follows from the tile's integer pixel coordinates, which the host clamps to the image;
// a marker's position only enters an LDS index after it is clipped to the tile. Of an image exactly the bytes
// [dst + y * w * bpp, + w * bpp) of rows 0 .. h-1 are written; of its source exactly the w bytes of each row read.
#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

constexpr int VIEW_THREADS = 256;
static_assert(VIEW_TILE_W == 64 && VIEW_TILE_H * 16 == VIEW_THREADS, "4 pixels of a 64-pixel row per lane");

int view_check_style(const svo_view_style* s, int max_levels, const char* who) {
    if (!s) return svo_set_error(SVO_ERR_INVALID, "%s: no style", who);
    if (s->plane != SVO_PLANE_LEFT && s->plane != SVO_PLANE_RIGHT) return svo_set_error(SVO_ERR_INVALID, "%s: plane %d", who, s->plane);
    if (s->level < 0 || s->level >= (s->plane == SVO_PLANE_LEFT ? max_levels : 1))
        return svo_set_error(SVO_ERR_INVALID, "%s: level %d of plane %d", who, s->level, s->plane);
    if (s->pixel != SVO_PIXEL_GRAY8 && s->pixel != SVO_PIXEL_RGB8 && s->pixel != SVO_PIXEL_RGBA8)
        return svo_set_error(SVO_ERR_INVALID, "%s: pixel format %d", who, s->pixel);
    if (s->markers != 0 && s->markers != 1) return svo_set_error(SVO_ERR_INVALID, "%s: markers %d", who, s->markers);
    if (s->markers && (s->plane != SVO_PLANE_LEFT || s->pixel == SVO_PIXEL_GRAY8))
        return svo_set_error(SVO_ERR_INVALID, "%s: markers need the left plane and RGB8 or RGBA8", who);
    if ((s->drop_flags & ~(uint32_t)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY)) || s->_reserved != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: drop_flags 0x%x has unknown bits, or _reserved is not 0", who, s->drop_flags);
    if (s->size < 0 || s->size > 64 || s->size_temporary < 0 || s->size_temporary > 64)
        return svo_set_error(SVO_ERR_INVALID, "%s: marker sizes %d / %d are not within 0 .. 64", who, s->size, s->size_temporary);
    return SVO_OK;
}

ViewParams view_params(const svo_view_style& s) {
    ViewParams p;
    p.level = s.level;
    p.bpp = s.pixel == SVO_PIXEL_GRAY8 ? 1 : s.pixel == SVO_PIXEL_RGB8 ? 3 : 4;
    p.markers = s.markers;
    p.drop_flags = s.drop_flags;
    const int size[2] = {s.size, s.size_temporary};
    for (int i = 0; i < 2; i++) {
        p.half_cross[i] = size[i] / 2;
        p.half_square[i] = (int)(size[i] * 0.8) / 2;
    }
    return p;
}

void view_tiles(const ImgView& src, uint8_t* dst, const KpsDev* kps, int n, std::vector<ViewTile>& out) {
    ViewTile t;
    t.src = src.data; t.dst = dst;
    t.kps2d = kps ? kps->kps2d : nullptr; t.flags = kps ? kps->flags : nullptr;
    t.level_type = kps ? kps->level_type : nullptr; t.color = kps ? kps->color : nullptr;
    t.src_stride = src.stride; t.w = src.w; t.h = src.h;
    t.n = kps ? n : 0;
    for (t.y0 = 0; t.y0 < src.h; t.y0 += VIEW_TILE_H)
        for (t.x0 = 0; t.x0 < src.w; t.x0 += VIEW_TILE_W) out.push_back(t);
}

// index + 1 of keypoint k into the owner plane along the run x in [xa, xb], y in [ya, yb] (one of the two is a
// single value), clipped to the tile's pixels [0, tw) x [0, th) (tile coordinates)
__device__ __forceinline__ void mark_run(uint32_t* owner, int xa, int xb, int ya, int yb, int tw, int th, uint32_t v) {
    xa = max(xa, 0); xb = min(xb, tw - 1);
    ya = max(ya, 0); yb = min(yb, th - 1);
    for (int y = ya; y <= yb; y++)
        for (int x = xa; x <= xb; x++) atomicMax(&owner[y * VIEW_TILE_W + x], v);
}

__global__ __launch_bounds__(VIEW_THREADS) void view_render_kernel(const ViewTile* __restrict__ tiles, const ViewParams p) {
    __shared__ uint4 owner4[VIEW_TILE_W * VIEW_TILE_H / 4];
    uint32_t* owner = reinterpret_cast<uint32_t*>(owner4);
    const ViewTile t = G(tiles)[blockIdx.x];
    const int tid = threadIdx.x;
    const int lx = (tid & 15) * 4, ly = tid >> 4;
    const int x = t.x0 + lx, y = t.y0 + ly;
    const int tw = min(VIEW_TILE_W, t.w - t.x0), th = min(VIEW_TILE_H, t.h - t.y0);   // the tile's pixels inside the image
    const bool row = ly < th;
    const int px = row ? max(0, min(4, tw - lx)) : 0;                                // pixels of this lane: 0 .. 4

    // 1. the gray bytes
    uint32_t gray = 0;
    if (px > 0) {
        SVO_GP(const uint8_t) s = G(t.src) + (int64_t)y * t.src_stride + x;
        if (px == 4 && ((uintptr_t)s & 3) == 0) {
            gray = *(SVO_GP(const uint32_t))s;
        } else {
            for (int i = 0; i < px; i++) gray |= (uint32_t)s[i] << (8 * i);
        }
    }

    // 2. the owner plane
    uint4 own = make_uint4(0, 0, 0, 0);
    if (p.markers) {
        owner4[tid] = own;
        __syncthreads();
        const float scale = __uint_as_float((uint32_t)(127 - p.level) << 23);        // 2^-level, exact
        for (int base = 0; base < t.n; base += VIEW_THREADS) {
            const int k = base + tid;
            if (k >= t.n) continue;
            const uint32_t flags = G(t.flags)[k];
            if (flags & p.drop_flags) continue;
            const svo_kp2d c = G(t.kps2d)[k];
            const float fx = c.x * scale, fy = c.y * scale;
            // not finite, or beyond any image: no marker (and no float -> int conversion of such a value)
            if (!(fabsf(fx) < 32768.f) || !(fabsf(fy) < 32768.f)) continue;
            const int cx = (int)fx - t.x0, cy = (int)fy - t.y0;                      // truncated toward zero; tile coordinates
            const int tmp = (flags & SVO_IGNORE_TEMPORARY) ? 1 : 0;
            const bool cross = ((G(t.level_type)[k] >> 8) & 0xff) == SVO_KP_FAST;
            const int h = cross ? p.half_cross[tmp] : p.half_square[tmp];
            if (cx + h < 0 || cx - h >= tw || cy + h < 0 || cy - h >= th) continue;  // the bounding box misses the tile
            const uint32_t v = (uint32_t)k + 1u;
            if (cross) {
                mark_run(owner, cx - h, cx + h, cy, cy, tw, th, v);
                mark_run(owner, cx, cx, cy - h, cy + h, tw, th, v);
            } else {
                mark_run(owner, cx - h, cx + h, cy - h, cy - h, tw, th, v);
                mark_run(owner, cx - h, cx + h, cy + h, cy + h, tw, th, v);
                mark_run(owner, cx - h, cx - h, cy - h, cy + h, tw, th, v);
                mark_run(owner, cx + h, cx + h, cy - h, cy + h, tw, th, v);
            }
        }
        __syncthreads();
        own = owner4[tid];
    }
    if (px == 0) return;

    // 3. compose and store
    const uint32_t o[4] = {own.x, own.y, own.z, own.w};
    uint32_t rgb[4];                                                                 // r | g << 8 | b << 16 | 255 << 24
    for (int i = 0; i < 4; i++) {
        const uint32_t g = (gray >> (8 * i)) & 0xffu;
        rgb[i] = (o[i] ? (G(t.color)[o[i] - 1] & 0xffffffu) : g * 0x010101u) | 0xff000000u;
    }
    const int64_t at = ((int64_t)y * t.w + x) * p.bpp;
    SVO_GP(uint8_t) d = G(t.dst) + at;
    const bool wide = px == 4 && ((uintptr_t)d & 3) == 0;
    if (p.bpp == 4) {
        if (px == 4 && ((uintptr_t)d & 15) == 0) {
            *(SVO_GP(uint4))d = make_uint4(rgb[0], rgb[1], rgb[2], rgb[3]);
        } else {
            for (int i = 0; i < px; i++) ((SVO_GP(uint32_t))d)[i] = rgb[i];          // (an RGBA image is 4-byte aligned)
        }
    } else if (p.bpp == 3) {
        if (wide) {
            const uint32_t a = rgb[0] & 0xffffffu, b = rgb[1] & 0xffffffu, c = rgb[2] & 0xffffffu, e = rgb[3] & 0xffffffu;
            SVO_GP(uint32_t) d4 = (SVO_GP(uint32_t))d;
            d4[0] = a | b << 24;
            d4[1] = b >> 8 | c << 16;
            d4[2] = c >> 16 | e << 8;
        } else {
            for (int i = 0; i < px; i++) {
                d[3 * i] = (uint8_t)rgb[i]; d[3 * i + 1] = (uint8_t)(rgb[i] >> 8); d[3 * i + 2] = (uint8_t)(rgb[i] >> 16);
            }
        }
    } else {
        if (wide) {
            *(SVO_GP(uint32_t))d = gray;
        } else {
            for (int i = 0; i < px; i++) d[i] = (uint8_t)(gray >> (8 * i));
        }
    }
}

void launch_view(const ViewTile* d_tiles, int n_tiles, const ViewParams& p, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(view_render_kernel, dim3(n_tiles), dim3(VIEW_THREADS), 0, stream, d_tiles, p);
}

}  // namespace svo
