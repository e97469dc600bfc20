// scene.hip — the viewer's 3-D scene as RGB8 / RGBA8 images, many images in one launch. The reference's second
// window (src/qt-viewer/PointCloudViewer.qml) draws every keyframe's points as depth-tested squares on white, the
// trajectory as a line strip and a wire frustum per keyframe and at the current pose. The picture is stated exactly
// in include/svo_hip.h ("scene"): points and one-pixel lines, a 64-bit key per covering element, the smallest key
// wins. This file is that statement as a kernel.
//
// The host cuts every output image into tiles of SCENE_TILE_W x SCENE_TILE_H pixels (SceneTile) and describes
// every image once (SceneImage: camera, destination, a table of keyframe sets, an array of line records). A
// workgroup of 256 lanes takes one tile:
//
//  1. a plane of 64-bit keys in LDS (64 x 16 x 8 B = 8 KB) is cleared to all ones;
//  2. the image's points are walked set by set, 256 keypoints at a time: a lane filters its keypoint as the map
//     export does, transforms and projects it, rejects it against the tile by its square's bounding box and offers
//     its key with an LDS 64-bit atomic min along the square's pixels, clipped to the tile;
//  3. then the image's lines, 256 at a time: a lane transforms both ends, clips against `near`, projects, rejects by
//     bounding box and walks the sub-range of i whose major coordinate lies inside the tile. The major axis moves
//     by exactly +-1 per i (rdiv(i d, |d|) = +-i), so that sub-range follows in closed form and has at most 64
//     entries; the minor coordinate rdiv(i dm, n) is divided out once in int64 at the first i and then carried
//     with its remainder (|dm| <= n: it moves by at most 1 per i);
//  4. after the barrier lane i decodes the 4 pixels (4 (i % 16) .. + 3, i / 16) of the tile and stores them: RGBA
//     as one 16-byte store, RGB as three dwords where the address allows, else pixel by pixel / byte by byte.
//
// The min makes the bytes independent of the order the lanes arrive in: two runs give the same image. Every tile
// re-projects every element of its image, which is most of the kernel's time (DESIGN 4.12 has the figures). That is
// fine for the few thousand keypoints of a map and not for a dense cloud of 10^5 records per image.
//
// Cloud points (include/svo_hip.h, "scene clouds") therefore take a projection pass of their own, scene_splat_kernel:
// the host cuts every span of svo_map_point records into pieces of SCENE_SPLAT_PIECE records (SceneSpan), one
// workgroup each. A lane loads its 16-byte record in one load, tests the flags, transforms and projects it with the
// device functions of step 2 (the arithmetic is the same by construction), clips its square to the image and offers
// its key with a 64-bit global atomic min, result unused, to the image's key plane uint64[h][w], which the host
// clears to all ones on the same stream beforehand. scene_render_kernel<true> then seeds its LDS plane in step 1
// from that plane (all ones for the tile's pixels outside the image and for an image without a plane) and goes on
// unchanged; scene_render_kernel<false> is the kernel as it was and runs whenever no image of a launch has a plane.
// Every record is visited once per image, not once per tile.
//
// Bounds of the splat pass: a plane address is y * w + x with x, y already clipped to [0, w) x [0, h); of a piece
// exactly records [0, n) are read; no float becomes an integer before scene_project's 2^15 rule has passed.
//
// Bounds: every LDS index and every global address follows from integers already clipped to the tile, which the
// host clamps to the image. A projected coordinate only becomes an integer after |u|, |v| < 2^15 is known, so
// pixel differences stay below 2^17 and i * d below 2^33 (int64). Of an image exactly the bytes
// [dst + y * w * bpp, + w * bpp) of rows 0 .. h-1 are written. Of a set keypoints [0, n) of its five planes are
// read, of the lines records [0, n_lines).
#include <cmath>

#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

constexpr int SCENE_THREADS = 256;
static_assert(SCENE_TILE_W == 64 && SCENE_TILE_H * 16 == SCENE_THREADS, "4 pixels of a 64-pixel row per lane");
static_assert(sizeof(svo_map_point) == 16 && sizeof(SceneSpan) == 16 && SCENE_SPLAT_PIECE % SCENE_THREADS == 0, "a record is one 16-byte load");
static_assert(sizeof(svo_scene_line) == 32 && sizeof(svo_scene_camera) == 64 && sizeof(svo_scene_segment) == 64, "record sizes of the C ABI");
constexpr uint32_t SCENE_FLAG_BITS = SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY;
constexpr int SCENE_MAX_SIDE = 4096;

int scene_check_style(const svo_scene_style* s, const char* who) {
    if (!s) return svo_set_error(SVO_ERR_INVALID, "%s: no style", who);
    if (s->cols < 1 || s->cols > SCENE_MAX_SIDE || s->rows < 1 || s->rows > SCENE_MAX_SIDE)
        return svo_set_error(SVO_ERR_INVALID, "%s: %d x %d is not within 1 .. %d a side", who, s->cols, s->rows, SCENE_MAX_SIDE);
    if (s->pixel != SVO_PIXEL_RGB8 && s->pixel != SVO_PIXEL_RGBA8) return svo_set_error(SVO_ERR_INVALID, "%s: pixel format %d", who, s->pixel);
    if (s->point_size < 1 || s->point_size > 16) return svo_set_error(SVO_ERR_INVALID, "%s: point_size %d is not within 1 .. 16", who, s->point_size);
    if ((s->background | s->trajectory_rgb | s->keyframe_rgb | s->pose_rgb) >> 24)
        return svo_set_error(SVO_ERR_INVALID, "%s: a colour is r << 16 | g << 8 | b", who);
    if (!std::isfinite(s->frustum_w) || !std::isfinite(s->frustum_h) || !std::isfinite(s->frustum_d))
        return svo_set_error(SVO_ERR_INVALID, "%s: the frustum's dimensions are not finite", who);
    if (s->show & ~(uint32_t)(SVO_SCENE_POINTS | SVO_SCENE_TRAJECTORY | SVO_SCENE_KEYFRAMES | SVO_SCENE_POSE))
        return svo_set_error(SVO_ERR_INVALID, "%s: show 0x%x has unknown bits", who, s->show);
    if (s->from_keyframe < 0 || s->trajectory_tail < 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: from_keyframe %d, trajectory_tail %d", who, s->from_keyframe, s->trajectory_tail);
    if ((s->filter.drop_flags & ~SCENE_FLAG_BITS) || s->filter._reserved != 0 || s->_reserved != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: filter.drop_flags 0x%x has unknown bits, or a _reserved is not 0", who, s->filter.drop_flags);
    return SVO_OK;
}

int scene_check_camera(const svo_scene_camera* c, const char* who, int i) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "%s: no cameras", who);
    bool finite = std::isfinite(c->f) && std::isfinite(c->cx) && std::isfinite(c->cy) && std::isfinite(c->near);
    for (float v : c->view) finite = finite && std::isfinite(v);
    if (!finite || !(c->f > 0) || !(c->near > 0))
        return svo_set_error(SVO_ERR_INVALID, "%s: camera %d: an entry is not finite, or f or near is not > 0", who, i);
    return SVO_OK;
}

// r << 16 | g << 8 | b as the bytes r, g, b, 255 of a little-endian dword
__host__ __device__ inline uint32_t scene_rgba(uint32_t rgb) {
    return ((rgb >> 16) & 0xffu) | (rgb & 0xff00u) | ((rgb & 0xffu) << 16) | 0xff000000u;
}

SceneParams scene_params(const svo_scene_style& s) {
    SceneParams p;
    p.bpp = s.pixel == SVO_PIXEL_RGB8 ? 3 : 4;
    p.point_size = s.point_size;
    p.background = scene_rgba(s.background);
    p.filter = s.filter;
    return p;
}

void scene_shape(const svo_scene_style& s, int cols, int rows, int64_t* pitch, int64_t* image_bytes) {
    const int64_t p = (int64_t)cols * (s.pixel == SVO_PIXEL_RGB8 ? 3 : 4);
    if (pitch) *pitch = p;
    if (image_bytes) *image_bytes = (p * rows + 255) / 256 * 256;
}

SceneSet scene_set(const KpsDev& k, int n, int own_id) {
    return SceneSet{reinterpret_cast<const uint32_t*>(k.kps3d), k.flags, k.kf_id, k.inl, k.color, n, own_id};
}

void scene_tiles(int image, int w, int h, std::vector<SceneTile>& out) {
    SceneTile t{image, 0, 0, 0};
    for (t.y0 = 0; t.y0 < h; t.y0 += SCENE_TILE_H)
        for (t.x0 = 0; t.x0 < w; t.x0 += SCENE_TILE_W) out.push_back(t);
}

__device__ __forceinline__ bool scene_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // (false for a NaN)

// c = T(x, y, z); false unless every c_k is finite
__device__ __forceinline__ bool scene_transform(const svo_scene_camera& cam, float x, float y, float z, float c[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = ((cam.view[4 * k] * x + cam.view[4 * k + 1] * y) + cam.view[4 * k + 2] * z) + cam.view[4 * k + 3];
    return scene_finite(c[0]) && scene_finite(c[1]) && scene_finite(c[2]);
}

// (X, Y) = (floor(u), floor(v)) of a camera-frame point with c_2 >= near; false unless |u|, |v| < 2^15 (a NaN fails;
// no float -> int conversion of such a value)
__device__ __forceinline__ bool scene_project(const svo_scene_camera& cam, const float c[3], int& X, int& Y) {
    const float u = (cam.f * c[0]) / c[2] + cam.cx, v = (cam.f * c[1]) / c[2] + cam.cy;
    if (!(fabsf(u) < 32768.f) || !(fabsf(v) < 32768.f)) return false;
    X = (int)floorf(u); Y = (int)floorf(v);
    return true;
}

// the key of an element at `depth` (> 0: its bits order as the values do) into the tile's pixel (x, y), tile
// coordinates inside [0, SCENE_TILE_W) x [0, SCENE_TILE_H)
__device__ __forceinline__ void scene_offer(unsigned long long* keys, int x, int y, float depth, uint32_t low) {
    atomicMin(&keys[y * SCENE_TILE_W + x], (unsigned long long)__float_as_uint(depth) << 32 | low);
}

// One lane per record of a piece; SCENE_SPLAT_PIECE / SCENE_THREADS records per lane, a wave's 64 records adjacent.
__global__ __launch_bounds__(SCENE_THREADS) void scene_splat_kernel(const SceneSpan* __restrict__ spans,
                                                                    const SceneImage* __restrict__ images,
                                                                    unsigned long long* const* __restrict__ planes, const SceneParams p) {
    const SceneSpan sp = G(spans)[blockIdx.x];
    const SceneImage im = G(images)[sp.image];
    SVO_GP(unsigned long long) plane = G(G(planes)[sp.image]);
    SVO_GP(const uint4) rec = (SVO_GP(const uint4))G(sp.points);
    const int s = p.point_size, w = im.w, h = im.h;
    for (int k = threadIdx.x; k < sp.n; k += SCENE_THREADS) {
        const uint4 q = rec[k];                            // x, y, z, r | g << 8 | b << 16 | flags << 24
        const uint32_t flags = q.w >> 24;
        // (the transform comes before the flags test so that all four words are needed at once: one 16-byte load,
        // not a dword for the flags and three more behind the branch)
        float c[3];
        const bool finite = scene_transform(im.cam, __uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), c);
        if ((flags & (SVO_CLOUD_DROPPED | p.filter.drop_flags)) || !finite) continue;
        if (!(c[2] >= im.cam.near)) continue;
        int X, Y;
        if (!scene_project(im.cam, c, X, Y)) continue;
        // the square, clipped to the image
        int xa = X - (s - 1) / 2, ya = Y - (s - 1) / 2;
        int xb = xa + s - 1, yb = ya + s - 1;
        xa = max(xa, 0); xb = min(xb, w - 1);
        ya = max(ya, 0); yb = min(yb, h - 1);
        if (xa > xb || ya > yb) continue;
        const uint32_t low = (uint32_t)SVO_SCENE_CLASS_CLOUD << 24 | (q.w & 0xffu) << 16 | (q.w & 0xff00u) | ((q.w >> 16) & 0xffu);
        const unsigned long long key = (unsigned long long)__float_as_uint(c[2]) << 32 | low;
        for (int y = ya; y <= yb; y++)
            for (int x = xa; x <= xb; x++) atomicMin((unsigned long long*)(plane + ((size_t)y * w + x)), key);
    }
}

template <bool CLOUDS>
__global__ __launch_bounds__(SCENE_THREADS) void scene_render_kernel(const SceneTile* __restrict__ tiles,
                                                                     const SceneImage* __restrict__ images,
                                                                     const unsigned long long* const* __restrict__ planes,
                                                                     const SceneParams p) {
    __shared__ unsigned long long keys[SCENE_TILE_W * SCENE_TILE_H];
    const SceneTile t = G(tiles)[blockIdx.x];
    const SceneImage im = G(images)[t.image];
    const int tid = threadIdx.x;
    const int tw = min(SCENE_TILE_W, im.w - t.x0), th = min(SCENE_TILE_H, im.h - t.y0);   // the tile's pixels inside the image

    // 1. the key plane
    if (CLOUDS) {
        SVO_GP(const unsigned long long) plane = G(G(planes)[t.image]);   // (null: an image without cloud points)
        for (int i = tid; i < SCENE_TILE_W * SCENE_TILE_H; i += SCENE_THREADS) {
            const int x = i % SCENE_TILE_W, y = i / SCENE_TILE_W;
            keys[i] = plane && x < tw && y < th ? plane[(size_t)(t.y0 + y) * im.w + (t.x0 + x)] : ~0ull;
        }
    } else {
        for (int i = tid; i < SCENE_TILE_W * SCENE_TILE_H; i += SCENE_THREADS) keys[i] = ~0ull;
    }
    __syncthreads();

    // 2. the points
    const int s = p.point_size;
    for (int set_i = 0; set_i < im.n_sets; set_i++) {
        const SceneSet set = G(im.sets)[set_i];
        for (int base = 0; base < set.n; base += SCENE_THREADS) {
            const int k = base + tid;
            if (k >= set.n) continue;
            const uint32_t flags = G(set.flags)[k];
            if (flags & p.filter.drop_flags) continue;
            if (p.filter.own_only && G(set.kf_id)[k] != set.own_id) continue;
            if (G(set.inl)[k] < p.filter.min_inliers) continue;
            SVO_GP(const uint32_t) w3 = G(set.kps3d) + (size_t)k * 3;
            float c[3];
            if (!scene_transform(im.cam, __uint_as_float(w3[0]), __uint_as_float(w3[1]), __uint_as_float(w3[2]), c)) continue;
            if (!(c[2] >= im.cam.near)) continue;
            int X, Y;
            if (!scene_project(im.cam, c, X, Y)) continue;
            // the square in tile coordinates, clipped to the tile
            int xa = X - (s - 1) / 2 - t.x0, ya = Y - (s - 1) / 2 - t.y0;
            int xb = xa + s - 1, yb = ya + s - 1;
            xa = max(xa, 0); xb = min(xb, tw - 1);
            ya = max(ya, 0); yb = min(yb, th - 1);
            if (xa > xb || ya > yb) continue;
            const uint32_t col = G(set.color)[k];
            const uint32_t low = (uint32_t)SVO_SCENE_CLASS_POINT << 24 | (col & 0xffu) << 16 | (col & 0xff00u) | ((col >> 16) & 0xffu);
            for (int y = ya; y <= yb; y++)
                for (int x = xa; x <= xb; x++) scene_offer(keys, x, y, c[2], low);
        }
    }

    // 3. the lines
    const int bx0 = t.x0, bx1 = t.x0 + tw - 1, by0 = t.y0, by1 = t.y0 + th - 1;   // the tile, image coordinates
    for (int base = 0; base < im.n_lines; base += SCENE_THREADS) {
        const int k = base + tid;
        if (k >= im.n_lines) continue;
        SVO_GP(const uint4) rec = (SVO_GP(const uint4))G(im.lines) + (size_t)k * 2;
        const uint4 q0 = rec[0], q1 = rec[1];
        float a[3], b[3];
        if (!scene_transform(im.cam, __uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z), a)) continue;
        if (!scene_transform(im.cam, __uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y), b)) continue;
        const float near = im.cam.near;
        const bool a_near = a[2] < near, b_near = b[2] < near;
        if (a_near && b_near) continue;
        if (a_near) {
            const float f = (near - a[2]) / (b[2] - a[2]);
            a[0] = a[0] + f * (b[0] - a[0]);
            a[1] = a[1] + f * (b[1] - a[1]);
            a[2] = near;
            if (!scene_finite(a[0]) || !scene_finite(a[1])) continue;
        } else if (b_near) {
            const float f = (near - b[2]) / (a[2] - b[2]);
            b[0] = b[0] + f * (a[0] - b[0]);
            b[1] = b[1] + f * (a[1] - b[1]);
            b[2] = near;
            if (!scene_finite(b[0]) || !scene_finite(b[1])) continue;
        }
        int X0, Y0, X1, Y1;
        if (!scene_project(im.cam, a, X0, Y0) || !scene_project(im.cam, b, X1, Y1)) continue;
        if (min(X0, X1) > bx1 || max(X0, X1) < bx0 || min(Y0, Y1) > by1 || max(Y0, Y1) < by0) continue;   // the bounding box misses the tile
        const uint32_t low = q1.z;
        const float z0 = a[2], z1 = b[2];
        const int dx = X1 - X0, dy = Y1 - Y0;
        const int n = max(abs(dx), abs(dy));
        if (n == 0) {                                      // (inside the tile: its bounding box is the pixel)
            scene_offer(keys, X0 - t.x0, Y0 - t.y0, z0, low);
            continue;
        }
        // M: the major axis (n = |dM|, it moves by sM per i), m: the minor one
        const bool xmajor = abs(dx) >= abs(dy);
        const int M0 = xmajor ? X0 : Y0, dM = xmajor ? dx : dy, m0 = xmajor ? Y0 : X0, dm = xmajor ? dy : dx;
        const int Mlo = xmajor ? bx0 : by0, Mhi = xmajor ? bx1 : by1, mlo = xmajor ? by0 : bx0, mhi = xmajor ? by1 : bx1;
        const int sM = dM > 0 ? 1 : -1;
        const int ilo = max(0, sM > 0 ? Mlo - M0 : M0 - Mhi), ihi = min(n, sM > 0 ? Mhi - M0 : M0 - Mlo);
        if (ilo > ihi) continue;
        // rdiv(ilo * dm, n) = q, with the remainder rem in [0, 2 n)
        const long long den = 2ll * n, num = 2ll * ilo * dm + n;
        long long q64 = num / den;
        if (num - q64 * den < 0) q64--;
        int q = (int)q64, rem = (int)(num - q64 * den);
        const float zd = z1 - z0, fn = (float)n;
        for (int i = ilo; i <= ihi; i++) {
            const int M = M0 + sM * i, m = m0 + q;
            if (m >= mlo && m <= mhi) {
                const float z = z0 + zd * ((float)i / fn);
                scene_offer(keys, (xmajor ? M : m) - t.x0, (xmajor ? m : M) - t.y0, z, low);
            }
            rem += 2 * dm;                                 // |2 dm| <= 2 n: one step at most
            if (rem >= (int)den) { rem -= (int)den; q++; }
            else if (rem < 0) { rem += (int)den; q--; }
        }
    }
    __syncthreads();

    // 4. decode and store
    const int lx = (tid & 15) * 4, ly = tid >> 4;
    const int px = ly < th ? max(0, min(4, tw - lx)) : 0;                            // pixels of this lane: 0 .. 4
    if (px == 0) return;
    uint32_t rgb[4];                                                                 // r | g << 8 | b << 16 | 255 << 24
    for (int i = 0; i < 4; i++) {
        const unsigned long long key = keys[ly * SCENE_TILE_W + lx + i];
        rgb[i] = key == ~0ull ? p.background : scene_rgba((uint32_t)key);
    }
    const int x = t.x0 + lx, y = t.y0 + ly;
    SVO_GP(uint8_t) d = G(im.dst) + ((int64_t)y * im.w + x) * p.bpp;
    if (p.bpp == 4) {
        if (px == 4 && ((uintptr_t)d & 15) == 0) {
            *(SVO_GP(uint4))d = make_uint4(rgb[0], rgb[1], rgb[2], rgb[3]);
        } else {
            for (int i = 0; i < px; i++) ((SVO_GP(uint32_t))d)[i] = rgb[i];          // (an RGBA image is 4-byte aligned)
        }
    } else {
        if (px == 4 && ((uintptr_t)d & 3) == 0) {
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
    }
}

void launch_scene(const SceneTile* d_tiles, int n_tiles, const SceneImage* d_images, const SceneParams& p, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(scene_render_kernel<false>, dim3(n_tiles), dim3(SCENE_THREADS), 0, stream, d_tiles, d_images, nullptr, p);
}

void launch_scene_clouds(const SceneTile* d_tiles, int n_tiles, const SceneImage* d_images, unsigned long long* const* d_planes,
                         const SceneParams& p, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(scene_render_kernel<true>, dim3(n_tiles), dim3(SCENE_THREADS), 0, stream, d_tiles, d_images, d_planes, p);
}

void launch_scene_splat(const SceneSpan* d_spans, int n_spans, const SceneImage* d_images, unsigned long long* const* d_planes,
                        const SceneParams& p, int point_size, hipStream_t stream) {
    if (n_spans <= 0) return;
    SceneParams q = p;
    q.point_size = point_size;
    hipLaunchKernelGGL(scene_splat_kernel, dim3(n_spans), dim3(SCENE_THREADS), 0, stream, d_spans, d_images, d_planes, q);
}

}  // namespace svo
