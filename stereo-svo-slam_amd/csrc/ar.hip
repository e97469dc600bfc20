// ar.hip — the AR demo's picture as RGB8 / RGBA8 images, many images in two launches. The reference's AR demo
// (src/ar-app/) lays a lit mesh, fixed in the world, over the left camera image, seen from the tracked pose through
// the pinhole intrinsics. The picture is stated exactly in include/svo_hip.h ("ar"): flat-shaded triangles snapped to
// 4 sub-pixel bits, int64 edge functions at the pixel centres, a 64-bit key per covering triangle, the smallest key
// wins, the gray plane where nobody covers. This file is that statement as two kernels.
//
//  first launch (ar_setup_kernel): one lane per (image, triangle), a workgroup per ArSetup item (256 triangles of
//  one draw). The lane gathers the three vertices (indices checked against n_vertices), takes them to the world and
//  into the camera, projects and snaps them, shades the face, and writes a 64-byte ArRecord: six ints, three depths,
//  the shaded colour and the box of pixels whose centres can lie inside, clipped to the image. A dropped triangle
//  (and one with A == 0 or an empty box) gets the empty box. A triangle costs three transforms, six divisions, a
//  square root: done here once, not once per tile as scene.hip does with its points.
//
//  second launch (ar_render_kernel): a workgroup of 256 lanes per 64 x 16 tile (ArTile).
//  1. a plane of 64-bit keys in LDS (8 KB) is cleared to all ones;
//  2. the image's records are walked 256 at a time. A lane reads its record's box (16 bytes) and clips it to the
//     tile; an empty intersection costs nothing more. A box of at most AR_SMALL_PIXELS pixels is rasterised by the
//     lane itself: it walks the box, carries the three edge functions in int64 and offers the keys of the covered
//     pixels with an LDS 64-bit atomic min. A larger box is queued in LDS (a ring of 256 record indices);
//  3. if any lane queued (one barrier that votes), the whole workgroup takes the queued records one by one: every
//     lane tests its own 4 pixels (the ones it stores in 4.) and lowers their keys without atomics: between the two
//     barriers of this pass nobody else touches them;
//  4. lane i decodes the 4 pixels (4 (i % 16) .. + 3, i / 16) of the tile, takes the background byte where the key is
//     still all ones, and stores as scene.hip does: RGBA as one 16-byte store, RGB as three dwords where the address
//     allows, else pixel by pixel / byte by byte.
//
// The min makes the bytes independent of the order in which lanes arrive and of the order of the queue.
// AR_SMALL_PIXELS = 64 is the best of the eight values measured on one workload; on another it is a guess.
//
// Bounds: a projected coordinate only becomes an integer after |u|, |v| < 2^15 is known, so |X|, |Y| < 2^19, the
// differences stay below 2^20 and the edge functions below 2^41 (int64). A record's box is clipped to the image by
// the first launch and to the tile by the second (the host clamps tiles to the image), and every LDS index and
// pixel address follows from those integers. Of an image exactly the bytes [dst + y * w * bpp, + w * bpp) of rows
// 0 .. h-1 are written and the bytes [src + y * stride, + w) read; of a draw triangles [0, n_triangles), its rgb
// likewise, and vertices [0, n_vertices); of the records [0, n_records).
//
// Occlusion (include/svo_hip.h, "ar occlusion"): ar_render_kernel<true> is the same kernel with an occluder per image,
// an organized lattice of svo_map_point records. ar_render_kernel<false> is the kernel above, argument for argument.
//  - before the record walk every lane asks for the records of up to four cells of its tile, 16 bytes each (one
//    global_load_dwordx4), consecutive lanes consecutive cells of a lattice row, so that they are in flight during the
//    walk; after it the lane reduces each to one float (z, or +inf where nothing occludes) in an LDS plane of at most
//    1024 floats; one barrier;
//  - in 4. a lane looks up the cell of each of its four pixels (one division for the first, then carried), compares
//    the winner's depth with zo + margin, and drops or dims; the lanes' covered / hidden counts (0 .. 4) are summed per
//    wavefront with three ballots and popcounts each, per workgroup with one LDS atomic add per wavefront, and the
//    workgroup adds its pair to the image's two 64-bit counters with integer atomics: no order can change the sums.
// Bounds of the occluded part: with the tile [bx0, bx1] x [by0, by1] inside the image and step >= 1, the tile's cells
// are cx0 = bx0 / step .. min(bx1 / step, cols - 1) and likewise in y: ncx x ncy of them, both <= 0 made 0 (the tile
// lies beyond the lattice; no record is read). bx1 - bx0 <= 63 and by1 - by0 <= 15 give ncx <= 63 / step + 2 and
// ncy <= 15 / step + 2, and since tiles start at multiples of 64 and 16, ncx * ncy <= 1024 = AR_OCC_CELLS, reached at
// step 1 (n_cells is clipped to it all the same, and a lookup beyond n_cells occludes nothing). A record address is
// (cy0 + q) * cols + cx0 + r with q < ncy, r < ncx, so row <= rows - 1 and column <= cols - 1: inside the cols x rows
// records the host checked. A pixel x >= bx0, y >= by0 has ix = x / step - cx0 >= 0, iy >= 0, and is looked up only
// when ix < ncx and iy < ncy. The counters are words 0 and 1 of the image's ArOccluder::counts.
// LDS banks of the plane (ds_read_b32: bank = word % 32, conflicts within a 32-lane half, which holds two tile rows
// of 16 lanes): lane l of a row reads word (4 l + i) / step of its cell row. step >= 4: the four pixels of a lane share
// a cell and 16 lanes read 16 / (step / 4) consecutive or equal words: no conflict, equal addresses broadcast; the
// second row of the half reads the same words (same cell row) or words ncx further on. step 2: words 2 l + i / 2, 32
// distinct words a row: no conflict within a row, two-way against the other row when it is another cell row. step 1:
// words 4 l + i, stride 4: two-way within a row, four-way with the other row (+64 words). step 3: stride 4 / 3, at
// most two-way. These are four reads per lane per tile; they were not measured apart from the kernel's time.
#include <cmath>

#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

static_assert(AR_TILE_W == 64 && AR_TILE_H * 16 == AR_THREADS, "4 pixels of a 64-pixel row per lane");
static_assert(sizeof(ArRecord) == 64 && sizeof(svo_ar_camera) == 64 && sizeof(svo_ar_segment) == 64 && sizeof(svo_ar_instance) == 64 &&
              sizeof(svo_ar_draw) == 88 && sizeof(svo_ar_style) == 32 && sizeof(svo_ar_mesh) == 40, "record sizes of the C ABI");
static_assert(sizeof(svo_ar_visibility) == 32 && sizeof(svo_ar_occlusion) == 128 && sizeof(svo_ar_occluder) == 24 && sizeof(ArOccluder) == 32 &&
              sizeof(svo_map_point) == 16, "record sizes of ar occlusion");
#ifndef SVO_AR_SMALL_PIXELS
#define SVO_AR_SMALL_PIXELS 64                             // (-DSVO_AR_SMALL_PIXELS=n: the variants tools/ar_bench.py compared)
#endif
constexpr int AR_SMALL_PIXELS = SVO_AR_SMALL_PIXELS;

int ar_check_style(const svo_ar_style* s, const char* who) {
    if (!s) return svo_set_error(SVO_ERR_INVALID, "%s: no style", who);
    if (s->pixel != SVO_PIXEL_RGB8 && s->pixel != SVO_PIXEL_RGBA8) return svo_set_error(SVO_ERR_INVALID, "%s: pixel format %d", who, s->pixel);
    if (!std::isfinite(s->light[0]) || !std::isfinite(s->light[1]) || !std::isfinite(s->light[2]))
        return svo_set_error(SVO_ERR_INVALID, "%s: the light is not finite", who);
    if (!(s->ambient >= 0) || !(s->ambient <= 1)) return svo_set_error(SVO_ERR_INVALID, "%s: ambient is not within 0 .. 1", who);
    if (!(s->near > 0) || !std::isfinite(s->near)) return svo_set_error(SVO_ERR_INVALID, "%s: near is not > 0 and finite", who);
    if (s->_reserved[0] != 0 || s->_reserved[1] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    return SVO_OK;
}

int ar_check_occluder(const svo_ar_occluder* o, const char* who, int i) {
    if (!o) return svo_set_error(SVO_ERR_INVALID, "%s: no occluders", who);
    if (o->_reserved != 0 || (o->records && (o->step < 1 || o->step > 16 || o->cols <= 0 || o->rows <= 0 || ((uintptr_t)o->records & 15))))
        return svo_set_error(SVO_ERR_INVALID, "%s: image %d: an occluder of step 1 .. 16, cols and rows > 0, records 16-byte aligned, _reserved 0", who, i);
    return SVO_OK;
}

int ar_check_camera(const svo_ar_camera* c, const char* who, int i) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "%s: no cameras", who);
    bool finite = std::isfinite(c->fx) && std::isfinite(c->fy) && std::isfinite(c->cx) && std::isfinite(c->cy);
    for (float v : c->view) finite = finite && std::isfinite(v);
    if (!finite || !(c->fx > 0) || !(c->fy > 0))
        return svo_set_error(SVO_ERR_INVALID, "%s: camera %d: an entry is not finite, or fx or fy is not > 0", who, i);
    return SVO_OK;
}

int ar_check_occlusion(const svo_ar_occlusion* o, const char* who) {
    if (!o) return SVO_OK;
    if (o->on != 0 && o->on != 1) return svo_set_error(SVO_ERR_INVALID, "%s: occlusion: on %d is neither 0 nor 1", who, o->on);
    if (o->hidden != SVO_AR_HIDDEN_DROP && o->hidden != SVO_AR_HIDDEN_DIM) return svo_set_error(SVO_ERR_INVALID, "%s: occlusion: hidden %d", who, o->hidden);
    if (o->alpha < 0 || o->alpha > 256) return svo_set_error(SVO_ERR_INVALID, "%s: occlusion: alpha %d is not within 0 .. 256", who, o->alpha);
    if (!(o->margin >= 0) || !std::isfinite(o->margin)) return svo_set_error(SVO_ERR_INVALID, "%s: occlusion: margin is negative or not finite", who);
    if (o->_reserved[0] != 0 || o->_reserved[1] != 0 || o->_reserved[2] != 0 || o->_reserved2 != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: occlusion: a _reserved is not 0", who);
    return SVO_OK;
}

ArOcclusion ar_occlusion(const svo_ar_occlusion& o) { return ArOcclusion{o.hidden, o.alpha, o.margin, o.drop_flags}; }

ArParams ar_params(const svo_ar_style& s) {
    return ArParams{s.pixel == SVO_PIXEL_RGB8 ? 3 : 4, {s.light[0], s.light[1], s.light[2]}, s.ambient, s.near};
}

void ar_shape(const svo_ar_style& s, int cols, int rows, int64_t* pitch, int64_t* image_bytes) {
    const int64_t p = (int64_t)cols * (s.pixel == SVO_PIXEL_RGB8 ? 3 : 4);
    if (pitch) *pitch = p;
    if (image_bytes) *image_bytes = (p * rows + 255) / 256 * 256;
}

int ar_work(int image, int w, int h, const svo_ar_draw* draws, int n_draws, std::vector<ArSetup>& setup, std::vector<ArTile>& tiles) {
    ArTile t{image, 0, 0, 0};
    for (t.y0 = 0; t.y0 < h; t.y0 += AR_TILE_H)
        for (t.x0 = 0; t.x0 < w; t.x0 += AR_TILE_W) tiles.push_back(t);
    int rec = 0;
    for (int d = 0; d < n_draws; d++) {
        for (int t0 = 0; t0 < draws[d].n_triangles; t0 += AR_THREADS) setup.push_back(ArSetup{image, d, t0, rec + t0});
        rec += draws[d].n_triangles;
    }
    return rec;
}

__device__ __forceinline__ bool ar_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // (false for a NaN)

// o_k = ((m[4k] * x + m[4k+1] * y) + m[4k+2] * z) + m[4k+3]; false unless every o_k is finite
__device__ __forceinline__ bool ar_transform(const float m[12], const float v[3], float o[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = ((m[4 * k] * v[0] + m[4 * k + 1] * v[1]) + m[4 * k + 2] * v[2]) + m[4 * k + 3];
    return ar_finite(o[0]) && ar_finite(o[1]) && ar_finite(o[2]);
}

// c' = min(255, (int)(c * shade + 0.5f))
__device__ __forceinline__ uint32_t ar_channel(uint32_t c, float shade) { return (uint32_t)min(255, (int)((float)c * shade + 0.5f)); }

__global__ __launch_bounds__(AR_THREADS) void ar_setup_kernel(const ArSetup* __restrict__ items, const ArImage* __restrict__ images, const ArParams p) {
    const ArSetup it = G(items)[blockIdx.x];
    const ArImage im = G(images)[it.image];
    const svo_ar_draw dr = G(im.draws)[it.draw];
    const int t = it.t0 + (int)threadIdx.x, r = it.rec0 + (int)threadIdx.x;
    if (t >= dr.n_triangles || r >= im.n_records) return;
    SVO_GP(uint4) out = (SVO_GP(uint4))G(im.records) + (size_t)r * 4;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0, q2 = q0, q3 = make_uint4(1, 1, 0, 0);   // the empty box
    float w[3][3], c2[3];
    int X[3], Y[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int vi = G(dr.triangles)[(size_t)t * 3 + j];
        if ((unsigned)vi >= (unsigned)dr.n_vertices) { ok = false; break; }
        SVO_GP(const float) vp = G(dr.vertices) + (size_t)vi * 3;
        const float v[3] = {vp[0], vp[1], vp[2]};
        float c[3];
        if (!ar_transform(dr.model, v, w[j]) || !ar_transform(im.cam.view, w[j], c) || c[2] < p.near) { ok = false; break; }
        const float u = (im.cam.fx * c[0]) / c[2] + im.cam.cx, vv = (im.cam.fy * c[1]) / c[2] + im.cam.cy;
        if (!(fabsf(u) < 32768.f) || !(fabsf(vv) < 32768.f)) { ok = false; break; }   // (a NaN fails; no float -> int conversion of such a value)
        X[j] = (int)floorf(u * 16.f); Y[j] = (int)floorf(vv * 16.f);
        c2[j] = c[2];
    }
    if (ok) {
        const long long A = (long long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (X[2] - X[0]);
        // the pixels whose centre 16 p + 8 lies within [min, max]: ceil((min - 8) / 16) .. floor((max - 8) / 16)
        const int bx0 = max((min(X[0], min(X[1], X[2])) + 7) >> 4, 0), bx1 = min((max(X[0], max(X[1], X[2])) - 8) >> 4, im.w - 1);
        const int by0 = max((min(Y[0], min(Y[1], Y[2])) + 7) >> 4, 0), by1 = min((max(Y[0], max(Y[1], Y[2])) - 8) >> 4, im.h - 1);
        if (A != 0 && bx0 <= bx1 && by0 <= by1) {
            float e1[3], e2[3];
#pragma unroll
            for (int k = 0; k < 3; k++) { e1[k] = w[1][k] - w[0][k]; e2[k] = w[2][k] - w[0][k]; }
            const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
            const float q = (nx * nx + ny * ny) + nz * nz;
            const float d = (nx * p.light[0] + ny * p.light[1]) + nz * p.light[2];
            const float tt = fabsf(d) / sqrtf(q);
            const float s = (q == 0.f || tt != tt) ? 0.f : (tt < 1.f ? tt : 1.f);
            const float shade = p.ambient + (1.f - p.ambient) * s;
            const uint32_t rgb = dr.rgb ? G(dr.rgb)[t] : dr.rgb_all;
            const uint32_t col = ar_channel((rgb >> 16) & 0xffu, shade) << 16 | ar_channel((rgb >> 8) & 0xffu, shade) << 8 | ar_channel(rgb & 0xffu, shade);
            q0 = make_uint4((uint32_t)X[0], (uint32_t)Y[0], (uint32_t)X[1], (uint32_t)Y[1]);
            q1 = make_uint4((uint32_t)X[2], (uint32_t)Y[2], __float_as_uint(c2[0]), __float_as_uint(c2[1]));
            q2 = make_uint4(__float_as_uint(c2[2]), col, 0, 0);
            q3 = make_uint4((uint32_t)bx0, (uint32_t)by0, (uint32_t)bx1, (uint32_t)by1);
        }
    }
    out[0] = q0; out[1] = q1; out[2] = q2; out[3] = q3;
}

// A record's three edge functions as E_k(px, py) = e0[k] + ex[k] * px + ey[k] * py at the centre of pixel (px, py),
// already negated when A < 0, with (float)A, the depths and the colour
struct ArTri {
    long long e0[3], ex[3], ey[3];
    float fA, z[3];
    uint32_t rgb;
};

__device__ __forceinline__ ArTri ar_tri(const uint4 q0, const uint4 q1, const uint4 q2) {
    const int X[3] = {(int)q0.x, (int)q0.z, (int)q1.x}, Y[3] = {(int)q0.y, (int)q0.w, (int)q1.y};
    ArTri t;
    long long A = (long long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (X[2] - X[0]);
    const long long sg = A < 0 ? -1 : 1;
    A *= sg;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;          // E_k belongs to the edge a -> b, opposite vertex k
        const long long dX = sg * (X[b] - X[a]), dY = sg * (Y[b] - Y[a]);
        // dX (16 py + 8 - Ya) - dY (16 px + 8 - Xa)
        t.e0[k] = dX * (8 - Y[a]) - dY * (8 - X[a]);
        t.ex[k] = -16 * dY;
        t.ey[k] = 16 * dX;
    }
    t.fA = (float)A;
    t.z[0] = __uint_as_float(q1.z); t.z[1] = __uint_as_float(q1.w); t.z[2] = __uint_as_float(q2.x);
    t.rgb = q2.y;
    return t;
}

// the key of a covered pixel with edge values e (all >= 0)
__device__ __forceinline__ unsigned long long ar_key(const ArTri& t, long long e0, long long e1, long long e2) {
    const float l0 = (float)e0 / t.fA, l1 = (float)e1 / t.fA, l2 = (float)e2 / t.fA;
    const float z = (l0 * t.z[0] + l1 * t.z[1]) + l2 * t.z[2];
    return (unsigned long long)__float_as_uint(z) << 32 | t.rgb;
}

// What the occluded kernel gets beyond the three arguments of ar_render_kernel<false>
struct ArOcclArgs {
    const ArOccluder* occluders;
    ArOcclusion o;
};
constexpr int AR_OCC_CELLS = AR_TILE_W * AR_TILE_H;        // cells a tile can touch: most at step 1 (see the header comment)

// the staged occluder plane and the workgroup's two counters: LDS of ar_render_kernel<true> only
__device__ __forceinline__ float* ar_occ_plane() {
    __shared__ float occ[AR_OCC_CELLS];
    return occ;
}
__device__ __forceinline__ unsigned int* ar_occ_counts() {
    __shared__ unsigned int vis[2];
    return vis;
}

// a record as one float: its z where it occludes, +inf where nothing does (dropped, a drop_flags bit, z not finite or <= 0)
__device__ __forceinline__ float ar_occluder_depth(const uint4 r, uint32_t drop_flags) {
    const float z = __uint_as_float(r.z);
    const uint32_t flags = r.w >> 24;
    return ((flags & ((uint32_t)SVO_CLOUD_DROPPED | drop_flags)) == 0 && z > 0.f && ar_finite(z)) ? z : INFINITY;
}

// the lanes' counts (0 .. 4 each) summed over the wavefront: one ballot and popcount per bit
__device__ __forceinline__ unsigned int ar_wave_sum(int v) {
    return (unsigned int)(__popcll(__ballot(v & 1)) + 2 * __popcll(__ballot(v & 2)) + 4 * __popcll(__ballot(v & 4)));
}

// OCCLUDE = false: the kernel of "ar", three arguments. OCCLUDE = true: "ar occlusion", one ArOcclArgs more.
template <bool OCCLUDE, typename... Occl>
__global__ __launch_bounds__(AR_THREADS) void ar_render_kernel(const ArTile* __restrict__ tiles, const ArImage* __restrict__ images, const ArParams p,
                                                              const Occl... occl) {
    static_assert(sizeof...(Occl) == (OCCLUDE ? 1 : 0), "the occluded kernel takes one ArOcclArgs");
    const ArOcclArgs oa{occl...};                           // (OCCLUDE = false: all zero and never read)
    __shared__ unsigned long long keys[AR_TILE_W * AR_TILE_H];
    __shared__ int queue[AR_THREADS];
    __shared__ int n_queue;
    const ArTile t = G(tiles)[blockIdx.x];
    const ArImage im = G(images)[t.image];
    const int tid = threadIdx.x;
    const int tw = min(AR_TILE_W, im.w - t.x0), th = min(AR_TILE_H, im.h - t.y0);   // the tile's pixels inside the image
    const int bx0 = t.x0, bx1 = t.x0 + tw - 1, by0 = t.y0, by1 = t.y0 + th - 1;      // the tile, image coordinates
    const int lx = (tid & 15) * 4, ly = tid >> 4;                                   // this lane's pixels, tile coordinates

    // 1. the key plane
    for (int i = tid; i < AR_TILE_W * AR_TILE_H; i += AR_THREADS) keys[i] = ~0ull;
    if (tid == 0) n_queue = 0;
    // (occluded) the tile's cells [cx0, cx0 + ncx) x [cy0, cy0 + ncy) of the lattice, clipped to it; their records
    // are asked for here, 16 bytes a lane and consecutive lanes consecutive cells of a lattice row, and first used
    // after the record walk
    int cx0 = 0, cy0 = 0, ncx = 0, ncy = 0, n_cells = 0, step = 1;
    uint4 staged[AR_OCC_CELLS / AR_THREADS];
    if constexpr (OCCLUDE) {
        const ArOccluder oc = G(oa.occluders)[t.image];
        if (tid == 0) { ar_occ_counts()[0] = 0; ar_occ_counts()[1] = 0; }
        if (oc.records) {
            step = oc.step;
            cx0 = bx0 / step; cy0 = by0 / step;
            ncx = min(bx1 / step, oc.cols - 1) - cx0 + 1; ncy = min(by1 / step, oc.rows - 1) - cy0 + 1;
            if (ncx <= 0 || ncy <= 0) ncx = ncy = 0;             // the tile lies beyond the lattice
            n_cells = min(ncx * ncy, AR_OCC_CELLS);
        }
        SVO_GP(const uint4) cells = (SVO_GP(const uint4))G(oc.records);
        // cell c = tid + j * AR_THREADS is (c % ncx, c / ncx) of the tile's cells: one division, then carried
        const int div = max(ncx, 1), dq = AR_THREADS / div, dr = AR_THREADS % div;
        int cq = tid / div, cr = tid % div;
#pragma unroll
        for (int j = 0; j < AR_OCC_CELLS / AR_THREADS; j++) {
            if (tid + j * AR_THREADS < n_cells) staged[j] = cells[(int64_t)(cy0 + cq) * oc.cols + (cx0 + cr)];
            cq += dq; cr += dr;
            if (cr >= div) { cr -= div; cq++; }
        }
    }
    __syncthreads();

    // 2. and 3. the records
    SVO_GP(const uint4) recs = (SVO_GP(const uint4))G(im.records);
    int taken = 0;                                          // queue entries consumed so far (the ring's read position)
    for (int base = 0; base < im.n_records; base += AR_THREADS) {
        const int k = base + tid;
        int queued = 0;
        if (k < im.n_records) {
            const uint4 bb = recs[(size_t)k * 4 + 3];
            const int xa = max((int)bb.x, bx0), ya = max((int)bb.y, by0), xb = min((int)bb.z, bx1), yb = min((int)bb.w, by1);
            if (xa <= xb && ya <= yb) {
                if ((xb - xa + 1) * (yb - ya + 1) > AR_SMALL_PIXELS) {
                    queue[atomicAdd(&n_queue, 1) & (AR_THREADS - 1)] = k;   // (at most 256 per round, all taken before the next)
                    queued = 1;
                } else {
                    const ArTri tr = ar_tri(recs[(size_t)k * 4], recs[(size_t)k * 4 + 1], recs[(size_t)k * 4 + 2]);
                    for (int y = ya; y <= yb; y++) {
                        long long e0 = tr.e0[0] + tr.ex[0] * xa + tr.ey[0] * y, e1 = tr.e0[1] + tr.ex[1] * xa + tr.ey[1] * y,
                                  e2 = tr.e0[2] + tr.ex[2] * xa + tr.ey[2] * y;
                        for (int x = xa; x <= xb; x++) {
                            if ((e0 | e1 | e2) >= 0) atomicMin(&keys[(y - t.y0) * AR_TILE_W + (x - t.x0)], ar_key(tr, e0, e1, e2));
                            e0 += tr.ex[0]; e1 += tr.ex[1]; e2 += tr.ex[2];
                        }
                    }
                }
            }
        }
        if (__syncthreads_or(queued)) {
            const int m = n_queue - taken;
            for (int i = 0; i < m; i++) {
                const int kq = queue[(taken + i) & (AR_THREADS - 1)];
                const uint4 bb = recs[(size_t)kq * 4 + 3];
                // this lane's pixels inside the record's box (the box lies inside the image; the lane's row and
                // columns are clipped to it, so they lie inside the tile's part of the image too)
                const int y = t.y0 + ly;
                const int xa = max((int)bb.x, t.x0 + lx), xb = min((int)bb.z, t.x0 + lx + 3);
                if (y < (int)bb.y || y > (int)bb.w || xa > xb) continue;
                const ArTri tr = ar_tri(recs[(size_t)kq * 4], recs[(size_t)kq * 4 + 1], recs[(size_t)kq * 4 + 2]);
                long long e0 = tr.e0[0] + tr.ex[0] * xa + tr.ey[0] * y, e1 = tr.e0[1] + tr.ex[1] * xa + tr.ey[1] * y,
                          e2 = tr.e0[2] + tr.ex[2] * xa + tr.ey[2] * y;
                for (int x = xa; x <= xb; x++) {
                    if ((e0 | e1 | e2) >= 0) {
                        const unsigned long long key = ar_key(tr, e0, e1, e2);
                        unsigned long long& slot = keys[ly * AR_TILE_W + (x - t.x0)];
                        if (key < slot) slot = key;
                    }
                    e0 += tr.ex[0]; e1 += tr.ex[1]; e2 += tr.ex[2];
                }
            }
            taken += m;
            __syncthreads();
        }
    }
    // (every round ends with a barrier, so the keys are final here)

    // 4. decode and store; (occluded) the staged records become the plane of occluder depths first
    if constexpr (OCCLUDE) {
        float* occ = ar_occ_plane();
#pragma unroll
        for (int j = 0; j < AR_OCC_CELLS / AR_THREADS; j++) {
            const int c = tid + j * AR_THREADS;
            if (c < n_cells) occ[c] = ar_occluder_depth(staged[j], oa.o.drop_flags);
        }
        __syncthreads();
    }
    const int px = ly < th ? max(0, min(4, tw - lx)) : 0;                            // pixels of this lane: 0 .. 4
    if constexpr (!OCCLUDE)
        if (px == 0) return;
    int n_covered = 0, n_hidden = 0;                                                 // (occluded) of this lane's pixels
    if (px > 0) {
        const int x = t.x0 + lx, y = t.y0 + ly;
        SVO_GP(const uint8_t) g = G(im.src) + (int64_t)y * im.src_stride + x;
        uint32_t rgb[4];                                                             // r | g << 8 | b << 16 | 255 << 24
        // (occluded) the cell of pixel x + i, relative to the tile's first: x / step once, then carried with x % step.
        // x >= bx0 and y >= by0, so ix, iy >= 0
        int ix = 0, xr = 0, iy = 0;
        if constexpr (OCCLUDE) {
            ix = x / step - cx0; xr = x % step; iy = y / step - cy0;
        }
        for (int i = 0; i < 4; i++) {
            const unsigned long long key = keys[ly * AR_TILE_W + lx + i];
            bool hide = false;
            if constexpr (OCCLUDE) {
                const int at = iy * ncx + ix;
                const bool has_cell = ix < ncx && iy < ncy && at < n_cells;          // a cell outside the staged ones occludes nothing
                if (++xr == step) { xr = 0; ix++; }
                if (key != ~0ull && i < px) {
                    const float zo = has_cell ? ar_occ_plane()[at] : INFINITY;
                    hide = __uint_as_float((uint32_t)(key >> 32)) > zo + oa.o.margin;
                    n_covered++;
                    n_hidden += hide;
                }
            }
            bool background = key == ~0ull;
            if constexpr (OCCLUDE) {
                background = background || (hide && oa.o.hidden == SVO_AR_HIDDEN_DROP);
            }
            if (background) {
                const uint32_t v = i < px ? g[i] : 0;
                rgb[i] = v | v << 8 | v << 16 | 0xff000000u;
            } else {
                uint32_t c = (uint32_t)key;
                if constexpr (OCCLUDE) {
                    if (hide) {                                                      // dim: (c' (256 - a) + g a + 128) >> 8 per channel
                        const uint32_t a = (uint32_t)oa.o.alpha, ga = (uint32_t)g[i] * a + 128u;
                        c = ((((c >> 16) & 0xffu) * (256u - a) + ga) >> 8) << 16 | ((((c >> 8) & 0xffu) * (256u - a) + ga) >> 8) << 8 |
                            (((c & 0xffu) * (256u - a) + ga) >> 8);
                    }
                }
                rgb[i] = ((c >> 16) & 0xffu) | (c & 0xff00u) | ((c & 0xffu) << 16) | 0xff000000u;
            }
        }
        SVO_GP(uint8_t) d = G(im.dst) + ((int64_t)y * im.w + x) * p.bpp;
        if (p.bpp == 4) {
            if (px == 4 && ((uintptr_t)d & 15) == 0) {
                *(SVO_GP(uint4))d = make_uint4(rgb[0], rgb[1], rgb[2], rgb[3]);
            } else {
                for (int i = 0; i < px; i++) ((SVO_GP(uint32_t))d)[i] = rgb[i];      // (an RGBA image is 4-byte aligned)
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
    // (occluded) the counts: per wavefront by ballot and popcount, per workgroup in LDS, then one pair of 64-bit
    // integer adds to the image's counters. Every lane of the workgroup arrives here.
    if constexpr (OCCLUDE) {
        unsigned int* vis = ar_occ_counts();
        const unsigned int wave_covered = ar_wave_sum(n_covered), wave_hidden = ar_wave_sum(n_hidden);
        if ((tid & (warpSize - 1)) == 0) {
            if (wave_covered) atomicAdd(&vis[0], wave_covered);
            if (wave_hidden) atomicAdd(&vis[1], wave_hidden);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long* counts = G(oa.occluders)[t.image].counts;
            if (vis[0]) atomicAdd(&counts[0], (unsigned long long)vis[0]);
            if (vis[1]) atomicAdd(&counts[1], (unsigned long long)vis[1]);
        }
    }
}

void launch_ar_setup(const ArSetup* d_setup, int n_setup, const ArImage* d_images, const ArParams& p, hipStream_t stream) {
    if (n_setup <= 0) return;
    hipLaunchKernelGGL(ar_setup_kernel, dim3(n_setup), dim3(AR_THREADS), 0, stream, d_setup, d_images, p);
}

void launch_ar(const ArTile* d_tiles, int n_tiles, const ArImage* d_images, const ArParams& p, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL((ar_render_kernel<false>), dim3(n_tiles), dim3(AR_THREADS), 0, stream, d_tiles, d_images, p);
}

void launch_ar_occluded(const ArTile* d_tiles, int n_tiles, const ArImage* d_images, const ArOccluder* d_occluders, const ArParams& p,
                        const ArOcclusion& o, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL((ar_render_kernel<true, ArOcclArgs>), dim3(n_tiles), dim3(AR_THREADS), 0, stream, d_tiles, d_images, p,
                       ArOcclArgs{d_occluders, o});
}

}  // namespace svo
