// rectify.hip — the input stage of EurocInput::read (src/app/euroc_input.cpp:69-70):
// cv::remap(raw, out, M1, M2, INTER_LINEAR) with BORDER_CONSTANT 0 on 8-bit images and CV_32FC1 maps,
// bit-exact to OpenCV's fixed-point path (RemapInvoker + remapBilinear, INTER_BITS = 5,
// INTER_REMAP_COEF_BITS = 15). Per output pixel, m = (map_x, map_y):
//
//  * m non-finite or |m*32| >= 2^31: 0 (cvRound gives INT_MIN there: outside every image);
//  * X = round_half_even(mx*32), Y likewise (the product is exact); sx = X >> 5, sy = Y >> 5 (floor),
//    fx = X & 31, fy = Y & 31;
//  * taps v00 = src[sy][sx], v01 = src[sy][sx+1], v10 = src[sy+1][sx], v11 = src[sy+1][sx+1], 0 outside
//    the image; weights 32(32-fx)(32-fy), 32 fx(32-fy), 32(32-fx)fy, 32 fx fy (sum 2^15);
//  * out = (sum w v + 2^14) >> 15 = (sum' + 512) >> 10 over the products without the factor 32.
//    OpenCV's int16 table stores 32767 for the weight 2^15 of an integer position and moves the
//    remainder to another tap; the result is still v00 there (the difference is below 2^14).
//
// The kernels:
//  * remap_prep_kernel (once per map): float maps -> fixed point in 64x64 output tiles, with the
//    non-finite / range rule applied explicitly (a plain float->int conversion is undefined in C++ for
//    those and gives 0 for NaN on the GPU), plus per tile the bounding box of the source taps;
//  * remap_linear_kernel (per frame): one workgroup per (output tile, REMAP_SPB images, side). The
//    tile's map entries are loaded once (16 B per lane) and reused for every image of the workgroup.
//    Where the tile's source box, clipped to the image, fits REMAP_LDS_BYTES it is staged in LDS with
//    dword loads and the four taps are gathered from there; otherwise (random or extreme maps) they are
//    gathered from global memory. Four output pixels of a row per lane, stored as one dword.
//  * remap_linear_multi_kernel (per frame, when the images of a launch do not share one map: camera rigs):
//    the same per-image work, one workgroup per (output tile, chunk, side), where the host has sorted the
//    images by map and cut every run of equal maps into chunks of at most REMAP_SPB images; and
//    remap_linear_single_kernel, its form without the image loop for launches whose every chunk is one image.
//
// Every address a tap forms lies inside the source image (or the staged box, which is inside it): the
// tests are on clamped int16 positions (|x|, |y| <= 16384), so nothing can wrap.
#include "svo_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace svo {

constexpr int REMAP_THREADS = 256;
constexpr int REMAP_SPB = 16;              // images per workgroup of remap_linear_kernel (map entries read once for them)
constexpr int REMAP_LDS_BYTES = 12288;     // staged source box (EuRoC: at most 68 x 68 of a 64 x 64 tile)
constexpr int REMAP_ENTRIES = REMAP_TILE * REMAP_TILE;

static_assert(REMAP_THREADS == 16 * 16, "a lane covers 4 columns of 4 rows (16 lanes per 64-pixel row)");

size_t remap_map_bytes(int w, int h) {
    const size_t tiles = (size_t)((w + REMAP_TILE - 1) / REMAP_TILE) * ((h + REMAP_TILE - 1) / REMAP_TILE);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    return al(tiles * REMAP_ENTRIES * 4) + al(tiles * REMAP_ENTRIES * 2) + al(tiles * sizeof(int4));
}

RemapMap remap_map_view(void* base, int w, int h) {
    RemapMap m;
    m.w = w; m.h = h;
    m.tiles_x = (w + REMAP_TILE - 1) / REMAP_TILE;
    m.tiles_y = (h + REMAP_TILE - 1) / REMAP_TILE;
    const size_t tiles = (size_t)m.tiles_x * m.tiles_y;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    uint8_t* p = static_cast<uint8_t*>(base);
    m.xy = reinterpret_cast<const uint32_t*>(p);
    m.frac = reinterpret_cast<const uint16_t*>(p + al(tiles * REMAP_ENTRIES * 4));
    m.box = reinterpret_cast<const int4*>(p + al(tiles * REMAP_ENTRIES * 4) + al(tiles * REMAP_ENTRIES * 2));
    return m;
}

// one coordinate: X = round_half_even(m * 32) where |m * 32| < 2^31 (false for NaN and inf)
__device__ __forceinline__ int fix5(float m, bool& ok) {
    const float v = m * 32.0f;
    ok = fabsf(v) < 2147483648.0f;
    return ok ? (int)__builtin_rintf(v) : 0;
}

__global__ __launch_bounds__(REMAP_THREADS) void remap_prep_kernel(const float* __restrict__ map_x,
                                                                   const float* __restrict__ map_y, RemapMap m) {
    __shared__ int s_box[4];
    const int t = blockIdx.x;
    const int tx = t % m.tiles_x, ty = t / m.tiles_x;
    const int lane = threadIdx.x;
    const int c4 = (lane & 15) * 4, r0 = lane >> 4;
    if (lane == 0) { s_box[0] = INT_MAX; s_box[1] = INT_MIN; s_box[2] = INT_MAX; s_box[3] = INT_MIN; }
    __syncthreads();
    int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
    SVO_GP(const float) gx = G(map_x);
    SVO_GP(const float) gy = G(map_y);
    SVO_GP(uint4) oxy = (SVO_GP(uint4))G(const_cast<uint32_t*>(m.xy) + (size_t)t * REMAP_ENTRIES);
    SVO_GP(uint2) ofr = (SVO_GP(uint2))G(const_cast<uint16_t*>(m.frac) + (size_t)t * REMAP_ENTRIES);
    for (int k = 0; k < 4; k++) {
        const int r = r0 + 16 * k, y = ty * REMAP_TILE + r;
        uint32_t e[4], f[4];
        for (int j = 0; j < 4; j++) {
            const int x = tx * REMAP_TILE + c4 + j;
            int sx = -2, sy = -2, fr = 0;
            if (x < m.w && y < m.h) {
                bool okx, oky;
                const int X = fix5(gx[(size_t)y * m.w + x], okx);
                const int Y = fix5(gy[(size_t)y * m.w + x], oky);
                if (okx && oky) {
                    sx = min(max(X >> 5, -2), REMAP_MAX_SRC);
                    sy = min(max(Y >> 5, -2), REMAP_MAX_SRC);
                    fr = (X & 31) | (Y & 31) << 5;
                }
            }
            // taps sx, sx + 1 (sy, sy + 1) can fall inside an image of at most REMAP_MAX_SRC a side
            if (sx >= -1 && sx < REMAP_MAX_SRC && sy >= -1 && sy < REMAP_MAX_SRC) {
                bx0 = min(bx0, max(sx, 0)); bx1 = max(bx1, sx + 1);
                by0 = min(by0, max(sy, 0)); by1 = max(by1, sy + 1);
            }
            e[j] = ((uint32_t)sx & 0xffffu) | (uint32_t)sy << 16;
            f[j] = (uint32_t)fr;
        }
        oxy[r * 16 + (lane & 15)] = make_uint4(e[0], e[1], e[2], e[3]);
        ofr[r * 16 + (lane & 15)] = make_uint2(f[0] | f[1] << 16, f[2] | f[3] << 16);
    }
    if (bx0 != INT_MAX) {
        atomicMin(&s_box[0], bx0); atomicMax(&s_box[1], bx1);
        atomicMin(&s_box[2], by0); atomicMax(&s_box[3], by1);
    }
    __syncthreads();
    if (lane == 0) {
        int4* ob = const_cast<int4*>(m.box) + t;
        *G(ob) = s_box[0] == INT_MAX ? make_int4(0, -1, 0, -1) : make_int4(s_box[0], s_box[1], s_box[2], s_box[3]);
    }
}

// the 16 output pixels of a lane (4 rows r0 + 16k, 4 columns c4 .. c4+3) of one image, a row of 4 at a
// time: tap(x, y) -> 0..255, store(k, 4 pixels). The scheduling barrier keeps the rows apart (hoisting all
// 64 taps costs more registers than the occupancy allows).
template <typename Tap, typename Store>
__device__ __forceinline__ void remap_gather(const uint32_t (&xy)[16], const uint32_t (&fr)[8], Tap tap, Store store) {
    for (int k = 0; k < 4; k++) {
        uint32_t packed = 0;
        for (int j = 0; j < 4; j++) {
            const uint32_t e = xy[4 * k + j];
            const uint32_t f = (fr[2 * k + (j >> 1)] >> (16 * (j & 1))) & 0xffffu;
            const int sx = (int)(int16_t)(e & 0xffffu), sy = (int)e >> 16;
            const int fx = (int)(f & 31u), fy = (int)(f >> 5) & 31;
            const int v00 = tap(sx, sy), v01 = tap(sx + 1, sy), v10 = tap(sx, sy + 1), v11 = tap(sx + 1, sy + 1);
            const int s = v00 * (32 - fx) * (32 - fy) + v01 * fx * (32 - fy) + v10 * (32 - fx) * fy + v11 * fx * fy;
            packed |= (uint32_t)((s + 512) >> 10) << (8 * j);
        }
        store(k, packed);
        __builtin_amdgcn_sched_barrier(0);
    }
}

__global__ __launch_bounds__(REMAP_THREADS) void remap_linear_kernel(RemapLaunch a) {
    __shared__ uint32_t s_src[REMAP_LDS_BYTES / 4];
    const int side = blockIdx.z;
    const RemapMap m = side ? a.map[1] : a.map[0];
    const int t = blockIdx.x;
    const int tx = t % m.tiles_x, ty = t / m.tiles_x;
    const int lane = threadIdx.x;
    const int c4 = (lane & 15) * 4, r0 = lane >> 4;
    // the tile's map entries: once for every image of the workgroup
    uint32_t xy[16], fr[8];
    SVO_GP(const uint4) pxy = (SVO_GP(const uint4))G(m.xy + (size_t)t * REMAP_ENTRIES);
    SVO_GP(const uint2) pfr = (SVO_GP(const uint2))G(m.frac + (size_t)t * REMAP_ENTRIES);
    for (int k = 0; k < 4; k++) {
        const uint4 v = pxy[(r0 + 16 * k) * 16 + (lane & 15)];
        const uint2 f = pfr[(r0 + 16 * k) * 16 + (lane & 15)];
        xy[4 * k] = v.x; xy[4 * k + 1] = v.y; xy[4 * k + 2] = v.z; xy[4 * k + 3] = v.w;
        fr[2 * k] = f.x; fr[2 * k + 1] = f.y;
    }
    const int4 box = *G(m.box + t);
    const int i0 = blockIdx.y * REMAP_SPB, i1 = min(a.n, i0 + REMAP_SPB);
    for (int i = i0; i < i1; i++) {
        // (the entries pass through an empty asm per image: otherwise the decoded positions and weights of
        // all 16 pixels are hoisted out of the image loop, 256 VGPRs instead of the ~60 the kernel needs)
        for (int j = 0; j < 16; j++) asm volatile("" : "+v"(xy[j]));
        for (int j = 0; j < 8; j++) asm volatile("" : "+v"(fr[j]));
        const RemapImg im = G(a.img)[side * a.n + i];
        const ImgView src = im.src, dst = im.dst;
        // the tile's source box on this image (x0, y0 >= 0 already)
        const int bx0 = box.x, bx1 = min(box.y, src.w - 1), by0 = box.z, by1 = min(box.w, src.h - 1);
        const bool empty = bx1 < bx0 || by1 < by0;
        const int xs = bx0 & ~3;                                   // staged from a dword boundary
        const int nd = empty ? 0 : ((bx1 - xs) >> 2) + 1;          // dwords per staged row
        const int rows = empty ? 0 : by1 - by0 + 1;
        const bool dal = ((reinterpret_cast<uintptr_t>(dst.data) | (uintptr_t)dst.stride) & 3) == 0;
        const int X = tx * REMAP_TILE + c4;
        auto store = [&](int k, uint32_t v) {
            const int Y = ty * REMAP_TILE + r0 + 16 * k;
            if (Y >= dst.h || X >= dst.w) return;
            SVO_GP(uint8_t) drow = dst.gw() + (size_t)Y * dst.stride;
            if (dal && X + 3 < dst.w) {
                *(SVO_GP(uint32_t))(drow + X) = v;
            } else {
                for (int j = 0; j < 4; j++)
                    if (X + j < dst.w) drow[X + j] = (uint8_t)(v >> (8 * j));
            }
        };
        if ((long long)rows * nd * 4 <= REMAP_LDS_BYTES) {
            __syncthreads();                                       // the previous image's gather is done
            const bool al = ((reinterpret_cast<uintptr_t>(src.data) | (uintptr_t)src.stride) & 3) == 0;
            SVO_GP(const uint8_t) sp = src.g();
            for (int idx = lane; idx < rows * nd; idx += REMAP_THREADS) {
                const int r = idx / nd, d = idx - r * nd;
                const int col = xs + 4 * d;                        // 0 <= col <= bx1 < src.w
                SVO_GP(const uint8_t) row = sp + (size_t)(by0 + r) * src.stride;
                uint32_t v;
                if (al && col + 3 < src.w) {
                    v = *(SVO_GP(const uint32_t))(row + col);
                } else {
                    v = 0;
                    for (int j = 0; j < 4; j++)
                        if (col + j < src.w) v |= (uint32_t)row[col + j] << (8 * j);
                }
                s_src[idx] = v;
            }
            __syncthreads();
            const SVO_LDS(uint8_t)* lds = (const SVO_LDS(uint8_t)*)s_src;
            const int pitch = nd * 4;
            const unsigned bw = (unsigned)(bx1 - bx0), bh = (unsigned)(by1 - by0);
            remap_gather(xy, fr, [&](int x, int y) -> int {
                const bool in = !empty && (unsigned)(x - bx0) <= bw && (unsigned)(y - by0) <= bh;
                return in ? (int)lds[(y - by0) * pitch + (x - xs)] : 0;
            }, store);
        } else {
            SVO_GP(const uint8_t) sp = src.g();
            remap_gather(xy, fr, [&](int x, int y) -> int {
                const bool in = (unsigned)x < (unsigned)src.w && (unsigned)y < (unsigned)src.h;
                return in ? (int)sp[(size_t)y * src.stride + x] : 0;
            }, store);
        }
    }
}

// ---- a map per image. remap_linear_kernel above stays as it was measured; the forms below restate its
// per-image work as functions of the tile's entries

// the tile's map entries as a lane holds them: 16 positions, 16 fractions (two per dword), the tile's source box
struct RemapTile {
    uint32_t xy[16], fr[8];
    int4 box;
};

__device__ __forceinline__ void remap_load_tile(const RemapMap& m, int t, int lane, RemapTile& e) {
    const int r0 = lane >> 4;
    SVO_GP(const uint4) pxy = (SVO_GP(const uint4))G(m.xy + (size_t)t * REMAP_ENTRIES);
    SVO_GP(const uint2) pfr = (SVO_GP(const uint2))G(m.frac + (size_t)t * REMAP_ENTRIES);
    for (int k = 0; k < 4; k++) {
        const uint4 v = pxy[(r0 + 16 * k) * 16 + (lane & 15)];
        const uint2 f = pfr[(r0 + 16 * k) * 16 + (lane & 15)];
        e.xy[4 * k] = v.x; e.xy[4 * k + 1] = v.y; e.xy[4 * k + 2] = v.z; e.xy[4 * k + 3] = v.w;
        e.fr[2 * k] = f.x; e.fr[2 * k + 1] = f.y;
    }
    e.box = *G(m.box + t);
}

// output tile (tx, ty) of one image through the entries `e`: the LDS box path where the tile's source box fits,
// else the global gather (both kernels below)
__device__ __forceinline__ void remap_image(const RemapTile& e, const RemapImg& im, int tx, int ty, int lane, uint32_t* s_src) {
    const int c4 = (lane & 15) * 4, r0 = lane >> 4;
    const int4 box = e.box;
    const ImgView src = im.src, dst = im.dst;
    // the tile's source box on this image (x0, y0 >= 0 already)
    const int bx0 = box.x, bx1 = min(box.y, src.w - 1), by0 = box.z, by1 = min(box.w, src.h - 1);
    const bool empty = bx1 < bx0 || by1 < by0;
    const int xs = bx0 & ~3;                                   // staged from a dword boundary
    const int nd = empty ? 0 : ((bx1 - xs) >> 2) + 1;          // dwords per staged row
    const int rows = empty ? 0 : by1 - by0 + 1;
    const bool dal = ((reinterpret_cast<uintptr_t>(dst.data) | (uintptr_t)dst.stride) & 3) == 0;
    const int X = tx * REMAP_TILE + c4;
    auto store = [&](int k, uint32_t v) {
        const int Y = ty * REMAP_TILE + r0 + 16 * k;
        if (Y >= dst.h || X >= dst.w) return;
        SVO_GP(uint8_t) drow = dst.gw() + (size_t)Y * dst.stride;
        if (dal && X + 3 < dst.w) {
            *(SVO_GP(uint32_t))(drow + X) = v;
        } else {
            for (int j = 0; j < 4; j++)
                if (X + j < dst.w) drow[X + j] = (uint8_t)(v >> (8 * j));
        }
    };
    if ((long long)rows * nd * 4 <= REMAP_LDS_BYTES) {
        __syncthreads();                                       // the previous image's gather is done
        const bool al = ((reinterpret_cast<uintptr_t>(src.data) | (uintptr_t)src.stride) & 3) == 0;
        SVO_GP(const uint8_t) sp = src.g();
        for (int idx = lane; idx < rows * nd; idx += REMAP_THREADS) {
            const int r = idx / nd, d = idx - r * nd;
            const int col = xs + 4 * d;                        // 0 <= col <= bx1 < src.w
            SVO_GP(const uint8_t) row = sp + (size_t)(by0 + r) * src.stride;
            uint32_t v;
            if (al && col + 3 < src.w) {
                v = *(SVO_GP(const uint32_t))(row + col);
            } else {
                v = 0;
                for (int j = 0; j < 4; j++)
                    if (col + j < src.w) v |= (uint32_t)row[col + j] << (8 * j);
            }
            s_src[idx] = v;
        }
        __syncthreads();
        const SVO_LDS(uint8_t)* lds = (const SVO_LDS(uint8_t)*)s_src;
        const int pitch = nd * 4;
        const unsigned bw = (unsigned)(bx1 - bx0), bh = (unsigned)(by1 - by0);
        remap_gather(e.xy, e.fr, [&](int x, int y) -> int {
            const bool in = !empty && (unsigned)(x - bx0) <= bw && (unsigned)(y - by0) <= bh;
            return in ? (int)lds[(y - by0) * pitch + (x - xs)] : 0;
        }, store);
    } else {
        SVO_GP(const uint8_t) sp = src.g();
        remap_gather(e.xy, e.fr, [&](int x, int y) -> int {
            const bool in = (unsigned)x < (unsigned)src.w && (unsigned)y < (unsigned)src.h;
            return in ? (int)sp[(size_t)y * src.stride + x] : 0;
        }, store);
    }
}

// (the entries pass through an empty asm per image of a loop: otherwise the decoded positions and weights of
// all 16 pixels are hoisted out of the image loop, 256 VGPRs instead of the ~60 the kernel needs)
__device__ __forceinline__ void remap_pin_tile(RemapTile& e) {
    for (int j = 0; j < 16; j++) asm volatile("" : "+v"(e.xy[j]));
    for (int j = 0; j < 8; j++) asm volatile("" : "+v"(e.fr[j]));
}

// A map per image: workgroup (output tile, chunk blockIdx.y of the table, side). A chunk is at most REMAP_SPB
// images of one run (images that share a map), so they still share the tile's map loads. LOOP = false: every
// chunk of the launch is one image (a map of its own per image): no image loop, nothing kept live across one.
template <bool LOOP>
__device__ __forceinline__ void remap_multi(const RemapMultiLaunch& a, uint32_t* s_src) {
    const int side = blockIdx.z;
    const RemapChunk ch = G(a.chunks)[blockIdx.y];
    RemapMap m = a.shape;                                      // the launch's maps differ in their storage only
    const uint8_t* base = side ? ch.map[1] : ch.map[0];
    m.xy = reinterpret_cast<const uint32_t*>(base);
    m.frac = reinterpret_cast<const uint16_t*>(base + a.frac_offset);
    m.box = reinterpret_cast<const int4*>(base + a.box_offset);
    const int t = blockIdx.x;
    const int tx = t % m.tiles_x, ty = t / m.tiles_x;
    const int lane = threadIdx.x;
    RemapTile e;
    remap_load_tile(m, t, lane, e);
    if (LOOP) {
        const int i1 = min(a.n, ch.first + min(ch.count, REMAP_SPB));
        for (int i = max(ch.first, 0); i < i1; i++) {
            remap_pin_tile(e);
            const RemapImg im = G(a.img)[side * a.n + i];
            remap_image(e, im, tx, ty, lane, s_src);
        }
    } else if (ch.first >= 0 && ch.first < a.n) {
        const RemapImg im = G(a.img)[side * a.n + ch.first];
        remap_image(e, im, tx, ty, lane, s_src);
    }
}

__global__ __launch_bounds__(REMAP_THREADS) void remap_linear_multi_kernel(RemapMultiLaunch a) {
    __shared__ uint32_t s_src[REMAP_LDS_BYTES / 4];
    remap_multi<true>(a, s_src);
}

__global__ __launch_bounds__(REMAP_THREADS) void remap_linear_single_kernel(RemapMultiLaunch a) {
    __shared__ uint32_t s_src[REMAP_LDS_BYTES / 4];
    remap_multi<false>(a, s_src);
}

// ---- maps from calibrations: cv::initUndistortRectifyMap (src/app/euroc_input.cpp:48-49), the f64 statement of
// include/svo_hip.h. One workgroup per (output tile, camera), a lane's 16 pixels as in remap_prep_kernel, a row of 4
// at a time (the scheduling barrier keeps the f64 temporaries of the rows apart). The camera's block is uniform per
// workgroup and only read: it comes through the constant address space (scalar loads into SGPRs). -ffp-contract=off
// keeps every product and sum rounded on its own, and f64 division is correctly rounded: the floats are the
// statement's, bit for bit.
//  * FUSED = false (svo_build_rectify_maps): the two floats are stored, a row of 4 as one 16-byte store where the
//    row pitch and the plane's address allow;
//  * FUSED = true (svo_ctx_add_rigs_calibrated, svo_ctx_set_calibration): the float goes straight through what
//    remap_prep_kernel does with it: fix5, the packed entries, the tile's source box. No float plane exists.
#if defined(__HIP_DEVICE_COMPILE__)
#define SVO_KP(T) __attribute__((address_space(4))) T*
#else
#define SVO_KP(T) T*
#endif

template <bool FUSED>
__global__ __launch_bounds__(REMAP_THREADS) void rig_maps_kernel(const RigCam* __restrict__ cams, RemapMap m,
                                                                 size_t frac_offset, size_t box_offset) {
    __shared__ int s_box[4];
    const int tiles = m.tiles_x * m.tiles_y;
    const int cam = blockIdx.x / tiles, t = blockIdx.x - cam * tiles;
    const int tx = t % m.tiles_x, ty = t / m.tiles_x;
    const int lane = threadIdx.x;
    const int c4 = (lane & 15) * 4, r0 = lane >> 4;
    const RigCam c = ((SVO_KP(const RigCam))cams)[cam];
    if (FUSED) {
        if (lane == 0) { s_box[0] = INT_MAX; s_box[1] = INT_MIN; s_box[2] = INT_MAX; s_box[3] = INT_MIN; }
        __syncthreads();
    }
    int bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN;
    SVO_GP(float) gx = G(c.map_x);
    SVO_GP(float) gy = G(c.map_y);
    SVO_GP(uint4) oxy = (SVO_GP(uint4))G(reinterpret_cast<uint32_t*>(c.fixed) + (size_t)t * REMAP_ENTRIES);
    SVO_GP(uint2) ofr = (SVO_GP(uint2))G(reinterpret_cast<uint16_t*>(c.fixed + frac_offset) + (size_t)t * REMAP_ENTRIES);
    const bool vec = (m.w & 3) == 0 && ((reinterpret_cast<uintptr_t>(c.map_x) | reinterpret_cast<uintptr_t>(c.map_y)) & 15) == 0;
    const int x0 = tx * REMAP_TILE + c4;
    for (int k = 0; k < 4; k++) {
        const int r = r0 + 16 * k, y = ty * REMAP_TILE + r;
        const double i = (double)y;
        const double rowX = i * c.ir[1] + c.ir[2], rowY = i * c.ir[4] + c.ir[5], rowW = i * c.ir[7] + c.ir[8];
        float mx[4], my[4];
        for (int j = 0; j < 4; j++) {
            const double col = (double)(x0 + j);
            const double X = col * c.ir[0] + rowX, Y = col * c.ir[3] + rowY, W = col * c.ir[6] + rowW;
            const double iw = 1.0 / W;
            const double x = X * iw, yy = Y * iw;
            const double x2 = x * x, y2 = yy * yy, r2 = x2 + y2, _2xy = (2 * x) * yy;
            const double kr = (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) / (1 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
            const double xd = (x * kr + c.p1 * _2xy) + c.p2 * (r2 + 2 * x2);
            const double yd = (yy * kr + c.p1 * (r2 + 2 * y2)) + c.p2 * _2xy;
            mx[j] = (float)(c.fx * xd + c.u0);
            my[j] = (float)(c.fy * yd + c.v0);
        }
        if (!FUSED) {
            if (y < m.h && x0 < m.w) {
                const size_t o = (size_t)y * m.w + x0;
                if (vec && x0 + 3 < m.w) {
                    *(SVO_GP(float4))(gx + o) = make_float4(mx[0], mx[1], mx[2], mx[3]);
                    *(SVO_GP(float4))(gy + o) = make_float4(my[0], my[1], my[2], my[3]);
                } else {
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < m.w) { gx[o + j] = mx[j]; gy[o + j] = my[j]; }
                }
            }
        } else {
            // (remap_prep_kernel's entry of the float it would have read)
            uint32_t e[4], f[4];
            for (int j = 0; j < 4; j++) {
                int sx = -2, sy = -2, fr = 0;
                if (x0 + j < m.w && y < m.h) {
                    bool okx, oky;
                    const int X = fix5(mx[j], okx);
                    const int Y = fix5(my[j], oky);
                    if (okx && oky) {
                        sx = min(max(X >> 5, -2), REMAP_MAX_SRC);
                        sy = min(max(Y >> 5, -2), REMAP_MAX_SRC);
                        fr = (X & 31) | (Y & 31) << 5;
                    }
                }
                if (sx >= -1 && sx < REMAP_MAX_SRC && sy >= -1 && sy < REMAP_MAX_SRC) {
                    bx0 = min(bx0, max(sx, 0)); bx1 = max(bx1, sx + 1);
                    by0 = min(by0, max(sy, 0)); by1 = max(by1, sy + 1);
                }
                e[j] = ((uint32_t)sx & 0xffffu) | (uint32_t)sy << 16;
                f[j] = (uint32_t)fr;
            }
            oxy[r * 16 + (lane & 15)] = make_uint4(e[0], e[1], e[2], e[3]);
            ofr[r * 16 + (lane & 15)] = make_uint2(f[0] | f[1] << 16, f[2] | f[3] << 16);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (FUSED) {
        if (bx0 != INT_MAX) {
            atomicMin(&s_box[0], bx0); atomicMax(&s_box[1], bx1);
            atomicMin(&s_box[2], by0); atomicMax(&s_box[3], by1);
        }
        __syncthreads();
        if (lane == 0) {
            int4* ob = reinterpret_cast<int4*>(c.fixed + box_offset) + t;
            *G(ob) = s_box[0] == INT_MAX ? make_int4(0, -1, 0, -1) : make_int4(s_box[0], s_box[1], s_box[2], s_box[3]);
        }
    }
}

bool rectify_inverse(const svo_camera_calibration& cal, double ir[9]) {
    const double* all[4] = {cal.K, cal.D, cal.R, cal.P};
    const int len[4] = {9, 8, 9, 9};
    for (int q = 0; q < 4; q++)
        for (int k = 0; k < len[q]; k++)
            if (!std::isfinite(all[q][k])) return false;
    const double *P = cal.P, *R = cal.R;
    double M[9];
    for (int r = 0; r < 3; r++)
        for (int cc = 0; cc < 3; cc++) M[3 * r + cc] = (P[3 * r] * R[cc] + P[3 * r + 1] * R[3 + cc]) + P[3 * r + 2] * R[6 + cc];
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double det = (a * c00 + b * c01) + c * c02;
    if (det == 0 || !std::isfinite(det)) return false;
    const double t = 1.0 / det;
    const double out[9] = {c00 * t, (c * h - b * i) * t, (b * f - c * e) * t,
                           c01 * t, (a * i - c * g) * t, (c * d - a * f) * t,
                           c02 * t, (b * g - a * h) * t, (a * e - b * d) * t};
    std::copy(out, out + 9, ir);
    return true;
}

bool rig_camera(const svo_camera_calibration& cal, RigCam& out) {
    if (!rectify_inverse(cal, out.ir)) return false;
    out.fx = cal.K[0]; out.fy = cal.K[4]; out.u0 = cal.K[2]; out.v0 = cal.K[5];
    out.k1 = cal.D[0]; out.k2 = cal.D[1]; out.p1 = cal.D[2]; out.p2 = cal.D[3];
    out.k3 = cal.D[4]; out.k4 = cal.D[5]; out.k5 = cal.D[6]; out.k6 = cal.D[7];
    out.map_x = out.map_y = nullptr;
    out.fixed = nullptr;
    return true;
}

void launch_rig_maps(const RigCam* d_cams, int n, int w, int h, bool fused, hipStream_t stream) {
    if (n <= 0) return;
    const RemapMap m = remap_map_view(nullptr, w, h);            // (a view on a null base: the offsets in a map's storage)
    const size_t frac_offset = reinterpret_cast<uintptr_t>(m.frac), box_offset = reinterpret_cast<uintptr_t>(m.box);
    const dim3 grid((unsigned)(m.tiles_x * m.tiles_y) * (unsigned)n);
    if (fused) hipLaunchKernelGGL(rig_maps_kernel<true>, grid, dim3(REMAP_THREADS), 0, stream, d_cams, m, frac_offset, box_offset);
    else hipLaunchKernelGGL(rig_maps_kernel<false>, grid, dim3(REMAP_THREADS), 0, stream, d_cams, m, frac_offset, box_offset);
}

void launch_remap_prep(const float* map_x, const float* map_y, const RemapMap& m, hipStream_t stream) {
    hipLaunchKernelGGL(remap_prep_kernel, dim3(m.tiles_x * m.tiles_y), dim3(REMAP_THREADS), 0, stream, map_x, map_y, m);
}

void launch_remap(const RemapLaunch& a, int n_sides, hipStream_t stream) {
    const RemapMap& m = a.map[0];
    dim3 grid(m.tiles_x * m.tiles_y, (a.n + REMAP_SPB - 1) / REMAP_SPB, n_sides);
    hipLaunchKernelGGL(remap_linear_kernel, grid, dim3(REMAP_THREADS), 0, stream, a);
}

int remap_chunks(const int* map_of_image, int n, std::vector<int>& order, std::vector<RemapChunkSpan>& chunks) {
    order.resize((size_t)n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return map_of_image[a] < map_of_image[b]; });
    chunks.clear();
    int longest = 0;
    for (int i0 = 0; i0 < n;) {
        int i1 = i0 + 1;
        while (i1 < n && map_of_image[order[i1]] == map_of_image[order[i0]]) i1++;
        longest = std::max(longest, i1 - i0);
        for (int k = i0; k < i1; k += REMAP_SPB) chunks.push_back({map_of_image[order[i0]], k, std::min(REMAP_SPB, i1 - k)});
        i0 = i1;
    }
    return longest;
}

void launch_remap_multi(RemapMultiLaunch a, int w, int h, int n_chunks, bool single_images, int n_sides, hipStream_t stream) {
    a.shape = remap_map_view(nullptr, w, h);
    a.frac_offset = reinterpret_cast<uintptr_t>(a.shape.frac);   // (views on a null base: the offsets in a map's storage)
    a.box_offset = reinterpret_cast<uintptr_t>(a.shape.box);
    dim3 grid(a.shape.tiles_x * a.shape.tiles_y, n_chunks, n_sides);
    if (single_images) hipLaunchKernelGGL(remap_linear_single_kernel, grid, dim3(REMAP_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(remap_linear_multi_kernel, grid, dim3(REMAP_THREADS), 0, stream, a);
}

}  // namespace svo
