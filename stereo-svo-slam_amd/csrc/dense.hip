// dense.hip — the disparity search of ssd_disparity_kernel (depth.hip; DepthFilter::calculate_disparities,
// depth_filter.cpp:259-327, clamp_half = 1) at every point of a lattice, many image pairs in one launch. The picture
// is stated exactly in include/svo_hip.h ("dense"): the reference's clipped template and region boxes, the exact
// integer SSD rounded once to float, the first minimum in row-major order and the tie-averaged column. This file is
// that statement in a form whose work per lattice point and candidate does not grow with the window.
//
// For a fixed candidate offset (dy, j) the SSD of every point is a box sum over one plane,
//   E[yy][xx] = (R[yy + dy][xx + j] - L[yy][xx])^2,      SSD = sum of E over [y11, y12) x [x11, x12),
// indexed by the LEFT pixel, because x21 = x11 and the vertical offset of candidate k is dy = (y21 - y11) + k. So:
//
//  * a workgroup of 256 lanes owns 256 consecutive left columns (lane = column) and a band of at most DENSE_BAND
//    lattice rows. The left rows of the band (<= DENSE_L_ROWS) and the right rows around them (+- search_y, + search_x
//    columns) are staged in LDS once, zero outside the image;
//  * candidates are walked in the statement's order, dy outer (every point's k ascends with dy), j inner. Per
//    candidate a lane carries the column sum C of E over the template rows and slides it down the band: rows entering
//    [y11, y12) are added, rows leaving subtracted, so the clipped boxes at the top and bottom border need no branch
//    of their own. It keeps one C per lattice row of the band;
//  * the 64 lanes of a wave take an inclusive prefix sum of each C in the DPP network (six adds, no LDS), store it
//    and the wave's total in LDS, and after ONE barrier per candidate the lane of a lattice point reads
//    P[x12] - P[x11] per row: the clipped boxes at the left and right border and any step are only other indices.
//    The two sets of prefix buffers alternate;
//  * that lane converts the int32 once to float and updates (best, minx, sum, count) of the row, which live in
//    registers for the whole candidate walk (the row loops are unrolled: DENSE_BAND x 4 registers). The update is
//    written with selects: with branches hipcc (ROCm 7.2) copied the state arrays about under partial exec masks and
//    best[] kept the first candidate's value.
//
// Exact int32 throughout: a column sum is at most 35 * 255^2, a prefix over 256 columns 35 * 255^2 * 256 < 2^31.
// No atomics; a point's value depends on its candidates' order only, which is the same for any launch geometry.
// A lane at column x owns the lattice point at x when x lies in the tile's span of 257 - win columns: its template
// box [x - wb, x + wa] then lies inside the 256 columns (226 of 256 lanes carry points at win = 31, step 1).
//
// LDS: 48 x 256 + 64 x 320 + 2 x 8 x (256 + 4) x 4 = 49 408 bytes per workgroup, three workgroups per CU with 111 KB
// left beside them for the step kernels of another group. Bank behaviour: the 64 lanes of a wave read 64 consecutive
// bytes of a row.
//
// Bounds: every LDS index follows from tid, j <= 64, dy + search_y <= 16 and a left row in [yl0, yl0 + 48); global
// reads are guarded by 0 <= xx < w, 0 <= yy < h; of an image exactly out[0 .. planes * cols * rows) is written.
#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

constexpr int DENSE_THREADS = 256;
constexpr int DENSE_BAND = 8;                              // lattice rows of a workgroup at most (their state is in registers)
constexpr int DENSE_FEW_WORKGROUPS = 384;                  // below it a launch runs with half the band (dense_plan)
constexpr int DENSE_L_ROWS = 48;                           // left rows in LDS: (band - 1) * step + win <= 48
constexpr int DENSE_MAX_WIN = 35, DENSE_MAX_SX = 64, DENSE_MAX_SY = 8, DENSE_MAX_STEP = 16;
constexpr int DENSE_R_ROWS = DENSE_L_ROWS + 2 * DENSE_MAX_SY;
constexpr int DENSE_R_COLS = DENSE_THREADS + DENSE_MAX_SX;
static_assert(sizeof(svo_disparity_style) == 32 && sizeof(svo_disparity_segment) == 64 && sizeof(DenseImage) == 48, "record sizes");
static_assert((long long)DENSE_MAX_WIN * 255 * 255 * DENSE_THREADS < (1ll << 31), "a prefix over the columns fits int32");

// lattice rows of a workgroup and left columns that carry its points
__host__ __device__ inline int dense_band(int step, int win, int cap) {
    const int b = (DENSE_L_ROWS - win) / step + 1;
    return b < cap ? b : cap;
}
__host__ __device__ inline int dense_span(int win) { return DENSE_THREADS + 1 - win; }

int dense_check_style(const svo_disparity_style* s, const svo_camera_settings* cam, const char* who, DenseParams* out) {
    if (!s) return svo_set_error(SVO_ERR_INVALID, "%s: no style", who);
    if (s->value != SVO_DENSE_DISPARITY && s->value != SVO_DENSE_DEPTH) return svo_set_error(SVO_ERR_INVALID, "%s: value %d", who, s->value);
    if (s->step < 1 || s->step > DENSE_MAX_STEP) return svo_set_error(SVO_ERR_INVALID, "%s: step %d is not within 1 .. %d", who, s->step, DENSE_MAX_STEP);
    if (s->cost != 0 && s->cost != 1) return svo_set_error(SVO_ERR_INVALID, "%s: cost %d", who, s->cost);
    if (s->_reserved[0] != 0 || s->_reserved[1] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    if (!cam && (s->win == 0 || s->search_x == 0 || s->search_y == 0))
        return svo_set_error(SVO_ERR_INVALID, "%s: win, search_x and search_y must be given", who);
    const int win = s->win ? s->win : cam->window_size_depth_calculator;
    const int sx = s->search_x ? s->search_x : cam->search_x, sy = s->search_y ? s->search_y : cam->search_y;
    if (win < 1 || win > DENSE_MAX_WIN || sx < 0 || sx > DENSE_MAX_SX || sy < 0 || sy > DENSE_MAX_SY)
        return svo_set_error(SVO_ERR_INVALID, "%s: win %d, search_x %d, search_y %d: win 1 .. 35, search_x <= 64, search_y <= 8 supported", who,
                             win, sx, sy);
    if (out) *out = DenseParams{s->value, s->step, win, sx, sy, s->cost, DENSE_BAND};
    return SVO_OK;
}

void dense_shape(const DenseParams& p, int w, int h, int* cols, int* rows, int* planes, int64_t* image_bytes, int lr) {
    const int c = w / p.step, r = h / p.step, n = 1 + p.cost + lr;
    if (cols) *cols = c;
    if (rows) *rows = r;
    if (planes) *planes = n;
    if (image_bytes) *image_bytes = ((int64_t)n * c * r * 4 + 255) / 256 * 256;
}

int dense_tiles(const DenseParams& p, int w, int h) {
    const int span = dense_span(p.win), band = dense_band(p.step, p.win, p.band);
    return ((w + span - 1) / span) * ((h / p.step + band - 1) / band);
}

// A launch of few workgroups is bound by the latency of one wave per SIMD: half the band gives twice the workgroups,
// each with less to do. The values do not depend on the band.
// (SVO_DENSE_FEW_WORKGROUPS: another bound, so that tests reach both bands whatever their images' size)
void dense_plan(DenseParams& p, long long workgroups_at_full_band) {
    long long few = DENSE_FEW_WORKGROUPS;
    if (const char* e = std::getenv("SVO_DENSE_FEW_WORKGROUPS")) few = std::atoll(e);
    p.band = workgroups_at_full_band < few ? DENSE_BAND / 2 : DENSE_BAND;
}

// inclusive prefix sum over the 64 lanes of a wave in the DPP network: four shifts inside each row of 16 lanes (a lane
// without a source keeps the 0 of `old`), then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2, 3
__device__ __forceinline__ int dense_wave_prefix(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15, rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31, rows 2 and 3
    return v;
}

// MIRROR: the reverse search of the cross-check (include/svo_hip.h, "cross-check"; lr.hip has the rest). The point rule
// runs on the mirrored, swapped planes Lm[y][u] = R[y][W - 1 - u], Rm[y][u] = L[y][W - 1 - u]: the two staging loops
// read column W - 1 - xx of the other plane (byte loads: a wave reads 64 consecutive bytes in descending order, at any
// base and stride), the lattice has every column (column step 1) and the rows of the forward lattice, and the disparity
// of mirrored column u goes to out[iy][W - 1 - u], a plane of rows x W floats indexed by the right image's own column.
// Nothing after the staging differs. MIRROR = false is the kernel as it was.
template <bool MIRROR>
__global__ __launch_bounds__(DENSE_THREADS) void dense_disparity_kernel(const std::conditional_t<MIRROR, LrImage, DenseImage>* __restrict__ images,
                                                                        const DenseParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t s_l[DENSE_L_ROWS * DENSE_THREADS];
    __shared__ __attribute__((aligned(16))) uint8_t s_r[DENSE_R_ROWS * DENSE_R_COLS];
    __shared__ int s_p[2][DENSE_BAND][DENSE_THREADS];
    __shared__ int s_t[2][DENSE_BAND][DENSE_THREADS / 64];
    const auto im = G(images)[blockIdx.y];
    const int W = im.w, H = im.h, step = p.step, win = p.win, sx = p.search_x, sy = p.search_y;
    const int cstep = MIRROR ? 1 : step;                   // the lattice's column step
    const int cols = W / cstep, rows = H / step;
    const uint8_t* const src_l = MIRROR ? im.right : im.left;
    const uint8_t* const src_r = MIRROR ? im.left : im.right;
    const int stride_l = MIRROR ? im.right_stride : im.left_stride, stride_r = MIRROR ? im.left_stride : im.right_stride;
    const int wb = win / 2, wa = (win + 1) / 2;
    const int span = dense_span(win), band = dense_band(step, win, p.band);
    const int ntx = (W + span - 1) / span, nty = (rows + band - 1) / band;
    if ((int)blockIdx.x >= ntx * nty) return;              // (the grid is sized for the launch's largest image)
    const int tx = (int)blockIdx.x % ntx, ty = (int)blockIdx.x / ntx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X0 = tx * span - wb;                         // the left column of lane 0
    const int iy0 = ty * band, nrow = min(band, rows - iy0);
    const int yc0 = iy0 * step + step / 2;                 // the pixel row of the band's first lattice row
    const int yl0 = max(0, yc0 - wb);                      // the left row of LDS row 0

    // the band's planes, zero outside the images
    for (int i = tid; i < DENSE_L_ROWS * DENSE_THREADS; i += DENSE_THREADS) {
        const int yy = yl0 + i / DENSE_THREADS, xx = X0 + i % DENSE_THREADS;
        s_l[i] = (yy < H && xx >= 0 && xx < W) ? G(src_l)[(int64_t)yy * stride_l + (MIRROR ? W - 1 - xx : xx)] : (uint8_t)0;
    }
    for (int i = tid; i < DENSE_R_ROWS * DENSE_R_COLS; i += DENSE_THREADS) {
        const int yy = yl0 - sy + i / DENSE_R_COLS, xx = X0 + i % DENSE_R_COLS;
        s_r[i] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? G(src_r)[(int64_t)yy * stride_r + (MIRROR ? W - 1 - xx : xx)] : (uint8_t)0;
    }

    // this lane's lattice point, if it has one: column x of the tile's span
    const int x = X0 + tid, xl = x - cstep / 2;
    const bool in_span = tid >= wb && tid < wb + span && xl >= 0 && xl % cstep == 0 && xl / cstep < cols;
    const int ix = in_span ? xl / cstep : 0;
    const int x11 = max(0, x - wb), x12 = min(W - 1, x + wa), x22 = min(W - 1, x + wa + sx);
    const int tw = x12 - x11, mw = (x22 - x11) - tw + 1;
    const bool xok = !(x12 <= 0 || x11 >= W - 1 || x22 <= 0) && tw > 0 && mw > 0;
    const int pa = in_span ? min(max(x11 - X0, 0), DENSE_THREADS) : 0;   // the box is prefix[pb] - prefix[pa]
    const int pb = in_span ? min(max(x12 - X0, 0), DENSE_THREADS) : 0;

    // per lattice row of the band (the same for every lane): its template rows as LDS rows [row_lo, row_hi) and the
    // vertical offsets dy of its candidates k = 0 .. mh - 1, [dy_lo, dy_hi] (empty for an invalid row)
    int row_lo[DENSE_BAND], row_hi[DENSE_BAND], dy_lo[DENSE_BAND], dy_hi[DENSE_BAND];
#pragma unroll
    for (int r = 0; r < DENSE_BAND; r++) {
        const int y = yc0 + min(r, nrow - 1) * step;
        const int y11 = max(0, y - wb), y12 = min(H, y + wa);
        const int y21 = max(0, y - wb - sy), y22 = min(H - 1, y + wa + sy);
        const int th = y12 - y11, mh = (y22 - y21) - th + 1;
        const bool yok = r < nrow && !(y12 <= 0 || y11 >= H - 1 || y22 <= 0 || y21 >= H - 1) && th > 0 && mh > 0;
        row_lo[r] = y11 - yl0; row_hi[r] = y12 - yl0;
        dy_lo[r] = y21 - y11; dy_hi[r] = yok ? dy_lo[r] + mh - 1 : dy_lo[r] - 1;
    }

    float best[DENSE_BAND];
    int minx[DENSE_BAND], sum[DENSE_BAND], cnt[DENSE_BAND];
#pragma unroll
    for (int r = 0; r < DENSE_BAND; r++) { best[r] = 0.f; minx[r] = 0; sum[r] = 0; cnt[r] = 0; }
    __syncthreads();

    int buf = 0;
    for (int dy = -sy; dy <= sy; dy++) {
        for (int j = 0; j <= sx; j++) {
            const uint8_t* lp = s_l + tid;
            const uint8_t* rp = s_r + (dy + sy) * DENSE_R_COLS + tid + j;
            // 1. the column sums of the band's rows: C slides down the LDS rows [lo, hi)
            int Cr[DENSE_BAND];
            int C = 0, lo = 0, hi = 0;
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
#pragma unroll 8
                for (const int to = row_hi[r]; hi < to; hi++) {
                    const int d = (int)rp[hi * DENSE_R_COLS] - (int)lp[hi * DENSE_THREADS];
                    C += d * d;
                }
#pragma unroll 4
                for (const int to = row_lo[r]; lo < to; lo++) {
                    const int d = (int)rp[lo * DENSE_R_COLS] - (int)lp[lo * DENSE_THREADS];
                    C -= d * d;
                }
                Cr[r] = C;
            }
            // 2. inclusive prefixes over the wave's columns
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) Cr[r] = dense_wave_prefix(Cr[r]);
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
                s_p[buf][r][tid] = Cr[r];
                if (lane == 63) s_t[buf][r][wave] = Cr[r];
            }
            __syncthreads();
            // 3. the boxes and the running argmin (selects, no branch on the lane: the rows' state stays in registers)
            const bool act = in_span && xok && j < mw;
            const int ia = max(pa - 1, 0), ib = max(pb - 1, 0), wva = ia >> 6, wvb = ib >> 6;
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
                if (dy < dy_lo[r] || dy > dy_hi[r]) continue;   // (the same for every lane)
                const int t0 = s_t[buf][r][0], t1 = s_t[buf][r][1], t2 = s_t[buf][r][2];
                const int fa = pa > 0 ? s_p[buf][r][ia] + (wva > 0 ? t0 : 0) + (wva > 1 ? t1 : 0) + (wva > 2 ? t2 : 0) : 0;
                const int fb = pb > 0 ? s_p[buf][r][ib] + (wvb > 0 ? t0 : 0) + (wvb > 1 ? t1 : 0) + (wvb > 2 ? t2 : 0) : 0;
                const float val = (float)(fb - fa);
                const bool lower = act && (cnt[r] == 0 || val < best[r]);
                const bool tie = act && !lower && val == best[r] && j >= minx[r];
                best[r] = lower ? val : best[r];
                minx[r] = lower ? j : minx[r];
                sum[r] = lower ? j : sum[r] + (tie ? j : 0);
                cnt[r] = lower ? 1 : cnt[r] + (tie ? 1 : 0);
            }
            buf ^= 1;
        }
    }

    if (!in_span) return;
    SVO_GP(float) out = G(im.out);
    if (MIRROR) {                                          // the disparity alone, at the unmirrored column
#pragma unroll
        for (int r = 0; r < DENSE_BAND; r++) {
            if (r >= nrow) continue;
            const float d = (float)sum[r] / (float)cnt[r];
            out[(int64_t)(iy0 + r) * W + (W - 1 - ix)] = xok && cnt[r] > 0 ? (d < 0.5f ? 0.5f : d) : -1.f;
        }
        return;
    }
    const int64_t plane = (int64_t)cols * rows;
#pragma unroll
    for (int r = 0; r < DENSE_BAND; r++) {
        if (r >= nrow) continue;
        const bool valid = xok && cnt[r] > 0;
        float val = p.value == SVO_DENSE_DEPTH ? 0.f : -1.f;
        if (valid) {
            const float d = (float)sum[r] / (float)cnt[r];
            const float disp = d < 0.5f ? 0.5f : d;
            val = p.value == SVO_DENSE_DEPTH ? im.baseline / disp : disp;
        }
        const int64_t at = (int64_t)(iy0 + r) * cols + ix;
        out[at] = val;
        if (p.cost) out[plane + at] = valid ? best[r] : -1.f;
    }
}

// The cost volume of include/svo_hip.h ("sgm"): dense_disparity_kernel's tile, staging, sliding column sums and prefix,
// with the candidates walked j outer, dy inner, so that the state of a lattice row is one running minimum over dy (the
// exact int32 SSD, never a float). After the dy loop the point's lane divides by its area, caps and stores one uint16
// per row at [iy][ix][j]; after the last j it stores the count plane. Of an image exactly vol[0 .. rows * cols * D) and
// count[0 .. rows * cols) are written.
// MIRROR: the reverse volume of a checked SGM map (include/svo_hip.h, "sgm cross-check"). As in
// dense_disparity_kernel<true> the two staging loops read column W - 1 - xx of the other plane; unlike there the lattice
// keeps its column step, so cols, ix and every index after the staging are those of MIRROR = false, in the mirrored
// pair's own coordinates. MIRROR = false is the kernel as it was.
template <bool MIRROR>
__global__ __launch_bounds__(DENSE_THREADS) void dense_cost_volume_kernel(const CostImage* __restrict__ images, const DenseParams p,
                                                                          const int cost_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t s_l[DENSE_L_ROWS * DENSE_THREADS];
    __shared__ __attribute__((aligned(16))) uint8_t s_r[DENSE_R_ROWS * DENSE_R_COLS];
    __shared__ int s_p[2][DENSE_BAND][DENSE_THREADS];
    __shared__ int s_t[2][DENSE_BAND][DENSE_THREADS / 64];
    const auto im = G(images)[blockIdx.y];
    const int W = im.w, H = im.h, step = p.step, win = p.win, sx = p.search_x, sy = p.search_y;
    const int cols = W / step, rows = H / step, D = sx + 1;
    const int wb = win / 2, wa = (win + 1) / 2;
    const int span = dense_span(win), band = dense_band(step, win, p.band);
    const int ntx = (W + span - 1) / span, nty = (rows + band - 1) / band;
    if ((int)blockIdx.x >= ntx * nty) return;
    const int tx = (int)blockIdx.x % ntx, ty = (int)blockIdx.x / ntx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X0 = tx * span - wb;
    const int iy0 = ty * band, nrow = min(band, rows - iy0);
    const int yc0 = iy0 * step + step / 2;
    const int yl0 = max(0, yc0 - wb);

    const uint8_t* const src_l = MIRROR ? im.right : im.left;
    const uint8_t* const src_r = MIRROR ? im.left : im.right;
    const int stride_l = MIRROR ? im.right_stride : im.left_stride, stride_r = MIRROR ? im.left_stride : im.right_stride;
    for (int i = tid; i < DENSE_L_ROWS * DENSE_THREADS; i += DENSE_THREADS) {
        const int yy = yl0 + i / DENSE_THREADS, xx = X0 + i % DENSE_THREADS;
        s_l[i] = (yy < H && xx >= 0 && xx < W) ? G(src_l)[(int64_t)yy * stride_l + (MIRROR ? W - 1 - xx : xx)] : (uint8_t)0;
    }
    for (int i = tid; i < DENSE_R_ROWS * DENSE_R_COLS; i += DENSE_THREADS) {
        const int yy = yl0 - sy + i / DENSE_R_COLS, xx = X0 + i % DENSE_R_COLS;
        s_r[i] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? G(src_r)[(int64_t)yy * stride_r + (MIRROR ? W - 1 - xx : xx)] : (uint8_t)0;
    }

    const int x = X0 + tid, xl = x - step / 2;
    const bool in_span = tid >= wb && tid < wb + span && xl >= 0 && xl % step == 0 && xl / step < cols;
    const int ix = in_span ? xl / step : 0;
    const int x11 = max(0, x - wb), x12 = min(W - 1, x + wa), x22 = min(W - 1, x + wa + sx);
    const int tw = x12 - x11, mw = (x22 - x11) - tw + 1;
    const bool xok = !(x12 <= 0 || x11 >= W - 1 || x22 <= 0) && tw > 0 && mw > 0;
    const int pa = in_span ? min(max(x11 - X0, 0), DENSE_THREADS) : 0;
    const int pb = in_span ? min(max(x12 - X0, 0), DENSE_THREADS) : 0;

    int row_lo[DENSE_BAND], row_hi[DENSE_BAND], dy_lo[DENSE_BAND], dy_hi[DENSE_BAND];
#pragma unroll
    for (int r = 0; r < DENSE_BAND; r++) {
        const int y = yc0 + min(r, nrow - 1) * step;
        const int y11 = max(0, y - wb), y12 = min(H, y + wa);
        const int y21 = max(0, y - wb - sy), y22 = min(H - 1, y + wa + sy);
        const int th = y12 - y11, mh = (y22 - y21) - th + 1;
        const bool yok = r < nrow && !(y12 <= 0 || y11 >= H - 1 || y22 <= 0 || y21 >= H - 1) && th > 0 && mh > 0;
        row_lo[r] = y11 - yl0; row_hi[r] = y12 - yl0;
        dy_lo[r] = y21 - y11; dy_hi[r] = yok ? dy_lo[r] + mh - 1 : dy_lo[r] - 1;
    }
    __syncthreads();

    SVO_GP(uint16_t) vol = G(im.vol);
    const int ia = max(pa - 1, 0), ib = max(pb - 1, 0), wva = ia >> 6, wvb = ib >> 6;
    int buf = 0;
    for (int j = 0; j <= sx; j++) {
        int best[DENSE_BAND];
#pragma unroll
        for (int r = 0; r < DENSE_BAND; r++) best[r] = 0x7fffffff;
        for (int dy = -sy; dy <= sy; dy++) {
            const uint8_t* lp = s_l + tid;
            const uint8_t* rp = s_r + (dy + sy) * DENSE_R_COLS + tid + j;
            int Cr[DENSE_BAND];
            int C = 0, lo = 0, hi = 0;
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
#pragma unroll 8
                for (const int to = row_hi[r]; hi < to; hi++) {
                    const int d = (int)rp[hi * DENSE_R_COLS] - (int)lp[hi * DENSE_THREADS];
                    C += d * d;
                }
#pragma unroll 4
                for (const int to = row_lo[r]; lo < to; lo++) {
                    const int d = (int)rp[lo * DENSE_R_COLS] - (int)lp[lo * DENSE_THREADS];
                    C -= d * d;
                }
                Cr[r] = C;
            }
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) Cr[r] = dense_wave_prefix(Cr[r]);
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
                s_p[buf][r][tid] = Cr[r];
                if (lane == 63) s_t[buf][r][wave] = Cr[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
                if (dy < dy_lo[r] || dy > dy_hi[r]) continue;   // (the same for every lane)
                const int t0 = s_t[buf][r][0], t1 = s_t[buf][r][1], t2 = s_t[buf][r][2];
                const int fa = pa > 0 ? s_p[buf][r][ia] + (wva > 0 ? t0 : 0) + (wva > 1 ? t1 : 0) + (wva > 2 ? t2 : 0) : 0;
                const int fb = pb > 0 ? s_p[buf][r][ib] + (wvb > 0 ? t0 : 0) + (wvb > 1 ? t1 : 0) + (wvb > 2 ? t2 : 0) : 0;
                best[r] = min(best[r], fb - fa);
            }
            buf ^= 1;
        }
        if (in_span) {
#pragma unroll
            for (int r = 0; r < DENSE_BAND; r++) {
                if (r >= nrow) continue;
                const bool valid = xok && dy_hi[r] >= dy_lo[r];
                const int area = max(tw * (row_hi[r] - row_lo[r]), 1);
                const int c = valid ? (j < mw ? min(cost_cap, best[r] / area) : cost_cap) : 0;
                vol[((int64_t)(iy0 + r) * cols + ix) * D + j] = (uint16_t)c;
            }
        }
    }
    if (!in_span) return;
    SVO_GP(uint16_t) count = G(im.count);
#pragma unroll
    for (int r = 0; r < DENSE_BAND; r++) {
        if (r >= nrow) continue;
        count[(int64_t)(iy0 + r) * cols + ix] = (uint16_t)(xok && dy_hi[r] >= dy_lo[r] ? mw : 0);
    }
}

void launch_dense_cost_volume(const CostImage* d_images, int n, int tiles, const DenseParams& p, int cost_cap, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(dense_cost_volume_kernel<false>, dim3(tiles, n), dim3(DENSE_THREADS), 0, stream, d_images, p, cost_cap);
}

void launch_dense_cost_volume_mirrored(const CostImage* d_images, int n, int tiles, const DenseParams& p, int cost_cap, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(dense_cost_volume_kernel<true>, dim3(tiles, n), dim3(DENSE_THREADS), 0, stream, d_images, p, cost_cap);
}

void launch_dense(const DenseImage* d_images, int n, int tiles, const DenseParams& p, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(dense_disparity_kernel<false>, dim3(tiles, n), dim3(DENSE_THREADS), 0, stream, d_images, p);
}

void launch_dense_reverse(const LrImage* d_images, int n, int tiles, const DenseParams& p, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(dense_disparity_kernel<true>, dim3(tiles, n), dim3(DENSE_THREADS), 0, stream, d_images, p);
}

}  // namespace svo
