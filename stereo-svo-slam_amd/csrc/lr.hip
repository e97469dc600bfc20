// lr.hip — the left-right cross-check of a dense disparity search (include/svo_hip.h, "cross-check"). The forward
// search (dense_disparity_kernel<false>, dense.hip) has written a disparity per lattice point, the reverse search
// (dense_disparity_kernel<true>) a disparity per column of every lattice row, indexed by the right image's column.
// lr_check_kernel streams over the lattice: per point it reads its forward disparity, gathers the reverse disparity
// at xr = x + (int)(disp + 0.5f) of its row, writes lr (-1: invalid forward, -2: xr outside or the reverse search
// invalid, else |disp - rd|), and writes the value plane in place: the invalid value where the point fails at
// max_lr_diff > 0, else the disparity, or baseline / disparity for SVO_DENSE_DEPTH (the division of the unchecked
// kernel, so the same bits).
//
// A workgroup of 256 lanes takes LR_TILE = 1024 consecutive lattice points of one image (blockIdx.y: its table entry,
// as in dense.hip), a lane four consecutive ones: four loads in flight, then four gathers. A lane reads and writes
// only its own points of the value plane, so the plane is converted in place; the reverse plane is only read. About
// 8 B in and 4 to 8 B out per lattice point; no LDS, no atomics; the roof is HBM.
//
// LATTICE: the check of an SGM map (include/svo_hip.h, "sgm cross-check"). The reverse plane is the SGM disparity of
// the mirrored pair over its own lattice, cols x rows floats, and the point gathers the cell that holds its matched
// column: ixm = min((W - 1 - xr) / step, cols - 1). Nothing else differs.
//
// Bounds: of an image, floats [0, cols * rows) of value and lr are read / written (k < total), and floats
// [iy * w + xr] of the reverse plane with iy < rows, x <= xr <= w - 1 (xr > w - 1 is tested before the read).
// LATTICE: floats [iy * cols + ixm] with iy < rows and, as 0 <= W - 1 - xr under the same test, 0 <= ixm <= cols - 1
// by the clamp (which bites only where W % step >= 2 + step / 2 leaves columns beyond the last cell).
#include <cmath>

#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

constexpr int LR_THREADS = 256;
constexpr int LR_POINTS = LR_TILE / LR_THREADS;
static_assert(sizeof(svo_stereo_check) == 32 && sizeof(LrImage) == 64, "record sizes");

int lr_check_parse(const svo_stereo_check* s, bool cloud, const char* who, LrCheck* out) {
    if (out) *out = LrCheck{};
    if (!s) return SVO_OK;
    if (s->lr != 0 && s->lr != 1) return svo_set_error(SVO_ERR_INVALID, "%s: check: lr %d", who, s->lr);
    if (!(s->max_lr_diff >= 0.f) || !(s->max_lr_diff <= FLT_MAX))
        return svo_set_error(SVO_ERR_INVALID, "%s: check: max_lr_diff is negative or not finite", who);
    for (const int32_t r : s->_reserved)
        if (r != 0) return svo_set_error(SVO_ERR_INVALID, "%s: check: a _reserved is not 0", who);
    if (cloud && s->lr == 1 && s->max_lr_diff == 0.f)
        return svo_set_error(SVO_ERR_INVALID, "%s: check: a cloud needs max_lr_diff > 0", who);
    if (out) *out = LrCheck{s->lr, s->max_lr_diff};
    return SVO_OK;
}

template <bool LATTICE>
__global__ __launch_bounds__(LR_THREADS) void lr_check_kernel(const LrImage* __restrict__ images, const LrParams p) {
    const LrImage im = G(images)[blockIdx.y];
    const int W = im.w, cols = W / p.step, total = cols * (im.h / p.step);
    const int k0 = ((int)blockIdx.x * LR_THREADS + (int)threadIdx.x) * LR_POINTS;
    if (k0 >= total) return;                               // (the grid is sized for the launch's largest image)
    SVO_GP(float) value = G(im.value);
    SVO_GP(const float) rev = G((const float*)im.out);
    float disp[LR_POINTS], rd[LR_POINTS];
    int xr[LR_POINTS];
#pragma unroll
    for (int q = 0; q < LR_POINTS; q++) disp[q] = k0 + q < total ? value[k0 + q] : -1.f;
#pragma unroll
    for (int q = 0; q < LR_POINTS; q++) {
        const int k = k0 + q, iy = k / cols, ix = k - iy * cols;
        const int x = ix * p.step + p.step / 2;
        xr[q] = x + (int)(disp[q] + 0.5f);
        const int64_t at = LATTICE ? (int64_t)iy * cols + min((W - 1 - xr[q]) / p.step, cols - 1) : (int64_t)iy * W + xr[q];
        rd[q] = (disp[q] >= 0.f && xr[q] <= W - 1) ? rev[at] : -1.f;
    }
    const float inv = p.value == SVO_DENSE_DEPTH ? 0.f : -1.f;
#pragma unroll
    for (int q = 0; q < LR_POINTS; q++) {
        if (k0 + q >= total) continue;
        const bool valid = disp[q] >= 0.f;                 // (-1: invalid; a valid disparity is >= 0.5)
        const float lr = !valid ? -1.f : (xr[q] > W - 1 || rd[q] < 0.f) ? -2.f : fabsf(disp[q] - rd[q]);
        const bool fails = p.max_lr_diff > 0.f && (lr < 0.f || lr > p.max_lr_diff);
        if (im.lr) G(im.lr)[k0 + q] = lr;
        if (!valid || fails) value[k0 + q] = inv;
        else if (p.value == SVO_DENSE_DEPTH) value[k0 + q] = im.baseline / disp[q];
    }
}

void launch_lr_check(const LrImage* d_images, int n, int tiles, const LrParams& p, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(lr_check_kernel<false>, dim3(tiles, n), dim3(LR_THREADS), 0, stream, d_images, p);
}

void launch_lr_check_lattice(const LrImage* d_images, int n, int tiles, const LrParams& p, hipStream_t stream) {
    if (n <= 0 || tiles <= 0) return;
    hipLaunchKernelGGL(lr_check_kernel<true>, dim3(tiles, n), dim3(LR_THREADS), 0, stream, d_images, p);
}

}  // namespace svo
