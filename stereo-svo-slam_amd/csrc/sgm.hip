// sgm.hip — semi-global aggregation over the cost volumes of a dense search (include/svo_hip.h, "sgm"): the four
// scanline paths through uint16 [rows][cols][D] volumes, their sum S and the value rule (first minimum of S over the
// point's candidates, parabola through its neighbours), many volumes in one launch.
//
// D <= 64, so a scanline is one wavefront with one candidate per lane: lane j holds P(j) = L_r(p - r, j), lanes >= D
// hold SGM_BIG, which never wins a minimum. Per point
//   * m = min_j P(j) is a DPP min reduction (the shifts and row broadcasts of dense_wave_prefix) and one readlane;
//   * P(j - 1) and P(j + 1) are wave_shr:1 and wave_shl:1 of the DPP network; the lane without a source keeps SGM_BIG;
//   * L = C + min(P, min(P(j - 1), P(j + 1)) + p1, m + p2) - m. All int32, all below 2^30.
// The chain from point to point is serial; the loads of C (and of S) for the next SGM_AHEAD points do not depend on it
// and are issued before the chain walks them.
//
// Two launches, ordered by the stream: ROWS (a wavefront per lattice row) walks its line forwards and stores L into S,
// then backwards and adds; COLUMNS (a wavefront per lattice column) walks down and adds, then up, and there S is
// complete in the lane's register: the argmin over the first `count` lanes is a min reduction of the key S << 6 | j
// (the lowest lane wins a tie), S(j0 - 1) and S(j0 + 1) come by readlane, and lane 0 writes the value and cost. Every
// entry of S belongs to one lane of one wavefront per launch, which reads it after it wrote it: no atomics. Integer
// sums commute, so the order of the paths cannot change a bit.
//
// Entries of a caller's volume above cost_cap are read as cost_cap, so S <= 4 * (cost_cap + p2) <= 65535 always fits
// its uint16.
//
// Bounds: a wavefront owns line `line` < lines of its image and touches vol / sum at (point * D + lane) for lane < D
// and point < cols * rows only; count and out at point < cols * rows (out + plane with cost; never for a reverse
// volume of a checked job, whose out is one plane). No LDS.
//
// A checked job (include/svo_hip.h, "sgm cross-check") puts the volumes of the mirrored pairs behind the forward ones
// in the same table, so the same two launches carry both: the kernel is latency bound with few images,
// and twice the entries of a launch cost less than a second pair of launches.
#include "svo_host.hpp"
#include "svo_tracker.hpp"

namespace svo {

constexpr int SGM_THREADS = 256, SGM_WAVES = SGM_THREADS / 64;
constexpr int SGM_AHEAD = 8;                               // points whose loads are in flight ahead of the chain
constexpr int SGM_BIG = 1 << 29;
static_assert(sizeof(svo_sgm_params) == 32 && sizeof(SgmImage) == 48 && sizeof(CostImage) == 48, "record sizes");

int sgm_check_params(const svo_sgm_params* s, const char* who, SgmParams* out) {
    if (!s) return svo_set_error(SVO_ERR_INVALID, "%s: no svo_sgm_params", who);
    if (s->paths != 4) return svo_set_error(SVO_ERR_INVALID, "%s: paths %d (4 supported; 8 is reserved)", who, s->paths);
    if (s->p1 < 1 || s->p2 < s->p1) return svo_set_error(SVO_ERR_INVALID, "%s: p1 %d, p2 %d: 1 <= p1 <= p2", who, s->p1, s->p2);
    if (s->cost_cap < 1 || s->p2 > 65535 || s->cost_cap > 65535 || 4 * ((int64_t)s->cost_cap + s->p2) > 65535)
        return svo_set_error(SVO_ERR_INVALID, "%s: cost_cap %d, p2 %d: cost_cap >= 1 and 4 * (cost_cap + p2) <= 65535", who, s->cost_cap, s->p2);
    if (s->subpixel != 0 && s->subpixel != 1) return svo_set_error(SVO_ERR_INVALID, "%s: subpixel %d", who, s->subpixel);
    if (s->_reserved[0] != 0 || s->_reserved[1] != 0 || s->_reserved[2] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    if (out) *out = SgmParams{s->p1, s->p2, s->cost_cap, s->subpixel, 0, 0, 0};
    return SVO_OK;
}

// the minimum over the 64 lanes of a wave, in every lane's scalar view: dense_wave_prefix with min in the place of +
// (a lane without a source keeps its own value), then lane 63
__device__ __forceinline__ int sgm_wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));   // row_bcast:15, rows 1 and 3
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));   // row_bcast:31, rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// L_r(p, .) from P = L_r(p - r, .) and the lane's C(p, j); a lane >= D (live false) stays at SGM_BIG
__device__ __forceinline__ int sgm_step(int P, int c, int p1, int p2, bool live) {
    const int m = sgm_wave_min(P);
    const int below = __builtin_amdgcn_update_dpp(SGM_BIG, P, 0x138, 0xf, 0xf, false);   // wave_shr:1: P(j - 1)
    const int above = __builtin_amdgcn_update_dpp(SGM_BIG, P, 0x130, 0xf, 0xf, false);   // wave_shl:1: P(j + 1)
    const int L = c + min(min(P, min(below, above) + p1), m + p2) - m;
    return live ? L : SGM_BIG;
}

// the value and cost of one point from its complete S (every lane its own), in every lane
__device__ __forceinline__ void sgm_value(int S, int lane, int count, const SgmParams& p, bool depth, float baseline, float* value, float* cost) {
    const int key = sgm_wave_min(lane < count ? (S << 6 | lane) : 0x7fffffff);
    *value = depth ? 0.f : -1.f;
    *cost = -1.f;
    if (count <= 0) return;                                // (the same for every lane)
    const int j0 = key & 63, b = key >> 6;
    float d = (float)j0;
    if (p.subpixel && j0 > 0 && j0 < count - 1) {
        const int a = __builtin_amdgcn_readlane(S, j0 - 1), c = __builtin_amdgcn_readlane(S, j0 + 1);
        d = d + (float)(a - c) / (float)(2 * (a - 2 * b + c));
    }
    const float disp = d < 0.5f ? 0.5f : d;
    *value = depth ? baseline / disp : disp;
    *cost = (float)b;
}

// COLUMNS false: a wavefront per lattice row, S = L(+1, 0) + L(-1, 0) is stored. COLUMNS true: a wavefront per
// lattice column, L(0, +1) is added to S in memory, L(0, -1) in the register, and the value rule follows.
template <bool COLUMNS>
__global__ __launch_bounds__(SGM_THREADS) void sgm_paths_kernel(const SgmImage* __restrict__ images, const SgmParams p) {
    const auto im = G(images)[blockIdx.y];
    const int lane = threadIdx.x & 63, line = (int)blockIdx.x * SGM_WAVES + ((int)threadIdx.x >> 6);
    const int lines = COLUMNS ? im.cols : im.rows, len = COLUMNS ? im.rows : im.cols;
    if (line >= lines) return;                             // (whole wavefronts; there is no barrier below)
    const int D = im.D, p1 = p.p1, p2 = p.p2, cap = p.cost_cap;
    const bool live = lane < D;
    const int64_t first = COLUMNS ? line : (int64_t)line * im.cols;   // the line's first point, and the points between two of its points
    const int64_t pitch = COLUMNS ? im.cols : 1;
    SVO_GP(const uint16_t) vol = G(im.vol);
    SVO_GP(uint16_t) sum = G(im.sum);
    const int lj = live ? lane : 0;

    // forwards
    int P = SGM_BIG;
    for (int i0 = 0; i0 < len; i0 += SGM_AHEAD) {
        int c[SGM_AHEAD], s[SGM_AHEAD];
#pragma unroll
        for (int k = 0; k < SGM_AHEAD; k++) {
            const int64_t at = (first + (int64_t)min(i0 + k, len - 1) * pitch) * D + lj;
            c[k] = min((int)vol[at], cap);
            s[k] = COLUMNS ? (int)sum[at] : 0;
        }
#pragma unroll
        for (int k = 0; k < SGM_AHEAD; k++) {
            if (i0 + k >= len) break;
            P = i0 + k == 0 ? (live ? c[k] : SGM_BIG) : sgm_step(P, c[k], p1, p2, live);
            if (live) sum[(first + (int64_t)(i0 + k) * pitch) * D + lane] = (uint16_t)(s[k] + P);
        }
    }

    // backwards
    SVO_GP(const uint16_t) count = G(im.count);
    SVO_GP(float) out = G(im.out);
    const int64_t plane = (int64_t)im.cols * im.rows;
    // (a reverse volume of a checked job, the same for the whole workgroup: its disparity alone)
    const bool reverse = p.reverse_from > 0 && (int)blockIdx.y >= p.reverse_from;
    const bool depth = !reverse && p.value == SVO_DENSE_DEPTH, with_cost = !reverse && p.cost;
    P = SGM_BIG;
    for (int i0 = len - 1; i0 >= 0; i0 -= SGM_AHEAD) {
        int c[SGM_AHEAD], s[SGM_AHEAD], n[SGM_AHEAD];
#pragma unroll
        for (int k = 0; k < SGM_AHEAD; k++) {
            const int64_t pt = first + (int64_t)max(i0 - k, 0) * pitch;
            c[k] = min((int)vol[pt * D + lj], cap);
            s[k] = (int)sum[pt * D + lj];
            n[k] = COLUMNS ? (count ? (int)count[pt] : D) : 0;
        }
#pragma unroll
        for (int k = 0; k < SGM_AHEAD; k++) {
            if (i0 - k < 0) break;
            const int64_t pt = first + (int64_t)(i0 - k) * pitch;
            P = i0 - k == len - 1 ? (live ? c[k] : SGM_BIG) : sgm_step(P, c[k], p1, p2, live);
            if (!COLUMNS) {
                if (live) sum[pt * D + lane] = (uint16_t)(s[k] + P);
            } else {
                float value, cost;
                sgm_value(live ? s[k] + P : 0, lane, min(n[k], D), p, depth, im.baseline, &value, &cost);
                if (lane == 0) {
                    out[pt] = value;
                    if (with_cost) out[plane + pt] = cost;
                }
            }
        }
    }
}

void launch_sgm(const SgmImage* d_images, int n, int max_cols, int max_rows, const SgmParams& p, hipStream_t stream) {
    if (n <= 0 || max_cols <= 0 || max_rows <= 0) return;
    hipLaunchKernelGGL(sgm_paths_kernel<false>, dim3((max_rows + SGM_WAVES - 1) / SGM_WAVES, n), dim3(SGM_THREADS), 0, stream, d_images, p);
    hipLaunchKernelGGL(sgm_paths_kernel<true>, dim3((max_cols + SGM_WAVES - 1) / SGM_WAVES, n), dim3(SGM_THREADS), 0, stream, d_images, p);
}

}  // namespace svo
