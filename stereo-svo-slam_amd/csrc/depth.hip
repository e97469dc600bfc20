// depth.hip — rows C1, C2, D1, D3 of SURVEY §8a: the stereo depth filter
// DepthFilter::update_depth (src/lib/depth_filter.cpp:40-50).
//
//  * ssd_disparity_kernel (C1): calculate_disparities (depth_filter.cpp:259-327)
//    and the identical loop of DepthCalculator::calculate_depth
//    (depth_calculator.cpp:200-240). One wavefront per keypoint; template and
//    search region live in LDS; exact int32 SSD (cv::matchTemplate TM_SQDIFF),
//    first minimum of the float map in row-major order (cv::minMaxLoc) and
//    the tie-averaged column of :313-323.
//  * filter_update_kernel (C2, D1, D3): outlier_check (:52-128),
//    update_kps3d (:130-257), the flag/write-back loop of
//    StereoSlam::new_image (src/lib/stereo_slam.cpp:205-229) and the counter
//    of KeyFrameManager::keyframe_needed (keyframe_manager.cpp:47-74).
#include "ssd_common.hpp"

namespace svo {

constexpr int SSD_P_STRIDE = 100;               // ints per row of the column-sum prefixes: >= region width + 1, and = 4 mod 16, so
                                                // the rows 4 * (lane >> 4) of a gather start 16 banks apart

// what a barrier is to a workgroup of one wavefront: LDS operations of a wave complete in program order, so the
// compiler keeping that order is all there is to do
__device__ __forceinline__ void ssd_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive prefix sum over the 64 lanes: four shifts inside the 16-lane rows, then row_bcast:15 / row_bcast:31
// carry a row's last lane into the rows after it (wave_sum_bcast_i, svo_device.hpp)
__device__ __forceinline__ int ssd_wave_scan_i(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1 (a lane without a source adds 0)
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2 and 3
    return v;
}

// The cross term of NMB x NJB blocks of the match map: per template row one Toeplitz B fragment (5 dwords +
// v_alignbyte), then per block one ds_read_b128 A fragment and one v_mfma_i32_16x16x64_i8. The block counts are
// template parameters so that a row's reads stand in one basic block, ahead of its matrix instructions.
template <int R_ROWS, int N_MB, int N_JB, int NMB, int NJB>
__device__ __forceinline__ void ssd_cross(const uint8_t* s_t, const uint8_t* s_r, int th, int lane, ssd_v4i (&acc)[N_MB][N_JB]) {
    const int fm = lane & 15, fh = lane >> 4;        // fragment row / column and 16-byte k slice
    // B: bytes [16 + 16 fh - fm, +16) of the padded template row
    const int o = 16 + 16 * fh - fm;
    const uint32_t* tb = reinterpret_cast<const uint32_t*>(s_t) + (o >> 2);
    const unsigned sh = (unsigned)(o & 3);
    const uint8_t* ab = s_r + 16 * fh;
    // the operands of a template row: five dwords of the template and a 16-byte piece of the region per block
    struct Row { uint32_t t[5]; ssd_v4i af[NMB][NJB]; };
    auto read_row = [&](int r, Row& w) {
        const uint32_t* t = tb + r * (SSD_T_STRIDE / 4);
#pragma unroll
        for (int d = 0; d < 5; d++) w.t[d] = t[d];
#pragma unroll
        for (int mb = 0; mb < NMB; mb++)
#pragma unroll
            for (int jb = 0; jb < NJB; jb++)
                w.af[mb][jb] = *reinterpret_cast<const ssd_v4i*>(ab + 16 * jb + min(16 * mb + fm + r, R_ROWS - 1) * SSD_R_STRIDE);
    };
    auto use_row = [&](const Row& w) {
        ssd_v4i bf;
        bf.x = (int)__builtin_amdgcn_alignbyte(w.t[1], w.t[0], sh);
        bf.y = (int)__builtin_amdgcn_alignbyte(w.t[2], w.t[1], sh);
        bf.z = (int)__builtin_amdgcn_alignbyte(w.t[3], w.t[2], sh);
        bf.w = (int)__builtin_amdgcn_alignbyte(w.t[4], w.t[3], sh);
#pragma unroll
        for (int mb = 0; mb < NMB; mb++)
#pragma unroll
            for (int jb = 0; jb < NJB; jb++)
                acc[mb][jb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w.af[mb][jb], bf, acc[mb][jb], 0, 0, 0);
    };
    if constexpr (NMB * NJB <= 5) {
        // one wave has nobody to hide its LDS round trip behind: two rows per trip, all their reads issued first.
        // Template row th is staged as zeros (th <= SSD_MAX_WIN, and s_t has one row more), so an odd th adds 0.
        for (int r = 0; r < th; r += 2) {
            Row r0, r1;
            read_row(r, r0);
            read_row(r + 1, r1);
            use_row(r0);
            use_row(r1);
        }
    } else {
        for (int r = 0; r < th; r++) {     // (ten blocks: two rows' operands do not fit 128 registers)
            Row cur;
            read_row(r, cur);
            use_row(cur);
        }
    }
}
template <int R_ROWS, int N_MB, int N_JB, int NMB>
__device__ __forceinline__ void ssd_cross_jb(const uint8_t* s_t, const uint8_t* s_r, int th, int lane, int n_jb,
                                             ssd_v4i (&acc)[N_MB][N_JB]) {
    static_assert(N_JB == 5, "one case per column block count");
    switch (n_jb) {
        case 1: ssd_cross<R_ROWS, N_MB, N_JB, NMB, 1>(s_t, s_r, th, lane, acc); break;
        case 2: ssd_cross<R_ROWS, N_MB, N_JB, NMB, 2>(s_t, s_r, th, lane, acc); break;
        case 3: ssd_cross<R_ROWS, N_MB, N_JB, NMB, 3>(s_t, s_r, th, lane, acc); break;
        case 4: ssd_cross<R_ROWS, N_MB, N_JB, NMB, 4>(s_t, s_r, th, lane, acc); break;
        default: ssd_cross<R_ROWS, N_MB, N_JB, NMB, 5>(s_t, s_r, th, lane, acc); break;
    }
}

// C1. One wavefront per keypoint (single-wave workgroups: a keypoint starts as soon as one wave slot and 9.4 KB of
// LDS are free anywhere, where the four-wave workgroup this replaced waited for four slots and 15 KB on one CU).
// cv::matchTemplate(TM_SQDIFF) is
//   SSD[k][j] = sum_w R^2 - 2 sum_w R*T + sum T^2   over the window w at offset (k, j),
// exact in integers, and it is invariant to subtracting 128 from every pixel, so both images
// are staged as signed bytes (x ^ 0x80).
//  * The cross term is a correlation: 0.76 M multiply-adds per keypoint at the C2 settings,
//    the one place of this path with GEMM-class arithmetic. It runs on the matrix cores as a
//    Toeplitz product, one v_mfma_i32_16x16x64_i8 per template row r and 16-column block j0:
//        D[k][n] += sum_x A[k][x] * B[x][n],  A[k][x] = R[k + r][j0 + x]  (aligned 16 B / lane),
//                                             B[x][n] = T[r][x - n]       (0 outside the row),
//    so D[k][n] accumulates sum_{r,c} R[k+r][j0+n+c] T[r][c] over the th rows. Rows k >= mh and
//    columns j >= mw of D are computed and dropped. B depends on the template row and the lane only: it is built
//    once per row (zero-padded template, 5 dwords + v_alignbyte) and serves every block of the map, whose
//    accumulators all stay in registers. Any k-order inside the instruction is fine as long as A and B agree:
//    lane l holds bytes 16*(l>>4) .. +15 of its row / column for both operands.
//  * sum_w R^2: a lane owns region columns lane and lane + 64 and keeps their sliding column sums W[k][x] =
//    sum_{r<th} R[k+r][x]^2 of all map rows in registers. Once the matrix loop is done with the region tile, the
//    prefix sums of W along x (a wave scan) take its place, and a window sum is P[k][j + tw] - P[k][j], gathered
//    in the accumulators' layout. The match map itself is never stored.
//  * argmin: cv::minMaxLoc runs on matchTemplate's CV_32F result, so it is the first minimum in row-major
//    order of the map ROUNDED TO FLOAT (two integers above 2^24 that round to one float tie, and the earlier
//    wins); the key is (bits of (float)SSD, index). Then the tie-averaged column of :313-323.
// SSD_MAX_WIN / SSD_MAX_MH: what the LDS is sized for. The window kernels of a step share each CU's 160 KB with
// the alignment kernel's 38 KB per wavefront, and what fits is what runs: the shape for windows up to 31 and
// search_y up to 6 (every configuration of the reference) takes 9.4 KB, the other 11.0.
template <int SSD_MAX_WIN, int SSD_MAX_MH>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void ssd_disparity_kernel(const SsdArgs* __restrict__ args) {
    constexpr int SSD_R_ROWS = SSD_MAX_WIN + SSD_MAX_MH, SSD_T_ROWS = SSD_MAX_WIN + 1;
    constexpr int N_MB = (SSD_MAX_MH + 15) / 16, N_JB = (SSD_MAX_MW + 15) / 16;
    const SsdArgs& a = args[blockIdx.y];
    if (a.enable && !*G(a.enable)) return;
    const int n = *G(a.n_ptr);
    const int kp = a.first + (a.first_ptr ? *G(a.first_ptr) : 0) + (int)blockIdx.x;
    if (kp >= n) return;
    const int lane = threadIdx.x;

    __shared__ __attribute__((aligned(16))) uint8_t s_t[SSD_T_ROWS * SSD_T_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t s_r[SSD_R_ROWS * SSD_R_STRIDE];

    const int window_before = a.win / 2, window_after = (a.win + 1) / 2;
    const int cols = a.left.w, rows = a.left.h;
    const svo_kp2d p = G(a.kps2d)[kp];
    const int x = (int)p.x, y = (int)p.y;
    const int x11 = max(0, x - window_before);
    const int x12 = min(cols - 1, x + window_after);
    const int y11 = max(0, y - window_before);
    const int y12 = min(rows, y + window_after);
    const int x21 = x11;
    const int x22 = min(cols - 1, x + window_after + a.search_x);
    const int y21 = max(0, y - window_before - a.search_y);
    const int y22 = min(rows - 1, y + window_after + a.search_y);
    const int tw = x12 - x11, th = y12 - y11, rw = x22 - x21, rh = y22 - y21;
    const int mw = rw - tw + 1, mh = rh - th + 1;
    bool skip = false;
    if (a.clamp_half && (x12 <= 0 || y12 <= 0 || x11 >= cols - 1 || y11 >= rows - 1)) skip = true;
    if (a.clamp_half && (x22 <= 0 || y22 <= 0 || x21 >= cols - 1 || y21 >= rows - 1)) skip = true;
    if (tw <= 0 || th <= 0 || mw <= 0 || mh <= 0) skip = true;
    if (tw > SSD_MAX_WIN || th > SSD_MAX_WIN || mw > SSD_MAX_MW || mh > SSD_MAX_MH || rw >= SSD_P_STRIDE ||
        rh > SSD_R_ROWS)
        skip = true;  // the host validates window sizes; never taken with valid settings
    if (skip) {
        if (lane == 0) G(a.disparity)[kp] = -1.0f;
        return;
    }

    // ---- stage: template rows as [16 zero bytes | row ^ 0x80 | zeros], search region ^ 0x80 (bytes past
    // the region's width: 0x80), 16 bytes per lane and chunk: a template row is three chunks, a region row
    // up to six. A lane has 3 + 7 chunks (4 + 8 in the large shape): the 16-byte loads of all of them are issued
    // first, then the dword and byte loads of chunks that cross the image's right edge, and only then is anything
    // used.
    static_assert(SSD_T_STRIDE % 16 == 0 && SSD_R_STRIDE % 16 == 0, "rows are whole 16-byte chunks");
    {
        constexpr int T_CH = SSD_T_STRIDE / 16, R_CH = SSD_R_STRIDE / 16;
        constexpr int NT = SSD_T_ROWS * T_CH, NR = SSD_R_ROWS * R_CH, T_TRIPS = (NT + 63) / 64, R_TRIPS = (NR + 63) / 64;
        uint4 tv[T_TRIPS], rv[R_TRIPS];
        const int lw = a.left.w, rwid = a.right.w;
#pragma unroll
        for (int t = 0; t < T_TRIPS; t++) {
            const int i = lane + 64 * t, r = i / T_CH, c = 16 * (i % T_CH - 1);    // c: template column of the chunk's first byte
            tv[t] = make_uint4(0, 0, 0, 0);
            if (r < th && c >= 0 && c < tw && x11 + c + 16 <= lw) tv[t] = load_u8x16_whole(a.left, y11 + r, x11 + c);
        }
#pragma unroll
        for (int t = 0; t < R_TRIPS; t++) {
            const int i = lane + 64 * t, r = i / R_CH, c = 16 * (i % R_CH);
            rv[t] = make_uint4(0, 0, 0, 0);
            if (r < rh && c < rw && x21 + c + 16 <= rwid) rv[t] = load_u8x16_whole(a.right, y21 + r, x21 + c);
        }
#pragma unroll
        for (int t = 0; t < T_TRIPS; t++) {
            const int i = lane + 64 * t, r = i / T_CH, c = 16 * (i % T_CH - 1);
            if (r < th && c >= 0 && c < tw && x11 + c + 16 > lw) tv[t] = load_u8x16_edge(a.left, y11 + r, x11 + c);
        }
#pragma unroll
        for (int t = 0; t < R_TRIPS; t++) {
            const int i = lane + 64 * t, r = i / R_CH, c = 16 * (i % R_CH);
            if (r < rh && c < rw && x21 + c + 16 > rwid) rv[t] = load_u8x16_edge(a.right, y21 + r, x21 + c);
        }
#pragma unroll
        for (int t = 0; t < T_TRIPS; t++) {
            const int i = lane + 64 * t, r = i / T_CH, c = 16 * (i % T_CH - 1);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r < th && c >= 0 && c < tw) v = finish_u8x16(tv[t], tw - c, 0x80808080u, 0u);
            if (NT % 64 == 0 || i < NT) reinterpret_cast<uint4*>(s_t)[i] = v;
        }
#pragma unroll
        for (int t = 0; t < R_TRIPS; t++) {
            const int i = lane + 64 * t, r = i / R_CH, c = 16 * (i % R_CH);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r < rh && c < rw) v = finish_u8x16(rv[t], rw - c, 0x80808080u, 0x80808080u);
            if (NR % 64 == 0 || i < NR) reinterpret_cast<uint4*>(s_r)[i] = v;
        }
    }
    ssd_wave_sync();

    // ---- sum T^2: a lane per template row
    int stt = 0;
    if (lane < th) {
        const uint32_t* trow = reinterpret_cast<const uint32_t*>(s_t + lane * SSD_T_STRIDE) + 4;
#pragma unroll
        for (int d = 0; d < 9; d++) stt = __builtin_amdgcn_sdot4((int)trow[d], (int)trow[d], stt, false);
    }
    stt = wave_sum_dpp_i(stt);

    // ---- cross term on the matrix cores: every block of the match map in this wave
    const int n_jb = (mw + 15) >> 4;
    const int fm = lane & 15, fh = lane >> 4;
    ssd_v4i acc[N_MB][N_JB];
#pragma unroll
    for (int mb = 0; mb < N_MB; mb++)
#pragma unroll
        for (int jb = 0; jb < N_JB; jb++) acc[mb][jb] = ssd_v4i{0, 0, 0, 0};
    static_assert(N_MB <= 2, "two row blocks of 16 at most");
    if (N_MB == 2 && mh > 16) ssd_cross_jb<SSD_R_ROWS, N_MB, N_JB, N_MB>(s_t, s_r, th, lane, n_jb, acc);
    else ssd_cross_jb<SSD_R_ROWS, N_MB, N_JB, 1>(s_t, s_r, th, lane, n_jb, acc);
    // ---- column sums W[k][x] = sum_{r<th} R[k+r][x]^2 of region columns lane and lane + 64 (both inside the tile's
    // 144 bytes; what columns >= rw give is never used), the reads of a sweep issued together: eight rows of the
    // first window at a time, then the rows entering and leaving for all other map rows at once. Rows up to
    // SSD_R_ROWS - 2 are read, all staged.
    int w0[SSD_MAX_MH], w1[SSD_MAX_MH];
    {
        const int8_t* col = reinterpret_cast<const int8_t*>(s_r) + lane;
        int sq0 = 0, sq1 = 0;
        for (int r0 = 0; r0 < th; r0 += 8) {
            int v0[8], v1[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int rr = min(r0 + i, SSD_R_ROWS - 1);
                v0[i] = col[rr * SSD_R_STRIDE];
                v1[i] = col[rr * SSD_R_STRIDE + 64];
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const bool in = r0 + i < th;
                sq0 += in ? __mul24(v0[i], v0[i]) : 0;
                sq1 += in ? __mul24(v1[i], v1[i]) : 0;
            }
        }
        w0[0] = sq0; w1[0] = sq1;
        const int8_t* coln = col + (th - 1) * SSD_R_STRIDE;
        int n0[SSD_MAX_MH], n1[SSD_MAX_MH], o0[SSD_MAX_MH], o1[SSD_MAX_MH];
#pragma unroll
        for (int k = 1; k < SSD_MAX_MH; k++) {
            n0[k] = coln[k * SSD_R_STRIDE]; n1[k] = coln[k * SSD_R_STRIDE + 64];
            o0[k] = col[(k - 1) * SSD_R_STRIDE]; o1[k] = col[(k - 1) * SSD_R_STRIDE + 64];
        }
#pragma unroll
        for (int k = 1; k < SSD_MAX_MH; k++) {
            sq0 += __mul24(n0[k], n0[k]) - __mul24(o0[k], o0[k]);
            sq1 += __mul24(n1[k], n1[k]) - __mul24(o1[k], o1[k]);
            w0[k] = sq0; w1[k] = sq1;
        }
    }
    ssd_wave_sync();

    // ---- prefix sums of W along the columns take the place of the region tile, which nobody reads any more:
    // P[k][0] = 0, P[k][x + 1] = W[k][0] + .. + W[k][x] for x < rw
    static_assert(sizeof(int) * SSD_MAX_MH * SSD_P_STRIDE <= SSD_R_ROWS * SSD_R_STRIDE, "the prefix rows must fit the region tile");
    static_assert(SSD_MAX_WIN + SSD_MAX_MW <= SSD_P_STRIDE && SSD_P_STRIDE <= 128 + 1, "a row holds rw + 1 prefixes of two columns per lane");
    int* const s_p = reinterpret_cast<int*>(s_r);
#pragma unroll
    for (int k = 0; k < SSD_MAX_MH; k++) {
        if (k < mh) {
            const int p0 = ssd_wave_scan_i(w0[k]);
            const int p1 = ssd_wave_scan_i(w1[k]) + __builtin_amdgcn_readlane(p0, 63);
            if (lane == 0) s_p[k * SSD_P_STRIDE] = 0;
            if (lane < rw) s_p[k * SSD_P_STRIDE + lane + 1] = p0;
            if (lane + 64 < rw) s_p[k * SSD_P_STRIDE + lane + 65] = p1;
        }
    }
    ssd_wave_sync();

    // ---- the map in the accumulators' layout (C/D: col = lane & 15, row = 4 (lane >> 4) + reg) and its argmin.
    // first minimum of the FLOAT map in row-major order == smallest (float bits, index) key: an SSD is not
    // negative, and non-negative floats order like their bit patterns. Above 2^24 different integers round to
    // one float, and cv::minMaxLoc sees the floats: the earlier position wins, not the smaller integer.
    // An accumulator register then holds the float's bits for the tie pass.
    unsigned long long best = ~0ull;
#pragma unroll
    for (int mb = 0; mb < N_MB; mb++)
#pragma unroll
        for (int jb = 0; jb < N_JB; jb++) {
            if (jb < n_jb && 16 * mb < mh) {
                const int j = 16 * jb + fm, jc = min(j, mw - 1);     // (clamped: a dropped entry reads inside the rows too)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int k = 16 * mb + 4 * fh + i, kc = min(k, SSD_MAX_MH - 1);
                    const int* prow = &s_p[kc * SSD_P_STRIDE + jc];
                    const int ssd = prow[tw] - prow[0] + stt - 2 * acc[mb][jb][i];
                    const float f = (float)ssd;
                    acc[mb][jb][i] = (int)__float_as_uint(f);
                    if (k < mh && j < mw) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(f) << 32) | (unsigned)(k * mw + j);
                        best = key < best ? key : best;
                    }
                }
            }
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    // (every lane holds the same key now: taken as wave-uniform values)
    const int min_o = __builtin_amdgcn_readfirstlane((int)(best & 0xffffffffu));
    const int minx = min_o % mw, miny = min_o / mw;
    const float minVal = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)(best >> 32)));

    int sumj = 0, cnt = 0;
#pragma unroll
    for (int mb = 0; mb < N_MB; mb++)
#pragma unroll
        for (int jb = 0; jb < N_JB; jb++) {
            const int j = 16 * jb + fm;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = 16 * mb + 4 * fh + i;
                // (a block that was not computed has j >= mw or k >= mh)
                if (k < mh && j < mw && j >= minx && k >= miny && (double)__uint_as_float((unsigned)acc[mb][jb][i]) <= (double)minVal) { sumj += j; cnt++; }
            }
        }
    sumj = wave_sum_dpp_i(sumj);
    cnt = wave_sum_dpp_i(cnt);
    if (lane == 0) {
        float minPos = (float)sumj;    // sum of small ints: exact in float in any order
        minPos = minPos / cnt;
        G(a.disparity)[kp] = a.clamp_half ? fmaxf(0.5f, minPos) : minPos;
    }
}

int ssd_pick_max_win(int win, int search_y) { return win <= 31 && 2 * search_y + 1 <= 13 ? 31 : SSD_WIN_ALL; }

void launch_ssd(const SsdArgs* d_args, int batch, int max_n, int win, int search_y, hipStream_t stream) {
    if (max_n <= 0) return;
#ifdef SVO_SSD_FOUR_WAVES     // diagnostic builds (tools/build_variants.sh): the replaced kernel on the product path, for A/B runs
    launch_ssd_ref(d_args, batch, max_n, win, search_y, stream);
    return;
#endif
    if (ssd_pick_max_win(win, search_y) == 31)
        hipLaunchKernelGGL((ssd_disparity_kernel<31, 13>), dim3(max_n, batch), dim3(64), 0, stream, d_args);
    else
        hipLaunchKernelGGL((ssd_disparity_kernel<SSD_WIN_ALL, SSD_MH_ALL>), dim3(max_n, batch), dim3(64), 0, stream, d_args);
}

// -------------------------------------------------------------------------
// One wavefront per 64 keypoints (grid: 64-keypoint blocks x sequences): single-wave workgroups find a
// slot as soon as any wave of the window kernels sharing the GPU retires, a 256-thread workgroup
// waits for four on one CU (measured 0.27 ms per launch against 0.013 ms alone). The frame's pose
// matrices are wave-uniform and computed by every lane; the inside counter is added atomically
// (the caller zeroes it: the reprojection kernel of the same frame, ReprojArgs::zero_out).
__global__ __launch_bounds__(64) void filter_update_kernel(const FilterArgs* __restrict__ args) {
    const FilterArgs& a = args[blockIdx.y];
    const int n = *G(a.n_ptr);
    if ((int)blockIdx.x * 64 >= n) return;
    const int tid = threadIdx.x;
    PoseMats s_frame;
    {
        float pose[6];
        for (int i = 0; i < 6; i++) pose[i] = G(a.frame_pose)[i];
        pose_mats(pose, s_frame);
    }
    const float fx = a.cam.fx, fy = a.cam.fy, cx = a.cam.cx, cy = a.cam.cy, baseline = a.cam.baseline;
    const CamD camd = make_camd(fx, fy, cx, cy, a.cam);
    int inside = 0;

    if (const int i = blockIdx.x * 64 + tid; i < n) {        // one keypoint per lane
        // references: explicit arrays (stage API) or the keyframe table (tracker)
        float kfp[6];
        svo_kp3d r3;
        svo_kp2d r2;
        SVO_GP(KfDev) kf = nullptr;
        int kidx = 0;
        if (a.kfs) {
            kf = &G(a.kfs)[G(a.kf_id)[i] & a.kf_mask];             // (the table is a ring over the ids)
            kidx = G(a.kp_index)[i];
            for (int q = 0; q < 6; q++) kfp[q] = kf->pose[q];
            r3 = G(kf->kps3d)[kidx];
            r2 = G(kf->kps2d)[kidx];
        } else {
            for (int q = 0; q < 6; q++) kfp[q] = G(a.kf_pose)[(size_t)i * 6 + q];
            r3 = svo_kp3d{0, 0, 0};
            r2 = svo_kp2d{0, 0};
            if (a.ref3d) r3 = G(a.ref3d)[i];
            if (a.ref2d) r2 = G(a.ref2d)[i];
        }
        PoseMats km;
        pose_mats(kfp, km);
        const svo_kp2d kp2 = G(a.kps2d)[i];
        uint32_t flags = G(a.flags)[i];
        int outl = G(a.outlier_count)[i], inl = G(a.inlier_count)[i];

        if (a.do_outlier_check) {   // depth_filter.cpp:52-128
            const float d = G(a.disparity)[i];
            const float _z = baseline / (d < 0.5f ? 0.5f : d);   // std::max<float>(d, 0.5) is (a < b) ? b : a: a NaN stays (fmaxf drops it)
            const float _x = (kp2.x - cx) / fx * _z;
            const float _y = (kp2.y - cy) / fy * _z;
            float pw[3] = {_x, _y, _z};
            mat33f_vec(s_frame.R, pw, pw);
            pw[0] += s_frame.t[0]; pw[1] += s_frame.t[1]; pw[2] += s_frame.t[2];
            float av[3] = {pw[0] - kfp[0], pw[1] - kfp[1], pw[2] - kfp[2]};
            mat33f_vec(km.Ri, av, av);
            float rv[3] = {r3.x - kfp[0], r3.y - kfp[1], r3.z - kfp[2]};
            mat33f_vec(km.Ri, rv, rv);
            const float disp_ref = baseline / rv[2];
            const float disp = baseline / av[2];
            const float pixel_distance = disp - disp_ref;
            if (fabsf(pixel_distance) > 5 * 0.5f) outl++;
            else inl++;
        }

        svo_kp3d p3 = G(a.kps3d)[i];
        if (a.do_update) {          // depth_filter.cpp:130-257
            const float c1[3] = {kfp[0], kfp[1], kfp[2]};
            const float c2[3] = {s_frame.t[0], s_frame.t[1], s_frame.t[2]};
            float diff[3] = {fabsf(c1[0] - c2[0]), fabsf(c1[1] - c2[1]), fabsf(c1[2] - c2[2])};
            mat33f_vec(km.Ri, diff, diff);
            if (flags & (SVO_IGNORE_COMPLETELY | SVO_IGNORE_DURING_REFINEMENT)) {
                outl++;
            } else if (!((double)diff[0] < 0.1 && (double)diff[1] < 0.1)) {
                float p1[3] = {r2.x - cx, r2.y - cy, fx};
                mat33f_vec(km.R, p1, p1);
                float p2[3] = {kp2.x - cx, kp2.y - cy, fx};
                mat33f_vec(s_frame.R, p2, p2);
                const float A[6] = {p1[0], -p2[0], p1[1], -p2[1], p1[2], -p2[2]};
                const float yv[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
                float l[2];
                solve_svd_3x2(A, yv, l);
                const float deviation =
                    (float)(0.5 / (double)sqrtf(diff[0] * diff[0] + diff[1] * diff[1]));
                const float Rm = deviation * deviation;
                float Mx[9];
#pragma unroll
                for (int k = 0; k < 9; k++) Mx[k] = km.Ri[k] * l[0];
                const float pc[3] = {p1[0] - c1[0], p1[1] - c1[1], p1[2] - c1[2]};
                float new_p[3];
                mat33f_vec(Mx, pc, new_p);
                float _z = new_p[2];
                float kx = G(a.kf_inv_depth)[i], kP = G(a.kf_variance)[i];
                kf1_update(kx, kP, 0.0001f, Rm, 1 / _z);
                G(a.kf_inv_depth)[i] = kx;
                G(a.kf_variance)[i] = kP;
                _z = (float)(1.0 / (double)kx);
                const float _x = (r2.x - cx) / fx * _z;
                const float _y = (r2.y - cy) / fy * _z;
                float cp[3] = {_x, _y, _z};
                mat33f_vec(km.R, cp, cp);
                p3.x = c1[0] + cp[0];
                p3.y = c1[1] + cp[1];
                p3.z = c1[2] + cp[2];
            }
        }

        if (a.do_flags) {           // stereo_slam.cpp:205-226
            if (outl > inl) flags |= SVO_IGNORE_COMPLETELY;
            if (inl > outl) flags &= ~(uint32_t)SVO_IGNORE_TEMPORARY;
            if (kf) {
                G(kf->kps3d)[kidx] = p3;
                const uint32_t keep = G(kf->flags)[kidx] & SVO_IGNORE_DURING_REFINEMENT;
                G(kf->flags)[kidx] = keep | (flags & (SVO_IGNORE_TEMPORARY | SVO_IGNORE_COMPLETELY));
                G(kf->inlier_count)[kidx] = inl;
                G(kf->outlier_count)[kidx] = outl;
            }
        }
        G(a.kps3d)[i] = p3;
        if (a.do_flags) G(a.flags)[i] = flags;
        G(a.outlier_count)[i] = outl;
        G(a.inlier_count)[i] = inl;

        if (a.do_reproject) {       // stereo_slam.cpp:228-229 + keyframe_manager.cpp:55-64
            const svo_kp2d q = project_point(s_frame.Rd, s_frame.t, camd, p3);
            G(a.kps2d)[i] = q;
            if (q.x > 0 && q.y > 0 && q.x < a.width && q.y < a.height && !(flags & SVO_IGNORE_COMPLETELY))
                inside++;
        }
    }
    if (a.inside_count) {
        inside = wave_sum_i(inside);
        if (tid == 0 && inside) atomicAdd(a.inside_count, inside);
    }
}

void launch_filter(const FilterArgs* d_args, int batch, int max_n, hipStream_t stream) {
    if (max_n <= 0) return;
    hipLaunchKernelGGL(filter_update_kernel, dim3((max_n + 63) / 64, batch), dim3(64), 0, stream, d_args);
}

}  // namespace svo
