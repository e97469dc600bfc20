// svo_capi_check.hip — the diagnostics of the stage-level C API that pin the tracker's launch forms to the oracle:
// the 6x6 solve checks, the *_batch entries that launch a kernel the way the tracker does over the caller's memory,
// and the queries of the layouts and launch shapes those entries work with.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "ssd_common.hpp"
#include "svo_handle.hpp"

using namespace svo;

// the batch of a *_batch entry: 1..4096 sequences
static bool bad_batch(int batch, const void* seqs) { return batch < 1 || batch > 4096 || !seqs; }

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
    if (bad_batch(batch, n_dev) || n_bound < 0 || stride < n_bound)
        return svo_set_error(SVO_ERR_INVALID, "%s: need 1 <= batch <= 4096, n_dev and 0 <= n_bound <= stride", who);
    std::vector<int32_t> n((size_t)batch);
    HIP_TRY(hipMemcpy(n.data(), n_dev, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; b++)
        if (n[(size_t)b] < 0 || n[(size_t)b] > n_bound)
            return svo_set_error(SVO_ERR_INVALID, "%s: n_dev[%d] = %d is outside 0..n_bound = %d", who, b, n[(size_t)b], n_bound);
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
    rc = stage(h, blocks, &d);
    if (rc) return rc;
    const LaunchStatus st = launch_reproj(d, batch, n_bound, h->stream);
    HIP_TRY(st.err);
    if (waves) *waves = st.shape.waves;
    if (cap) *cap = st.shape.cap;
    if (!st.shape.fits) return svo_set_error(SVO_ERR_CAPACITY, "svo_reproj_gn_batch: %d keypoints do not fit LDS", n_bound);
    return finish_launch(h);
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
    rc = stage(h, blocks, &d);
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

// svo_sia_records_check: the alignment records of sia_prep_kernel (sia.hip) against the kernel it replaced.
// sia_prep_ref_kernel is that kernel as it was, one lane per (keypoint, patch pixel) and every tap a byte load of its
// own: 49 loads per lane behind three bounds branches, stores of sixteen 16-byte pieces per instruction. It runs only
// here, as the definition of every word of rec_ws (values, NaN payloads, and which words are written at all).
__global__ __launch_bounds__(64) void sia_prep_ref_kernel(const SiaArgs* __restrict__ args) {
    const SiaArgs& a = args[blockIdx.z];
    const int n = min(*G(a.n_ptr), a.rec_cap);
    const int level = a.cam.min_pyramid_level_pose_estimation + blockIdx.y;
    if (level >= a.cam.max_pyramid_levels) return;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    const int kp = idx >> 4, px = idx & 15;
    const int span = (n + 3) & ~3;                       // the consumer copies float4 columns
    if (kp >= span) return;                              // (whole 16-lane rows leave together)
    const ImgView prev = a.prev[level];
    const int divider = 1 << level;
    float g0 = 0, g1 = 0, psr = __builtin_nanf(""), i1 = __builtin_nanf("");
    const bool active = kp < n && !(a.flags && (G(a.flags)[kp] & SVO_IGNORE_TEMPORARY));
    if (active) {
        svo_kp2d kref = G(a.kps2d)[kp];
        if (level != 0) { kref.x /= divider; kref.y /= divider; }      // setLevel
        // the reference's walk over the patch: x++ per column, x -= 4 and y++ per row (float arithmetic)
        float kx = kref.x - 2.f, ky = kref.y - 2.f;
        for (int rr = 0; rr < (px >> 2); rr++) {
            kx += 1.f; kx += 1.f; kx += 1.f; kx += 1.f;
            kx -= 4.f;
            ky += 1.f;
        }
        for (int cc = 0; cc < (px & 3); cc++) kx += 1.f;
        // calculate_hessian bounds (:351-352)
        if (!(((double)kx - 2.0) < 0 || ((double)ky - 2.0) < 0 ||
              ((double)kx + 3.0) >= prev.w || ((double)ky + 3.0) >= prev.h)) {
            const float int1 = patch_sum(prev.g(), prev.stride, kx + 1, ky);
            const float int2 = patch_sum(prev.g(), prev.stride, kx - 1, ky);
            const float int3 = patch_sum(prev.g(), prev.stride, kx, ky + 1);
            const float int4 = patch_sum(prev.g(), prev.stride, kx, ky - 1);
            g0 = int1 - int2; g1 = int3 - int4;
        }
        // reference half of the residual test (:449-453)
        if (!(((double)kx - 1.0) < 0 || ((double)ky - 1.0) < 0 ||
              ((double)kx + 2.0) > prev.w || ((double)ky + 2.0) > prev.h))
            psr = patch_sum(prev.g(), prev.stride, kx, ky);
        // reference half of the cost (image_comparison.cpp:20-88): one window test per keypoint
        const int ps = a.cam.window_size_pose_estimator;
        const float half_size = ((float)ps - 1.0f) / 2.0f;
        const float s1x = kref.x - half_size, s1y = kref.y - half_size;
        const float f1x = floorf(s1x), f1y = floorf(s1y);
        if (f1x >= 0.f && f1y >= 0.f && f1x < 65536.f && f1y < 65536.f) {
            const int ip1x = (int)f1x, ip1y = (int)f1y;
            if (ip1y + ps < prev.h && ip1x + ps < prev.w) {
                const float x12 = s1x - (float)ip1x, y12 = s1y - (float)ip1y;
                const float x11 = 1.0f - x12, y11 = 1.0f - y12;
                const float m0 = x11 * y11, m1 = x12 * y11, m2 = x11 * y12, m3 = x12 * y12;
                const uint8_t* p = prev.g() + (size_t)((px >> 2) + ip1y) * prev.stride + (px & 3) + ip1x;
                float t = 0;
                t += m0 * (float)p[0];
                t += m1 * (float)p[1];
                t += m2 * (float)p[prev.stride];
                t += m3 * (float)p[prev.stride + 1];
                i1 = t;
            }
        }
    }
    float* out = G(a.rec_ws) + (size_t)blockIdx.y * SIA_REC_ROWS * a.rec_cap;
    out[(size_t)(REC_I1 * 16 + px) * a.rec_cap + kp] = i1;
    out[(size_t)(REC_PS * 16 + px) * a.rec_cap + kp] = psr;
    out[(size_t)(REC_G0 * 16 + px) * a.rec_cap + kp] = g0;
    out[(size_t)(REC_G1 * 16 + px) * a.rec_cap + kp] = g1;
    const float gxx = row16_sum_dpp(g0 * g0), gxy = row16_sum_dpp(g0 * g1), gyy = row16_sum_dpp(g1 * g1);
    if (px == 0) {
        out[(size_t)64 * a.rec_cap + kp] = gxx;
        out[(size_t)65 * a.rec_cap + kp] = gxy;
        out[(size_t)66 * a.rec_cap + kp] = gyy;
    }
}

// words that differ between a[0..n) and b[0..n): out[0] += their number, out[1] = min(out[1], the first one's index)
__global__ void __launch_bounds__(256) words_diff_kernel(const uint32_t* a, const uint32_t* b, size_t n, unsigned long long* out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        if (a[i] != b[i]) {
            atomicAdd(&out[0], 1ull);
            atomicMin(&out[1], (unsigned long long)i);
        }
}

// Both kernels on the same batch of SiaArgs: `batch` sequences with keypoint arrays of `stride` slots each (kps2d,
// flags — null: no flags), n_dev[b] <= n_bound keypoints, prev_pyr[b * max_pyramid_levels + level] the previous
// frame's level images (any base alignment, any stride >= width, at least 3 x 3; the levels below
// min_pyramid_level_pose_estimation are not read). Each kernel writes a workspace of its own, [batch][levels
// used][68][rec_cap] floats filled with ws_fill first, so a word only one of them writes differs too. n_diff: the
// number of differing 32-bit words, first_diff: the index of the first (-1: none); rec_out: null, or device memory that
// receives the new kernel's workspace; ref_out: the same for the reference kernel's.
extern "C" int svo_sia_records_check(svo_handle* h, int batch, int stride, const int32_t* n_dev, int n_bound,
                                     const svo_kp2d* kps2d, const uint32_t* flags, const svo_image* prev_pyr,
                                     const svo_camera_settings* cam, int rec_cap, uint32_t ws_fill, float* rec_out,
                                     float* ref_out, int64_t* n_diff, int64_t* first_diff) {
    CHECK_H(h);
    if (!cam || !prev_pyr || !n_diff || !first_diff || (n_bound > 0 && !kps2d))
        return svo_set_error(SVO_ERR_INVALID, "svo_sia_records_check: bad arguments");
    if (cam->max_pyramid_levels < 1 || cam->max_pyramid_levels > 7 || cam->min_pyramid_level_pose_estimation < 0 ||
        cam->min_pyramid_level_pose_estimation >= cam->max_pyramid_levels)
        return svo_set_error(SVO_ERR_INVALID, "svo_sia_records_check: max_pyramid_levels must be 1..7, min below it");
    if (rec_cap < 4 || (rec_cap & 3) || rec_cap < n_bound || rec_cap > (1 << 20))
        return svo_set_error(SVO_ERR_INVALID, "svo_sia_records_check: rec_cap must be a multiple of 4 in n_bound..2^20");
    int rc = check_batch_counts("svo_sia_records_check", batch, stride, n_dev, n_bound);
    if (rc) return rc;
    const int levels = cam->max_pyramid_levels;
    for (int b = 0; b < batch; b++)
        for (int l = cam->min_pyramid_level_pose_estimation; l < levels; l++) {
            const svo_image& p = prev_pyr[(size_t)b * levels + l];
            if (!p.data || p.width < 3 || p.height < 3 || p.stride < p.width)
                return svo_set_error(SVO_ERR_INVALID, "svo_sia_records_check: sequence %d level %d: no image of at least 3 x 3", b, l);
        }
    const size_t rec_floats = sia_rec_ws_floats(*cam, rec_cap), words = rec_floats * (size_t)batch;
    DevPtr<float> ws;
    DevPtr<unsigned long long> res;
    HIP_TRY(dev_malloc(ws, sizeof(float) * 2 * words));
    HIP_TRY(dev_malloc(res, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws.get()), (int)ws_fill, 2 * words, h->stream));
    const unsigned long long init[2] = {0ull, ~0ull};
    HIP_TRY(hipMemcpyAsync(res.get(), init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    std::vector<SiaArgs> blocks((size_t)2 * batch);          // [0, batch): the kernel's, [batch, 2 batch): the reference's
    for (int k = 0; k < 2 * batch; k++) {
        SiaArgs& sa = blocks[(size_t)k];
        const int b = k % batch;
        memset(&sa, 0, sizeof(sa));
        for (int l = cam->min_pyramid_level_pose_estimation; l < levels; l++) sa.prev[l] = make_view(prev_pyr[(size_t)b * levels + l]);
        sa.cam = *cam;
        sa.n_ptr = n_dev + b;
        sa.kps2d = kps2d ? kps2d + (size_t)b * (size_t)stride : nullptr;
        sa.flags = flags ? flags + (size_t)b * (size_t)stride : nullptr;
        sa.rec_ws = ws.get() + (size_t)k * rec_floats;
        sa.rec_cap = rec_cap;
        sa.dbg_level = -1;
        sa.cap = stride;
    }
    SiaArgs* d;
    rc = stage(h, blocks, &d);
    if (rc) return rc;
    launch_sia_prep(d, batch, *cam, n_bound, h->stream);
    HIP_TRY(hipGetLastError());
    const int nb = n_bound > 1 ? n_bound : 1;
    sia_prep_ref_kernel<<<dim3((((nb + 3) & ~3) * 16 + 63) / 64, levels - cam->min_pyramid_level_pose_estimation, batch), 64, 0,
                          h->stream>>>(d + batch);
    HIP_TRY(hipGetLastError());
    words_diff_kernel<<<(unsigned)std::min<size_t>((words + 255) / 256, 1024), 256, 0, h->stream>>>(
        reinterpret_cast<const uint32_t*>(ws.get()), reinterpret_cast<const uint32_t*>(ws.get() + words), words, res.get());
    HIP_TRY(hipGetLastError());
    if (rec_out) HIP_TRY(hipMemcpyAsync(rec_out, ws.get(), sizeof(float) * words, hipMemcpyDeviceToDevice, h->stream));
    if (ref_out) HIP_TRY(hipMemcpyAsync(ref_out, ws.get() + words, sizeof(float) * words, hipMemcpyDeviceToDevice, h->stream));
    unsigned long long got[2];
    HIP_TRY(hipMemcpyAsync(got, res.get(), sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n_diff = (int64_t)got[0];
    *first_diff = got[0] ? (int64_t)got[1] : -1;
    return SVO_OK;            // (the workspaces are freed here: the launches are complete)
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
    rc = stage(h, blocks, &d);
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
    if (bad_batch(batch, seqs) || n_bound < 0)
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
    int rc = stage(h, table, &d_table);
    if (rc) return rc;
    DevPtr<PoseMats> mats;
    if (use_mats) {
        std::vector<const float*> poses((size_t)batch);
        for (int b = 0; b < batch; b++) poses[(size_t)b] = seqs[b].pose;
        const float** d_poses;
        rc = stage(h, poses, &d_poses);
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
    rc = stage(h, blocks, &d);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    launch_klt(d, batch, n_bound, win, h->stream);
    return finish_launch(h);                       // (mats is freed on return: the launch is complete)
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
    if (bad_batch(batch, seqs) || cap < 1)
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
    const int rc = stage(h, blocks, &d);
    if (rc) return rc;
    if (threads) *threads = compact_pick_threads(cap);
    launch_compact(d, batch, cap, h->stream);
    return finish_launch(h);
}

extern "C" int svo_keyframe_merge_batch(svo_handle* h, int batch, const svo_merge_sequence* seqs, int n_levels,
                                        int max_cells, int cap, int* threads) {
    CHECK_H(h);
    if (bad_batch(batch, seqs) || n_levels < 1 || n_levels > SVO_MAX_PYRAMID_LEVELS || max_cells < 1 || cap < 1)
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
    const int rc = stage(h, blocks, &d);
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
    if (bad_batch(batch, seqs) || cap < 1)
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
    const int rc = stage(h, blocks, &d);
    if (rc) return rc;
    launch_kf_init(d, batch, h->stream);
    return finish_launch(h);
}

// the checks of the two SSD entries and the argument blocks as pack_ssd fills them. own_disparity: the sequences'
// disparity arrays are the output (svo_ssd_disparity_batch) and must exist; otherwise the caller sets the blocks' own.
static int ssd_fill_blocks(const char* who, svo_handle* h, int batch, const svo_ssd_sequence* seqs, int n_bound, int win,
                           int search_y, bool own_disparity, std::vector<SsdArgs>& blocks) {
    constexpr int kMaxIndex = 1 << 29;             // first, *first_ptr and n_bound: their sum stays an int
    if (bad_batch(batch, seqs) || n_bound < 0 || n_bound > kMaxIndex)
        return svo_set_error(SVO_ERR_INVALID, "%s: need 1 <= batch <= 4096, seqs and 0 <= n_bound <= 2^29", who);
    if (win < 1 || win > 35 || search_y < 0 || search_y > 8)
        return svo_set_error(SVO_ERR_INVALID, "%s: win<=35, search_y<=8 supported", who);
    HIP_TRY(hipStreamSynchronize(h->stream));
    blocks.resize((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const svo_ssd_sequence& s = seqs[b];
        if (klt_bad_view(s.left) || klt_bad_view(s.right) || !s.n || s.cap < 0 ||
            (s.cap > 0 && (!s.kps2d || (own_disparity && !s.disparity))) || s.first < 0 || s.first > kMaxIndex)
            return svo_set_error(SVO_ERR_INVALID, "%s: sequence %d: bad arguments", who, b);
        if (s.win < 1 || s.win > win || s.search_x < 0 || s.search_x > 64 || s.search_y < 0 || s.search_y > search_y)
            return svo_set_error(SVO_ERR_INVALID, "%s: sequence %d: win %d, search_x %d, search_y %d exceed "
                                 "the launch's %d, 64, %d", who, b, s.win, s.search_x, s.search_y, win, search_y);
        int32_t n = 0, first = 0;
        if (const int rc = read_i32(s.n, 1, &n)) return rc;
        if (s.first_ptr)
            if (const int rc = read_i32(s.first_ptr, 1, &first)) return rc;
        if (n < 0 || n > s.cap || first < 0 || first > kMaxIndex)
            return svo_set_error(SVO_ERR_INVALID, "%s: sequence %d: n = %d is outside 0..cap = %d, or "
                                 "*first_ptr = %d is outside 0..2^29", who, b, n, s.cap, first);
        SsdArgs& sa = blocks[(size_t)b];
        memset(&sa, 0, sizeof(sa));
        sa.left = make_view(s.left); sa.right = make_view(s.right);
        sa.n_ptr = s.n; sa.kps2d = s.kps2d; sa.disparity = s.disparity;
        sa.win = s.win; sa.search_x = s.search_x; sa.search_y = s.search_y; sa.clamp_half = s.clamp_half;
        sa.first = s.first; sa.first_ptr = s.first_ptr;
        sa.enable = s.enable;
    }
    return SVO_OK;
}

extern "C" int svo_ssd_disparity_batch(svo_handle* h, int batch, const svo_ssd_sequence* seqs, int n_bound, int win,
                                       int search_y, int* max_win) {
    CHECK_H(h);
    std::vector<SsdArgs> blocks;
    int rc = ssd_fill_blocks("svo_ssd_disparity_batch", h, batch, seqs, n_bound, win, search_y, true, blocks);
    if (rc) return rc;
    SsdArgs* d;
    rc = stage(h, blocks, &d);
    if (rc) return rc;
    if (max_win) *max_win = ssd_pick_max_win(win, search_y);
    launch_ssd(d, batch, n_bound, win, search_y, h->stream);
    return finish_launch(h);
}

// svo_ssd_disparity_check: ssd_disparity_kernel (depth.hip) against the kernel it replaced. ssd_disparity_ref_kernel is
// that kernel as it was: one workgroup of four waves per keypoint, a wave per (16-row, 16-column) block of the match map
// with a Toeplitz fragment of its own, the column sums in a plane of LDS, five barriers. It runs only here, as the
// definition of every disparity word (values, -1 for a skipped keypoint, and which entries are written at all).
constexpr int SSD_W_STRIDE = 105;               // ints per row of the column sums (= 1 mod 8: the 8 rows x 8 segments of 8 columns
                                                // that a wave reads in the row pass hit 64 different banks; 100 was a 4-way conflict)
constexpr int SSD_REF_THREADS = 256;

template <int SSD_MAX_WIN, int SSD_MAX_MH>
__global__ __launch_bounds__(SSD_REF_THREADS) void ssd_disparity_ref_kernel(const SsdArgs* __restrict__ args) {
    constexpr int SSD_THREADS = SSD_REF_THREADS;
    constexpr int SSD_R_ROWS = SSD_MAX_WIN + SSD_MAX_MH, SSD_MAX_MATCH = SSD_MAX_MW * SSD_MAX_MH;
    const SsdArgs& a = args[blockIdx.y];
    if (a.enable && !*G(a.enable)) return;
    const int n = *G(a.n_ptr);
    const int kp = a.first + (a.first_ptr ? *G(a.first_ptr) : 0) + (int)blockIdx.x;
    if (kp >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    __shared__ __attribute__((aligned(16))) uint8_t s_t[(SSD_MAX_WIN + 1) * SSD_T_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t s_r[SSD_R_ROWS * SSD_R_STRIDE];
    __shared__ int s_w[SSD_MAX_MH * SSD_W_STRIDE];
    __shared__ int s_tt[4];
    __shared__ unsigned long long s_key[SSD_THREADS / 64];
    __shared__ int s_sum[SSD_THREADS / 64], s_cnt[SSD_THREADS / 64];

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
    if (tw > SSD_MAX_WIN || th > SSD_MAX_WIN || mw > SSD_MAX_MW || mh > SSD_MAX_MH || rw > SSD_W_STRIDE ||
        rh > SSD_R_ROWS)
        skip = true;  // the host validates window sizes; never taken with valid settings
    if (skip) {
        if (tid == 0) G(a.disparity)[kp] = -1.0f;
        return;
    }

    // ---- stage: template rows as [16 zero bytes | row ^ 0x80 | zeros], search region ^ 0x80 (bytes past
    // the region's width: 0x80), 16 bytes per lane and step: a template row is three chunks, a region row
    // up to six
    static_assert(SSD_T_STRIDE % 16 == 0 && SSD_R_STRIDE % 16 == 0, "rows are whole 16-byte chunks");
    for (int i = tid; i < (SSD_MAX_WIN + 1) * (SSD_T_STRIDE / 16); i += SSD_THREADS) {
        const int r = i / (SSD_T_STRIDE / 16), ch = i % (SSD_T_STRIDE / 16);
        const int c = 16 * (ch - 1);                      // template column of the chunk's first byte
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < th && c >= 0 && c < tw) v = load_u8x16(a.left, y11 + r, x11 + c, tw - c, 0x80808080u, 0u);
        reinterpret_cast<uint4*>(s_t)[i] = v;
    }
    for (int i = tid; i < SSD_R_ROWS * (SSD_R_STRIDE / 16); i += SSD_THREADS) {
        const int r = i / (SSD_R_STRIDE / 16), ch = i % (SSD_R_STRIDE / 16);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < rh && 16 * ch < rw) v = load_u8x16(a.right, y21 + r, x21 + 16 * ch, rw - 16 * ch, 0x80808080u, 0x80808080u);
        reinterpret_cast<uint4*>(s_r)[i] = v;
    }
    __syncthreads();

    // ---- sum T^2 (wave 3) and the column sums W[k][x] = sum_{r<th} R[k+r][x]^2 (one thread per column)
    if (wave == SSD_THREADS / 64 - 1) {
        int tt = 0;
        if (lane < th) {
            const uint32_t* trow = reinterpret_cast<const uint32_t*>(s_t + lane * SSD_T_STRIDE) + 4;
#pragma unroll
            for (int d = 0; d < 9; d++) tt = __builtin_amdgcn_sdot4((int)trow[d], (int)trow[d], tt, false);
        }
        tt = wave_sum_dpp_i(tt);
        if (lane == 0) s_tt[0] = tt;
    }
    if (tid < rw) {
        const int8_t* col = reinterpret_cast<const int8_t*>(s_r) + tid;
        int sq = 0;
        for (int r = 0; r < th; r++) {
            const int v = col[r * SSD_R_STRIDE];
            sq += __mul24(v, v);
        }
        s_w[tid] = sq;
        for (int k = 1; k < mh; k++) {
            const int vn = col[(k + th - 1) * SSD_R_STRIDE], vo = col[(k - 1) * SSD_R_STRIDE];
            sq += __mul24(vn, vn) - __mul24(vo, vo);
            s_w[k * SSD_W_STRIDE + tid] = sq;
        }
    }

    // ---- cross term on the matrix cores: wave -> (row block, column block) of the match map
    const int n_jb = (mw + 15) >> 4, n_mb = (mh + 15) >> 4;
    const int fm = lane & 15, fh = lane >> 4;        // fragment row / column and 16-byte k slice
    constexpr int SSD_SLOTS = (10 + SSD_THREADS / 64 - 1) / (SSD_THREADS / 64);   // <= 2 x 5 blocks over the waves
    ssd_v4i acc[SSD_SLOTS];
    int task_of[SSD_SLOTS];
#pragma unroll
    for (int t = 0; t < SSD_SLOTS; t++) { acc[t] = ssd_v4i{0, 0, 0, 0}; task_of[t] = -1; }
    {
        int slot = 0;
        for (int task = wave; task < n_jb * n_mb && slot < SSD_SLOTS; task += SSD_THREADS / 64, slot++) {
            task_of[slot] = task;
            const int mb = task >= n_jb ? 1 : 0, jb = task - mb * n_jb;      // (at most two row blocks: the map has <= 17 rows)
            // B: bytes [16 + 16 fh - fm, +16) of the padded template row
            const int o = 16 + 16 * fh - fm;
            const uint32_t* tb = reinterpret_cast<const uint32_t*>(s_t) + (o >> 2);
            const unsigned sh = (unsigned)(o & 3);
            const uint8_t* ab = s_r + (16 * jb + 16 * fh);
            const int arow = 16 * mb + fm;
            ssd_v4i c = {0, 0, 0, 0};
            for (int r = 0; r < th; r++) {
                const uint32_t* t = tb + r * (SSD_T_STRIDE / 4);
                const uint32_t t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];
                ssd_v4i bf;
                bf.x = (int)__builtin_amdgcn_alignbyte(t1, t0, sh);
                bf.y = (int)__builtin_amdgcn_alignbyte(t2, t1, sh);
                bf.z = (int)__builtin_amdgcn_alignbyte(t3, t2, sh);
                bf.w = (int)__builtin_amdgcn_alignbyte(t4, t3, sh);
                const ssd_v4i af = *reinterpret_cast<const ssd_v4i*>(ab + min(arow + r, SSD_R_ROWS - 1) * SSD_R_STRIDE);
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, c, 0, 0, 0);
            }
            acc[slot] = c;
        }
    }
    __syncthreads();

    // ---- window sums of R^2: rows of W, 8 sliding segments per map row -> s_m. The match map takes
    // the place of the search region, which nobody reads after the barrier above
    static_assert(sizeof(int) * SSD_MAX_MATCH <= SSD_R_ROWS * SSD_R_STRIDE, "match map must fit the region tile");
    static_assert(SSD_MAX_MH <= 32, "two row blocks of 16 at most");
    int* const s_m = reinterpret_cast<int*>(s_r);
    {
        const int seg_len = (mw + 7) >> 3;
        for (int item = tid; item < mh * 8; item += SSD_THREADS) {
            const int k = item >> 3, j0 = (item & 7) * seg_len, j1 = min(mw, j0 + seg_len);
            if (j0 < j1) {
                const int* wrow = &s_w[k * SSD_W_STRIDE];
                int sq = 0;
                for (int c = 0; c < tw; c++) sq += wrow[j0 + c];
                s_m[k * mw + j0] = sq;
                for (int j = j0 + 1; j < j1; j++) {
                    sq += wrow[j + tw - 1] - wrow[j - 1];
                    s_m[k * mw + j] = sq;
                }
            }
        }
    }
    __syncthreads();
    {
        const int stt = s_tt[0];
#pragma unroll
        for (int slot = 0; slot < SSD_SLOTS; slot++) {
            const int task = task_of[slot];
            if (task < 0) continue;
            const int mb = task >= n_jb ? 1 : 0, jb = task - mb * n_jb;      // (at most two row blocks: the map has <= 17 rows)
            const int j = 16 * jb + fm;                     // C/D: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = 16 * mb + 4 * fh + i;
                if (k < mh && j < mw) s_m[k * mw + j] += stt - 2 * acc[slot][i];
            }
        }
    }
    __syncthreads();

    const int nm = mw * mh;
    unsigned long long best = ~0ull;
    for (int o = tid; o < nm; o += SSD_THREADS) {
        const unsigned long long key = ((unsigned long long)__float_as_uint((float)s_m[o]) << 32) | (unsigned)o;
        best = key < best ? key : best;
    }
    // first minimum of the FLOAT map in row-major order == smallest (float bits, index) key: an SSD is not
    // negative, and non-negative floats order like their bit patterns. Above 2^24 different integers round to
    // one float, and cv::minMaxLoc sees the floats: the earlier position wins, not the smaller integer.
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    if ((tid & 63) == 0) s_key[tid >> 6] = best;
    __syncthreads();
    best = s_key[0];
    for (int w = 1; w < SSD_THREADS / 64; w++) best = s_key[w] < best ? s_key[w] : best;
    const int min_o = (int)(best & 0xffffffffu);
    const int minx = min_o % mw, miny = min_o / mw;
    const float minVal = __uint_as_float((unsigned)(best >> 32));

    int sumj = 0, cnt = 0;
    // o / mw without an integer division: exact for o * mw < 2^20 (the map has at most 65 x 17 entries)
    const unsigned magic = ((1u << 20) + (unsigned)mw - 1u) / (unsigned)mw;
    for (int o = tid; o < nm; o += SSD_THREADS) {
        const int k = (int)(((unsigned)o * magic) >> 20), j = o - k * mw;
        if (j >= minx && k >= miny && (double)(float)s_m[o] <= (double)minVal) { sumj += j; cnt++; }
    }
    sumj = wave_sum_dpp_i(sumj);
    cnt = wave_sum_dpp_i(cnt);
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sumj; s_cnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        int ts = 0, tc = 0;
        for (int w = 0; w < SSD_THREADS / 64; w++) { ts += s_sum[w]; tc += s_cnt[w]; }
        float minPos = (float)ts;      // sum of small ints: exact in float in any order
        minPos = minPos / tc;
        G(a.disparity)[kp] = a.clamp_half ? fmaxf(0.5f, minPos) : minPos;
    }
}

void svo::launch_ssd_ref(const SsdArgs* d_args, int batch, int max_n, int win, int search_y, hipStream_t stream) {
    if (max_n <= 0) return;
    if (ssd_pick_max_win(win, search_y) == 31)
        hipLaunchKernelGGL((ssd_disparity_ref_kernel<31, 13>), dim3(max_n, batch), dim3(SSD_REF_THREADS), 0, stream, d_args);
    else
        hipLaunchKernelGGL((ssd_disparity_ref_kernel<SSD_WIN_ALL, SSD_MH_ALL>), dim3(max_n, batch), dim3(SSD_REF_THREADS), 0, stream, d_args);
}

// Both kernels on the same batch of svo_ssd_sequence, through launch_ssd's form (grid (n_bound, batch), the shape
// that win and search_y choose). Neither writes the sequences' own disparity arrays (they may be NULL): each kernel
// gets [batch][stride] floats of its own, every word set to `fill` first, sequence b's entries at b * stride, so an
// entry that only one kernel writes differs too, and an entry nobody wrote still holds `fill`. stride >= every cap.
// n_diff: the number of differing 32-bit words, first_diff: the index of the first (-1: none); disp_out / ref_out: null,
// or device memory of [batch][stride] floats that receives the kernel's / the reference kernel's array.
extern "C" int svo_ssd_disparity_check(svo_handle* h, int batch, const svo_ssd_sequence* seqs, int n_bound, int win,
                                       int search_y, int stride, uint32_t fill, float* disp_out, float* ref_out,
                                       int64_t* n_diff, int64_t* first_diff) {
    CHECK_H(h);
    if (!n_diff || !first_diff || stride < 1)
        return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_check: need n_diff, first_diff and stride >= 1");
    std::vector<SsdArgs> blocks;
    int rc = ssd_fill_blocks("svo_ssd_disparity_check", h, batch, seqs, n_bound, win, search_y, false, blocks);
    if (rc) return rc;
    for (int b = 0; b < batch; b++)
        if (seqs[b].cap > stride)
            return svo_set_error(SVO_ERR_INVALID, "svo_ssd_disparity_check: sequence %d: cap %d exceeds stride %d", b, seqs[b].cap, stride);
    const size_t words = (size_t)batch * (size_t)stride;
    DevPtr<float> ws;
    DevPtr<unsigned long long> res;
    HIP_TRY(dev_malloc(ws, sizeof(float) * 2 * words));
    HIP_TRY(dev_malloc(res, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws.get()), (int)fill, 2 * words, h->stream));
    const unsigned long long init[2] = {0ull, ~0ull};
    HIP_TRY(hipMemcpyAsync(res.get(), init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    blocks.resize((size_t)2 * batch);                        // [0, batch): the kernel's, [batch, 2 batch): the reference's
    for (int b = 0; b < batch; b++) {
        blocks[(size_t)b].disparity = ws.get() + (size_t)b * stride;
        blocks[(size_t)(batch + b)] = blocks[(size_t)b];
        blocks[(size_t)(batch + b)].disparity = ws.get() + words + (size_t)b * stride;
    }
    SsdArgs* d;
    rc = stage(h, blocks, &d);
    if (rc) return rc;
    launch_ssd(d, batch, n_bound, win, search_y, h->stream);
    HIP_TRY(hipGetLastError());
    launch_ssd_ref(d + batch, batch, n_bound, win, search_y, h->stream);
    HIP_TRY(hipGetLastError());
    words_diff_kernel<<<(unsigned)std::min<size_t>((words + 255) / 256, 1024), 256, 0, h->stream>>>(
        reinterpret_cast<const uint32_t*>(ws.get()), reinterpret_cast<const uint32_t*>(ws.get() + words), words, res.get());
    HIP_TRY(hipGetLastError());
    if (disp_out) HIP_TRY(hipMemcpyAsync(disp_out, ws.get(), sizeof(float) * words, hipMemcpyDeviceToDevice, h->stream));
    if (ref_out) HIP_TRY(hipMemcpyAsync(ref_out, ws.get() + words, sizeof(float) * words, hipMemcpyDeviceToDevice, h->stream));
    unsigned long long got[2];
    HIP_TRY(hipMemcpyAsync(got, res.get(), sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n_diff = (int64_t)got[0];
    *first_diff = got[0] ? (int64_t)got[1] : -1;
    return SVO_OK;            // (the workspaces are freed here: the launches are complete)
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
    if (bad_batch(batch, seqs) || n_bound < 0)
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
    const int rc = stage(h, blocks, &d);
    if (rc) return rc;
    launch_filter(d, batch, n_bound, h->stream);
    return finish_launch(h);
}
