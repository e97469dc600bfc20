// svo_device.hpp — device-side math shared by the gfx950 kernels.
//
// The float arithmetic follows the reference expression by expression
// (built with -ffp-contract=off: no fused multiply-add), so per-element
// results match a CPU evaluation of the same formulas; only the order of the
// big reductions differs. Reference lines are cited per function
// (paths relative to the reference repository).
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/svo_types.h"
#include "../../include/svo_libm.h"

namespace svo {

// Pointers that reach a kernel through an argument block in memory are generic to the compiler:
// it emits flat_load / flat_store and must drain vmcnt AND lgkmcnt around every LDS access next to
// them. Device code therefore casts them to the global address space where they are used
// (G(ptr), ImgView::g()): global_load / global_store with counted waits, scalar loads for
// wave-uniform values.
#if defined(__HIP_DEVICE_COMPILE__)
#define SVO_GP(T) __attribute__((address_space(1))) T*
#else
#define SVO_GP(T) T*      /* host pass: device functions are only parsed */
#endif
template <class T>
__device__ __forceinline__ SVO_GP(T) G(T* p) { return (SVO_GP(T))p; }

struct ImgView {
    const uint8_t* data;
    int w, h, stride;
    __device__ __forceinline__ SVO_GP(const uint8_t) g() const { return (SVO_GP(const uint8_t))data; }
    __device__ __forceinline__ SVO_GP(uint8_t) gw() const { return (SVO_GP(uint8_t))data; }
};

__host__ __device__ inline ImgView make_view(const svo_image& im) {
    return ImgView{im.data, im.width, im.height, im.stride};
}

// ------------------------------------------------------ address-space typed access
// A generic pointer that is known to point into LDS: cast to address space 3 so
// the compiler emits ds_read/ds_write instead of flat instructions.
#define SVO_LDS(T) __attribute__((address_space(3))) T
template <bool LDS, typename T>
__device__ inline T mem_ld(const T* p, int i) {
    if constexpr (LDS) return ((const SVO_LDS(T)*)p)[i];
    else return p[i];
}
template <bool LDS, typename T>
__device__ inline void mem_st(T* p, int i, const T& v) {
    if constexpr (LDS) ((SVO_LDS(T)*)p)[i] = v;
    else p[i] = v;
}

// ---------------------------------------------------------------- wave ops
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// DPP (data-parallel primitive) cross-lane adds: no LDS crossbar, ~1 VALU op each.
// A DPP row is 16 lanes; controls: quad_perm(1,0,3,2)=0xB1, quad_perm(2,3,0,1)=0x4E,
// row_half_mirror=0x141, row_mirror=0x140.
template <int CTRL>
__device__ inline float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ inline int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
// sum over each group of 16 consecutive lanes, result in all 16 lanes (fixed order)
__device__ inline float row16_sum_dpp(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return v;
}
__device__ inline int row16_sum_dpp_i(int v) {
    v += dpp_i<0xB1>(v);
    v += dpp_i<0x4E>(v);
    v += dpp_i<0x141>(v);
    v += dpp_i<0x140>(v);
    return v;
}
// sum over the 64 lanes of the wave, same value (and same rounding) in every lane
__device__ inline float wave_sum_dpp(float v) {
    v = row16_sum_dpp(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return ((r0 + r1) + r2) + r3;
}
__device__ inline int wave_sum_dpp_i(int v) {
    v = row16_sum_dpp_i(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
           __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
// sum over the 64 lanes with the wave-wide DPP forms of gfx9 (row_bcast:15 / row_bcast:31 carry a
// row's last lane into the next rows): six fused v_add_u32_dpp and one v_readlane (wave_sum_dpp_i:
// four adds, four readlanes, three scalar adds). Integer adds: any order gives the same bits.
__device__ inline int wave_sum_bcast_i(int v) {
    v = row16_sum_dpp_i(v);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}
// exact sum of per-lane int32 partials (|v| < 2^31) as a double (|sum| < 2^37 is an integer a double
// holds exactly): low 16 bits and the signed high part are reduced separately in int32. (float) of
// the result rounds the exact integer once, like (float) of the 64-bit integer sum.
__device__ inline double wave_sum_i32_to_f64(int v) {
    const int lo = wave_sum_bcast_i(v & 0xFFFF);
    const int hi = wave_sum_bcast_i(v >> 16);
    return (double)hi * 65536.0 + (double)lo;
}
// exact 64-bit sum of per-lane int32 partials (|v| < 2^31): low 16 bits and the
// signed high part are reduced separately in int32 and recombined
__device__ inline long long wave_sum_i32_to_i64(int v) {
    const int lo = wave_sum_dpp_i(v & 0xFFFF);
    const int hi = wave_sum_dpp_i(v >> 16);
    return (long long)hi * 65536LL + (long long)lo;
}

// ------------------------------------------------- reference-order sums
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

// sequential sum of buf[0..n) continuing from s. buf is in LDS, zero padded to a multiple of 128
// floats (adding the zeros is exact): every block of 128 is 32 ds_read_b128 issued back to back
// and one chain of 128 adds behind them, so the add chain, not the LDS, sets the pace.
__device__ inline float ordered_sum(const float* buf, int n, float s) {
    const SVO_LDS(v4f)* p = (const SVO_LDS(v4f)*)buf;
    for (int b = 0; b < n; b += 128, p += 32) {
        v4f v[32];
#pragma unroll
        for (int j = 0; j < 32; j++) v[j] = p[j];
#pragma unroll
        for (int j = 0; j < 32; j++) { s += v[j].x; s += v[j].y; s += v[j].z; s += v[j].w; }
    }
    return s;
}

// sequential sum over the 64 lanes of a wave, lane 0 first (v_readlane + add: no LDS), continuing from s
__device__ inline float ordered_wave_sum(float v, float s) {
#pragma unroll
    for (int j = 0; j < 64; j++) s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
    return s;
}

// ------------------------------------------------------------- rotations
// cv::Rodrigues (vector -> matrix) in double: PoseManager::set_pose,
// src/lib/pose_manager.cpp:15-16, and inside cv::projectPoints,
// src/lib/transform_keypoints.cpp:45. R(-r) is exactly the transpose.
__host__ __device__ inline void rodrigues_d(const float r[3], double R[9]) {
    double rx = r[0], ry = r[1], rz = r[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 9; i++) R[i] = 0.0;
        R[0] = R[4] = R[8] = 1.0;
        return;
    }
    double s, c;
    svo_sincos(theta, &s, &c);   // the same polynomial as the oracle: include/svo_libm.h
    const double c1 = 1.0 - c;
    const double itheta = 1.0 / theta;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double e = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        double t = c * e;
        t = t + c1 * rrt[k];
        R[k] = t + s * r_x[k];
    }
}

// Everything a kernel needs about one pose: R(r) in double (R(-r) = transpose),
// the float copies PoseManager caches, and the translation.
struct PoseMats {
    double Rd[9];   // R(r)
    float R[9];     // (float)R(r)      get_rotation_matrix()
    float Ri[9];    // (float)R(-r)     get_inv_rotation_matrix()
    float t[3];
};

__device__ inline void pose_mats(const float pose[6], PoseMats& m) {
    const float r[3] = {pose[3], pose[4], pose[5]};
    rodrigues_d(r, m.Rd);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            m.R[i * 3 + j] = (float)m.Rd[i * 3 + j];
            m.Ri[i * 3 + j] = (float)m.Rd[j * 3 + i];
        }
    m.t[0] = pose[0]; m.t[1] = pose[1]; m.t[2] = pose[2];
}

// Matx33f * Vec3f: s = 0; s += a[k]*v[k]
__device__ inline void mat33f_vec(const float* a, const float v[3], float out[3]) {
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += a[i * 3 + k] * v[k];
        t[i] = s;
    }
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
}

// The kps3d a new keypoint gets (DepthCalculator::calculate_depth, src/lib/depth_calculator.cpp:241-256): the camera
// frame point of the pixel (x, y) with that disparity into loc (loc[2] is the reference's _z), and loc in the world
// frame of a pose. kf_init_kernel (keyframe.hip) and the cloud kernels (cloud.hip) both call these, so the two cannot
// drift.
__device__ inline void kp_triangulate(float x, float y, float disparity, float fx, float fy, float cx, float cy, float baseline,
                                      float loc[3]) {
    const float _z = baseline / fmaxf(0.5f, disparity);
    const float _x = (x - cx) / fx * _z;
    const float _y = (y - cy) / fy * _z;
    loc[0] = _x; loc[1] = _y; loc[2] = _z;
}
__device__ inline svo_kp3d kp_to_world(const PoseMats& pm, const float loc[3]) {
    float w[3];
    mat33f_vec(pm.R, loc, w);
    return svo_kp3d{w[0] + pm.t[0], w[1] + pm.t[1], w[2] + pm.t[2]};
}

// project_keypoints, src/lib/transform_keypoints.cpp:11-48: translate by -t in
// float, then cv::projectPoints(rvec = -r, tvec = 0) in double, float store.
struct CamD {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};
__device__ inline CamD make_camd(float fx, float fy, float cx, float cy, const svo_camera_settings& c) {
    return CamD{(double)fx, (double)fy, (double)cx, (double)cy, (double)c.k1, (double)c.k2,
                (double)c.p1, (double)c.p2, (double)c.k3};
}
__device__ inline svo_kp2d project_point(const double Rd[9], const float t[3], const CamD& c,
                                         const svo_kp3d P) {
    const float Xf = P.x - t[0], Yf = P.y - t[1], Zf = P.z - t[2];
    const double X = Xf, Y = Yf, Z = Zf;
    // rows of R(-r) are columns of R(r)
    double x = Rd[0] * X + Rd[3] * Y + Rd[6] * Z + 0.0;
    double y = Rd[1] * X + Rd[4] * Y + Rd[7] * Z + 0.0;
    double z = Rd[2] * X + Rd[5] * Y + Rd[8] * Z + 0.0;
    z = z ? 1. / z : 1;
    x *= z; y *= z;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = 1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6;
    const double xd = x * cdist + c.p1 * a1 + c.p2 * a2;
    const double yd = y * cdist + c.p1 * a3 + c.p2 * a1;
    svo_kp2d o;
    o.x = (float)(xd * c.fx + c.cx);
    o.y = (float)(yd * c.fy + c.cy);
    return o;
}

// 2x6 Jacobian of src/lib/pose_estimator.cpp:343-344 / pose_refinement.cpp:380-381
__device__ inline void pose_jacobian(float fx, float fy, float x, float y, float z, float J[12]) {
    J[0] = -fx / z;  J[1] = 0;       J[2] = fx * x / (z * z);
    J[3] = fx * x * y / (z * z);     J[4] = -fx * (1 + (x * x) / (z * z)); J[5] = fx * y / z;
    J[6] = 0;        J[7] = -fy / z; J[8] = fy * y / (z * z);
    J[9] = fy * (1 + (y * y) / (z * z)); J[10] = -fy * x * y / (z * z);    J[11] = -fy * x / z;
}

// exponential_map, src/include/exponential_map.hpp:12-37 (norm fixed to 1,
// double scale factors applied to a float matrix).
__device__ inline void exponential_map(const float twist[6], float out[6]) {
    const float v[3] = {twist[0], twist[1], twist[2]};
    const float w[3] = {twist[3], twist[4], twist[5]};
    const float K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    float K2[9], M[9];
    const float norm = 1.0f;
    // 1 - cos(1.0) and 1.0 - sin(1.0) in double (the device math library would not fold them)
    const double c1 = 0x1.d6bafe095f2e8p-2;
    const double c2 = 0x1.44aadc3dbcc48p-3;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += K[i * 3 + k] * K[k * 3 + j];
            K2[i * 3 + j] = s;
        }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const float e = (k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f;
        const float t0 = e * norm;
        const float t1 = (float)(K[k] * c1);
        const float t2 = (float)(K2[k] * c2);
        M[k] = (t0 + t1) + t2;
    }
    float t[3];
    mat33f_vec(M, v, t);
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
    out[3] = w[0]; out[4] = w[1]; out[5] = w[2];
}

// ------------------------------------------------------------- small SVD
// One-sided Jacobi SVD on the rows of At (OpenCV JacobiSVDImpl_<float>):
// float data, double dot products. Reached in the reference through
// Matx66f::inv(DECOMP_SVD) (pose_estimator.cpp:405, pose_refinement.cpp:398),
// cv::solve(DECOMP_SVD) (depth_filter.cpp:200) and cv::KalmanFilter::correct.
template <int M, int N>
__host__ __device__ inline void jacobi_svd(float (&At)[N][M], float (&W)[N], float (&Vt)[N][N]) {
    const float eps = FLT_EPSILON * 2;
    double Wd[N];
    for (int i = 0; i < N; i++) {
        double sd = 0;
        for (int k = 0; k < M; k++) { const float t = At[i][k]; sd += (double)t * t; }
        Wd[i] = sd;
        for (int k = 0; k < N; k++) Vt[i][k] = 0;
        Vt[i][i] = 1;
    }
    const int max_iter = M > 30 ? M : 30;
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                double a = Wd[i], p = 0, b = Wd[j];
                for (int k = 0; k < M; k++) p += (double)At[i][k] * At[j][k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = svo_hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < M; k++) {
                    const float t0 = c * At[i][k] + s * At[j][k];
                    const float t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                Wd[i] = a; Wd[j] = b;
                changed = true;
                for (int k = 0; k < N; k++) {
                    const float t0 = c * Vt[i][k] + s * Vt[j][k];
                    const float t1 = -s * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0; Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; i++) {
        double sd = 0;
        for (int k = 0; k < M; k++) { const float t = At[i][k]; sd += (double)t * t; }
        Wd[i] = sqrt(sd);
    }
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        for (int k = i + 1; k < N; k++)
            if (Wd[j] < Wd[k]) j = k;
        if (i != j) {
            const double tw = Wd[i]; Wd[i] = Wd[j]; Wd[j] = tw;
            for (int k = 0; k < M; k++) { const float t = At[i][k]; At[i][k] = At[j][k]; At[j][k] = t; }
            for (int k = 0; k < N; k++) { const float t = Vt[i][k]; Vt[i][k] = Vt[j][k]; Vt[j][k] = t; }
        }
    }
    for (int i = 0; i < N; i++) {
        W[i] = (float)Wd[i];
        const double sd = Wd[i];
        const float s = (float)(sd > (double)FLT_MIN ? 1 / sd : 0.);
        for (int k = 0; k < M; k++) At[i][k] *= s;
    }
}

// Tail of the 6x6 Jacobi SVDs below, after the sweeps: singular values from the rotated rows,
// selection sort (largest first), rows of At scaled to unit length.
__device__ inline void svd6_finish(float (&At)[6][6], float (&W)[6], float (&Vt)[6][6]) {
    double Wd[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) { const float t = At[i][k]; sd = __builtin_fma((double)t, (double)t, sd); }
        Wd[i] = sqrt(sd);
    }
    // selection sort, largest first: row i <-> the first maximum of rows i..5
#pragma unroll
    for (int i = 0; i < 5; i++) {
        int j = i;
        double wj = Wd[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++)
            if (wj < Wd[k]) { j = k; wj = Wd[k]; }
#pragma unroll
        for (int k = i + 1; k < 6; k++)
            if (j == k) {
                const double tw = Wd[i]; Wd[i] = Wd[k]; Wd[k] = tw;
#pragma unroll
                for (int q = 0; q < 6; q++) { const float t = At[i][q]; At[i][q] = At[k][q]; At[k][q] = t; }
#pragma unroll
                for (int q = 0; q < 6; q++) { const float t = Vt[i][q]; Vt[i][q] = Vt[k][q]; Vt[k][q] = t; }
            }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        W[i] = (float)Wd[i];
        const double sd = Wd[i];
        const float s = (float)(sd > (double)FLT_MIN ? 1 / sd : 0.);
#pragma unroll
        for (int k = 0; k < 6; k++) At[i][k] *= s;
    }
}

// The same one-sided Jacobi SVD for the 6x6 systems of the Gauss-Newton kernels, written so
// that every array index is a compile-time constant (all loops over rows / columns / pairs are
// unrolled, the selection sort swaps under predicates): At, Vt and W live in registers instead of
// scratch memory. Same operations in the same order as jacobi_svd<6,6>: same bits.
// (The product of two floats is exact in double, so fma(x, y, acc) == acc + x * y bit for bit: the
// sums of squares and the dot products below use one instruction per term.)
// Sequential reference of jacobi_svd6_lanes (svo_pinv6_check only); returns the sweeps run.
__device__ inline int jacobi_svd6_reg(float (&At)[6][6], float (&W)[6], float (&Vt)[6][6]) {
    const float eps = FLT_EPSILON * 2;
    double Wd[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) { const float t = At[i][k]; sd = __builtin_fma((double)t, (double)t, sd); }
        Wd[i] = sd;
#pragma unroll
        for (int k = 0; k < 6; k++) Vt[i][k] = (i == k) ? 1.f : 0.f;
    }
    int sweeps = 30;
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 5; i++)
#pragma unroll
            for (int j = i + 1; j < 6; j++) {
                double a = Wd[i], p = 0, b = Wd[j];
#pragma unroll
                for (int k = 0; k < 6; k++) p = __builtin_fma((double)At[i][k], (double)At[j][k], p);
                // |p| <= eps * sqrt(a*b) of the reference, decided without the square root whenever
                // p^2 and eps^2 a b are further apart than any rounding error of either side (1e-9
                // relative, the errors are ~1e-16); the exact expression decides the rest (and NaNs)
                const double pp = p * p, ee = ((double)eps * (double)eps) * (a * b);
                bool rotate = pp > ee * (1 + 1e-9);
                if (!rotate && !(pp < ee * (1 - 1e-9))) rotate = !(fabs(p) <= eps * sqrt(a * b));
                if (rotate) {
                    p *= 2;
                    const double beta = a - b, gamma = svo_hypot(p, beta);
                    // beta < 0: s = sqrt((gamma - beta) / 2 / gamma), c = p / (2 gamma s); else c and s swap
                    // roles with (gamma + beta) / (2 gamma): one square root and one division serve both
                    const bool neg = beta < 0;
                    const double num = neg ? (gamma - beta) * 0.5 : (gamma + beta);
                    const double den = neg ? gamma : gamma * 2;
                    const float r1 = (float)sqrt(num / den);
                    const float r2 = (float)(p / (gamma * r1 * 2));
                    const float c = neg ? r2 : r1, s = neg ? r1 : r2;
                    a = b = 0;
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        const float t0 = c * At[i][k] + s * At[j][k];
                        const float t1 = -s * At[i][k] + c * At[j][k];
                        At[i][k] = t0; At[j][k] = t1;
                        a = __builtin_fma((double)t0, (double)t0, a); b = __builtin_fma((double)t1, (double)t1, b);
                    }
                    Wd[i] = a; Wd[j] = b;
                    changed = true;
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        const float t0 = c * Vt[i][k] + s * Vt[j][k];
                        const float t1 = -s * Vt[i][k] + c * Vt[j][k];
                        Vt[i][k] = t0; Vt[j][k] = t1;
                    }
                }
            }
        if (!changed) { sweeps = iter + 1; break; }
    }
    svd6_finish(At, W, Vt);
    return sweeps;
}

// Schedule of jacobi_svd6_lanes, generated by tools/svd_schedule.py (and checked against it by
// tests/test_svd_schedule_cpu.py). Position q of the 6-round body pairs row r with row
// (kSvdPartner[q] >> 4r) & 7 (itself: idle this round); bit r of kSvdLag[q] marks a pair of the
// previous sweep (t - 1 in body iteration t), the other pairs belong to sweep t.
// SVD-SCHEDULE-BEGIN
constexpr uint32_t kSvdPartner[6] = {0x76234501u, 0x76345012u, 0x76450123u, 0x76501234u, 0x76012345u, 0x76123450u};
constexpr uint32_t kSvdLag[6] = {0x3Cu, 0x28u, 0x30u, 0x00u, 0x00u, 0x00u};
// SVD-SCHEDULE-END

// jacobi_svd6_reg with the rotations of disjoint row pairs in parallel lanes: the same bits out
// for every input, fewer dependent steps. Lane r (r = lane & 7 < 6) owns row r of At and Vt and its
// Wd[r]; lanes with r = 6, 7 idle.
//
// Why the bits are the same. A rotation of rows (i, j) reads and writes only rows i and j of At and
// Vt, Wd[i] and Wd[j], and sets the `changed` flag. Two rotations on disjoint row pairs therefore
// commute exactly, and any order of the pairs that keeps, for every row, the reference's order of
// the pairs touching it (a topological order of the row-dependency graph of the cyclic sweep
// (0,1) (0,2) .. (0,5) (1,2) .. (4,5), sweep after sweep) gives every pair the same operands as the
// sequential loop. kSvdPartner / kSvdLag are that order scheduled as early as possible: sweep t
// runs in positions 1-6 of body iteration t and its last three pairs, (2,5) (3,4) / (3,5) / (4,5),
// in positions 1-3 of iteration t + 1, beside the first pairs of sweep t + 1. 6 rounds per sweep
// instead of 15.
// Within a pair both lanes compute p, the skip test, beta, gamma, c and s with the reference's
// operations on the same operands (a = Wd of the low row, b = Wd of the high row; fma(x, y, acc)
// with an exact product does not depend on the order of x and y), so both decide and round alike.
// The low lane writes c*own + s*partner (the reference's t0), the high lane c*own + (-s)*partner,
// which is the reference's t1 = -s*Ai + c*Aj with the addition commuted (-ffp-contract=off: no fma).
//
// Stopping. Iteration 0 masks its sweep -1 pairs, which leaves sweep 0 scheduled as early as
// possible. After position 3 of iteration t >= 1 sweep t - 1 is complete; the reference stops after
// it if it rotated nothing, and so does this loop. The pairs of sweep t that already ran by then,
// (0,1) (0,2) (0,3) (1,2), include every earlier pair of sweep t on their rows, and they were no-ops:
// sweep t - 1 left every row as it found it, so each of them saw the operands its sweep t - 1 twin
// saw (inductively, in dependency order, the pairs before it having skipped as well) and skipped alike.
// The reference runs at most 30 sweeps (iter < 30): pairs of sweep 30 are masked and the loop stops
// after position 3 of iteration 30. Returns the sweep count of the reference loop.
//
// Precondition: the wave is converged (all 64 lanes active). In: a = row r of At (r = 6, 7: zeros).
// Out: a, v = rows r of the rotated At and of Vt, before the sort and the scaling.
__device__ inline int svd6_sweeps_lanes(float (&a)[6], float (&v)[6]) {
    const float eps = FLT_EPSILON * 2;
    const int lane = (int)__lane_id();
    const int r = lane & 7;
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = (r == k) ? 1.f : 0.f;
    double wd = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) wd = __builtin_fma((double)a[k], (double)a[k], wd);

    // per position: the partner lane's byte address for ds_bpermute, this lane's role, its sweep lag
    int addr[6];
    bool pair[6], low[6], lag[6];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const int pr = (int)((kSvdPartner[q] >> (4 * r)) & 7u);
        addr[q] = ((lane & ~7) | pr) << 2;
        pair[q] = pr != r;
        low[q] = r < pr;
        lag[q] = ((kSvdLag[q] >> r) & 1u) != 0;
    }

    bool chg_prev = false, chg_cur = false;   // rotations of sweep t - 1 / sweep t seen by this lane
    auto round = [&](int q, int t) {
        // the partner's row: 14 dwords fetched in one batch
        float pa[6], pv[6];
#pragma unroll
        for (int k = 0; k < 6; k++) pa[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(addr[q], __float_as_int(a[k])));
#pragma unroll
        for (int k = 0; k < 6; k++) pv[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(addr[q], __float_as_int(v[k])));
        const int wlo = __builtin_amdgcn_ds_bpermute(addr[q], (int)__double2loint(wd));
        const int whi = __builtin_amdgcn_ds_bpermute(addr[q], (int)__double2hiint(wd));
        const double wp = __hiloint2double(whi, wlo);
        const int sweep = t - (lag[q] ? 1 : 0);
        const bool live = pair[q] && sweep >= 0 && sweep < 30;
        double wa = low[q] ? wd : wp, p = 0, wb = low[q] ? wp : wd;
#pragma unroll
        for (int k = 0; k < 6; k++) p = __builtin_fma((double)a[k], (double)pa[k], p);
        const double pp = p * p, ee = ((double)eps * (double)eps) * (wa * wb);
        bool rotate = pp > ee * (1 + 1e-9);
        if (!rotate && !(pp < ee * (1 - 1e-9))) rotate = !(fabs(p) <= eps * sqrt(wa * wb));
        rotate = rotate && live;
        if (rotate) {
            p *= 2;
            const double beta = wa - wb, gamma = svo_hypot(p, beta);
            const bool neg = beta < 0;
            const double num = neg ? (gamma - beta) * 0.5 : (gamma + beta);
            const double den = neg ? gamma : gamma * 2;
            const float r1 = (float)sqrt(num / den);
            const float r2 = (float)(p / (gamma * r1 * 2));
            const float c = neg ? r2 : r1, s = neg ? r1 : r2;
            const float se = low[q] ? s : -s;
            double w = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const float t0 = c * a[k] + se * pa[k];
                a[k] = t0;
                w = __builtin_fma((double)t0, (double)t0, w);
            }
            wd = w;
#pragma unroll
            for (int k = 0; k < 6; k++) v[k] = c * v[k] + se * pv[k];
        }
        if (lag[q]) chg_prev = chg_prev || rotate;
        else chg_cur = chg_cur || rotate;
    };

    int t = 0;
    for (;; t++) {
        round(0, t);
        round(1, t);
        round(2, t);
        if (t == 30 || (t >= 1 && __builtin_amdgcn_ballot_w64(chg_prev) == 0)) break;
        round(3, t);
        round(4, t);
        round(5, t);
        chg_prev = chg_cur;
        chg_cur = false;
    }
    return t;
}

// The round-4 form of the solve's SVD (svo_pinv6_check, svo_solve6_check impl 0 only): the sweeps in
// lanes, then At, W and Vt wave-uniform (v_readlane) through svd6_finish. Precondition: the wave is
// converged and At holds the same values in every lane.
__device__ inline int jacobi_svd6_lanes(float (&At)[6][6], float (&W)[6], float (&Vt)[6][6]) {
    const int r = (int)__lane_id() & 7;
    float a[6], v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        float x = 0.f;
#pragma unroll
        for (int i = 0; i < 6; i++) x = (r == i) ? At[i][k] : x;
        a[k] = x;
    }
    const int t = svd6_sweeps_lanes(a, v);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k < 6; k++) {
            At[i][k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[k]), i));
            Vt[i][k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), i));
        }
    svd6_finish(At, W, Vt);
    return t;
}

// pinv(H) from its SVD (Matx66f::inv(DECOMP_SVD)): V diag(1/w) U^T with the SVBkSb threshold; zeros
// when sigma_max < FLT_EPSILON or sigma_min / sigma_max == 0.
__device__ inline void svd6_pinv(const float (&At)[6][6], const float (&W)[6], const float (&Vt)[6][6],
                                  float Hinv[36]) {
#pragma unroll
    for (int i = 0; i < 36; i++) Hinv[i] = 0;
    double threshold = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) threshold += W[i];
    threshold *= (float)(DBL_EPSILON * 2);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double wi = W[i];
        if (!(fabs(wi) <= threshold)) {
            wi = 1 / wi;
            double buffer[6];
#pragma unroll
            for (int j = 0; j < 6; j++) buffer[j] = At[i][j] * wi;
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const float sv = Vt[i][r];
#pragma unroll
                for (int j = 0; j < 6; j++) Hinv[r * 6 + j] = (float)(Hinv[r * 6 + j] + sv * buffer[j]);
            }
        }
    }
    const bool ok = W[0] >= FLT_EPSILON ? (W[5] / W[0] != 0) : false;
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 36; i++) Hinv[i] = 0;
    }
}

// Per-lane outputs of svd6_tail_lanes for svo_solve6_check: lane L = 6i + j < 36 holds Hinv(i, j),
// U^T(i, j), Vt(i, j) and W[i].
struct Solve6Lane {
    float hinv, ut, vt, w;
};

// What follows the sweeps of the exact solve — svd6_finish, svd6_pinv and delta = Hinv b of the
// round-4 solve (jacobi_svd6_lanes + svd6_pinv + the product in gn_solve6) — with the elements in
// lanes instead of wave-uniform registers. In: a, v from svd6_sweeps_lanes (row r = lane & 7 < 6);
// bf(j) = b[j]. Out: delta wave-uniform. Precondition: the wave is converged.
//
// Why the bits are the same. Every element below is computed by one lane with the reference's
// operations on the reference's operands in the reference's order; only where the operands live changes.
// - Wd: lane r sums its own row's squares (k order, fma with exact products) and takes the square root.
// - The sort: the six Wd are read back wave-uniform and the selection sort runs on them with the
//   reference's compares ("first maximum of rows i..5", the same swaps, ties and NaNs included) while
//   an index array follows the swaps: src[i] is the row that ends at position i. The sort moves rows
//   whole, so sorted row i is unsorted row src[i], element by element.
// - Lane L = 6i + j takes U^T(i, j), Vt(i, j) from row src[i] (one ds_bpermute each, from lane 8j + src[i],
//   which picked element j of its row) and scales U^T(i, j) by the reference's s_i, from Wd sorted.
// - The pseudo-inverse: threshold is the ordered sum of the wave-uniform W. Lane 6i + j holds
//   buffer[j] = U^T(i, j) * (1 / W[i]) of row i, the reference's double. Lane (r, j) runs its own chain
//   Hinv(r, j) = (float)(Hinv(r, j) + Vt(i, r) * buffer[j]) over i = 0..5 in order, taking Vt(i, r) from
//   lane 6i + r and buffer[j] from lane 6i + j, and skips row i under the same wave-uniform test
//   fabs(W[i]) <= threshold. The `ok` test zeroes it as before.
// - The step: lane L forms Hinv(r, j) * b[j] (the product of sacc += Hinv * b, -ffp-contract=off), lane r
//   adds the six products of its row to 0 in j order, and delta[r] is read back wave-uniform.
__device__ inline void svd6_tail_lanes(const float (&a)[6], const float (&v)[6], float b_j, float delta[6],
                                       Solve6Lane* out = nullptr) {
    const int lane = (int)__lane_id();
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) sd = __builtin_fma((double)a[k], (double)a[k], sd);
    const double wr = sqrt(sd);
    double w[6];
    int src[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        w[i] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wr), i),
                                __builtin_amdgcn_readlane(__double2loint(wr), i));
        src[i] = i;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        int j = i;
        double wj = w[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++)
            if (wj < w[k]) { j = k; wj = w[k]; }
#pragma unroll
        for (int k = i + 1; k < 6; k++)
            if (j == k) {
                const double tw = w[i]; w[i] = w[k]; w[k] = tw;
                const int ts = src[i]; src[i] = src[k]; src[k] = ts;
            }
    }
    // lane L = 6i + j (lanes past 35 mirror lane 35)
    const int L = lane < 36 ? lane : 35;
    const int i = L / 6, j = L - 6 * i;
    // (elements picked with bit masks: a chain of selects between the elements of an array is folded into
    // one load at a lane-dependent index, which moves the array to scratch memory)
    int si = 0, wlo = 0, whi = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const int m = -(int)(i == q);
        si |= m & src[q];
        wlo |= m & __double2loint(w[q]);
        whi |= m & __double2hiint(w[q]);
    }
    const double wi = __hiloint2double(whi, wlo);
    // lane 8g + r offers element g of its row r; lane L reads element j of row src[i]
    const int g = lane >> 3;
    int agb = 0, vgb = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int m = -(int)(g == k);
        agb |= m & __float_as_int(a[k]);
        vgb |= m & __float_as_int(v[k]);
    }
    const int from = (8 * j + si) << 2;
    float ut = __int_as_float(__builtin_amdgcn_ds_bpermute(from, agb));
    const float vt = __int_as_float(__builtin_amdgcn_ds_bpermute(from, vgb));
    const float wf = (float)wi;
    const float sc = (float)(wi > (double)FLT_MIN ? 1 / wi : 0.);
    ut *= sc;

    float W[6];
#pragma unroll
    for (int q = 0; q < 6; q++) W[q] = (float)w[q];
    double threshold = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) threshold += W[q];
    threshold *= (float)(DBL_EPSILON * 2);
    const double buf = ut * (1 / (double)wf);
    const int blo = __double2loint(buf), bhi = __double2hiint(buf);
    float h = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const int fb = (6 * q + j) << 2, fv = (6 * q + i) << 2;
        const double bq = __hiloint2double(__builtin_amdgcn_ds_bpermute(fb, bhi), __builtin_amdgcn_ds_bpermute(fb, blo));
        const float sv = __int_as_float(__builtin_amdgcn_ds_bpermute(fv, __float_as_int(vt)));
        const double wq = W[q];
        if (!(fabs(wq) <= threshold)) h = (float)(h + sv * bq);
    }
    const bool ok = W[0] >= FLT_EPSILON ? (W[5] / W[0] != 0) : false;
    if (!ok) h = 0;
    if (out) *out = Solve6Lane{h, ut, vt, wf};

    const float p = h * b_j;
    const int rr = lane < 6 ? lane : 0;
    float sacc = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) sacc += __int_as_float(__builtin_amdgcn_ds_bpermute((6 * rr + c) << 2, __float_as_int(p)));
#pragma unroll
    for (int q = 0; q < 6; q++) delta[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sacc), q));
}

// Index of H(r, c), r <= c, among the 21 upper-triangle sums (row-major, as the accumulators store them).
__device__ inline int h6_tri(int r, int c) { return r * (11 - r) / 2 + c; }

// The exact solve delta = pinv(H) b straight from the accumulators: sums[0..20] the upper triangle of the
// symmetric H, sums[21..26] b (LDS). Lane r = lane & 7 < 6 reads row r of H (= row r of At), lane L < 36
// b[L % 6]; no wave-uniform H. Precondition: the wave is converged. Returns the sweeps run.
__device__ inline int gn_solve6_sums(const SVO_LDS(float)* sums, float delta[6]) {
    const int lane = (int)__lane_id();
    const int r = lane & 7;
    float a[6], v[6];
#pragma unroll
    for (int k = 0; k < 6; k++) a[k] = r < 6 ? sums[h6_tri(min(r, k), max(r, k))] : 0.f;
    const float b_j = sums[21 + (lane < 36 ? lane : 35) % 6];
    const int sw = svd6_sweeps_lanes(a, v);
    svd6_tail_lanes(a, v, b_j, delta);
    return sw;
}

// delta = pinv(H) b for the Gauss-Newton steps (pose_estimator.cpp:405,484;
// pose_refinement.cpp:398-399). Fast path: when H is comfortably positive
// definite its pseudo-inverse is its inverse, so H delta = b is solved by an
// LDL^T factorisation in double (~150 flops on one lane instead of a Jacobi
// SVD). Anything else (a pivot below 1e-6 of the largest diagonal entry, i.e.
// rank deficient at float precision, or H = 0) takes the SVD route of the
// reference, which is also what `exact` forces for every call.
__device__ inline void gn_solve6(const float H[36], const float b[6], float delta[6], bool exact) {
    bool ok = !exact;
    if (ok) {
        double L[6][6], D[6], dmax = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) dmax = fmax(dmax, (double)H[i * 6 + i]);
        const double tiny = dmax * 1e-6;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double d = H[j * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
            if (!(d > tiny) || !(dmax > 0)) ok = false;
            D[j] = d;
            const double id = 1.0 / d;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double v = H[i * 6 + j];
#pragma unroll
                for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
                L[i][j] = v * id;
            }
        }
        if (ok) {
            double z[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double v = b[i];
#pragma unroll
                for (int k = 0; k < i; k++) v -= L[i][k] * z[k];
                z[i] = v;
            }
#pragma unroll
            for (int i = 0; i < 6; i++) z[i] /= D[i];
#pragma unroll
            for (int i = 5; i >= 0; i--) {
                double v = z[i];
#pragma unroll
                for (int k = i + 1; k < 6; k++) v -= L[k][i] * z[k];
                z[i] = v;
                delta[i] = (float)v;
            }
            return;
        }
    }
    // the exact solve in lanes: lane r takes row r of At = H^T, lane L < 36 b[L % 6] (bit masks: see
    // svd6_tail_lanes)
    const int lane = (int)__lane_id();
    const int r = lane & 7, jb = (lane < 36 ? lane : 35) % 6;
    float a[6], v[6];
    int bb = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int x = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) x |= -(int)(r == i) & __float_as_int(H[k * 6 + i]);
        a[k] = __int_as_float(x);
        bb |= -(int)(jb == k) & __float_as_int(b[k]);
    }
    const float b_j = __int_as_float(bb);
    svd6_sweeps_lanes(a, v);
    svd6_tail_lanes(a, v, b_j, delta);
}

// cv::solve(A[3x2], b, x, DECOMP_SVD), src/lib/depth_filter.cpp:194-200
__device__ inline void solve_svd_3x2(const float A[6], const float b[3], float x[2]) {
    float At[2][3], Vt[2][2], W[2];
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) At[i][j] = A[j * 2 + i];
    jacobi_svd<3, 2>(At, W, Vt);
    x[0] = x[1] = 0;
    double threshold = ((double)W[0] + (double)W[1]) * (float)(DBL_EPSILON * 2);
    for (int i = 0; i < 2; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < 3; j++) s += At[i][j] * b[j];
        s *= wi;
        for (int j = 0; j < 2; j++) x[j] = (float)(x[j] + s * Vt[i][j]);
    }
}

// 1-state cv::KalmanFilter predict()+correct(meas) with A = H = 1
// (src/lib/depth_filter.cpp:202-215); gain through the 1x1 SVD solve.
__device__ inline void kf1_update(float& x, float& P, float Q, float R, float meas) {
    const float statePre = (float)((double)1.0f * (double)x);
    const float temp1 = (float)((double)1.0f * (double)P);
    const float errorCovPre = (float)((double)temp1 * (double)1.0f + (double)Q);
    const float temp2 = (float)((double)1.0f * (double)errorCovPre);
    const float temp3 = (float)((double)temp2 * (double)1.0f + (double)R);
    // 1x1 Jacobi SVD: w = |a|, u = a * (float)(1/w), v = 1
    float gain = 0;
    {
        const double sd = sqrt((double)temp3 * temp3);
        const float w = (float)sd;
        const float u = temp3 * (float)(sd > (double)FLT_MIN ? 1 / sd : 0.);
        const double threshold = (double)w * (float)(DBL_EPSILON * 2);
        if (!(fabs((double)w) <= threshold)) {
            const double wi = 1 / (double)w;
            double s = 0;
            s += u * temp2;
            s *= wi;
            gain = (float)(0.0f + s * 1.0f);
        }
    }
    const float temp5 = meas - (float)((double)1.0f * (double)statePre);
    x = (float)((double)gain * (double)temp5 + (double)statePre);
    P = (float)(-((double)gain * (double)temp2) + (double)errorCovPre);
}

// get_patch_sum, src/lib/pose_estimator.cpp:82-112 (3x3 taps = area sum of a
// 2x2 box centred at `c`; callers guard the bounds)
__device__ inline float patch_sum(const uint8_t* img, int stride, float cx, float cy) {
    const float sx = cx - 0.5f, sy = cy - 0.5f;
    const float fx_ = floorf(sx), fy_ = floorf(sy);
    const int ipx = (int)fx_, ipy = (int)fy_;
    const float x2 = sx - (float)ipx, y2 = sy - (float)ipy;
    const float x1 = 1.0f - x2, y1 = 1.0f - y2;
    const uint8_t* s1 = img + (long)ipy * stride + ipx;
    const uint8_t* s2 = s1 + stride;
    const uint8_t* s3 = s2 + stride;
    const float intensity = x1 * y1 * (float)s1[0] + y1 * (float)s1[1] + x2 * y1 * (float)s1[2] +
                            x1 * (float)s2[0] + (float)s2[1] + x2 * (float)s2[2] +
                            x1 * y2 * (float)s3[0] + y2 * (float)s3[1] + x2 * y2 * (float)s3[2];
    return intensity;
}

__device__ inline int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

}  // namespace svo
