// pose_filter.hip — the 12-state pose filter of many slots in one launch (svo_submit_pose_updates,
// svo_pose_filter_batch): every sample is one StereoSlam::update_pose (src/lib/stereo_slam.cpp:296-359), the samples
// of a state run in order, the states are independent. The yardstick is the host's PoseFilter::update
// (svo_group_state.hpp): for finite inputs every output bit is its bit.
//
// Mapping: one lane per state, one wavefront per workgroup. All matrices of a lane live in LDS, element e of lane l
// at [e][l] (a dword per lane and element: no bank conflicts, no dynamically indexed register arrays, so no scratch):
// four 12x12 float matrices, the two state vectors and the Jacobi loop's squared row norms, 159,744 bytes of the CU's
// 163,840. The Jacobi SVD is jacobi_svd<12,12> (svo_device.hpp) statement by statement: 66 row pairs per sweep in
// the cyclic order, at most 30 sweeps, so the kernel terminates on any input (non-finite inputs: values unspecified).
// Lanes diverge on the rotation's skip branch and on the sweep count; the loops' trip counts are uniform.
//
// Products that PoseFilter::gemm multiplies out and this kernel skips. A, Hm and Q of a PoseFilter are the ctor's
// pattern (A = I + dt on the diagonal of the upper right 6x6 block, Hm = I, Q = 100 I), R is diagonal. gemm sums
// s = 0; s += (double)a * (double)b for p = 0..11; s *= alpha; s += c * beta; (float)s. Two facts carry every skip:
//   (1) s starts as +0 and a sum of doubles is -0 only when both terms are -0, so s is never -0 after an addition;
//       a term whose factor is a structural zero is +-0 for finite inputs, and adding +-0 to an s that is not -0
//       leaves s as it is. Such terms are dropped, the others keep their order in p.
//   (2) a factor 1 is exact: (double)1 * (double)b == (double)b, s * 1.0 == s, c * 1.0 == c; alpha = -1 is a
//       negation, written as such a product.
// What is left per element:
//   A * x, A * P        : (0.0 + b[i]) and, for rows 0..5, + (double)dt * b[6+i]            (the leading 0.0 + stays:
//   (A P) * At + Q      : (0.0 + t[i][j]) and, for columns 0..5, + t[i][6+j] * dt;           it turns -0 into +0)
//                         + 100.0 on the diagonal (off it, c * beta is +0: dropped by (1))
//   Hm * P, Hm * x      : (float)(0.0 + b[i][j])                                             (temp2, hx)
//   temp2 * Hmt + R     : (0.0 + temp2[i][j]), + (double)R[i][i] on the diagonal
//   gain * temp5 + x, -(gain * temp2) + P : all twelve products, as written.
// solve_svd and jacobi_svd skip nothing.
#include <hip/hip_runtime.h>

#include <float.h>

#include "svo_tracker.hpp"

namespace svo {

namespace {

constexpr int PN = 12;                 // states of the filter
constexpr int PL = POSE_FILTER_LANES;  // lanes (= filter states) of a workgroup

struct PfLds {
    double Wd[PN][PL];                 // jacobi: squared row norms, then the singular values (as float values)
    float At[PN * PN][PL];             // errorCovPost between two samples; the solve's At
    float Vt[PN * PN][PL];
    float P[PN * PN][PL];              // errorCovPre
    float X[PN * PN][PL];              // temp1 of predict; the solve's X = gain transposed
    float x[PN][PL], xp[PN][PL];       // statePost, statePre
};
static_assert(sizeof(PfLds) == 159744, "the layout the file's header states");

// the value gemm gives an element that only a factor 1 reaches: -0 becomes +0
__device__ inline float canon(float v) { return (float)(0.0 + (double)v); }

// jacobi_svd<12, 12> on lane l's At / Vt; W goes to Wd as float values
__device__ inline void jacobi12(PfLds& s, const int l) {
#define AT(i, k) s.At[(i) * PN + (k)][l]
#define VT(i, k) s.Vt[(i) * PN + (k)][l]
    const float eps = FLT_EPSILON * 2;
    for (int i = 0; i < PN; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < PN; k++) { const float t = AT(i, k); sd += (double)t * t; }
        s.Wd[i][l] = sd;
#pragma unroll
        for (int k = 0; k < PN; k++) VT(i, k) = 0;
        VT(i, i) = 1;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < PN - 1; i++)
            for (int j = i + 1; j < PN; j++) {
                double a = s.Wd[i][l], p = 0, b = s.Wd[j][l];
                float ri[PN], rj[PN];
#pragma unroll
                for (int k = 0; k < PN; k++) { ri[k] = AT(i, k); rj[k] = AT(j, k); }
#pragma unroll
                for (int k = 0; k < PN; k++) p += (double)ri[k] * rj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = svo_hypot(p, beta);
                float c, sn;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    sn = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * sn * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    sn = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < PN; k++) {
                    const float t0 = c * ri[k] + sn * rj[k];
                    const float t1 = -sn * ri[k] + c * rj[k];
                    AT(i, k) = t0; AT(j, k) = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                s.Wd[i][l] = a; s.Wd[j][l] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < PN; k++) {
                    const float vi = VT(i, k), vj = VT(j, k);
                    const float t0 = c * vi + sn * vj;
                    const float t1 = -sn * vi + c * vj;
                    VT(i, k) = t0; VT(j, k) = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < PN; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < PN; k++) { const float t = AT(i, k); sd += (double)t * t; }
        s.Wd[i][l] = sqrt(sd);
    }
    for (int i = 0; i < PN - 1; i++) {
        int j = i;
        for (int k = i + 1; k < PN; k++)
            if (s.Wd[j][l] < s.Wd[k][l]) j = k;
        if (i != j) {
            const double tw = s.Wd[i][l]; s.Wd[i][l] = s.Wd[j][l]; s.Wd[j][l] = tw;
            for (int k = 0; k < PN; k++) { const float t = AT(i, k); AT(i, k) = AT(j, k); AT(j, k) = t; }
            for (int k = 0; k < PN; k++) { const float t = VT(i, k); VT(i, k) = VT(j, k); VT(j, k) = t; }
        }
    }
    for (int i = 0; i < PN; i++) {
        const double sd = s.Wd[i][l];
        s.Wd[i][l] = (double)(float)sd;                       // W[i]
        const float sc = (float)(sd > (double)FLT_MIN ? 1 / sd : 0.);
#pragma unroll
        for (int k = 0; k < PN; k++) AT(i, k) *= sc;
    }
}

__global__ __launch_bounds__(PL) void pose_filter_kernel(const PoseFilterArgs a) {
    __shared__ PfLds s;
    const int l = threadIdx.x;
    const int b = blockIdx.x * PL + l;
    if (b >= a.n_states) return;                              // (no barrier below: a lane is on its own)
    const int k0 = max(a.first[b], 0), k1 = min(a.first[b + 1], a.n_samples);
    if (k1 <= k0) return;                                     // no sample: the state's outputs stay as they are
    const float* in = a.state_in + (size_t)b * POSE_FILTER_IN_FLOATS;
    for (int i = 0; i < PN; i++) s.x[i][l] = in[i];
    for (int e = 0; e < PN * PN; e++) s.At[e][l] = in[PN + e];
    float prev[6];                                            // what a chained sample measures
#pragma unroll
    for (int i = 0; i < 6; i++) prev[i] = a.start_pose[(size_t)b * 6 + i];

    for (int k = k0; k < k1; k++) {
        const svo_pose_sample& sm = a.samples[k];
        const float dtf = (float)sm.dt;                       // A[i][6+i]
        const bool chain = (sm.flags & SVO_POSE_SAMPLE_CHAIN) != 0;
        // ---- predict: statePre = A statePost; errorCovPre = A errorCovPost At + Q
        for (int i = 0; i < PN; i++) {
            double acc = 0.0 + (double)s.x[i][l];
            if (i < 6) acc += (double)dtf * (double)s.x[6 + i][l];
            s.xp[i][l] = (float)acc;
        }
        for (int i = 0; i < PN; i++)
            for (int j = 0; j < PN; j++) {                    // temp1 = A errorCovPost
                double acc = 0.0 + (double)s.At[i * PN + j][l];
                if (i < 6) acc += (double)dtf * (double)s.At[(6 + i) * PN + j][l];
                s.X[i * PN + j][l] = (float)acc;
            }
        for (int i = 0; i < PN; i++)
            for (int j = 0; j < PN; j++) {
                double acc = 0.0 + (double)s.X[i * PN + j][l];
                if (j < 6) acc += (double)s.X[i * PN + 6 + j][l] * (double)dtf;
                if (i == j) acc += 100.0;
                s.P[i * PN + j][l] = (float)acc;
            }
        // ---- correct: temp2 = canon(errorCovPre); temp3 = temp2 + R; its transpose is the solve's At
        for (int i = 0; i < PN; i++)
            for (int j = 0; j < PN; j++) {
                double acc = 0.0 + (double)canon(s.P[i * PN + j][l]);
                if (i == j) acc += (double)(i < 6 ? sm.pose_var[i] : sm.speed_var[i - 6]);
                s.At[j * PN + i][l] = (float)acc;
            }
        jacobi12(s, l);
        // ---- solve_svd(temp3, temp2) -> X (temp4); gain = X transposed
        for (int e = 0; e < PN * PN; e++) s.X[e][l] = 0;
        double threshold = 0;
        for (int i = 0; i < PN; i++) threshold += s.Wd[i][l];
        threshold *= (float)(DBL_EPSILON * 2);
        for (int i = 0; i < PN; i++) {
            double wi = s.Wd[i][l];
            if (fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            double buffer[PN];
#pragma unroll
            for (int j = 0; j < PN; j++) buffer[j] = 0;
            for (int r = 0; r < PN; r++) {
                const float sv = s.At[i * PN + r][l];
#pragma unroll
                for (int j = 0; j < PN; j++) buffer[j] = buffer[j] + (double)(sv * canon(s.P[r * PN + j][l]));
            }
#pragma unroll
            for (int j = 0; j < PN; j++) buffer[j] *= wi;
            for (int r = 0; r < PN; r++) {
                const float sv = s.Vt[i * PN + r][l];
#pragma unroll
                for (int j = 0; j < PN; j++) s.X[r * PN + j][l] = (float)(s.X[r * PN + j][l] + sv * buffer[j]);
            }
        }
        // ---- statePost = gain (z - Hm statePre) + statePre
        float t5[PN];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            t5[i] = (chain ? prev[i] : sm.pose[i]) - canon(s.xp[i][l]);
            t5[6 + i] = sm.speed[i] - canon(s.xp[6 + i][l]);
        }
        for (int i = 0; i < PN; i++) {
            double acc = 0;
#pragma unroll
            for (int p = 0; p < PN; p++) acc += (double)s.X[p * PN + i][l] * (double)t5[p];
            acc *= 1.0;
            acc += (double)s.xp[i][l] * 1.0;
            s.x[i][l] = (float)acc;
        }
        // ---- errorCovPost = -(gain temp2) + errorCovPre (into At: the solve is done with it)
        for (int i = 0; i < PN; i++) {
            float g[PN];
#pragma unroll
            for (int p = 0; p < PN; p++) g[p] = s.X[p * PN + i][l];
            for (int j = 0; j < PN; j++) {
                double acc = 0;
#pragma unroll
                for (int p = 0; p < PN; p++) acc += (double)g[p] * (double)canon(s.P[p * PN + j][l]);
                acc *= -1.0;
                acc += (double)s.P[i * PN + j][l] * 1.0;
                s.At[i * PN + j][l] = (float)acc;
            }
        }
        if (a.filtered)
#pragma unroll
            for (int i = 0; i < 6; i++) a.filtered[(size_t)k * 6 + i] = s.x[i][l];
#pragma unroll
        for (int i = 0; i < 6; i++) prev[i] = s.x[i][l];
    }

    float* out = a.state_out + (size_t)b * POSE_FILTER_OUT_FLOATS;      // statePre | statePost | errorCovPre | errorCovPost | gain
    for (int i = 0; i < PN; i++) { out[i] = s.xp[i][l]; out[PN + i] = s.x[i][l]; }
    out += 2 * PN;
    for (int e = 0; e < PN * PN; e++) { out[e] = s.P[e][l]; out[PN * PN + e] = s.At[e][l]; }
    out += 2 * PN * PN;
    for (int i = 0; i < PN; i++)
        for (int j = 0; j < PN; j++) out[i * PN + j] = s.X[j * PN + i][l];
#undef AT
#undef VT
}

}  // namespace

void launch_pose_filter(const PoseFilterArgs& a, hipStream_t stream) {
    if (a.n_states <= 0) return;
    hipLaunchKernelGGL(pose_filter_kernel, dim3((a.n_states + PL - 1) / PL), dim3(PL), 0, stream, a);
}

}  // namespace svo
