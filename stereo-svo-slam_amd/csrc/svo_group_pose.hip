// svo_group_pose.hip — the batched pose-filter updates of a sequence group (svo_submit_pose_updates): the filters of
// its named slots go up, run all their samples in one launch of pose_filter.hip's kernel and come back into
// Seq::kf. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

// where the arrays of one job lie: the upload block (samples first: they hold doubles) and the download block
struct PoseLayout {
    size_t samples = 0, state_in, start, first, up_bytes;
    size_t state_out = 0, filtered, down_bytes;
    PoseLayout(int n, int total) {
        state_in = sizeof(svo_pose_sample) * (size_t)total;
        start = state_in + sizeof(float) * POSE_FILTER_IN_FLOATS * (size_t)n;
        first = start + sizeof(float) * 6 * (size_t)n;
        up_bytes = first + sizeof(int) * ((size_t)n + 1);
        filtered = sizeof(float) * POSE_FILTER_OUT_FLOATS * (size_t)n;
        down_bytes = filtered + sizeof(float) * 6 * (size_t)total;
    }
};

// the job's blocks hold up_bytes / down_bytes (pinned and device); grown ones replace the old
int reserve_pose_blocks(svo_group* c, size_t up_bytes, size_t down_bytes) {
    if (up_bytes <= c->pose_up_bytes && down_bytes <= c->pose_down_bytes) return SVO_OK;
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    up_bytes = std::max(align_up(up_bytes, 256), c->pose_up_bytes);
    down_bytes = std::max(align_up(down_bytes, 256), c->pose_down_bytes);
    if (c->d_pose) dev_release(c, c->d_pose, c->pose_up_bytes + c->pose_down_bytes);
    c->d_pose = nullptr; c->pose_up_bytes = c->pose_down_bytes = 0;
    c->pose_host.reset();
    HIP_TRY(pinned_malloc(c->pose_host, up_bytes + down_bytes));
    if (const int rc = dev_alloc(c, &c->d_pose, up_bytes + down_bytes, false)) return rc;
    c->pose_up_bytes = up_bytes; c->pose_down_bytes = down_bytes;
    return SVO_OK;
}

// The kernel multiplies out only what the ctor's pattern leaves of A, Hm, Q and R (pose_filter.hip). Every filter
// the tracker makes has it; a snapshot's host part could carry another.
bool has_ctor_pattern(const PoseFilter& kf) {
    constexpr int N = PoseFilter::N;
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            const int e = i * N + j;
            const bool dt = i < 6 && j == 6 + i;          // (set by every update)
            if (!dt && kf.A[e] != (i == j ? 1.f : 0.f)) return false;
            if (kf.Hm[e] != (i == j ? 1.f : 0.f) || kf.Q[e] != (i == j ? 100.f : 0.f)) return false;
            if (i != j && kf.R[e] != 0.f) return false;
        }
    return true;
}

}  // namespace

// The group's share of an svo_submit_pose_updates: counts[i] > 0 samples for slot seqs[i] (index in the group), the
// samples in that order; filtered[i]: where the slot's filtered poses go (host memory), or null. One upload, one
// launch, one download; delivered on return.
int grp_pose_updates(svo_group* c, const int* seqs, const int* counts, int n, const svo_pose_sample* samples,
                     float* const* filtered) {
    if (const int rc = reject_if_failed(c, "svo_submit_pose_updates")) return rc;
    if (n <= 0) return SVO_OK;
    HIP_TRY(hipSetDevice(c->device));
    flush_pending(c);
    int total = 0;
    for (int i = 0; i < n; i++) total += counts[i];
    const PoseLayout lay(n, total);
    if (const int rc = reserve_pose_blocks(c, lay.up_bytes, lay.down_bytes)) return rc;
    uint8_t* hu = c->pose_host.get();
    uint8_t* hd = hu + c->pose_up_bytes;
    uint8_t* du = c->d_pose;
    uint8_t* dd = du + c->pose_up_bytes;
    std::memcpy(hu + lay.samples, samples, sizeof(svo_pose_sample) * (size_t)total);
    float* state_in = reinterpret_cast<float*>(hu + lay.state_in);
    float* start = reinterpret_cast<float*>(hu + lay.start);
    int* first = reinterpret_cast<int*>(hu + lay.first);
    first[0] = 0;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        if (!has_ctor_pattern(q.kf))
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: the filter of slot %d (index in its group) does not have the tracker's A, H, Q and R pattern", seqs[i]);
        std::memcpy(state_in + (size_t)i * POSE_FILTER_IN_FLOATS, q.kf.statePost, sizeof(q.kf.statePost));
        std::memcpy(state_in + (size_t)i * POSE_FILTER_IN_FLOATS + PoseFilter::N, q.kf.errorCovPost, sizeof(q.kf.errorCovPost));
        std::memcpy(start + (size_t)i * 6, q.pose, sizeof(q.pose));
        first[i + 1] = first[i] + counts[i];
    }
    hipStream_t st = c->stream.get();
    HIP_TRY(hipMemcpyAsync(du, hu, lay.up_bytes, hipMemcpyHostToDevice, st));
    PoseFilterArgs a;
    a.n_states = n; a.n_samples = total;
    a.samples = reinterpret_cast<const svo_pose_sample*>(du + lay.samples);
    a.state_in = reinterpret_cast<const float*>(du + lay.state_in);
    a.start_pose = reinterpret_cast<const float*>(du + lay.start);
    a.first = reinterpret_cast<const int*>(du + lay.first);
    a.state_out = reinterpret_cast<float*>(dd + lay.state_out);
    a.filtered = reinterpret_cast<float*>(dd + lay.filtered);
    launch_pose_filter(a, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hd, dd, lay.down_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    const float* out = reinterpret_cast<const float*>(hd + lay.state_out);
    const float* fl = reinterpret_cast<const float*>(hd + lay.filtered);
    for (int i = 0; i < n; i++, out += POSE_FILTER_OUT_FLOATS) {
        PoseFilter& kf = c->seqs[seqs[i]].kf;
        constexpr int N = PoseFilter::N, NN = N * N;
        std::memcpy(kf.statePre, out, sizeof(kf.statePre));
        std::memcpy(kf.statePost, out + N, sizeof(kf.statePost));
        std::memcpy(kf.errorCovPre, out + 2 * N, sizeof(kf.errorCovPre));
        std::memcpy(kf.errorCovPost, out + 2 * N + NN, sizeof(kf.errorCovPost));
        std::memcpy(kf.gain, out + 2 * N + 2 * NN, sizeof(kf.gain));
        // what the host loop leaves in A and R: the last sample's time step and variances
        const svo_pose_sample& last = samples[first[i + 1] - 1];
        for (int k = 0; k < 6; k++) {
            kf.A[k * N + 6 + k] = (float)last.dt;
            kf.R[k * N + k] = last.pose_var[k];
            kf.R[(6 + k) * N + 6 + k] = last.speed_var[k];
        }
        if (filtered[i]) std::memcpy(filtered[i], fl + (size_t)first[i] * 6, sizeof(float) * 6 * (size_t)counts[i]);
    }
    return SVO_OK;
}
