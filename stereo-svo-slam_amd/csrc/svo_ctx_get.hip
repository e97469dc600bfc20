// svo_ctx_get.hip — the per-sequence getters of the C ABI. Each one starts at ctx_seq (svo_ctx_state.hpp): the queues
// have drained, so the group's state (svo_group_state.hpp) is read directly, between two steps.
#include <algorithm>
#include <cstring>

#include "svo_ctx_state.hpp"
#include "svo_group_state.hpp"

static int fetch_info(int n, const svo::KpsDev& k, svo_kp2d* kps2d, svo_kp3d* kps3d, svo_kp_info* info) {
    if (n <= 0) return SVO_OK;
    if (kps2d) HIP_TRY(hipMemcpy(kps2d, k.kps2d, sizeof(svo_kp2d) * n, hipMemcpyDeviceToHost));
    if (kps3d) HIP_TRY(hipMemcpy(kps3d, k.kps3d, sizeof(svo_kp3d) * n, hipMemcpyDeviceToHost));
    if (!info) return SVO_OK;
    std::vector<uint32_t> fl(n), col(n);
    std::vector<int> kf(n), ki(n), ou(n), in(n), lt(n);
    std::vector<float> kx(n), kP(n), sc(n);
    const struct { void* dst; const void* src; } arrays[] = {
        {fl.data(), k.flags}, {ou.data(), k.outl}, {in.data(), k.inl}, {kf.data(), k.kf_id}, {ki.data(), k.kp_index},
        {kx.data(), k.kfx}, {kP.data(), k.kfP}, {sc.data(), k.score}, {lt.data(), k.level_type}, {col.data(), k.color}};
    for (const auto& a : arrays) HIP_TRY(hipMemcpy(a.dst, a.src, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));   // (all 4-byte)
    for (int i = 0; i < n; i++) {
        svo_kp_info& o = svo::clear(info[i]);
        o.score = sc[i]; o.level = lt[i] & 0xff; o.type = (lt[i] >> 8) & 0xff;
        o.keyframe_id = kf[i]; o.keypoint_index = ki[i];
        o.color[0] = col[i] & 0xff; o.color[1] = (col[i] >> 8) & 0xff; o.color[2] = (col[i] >> 16) & 0xff;
        o.ignore_during_refinement = (fl[i] & SVO_IGNORE_DURING_REFINEMENT) != 0;
        o.ignore_completely = (fl[i] & SVO_IGNORE_COMPLETELY) != 0;
        o.ignore_temporary = (fl[i] & SVO_IGNORE_TEMPORARY) != 0;
        o.outlier_count = ou[i]; o.inlier_count = in[i];
        o.kf_inv_depth = kx[i]; o.kf_variance = kP[i];
    }
    return SVO_OK;
}

extern "C" int svo_get_pose(svo_ctx* ctx, int seq, float pose[6]) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    svo::flush_pending(c);
    std::memcpy(pose, c->seqs[s].pose, sizeof(float) * 6);
    return SVO_OK;
}

extern "C" int svo_get_frame_keypoints(svo_ctx* ctx, int seq, svo_kp2d* kps2d, svo_kp3d* kps3d,
                                       svo_kp_info* info, int cap, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    const svo::Seq& q = c->seqs[s];
    if (n) *n = q.n_host;
    return fetch_info(std::min(cap, q.n_host), q.kps[q.cur], kps2d, kps3d, info);
}

extern "C" int svo_get_keyframe_count(svo_ctx* ctx, int seq, int* count) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    if (count) *count = (int)c->seqs[s].kfs.size();
    return SVO_OK;
}

extern "C" int svo_get_keyframe(svo_ctx* ctx, int seq, int id, svo_kp2d* kps2d, svo_kp3d* kps3d,
                                svo_kp_info* info, float pose[6], int cap, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    const svo::Seq& q = c->seqs[s];
    if (id < 0 || id >= (int)q.kfs.size()) return svo_set_error(SVO_ERR_INVALID, "keyframe %d does not exist", id);
    if (id < q.kfs.first()) return svo_set_error(SVO_ERR_INVALID, "keyframe %d was trimmed", id);
    const svo::KfHost& k = q.kfs[id];
    if (n) *n = k.n;
    if (pose) std::memcpy(pose, k.pose, sizeof(float) * 6);
    return fetch_info(std::min(cap, k.n), k.kps, kps2d, kps3d, info);
}

extern "C" int svo_get_trajectory(svo_ctx* ctx, int seq, svo_pose* out, int cap, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    svo::flush_pending(c);
    const svo::Seq& q = c->seqs[s];
    if (n) *n = (int)q.trajectory.size();
    const int m = std::min<int>(cap, (int)q.trajectory.size());
    if (out && m > 0) std::memcpy(out, q.trajectory.data(), sizeof(svo_pose) * m);
    return SVO_OK;
}

extern "C" int svo_update_pose(svo_ctx* ctx, int seq, const float pose[6], const float speed[6],
                               const float pose_var[6], const float speed_var[6], double dt,
                               float filtered[6]) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    svo::flush_pending(c);
    c->seqs[s].kf.update(pose, speed, pose_var, speed_var, dt, filtered);
    return SVO_OK;
}

extern "C" int svo_get_frame_stats(svo_ctx* ctx, int seq, svo_frame_stats* out) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    if (out) *out = c->seqs[s].stats;
    return SVO_OK;
}

extern "C" int svo_get_finished_runs(svo_ctx* ctx, int seq, int* n) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    if (n) *n = (int)std::count_if(c->finished.begin(), c->finished.end(), [s](const svo::FinishedRun& f) { return f.info.seq == s; });
    return SVO_OK;
}

extern "C" int svo_get_finished_run(svo_ctx* ctx, int seq, int i, svo_run_info* info, svo_pose* trajectory,
                                    int cap, int* n_poses) {
    svo_group* c; int s;
    if (const int rc = ctx_seq(ctx, seq, &c, &s)) return rc;
    int k = 0;
    for (const svo::FinishedRun& f : c->finished) {
        if (f.info.seq != s || k++ != i) continue;
        if (info) { *info = f.info; info->seq = seq; }
        if (n_poses) *n_poses = (int)f.trajectory.size();
        const int m = std::min<int>(cap, (int)f.trajectory.size());
        if (trajectory && m > 0) std::memcpy(trajectory, f.trajectory.data(), sizeof(svo_pose) * m);
        return SVO_OK;
    }
    return svo_set_error(SVO_ERR_INVALID, "sequence %d has no finished run %d", seq, i);
}
