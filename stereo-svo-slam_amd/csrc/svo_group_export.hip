// svo_group_export.hip — the bulk export of a sequence group (svo_submit_export): the frames or newest keyframes
// of its named slots as segments and records, packed by export.hip's kernel, and svo_export_capacity. The state is
// svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

extern "C" int svo_export_capacity(const svo_camera_settings* cam, int width, int height, int* records_per_sequence) {
    if (!records_per_sequence) return svo_set_error(SVO_ERR_INVALID, "svo_export_capacity: bad arguments");
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    *records_per_sequence = keypoint_capacity(*cam, width, height);
    return SVO_OK;
}

int grp_capacity(const svo_group* c) { return c->cap; }

// The named slots of the group as segments and records (svo_submit_export). The counts are the host's own
// (Seq::n_host, KfHost::n), so the tile table is built here (group_tile_table: in the group's argument blocks, one
// launch unless it outgrows them). Host mode packs into the staging block and copies the used prefix of each
// array out.
int grp_export(svo_group* c, int what, int mem, const int* seqs, const int* seg, int n, int seq0, int64_t base,
               const svo_export_dst* dst) {
    if (const int rc = job_begin(c, "svo_submit_export")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    svo_kp2d* o2 = dst->kps2d ? dst->kps2d + base : nullptr;
    svo_kp3d* o3 = dst->kps3d ? dst->kps3d + base : nullptr;
    svo_kp_info* oi = dst->info ? dst->info + base : nullptr;
    const bool any = o2 || o3 || oi;
    if (host && any) {
        const size_t records = (size_t)c->B * c->cap;
        if (!c->d_export)
            if (const int rc = dev_alloc(c, &c->d_export, records * (sizeof(svo_kp2d) + sizeof(svo_kp3d) + sizeof(svo_kp_info)))) return rc;
        if (o2) o2 = reinterpret_cast<svo_kp2d*>(c->d_export);
        if (o3) o3 = reinterpret_cast<svo_kp3d*>(c->d_export + records * sizeof(svo_kp2d));
        if (oi) oi = reinterpret_cast<svo_kp_info*>(c->d_export + records * (sizeof(svo_kp2d) + sizeof(svo_kp3d)));
    }
    // (SVO_EXPORT_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
    auto table = group_tile_table<ExportTile>(
        c, "SVO_EXPORT_TABLE_TILES", [&](const ExportTile* d, int m, hipStream_t s) { launch_export(d, m, o2, o3, oi, s); });
    int64_t used = 0;                        // records of the group so far
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_export_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.keyframe_id = -1;
        e.is_keyframe = q.stats.is_keyframe; e.time_stamp = (float)q.ts;
        const KpsDev* src = &q.kps[q.cur];
        if (what == SVO_EXPORT_FRAMES) {
            e.n = q.n_host;
            std::memcpy(e.pose, q.pose, sizeof(e.pose));
        } else if (!q.kfs.empty()) {
            const KfHost& k = q.kfs.back();
            e.keyframe_id = (int)q.kfs.size() - 1;
            e.n = k.n;
            std::memcpy(e.pose, k.pose, sizeof(e.pose));
            src = &k.kps;
        }
        used = (int64_t)align_up((size_t)used, 4);
        e.first = base + used;
        for (int start = 0; any && start < e.n; start += EXPORT_TILE)
            if (const int rc = table.add(export_tile(*src, start, std::min(EXPORT_TILE, e.n - start), used))) return rc;
        used += e.n;
    }
    if (const int rc = table.launch(false)) return rc;
    if (host && used > 0) {
        if (o2) HIP_TRY(hipMemcpyAsync(dst->kps2d + base, o2, sizeof(svo_kp2d) * used, hipMemcpyDeviceToHost, st));
        if (o3) HIP_TRY(hipMemcpyAsync(dst->kps3d + base, o3, sizeof(svo_kp3d) * used, hipMemcpyDeviceToHost, st));
        if (oi) HIP_TRY(hipMemcpyAsync(dst->info + base, oi, sizeof(svo_kp_info) * used, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}
