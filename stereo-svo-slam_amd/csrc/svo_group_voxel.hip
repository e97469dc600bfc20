// svo_group_voxel.hip — the voxel maps of a sequence group (include/svo_hip.h, "voxel maps"): a map per slot that has
// one, the fuse job (the organized world-frame clouds of the named slots, computed by grp_export_cloud in device mode
// into a block of the group, then one fuse launch per chunk), the export job (voxel.hip's count, scan, pairs, sort
// and gather per slot), the clear job and the prune job (voxel.hip's rebuild in place per slot; "voxel prune"). A map belongs to the slot: nothing else in the group touches it. The host
// arithmetic is svo_voxel_plan.hpp's, the state svo_group_state.hpp's. "voxel entries": the save job (the export job with
// voxel.hip's pack in place of its gather), the load job (one merge launch for the group's share) and the resize (a
// rehash per slot into a new allocation, between jobs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"
#include "svo_voxel_plan.hpp"

using namespace svo;

namespace {

constexpr size_t FUSE_STAGING_BYTES = (size_t)256 << 20;   // the slots of one chunk stage at most so much (one slot always fits)

VoxelMapDev map_dev(const svo_group::VoxelSlot& v) { return VoxelMapDev{v.p, v.params.voxel, v.params.log2_capacity, v.params.drop_flags, 0}; }

void drop_map(svo_group* c, svo_group::VoxelSlot& v) {
    if (v.p) dev_release(c, v.p, voxel_map_bytes(v.params.log2_capacity));
    v = svo_group::VoxelSlot{};
}

// the mirror of an empty map
VoxelHeader empty_head(const svo_voxel_params& p) {
    VoxelHeader h{};
    h.magic = VOXEL_MAGIC; h.log2_capacity = p.log2_capacity; h.voxel = p.voxel; h.drop_flags = p.drop_flags;
    return h;
}

}  // namespace

int grp_set_voxel_maps(svo_group* c, const int* seqs, int n, const svo_voxel_params* params) {
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream.get();
    HIP_TRY(hipStreamSynchronize(st));
    if (c->voxel_maps.empty()) {
        if (!params) return SVO_OK;
        c->voxel_maps.resize((size_t)c->B);
    }
    for (int i = 0; i < n; i++) {
        svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[i]];
        drop_map(c, v);
        if (!params) continue;
        if (const int rc = dev_alloc(c, &v.p, voxel_map_bytes(params->log2_capacity), false)) return rc;
        v.params = *params;
        v.head = empty_head(*params);
        launch_voxel_clear(map_dev(v), st);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SVO_OK;
}

bool grp_voxel_map_info(svo_group* c, int seq, svo_voxel_map_info* info) {
    if (c->voxel_maps.empty() || !c->voxel_maps[(size_t)seq].p) return false;
    const VoxelHeader& h = c->voxel_maps[(size_t)seq].head;
    if (info)
        *info = svo_voxel_map_info{h.voxel, h.log2_capacity, h.drop_flags, 0, (int64_t)h.n_voxels, (int64_t)h.n_fused, (int64_t)h.n_outside,
                                   (int64_t)h.overflow};
    return true;
}

int grp_clear_voxel_maps(svo_group* c, const int* seqs, int n) {
    if (const int rc = job_begin(c, "svo_submit_clear_voxel_maps")) return rc;
    if (c->voxel_maps.empty()) return SVO_OK;
    hipStream_t st = c->stream.get();
    for (int i = 0; i < n; i++) {
        svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[i]];
        if (!v.p) continue;
        launch_voxel_clear(map_dev(v), st);
        HIP_TRY(hipGetLastError());
        v.head = empty_head(v.params);
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SVO_OK;
}

// The statuses are settled on the host first (no map, no frame or keyframe, the load bound with the mirror's
// n_voxels); the slots that are left run in chunks: grp_export_cloud in device mode writes the chunk's organized
// records into d_voxel_records, one fuse launch puts them into the slots' maps, one launch gathers the maps' headers
// and one copy brings them back: the new mirrors, and what the job added to the counters. With sgm the records are the
// SGM cloud job's (svo_submit_fuse_clouds_sgm): its planes and check in the group's d_sgm block, no reverse block.
int grp_fuse_clouds(svo_group* c, int what, const int* seqs, const int* seg, int n, int seq0, const svo_cloud_style* style,
                    const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info, const svo_sgm_params* sgm) {
    if (const int rc = job_begin(c, "svo_submit_fuse_clouds")) return rc;
    hipStream_t st = c->stream.get();
    svo_cloud_style organized = *style;
    organized.layout = SVO_CLOUD_ORGANIZED;
    const int64_t points = grp_cloud_points(c, &organized);
    std::vector<int> todo, todo_at;                          // the slots to fuse (indices in the group) and their position in the job
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_fuse_info& f = clear(info[seg[i]]);
        f.seq = seq0 + seqs[i]; f.run = q.run; f.frame_id = q.frame_id; f.keyframe_id = -1;
        const svo_group::VoxelSlot* v = c->voxel_maps.empty() ? nullptr : &c->voxel_maps[(size_t)seqs[i]];
        if (!v || !v->p) { f.status = SVO_FUSE_NO_MAP; continue; }
        f.n_voxels = (int64_t)v->head.n_voxels;
        if (what == SVO_EXPORT_FRAMES ? q.frame_id < 0 : q.kfs.empty()) { f.status = SVO_FUSE_NONE; continue; }
        if (!voxel_load_ok(v->head.n_voxels, (uint64_t)points, v->params.log2_capacity)) { f.status = SVO_FUSE_FULL; continue; }
        f.status = SVO_FUSE_OK;
        todo.push_back(seqs[i]);
        todo_at.push_back(seg[i]);
    }
    if (todo.empty()) return SVO_OK;
    const size_t rec_bytes = sizeof(svo_map_point) * (size_t)points;
    // (SVO_CLOUD_CHUNK_SLOTS: fewer slots per chunk, so that tests reach the chunked path)
    const size_t per_slot = (size_t)grp_cloud_slot_bytes(c, &organized, check, sgm) + rec_bytes;
    const size_t m_max = std::min(todo.size(), table_tiles("SVO_CLOUD_CHUNK_SLOTS", std::max<size_t>(1, FUSE_STAGING_BYTES / std::max<size_t>(per_slot, 1))));
    if (const int rc = c->d_voxel_records.reserve(c, m_max * rec_bytes)) return rc;
    svo_map_point* const d_records = reinterpret_cast<svo_map_point*>(c->d_voxel_records.p);
    // the tables of a chunk: maps | headers | spans, m_max of each
    const size_t maps_off = 0, heads_off = voxel_up256(sizeof(VoxelMapDev) * m_max), spans_off = heads_off + voxel_up256(sizeof(VoxelHeader) * m_max);
    if (const int rc = c->d_voxel_tables.reserve(c, spans_off + voxel_up256(sizeof(VoxelSpanDev) * m_max))) return rc;
    uint8_t* const h_tab = c->d_voxel_tables.host.get();
    uint8_t* const d_tab = c->d_voxel_tables.p;
    std::vector<svo_cloud_segment> csegs(m_max);
    std::vector<int> local(m_max);
    for (size_t j = 0; j < m_max; j++) local[j] = (int)j;
    for (size_t i0 = 0; i0 < todo.size(); i0 += m_max) {
        const int m = (int)std::min(m_max, todo.size() - i0);
        const svo_cloud_dst cloud_dst{csegs.data(), d_records, (int64_t)m * points};
        if (const int rc = grp_export_cloud(c, what, SVO_MEM_DEVICE, todo.data() + i0, local.data(), m, seq0, &organized, check, &cloud_dst, sgm)) return rc;
        VoxelMapDev* h_maps = reinterpret_cast<VoxelMapDev*>(h_tab + maps_off);
        VoxelSpanDev* h_spans = reinterpret_cast<VoxelSpanDev*>(h_tab + spans_off);
        int n_spans = 0;
        int64_t tiles = 0;
        for (int j = 0; j < m; j++) {
            const svo_group::VoxelSlot& v = c->voxel_maps[(size_t)todo[i0 + (size_t)j]];
            svo_fuse_info& f = info[todo_at[i0 + (size_t)j]];
            const svo_cloud_segment& e = csegs[(size_t)j];
            h_maps[j] = map_dev(v);
            f.keyframe_id = e.keyframe_id;
            std::memcpy(f.pose, e.pose, sizeof(f.pose));
            if (e.status != SVO_CLOUD_OK) { f.status = SVO_FUSE_NONE; continue; }
            f.n_offered = e.n_points;
            h_spans[n_spans++] = VoxelSpanDev{d_records + (int64_t)j * points, points, tiles, j, stamp};
            tiles += voxel_span_tiles(points);
        }
        HIP_TRY(hipMemcpyAsync(d_tab + maps_off, h_maps, sizeof(VoxelMapDev) * (size_t)m, hipMemcpyHostToDevice, st));
        if (n_spans > 0) {
            HIP_TRY(hipMemcpyAsync(d_tab + spans_off, h_spans, sizeof(VoxelSpanDev) * (size_t)n_spans, hipMemcpyHostToDevice, st));
            launch_voxel_fuse(reinterpret_cast<const VoxelSpanDev*>(d_tab + spans_off), n_spans, tiles,
                              reinterpret_cast<const VoxelMapDev*>(d_tab + maps_off), false, st);
            HIP_TRY(hipGetLastError());
        }
        launch_voxel_headers(reinterpret_cast<const VoxelMapDev*>(d_tab + maps_off), m, reinterpret_cast<VoxelHeader*>(d_tab + heads_off), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_tab + heads_off, d_tab + heads_off, sizeof(VoxelHeader) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // fused; the blocks are free for the next chunk
        const VoxelHeader* heads = reinterpret_cast<const VoxelHeader*>(h_tab + heads_off);
        for (int j = 0; j < m; j++) {
            svo_group::VoxelSlot& v = c->voxel_maps[(size_t)todo[i0 + (size_t)j]];
            svo_fuse_info& f = info[todo_at[i0 + (size_t)j]];
            f.n_fused = (int32_t)(heads[j].n_fused - v.head.n_fused);
            f.n_outside = (int32_t)(heads[j].n_outside - v.head.n_outside);
            f.n_voxels = (int64_t)heads[j].n_voxels;
            v.head = heads[j];
        }
    }
    return SVO_OK;
}

// grp_export_voxel_maps and grp_save_voxel_maps: the kept entries of each named slot's map in key order as the records
// `launch` writes (launch_voxel_extract: points; launch_voxel_pack: entries) into records[first_point ...].
template <class Record, class Launch>
static int export_records(svo_group* c, const char* who, int mem, const int* seqs, const int* seg, const svo_voxel_region* regions, int n, int seq0,
                          const svo_voxel_filter* filter, svo_voxel_segment* segments, Record* records, Launch launch) {
    if (const int rc = job_begin(c, who)) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        const svo_voxel_region& r = regions[i];
        svo_voxel_segment& e = clear(segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.first_point = r.first_point; e.status = SVO_VOXEL_NO_MAP;
        const svo_group::VoxelSlot* v = c->voxel_maps.empty() ? nullptr : &c->voxel_maps[(size_t)seqs[i]];
        if (!v || !v->p) continue;
        e.n_voxels = (int64_t)v->head.n_voxels; e.n_fused = (int64_t)v->head.n_fused;
        e.voxel = v->params.voxel; e.log2_capacity = v->params.log2_capacity;
        if (!voxel_extract_fits(e.n_voxels, r.point_capacity)) { e.status = SVO_VOXEL_TOO_SMALL; continue; }
        e.status = SVO_VOXEL_OK;
        if (e.n_voxels == 0) continue;
        const VoxelMapDev mp = map_dev(*v);
        const VoxelFilterDev f{std::max<uint32_t>(1u, filter->min_count), std::max(filter->min_stamp, r.min_stamp)};
        if (const int rc = c->d_voxel_offsets.reserve(c, voxel_offsets_bytes(mp.log2_capacity))) return rc;
        int32_t* offsets = reinterpret_cast<int32_t*>(c->d_voxel_offsets.p);
        launch_voxel_count(mp, f, offsets, st);
        HIP_TRY(hipGetLastError());
        int32_t kept = 0;
        HIP_TRY(hipMemcpyAsync(&kept, offsets + voxel_map_tiles(mp.log2_capacity), sizeof(kept), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (kept < 0 || !voxel_extract_fits(kept, r.point_capacity))
            return svo_set_error(SVO_ERR_INVALID, "%s: slot %d keeps %d entries, its mirror counts %lld", who, e.seq, kept,
                                 (long long)e.n_voxels);
        e.n_points = kept;
        if (kept == 0) continue;
        size_t temp_bytes = 0;
        if (const int rc = voxel_sort_temp_bytes((size_t)kept, &temp_bytes)) return rc;
        const VoxelExtractPlan plan = voxel_extract_plan((uint64_t)kept, temp_bytes);
        if (const int rc = c->d_voxel_sort.reserve(c, plan.bytes)) return rc;
        if (host)
            if (const int rc = c->d_voxel_out.reserve(c, sizeof(Record) * (size_t)kept)) return rc;
        uint8_t* ws = c->d_voxel_sort.p;
        Record* out = host ? reinterpret_cast<Record*>(c->d_voxel_out.p) : records + r.first_point;
        if (const int rc = launch(mp, f, offsets, (size_t)kept, reinterpret_cast<uint64_t*>(ws + plan.keys_in),
                                  reinterpret_cast<uint64_t*>(ws + plan.keys_out), reinterpret_cast<uint32_t*>(ws + plan.index_in),
                                  reinterpret_cast<uint32_t*>(ws + plan.index_out), ws + plan.sort_temp, temp_bytes, out, st))
            return rc;
        HIP_TRY(hipGetLastError());
        if (host) HIP_TRY(hipMemcpyAsync(records + r.first_point, out, sizeof(Record) * (size_t)kept, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // delivered, and the blocks are free for the next slot
    }
    return SVO_OK;
}

int grp_export_voxel_maps(svo_group* c, int mem, const int* seqs, const int* seg, const svo_voxel_region* regions, int n, int seq0,
                          const svo_voxel_filter* filter, const svo_voxel_dst* dst) {
    return export_records(c, "svo_submit_export_voxel_maps", mem, seqs, seg, regions, n, seq0, filter, dst->segments, dst->points, launch_voxel_extract);
}

int grp_save_voxel_maps(svo_group* c, int mem, const int* seqs, const int* seg, const svo_voxel_region* regions, int n, int seq0,
                        const svo_voxel_filter* filter, const svo_voxel_entry_dst* dst) {
    return export_records(c, "svo_submit_save_voxel_maps", mem, seqs, seg, regions, n, seq0, filter, dst->segments, dst->entries, launch_voxel_pack);
}

float grp_voxel_edge(const svo_group* c, int seq) {
    return c->voxel_maps.empty() || !c->voxel_maps[(size_t)seq].p ? 0.f : c->voxel_maps[(size_t)seq].params.voxel;
}

// The statuses are settled on the host first (no map, no pose, the staging bound with the mirror's n_voxels); one
// block holds the tile offsets and the staging of the largest slot, and the slots that are left use it one after the
// other in stream order: the six launches of launch_voxel_prune and a copy of the map's header, which is the new
// mirror. One wait at the end.
int grp_prune_voxel_maps(svo_group* c, const int* seqs, const int* seg, int n, int seq0, const svo_voxel_keep* keep, int center_mode,
                         const float* centers, svo_prune_info* info) {
    if (const int rc = job_begin(c, "svo_submit_prune_voxel_maps")) return rc;
    hipStream_t st = c->stream.get();
    struct Todo { int seq, at; VoxelKeepDev f; VoxelPrunePlan plan; size_t offsets; };
    std::vector<Todo> todo;
    size_t need = 0;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_prune_info& e = clear(info[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.status = SVO_PRUNE_NO_MAP;
        const svo_group::VoxelSlot* v = c->voxel_maps.empty() ? nullptr : &c->voxel_maps[(size_t)seqs[i]];
        if (!v || !v->p) continue;
        e.n_before = e.n_kept = (int64_t)v->head.n_voxels;
        Todo t{seqs[i], seg[i], VoxelKeepDev{std::max<uint32_t>(1u, keep->min_count), keep->min_stamp, {0, 0, 0}, keep->radius < 0 ? -1 : keep->radius}, {}, 0};
        e.status = SVO_PRUNE_NO_POSE;
        if (center_mode == SVO_PRUNE_CENTER_POSE && q.frame_id < 0) continue;
        if (keep->radius >= 0) {
            const float* at = center_mode == SVO_PRUNE_CENTER_POSE ? q.pose : centers + 3 * (size_t)i;
            std::memcpy(e.center, at, sizeof(e.center));
            // (a given centre was checked at the call, and the slot's map cannot have changed since: setters wait)
            if (!voxel_center_index(at[0], v->params.voxel, t.f.c[0]) || !voxel_center_index(at[1], v->params.voxel, t.f.c[1]) ||
                !voxel_center_index(at[2], v->params.voxel, t.f.c[2]))
                continue;
        }
        if (v->head.n_voxels > ((uint64_t)1 << v->params.log2_capacity) || !voxel_prune_plan(v->head.n_voxels, t.plan)) {
            e.status = SVO_PRUNE_TOO_LARGE;
            continue;
        }
        e.status = SVO_PRUNE_OK;
        for (int j = 0; j < 3; j++) e.center_voxel[j] = t.f.c[j];
        t.offsets = voxel_offsets_bytes(v->params.log2_capacity);
        need = std::max(need, t.offsets + t.plan.bytes);
        todo.push_back(t);
    }
    if (todo.empty()) return SVO_OK;
    if (const int rc = c->d_voxel_prune.reserve(c, need)) return rc;
    std::vector<VoxelHeader> heads(todo.size());
    for (size_t j = 0; j < todo.size(); j++) {
        const svo_group::VoxelSlot& v = c->voxel_maps[(size_t)todo[j].seq];
        launch_voxel_prune(map_dev(v), todo[j].f, reinterpret_cast<int32_t*>(c->d_voxel_prune.p), c->d_voxel_prune.p + todo[j].offsets,
                           v.head.n_voxels, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&heads[j], v.p, sizeof(VoxelHeader), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < todo.size(); j++) {
        svo_group::VoxelSlot& v = c->voxel_maps[(size_t)todo[j].seq];
        info[todo[j].at].n_kept = (int64_t)heads[j].n_voxels;
        v.head = heads[j];
    }
    return SVO_OK;
}

// grp_prune_voxel_maps with a carve ("voxel carve"). The statuses are settled on the host first (no map, an empty slot, no
// pose, the staging bound); the slots that are left run in chunks: grp_export_cloud in device mode writes the chunk's
// organized camera-frame records into the occluded AR job's block, then per slot the six launches of
// launch_voxel_carve in the prune job's block (tile offsets | staging | ballot words; the counters of every slot of the
// job lie behind them) and a copy of the map's header, the new mirror. One wait per chunk, one copy of all counters.
int grp_carve_voxel_maps(svo_group* c, const int* seqs, const int* seg, int n, int seq0, const svo_cloud_style* cloud, const svo_sgm_params* sgm,
                         const svo_stereo_check* check, const svo_voxel_carve_rule* carve, const svo_voxel_keep* keep, int center_mode,
                         const float* centers, svo_carve_info* info) {
    if (const int rc = job_begin(c, "svo_submit_carve_voxel_maps")) return rc;
    hipStream_t st = c->stream.get();
    struct Todo { int seq, at; VoxelKeepDev f; VoxelPrunePlan plan; size_t offsets; VoxelCarvePlan extra; };
    std::vector<Todo> todo;
    size_t need = 0;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_carve_info& e = clear(info[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.status = SVO_CARVE_NO_MAP;
        std::memcpy(e.pose, q.pose, sizeof(e.pose));
        const svo_group::VoxelSlot* v = c->voxel_maps.empty() ? nullptr : &c->voxel_maps[(size_t)seqs[i]];
        if (!v || !v->p) continue;
        e.n_before = e.n_kept = (int64_t)v->head.n_voxels;
        e.status = SVO_CARVE_NONE;
        if (q.frame_id < 0 || !q.cur_set) continue;
        Todo t{seqs[i], seg[i], VoxelKeepDev{std::max<uint32_t>(1u, keep->min_count), keep->min_stamp, {0, 0, 0}, keep->radius < 0 ? -1 : keep->radius}, {}, 0, {}};
        e.status = SVO_CARVE_NO_POSE;
        if (keep->radius >= 0) {
            const float* at = center_mode == SVO_PRUNE_CENTER_POSE ? q.pose : centers + 3 * (size_t)i;
            if (!voxel_center_index(at[0], v->params.voxel, t.f.c[0]) || !voxel_center_index(at[1], v->params.voxel, t.f.c[1]) ||
                !voxel_center_index(at[2], v->params.voxel, t.f.c[2]))
                continue;
        }
        if (v->head.n_voxels > ((uint64_t)1 << v->params.log2_capacity) || !voxel_prune_plan(v->head.n_voxels, t.plan)) {
            e.status = SVO_CARVE_TOO_LARGE;
            continue;
        }
        e.status = SVO_CARVE_OK;
        t.offsets = voxel_offsets_bytes(v->params.log2_capacity);
        t.extra = voxel_carve_plan(v->params.log2_capacity);
        need = std::max(need, t.offsets + t.plan.bytes + t.extra.counters);   // (the ballot words; the counters follow for all slots)
        todo.push_back(t);
    }
    if (todo.empty()) return SVO_OK;
    svo_cloud_style organized = *cloud;
    organized.layout = SVO_CLOUD_ORGANIZED;
    const int64_t points = grp_cloud_points(c, &organized);
    const size_t rec_bytes = sizeof(svo_map_point) * (size_t)points;
    // (SVO_AR_CHUNK_SLOTS: fewer slots per chunk, as in the occluded AR job)
    const size_t per_slot = (size_t)grp_cloud_slot_bytes(c, &organized, check, sgm) + rec_bytes;
    const size_t m_max = std::min(todo.size(), table_tiles("SVO_AR_CHUNK_SLOTS", std::max<size_t>(1, FUSE_STAGING_BYTES / std::max<size_t>(per_slot, 1))));
    if (const int rc = c->d_ar_occ.reserve(c, m_max * rec_bytes)) return rc;
    if (const int rc = c->d_voxel_prune.reserve(c, need + 256 * todo.size())) return rc;
    svo_map_point* const d_records = reinterpret_cast<svo_map_point*>(c->d_ar_occ.p);
    uint8_t* const block = c->d_voxel_prune.p;
    std::vector<VoxelHeader> heads(todo.size());
    std::vector<unsigned long long> counts(32 * todo.size(), 0);
    std::vector<svo_cloud_segment> csegs(m_max);
    std::vector<int> local(m_max), chunk_seqs(m_max);
    for (size_t j = 0; j < m_max; j++) local[j] = (int)j;
    const int cols = c->width / organized.step, rows = c->height / organized.step;
    for (size_t i0 = 0; i0 < todo.size(); i0 += m_max) {
        const int m = (int)std::min(m_max, todo.size() - i0);
        for (int j = 0; j < m; j++) chunk_seqs[(size_t)j] = todo[i0 + (size_t)j].seq;
        const svo_cloud_dst cloud_dst{csegs.data(), d_records, (int64_t)m * points};
        if (const int rc = grp_export_cloud(c, SVO_EXPORT_FRAMES, SVO_MEM_DEVICE, chunk_seqs.data(), local.data(), m, seq0, &organized, check, &cloud_dst, sgm))
            return rc;
        for (int j = 0; j < m; j++) {
            const Todo& t = todo[i0 + (size_t)j];
            const svo_group::VoxelSlot& v = c->voxel_maps[(size_t)t.seq];
            const Seq& q = c->seqs[t.seq];
            if (csegs[(size_t)j].status != SVO_CLOUD_OK)
                return svo_set_error(SVO_ERR_INVALID, "svo_submit_carve_voxel_maps: slot %d has a frame and no cloud", seq0 + t.seq);
            svo_ar_camera cam;
            svo_ar_camera_of_pose(q.pose, &q.cam, &cam);
            VoxelCarveRule rule{};
            rule.keep = t.f;
            rule.carve = voxel_carve_dev(*carve, cam, c->width, c->height, d_records + (int64_t)j * points, cols, rows, organized.step);
            rule.ballots = reinterpret_cast<unsigned long long*>(block + t.offsets + t.plan.bytes);
            rule.counters = reinterpret_cast<unsigned long long*>(block + need + 256 * (i0 + (size_t)j));
            launch_voxel_carve(map_dev(v), rule, reinterpret_cast<int32_t*>(block), block + t.offsets, v.head.n_voxels, st);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&heads[i0 + (size_t)j], v.p, sizeof(VoxelHeader), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));   // carved; the records are free for the next chunk
    }
    HIP_TRY(hipMemcpyAsync(counts.data(), block + need, 256 * todo.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < todo.size(); j++) {
        svo_group::VoxelSlot& v = c->voxel_maps[(size_t)todo[j].seq];
        svo_carve_info& e = info[todo[j].at];
        e.n_kept = (int64_t)heads[j].n_voxels;
        e.n_tested = (int32_t)counts[32 * j];
        e.n_carved = (int32_t)counts[32 * j + 1];
        v.head = heads[j];
    }
    return SVO_OK;
}

// The statuses are settled on the host first (no map, the load bound with the mirror's n_voxels, 0 for a replace); the
// slots that are left share one merge launch: host entries are staged in d_voxel_in, a replace clears its maps first,
// the tables (maps | headers | counts | spans) are the fuse job's block, one launch gathers the headers and one wait
// brings headers and counts back: the new mirrors and the infos.
int grp_load_voxel_maps(svo_group* c, int mode, int mem, const int* seqs, const int* seg, const svo_voxel_entry_span* spans, int n, int seq0,
                        svo_voxel_load_info* info) {
    if (const int rc = job_begin(c, "svo_submit_load_voxel_maps")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    std::vector<int> todo;                                   // positions in the group's share
    size_t in_bytes = 0;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_voxel_load_info& e = clear(info[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.status = SVO_VOXEL_LOAD_NO_MAP;
        const svo_group::VoxelSlot* v = c->voxel_maps.empty() ? nullptr : &c->voxel_maps[(size_t)seqs[i]];
        if (!v || !v->p) continue;
        e.n_voxels = (int64_t)v->head.n_voxels;
        e.status = SVO_VOXEL_LOAD_FULL;
        if (!voxel_merge_load_ok(mode == SVO_VOXEL_LOAD_REPLACE ? 0 : v->head.n_voxels, &spans[i].n, 1, v->params.log2_capacity)) continue;
        e.status = SVO_VOXEL_LOADED;
        todo.push_back(i);
        if (host) in_bytes += voxel_up256(sizeof(svo_voxel_entry) * (size_t)spans[i].n);
    }
    if (todo.empty()) return SVO_OK;
    const size_t m = todo.size();
    int64_t all_tiles = 0;                                   // (before any clear: a job too large for one launch changes nothing)
    for (size_t j = 0; j < m; j++) {
        all_tiles += voxel_entry_span_tiles(spans[todo[j]].n);
        if (all_tiles > INT32_MAX) return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_load_voxel_maps: too many records for one job");
    }
    if (host)
        if (const int rc = c->d_voxel_in.reserve(c, in_bytes)) return rc;
    const size_t maps_off = 0, heads_off = voxel_up256(sizeof(VoxelMapDev) * m), counts_off = heads_off + voxel_up256(sizeof(VoxelHeader) * m),
                 spans_off = counts_off + voxel_up256(sizeof(VoxelMergeCounts) * m);
    if (const int rc = c->d_voxel_tables.reserve(c, spans_off + voxel_up256(sizeof(VoxelEntrySpanDev) * m))) return rc;
    uint8_t* const h_tab = c->d_voxel_tables.host.get();
    uint8_t* const d_tab = c->d_voxel_tables.p;
    VoxelMapDev* h_maps = reinterpret_cast<VoxelMapDev*>(h_tab + maps_off);
    VoxelEntrySpanDev* h_spans = reinterpret_cast<VoxelEntrySpanDev*>(h_tab + spans_off);
    int n_spans = 0;
    int64_t tiles = 0;
    size_t in_at = 0;
    for (size_t j = 0; j < m; j++) {
        const svo_voxel_entry_span& s = spans[todo[j]];
        svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[todo[j]]];
        h_maps[j] = map_dev(v);
        if (mode == SVO_VOXEL_LOAD_REPLACE) {
            launch_voxel_clear(map_dev(v), st);
            HIP_TRY(hipGetLastError());
            v.head = empty_head(v.params);
        }
        if (s.n == 0) continue;
        const svo_voxel_entry* from = s.entries;
        if (host) {
            svo_voxel_entry* staged = reinterpret_cast<svo_voxel_entry*>(c->d_voxel_in.p + in_at);
            HIP_TRY(hipMemcpyAsync(staged, s.entries, sizeof(svo_voxel_entry) * (size_t)s.n, hipMemcpyHostToDevice, st));
            in_at += voxel_up256(sizeof(svo_voxel_entry) * (size_t)s.n);
            from = staged;
        }
        h_spans[n_spans++] = VoxelEntrySpanDev{from, s.n, tiles, (int32_t)j, 0};
        tiles += voxel_entry_span_tiles(s.n);
    }
    HIP_TRY(hipMemcpyAsync(d_tab + maps_off, h_maps, sizeof(VoxelMapDev) * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_tab + counts_off, 0, sizeof(VoxelMergeCounts) * m, st));
    if (n_spans > 0) {
        HIP_TRY(hipMemcpyAsync(d_tab + spans_off, h_spans, sizeof(VoxelEntrySpanDev) * (size_t)n_spans, hipMemcpyHostToDevice, st));
        launch_voxel_merge(reinterpret_cast<const VoxelEntrySpanDev*>(d_tab + spans_off), n_spans, tiles, reinterpret_cast<const VoxelMapDev*>(d_tab + maps_off),
                           reinterpret_cast<VoxelMergeCounts*>(d_tab + counts_off), st);
        HIP_TRY(hipGetLastError());
    }
    launch_voxel_headers(reinterpret_cast<const VoxelMapDev*>(d_tab + maps_off), (int)m, reinterpret_cast<VoxelHeader*>(d_tab + heads_off), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tab + heads_off, d_tab + heads_off, counts_off - heads_off + sizeof(VoxelMergeCounts) * m, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // loaded; the caller's entries and the blocks are free
    const VoxelHeader* heads = reinterpret_cast<const VoxelHeader*>(h_tab + heads_off);
    const VoxelMergeCounts* counts = reinterpret_cast<const VoxelMergeCounts*>(h_tab + counts_off);
    for (size_t j = 0; j < m; j++) {
        svo_voxel_load_info& e = info[seg[todo[j]]];
        e.n_offered = (int64_t)counts[j].n_offered; e.n_merged = (int64_t)counts[j].n_merged;
        e.n_skipped = (int64_t)counts[j].n_skipped; e.n_claimed = (int64_t)counts[j].n_claimed;
        e.n_voxels = (int64_t)heads[j].n_voxels;
        c->voxel_maps[(size_t)seqs[todo[j]]].head = heads[j];
    }
    return SVO_OK;
}

int grp_resize_voxel_maps(svo_group* c, const int* seqs, int n, int log2_capacity, int phase) {
    if (c->voxel_maps.empty()) return SVO_OK;
    auto moves = [&](const svo_group::VoxelSlot& v) { return v.p && v.params.log2_capacity != log2_capacity; };
    if (phase == VOXEL_RESIZE_CHECK) {
        for (int i = 0; i < n; i++) {
            const svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[i]];
            if (v.p && !voxel_rehash_ok(v.head.n_voxels, log2_capacity))
                return svo_set_error(SVO_ERR_CAPACITY, "svo_ctx_resize_voxel_maps: a slot's %llu voxels exceed %llu, the load limit of log2_capacity %d",
                                     v.head.n_voxels, (unsigned long long)voxel_load_limit(log2_capacity), log2_capacity);
        }
        return SVO_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (phase == VOXEL_RESIZE_ABORT) {                       // give back what VOXEL_RESIZE_ALLOC made
        for (int i = 0; i < n; i++) {
            svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[i]];
            if (v.next) dev_release(c, v.next, voxel_map_bytes(log2_capacity));
            v.next = nullptr;
        }
        return SVO_OK;
    }
    if (phase == VOXEL_RESIZE_ALLOC) {                       // every new map of the group, before any map is moved
        for (int i = 0; i < n; i++) {
            svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[i]];
            if (!moves(v)) continue;
            if (const int rc = dev_alloc(c, &v.next, voxel_map_bytes(log2_capacity), false)) return rc;
        }
        return SVO_OK;
    }
    hipStream_t st = c->stream.get();                        // VOXEL_RESIZE_MOVE
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        svo_group::VoxelSlot& v = c->voxel_maps[(size_t)seqs[i]];
        if (!moves(v) || !v.next) continue;
        svo_group::VoxelSlot to = v;
        to.p = v.next;
        to.next = nullptr;
        to.params.log2_capacity = log2_capacity;
        to.head.log2_capacity = log2_capacity;
        launch_voxel_rehash(map_dev(v), map_dev(to), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));   // moved: the old map can go
        v.next = nullptr;
        drop_map(c, v);
        v = to;
    }
    return SVO_OK;
}
