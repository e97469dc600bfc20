// svo_group_map.hip — the map export of a sequence group (svo_submit_export_map): every keyframe of its named slots
// from a given one on, filtered and compacted into 16-byte points by map.hip's kernels, as segments, keyframe entries
// and points; and svo_map_size. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

// (a trimmed slot: from its first resident keyframe on, if that is later; *from receives the effective start)
void grp_map_size(const svo_group* c, int seq, int from_keyframe, int* keyframes, int64_t* points_bound, int* from) {
    const Seq& q = c->seqs[seq];
    from_keyframe = std::max(from_keyframe, q.kfs.first());
    int64_t bound = 0;
    for (size_t k = (size_t)from_keyframe; k < q.kfs.size(); k++) bound += q.kfs[k].n;
    if (keyframes) *keyframes = (int)std::max<int64_t>(0, (int64_t)q.kfs.size() - from_keyframe);
    if (points_bound) *points_bound = bound;
    if (from) *from = from_keyframe;
}

// The named slots of the group as segments, keyframe entries and points (svo_submit_export_map). The keypoint counts
// are the host's own (KfHost::n): the capacities are checked against them before anything is launched, and the tile
// table is built here (group_tile_table: in the group's argument blocks). The kept counts of the keyframes come back
// in one copy; they place the keyframe entries and, in host mode, size the one copy of each slot's kept prefix out of
// the staging block.
int grp_export_map(svo_group* c, int mem, const int* seqs, const int* seg, const svo_map_region* regions, int n, int seq0,
                   const svo_map_filter* filter, const svo_map_dst* dst) {
    if (const int rc = job_begin(c, "svo_submit_export_map")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    struct Placed { int i, set0; int64_t stage; };   // a delivered slot: its first set and its first record of the staging block
    std::vector<Placed> placed;
    std::vector<MapTile> tiles;
    int sets = 0;
    int64_t staged = 0;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        const svo_map_region& r = regions[i];
        svo_map_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.time_stamp = (float)q.ts;
        e.n_keyframes = (int)q.kfs.size(); e.keyframes_retired = q.kfs_retired; e.first_keyframe = q.kfs.first();
        grp_map_size(c, seqs[i], r.from_keyframe, &e.n_exported, &e.points_bound, &e.from_keyframe);
        if (e.n_exported > r.keyframe_capacity || e.points_bound > r.point_capacity) {
            e.status = SVO_MAP_TOO_SMALL;
            continue;
        }
        if (e.n_exported == 0) continue;
        placed.push_back({i, sets, staged});
        const int region_tile = (int)tiles.size();
        for (int k = e.from_keyframe; k < e.n_keyframes; k++)
            map_tiles(q.kfs[k].kps, q.kfs[k].n, k, sets++, host ? staged : r.first_point, region_tile, tiles);
        staged += e.points_bound;
    }
    const int* kept = nullptr;               // per exported keyframe (set)
    if (!tiles.empty()) {
        if (const int rc = c->d_map_counts.reserve(c, sizeof(int) * align_up((size_t)sets + tiles.size(), 1024))) return rc;
        if (host && staged > 0)
            if (const int rc = c->d_map_points.reserve(c, sizeof(svo_map_point) * (size_t)staged)) return rc;
        svo_map_point* out = host ? c->d_map_points.p : dst->points;
        int* set_counts = c->d_map_counts.p;
        int* tile_counts = set_counts + sets;
        // (SVO_MAP_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
        auto table = group_tile_table<MapTile>(c, "SVO_MAP_TABLE_TILES", [&](const MapTile* d, int m, hipStream_t s) {
            launch_map(d, m, *filter, out, tile_counts, set_counts, s);
        });
        for (const MapTile& t : tiles)
            if (const int rc = table.add(t)) return rc;
        if (const int rc = table.launch(false)) return rc;
        kept = c->d_map_counts.host.get();
        HIP_TRY(hipMemcpyAsync(c->d_map_counts.host.get(), set_counts, sizeof(int) * (size_t)sets, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (const Placed& p : placed) {
        const Seq& q = c->seqs[seqs[p.i]];
        const svo_map_region& r = regions[p.i];
        svo_map_segment& e = dst->segments[seg[p.i]];
        int64_t at = 0;
        for (int j = 0; j < e.n_exported; j++) {
            const KfHost& k = q.kfs[e.from_keyframe + j];
            svo_map_keyframe& o = clear(dst->keyframes[r.first_keyframe_entry + j]);
            o.id = e.from_keyframe + j; o.n_total = k.n; o.n = kept[p.set0 + j];
            o.first = r.first_point + at;
            std::memcpy(o.pose, k.pose, sizeof(o.pose));
            at += o.n;
        }
        e.n_points = at;
        if (host && at > 0)
            HIP_TRY(hipMemcpyAsync(dst->points + r.first_point, c->d_map_points.p + p.stage, sizeof(svo_map_point) * (size_t)at,
                                   hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}
