// svo_capi_voxel.hip — the stage entries of the voxel maps (include/svo_hip.h, "voxel maps", "voxel prune", "voxel carve", "voxel
// entries"): clear, fuse, info, extract, prune, carve, pack, merge and rehash on maps in the caller's device memory, complete on return. Every check is made on the host before any
// launch (the params, the alignment, the header of each named map, the load bound), with the arithmetic of
// svo_voxel_plan.hpp; the kernels are voxel.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "svo_handle.hpp"
#include "svo_voxel_plan.hpp"

using namespace svo;

namespace svo {

int voxel_check_params(const svo_voxel_params* p, bool ctx, const char* who) {
    if (!p) return svo_set_error(SVO_ERR_INVALID, "%s: no params", who);
    if (!(p->voxel > 0.f) || !(p->voxel <= FLT_MAX)) return svo_set_error(SVO_ERR_INVALID, "%s: voxel must be finite and > 0", who);
    if (!voxel_log2_ok(p->log2_capacity, ctx))
        return svo_set_error(SVO_ERR_INVALID, "%s: log2_capacity %d outside %d .. %d", who, p->log2_capacity,
                             ctx ? VOXEL_LOG2_MIN_CTX : VOXEL_LOG2_MIN, VOXEL_LOG2_MAX);
    if ((p->drop_flags & ~(uint32_t)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY)) || p->_reserved != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: drop_flags 0x%x has unknown bits, or _reserved is not 0", who, p->drop_flags);
    return SVO_OK;
}

// the header of a map that was cleared with exactly these params
bool voxel_header_matches(const VoxelHeader& hd, const svo_voxel_params& p) {
    return hd.magic == VOXEL_MAGIC && hd.log2_capacity == p.log2_capacity && memcmp(&hd.voxel, &p.voxel, 4) == 0 && hd.drop_flags == p.drop_flags;
}

}  // namespace svo

static VoxelMapDev map_dev(void* data, const svo_voxel_params& p) {
    return VoxelMapDev{static_cast<uint8_t*>(data), p.voxel, p.log2_capacity, p.drop_flags, 0};
}

static int check_map(const svo_voxel_map* m, const char* who, int i) {
    if (!m) return svo_set_error(SVO_ERR_INVALID, "%s: no map", who);
    if (const int rc = voxel_check_params(&m->params, false, who)) return rc;
    if (!m->data || ((uintptr_t)m->data & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: map %d is NULL or not 16-byte aligned", who, i);
    return SVO_OK;
}

extern "C" int64_t svo_voxel_map_bytes(int log2_capacity) { return (int64_t)voxel_map_bytes(log2_capacity); }

extern "C" int svo_voxel_clear(svo_handle* h, void* map, const svo_voxel_params* params) {
    CHECK_H(h);
    const svo_voxel_map m{map, params ? *params : svo_voxel_params{}};
    if (!params) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_clear: no params");
    if (const int rc = check_map(&m, "svo_voxel_clear", 0)) return rc;
    launch_voxel_clear(map_dev(map, *params), h->stream);
    return finish_launch(h);
}

extern "C" int svo_voxel_info(svo_handle* h, const void* map, svo_voxel_map_info* info) {
    CHECK_H(h);
    if (!map || ((uintptr_t)map & 15) || !info) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_info: map is NULL or not 16-byte aligned, or no info");
    VoxelHeader hd;
    HIP_TRY(hipMemcpyAsync(&hd, map, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const svo_voxel_params p{hd.voxel, hd.log2_capacity, hd.drop_flags, 0};
    if (hd.magic != VOXEL_MAGIC || voxel_check_params(&p, false, "svo_voxel_info") != SVO_OK)
        return svo_set_error(SVO_ERR_INVALID, "svo_voxel_info: the map was never cleared");
    *info = svo_voxel_map_info{hd.voxel, hd.log2_capacity, hd.drop_flags, 0, (int64_t)hd.n_voxels, (int64_t)hd.n_fused, (int64_t)hd.n_outside,
                               (int64_t)hd.overflow};
    return SVO_OK;
}

extern "C" int svo_voxel_fuse(svo_handle* h, int n_spans, const svo_voxel_span* spans, int n_maps, const svo_voxel_map* maps) {
    CHECK_H(h);
    if (n_spans < 0 || n_maps < 0 || (n_spans > 0 && !spans) || (n_maps > 0 && !maps))
        return svo_set_error(SVO_ERR_INVALID, "svo_voxel_fuse: bad arguments");
    std::vector<VoxelMapDev> dmaps((size_t)n_maps);
    std::vector<const void*> seen;
    for (int i = 0; i < n_maps; i++) {
        if (const int rc = check_map(&maps[i], "svo_voxel_fuse", i)) return rc;
        dmaps[(size_t)i] = map_dev(maps[i].data, maps[i].params);
        seen.push_back(maps[i].data);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_fuse: a map is named twice");
    std::vector<VoxelSpanDev> dspans;
    std::vector<uint64_t> records((size_t)n_maps, 0);
    int64_t tiles = 0;
    for (int i = 0; i < n_spans; i++) {
        const svo_voxel_span& s = spans[i];
        if (!voxel_span_ok((uintptr_t)s.points, s.n)) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_fuse: span %d: n < 0, or records NULL or not 16-byte aligned", i);
        if (s.map < 0 || s.map >= n_maps) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_fuse: span %d names map %d of %d", i, s.map, n_maps);
        if (!voxel_add_records(records[(size_t)s.map], s.n)) return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_fuse: span %d: too many records", i);
        if (s.n == 0) continue;
        dspans.push_back(VoxelSpanDev{s.points, s.n, tiles, s.map, s.stamp});
        tiles += voxel_span_tiles(s.n);
        if (tiles > INT32_MAX) return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_fuse: too many records for one call");
    }
    if (n_maps == 0) return SVO_OK;
    // the tables of the call: the maps, their headers as the device holds them now, the spans
    const size_t maps_bytes = voxel_up256(sizeof(VoxelMapDev) * dmaps.size()), heads_bytes = voxel_up256(sizeof(VoxelHeader) * dmaps.size());
    if (const int rc = h->voxel_ws.reserve(maps_bytes + heads_bytes + voxel_up256(sizeof(VoxelSpanDev) * dspans.size()), h->stream)) return rc;
    VoxelMapDev* d_maps = reinterpret_cast<VoxelMapDev*>(h->voxel_ws.ptr.get());
    VoxelHeader* d_heads = reinterpret_cast<VoxelHeader*>(h->voxel_ws.ptr.get() + maps_bytes);
    VoxelSpanDev* d_spans = reinterpret_cast<VoxelSpanDev*>(h->voxel_ws.ptr.get() + maps_bytes + heads_bytes);
    std::vector<VoxelHeader> heads(dmaps.size());
    HIP_TRY(hipMemcpyAsync(d_maps, dmaps.data(), sizeof(VoxelMapDev) * dmaps.size(), hipMemcpyHostToDevice, h->stream));
    launch_voxel_headers(d_maps, n_maps, d_heads, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(heads.data(), d_heads, sizeof(VoxelHeader) * heads.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_maps; i++)
        if (!voxel_header_matches(heads[(size_t)i], maps[i].params))
            return svo_set_error(SVO_ERR_INVALID, "svo_voxel_fuse: map %d was not cleared with these params", i);
    for (int i = 0; i < n_maps; i++)
        if (!voxel_load_ok(heads[(size_t)i].n_voxels, records[(size_t)i], maps[i].params.log2_capacity))
            return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_fuse: map %d: %llu voxels + %llu records exceed %llu (SVO_MAP_TOO_SMALL's rule: the bound)", i,
                                 heads[(size_t)i].n_voxels, (unsigned long long)records[(size_t)i],
                                 (unsigned long long)voxel_load_limit(maps[i].params.log2_capacity));
    if (dspans.empty()) return SVO_OK;
    HIP_TRY(hipMemcpyAsync(d_spans, dspans.data(), sizeof(VoxelSpanDev) * dspans.size(), hipMemcpyHostToDevice, h->stream));
    // (SVO_VOXEL_LANE_ATOMICS: the other form of the kernel, for tools/voxel_bench.py and the tests of its equality)
    const char* form = std::getenv("SVO_VOXEL_LANE_ATOMICS");
    launch_voxel_fuse(d_spans, (int)dspans.size(), tiles, d_maps, form && std::atoi(form) != 0, h->stream);
    return finish_launch(h);
}

// svo_voxel_extract and svo_voxel_pack: the kept entries of a map in key order as records out[0, *n_out), by the
// launcher that writes that kind of record (launch_voxel_extract, launch_voxel_pack). The checks, the count pass, the
// answer on a capacity too small and the staging are one code; `records`, `align` and `count`: what the entry calls its
// records and its count, and the alignment the records need.
template <class Record, class Launch>
static int voxel_read_out(svo_handle* h, const char* who, const svo_voxel_map* map, const svo_voxel_filter* filter, Record* out, const char* records,
                          uintptr_t align, const char* count, int64_t capacity, int64_t* n_out, Launch launch) {
    if (const int rc = check_map(map, who, 0)) return rc;
    if (!n_out) return svo_set_error(SVO_ERR_INVALID, "%s: no %s", who, count);
    if (filter && (filter->_reserved[0] != 0 || filter->_reserved[1] != 0)) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    if (out && (((uintptr_t)out & (align - 1)) || capacity < 0))
        return svo_set_error(SVO_ERR_INVALID, "%s: %s not %d-byte aligned, or capacity < 0", who, records, (int)align);
    const VoxelFilterDev f{filter ? std::max<uint32_t>(1u, filter->min_count) : 1u, filter ? filter->min_stamp : 0u};
    const VoxelMapDev mp = map_dev(map->data, map->params);
    VoxelHeader hd;
    HIP_TRY(hipMemcpyAsync(&hd, map->data, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!voxel_header_matches(hd, map->params)) return svo_set_error(SVO_ERR_INVALID, "%s: the map was not cleared with these params", who);
    if (const int rc = h->voxel_ws.reserve(voxel_offsets_bytes(mp.log2_capacity), h->stream)) return rc;
    int32_t* tile_offsets = reinterpret_cast<int32_t*>(h->voxel_ws.ptr.get());
    launch_voxel_count(mp, f, tile_offsets, h->stream);
    HIP_TRY(hipGetLastError());
    int32_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, tile_offsets + voxel_map_tiles(mp.log2_capacity), sizeof(kept), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n_out = kept;
    if (!out) return SVO_OK;
    if (!voxel_extract_fits(kept, capacity)) return svo_set_error(SVO_ERR_CAPACITY, "%s: %d voxels kept, capacity %lld", who, kept, (long long)capacity);
    if (kept == 0) return SVO_OK;
    size_t temp_bytes = 0;
    if (const int rc = voxel_sort_temp_bytes((size_t)kept, &temp_bytes)) return rc;
    const VoxelExtractPlan plan = voxel_extract_plan((uint64_t)kept, temp_bytes);
    if (const int rc = h->voxel_sort_ws.reserve(plan.bytes, h->stream)) return rc;
    uint8_t* ws = h->voxel_sort_ws.ptr.get();
    if (const int rc = launch(mp, f, tile_offsets, (size_t)kept, reinterpret_cast<uint64_t*>(ws + plan.keys_in),
                              reinterpret_cast<uint64_t*>(ws + plan.keys_out), reinterpret_cast<uint32_t*>(ws + plan.index_in),
                              reinterpret_cast<uint32_t*>(ws + plan.index_out), ws + plan.sort_temp, temp_bytes, out, h->stream))
        return rc;
    return finish_launch(h);
}

extern "C" int svo_voxel_extract(svo_handle* h, const svo_voxel_map* map, const svo_voxel_filter* filter, svo_map_point* points,
                                 int64_t capacity, int64_t* n_points) {
    CHECK_H(h);
    return voxel_read_out(h, "svo_voxel_extract", map, filter, points, "points", 16, "n_points", capacity, n_points, launch_voxel_extract);
}

extern "C" int svo_voxel_pack(svo_handle* h, const svo_voxel_map* map, const svo_voxel_filter* filter, svo_voxel_entry* entries,
                              int64_t capacity, int64_t* n) {
    CHECK_H(h);
    return voxel_read_out(h, "svo_voxel_pack", map, filter, entries, "entries", 8, "n", capacity, n, launch_voxel_pack);
}

extern "C" int svo_voxel_merge(svo_handle* h, int n_spans, const svo_voxel_entry_span* spans, int n_maps, const svo_voxel_map* maps,
                               svo_voxel_merge_result* results) {
    CHECK_H(h);
    if (n_spans < 0 || n_maps < 0 || (n_spans > 0 && !spans) || (n_maps > 0 && !maps))
        return svo_set_error(SVO_ERR_INVALID, "svo_voxel_merge: bad arguments");
    std::vector<VoxelMapDev> dmaps((size_t)n_maps);
    std::vector<const void*> seen;
    for (int i = 0; i < n_maps; i++) {
        if (const int rc = check_map(&maps[i], "svo_voxel_merge", i)) return rc;
        dmaps[(size_t)i] = map_dev(maps[i].data, maps[i].params);
        seen.push_back(maps[i].data);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_merge: a map is named twice");
    std::vector<VoxelEntrySpanDev> dspans;
    std::vector<std::vector<int64_t>> counts((size_t)n_maps);   // the spans' record counts per map, for the load bound
    int64_t tiles = 0;
    for (int i = 0; i < n_spans; i++) {
        const svo_voxel_entry_span& s = spans[i];
        if (!voxel_entry_span_ok((uintptr_t)s.entries, s.n))
            return svo_set_error(SVO_ERR_INVALID, "svo_voxel_merge: span %d: n < 0, or entries NULL or not 8-byte aligned", i);
        if (s.map < 0 || s.map >= n_maps) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_merge: span %d names map %d of %d", i, s.map, n_maps);
        if (!voxel_edge_same(s.voxel, maps[s.map].params.voxel))
            return svo_set_error(SVO_ERR_INVALID, "svo_voxel_merge: span %d: its keys were made with voxel %.9g, map %d has %.9g", i, (double)s.voxel, s.map,
                                 (double)maps[s.map].params.voxel);
        counts[(size_t)s.map].push_back(s.n);
        if (s.n == 0) continue;
        dspans.push_back(VoxelEntrySpanDev{s.entries, s.n, tiles, s.map, 0});
        tiles += voxel_entry_span_tiles(s.n);
        if (tiles > INT32_MAX) return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_merge: too many records for one call");
    }
    if (n_maps == 0) return SVO_OK;
    // the tables of the call: the maps, their headers as the device holds them now, the counts, the spans
    const size_t maps_bytes = voxel_up256(sizeof(VoxelMapDev) * dmaps.size()), heads_bytes = voxel_up256(sizeof(VoxelHeader) * dmaps.size());
    const size_t counts_bytes = voxel_up256(sizeof(VoxelMergeCounts) * dmaps.size());
    if (const int rc = h->voxel_ws.reserve(maps_bytes + heads_bytes + counts_bytes + voxel_up256(sizeof(VoxelEntrySpanDev) * dspans.size()), h->stream))
        return rc;
    uint8_t* ws = h->voxel_ws.ptr.get();
    VoxelMapDev* d_maps = reinterpret_cast<VoxelMapDev*>(ws);
    VoxelHeader* d_heads = reinterpret_cast<VoxelHeader*>(ws + maps_bytes);
    VoxelMergeCounts* d_counts = reinterpret_cast<VoxelMergeCounts*>(ws + maps_bytes + heads_bytes);
    VoxelEntrySpanDev* d_spans = reinterpret_cast<VoxelEntrySpanDev*>(ws + maps_bytes + heads_bytes + counts_bytes);
    std::vector<VoxelHeader> heads(dmaps.size());
    HIP_TRY(hipMemcpyAsync(d_maps, dmaps.data(), sizeof(VoxelMapDev) * dmaps.size(), hipMemcpyHostToDevice, h->stream));
    launch_voxel_headers(d_maps, n_maps, d_heads, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(heads.data(), d_heads, sizeof(VoxelHeader) * heads.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_maps; i++)
        if (!voxel_header_matches(heads[(size_t)i], maps[i].params))
            return svo_set_error(SVO_ERR_INVALID, "svo_voxel_merge: map %d was not cleared with these params", i);
    for (int i = 0; i < n_maps; i++)
        if (!voxel_merge_load_ok(heads[(size_t)i].n_voxels, counts[(size_t)i].data(), (int)counts[(size_t)i].size(), maps[i].params.log2_capacity))
            return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_merge: map %d: %llu voxels and the call's records exceed %llu (the load bound)", i,
                                 heads[(size_t)i].n_voxels, (unsigned long long)voxel_load_limit(maps[i].params.log2_capacity));
    if (dspans.empty()) {
        if (results) std::fill(results, results + n_maps, svo_voxel_merge_result{0, 0, 0, 0});
        return SVO_OK;
    }
    HIP_TRY(hipMemcpyAsync(d_spans, dspans.data(), sizeof(VoxelEntrySpanDev) * dspans.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(VoxelMergeCounts) * dmaps.size(), h->stream));
    launch_voxel_merge(d_spans, (int)dspans.size(), tiles, d_maps, d_counts, h->stream);
    HIP_TRY(hipGetLastError());
    std::vector<VoxelMergeCounts> got(dmaps.size());
    HIP_TRY(hipMemcpyAsync(got.data(), d_counts, sizeof(VoxelMergeCounts) * got.size(), hipMemcpyDeviceToHost, h->stream));
    if (const int rc = finish_launch(h)) return rc;
    if (results)
        for (int i = 0; i < n_maps; i++)
            results[i] = svo_voxel_merge_result{(int64_t)got[(size_t)i].n_offered, (int64_t)got[(size_t)i].n_merged, (int64_t)got[(size_t)i].n_skipped,
                                                (int64_t)got[(size_t)i].n_claimed};
    return SVO_OK;
}

extern "C" int svo_voxel_rehash(svo_handle* h, const svo_voxel_map* src, void* dst, int dst_log2_capacity) {
    CHECK_H(h);
    if (const int rc = check_map(src, "svo_voxel_rehash", 0)) return rc;
    if (!voxel_log2_ok(dst_log2_capacity, false))
        return svo_set_error(SVO_ERR_INVALID, "svo_voxel_rehash: dst_log2_capacity %d outside %d .. %d", dst_log2_capacity, VOXEL_LOG2_MIN, VOXEL_LOG2_MAX);
    if (!dst || ((uintptr_t)dst & 15)) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_rehash: dst is NULL or not 16-byte aligned");
    if (voxel_ranges_overlap((uintptr_t)src->data, voxel_map_bytes(src->params.log2_capacity), (uintptr_t)dst, voxel_map_bytes(dst_log2_capacity)))
        return svo_set_error(SVO_ERR_INVALID, "svo_voxel_rehash: dst shares bytes with the map it is made from");
    VoxelHeader hd;
    HIP_TRY(hipMemcpyAsync(&hd, src->data, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!voxel_header_matches(hd, src->params)) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_rehash: the map was not cleared with these params");
    if (!voxel_rehash_ok(hd.n_voxels, dst_log2_capacity))
        return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_rehash: %llu voxels exceed %llu, the load limit of log2_capacity %d", hd.n_voxels,
                             (unsigned long long)voxel_load_limit(dst_log2_capacity), dst_log2_capacity);
    svo_voxel_params to = src->params;
    to.log2_capacity = dst_log2_capacity;
    launch_voxel_rehash(map_dev(src->data, src->params), map_dev(dst, to), h->stream);
    return finish_launch(h);
}

namespace svo {

// the keep rule as the kernels take it, or why it is rejected; center_voxel: the three indices (0 without a box)
int voxel_check_keep(const svo_voxel_keep* keep, const float* center, float voxel, const char* who, VoxelKeepDev* out) {
    if (!keep) return svo_set_error(SVO_ERR_INVALID, "%s: no keep rule", who);
    if (keep->_reserved[0] != 0 || keep->_reserved[1] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved of the keep rule is not 0", who);
    *out = VoxelKeepDev{std::max<uint32_t>(1u, keep->min_count), keep->min_stamp, {0, 0, 0}, keep->radius < 0 ? -1 : keep->radius};
    if (keep->radius < 0) return SVO_OK;
    for (int j = 0; j < 3; j++)
        if (!voxel_center_index(center[j], voxel, out->c[j]))
            return svo_set_error(SVO_ERR_INVALID, "%s: the centre's coordinate %d (%g) is not finite or lies outside the map's key range", who, j,
                                 (double)center[j]);
    return SVO_OK;
}

}  // namespace svo

extern "C" int svo_voxel_prune(svo_handle* h, const svo_voxel_map* map, const svo_voxel_keep* keep, svo_voxel_prune_result* out) {
    CHECK_H(h);
    if (const int rc = check_map(map, "svo_voxel_prune", 0)) return rc;
    VoxelKeepDev f;
    if (const int rc = voxel_check_keep(keep, keep ? keep->center : nullptr, map->params.voxel, "svo_voxel_prune", &f)) return rc;
    const VoxelMapDev mp = map_dev(map->data, map->params);
    VoxelHeader hd;
    HIP_TRY(hipMemcpyAsync(&hd, map->data, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!voxel_header_matches(hd, map->params)) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_prune: the map was not cleared with these params");
    VoxelPrunePlan plan;
    if (hd.n_voxels > ((uint64_t)1 << mp.log2_capacity) || !voxel_prune_plan(hd.n_voxels, plan))
        return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_prune: staging %llu entries exceeds %zu bytes", hd.n_voxels, VOXEL_PRUNE_STAGING_MAX);
    // the tile offsets, then the staging block
    const size_t offsets_bytes = voxel_offsets_bytes(mp.log2_capacity);
    if (const int rc = h->voxel_ws.reserve(offsets_bytes + plan.bytes, h->stream)) return rc;
    int32_t* tile_offsets = reinterpret_cast<int32_t*>(h->voxel_ws.ptr.get());
    launch_voxel_prune(mp, f, tile_offsets, h->voxel_ws.ptr.get() + offsets_bytes, hd.n_voxels, h->stream);
    HIP_TRY(hipGetLastError());
    int32_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, tile_offsets + voxel_map_tiles(mp.log2_capacity), sizeof(kept), hipMemcpyDeviceToHost, h->stream));
    if (const int rc = finish_launch(h)) return rc;
    if (out) *out = svo_voxel_prune_result{(int64_t)hd.n_voxels, (int64_t)kept, {f.c[0], f.c[1], f.c[2]}, 0};
    return SVO_OK;
}

namespace svo {

// the scalar fields of a carve and the image size, or why they are rejected
int voxel_check_carve_rule(const svo_voxel_carve_rule* carve, int width, int height, const char* who) {
    if (!carve) return svo_set_error(SVO_ERR_INVALID, "%s: no carve", who);
    if (!voxel_carve_scalars_ok(carve->margin, carve->near, carve->ring, width, height))
        return svo_set_error(SVO_ERR_INVALID, "%s: margin must be finite and >= 0, near finite and > 0, ring 0 or 1, the image 1 .. 32768 pixels a side", who);
    if (carve->_reserved[0] != 0 || carve->_reserved[1] != 0 || carve->_reserved[2] != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved of the carve is not 0", who);
    return SVO_OK;
}

// the carve as the kernels take it, or why it is rejected; the camera and the occluder are checked by the AR entry's
// own functions
int voxel_check_carve(const svo_voxel_carve_rule* carve, const svo_ar_camera* camera, int width, int height, const svo_ar_occluder* occluder,
                      const char* who, VoxelCarveDev* out) {
    if (const int rc = voxel_check_carve_rule(carve, width, height, who)) return rc;
    if (const int rc = ar_check_camera(camera, who, 0)) return rc;
    if (const int rc = ar_check_occluder(occluder, who, 0)) return rc;
    const svo_ar_occluder& o = *occluder;
    *out = voxel_carve_dev(*carve, *camera, width, height, o.records, o.cols, o.rows, o.step);
    return SVO_OK;
}

// records == nullptr: no evidence anywhere (cols, rows and step are not used then)
VoxelCarveDev voxel_carve_dev(const svo_voxel_carve_rule& carve, const svo_ar_camera& camera, int width, int height, const svo_map_point* records,
                              int cols, int rows, int step) {
    VoxelCarveDev d{};
    memcpy(d.view, camera.view, sizeof(d.view));
    d.fx = camera.fx; d.fy = camera.fy; d.cx = camera.cx; d.cy = camera.cy;
    d.w = (float)width; d.h = (float)height;
    d.margin = carve.margin; d.near = carve.near;
    d.records = records;
    d.cols = records ? cols : 0; d.rows = records ? rows : 0; d.step = records ? step : 1;
    d.drop_flags = ((uint32_t)SVO_CLOUD_DROPPED | carve.drop_flags) & 0xffu;
    d.max_last = carve.max_last;
    d.ring = carve.ring;
    return d;
}

}  // namespace svo

extern "C" int svo_voxel_carve(svo_handle* h, const svo_voxel_map* map, const svo_ar_camera* camera, int width, int height,
                               const svo_ar_occluder* occluder, const svo_voxel_carve_rule* carve, const svo_voxel_keep* keep,
                               svo_voxel_carve_result* result) {
    CHECK_H(h);
    if (const int rc = check_map(map, "svo_voxel_carve", 0)) return rc;
    const svo_voxel_keep all{0u, 0u, {0.f, 0.f, 0.f}, -1, {0, 0}};   // keep == NULL: every entry is kept by the keep rule
    VoxelCarveRule rule{};
    if (const int rc = voxel_check_keep(keep ? keep : &all, keep ? keep->center : all.center, map->params.voxel, "svo_voxel_carve", &rule.keep)) return rc;
    if (const int rc = voxel_check_carve(carve, camera, width, height, occluder, "svo_voxel_carve", &rule.carve)) return rc;
    const VoxelMapDev mp = map_dev(map->data, map->params);
    VoxelHeader hd;
    HIP_TRY(hipMemcpyAsync(&hd, map->data, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!voxel_header_matches(hd, map->params)) return svo_set_error(SVO_ERR_INVALID, "svo_voxel_carve: the map was not cleared with these params");
    VoxelPrunePlan plan;
    if (hd.n_voxels > ((uint64_t)1 << mp.log2_capacity) || !voxel_prune_plan(hd.n_voxels, plan))
        return svo_set_error(SVO_ERR_CAPACITY, "svo_voxel_carve: staging %llu entries exceeds %zu bytes", hd.n_voxels, VOXEL_PRUNE_STAGING_MAX);
    // the prune's block (tile offsets, staging), then the ballot words and the counters
    const size_t offsets_bytes = voxel_offsets_bytes(mp.log2_capacity);
    const VoxelCarvePlan extra = voxel_carve_plan(mp.log2_capacity);
    if (const int rc = h->voxel_ws.reserve(offsets_bytes + plan.bytes + extra.bytes, h->stream)) return rc;
    uint8_t* ws = h->voxel_ws.ptr.get();
    int32_t* tile_offsets = reinterpret_cast<int32_t*>(ws);
    rule.ballots = reinterpret_cast<unsigned long long*>(ws + offsets_bytes + plan.bytes + extra.ballots);
    rule.counters = reinterpret_cast<unsigned long long*>(ws + offsets_bytes + plan.bytes + extra.counters);
    // (SVO_VOXEL_CARVE_REEVALUATE: the other form of the kernels, for tools/voxel_bench.py and the test of its equality:
    // no ballot words, the stage pass evaluates the carve again)
    const char* form = std::getenv("SVO_VOXEL_CARVE_REEVALUATE");
    if (form && std::atoi(form) != 0) rule.ballots = nullptr;
    launch_voxel_carve(mp, rule, tile_offsets, ws + offsets_bytes, hd.n_voxels, h->stream);
    HIP_TRY(hipGetLastError());
    int32_t kept = 0;
    unsigned long long counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&kept, tile_offsets + voxel_map_tiles(mp.log2_capacity), sizeof(kept), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(counts, rule.counters, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
    if (const int rc = finish_launch(h)) return rc;
    if (result) *result = svo_voxel_carve_result{(int64_t)hd.n_voxels, (int64_t)kept, (int64_t)counts[0], (int64_t)counts[1]};
    return SVO_OK;
}
