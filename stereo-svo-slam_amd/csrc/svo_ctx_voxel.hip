// svo_ctx_voxel.hip — the voxel maps of the ctx's slots (svo_ctx_state.hpp): giving slots a map, its info, and the
// queued jobs that fuse dense clouds into the maps, export them, clear them and prune them; "voxel entries": the queued
// jobs that save and load the maps' raw entries, and the setter that moves the maps into tables of another size.
#include <functional>

#include "svo_ctx_state.hpp"
#include "svo_voxel_plan.hpp"

extern "C" int svo_ctx_set_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_params* params) {
    if (!c || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_voxel_maps: bad arguments");
    if (params)
        if (const int rc = svo::voxel_check_params(params, true, "svo_ctx_set_voxel_maps")) return rc;
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_ctx_set_voxel_maps", slots)) return rc;
    if (const int rc = ctx_drain(c)) return rc;
    for (auto& wp : c->workers) {
        SlotList local;
        if (!slots.share(wp->first, wp->count, local, every_slot)) continue;
        if (const int rc = grp_set_voxel_maps(wp->g.get(), local.seqs.data(), (int)local.seqs.size(), params)) return rc;
    }
    return SVO_OK;
}

extern "C" int svo_get_voxel_map_info(svo_ctx* ctx, int seq, svo_voxel_map_info* info) {
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    if (!grp_voxel_map_info(g, s, info)) return svo_set_error(SVO_ERR_INVALID, "svo_get_voxel_map_info: slot %d has no voxel map", seq);
    return SVO_OK;
}

// svo_submit_fuse_clouds (sgm == null) and svo_submit_fuse_clouds_sgm
static int submit_fuse_clouds(svo_ctx* c, const char* who, int what, const int* seqs, int n, const svo_cloud_style* style,
                              const svo_sgm_params* sgm, const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info) {
    if (const int rc = drop_check_that_is_off(&check, true, who)) return rc;
    if (!c || !info || !what_ok(what) || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (what %d)", who, what);
    if (const int rc = grp_check_cloud_style(c->g0(), style, check)) return rc;
    if (sgm)
        if (const int rc = grp_check_cloud_sgm(c->g0(), style, sgm, who)) return rc;
    if (style->frame != SVO_CLOUD_WORLD || style->layout != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: frame must be SVO_CLOUD_WORLD and layout 0", who);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, who, slots)) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<svo_ctx::FuseClouds>(c, slots, every_slot, [&](svo_ctx::FuseClouds& e) {
        e.what = what; e.style = *style; e.stamp = stamp; e.info = info;
        e.set_check(check);
        e.set_sgm(sgm);
    });
    return SVO_OK;
}

extern "C" int svo_submit_fuse_clouds(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                      const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info) {
    return submit_fuse_clouds(c, "svo_submit_fuse_clouds", what, seqs, n, style, nullptr, check, stamp, info);
}

// the fuse job over SGM maps (include/svo_hip.h, "sgm fusion"): the same queue entry carrying the params
extern "C" int svo_submit_fuse_clouds_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                          const svo_sgm_params* sgm, const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info) {
    if (!sgm) return svo_submit_fuse_clouds(c, what, seqs, n, style, check, stamp, info);
    return submit_fuse_clouds(c, "svo_submit_fuse_clouds_sgm", what, seqs, n, style, sgm, check, stamp, info);
}

extern "C" int svo_fuse_clouds_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style, const svo_sgm_params* sgm,
                                   const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info) {
    return then_wait(c, svo_submit_fuse_clouds_sgm(c, what, seqs, n, style, sgm, check, stamp, info));
}

extern "C" int svo_fuse_clouds(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style, const svo_stereo_check* check,
                               uint32_t stamp, svo_fuse_info* info) {
    return then_wait(c, svo_submit_fuse_clouds(c, what, seqs, n, style, check, stamp, info));
}

// svo_submit_export_voxel_maps (J = VoxelExport: points, 16-byte aligned) and svo_submit_save_voxel_maps (J = VoxelSave:
// entry records, 8-byte aligned): the same regions, filter and segments; `records` is dst's array of them
template <typename J, typename Dst>
static int submit_voxel_out(svo_ctx* c, const char* who, const int* seqs, int n, const svo_voxel_region* regions, const svo_voxel_filter* filter,
                            const Dst* dst, const void* records, const char* what, uintptr_t align, int mem) {
    if (!c || !dst || !dst->segments || !mem_ok(mem) || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (mem %d)", who, mem);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (slots.n > 0 && !regions) return svo_set_error(SVO_ERR_INVALID, "%s: no regions", who);
    const svo_voxel_filter f = filter ? *filter : svo_voxel_filter{0, 0, {0, 0}};
    if (f._reserved[0] != 0 || f._reserved[1] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    if ((uintptr_t)records & (align - 1)) return svo_set_error(SVO_ERR_INVALID, "%s: %s is not %d-byte aligned", who, what, (int)align);
    const int rc = check_slots_and_items(c, who, slots, [&](int i) {
        const svo_voxel_region& r = regions[i];
        if (r.first_point < 0 || r.point_capacity < 0 || r._reserved[0] != 0 || r._reserved[1] != 0 || r._reserved[2] != 0)
            return svo_set_error(SVO_ERR_INVALID, "%s: region %d has a negative field or a non-zero _reserved", who, i);
        if (r.point_capacity > 0 && !records) return svo_set_error(SVO_ERR_INVALID, "%s: region %d has a capacity, but %s is NULL", who, i, what);
        return (int)SVO_OK;
    });
    if (rc) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<J>(c, slots, [&](J& e, int i, int) { e.regions.push_back(regions[i]); return true; },
                     [&](J& e) { e.mem = mem; e.filter = f; e.dst = *dst; });
    return SVO_OK;
}

extern "C" int svo_submit_export_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_region* regions,
                                            const svo_voxel_filter* filter, const svo_voxel_dst* dst, int mem) {
    return submit_voxel_out<svo_ctx::VoxelExport>(c, "svo_submit_export_voxel_maps", seqs, n, regions, filter, dst, dst ? dst->points : nullptr, "points", 16, mem);
}

extern "C" int svo_submit_save_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_region* regions,
                                          const svo_voxel_filter* filter, const svo_voxel_entry_dst* dst, int mem) {
    return submit_voxel_out<svo_ctx::VoxelSave>(c, "svo_submit_save_voxel_maps", seqs, n, regions, filter, dst, dst ? dst->entries : nullptr, "entries", 8, mem);
}

extern "C" int svo_save_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_region* regions, const svo_voxel_filter* filter,
                                   const svo_voxel_entry_dst* dst, int mem) {
    return then_wait(c, svo_submit_save_voxel_maps(c, seqs, n, regions, filter, dst, mem));
}

extern "C" int svo_submit_load_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_entry_span* spans, int mode, int mem,
                                          svo_voxel_load_info* info) {
    const char* who = "svo_submit_load_voxel_maps";
    if (!c || !info || !mem_ok(mem) || !naming_ok(seqs, n) || (mode != SVO_VOXEL_LOAD_REPLACE && mode != SVO_VOXEL_LOAD_MERGE))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (mode %d, mem %d)", who, mode, mem);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (slots.n > 0 && !spans) return svo_set_error(SVO_ERR_INVALID, "%s: no spans", who);
    const int rc = check_slots_and_items(c, who, slots, [&](int i) {
        const svo_voxel_entry_span& s = spans[i];
        if (!svo::voxel_entry_span_ok((uintptr_t)s.entries, s.n))
            return svo_set_error(SVO_ERR_INVALID, "%s: span %d: n < 0, or entries NULL or not 8-byte aligned", who, i);
        const int seq = slots.at(i);
        for (auto& wp : c->workers) {
            if (seq < wp->first || seq >= wp->first + wp->count) continue;
            const float voxel = grp_voxel_edge(wp->g.get(), seq - wp->first);
            if (voxel > 0.f && !svo::voxel_edge_same(s.voxel, voxel))
                return svo_set_error(SVO_ERR_INVALID, "%s: span %d: its keys were made with voxel %.9g, the map of slot %d has %.9g", who, i, (double)s.voxel,
                                     seq, (double)voxel);
        }
        return (int)SVO_OK;
    });
    if (rc) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<svo_ctx::VoxelLoad>(c, slots, [&](svo_ctx::VoxelLoad& e, int i, int) { e.spans.push_back(spans[i]); return true; },
                                      [&](svo_ctx::VoxelLoad& e) { e.mode = mode; e.mem = mem; e.info = info; });
    return SVO_OK;
}

extern "C" int svo_load_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_entry_span* spans, int mode, int mem,
                                   svo_voxel_load_info* info) {
    return then_wait(c, svo_submit_load_voxel_maps(c, seqs, n, spans, mode, mem, info));
}

extern "C" int svo_ctx_resize_voxel_maps(svo_ctx* c, const int* seqs, int n, int log2_capacity) {
    if (!c || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_resize_voxel_maps: bad arguments");
    if (!svo::voxel_log2_ok(log2_capacity, true))
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_resize_voxel_maps: log2_capacity %d outside %d .. %d", log2_capacity, svo::VOXEL_LOG2_MIN_CTX,
                             svo::VOXEL_LOG2_MAX);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_ctx_resize_voxel_maps", slots)) return rc;
    if (const int rc = ctx_drain(c)) return rc;
    // every group passes a phase before any enters the next: every slot fits, then every new map exists, before a map moves
    auto phase = [&](int ph) {
        int first = SVO_OK;
        for (auto& wp : c->workers) {
            SlotList local;
            if (!slots.share(wp->first, wp->count, local, every_slot)) continue;
            const int rc = grp_resize_voxel_maps(wp->g.get(), local.seqs.data(), (int)local.seqs.size(), log2_capacity, ph);
            if (rc && ph != VOXEL_RESIZE_ABORT) return rc;
            if (rc && !first) first = rc;
        }
        return first;
    };
    if (const int rc = phase(VOXEL_RESIZE_CHECK)) return rc;
    if (const int rc = phase(VOXEL_RESIZE_ALLOC)) {
        const std::string why = svo_last_error();
        phase(VOXEL_RESIZE_ABORT);
        return svo_set_error(rc, "%s", why.c_str());
    }
    return phase(VOXEL_RESIZE_MOVE);
}

extern "C" int svo_export_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_region* regions, const svo_voxel_filter* filter,
                                     const svo_voxel_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_voxel_maps(c, seqs, n, regions, filter, dst, mem));
}

extern "C" int svo_submit_clear_voxel_maps(svo_ctx* c, const int* seqs, int n) {
    if (!c || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_clear_voxel_maps: bad arguments");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_submit_clear_voxel_maps", slots)) return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_clear_voxel_maps");
    submit_shares<svo_ctx::VoxelClear>(c, slots, every_slot, nothing_more);
    return SVO_OK;
}

// svo_submit_prune_voxel_maps, and svo_submit_carve_voxel_maps through `more`, which fills what the entry carries besides
static int submit_prune(svo_ctx* c, const char* who, const int* seqs, int n, const svo_voxel_keep* keep, int center_mode, const float* centers,
                        const std::function<void(svo_ctx::VoxelPrune&)>& more) {
    if (keep->_reserved[0] != 0 || keep->_reserved[1] != 0) return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    const bool given = center_mode == SVO_PRUNE_CENTER_GIVEN && keep->radius >= 0;
    auto center_of = [&](int i) { return centers && center_mode == SVO_PRUNE_CENTER_GIVEN ? centers + 3 * (size_t)i : keep->center; };
    const int rc = check_slots_and_items(c, who, slots, [&](int i) {
        if (!given) return (int)SVO_OK;
        const int s = slots.at(i);
        for (auto& wp : c->workers) {
            if (s < wp->first || s >= wp->first + wp->count) continue;
            const float voxel = grp_voxel_edge(wp->g.get(), s - wp->first);
            int32_t ci;
            for (int j = 0; j < 3 && voxel > 0.f; j++)
                if (!svo::voxel_center_index(center_of(i)[j], voxel, ci))
                    return svo_set_error(SVO_ERR_INVALID, "%s: slot %d: the centre's coordinate %d (%g) is not finite or lies outside the map's key range",
                                         who, s, j, (double)center_of(i)[j]);
        }
        return (int)SVO_OK;
    });
    if (rc) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<svo_ctx::VoxelPrune>(c, slots,
                                       [&](svo_ctx::VoxelPrune& e, int i, int) {
                                           const float* at = center_of(i);
                                           e.centers.insert(e.centers.end(), at, at + 3);
                                           return true;
                                       },
                                       [&](svo_ctx::VoxelPrune& e) { e.keep = *keep; e.center_mode = center_mode; more(e); });
    return SVO_OK;
}

extern "C" int svo_submit_prune_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_keep* keep, int center_mode, const float* centers,
                                           svo_prune_info* info) {
    if (!c || !keep || !info || !naming_ok(seqs, n) || (center_mode != SVO_PRUNE_CENTER_GIVEN && center_mode != SVO_PRUNE_CENTER_POSE))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_prune_voxel_maps: bad arguments (center_mode %d)", center_mode);
    return submit_prune(c, "svo_submit_prune_voxel_maps", seqs, n, keep, center_mode, centers, [&](svo_ctx::VoxelPrune& e) { e.info = info; });
}

// the carve job (include/svo_hip.h, "voxel carve"): the prune entry carrying a carve
extern "C" int svo_submit_carve_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_cloud_style* cloud, const svo_sgm_params* sgm,
                                           const svo_stereo_check* check, const svo_voxel_carve_rule* carve, const svo_voxel_keep* keep,
                                           int center_mode, const float* centers, svo_carve_info* info) {
    const char* who = "svo_submit_carve_voxel_maps";
    if (const int rc = drop_check_that_is_off(&check, true, who)) return rc;
    if (!c || !info || !naming_ok(seqs, n) || (center_mode != SVO_PRUNE_CENTER_GIVEN && center_mode != SVO_PRUNE_CENTER_POSE))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (center_mode %d)", who, center_mode);
    if (const int rc = grp_check_cloud_style(c->g0(), cloud, check)) return rc;
    if (sgm)
        if (const int rc = grp_check_cloud_sgm(c->g0(), cloud, sgm, who)) return rc;
    if (cloud->frame != SVO_CLOUD_CAMERA || cloud->layout != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: cloud.frame %d must be SVO_CLOUD_CAMERA and cloud.layout %d must be 0", who, cloud->frame, cloud->layout);
    if (const int rc = svo::voxel_check_carve_rule(carve, 1, 1, who)) return rc;
    const svo_voxel_keep all{0u, 0u, {0.f, 0.f, 0.f}, -1, {0, 0}};
    return submit_prune(c, who, seqs, n, keep ? keep : &all, center_mode, centers, [&](svo_ctx::VoxelPrune& e) {
        e.has_carve = true; e.carve = *carve; e.cloud = *cloud; e.carve_info = info;
        e.set_check(check);
        e.set_sgm(sgm);
    });
}

extern "C" int svo_carve_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_cloud_style* cloud, const svo_sgm_params* sgm,
                                    const svo_stereo_check* check, const svo_voxel_carve_rule* carve, const svo_voxel_keep* keep, int center_mode,
                                    const float* centers, svo_carve_info* info) {
    return then_wait(c, svo_submit_carve_voxel_maps(c, seqs, n, cloud, sgm, check, carve, keep, center_mode, centers, info));
}

extern "C" int svo_prune_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_keep* keep, int center_mode, const float* centers,
                                    svo_prune_info* info) {
    return then_wait(c, svo_submit_prune_voxel_maps(c, seqs, n, keep, center_mode, centers, info));
}
