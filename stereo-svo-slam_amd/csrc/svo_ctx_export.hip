// svo_ctx_export.hip — the export jobs of the ctx (svo_ctx_state.hpp) and their blocking twins: the bulk export of
// frames and keyframes, the map, the views, dense disparity and clouds, the scene pictures and the AR pictures (with
// the copy of the caller's meshes that the groups share), and svo_map_size.
#include <cmath>

#include "svo_ctx_state.hpp"

extern "C" int svo_submit_export(svo_ctx* c, int what, const int* seqs, int n, const svo_export_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || !what_ok(what) || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export: bad arguments (what %d, mem %d)", what, mem);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_submit_export", slots)) return rc;
    for (const void* p : {(const void*)dst->kps2d, (const void*)dst->kps3d, (const void*)dst->info})
        if ((uintptr_t)p & 3) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export: an array is not 4-byte aligned");
    const int64_t per_seq = grp_capacity(c->g0());
    if ((dst->kps2d || dst->kps3d || dst->info) && dst->capacity < slots.n * per_seq)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export: %d slots need arrays of %lld records, capacity %lld", slots.n,
                             (long long)(slots.n * per_seq), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, "svo_submit_export");
    int64_t before = 0;                          // named slots of the groups so far
    submit_shares<svo_ctx::Export>(c, slots, every_slot, [&](svo_ctx::Export& e) {
        e.what = what; e.mem = mem; e.dst = *dst; e.base = before * per_seq;
        before += (int64_t)e.seqs.size();
    });
    return SVO_OK;
}

extern "C" int svo_export(svo_ctx* c, int what, const int* seqs, int n, const svo_export_dst* dst, int mem) {
    return then_wait(c, svo_submit_export(c, what, seqs, n, dst, mem));
}

extern "C" int svo_submit_export_map(svo_ctx* c, const int* seqs, int n, const svo_map_region* regions,
                                     const svo_map_filter* filter, const svo_map_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: bad arguments (mem %d)", mem);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (slots.n > 0 && !regions) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: no regions");
    const svo_map_filter f = filter ? *filter : svo_map_filter{0, 0, 0, 0};
    if ((f.drop_flags & ~(uint32_t)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY)) || f._reserved != 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: drop_flags 0x%x has unknown bits, or _reserved is not 0", f.drop_flags);
    if ((uintptr_t)dst->points & 15) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: points is not 16-byte aligned");
    const int rc = check_slots_and_items(c, "svo_submit_export_map", slots, [&](int i) {
        const svo_map_region& r = regions[i];
        if (r.first_point < 0 || r.point_capacity < 0 || r.first_keyframe_entry < 0 || r.keyframe_capacity < 0 || r.from_keyframe < 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: region %d has a negative field", i);
        if ((r.point_capacity > 0 && !dst->points) || (r.keyframe_capacity > 0 && !dst->keyframes))
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: region %d has a capacity, but its array is NULL", i);
        return (int)SVO_OK;
    });
    if (rc) return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_map");
    submit_shares<svo_ctx::MapExport>(c, slots, [&](svo_ctx::MapExport& e, int i, int) { e.regions.push_back(regions[i]); return true; },
                                      [&](svo_ctx::MapExport& e) { e.mem = mem; e.filter = f; e.dst = *dst; });
    return SVO_OK;
}

extern "C" int svo_export_map(svo_ctx* c, const int* seqs, int n, const svo_map_region* regions, const svo_map_filter* filter,
                              const svo_map_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_map(c, seqs, n, regions, filter, dst, mem));
}

extern "C" int svo_map_size(svo_ctx* ctx, int seq, int from_keyframe, int* keyframes, int64_t* points_bound) {
    if (from_keyframe < 0) return svo_set_error(SVO_ERR_INVALID, "svo_map_size: from_keyframe %d", from_keyframe);
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    grp_map_size(g, s, from_keyframe, keyframes, points_bound);
    return SVO_OK;
}

// ------------------------------------------------------------------ views, dense disparity, dense clouds

namespace {

// what a job of one image (planes, records) per named slot carries besides its slots
template <typename J, typename Style, typename Dst>
void submit_image_shares(svo_ctx* c, const NamedSlots& slots, int what, int mem, const Style* style, const svo_stereo_check* check,
                         const Dst* dst) {
    submit_shares<J>(c, slots, every_slot, [&](J& e) {
        e.what = what; e.mem = mem; e.style = *style; e.dst = *dst;
        if constexpr (std::is_base_of_v<svo_ctx::StereoCheck, J>) e.set_check(check);
    });
}

}  // namespace

extern "C" int svo_submit_export_views(svo_ctx* c, int what, const int* seqs, int n, const svo_view_style* style,
                                       const svo_view_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || !what_ok(what) || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_views: bad arguments (what %d, mem %d)", what, mem);
    if (const int rc = grp_check_view_style(c->g0(), style)) return rc;
    if (!dst->pixels || ((uintptr_t)dst->pixels & 3))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_views: pixels is NULL or not 4-byte aligned");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_submit_export_views", slots)) return rc;
    if (const int rc = check_capacity("svo_submit_export_views", slots.n, grp_view_bytes(c->g0(), style), dst->capacity, "bytes")) return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_views");
    submit_image_shares<svo_ctx::ViewExport>(c, slots, what, mem, style, nullptr, dst);
    return SVO_OK;
}

extern "C" int svo_export_views(svo_ctx* c, int what, const int* seqs, int n, const svo_view_style* style,
                                const svo_view_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_views(c, what, seqs, n, style, dst, mem));
}

// (the checked entries report under the unchecked entries' names, but for the check that is off)
extern "C" int svo_submit_export_disparity_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                                   const svo_stereo_check* check, const svo_disparity_dst* dst, int mem) {
    if (const int rc = drop_check_that_is_off(&check, false, "svo_submit_export_disparity_checked")) return rc;
    if (!c || !dst || !dst->segments || !what_ok(what) || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: bad arguments (what %d, mem %d)", what, mem);
    if (const int rc = grp_check_disparity_style(c->g0(), style, check)) return rc;
    if (!dst->values || ((uintptr_t)dst->values & 15))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: values is NULL or not 16-byte aligned");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_submit_export_disparity", slots)) return rc;
    if (const int rc = check_capacity("svo_submit_export_disparity", slots.n, grp_disparity_bytes(c->g0(), style, check), dst->capacity, "bytes"))
        return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_disparity");
    submit_image_shares<svo_ctx::DisparityExport>(c, slots, what, mem, style, check, dst);
    return SVO_OK;
}

extern "C" int svo_submit_export_disparity(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                           const svo_disparity_dst* dst, int mem) {
    return svo_submit_export_disparity_checked(c, what, seqs, n, style, nullptr, dst, mem);
}

extern "C" int svo_export_disparity(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                    const svo_disparity_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_disparity(c, what, seqs, n, style, dst, mem));
}

extern "C" int svo_export_disparity_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                            const svo_stereo_check* check, const svo_disparity_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_disparity_checked(c, what, seqs, n, style, check, dst, mem));
}

// the disparity job in its SGM mode (include/svo_hip.h, "sgm"): the same queue entry carrying the params, and with a
// check that is on ("sgm cross-check") the check beside them
namespace {

int submit_disparity_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style, const svo_sgm_params* sgm,
                         const svo_stereo_check* check, const svo_disparity_dst* dst, int mem, const char* who) {
    if (!c || !dst || !dst->segments || !what_ok(what) || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (what %d, mem %d)", who, what, mem);
    if (const int rc = grp_check_disparity_style(c->g0(), style, check)) return rc;
    if (const int rc = grp_check_disparity_sgm(c->g0(), style, sgm, who)) return rc;
    if (!dst->values || ((uintptr_t)dst->values & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: values is NULL or not 16-byte aligned", who);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, who, slots)) return rc;
    if (const int rc = check_capacity(who, slots.n, grp_disparity_bytes(c->g0(), style, check), dst->capacity, "bytes")) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<svo_ctx::DisparityExport>(c, slots, every_slot, [&](svo_ctx::DisparityExport& e) {
        e.what = what; e.mem = mem; e.style = *style; e.dst = *dst;
        e.has_sgm = true; e.sgm = *sgm;
        e.set_check(check);
    });
    return SVO_OK;
}

}  // namespace

extern "C" int svo_submit_export_disparity_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                               const svo_sgm_params* sgm, const svo_disparity_dst* dst, int mem) {
    return submit_disparity_sgm(c, what, seqs, n, style, sgm, nullptr, dst, mem, "svo_submit_export_disparity_sgm");
}

extern "C" int svo_export_disparity_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                        const svo_sgm_params* sgm, const svo_disparity_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_disparity_sgm(c, what, seqs, n, style, sgm, dst, mem));
}

extern "C" int svo_submit_export_disparity_sgm_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                                       const svo_sgm_params* sgm, const svo_stereo_check* check,
                                                       const svo_disparity_dst* dst, int mem) {
    if (const int rc = drop_check_that_is_off(&check, false, "svo_submit_export_disparity_sgm_checked")) return rc;
    if (!check) return svo_submit_export_disparity_sgm(c, what, seqs, n, style, sgm, dst, mem);
    return submit_disparity_sgm(c, what, seqs, n, style, sgm, check, dst, mem, "svo_submit_export_disparity_sgm_checked");
}

extern "C" int svo_export_disparity_sgm_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                                const svo_sgm_params* sgm, const svo_stereo_check* check, const svo_disparity_dst* dst,
                                                int mem) {
    return then_wait(c, svo_submit_export_disparity_sgm_checked(c, what, seqs, n, style, sgm, check, dst, mem));
}

// the cloud job over an SGM map ("sgm cross-check"): the cloud job's queue entry carrying the params and the check
extern "C" int svo_submit_export_cloud_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                           const svo_sgm_params* sgm, const svo_stereo_check* check, const svo_cloud_dst* dst, int mem) {
    const char* const who = "svo_submit_export_cloud_sgm";
    if (const int rc = drop_check_that_is_off(&check, true, who)) return rc;
    if (!c || !dst || !dst->segments || !what_ok(what) || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (what %d, mem %d)", who, what, mem);
    if (const int rc = grp_check_cloud_style(c->g0(), style, check)) return rc;
    if (const int rc = grp_check_cloud_sgm(c->g0(), style, sgm, who)) return rc;
    if (!dst->points || ((uintptr_t)dst->points & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: points is NULL or not 16-byte aligned", who);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, who, slots)) return rc;
    if (const int rc = check_capacity(who, slots.n, grp_cloud_points(c->g0(), style), dst->capacity, "records")) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<svo_ctx::CloudExport>(c, slots, every_slot, [&](svo_ctx::CloudExport& e) {
        e.what = what; e.mem = mem; e.style = *style; e.dst = *dst;
        e.has_sgm = true; e.sgm = *sgm;
        e.set_check(check);
    });
    return SVO_OK;
}

extern "C" int svo_export_cloud_sgm(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style, const svo_sgm_params* sgm,
                                    const svo_stereo_check* check, const svo_cloud_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_cloud_sgm(c, what, seqs, n, style, sgm, check, dst, mem));
}

extern "C" int svo_submit_export_cloud_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                               const svo_stereo_check* check, const svo_cloud_dst* dst, int mem) {
    if (const int rc = drop_check_that_is_off(&check, true, "svo_submit_export_cloud_checked")) return rc;
    if (!c || !dst || !dst->segments || !what_ok(what) || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_cloud: bad arguments (what %d, mem %d)", what, mem);
    if (const int rc = grp_check_cloud_style(c->g0(), style, check)) return rc;
    if (!dst->points || ((uintptr_t)dst->points & 15))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_cloud: points is NULL or not 16-byte aligned");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_submit_export_cloud", slots)) return rc;
    if (const int rc = check_capacity("svo_submit_export_cloud", slots.n, grp_cloud_points(c->g0(), style), dst->capacity, "records")) return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_cloud");
    submit_image_shares<svo_ctx::CloudExport>(c, slots, what, mem, style, check, dst);
    return SVO_OK;
}

extern "C" int svo_submit_export_cloud(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                       const svo_cloud_dst* dst, int mem) {
    return svo_submit_export_cloud_checked(c, what, seqs, n, style, nullptr, dst, mem);
}

extern "C" int svo_export_cloud(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                const svo_cloud_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_cloud(c, what, seqs, n, style, dst, mem));
}

extern "C" int svo_export_cloud_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                        const svo_stereo_check* check, const svo_cloud_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_cloud_checked(c, what, seqs, n, style, check, dst, mem));
}

// ------------------------------------------------------------------ scene pictures

extern "C" int svo_submit_export_scenes(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                        const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    return svo_submit_export_scenes_clouds(c, seqs, n, style, nullptr, cameras, dst, mem);
}

// svo_submit_export_scenes_clouds (sgm == null) and svo_submit_export_scenes_clouds_sgm, whose params are checked
// whatever clouds->live says and used by the live layer only
static int submit_scenes_clouds(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style, const svo_scene_clouds* clouds,
                                const svo_sgm_params* sgm, const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    if (sgm) {
        const char* const who = "svo_submit_export_scenes_clouds_sgm";
        if (const int rc = svo::sgm_check_params(sgm, who, nullptr)) return rc;
        if (c && clouds && clouds->live == 1) {
            if (const int rc = grp_check_scene_clouds(c->g0(), clouds)) return rc;
            if (const int rc = grp_check_cloud_sgm(c->g0(), &clouds->cloud, sgm, who)) return rc;
        } else {
            sgm = nullptr;
        }
    }
    if (clouds && clouds->live == 0 && !clouds->extra) {             // (nothing to draw: the plain job, once the clouds are checked)
        if (c)
            if (const int rc = grp_check_scene_clouds(c->g0(), clouds)) return rc;
        clouds = nullptr;
    }
    if (!c || !dst || !dst->segments || !cameras || !mem_ok(mem) || !naming_ok(seqs, n))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes: bad arguments (mem %d)", mem);
    if (const int rc = svo::scene_check_style(style, "svo_submit_export_scenes")) return rc;
    if (!dst->pixels || ((uintptr_t)dst->pixels & 3))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes: pixels is NULL or not 4-byte aligned");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots_and_items(c, "svo_submit_export_scenes", slots,
                                             [&](int i) { return svo::scene_check_camera(&cameras[i], "svo_submit_export_scenes", i); }))
        return rc;
    if (clouds) {
        if (const int rc = grp_check_scene_clouds(c->g0(), clouds)) return rc;
        for (int i = 0; clouds->extra && i < slots.n; i++)
            if (!svo::scene_span_ok((uintptr_t)clouds->extra[i].points, clouds->extra[i].n))
                return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes_clouds: span %d: n %lld must be >= 0 and its records device memory, 16-byte aligned",
                                     i, (long long)clouds->extra[i].n);
    }
    if (const int rc = check_capacity("svo_submit_export_scenes", slots.n, grp_scene_bytes(style), dst->capacity, "bytes")) return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_scenes");
    submit_shares<svo_ctx::SceneExport>(c, slots, [&](svo_ctx::SceneExport& e, int i, int) {
        e.cameras.push_back(cameras[i]);
        if (clouds && clouds->extra) e.extra.push_back(clouds->extra[i]);
        return true;
    }, [&](svo_ctx::SceneExport& e) {
        e.mem = mem; e.style = *style; e.dst = *dst;
        if (clouds) { e.has_clouds = true; e.clouds = *clouds; }
        e.set_sgm(sgm);
    });
    return SVO_OK;
}

extern "C" int svo_submit_export_scenes_clouds(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                               const svo_scene_clouds* clouds, const svo_scene_camera* cameras, const svo_scene_dst* dst,
                                               int mem) {
    return submit_scenes_clouds(c, seqs, n, style, clouds, nullptr, cameras, dst, mem);
}

// the scene job whose live layer is the cloud of SGM maps (include/svo_hip.h, "sgm scene clouds")
extern "C" int svo_submit_export_scenes_clouds_sgm(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                                   const svo_scene_clouds* clouds, const svo_sgm_params* sgm,
                                                   const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    return submit_scenes_clouds(c, seqs, n, style, clouds, sgm, cameras, dst, mem);
}

extern "C" int svo_export_scenes_clouds_sgm(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style, const svo_scene_clouds* clouds,
                                            const svo_sgm_params* sgm, const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_scenes_clouds_sgm(c, seqs, n, style, clouds, sgm, cameras, dst, mem));
}

extern "C" int svo_export_scenes(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                 const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_scenes(c, seqs, n, style, cameras, dst, mem));
}

extern "C" int svo_export_scenes_clouds(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style, const svo_scene_clouds* clouds,
                                        const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_scenes_clouds(c, seqs, n, style, clouds, cameras, dst, mem));
}

// ------------------------------------------------------------------ AR pictures

// svo_submit_export_ar (occlusion == null), svo_submit_export_ar_occluded (sgm == null) and
// svo_submit_export_ar_occluded_sgm, whose params are checked whatever occlusion->on says and used with on == 1 only
static int submit_export_ar(svo_ctx* c, const char* who, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                            const svo_sgm_params* sgm, const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances, const int* first, int n_instances,
                            const svo_ar_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || !mem_ok(mem) || !naming_ok(seqs, n) || n_meshes < 0 ||
        n_instances < 0 || (n_meshes > 0 && !meshes) || (n_instances > 0 && !instances))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (mem %d, %d meshes, %d instances)", who, mem, n_meshes, n_instances);
    if (const int rc = svo::ar_check_style(style, who)) return rc;
    if (const int rc = grp_check_ar_occlusion(c->g0(), occlusion)) return rc;
    if (sgm) {
        if (const int rc = svo::sgm_check_params(sgm, who, nullptr)) return rc;
        if (occlusion && occlusion->on == 1) {
            if (const int rc = grp_check_cloud_sgm(c->g0(), &occlusion->cloud, sgm, who)) return rc;
        } else {
            sgm = nullptr;
        }
    }
    if (!dst->pixels || ((uintptr_t)dst->pixels & 3)) return svo_set_error(SVO_ERR_INVALID, "%s: pixels is NULL or not 4-byte aligned", who);
    const NamedSlots slots = ctx_slots(c, seqs, n);
    n = slots.n;
    if (const int rc = check_slots(c, who, slots)) return rc;
    if (first) {
        if (first[0] < 0 || first[n] != n_instances)
            return svo_set_error(SVO_ERR_INVALID, "%s: first starts at %d and ends at %d, not at >= 0 and %d", who, first[0], first[n], n_instances);
        for (int i = 0; i < n; i++)
            if (first[i + 1] < first[i]) return svo_set_error(SVO_ERR_INVALID, "%s: first does not ascend at %d", who, i);
    }
    auto job = std::make_shared<ArJob>();
    job->style = *style;
    for (int m = 0; m < n_meshes; m++) {
        const svo_ar_mesh& me = meshes[m];
        if (me.n_vertices < 0 || me.n_triangles < 0 || me._reserved != 0 || (me.n_vertices > 0 && !me.vertices) || (me.n_triangles > 0 && !me.triangles))
            return svo_set_error(SVO_ERR_INVALID, "%s: mesh %d: a negative count, a missing array, or _reserved is not 0", who, m);
        for (int64_t k = 0; k < (int64_t)me.n_triangles * 3; k++)
            if (me.triangles[k] < 0 || me.triangles[k] >= me.n_vertices)
                return svo_set_error(SVO_ERR_INVALID, "%s: mesh %d: triangle %lld names vertex %d of %d", who, m, (long long)(k / 3), me.triangles[k], me.n_vertices);
        for (int k = 0; me.rgb && k < me.n_triangles; k++)
            if (me.rgb[k] >> 24) return svo_set_error(SVO_ERR_INVALID, "%s: mesh %d: a colour is r << 16 | g << 8 | b", who, m);
        job->meshes.push_back(ArJob::Mesh{job->vertices.size() / 3, job->triangles.size() / 3, job->rgb.size(), me.n_vertices, me.n_triangles, me.rgb != nullptr});
        job->vertices.insert(job->vertices.end(), me.vertices, me.vertices + (size_t)me.n_vertices * 3);
        job->triangles.insert(job->triangles.end(), me.triangles, me.triangles + (size_t)me.n_triangles * 3);
        if (me.rgb) job->rgb.insert(job->rgb.end(), me.rgb, me.rgb + me.n_triangles);
    }
    std::vector<int64_t> tri_before((size_t)n_instances + 1, 0);     // triangles of the instances before each
    for (int k = 0; k < n_instances; k++) {
        const svo_ar_instance& in = instances[k];
        bool finite = true;
        for (float v : in.model) finite = finite && std::isfinite(v);
        if (!finite || in.mesh < 0 || in.mesh >= n_meshes || (in.rgb >> 24) || in._reserved[0] != 0 || in._reserved[1] != 0)
            return svo_set_error(SVO_ERR_INVALID, "%s: instance %d: a model entry that is not finite, mesh %d of %d, a colour with a top byte, or a _reserved that is not 0", who, k, in.mesh, n_meshes);
        tri_before[(size_t)k + 1] = tri_before[(size_t)k] + meshes[in.mesh].n_triangles;
    }
    job->instances.assign(instances, instances + n_instances);
    for (int i = 0; i < n; i++) {
        const int64_t tri = first ? tri_before[(size_t)first[i + 1]] - tri_before[(size_t)first[i]] : tri_before[(size_t)n_instances];
        if (tri > SVO_AR_MAX_TRIANGLES)
            return svo_set_error(SVO_ERR_CAPACITY, "%s: named slot %d shows %lld triangles, at most %d", who, i, (long long)tri, (int)SVO_AR_MAX_TRIANGLES);
    }
    if (const int rc = check_capacity(who, n, grp_ar_bytes(c->g0(), style), dst->capacity, "bytes")) return rc;
    if (c->failed.load()) return reject_failed(c, who);
    submit_shares<svo_ctx::ArExport>(c, slots, [&](svo_ctx::ArExport& e, int i, int) {
        e.inst0.push_back(first ? first[i] : 0); e.inst1.push_back(first ? first[i + 1] : n_instances);
        return true;
    }, [&](svo_ctx::ArExport& e) {
        e.mem = mem; e.job = job; e.dst = *dst;
        if (occlusion && occlusion->on == 1) { e.occluded = true; e.occlusion = *occlusion; }
        e.set_sgm(sgm);
    });
    return SVO_OK;
}

extern "C" int svo_submit_export_ar(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_mesh* meshes,
                                    int n_meshes, const svo_ar_instance* instances, const int* first, int n_instances,
                                    const svo_ar_dst* dst, int mem) {
    return submit_export_ar(c, "svo_submit_export_ar", seqs, n, style, nullptr, nullptr, meshes, n_meshes, instances, first, n_instances, dst, mem);
}

extern "C" int svo_submit_export_ar_occluded(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                                             const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances, const int* first,
                                             int n_instances, const svo_ar_dst* dst, int mem) {
    return submit_export_ar(c, "svo_submit_export_ar_occluded", seqs, n, style, occlusion, nullptr, meshes, n_meshes, instances, first, n_instances, dst, mem);
}

// the occluded job behind the depth of SGM maps (include/svo_hip.h, "sgm ar occlusion")
extern "C" int svo_submit_export_ar_occluded_sgm(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                                                 const svo_sgm_params* sgm, const svo_ar_mesh* meshes, int n_meshes,
                                                 const svo_ar_instance* instances, const int* first, int n_instances, const svo_ar_dst* dst,
                                                 int mem) {
    if (!sgm) return svo_submit_export_ar_occluded(c, seqs, n, style, occlusion, meshes, n_meshes, instances, first, n_instances, dst, mem);
    return submit_export_ar(c, "svo_submit_export_ar_occluded_sgm", seqs, n, style, occlusion, sgm, meshes, n_meshes, instances, first, n_instances,
                            dst, mem);
}

extern "C" int svo_export_ar_occluded_sgm(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                                          const svo_sgm_params* sgm, const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances,
                                          const int* first, int n_instances, const svo_ar_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_ar_occluded_sgm(c, seqs, n, style, occlusion, sgm, meshes, n_meshes, instances, first, n_instances, dst, mem));
}

extern "C" int svo_export_ar_occluded(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                                      const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances, const int* first, int n_instances,
                                      const svo_ar_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_ar_occluded(c, seqs, n, style, occlusion, meshes, n_meshes, instances, first, n_instances, dst, mem));
}

extern "C" int svo_export_ar(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_mesh* meshes, int n_meshes,
                             const svo_ar_instance* instances, const int* first, int n_instances, const svo_ar_dst* dst, int mem) {
    return then_wait(c, svo_submit_export_ar(c, seqs, n, style, meshes, n_meshes, instances, first, n_instances, dst, mem));
}
