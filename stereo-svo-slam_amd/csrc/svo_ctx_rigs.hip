// svo_ctx_rigs.hip — the cameras of the ctx (svo_ctx_state.hpp): its own calibration or rectification maps, and the
// table of camera rigs that slots are bound to (add, add calibrated, remove, assign, read out).
#include <algorithm>
#include <cmath>

#include "svo_ctx_state.hpp"

namespace {

// the kernel blocks of n (left, right) camera pairs, left[i] then right[i]: host only, the validation of every entry
// that takes calibrations
int rig_cameras(const char* who, const svo_ctx* c, const svo_camera_calibration* left, const svo_camera_calibration* right,
                int n, std::vector<svo::RigCam>& cams) {
    const long long tiles = (long long)((c->width + svo::REMAP_TILE - 1) / svo::REMAP_TILE) * ((c->height + svo::REMAP_TILE - 1) / svo::REMAP_TILE);
    if (tiles * 2 * n >= svo::RIG_MAX_WORKGROUPS) return svo_set_error(SVO_ERR_INVALID, "%s: %d rigs are too many for one call", who, n);
    cams.resize(2 * (size_t)n);
    for (int i = 0; i < n; i++)
        for (int side = 0; side < 2; side++)
            if (!svo::rig_camera(side ? right[i] : left[i], cams[2 * (size_t)i + side]))
                return svo_set_error(SVO_ERR_INVALID, "%s: rig %d, %s camera: a value is not finite, or P R has no inverse", who, i,
                                     side ? "right" : "left");
    return SVO_OK;
}

// the maps of cams.size() / 2 rigs in the kernels' form, out[i] = left map | right map, straight from the calibrations:
// one table upload, one launch, one synchronise for all of them; no float plane. A failure leaves `out` empty.
int build_calibrated_maps(svo_ctx* c, std::vector<svo::RigCam>& cams, std::vector<svo::DevPtr<uint8_t>>& out) {
    const size_t n = cams.size() / 2, map_bytes = svo::remap_map_bytes(c->width, c->height);
    std::vector<svo::DevPtr<uint8_t>> made(n);
    for (size_t i = 0; i < n; i++) {
        HIP_TRY(svo::dev_malloc(made[i], 2 * map_bytes));     // (per rig: svo_ctx_remove_rigs frees one)
        cams[2 * i].fixed = made[i].get();
        cams[2 * i + 1].fixed = made[i].get() + map_bytes;
    }
    if (n == 0) return SVO_OK;
    svo::DevPtr<svo::RigCam> table;
    HIP_TRY(svo::dev_malloc(table, sizeof(svo::RigCam) * cams.size()));
    svo::Stream st;
    HIP_TRY(svo::make_stream(st));
    HIP_TRY(hipMemcpyAsync(table.get(), cams.data(), sizeof(svo::RigCam) * cams.size(), hipMemcpyHostToDevice, st.get()));
    svo::launch_rig_maps(table.get(), (int)cams.size(), c->width, c->height, true, st.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st.get()));
    out = std::move(made);
    return SVO_OK;
}

}  // namespace

extern "C" int svo_ctx_set_calibration(svo_ctx* c, const svo_camera_calibration* left, const svo_camera_calibration* right) {
    if (!c || (left != nullptr) != (right != nullptr))
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_calibration: give both calibrations or none");
    if (!left) return svo_ctx_set_rectification(c, nullptr, nullptr, nullptr, nullptr, SVO_MEM_HOST);
    std::vector<svo::RigCam> cams;
    if (const int e = rig_cameras("svo_ctx_set_calibration", c, left, right, 1, cams)) return e;
    const int rc = ctx_drain(c);                  // (the groups are idle from here on: no frame reads the old maps)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the new set is built completely before it replaces the old one: a failure leaves the old setting
    std::vector<svo::DevPtr<uint8_t>> made;
    if (const int e = build_calibrated_maps(c, cams, made)) return e;
    const size_t map_bytes = svo::remap_map_bytes(c->width, c->height);
    for (int side = 0; side < 2; side++) c->rect[side] = svo::remap_map_view(made[0].get() + side * map_bytes, c->width, c->height);
    c->rect_mem = std::move(made[0]);             // (frees the previous set)
    for (auto& w : c->workers) grp_set_rectification(w->g.get(), c->rect);
    return SVO_OK;
}

extern "C" int svo_ctx_set_rectification(svo_ctx* c, const float* left_map_x, const float* left_map_y,
                                         const float* right_map_x, const float* right_map_y, int mem) {
    const float* maps[4] = {left_map_x, left_map_y, right_map_x, right_map_y};
    const int given = (int)std::count_if(maps, maps + 4, [](const float* p) { return p != nullptr; });
    if (!c || (given != 0 && given != 4) || !mem_ok(mem))
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_rectification: give all four maps or none, mem host or device");
    const int rc = ctx_drain(c);                  // (the groups are idle from here on: no frame reads the old maps)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (given == 0) {
        for (auto& w : c->workers) grp_set_rectification(w->g.get(), nullptr);
        c->rect_mem.reset();
        return SVO_OK;
    }
    // the new set is built completely before it replaces the old one: a failure leaves the old setting
    const size_t map_bytes = svo::remap_map_bytes(c->width, c->height);
    const size_t plane = sizeof(float) * (size_t)c->width * c->height;
    svo::DevPtr<uint8_t> mem_new;
    HIP_TRY(svo::dev_malloc(mem_new, 2 * map_bytes + (mem == SVO_MEM_HOST ? 4 * plane : 0)));
    svo::Stream st;                               // (uploads and conversion ordered on one stream of their own)
    HIP_TRY(svo::make_stream(st));
    const float* dev_maps[4];
    for (int i = 0; i < 4; i++) {
        if (mem == SVO_MEM_HOST) {
            float* d = reinterpret_cast<float*>(mem_new.get() + 2 * map_bytes + i * plane);
            HIP_TRY(hipMemcpyAsync(d, maps[i], plane, hipMemcpyHostToDevice, st.get()));
            dev_maps[i] = d;
        } else {
            dev_maps[i] = maps[i];
        }
    }
    svo::RemapMap rect[2];
    for (int side = 0; side < 2; side++) {
        rect[side] = svo::remap_map_view(mem_new.get() + side * map_bytes, c->width, c->height);
        svo::launch_remap_prep(dev_maps[2 * side], dev_maps[2 * side + 1], rect[side], st.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st.get()));
    c->rect[0] = rect[0];
    c->rect[1] = rect[1];
    c->rect_mem = std::move(mem_new);             // (frees the previous set)
    for (auto& w : c->workers) grp_set_rectification(w->g.get(), c->rect);
    return SVO_OK;
}

// ------------------------------------------------------------------ camera rigs

namespace {

// the four float maps of a rig (host or device memory) into the kernels' form: left map | right map in `out`
int build_rig_maps(svo_ctx* c, const float* const maps[4], int mem, svo::DevPtr<uint8_t>& out) {
    const size_t map_bytes = svo::remap_map_bytes(c->width, c->height);
    const size_t plane = sizeof(float) * (size_t)c->width * c->height;
    svo::DevPtr<uint8_t> mem_new, stage;
    HIP_TRY(svo::dev_malloc(mem_new, 2 * map_bytes));
    if (mem == SVO_MEM_HOST) HIP_TRY(svo::dev_malloc(stage, 4 * plane));
    svo::Stream st;                               // (uploads and conversion ordered on one stream of their own)
    HIP_TRY(svo::make_stream(st));
    const float* dev_maps[4];
    for (int i = 0; i < 4; i++) {
        dev_maps[i] = maps[i];
        if (mem != SVO_MEM_HOST) continue;
        float* d = reinterpret_cast<float*>(stage.get() + i * plane);
        HIP_TRY(hipMemcpyAsync(d, maps[i], plane, hipMemcpyHostToDevice, st.get()));
        dev_maps[i] = d;
    }
    for (int side = 0; side < 2; side++) {
        svo::launch_remap_prep(dev_maps[2 * side], dev_maps[2 * side + 1],
                               svo::remap_map_view(mem_new.get() + side * map_bytes, c->width, c->height), st.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st.get()));
    out = std::move(mem_new);
    return SVO_OK;
}

bool rig_exists(const svo_ctx* c, int id) { return id >= 0 && id < (int)c->rigs.size() && c->rigs[id].used; }

// the checks both ways of adding rigs share: the ten floats, all four maps or none, mem, _reserved
int check_rigs(const char* who, const svo_rig* rigs, int n) {
    for (int i = 0; i < n; i++) {
        const svo_rig& r = rigs[i];
        const float v[10] = {r.baseline, r.fx, r.fy, r.cx, r.cy, r.k1, r.k2, r.k3, r.p1, r.p2};
        for (float x : v)
            if (!std::isfinite(x)) return svo_set_error(SVO_ERR_INVALID, "%s: rig %d has a value that is not finite", who, i);
        if (!(r.fx > 0) || !(r.fy > 0)) return svo_set_error(SVO_ERR_INVALID, "%s: rig %d: fx and fy must be positive", who, i);
        const int given = (r.left_map_x != nullptr) + (r.left_map_y != nullptr) + (r.right_map_x != nullptr) + (r.right_map_y != nullptr);
        if ((given != 0 && given != 4) || (given == 4 && !mem_ok(r.mem)) || r._reserved != 0)
            return svo_set_error(SVO_ERR_INVALID, "%s: rig %d: give all four maps or none, mem host or device, _reserved 0", who, i);
    }
    return SVO_OK;
}

// a rig of the ctx with the ten floats of `r` (no maps yet)
svo_ctx::Rig new_rig(const svo_ctx* c, const svo_rig& r) {
    svo_ctx::Rig out;
    svo_camera_settings& s = out.cam;
    s = c->rigs[0].cam;                          // (the integer settings stay the ctx's)
    s.baseline = r.baseline; s.fx = r.fx; s.fy = r.fy; s.cx = r.cx; s.cy = r.cy;
    s.k1 = r.k1; s.k2 = r.k2; s.k3 = r.k3; s.p1 = r.p1; s.p2 = r.p2;
    out.used = true;
    return out;
}

}  // namespace

extern "C" int svo_ctx_add_rigs(svo_ctx* c, const svo_rig* rigs, int n, int* ids) {
    if (!c || n < 0 || (n > 0 && (!rigs || !ids))) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_add_rigs: bad arguments");
    if (const int e = check_rigs("svo_ctx_add_rigs", rigs, n)) return e;
    const int rc = ctx_drain(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // every rig is built before any is added: a failure adds nothing
    std::vector<svo_ctx::Rig> made((size_t)n);
    for (int i = 0; i < n; i++) {
        const svo_rig& r = rigs[i];
        made[i] = new_rig(c, r);
        if (!r.left_map_x) continue;
        const float* const maps[4] = {r.left_map_x, r.left_map_y, r.right_map_x, r.right_map_y};
        if (const int e = build_rig_maps(c, maps, r.mem, made[i].maps)) return e;
    }
    for (int i = 0; i < n; i++) {
        ids[i] = (int)c->rigs.size();
        c->rigs.push_back(std::move(made[i]));
    }
    return SVO_OK;
}

extern "C" int svo_ctx_add_rigs_calibrated(svo_ctx* c, const svo_rig* rigs, const svo_camera_calibration* left,
                                           const svo_camera_calibration* right, int n, int* ids) {
    const char* who = "svo_ctx_add_rigs_calibrated";
    if (!c || n < 0 || (n > 0 && (!rigs || !left || !right || !ids))) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments", who);
    if (const int e = check_rigs(who, rigs, n)) return e;
    for (int i = 0; i < n; i++)
        if (rigs[i].left_map_x) return svo_set_error(SVO_ERR_INVALID, "%s: rig %d: the maps come from the calibrations, the map pointers are NULL", who, i);
    std::vector<svo::RigCam> cams;
    if (const int e = rig_cameras(who, c, left, right, n, cams)) return e;
    const int rc = ctx_drain(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // every rig is built before any is added: a failure adds nothing
    std::vector<svo::DevPtr<uint8_t>> maps;
    if (const int e = build_calibrated_maps(c, cams, maps)) return e;
    for (int i = 0; i < n; i++) {
        svo_ctx::Rig r = new_rig(c, rigs[i]);
        r.maps = std::move(maps[i]);
        ids[i] = (int)c->rigs.size();
        c->rigs.push_back(std::move(r));
    }
    return SVO_OK;
}

extern "C" int svo_ctx_remove_rigs(svo_ctx* c, const int* ids, int n) {
    if (!c || n < 0 || (n > 0 && !ids)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_remove_rigs: bad arguments");
    const int rc = ctx_drain(c);                  // (the groups are idle from here on: no frame reads the maps)
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        if (ids[i] == 0 || !rig_exists(c, ids[i]))
            return svo_set_error(SVO_ERR_INVALID, "svo_ctx_remove_rigs: rig %d is rig 0 or does not exist", ids[i]);
        if (std::find(c->slot_rig.begin(), c->slot_rig.end(), ids[i]) != c->slot_rig.end())
            return svo_set_error(SVO_ERR_INVALID, "svo_ctx_remove_rigs: a slot is bound to rig %d", ids[i]);
    }
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < n; i++) {
        c->rigs[ids[i]].used = false;
        c->rigs[ids[i]].maps.reset();
    }
    return SVO_OK;
}

extern "C" int svo_ctx_assign_rigs(svo_ctx* c, const int* seqs, const int* rigs, int n) {
    if (!c || n < 0 || (n > 0 && (!seqs || !rigs))) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_assign_rigs: bad arguments");
    const NamedSlots slots{seqs, n};
    const int bad = slots.first_bad(c->B, false);
    for (int i = 0; i < n; i++) {                // (a slot's name is checked before its rig; it may be named twice)
        if (i == bad)
            return svo_set_error(SVO_ERR_INVALID, "svo_ctx_assign_rigs: sequence %d out of range", seqs[i]);
        if (!rig_exists(c, rigs[i])) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_assign_rigs: rig %d does not exist", rigs[i]);
    }
    if (c->failed.load()) return reject_failed(c, "svo_ctx_assign_rigs");
    const size_t map_bytes = svo::remap_map_bytes(c->width, c->height);
    submit_shares<svo_ctx::RigAssign>(c, slots, [&](svo_ctx::RigAssign& job, int i, int) {
        const svo_ctx::Rig& r = c->rigs[rigs[i]];
        const uint8_t* base = r.maps.get();
        job.bindings.push_back(RigBinding{rigs[i], r.cam, {base, base ? base + map_bytes : nullptr}});
        return true;
    }, nothing_more);
    for (int i = 0; i < n; i++) c->slot_rig[seqs[i]] = rigs[i];
    return SVO_OK;
}

extern "C" int svo_ctx_get_slot_rig(svo_ctx* c, int seq, int* rig, svo_camera_settings* cam) {
    if (!c || seq < 0 || seq >= c->B) return svo_set_error(SVO_ERR_INVALID, "bad ctx / sequence index");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    if (rig) *rig = c->slot_rig[seq];
    if (cam) *cam = c->rigs[c->slot_rig[seq]].cam;
    return SVO_OK;
}

extern "C" int svo_ctx_get_rigs(svo_ctx* c, int* n, int64_t* map_bytes) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_get_rigs: bad ctx");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    if (n) *n = (int)std::count_if(c->rigs.begin(), c->rigs.end(), [](const svo_ctx::Rig& r) { return r.used; });
    if (map_bytes) *map_bytes = (int64_t)c->rig_map_bytes();
    return SVO_OK;
}
