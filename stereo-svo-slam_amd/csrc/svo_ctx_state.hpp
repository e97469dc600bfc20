// svo_ctx_state.hpp — the public svo_ctx of the C ABI, internal to its translation units (only svo_ctx*.hip include
// it): the object with the kinds of job its queues hold, what the files share of the queue (svo_ctx.hip), and the
// steps every submit entry is made of: the head checks with their error texts, the split of the named slots over
// the groups, and submit-then-wait.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <variant>
#include <vector>

#include "svo_group.hpp"
#include "svo_host.hpp"
#include "svo_named_slots.hpp"
#include "svo_tracker.hpp"

// svo_ctx: the public object. Its sequences are split over 1..G groups; a group owns a
// HIP stream, its argument blocks and (G > 1) a host thread that drives it, so the groups
// run their frames independently: while one group waits for its keyframe decision or fills
// its argument blocks, the other group's kernels keep the GPU busy, and the latency-bound
// single-workgroup-per-sequence alignment kernel of one group overlaps the window kernels of
// the other. svo_submit_images() queues a frame set on every group and returns;
// svo_wait() drains the queues. svo_new_images() = submit + wait. Everything else a ctx can submit (the kinds of
// svo_ctx::Job) is an entry of the same queues, so it is ordered with the frame sets.
struct svo_ctx {
    // The kinds of job. Every kind but the frame set names slots: its base is the group's share of them
    // (svo_named_slots.hpp), the named slots as indices in the group, in named order, and (SlotShare) the segment of the
    // job each one fills.
    //
    // a frame set: the group's share of an svo_submit_images
    struct Frames {
        std::vector<const uint8_t*> left, right;
        std::vector<float> ts;
        int stride = 0, mem = 0;
    };
    // the end of some of the group's sequences (svo_ctx_restart_sequences)
    struct Restart : SlotList {};
    // a trim of keyframes (svo_submit_trim_keyframes): the id each slot's keyframes go below
    struct Trim : SlotList {
        std::vector<int> below;
    };
    // a rig assignment (svo_ctx_assign_rigs): what each slot is bound to
    struct RigAssign : SlotList {
        std::vector<RigBinding> bindings;
    };
    // the group's share of an svo_submit_export: the record of the caller's arrays the group packs from
    struct Export : SlotShare {
        int what = 0, mem = 0;
        int64_t base = 0;
        svo_export_dst dst{};
    };
    // the group's share of an svo_submit_export_map: the region each slot goes to
    struct MapExport : SlotShare {
        int mem = 0;
        std::vector<svo_map_region> regions;
        svo_map_filter filter{};
        svo_map_dst dst{};
    };
    // the group's share of an svo_submit_export_views, _disparity or _cloud: a slot fills the segment and the image,
    // planes or records of its named position
    template <typename Style, typename Dst>
    struct ImageExport : SlotShare {
        int what = 0, mem = 0;
        Style style{};
        Dst dst{};
    };
    using ViewExport = ImageExport<svo_view_style, svo_view_dst>;
    // the cross-check a job carries beside its style, or none
    struct StereoCheck {
        bool has_check = false;
        svo_stereo_check check{};
        const svo_stereo_check* check_ptr() const { return has_check ? &check : nullptr; }
        void set_check(const svo_stereo_check* p) {
            if (p) { has_check = true; check = *p; }
        }
    };
    template <typename Style, typename Dst>
    struct CheckedExport : ImageExport<Style, Dst>, StereoCheck {};
    // the SGM params a job carries beside its style, or none (the entries with _sgm in their names: the same job in
    // its SGM mode)
    struct SgmMode {
        bool has_sgm = false;
        svo_sgm_params sgm{};
        const svo_sgm_params* sgm_ptr() const { return has_sgm ? &sgm : nullptr; }
        void set_sgm(const svo_sgm_params* p) {
            if (p) { has_sgm = true; sgm = *p; }
        }
    };
    template <typename Style, typename Dst>
    struct SgmExport : CheckedExport<Style, Dst>, SgmMode {};
    using DisparityExport = SgmExport<svo_disparity_style, svo_disparity_dst>;
    using CloudExport = SgmExport<svo_cloud_style, svo_cloud_dst>;
    // the group's share of an svo_submit_export_scenes: the camera of each slot
    struct SceneExport : SlotShare, SgmMode {
        int mem = 0;
        std::vector<svo_scene_camera> cameras;
        svo_scene_style style{};
        svo_scene_dst dst{};
        // (svo_submit_export_scenes_clouds: the clouds and the span of each named slot of the group, or none)
        bool has_clouds = false;
        svo_scene_clouds clouds{};
        std::vector<svo_scene_span> extra;
    };
    // the group's share of an svo_submit_export_ar: the instances [inst0, inst1) of the job each slot shows, and the
    // job's copied arrays, which the groups share
    struct ArExport : SlotShare, SgmMode {
        int mem = 0;
        std::vector<int> inst0, inst1;
        std::shared_ptr<const ArJob> job;
        svo_ar_dst dst{};
        // (svo_submit_export_ar_occluded with on == 1: the occlusion)
        bool occluded = false;
        svo_ar_occlusion occlusion{};
    };
    // the group's share of an svo_submit_save: where each slot goes
    struct Save : SlotList {
        int mem = 0;
        std::vector<svo_snapshot> snaps;
    };
    // the group's share of an svo_submit_load: the checked snapshots of its slots (their seq: the index in the group)
    struct Load : SlotList {
        int mem = 0;
        std::vector<SnapshotLoad> loads;
    };
    // the group's share of an svo_submit_pose_updates: its named slots with a positive count, their samples in that
    // order, and where each slot's filtered poses go (the caller's memory, or null)
    struct PoseUpdates : SlotList {
        std::vector<int> counts;
        std::vector<svo_pose_sample> samples;
        std::vector<float*> filtered;
    };
    // the group's share of an svo_submit_fuse_clouds: a slot fills the info of its named position
    struct FuseClouds : SlotShare, StereoCheck, SgmMode {
        int what = 0;
        svo_cloud_style style{};
        uint32_t stamp = 0;
        svo_fuse_info* info = nullptr;
    };
    // the group's share of an svo_submit_export_voxel_maps, as MapExport
    struct VoxelExport : SlotShare {
        int mem = 0;
        std::vector<svo_voxel_region> regions;
        svo_voxel_filter filter{};
        svo_voxel_dst dst{};
    };
    // the group's share of an svo_submit_clear_voxel_maps
    struct VoxelClear : SlotList {};
    // the group's share of an svo_submit_prune_voxel_maps: a slot fills the info of its named position; in given
    // mode three floats per slot of the share
    // (svo_submit_carve_voxel_maps: the same entry carrying a carve, the cloud style of its occluder with the check
    // and the SGM params beside it, and the carve's own info records)
    struct VoxelPrune : SlotShare, StereoCheck, SgmMode {
        svo_voxel_keep keep{};
        int center_mode = 0;
        std::vector<float> centers;
        svo_prune_info* info = nullptr;
        bool has_carve = false;
        svo_voxel_carve_rule carve{};
        svo_cloud_style cloud{};
        svo_carve_info* carve_info = nullptr;
    };
    // the group's share of an svo_submit_save_voxel_maps, as VoxelExport with entry records
    struct VoxelSave : SlotShare {
        int mem = 0;
        std::vector<svo_voxel_region> regions;
        svo_voxel_filter filter{};
        svo_voxel_entry_dst dst{};
    };
    // the group's share of an svo_submit_load_voxel_maps: the span of each slot; a slot fills the info of its named position
    struct VoxelLoad : SlotShare {
        int mode = 0, mem = 0;
        std::vector<svo_voxel_entry_span> spans;
        svo_voxel_load_info* info = nullptr;
    };
    // one entry of a group's queue (the frame set first: a Job{} is one, with nothing allocated)
    using Job = std::variant<Frames, Restart, Trim, RigAssign, Export, MapExport, ViewExport, DisparityExport, CloudExport,
                             SceneExport, ArExport, Save, Load, PoseUpdates, FuseClouds, VoxelExport, VoxelClear, VoxelPrune, VoxelSave, VoxelLoad>;
    struct Worker {
        Group g;
        int first = 0, count = 0;
        std::thread th;
        std::mutex m;
        std::condition_variable cv, cv_idle;
        std::deque<Job> jobs;
        bool busy = false, stop = false;
        int err = SVO_OK;
        std::string msg;
        std::atomic<bool>* ctx_failed = nullptr;
    };
    int B = 0, device = 0, width = 0, height = 0;
    // A frame that fails in ONE group leaves the ctx's sequences at mixed frame ids: the failure is
    // latched here, the other groups drop what is still queued, and later submits are rejected.
    std::atomic<bool> failed{false};
    std::vector<std::unique_ptr<Worker>> workers;
    // svo_ctx_set_rectification: one read-only map set for every group (left, right), or none
    svo::DevPtr<uint8_t> rect_mem;
    svo::RemapMap rect[2];
    int input_format = SVO_INPUT_GRAY_PAIR;      // svo_ctx_set_input_format (every group has the same)
    // camera rigs (svo_ctx_add_rigs): rigs[id]; rigs[0] is the ctx's own settings (its maps: rect_mem). A removed
    // rig leaves an unused entry, so ids stay what they were. slot_rig: what each slot is bound to once everything
    // submitted so far has run (svo_ctx_assign_rigs records it at submit time).
    struct Rig {
        bool used = false;
        svo_camera_settings cam{};
        svo::DevPtr<uint8_t> maps;               // left map | right map, or null
    };
    std::vector<Rig> rigs;
    std::vector<int> slot_rig;
    size_t rig_map_bytes() const {
        size_t b = 0;
        for (size_t i = 1; i < rigs.size(); i++)
            if (rigs[i].used && rigs[i].maps) b += 2 * svo::remap_map_bytes(width, height);
        return b;
    }
    bool one_buffer() const { return svo::ingest_format(input_format)->buffers == 1; }
    const svo_group* g0() const { return workers[0]->g.get(); }   // (every group has the same size and settings)
};

namespace svo { int voxel_check_params(const svo_voxel_params* p, bool ctx, const char* who); }
namespace svo { int voxel_check_carve_rule(const svo_voxel_carve_rule* carve, int width, int height, const char* who); }   // svo_capi_voxel.hip
extern "C" int svo_ctx_set_exact_pinv(svo_ctx* c, int on);

// ------------------------------------------------------------------ the queue (svo_ctx.hip)

// the job joins the group's queue (one group: it runs here, on the caller's thread)
void worker_submit(svo_ctx::Worker& w, svo_ctx::Job&& job);
// wait for every group's queue; returns the first stored error (and clears it)
int ctx_drain(svo_ctx* c);
// the group of ctx sequence `seq` and its index there, once every queue of the ctx has drained, with the ctx's
// device current (the per-sequence getters start here)
int ctx_seq(svo_ctx* c, int seq, svo_group** g, int* local);
// nothing is queued on any group once one of them has failed (the first call after the failure reports its cause)
int reject_failed(svo_ctx* c, const char* name);

// ------------------------------------------------------------------ what a submit entry is made of
// An entry checks its arguments in an order of its own and formats the texts that only it has; the steps and texts
// that several share are here. `name`: the entry as its messages spell it.

inline bool what_ok(int what) { return what == SVO_EXPORT_FRAMES || what == SVO_EXPORT_LAST_KEYFRAMES; }
inline bool mem_ok(int mem) { return mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE; }
// seqs == NULL names every slot of the ctx, whatever n is; a list has n >= 0
inline bool naming_ok(const int* seqs, int n) { return !seqs || n >= 0; }
inline NamedSlots ctx_slots(const svo_ctx* c, const int* seqs, int n) { return NamedSlots{seqs, seqs ? n : c->B}; }

inline int reject_slot(const char* name, const NamedSlots& slots, int bad) {
    return svo_set_error(SVO_ERR_INVALID, "%s: sequence %d is out of range or named twice", name, slots.at(bad));
}
// every named slot exists and is named once
inline int check_slots(const svo_ctx* c, const char* name, const NamedSlots& slots) {
    const int bad = slots.first_bad(c->B, true);
    return bad < 0 ? SVO_OK : reject_slot(name, slots, bad);
}
// the same where every named position has an item of its own (a region, a camera, a count): position by position, a
// slot's name is checked before its item. item(i): the error of position i's item, or SVO_OK.
template <typename Item>
int check_slots_and_items(const svo_ctx* c, const char* name, const NamedSlots& slots, Item item) {
    const int bad = slots.first_bad(c->B, true);
    for (int i = 0; i < slots.n; i++) {
        if (i == bad) return reject_slot(name, slots, i);
        if (const int rc = item(i)) return rc;
    }
    return SVO_OK;
}
// n slots of per_slot units ("bytes", "records") each fit the caller's capacity
inline int check_capacity(const char* name, int n, int64_t per_slot, int64_t capacity, const char* units) {
    if (capacity >= n * per_slot) return SVO_OK;
    return svo_set_error(SVO_ERR_CAPACITY, "%s: %d slots need %lld %s, capacity %lld", name, n, (long long)(n * per_slot), units,
                         (long long)capacity);
}
// A cross-check with lr == 0 is off: once the check itself is checked (under the entry's own name, `who`), the job is
// the unchecked one and *check is null.
inline int drop_check_that_is_off(const svo_stereo_check** check, bool cloud, const char* who) {
    if (!*check || (*check)->lr != 0) return SVO_OK;
    if (const int rc = svo::lr_check_parse(*check, cloud, who, nullptr)) return rc;
    *check = nullptr;
    return SVO_OK;
}

// One job of kind J for every group that has a slot in it, in the order of the groups: per(job, i, local) for each
// of the group's named positions i (NamedSlots::share), fill(job) once for what the whole job carries, then the job
// joins the group's queue. The caller has made every check, the ctx's failed flag last.
template <typename J, typename Per, typename Fill>
void submit_shares(svo_ctx* c, const NamedSlots& slots, Per per, Fill fill) {
    for (auto& wp : c->workers) {
        J job;
        if (!slots.share(wp->first, wp->count, job, per)) continue;
        fill(job);
        worker_submit(*wp, std::move(job));
    }
}
// (a kind that keeps nothing per slot but the slot itself, or nothing per job)
inline bool every_slot(const SlotList&, int, int) { return true; }
inline void nothing_more(const SlotList&) {}

// the blocking twin of a submit entry: its result, or the result of the wait
inline int then_wait(svo_ctx* c, int rc) { return rc ? rc : svo_wait(c); }
