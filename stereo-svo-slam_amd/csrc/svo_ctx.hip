// svo_ctx.hip — the public svo_ctx of the C ABI: a set of sequence groups (svo_group.hpp), each
// on its own stream and host thread, with a queue of submitted frame sets, and the extern "C"
// entry points of the ctx. The per-sequence getters at the end read a group's state directly
// (svo_group_state.hpp); everything else drives the groups through svo_group.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <variant>
#include <vector>

#include "svo_group.hpp"
#include "svo_group_state.hpp"
#include "svo_host.hpp"
#include "svo_kernels.hpp"
#include "svo_named_slots.hpp"

// svo_ctx: the public object. Its sequences are split over 1..G groups; a group owns a
// HIP stream, its argument blocks and (G > 1) a host thread that drives it, so the groups
// run their frames independently: while one group waits for its keyframe decision or fills
// its argument blocks, the other group's kernels keep the GPU busy, and the latency-bound
// single-workgroup-per-sequence alignment kernel of one group overlaps the window kernels of
// the other. svo_submit_images() queues a frame set on every group and returns;
// svo_wait() drains the queues. svo_new_images() = submit + wait. Everything else a ctx can submit (the kinds of
// svo_ctx::Job) is an entry of the same queues, so it is ordered with the frame sets.
struct svo_ctx {
    // a frame set: the group's share of an svo_submit_images
    struct Frames {
        std::vector<const uint8_t*> left, right;
        std::vector<float> ts;
        int stride = 0, mem = 0;
    };
    // the end of some of the group's sequences (svo_ctx_restart_sequences): indices in the group
    struct Restart {
        std::vector<int> seqs;
    };
    // a trim of keyframes (svo_submit_trim_keyframes): indices in the group, and the id each one's keyframes go below
    struct Trim {
        std::vector<int> seqs, below;
    };
    // a rig assignment (svo_ctx_assign_rigs): indices in the group, and what each is bound to
    struct RigAssign {
        std::vector<int> seqs;
        std::vector<RigBinding> bindings;
    };
    // the group's share of an svo_submit_export: its named slots (indices in the group) in named order, the
    // segment each one fills, and the record of the caller's arrays the group packs from
    struct Export {
        int what = 0, mem = 0;
        std::vector<int> seqs, seg;
        int64_t base = 0;
        svo_export_dst dst{};
    };
    // the group's share of an svo_submit_export_map: its named slots (indices in the group) in named order, the
    // segment each one fills and the region it goes to
    struct MapExport {
        int mem = 0;
        std::vector<int> seqs, seg;
        std::vector<svo_map_region> regions;
        svo_map_filter filter{};
        svo_map_dst dst{};
    };
    // the group's share of an svo_submit_export_views, _disparity or _cloud: its named slots (indices in the group) in
    // named order and the segment (and image, planes or records) of the job each one fills
    template <typename Style, typename Dst>
    struct ImageExport {
        int what = 0, mem = 0;
        std::vector<int> seqs, seg;
        Style style{};
        Dst dst{};
    };
    using ViewExport = ImageExport<svo_view_style, svo_view_dst>;
    // (a checked job carries its cross-check beside the style: has_check)
    template <typename Style, typename Dst>
    struct CheckedExport : ImageExport<Style, Dst> {
        bool has_check = false;
        svo_stereo_check check{};
        const svo_stereo_check* check_ptr() const { return has_check ? &check : nullptr; }
    };
    using DisparityExport = CheckedExport<svo_disparity_style, svo_disparity_dst>;
    using CloudExport = CheckedExport<svo_cloud_style, svo_cloud_dst>;
    // the group's share of an svo_submit_export_scenes: its named slots (indices in the group) in named order, the
    // camera of each and the segment (and image) of the job each one fills
    struct SceneExport {
        int mem = 0;
        std::vector<int> seqs, seg;
        std::vector<svo_scene_camera> cameras;
        svo_scene_style style{};
        svo_scene_dst dst{};
        // (svo_submit_export_scenes_clouds: the clouds and the span of each named slot of the group, or none)
        bool has_clouds = false;
        svo_scene_clouds clouds{};
        std::vector<svo_scene_span> extra;
    };
    // the group's share of an svo_submit_export_ar: its named slots (indices in the group) in named order, the
    // instances [inst0, inst1) of the job each one shows, the segment (and image) of the job each one fills, and
    // the job's copied arrays, which the groups share
    struct ArExport {
        int mem = 0;
        std::vector<int> seqs, seg, inst0, inst1;
        std::shared_ptr<const ArJob> job;
        svo_ar_dst dst{};
        // (svo_submit_export_ar_occluded with on == 1: the occlusion)
        bool occluded = false;
        svo_ar_occlusion occlusion{};
    };
    // the group's share of an svo_submit_save: its named slots, indices in the group, and where each one goes
    struct Save {
        int mem = 0;
        std::vector<int> seqs;
        std::vector<svo_snapshot> snaps;
    };
    // the group's share of an svo_submit_load: the checked snapshots of its named slots (seq: index in the group)
    struct Load {
        int mem = 0;
        std::vector<SnapshotLoad> loads;
    };
    // the group's share of an svo_submit_pose_updates: its named slots with a positive count (indices in the group),
    // their samples in that order, and where each slot's filtered poses go (the caller's memory, or null)
    struct PoseUpdates {
        std::vector<int> seqs, counts;
        std::vector<svo_pose_sample> samples;
        std::vector<float*> filtered;
    };
    // the group's share of an svo_submit_fuse_clouds: its named slots (indices in the group) in named order and the
    // info of the job each one fills
    struct FuseClouds {
        int what = 0;
        std::vector<int> seqs, seg;
        svo_cloud_style style{};
        bool has_check = false;
        svo_stereo_check check{};
        uint32_t stamp = 0;
        svo_fuse_info* info = nullptr;
    };
    // the group's share of an svo_submit_export_voxel_maps, as MapExport
    struct VoxelExport {
        int mem = 0;
        std::vector<int> seqs, seg;
        std::vector<svo_voxel_region> regions;
        svo_voxel_filter filter{};
        svo_voxel_dst dst{};
    };
    // the group's share of an svo_submit_clear_voxel_maps: indices in the group
    struct VoxelClear {
        std::vector<int> seqs;
    };
    // one entry of a group's queue (the frame set first: a Job{} is one, with nothing allocated)
    using Job = std::variant<Frames, Restart, Trim, RigAssign, Export, MapExport, ViewExport, DisparityExport, CloudExport,
                             SceneExport, ArExport, Save, Load, PoseUpdates, FuseClouds, VoxelExport, VoxelClear>;
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
};

namespace {

// the job joins the group's queue (one group: it runs here, on the caller's thread)
void worker_submit(svo_ctx::Worker& w, svo_ctx::Job&& job);

// what a group runs for each kind of entry (seq0: the ctx slot of the group's first)
int run_job(svo_group* g, int, const svo_ctx::Frames& j) {
    return grp_new_images(g, j.left.data(), j.right.empty() ? nullptr : j.right.data(), j.stride, j.ts.data(), j.mem);
}
int run_job(svo_group* g, int, const svo_ctx::Restart& j) { return grp_restart_sequences(g, j.seqs.data(), (int)j.seqs.size()); }
int run_job(svo_group* g, int, const svo_ctx::Trim& j) { return grp_trim_keyframes(g, j.seqs.data(), j.below.data(), (int)j.seqs.size()); }
int run_job(svo_group* g, int, const svo_ctx::RigAssign& j) { return grp_assign_rigs(g, j.seqs.data(), j.bindings.data(), (int)j.seqs.size()); }
int run_job(svo_group* g, int seq0, const svo_ctx::Export& j) {
    return grp_export(g, j.what, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, j.base, &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::MapExport& j) {
    return grp_export_map(g, j.mem, j.seqs.data(), j.seg.data(), j.regions.data(), (int)j.seqs.size(), seq0, &j.filter, &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::ViewExport& j) {
    return grp_export_views(g, j.what, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::DisparityExport& j) {
    return grp_export_disparity(g, j.what, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.check_ptr(), &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::CloudExport& j) {
    return grp_export_cloud(g, j.what, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.check_ptr(), &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::SceneExport& j) {
    return grp_export_scenes_clouds(g, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.cameras.data(), &j.dst,
                                    j.has_clouds ? &j.clouds : nullptr, j.extra.empty() ? nullptr : j.extra.data());
}
int run_job(svo_group* g, int seq0, const svo_ctx::ArExport& j) {
    return grp_export_ar_occluded(g, j.mem, j.seqs.data(), j.seg.data(), j.inst0.data(), j.inst1.data(), (int)j.seqs.size(), seq0, j.job.get(), &j.dst,
                                  j.occluded ? &j.occlusion : nullptr);
}
int run_job(svo_group* g, int, const svo_ctx::Save& j) { return grp_save(g, j.seqs.data(), (int)j.seqs.size(), j.snaps.data(), j.mem); }
int run_job(svo_group* g, int, const svo_ctx::Load& j) { return grp_load(g, j.loads.data(), (int)j.loads.size(), j.mem); }
int run_job(svo_group* g, int, const svo_ctx::PoseUpdates& j) {
    return grp_pose_updates(g, j.seqs.data(), j.counts.data(), (int)j.seqs.size(), j.samples.data(), j.filtered.data());
}

int run_job(svo_group* g, int seq0, const svo_ctx::FuseClouds& j) {
    return grp_fuse_clouds(g, j.what, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.has_check ? &j.check : nullptr, j.stamp,
                           j.info);
}
int run_job(svo_group* g, int seq0, const svo_ctx::VoxelExport& j) {
    return grp_export_voxel_maps(g, j.mem, j.seqs.data(), j.seg.data(), j.regions.data(), (int)j.seqs.size(), seq0, &j.filter, &j.dst);
}
int run_job(svo_group* g, int, const svo_ctx::VoxelClear& j) { return grp_clear_voxel_maps(g, j.seqs.data(), (int)j.seqs.size()); }

void worker_run_job(svo_ctx::Worker& w, const svo_ctx::Job& job) {
    if (w.err != SVO_OK || w.ctx_failed->load()) return;   // after a failure (any group) the queues are dropped
    const int rc = std::visit([&w](const auto& j) { return run_job(w.g.get(), w.first, j); }, job);
    if (rc != SVO_OK) {
        w.err = rc;
        w.msg = svo_last_error();
        w.ctx_failed->store(true);
    }
}

void worker_loop(svo_ctx::Worker* w) {
    for (;;) {
        svo_ctx::Job job;
        {
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [w] { return w->stop || !w->jobs.empty(); });
            if (w->jobs.empty()) return;         // stop requested and nothing left
            job = std::move(w->jobs.front());
            w->jobs.pop_front();
            w->busy = true;
        }
        worker_run_job(*w, job);
        {
            std::lock_guard<std::mutex> lk(w->m);
            w->busy = false;
            if (w->jobs.empty()) w->cv_idle.notify_all();
        }
    }
}

void worker_submit(svo_ctx::Worker& w, svo_ctx::Job&& job) {
    if (w.th.joinable()) {
        {
            std::lock_guard<std::mutex> lk(w.m);
            w.jobs.push_back(std::move(job));
        }
        w.cv.notify_one();
    } else {
        worker_run_job(w, job);
    }
}

// wait for every group's queue; returns the first stored error (and clears it)
int ctx_drain(svo_ctx* c) {
    int rc = SVO_OK;
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        if (w.th.joinable()) {
            std::unique_lock<std::mutex> lk(w.m);
            w.cv_idle.wait(lk, [&w] { return w.jobs.empty() && !w.busy; });
        }
        if (w.err != SVO_OK && rc == SVO_OK) {
            rc = svo_set_error(w.err, "%s", w.msg.c_str());
            w.err = SVO_OK;
        }
    }
    return rc;
}

// the group of ctx sequence `seq` and its index there, once every queue of the ctx has drained, with the ctx's
// device current (the per-sequence getters start here)
int ctx_seq(svo_ctx* c, int seq, svo_group** g, int* local) {
    if (!c || seq < 0 || seq >= c->B) return svo_set_error(SVO_ERR_INVALID, "bad ctx / sequence index");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    for (auto& w : c->workers)
        if (seq < w->first + w->count) {
            *g = w->g.get();
            *local = seq - w->first;
            break;
        }
    HIP_TRY(hipSetDevice(c->device));
    return SVO_OK;
}

// nothing is queued on any group once one of them has failed (the first call after the failure reports its cause)
int reject_failed(svo_ctx* c, const char* name) {
    const int rc = ctx_drain(c);
    return rc ? rc : svo_set_error(SVO_ERR_INVALID, "%s: an earlier frame of this ctx failed; create a new ctx", name);
}

}  // namespace

extern "C" int svo_ctx_create(const svo_camera_settings* cam, int width, int height, int n_sequences,
                              int device, svo_ctx** out) {
    if (!cam || !out || n_sequences < 1) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_create: bad arguments");
    // SVO_GROUPS: number of independently driven groups. Default: groups of ~256 sequences — fewer per group
    // when a sequence carries many keypoints (131072 / keypoint capacity, at least 32: 64 at the 1920x1080
    // configuration, whose alignment launch is as slow as its slowest sequence whatever the group's size:
    // 256 sequences, frames/s: 1 group 12.1 K, 2 13.2 K, 4 14.1 K, 8 13.2 K; 512 in 8 18.2 K) —, at least
    // two from 64 sequences on, and one fewer than the hardware queues the HIP runtime uses
    // (GPU_MAX_HW_QUEUES, default 4): streams beyond that share a queue and serialise. Measured on
    // MI355X, 752x480, frames/s: 768 sequences 149 K as 3 groups, 106 K as 4, 119 K as 6 with 4
    // queues; with GPU_MAX_HW_QUEUES=8: 768 / 3 groups 154 K, 1024 / 4 162 K, 1536 / 6 170 K.
    int hwq = 4;
    if (const char* e = std::getenv("GPU_MAX_HW_QUEUES")) hwq = std::max(2, std::atoi(e));
    const int kp_cap = (cam->grid_width > 0 && cam->grid_height > 0 ? (width / cam->grid_width) * (height / cam->grid_height) : 0) + 64;
    const int per_group = std::max(32, std::min(256, 131072 / std::max(kp_cap, 1)));
    int G = n_sequences >= 64 ? std::max(2, (n_sequences + per_group / 2) / per_group) : 1;
    G = std::min(G, hwq - 1);
    if (const char* e = std::getenv("SVO_GROUPS")) G = std::atoi(e);
    G = std::max(1, std::min(G, std::min(n_sequences, 16)));
    std::unique_ptr<svo_ctx> c(new (std::nothrow) svo_ctx());
    if (!c) return svo_set_error(SVO_ERR_INVALID, "out of host memory");
    c->B = n_sequences; c->device = device; c->width = width; c->height = height;
    c->rigs.resize(1);
    c->rigs[0].used = true; c->rigs[0].cam = *cam;
    c->slot_rig.assign(n_sequences, 0);
    int first = 0;
    for (int g = 0; g < G; g++) {
        const int count = n_sequences / G + (g < n_sequences % G ? 1 : 0);
        auto w = std::make_unique<svo_ctx::Worker>();
        w->first = first; w->count = count; w->ctx_failed = &c->failed;
        const int rc = grp_create(cam, width, height, count, device, &w->g);
        if (rc) return rc;
        first += count;
        c->workers.push_back(std::move(w));
    }
    if (G > 1)
        for (auto& w : c->workers) w->th = std::thread(worker_loop, w.get());
    *out = c.release();
    return SVO_OK;
}

extern "C" int svo_ctx_destroy(svo_ctx* c) {
    if (!c) return SVO_OK;
    (void)ctx_drain(c);
    for (auto& w : c->workers) {
        if (w->th.joinable()) {
            {
                std::lock_guard<std::mutex> lk(w->m);
                w->stop = true;
            }
            w->cv.notify_all();
            w->th.join();
        }
        w->g.reset();
    }
    c->rect_mem.reset();                          // (after the groups that read it; the rigs' maps go with the ctx)
    delete c;
    return SVO_OK;
}

extern "C" int svo_ctx_get_groups(svo_ctx* c, int* n_groups) {
    if (!c || !n_groups) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_get_groups: bad arguments");
    *n_groups = (int)c->workers.size();
    return SVO_OK;
}

extern "C" int svo_submit_images(svo_ctx* c, const uint8_t* const* left, const uint8_t* const* right,
                                 int stride, const float* time_stamps, int mem) {
    if (!c || !left || !time_stamps || (!right && !c->one_buffer()))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_images: bad arguments");
    const svo::IngestFormat& f = *svo::ingest_format(c->input_format);
    if ((long long)stride < (long long)svo::ingest_row_pixels(f, c->width) * f.channels)   // (nothing is queued: the ctx stays usable)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_images: stride %d is below the row's bytes", stride);
    if (c->failed.load()) return reject_failed(c, "svo_submit_images");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::Frames job;
        job.left.assign(left + w.first, left + w.first + w.count);
        if (right && !c->one_buffer()) job.right.assign(right + w.first, right + w.first + w.count);   // (else: ignored)
        job.ts.assign(time_stamps + w.first, time_stamps + w.first + w.count);
        job.stride = stride; job.mem = mem;
        worker_submit(w, std::move(job));
    }
    return SVO_OK;
}

extern "C" int svo_ctx_restart_sequences(svo_ctx* c, const int* seqs, int n) {
    if (!c || n < 0 || (n > 0 && !seqs)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_restart_sequences: bad arguments");
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, false); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_restart_sequences: sequence %d out of range", slots.at(bad));
    if (c->failed.load()) return reject_failed(c, "svo_ctx_restart_sequences");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::Restart job;
        slots.each_in(w.first, w.count, [&](int, int local) { job.seqs.push_back(local); });
        if (!job.seqs.empty()) worker_submit(w, std::move(job));
    }
    return SVO_OK;
}

extern "C" int svo_submit_trim_keyframes(svo_ctx* c, const int* seqs, const int* below, int n) {
    if (!c || (seqs && n < 0)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_trim_keyframes: bad arguments");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_trim_keyframes: sequence %d is out of range or named twice", slots.at(bad));
    if (c->failed.load()) return reject_failed(c, "svo_submit_trim_keyframes");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::Trim job;
        slots.each_in(w.first, w.count, [&](int i, int local) {
            job.seqs.push_back(local);
            job.below.push_back(below ? below[i] : INT_MAX);     // (NULL: everything retired)
        });
        if (!job.seqs.empty()) worker_submit(w, std::move(job));
    }
    return SVO_OK;
}

extern "C" int svo_trim_keyframes(svo_ctx* c, const int* seqs, const int* below, int n) {
    const int rc = svo_submit_trim_keyframes(c, seqs, below, n);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_ctx_set_keyframe_window(svo_ctx* c, int keep) {
    if (!c || keep < -1) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_keyframe_window: bad ctx, or keep %d below -1", keep);
    const int rc = ctx_drain(c);
    if (!rc)
        for (auto& w : c->workers) grp_set_keyframe_window(w->g.get(), keep);
    return rc;
}

extern "C" int svo_get_keyframe_range(svo_ctx* ctx, int seq, svo_keyframe_range* out) {
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    if (out) *out = grp_keyframe_range(g, s);
    return SVO_OK;
}

extern "C" int svo_submit_export(svo_ctx* c, int what, const int* seqs, int n, const svo_export_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || (what != SVO_EXPORT_FRAMES && what != SVO_EXPORT_LAST_KEYFRAMES) ||
        (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export: bad arguments (what %d, mem %d)", what, mem);
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export: sequence %d is out of range or named twice", slots.at(bad));
    for (const void* p : {(const void*)dst->kps2d, (const void*)dst->kps3d, (const void*)dst->info})
        if ((uintptr_t)p & 3) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export: an array is not 4-byte aligned");
    const int64_t per_seq = grp_capacity(c->workers[0]->g.get());     // (the same in every group)
    if ((dst->kps2d || dst->kps3d || dst->info) && dst->capacity < n * per_seq)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export: %d slots need arrays of %lld records, capacity %lld", n,
                             (long long)(n * per_seq), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, "svo_submit_export");
    int64_t before = 0;                          // named slots of the groups so far
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::Export e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); });
        if (e.seqs.empty()) continue;
        e.what = what; e.mem = mem; e.dst = *dst; e.base = before * per_seq;
        before += (int64_t)e.seqs.size();
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_export(svo_ctx* c, int what, const int* seqs, int n, const svo_export_dst* dst, int mem) {
    const int rc = svo_submit_export(c, what, seqs, n, dst, mem);
    return rc ? rc : svo_wait(c);
}

namespace {

// what svo_submit_save and svo_submit_load check alike, before anything is queued
int check_snapshot_call(svo_ctx* c, const char* name, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    if (!c || n < 0 || (n > 0 && (!seqs || !snaps)) || (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (mem %d)", name, mem);
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: sequence %d is out of range or named twice", name, slots.at(bad));
    return SVO_OK;
}

}  // namespace

extern "C" int svo_submit_export_map(svo_ctx* c, const int* seqs, int n, const svo_map_region* regions,
                                     const svo_map_filter* filter, const svo_map_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: bad arguments (mem %d)", mem);
    if (!seqs) n = c->B;
    if (n > 0 && !regions) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: no regions");
    const svo_map_filter f = filter ? *filter : svo_map_filter{0, 0, 0, 0};
    if ((f.drop_flags & ~(uint32_t)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY)) || f._reserved != 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: drop_flags 0x%x has unknown bits, or _reserved is not 0", f.drop_flags);
    if ((uintptr_t)dst->points & 15) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: points is not 16-byte aligned");
    const NamedSlots slots{seqs, n};
    const int bad = slots.first_bad(c->B, true);
    for (int i = 0; i < n; i++) {                // (a slot's name is checked before its region)
        if (i == bad)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: sequence %d is out of range or named twice", slots.at(i));
        const svo_map_region& r = regions[i];
        if (r.first_point < 0 || r.point_capacity < 0 || r.first_keyframe_entry < 0 || r.keyframe_capacity < 0 || r.from_keyframe < 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: region %d has a negative field", i);
        if ((r.point_capacity > 0 && !dst->points) || (r.keyframe_capacity > 0 && !dst->keyframes))
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_map: region %d has a capacity, but its array is NULL", i);
    }
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_map");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::MapExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); e.regions.push_back(regions[i]); });
        if (e.seqs.empty()) continue;
        e.mem = mem; e.filter = f; e.dst = *dst;
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_export_map(svo_ctx* c, const int* seqs, int n, const svo_map_region* regions, const svo_map_filter* filter,
                              const svo_map_dst* dst, int mem) {
    const int rc = svo_submit_export_map(c, seqs, n, regions, filter, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_export_views(svo_ctx* c, int what, const int* seqs, int n, const svo_view_style* style,
                                       const svo_view_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || (what != SVO_EXPORT_FRAMES && what != SVO_EXPORT_LAST_KEYFRAMES) ||
        (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_views: bad arguments (what %d, mem %d)", what, mem);
    const svo_group* g0 = c->workers[0]->g.get();                    // (every group has the same settings)
    if (const int rc = grp_check_view_style(g0, style)) return rc;
    if (!dst->pixels || ((uintptr_t)dst->pixels & 3))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_views: pixels is NULL or not 4-byte aligned");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_views: sequence %d is out of range or named twice", slots.at(bad));
    const int64_t image_bytes = grp_view_bytes(g0, style);
    if (dst->capacity < n * image_bytes)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_views: %d slots need %lld bytes, capacity %lld", n,
                             (long long)(n * image_bytes), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_views");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::ViewExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); });
        if (e.seqs.empty()) continue;
        e.what = what; e.mem = mem; e.style = *style; e.dst = *dst;
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_export_views(svo_ctx* c, int what, const int* seqs, int n, const svo_view_style* style,
                                const svo_view_dst* dst, int mem) {
    const int rc = svo_submit_export_views(c, what, seqs, n, style, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_export_disparity_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                                   const svo_stereo_check* check, const svo_disparity_dst* dst, int mem) {
    if (check && check->lr == 0) {                                   // (off: the unchecked job, once the check itself is checked)
        if (const int rc = svo::lr_check_parse(check, false, "svo_submit_export_disparity_checked", nullptr)) return rc;
        check = nullptr;
    }
    if (!c || !dst || !dst->segments || (what != SVO_EXPORT_FRAMES && what != SVO_EXPORT_LAST_KEYFRAMES) ||
        (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: bad arguments (what %d, mem %d)", what, mem);
    const svo_group* g0 = c->workers[0]->g.get();                    // (every group has the same settings)
    if (const int rc = grp_check_disparity_style(g0, style, check)) return rc;
    if (!dst->values || ((uintptr_t)dst->values & 15))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: values is NULL or not 16-byte aligned");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: sequence %d is out of range or named twice", slots.at(bad));
    const int64_t image_bytes = grp_disparity_bytes(g0, style, check);
    if (dst->capacity < n * image_bytes)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_disparity: %d slots need %lld bytes, capacity %lld", n,
                             (long long)(n * image_bytes), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_disparity");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::DisparityExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); });
        if (e.seqs.empty()) continue;
        e.what = what; e.mem = mem; e.style = *style; e.dst = *dst;
        if (check) { e.has_check = true; e.check = *check; }
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_submit_export_disparity(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                           const svo_disparity_dst* dst, int mem) {
    return svo_submit_export_disparity_checked(c, what, seqs, n, style, nullptr, dst, mem);
}

extern "C" int svo_export_disparity(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                    const svo_disparity_dst* dst, int mem) {
    const int rc = svo_submit_export_disparity(c, what, seqs, n, style, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_export_disparity_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_disparity_style* style,
                                            const svo_stereo_check* check, const svo_disparity_dst* dst, int mem) {
    const int rc = svo_submit_export_disparity_checked(c, what, seqs, n, style, check, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_export_cloud_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                               const svo_stereo_check* check, const svo_cloud_dst* dst, int mem) {
    if (check && check->lr == 0) {                                   // (off: the unchecked job, once the check itself is checked)
        if (const int rc = svo::lr_check_parse(check, true, "svo_submit_export_cloud_checked", nullptr)) return rc;
        check = nullptr;
    }
    if (!c || !dst || !dst->segments || (what != SVO_EXPORT_FRAMES && what != SVO_EXPORT_LAST_KEYFRAMES) ||
        (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_cloud: bad arguments (what %d, mem %d)", what, mem);
    const svo_group* g0 = c->workers[0]->g.get();                    // (every group has the same settings)
    if (const int rc = grp_check_cloud_style(g0, style, check)) return rc;
    if (!dst->points || ((uintptr_t)dst->points & 15))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_cloud: points is NULL or not 16-byte aligned");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_cloud: sequence %d is out of range or named twice", slots.at(bad));
    const int64_t per_slot = grp_cloud_points(g0, style);
    if (dst->capacity < n * per_slot)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_cloud: %d slots need %lld records, capacity %lld", n,
                             (long long)(n * per_slot), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_cloud");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::CloudExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); });
        if (e.seqs.empty()) continue;
        e.what = what; e.mem = mem; e.style = *style; e.dst = *dst;
        if (check) { e.has_check = true; e.check = *check; }
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

namespace svo { int voxel_check_params(const svo_voxel_params* p, bool ctx, const char* who); }

extern "C" int svo_ctx_set_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_params* params) {
    if (!c || (seqs && n < 0)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_voxel_maps: bad arguments");
    if (params)
        if (const int rc = svo::voxel_check_params(params, true, "svo_ctx_set_voxel_maps")) return rc;
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_voxel_maps: sequence %d is out of range or named twice", slots.at(bad));
    if (const int rc = ctx_drain(c)) return rc;
    for (auto& wp : c->workers) {
        std::vector<int> local;
        slots.each_in(wp->first, wp->count, [&](int, int l) { local.push_back(l); });
        if (local.empty()) continue;
        if (const int rc = grp_set_voxel_maps(wp->g.get(), local.data(), (int)local.size(), params)) return rc;
    }
    return SVO_OK;
}

extern "C" int svo_get_voxel_map_info(svo_ctx* ctx, int seq, svo_voxel_map_info* info) {
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    if (!grp_voxel_map_info(g, s, info)) return svo_set_error(SVO_ERR_INVALID, "svo_get_voxel_map_info: slot %d has no voxel map", seq);
    return SVO_OK;
}

extern "C" int svo_submit_fuse_clouds(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                      const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info) {
    if (check && check->lr == 0) {                                   // (off: the unchecked job, once the check itself is checked)
        if (const int rc = svo::lr_check_parse(check, true, "svo_submit_fuse_clouds", nullptr)) return rc;
        check = nullptr;
    }
    if (!c || !info || (what != SVO_EXPORT_FRAMES && what != SVO_EXPORT_LAST_KEYFRAMES) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_fuse_clouds: bad arguments (what %d)", what);
    const svo_group* g0 = c->workers[0]->g.get();                    // (every group has the same settings)
    if (const int rc = grp_check_cloud_style(g0, style, check)) return rc;
    if (style->frame != SVO_CLOUD_WORLD || style->layout != 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_fuse_clouds: frame must be SVO_CLOUD_WORLD and layout 0");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_fuse_clouds: sequence %d is out of range or named twice", slots.at(bad));
    if (c->failed.load()) return reject_failed(c, "svo_submit_fuse_clouds");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::FuseClouds e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); });
        if (e.seqs.empty()) continue;
        e.what = what; e.style = *style; e.stamp = stamp; e.info = info;
        if (check) { e.has_check = true; e.check = *check; }
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_fuse_clouds(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style, const svo_stereo_check* check,
                               uint32_t stamp, svo_fuse_info* info) {
    const int rc = svo_submit_fuse_clouds(c, what, seqs, n, style, check, stamp, info);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_export_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_region* regions,
                                            const svo_voxel_filter* filter, const svo_voxel_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: bad arguments (mem %d)", mem);
    if (!seqs) n = c->B;
    if (n > 0 && !regions) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: no regions");
    const svo_voxel_filter f = filter ? *filter : svo_voxel_filter{0, 0, {0, 0}};
    if (f._reserved[0] != 0 || f._reserved[1] != 0) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: a _reserved is not 0");
    if ((uintptr_t)dst->points & 15) return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: points is not 16-byte aligned");
    const NamedSlots slots{seqs, n};
    const int bad = slots.first_bad(c->B, true);
    for (int i = 0; i < n; i++) {                // (a slot's name is checked before its region)
        if (i == bad)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: sequence %d is out of range or named twice", slots.at(i));
        const svo_voxel_region& r = regions[i];
        if (r.first_point < 0 || r.point_capacity < 0 || r._reserved[0] != 0 || r._reserved[1] != 0 || r._reserved[2] != 0)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: region %d has a negative field or a non-zero _reserved", i);
        if (r.point_capacity > 0 && !dst->points)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_voxel_maps: region %d has a capacity, but points is NULL", i);
    }
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_voxel_maps");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::VoxelExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) { e.seqs.push_back(local); e.seg.push_back(i); e.regions.push_back(regions[i]); });
        if (e.seqs.empty()) continue;
        e.mem = mem; e.filter = f; e.dst = *dst;
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_export_voxel_maps(svo_ctx* c, const int* seqs, int n, const svo_voxel_region* regions, const svo_voxel_filter* filter,
                                     const svo_voxel_dst* dst, int mem) {
    const int rc = svo_submit_export_voxel_maps(c, seqs, n, regions, filter, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_clear_voxel_maps(svo_ctx* c, const int* seqs, int n) {
    if (!c || (seqs && n < 0)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_clear_voxel_maps: bad arguments");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_clear_voxel_maps: sequence %d is out of range or named twice", slots.at(bad));
    if (c->failed.load()) return reject_failed(c, "svo_submit_clear_voxel_maps");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::VoxelClear e;
        slots.each_in(w.first, w.count, [&](int, int local) { e.seqs.push_back(local); });
        if (e.seqs.empty()) continue;
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_submit_export_cloud(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                       const svo_cloud_dst* dst, int mem) {
    return svo_submit_export_cloud_checked(c, what, seqs, n, style, nullptr, dst, mem);
}

extern "C" int svo_export_cloud(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                const svo_cloud_dst* dst, int mem) {
    const int rc = svo_submit_export_cloud(c, what, seqs, n, style, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_export_cloud_checked(svo_ctx* c, int what, const int* seqs, int n, const svo_cloud_style* style,
                                        const svo_stereo_check* check, const svo_cloud_dst* dst, int mem) {
    const int rc = svo_submit_export_cloud_checked(c, what, seqs, n, style, check, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_export_scenes(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                        const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    return svo_submit_export_scenes_clouds(c, seqs, n, style, nullptr, cameras, dst, mem);
}

extern "C" int svo_submit_export_scenes_clouds(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                               const svo_scene_clouds* clouds, const svo_scene_camera* cameras, const svo_scene_dst* dst,
                                               int mem) {
    if (clouds && clouds->live == 0 && !clouds->extra) {             // (nothing to draw: the plain job, once the clouds are checked)
        if (c)
            if (const int rc = grp_check_scene_clouds(c->workers[0]->g.get(), clouds)) return rc;
        clouds = nullptr;
    }
    if (!c || !dst || !dst->segments || !cameras || (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes: bad arguments (mem %d)", mem);
    if (const int rc = svo::scene_check_style(style, "svo_submit_export_scenes")) return rc;
    if (!dst->pixels || ((uintptr_t)dst->pixels & 3))
        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes: pixels is NULL or not 4-byte aligned");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    const int bad = slots.first_bad(c->B, true);
    for (int i = 0; i < n; i++) {                // (a slot's name is checked before its camera)
        if (i == bad)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes: sequence %d is out of range or named twice", slots.at(i));
        if (const int rc = svo::scene_check_camera(&cameras[i], "svo_submit_export_scenes", i)) return rc;
    }
    if (clouds) {
        if (const int rc = grp_check_scene_clouds(c->workers[0]->g.get(), clouds)) return rc;   // (every group has the same settings)
        for (int i = 0; clouds->extra && i < n; i++)
            if (!svo::scene_span_ok((uintptr_t)clouds->extra[i].points, clouds->extra[i].n))
                return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_scenes_clouds: span %d: n %lld must be >= 0 and its records device memory, 16-byte aligned",
                                     i, (long long)clouds->extra[i].n);
    }
    const int64_t image_bytes = grp_scene_bytes(style);
    if (dst->capacity < n * image_bytes)
        return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_scenes: %d slots need %lld bytes, capacity %lld", n,
                             (long long)(n * image_bytes), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, "svo_submit_export_scenes");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::SceneExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) {
            e.seqs.push_back(local); e.seg.push_back(i); e.cameras.push_back(cameras[i]);
            if (clouds && clouds->extra) e.extra.push_back(clouds->extra[i]);
        });
        if (e.seqs.empty()) continue;
        e.mem = mem; e.style = *style; e.dst = *dst;
        if (clouds) { e.has_clouds = true; e.clouds = *clouds; }
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_export_scenes(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style,
                                 const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    const int rc = svo_submit_export_scenes(c, seqs, n, style, cameras, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_export_scenes_clouds(svo_ctx* c, const int* seqs, int n, const svo_scene_style* style, const svo_scene_clouds* clouds,
                                        const svo_scene_camera* cameras, const svo_scene_dst* dst, int mem) {
    const int rc = svo_submit_export_scenes_clouds(c, seqs, n, style, clouds, cameras, dst, mem);
    return rc ? rc : svo_wait(c);
}

// svo_submit_export_ar (occlusion == null) and svo_submit_export_ar_occluded
static int submit_export_ar(svo_ctx* c, const char* who, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                            const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances, const int* first, int n_instances,
                            const svo_ar_dst* dst, int mem) {
    if (!c || !dst || !dst->segments || (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE) || (seqs && n < 0) || n_meshes < 0 ||
        n_instances < 0 || (n_meshes > 0 && !meshes) || (n_instances > 0 && !instances))
        return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments (mem %d, %d meshes, %d instances)", who, mem, n_meshes, n_instances);
    if (const int rc = svo::ar_check_style(style, who)) return rc;
    if (const int rc = grp_check_ar_occlusion(c->workers[0]->g.get(), occlusion)) return rc;   // (every group has the same size and settings)
    if (!dst->pixels || ((uintptr_t)dst->pixels & 3)) return svo_set_error(SVO_ERR_INVALID, "%s: pixels is NULL or not 4-byte aligned", who);
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, true); bad >= 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: sequence %d is out of range or named twice", who, slots.at(bad));
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
    const int64_t image_bytes = grp_ar_bytes(c->workers[0]->g.get(), style);   // (every group has the same size)
    if (dst->capacity < n * image_bytes)
        return svo_set_error(SVO_ERR_CAPACITY, "%s: %d slots need %lld bytes, capacity %lld", who, n, (long long)(n * image_bytes), (long long)dst->capacity);
    if (c->failed.load()) return reject_failed(c, who);
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::ArExport e;
        slots.each_in(w.first, w.count, [&](int i, int local) {
            e.seqs.push_back(local); e.seg.push_back(i);
            e.inst0.push_back(first ? first[i] : 0); e.inst1.push_back(first ? first[i + 1] : n_instances);
        });
        if (e.seqs.empty()) continue;
        e.mem = mem; e.job = job; e.dst = *dst;
        if (occlusion && occlusion->on == 1) { e.occluded = true; e.occlusion = *occlusion; }
        worker_submit(w, std::move(e));
    }
    return SVO_OK;
}

extern "C" int svo_submit_export_ar(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_mesh* meshes,
                                    int n_meshes, const svo_ar_instance* instances, const int* first, int n_instances,
                                    const svo_ar_dst* dst, int mem) {
    return submit_export_ar(c, "svo_submit_export_ar", seqs, n, style, nullptr, meshes, n_meshes, instances, first, n_instances, dst, mem);
}

extern "C" int svo_submit_export_ar_occluded(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                                             const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances, const int* first,
                                             int n_instances, const svo_ar_dst* dst, int mem) {
    return submit_export_ar(c, "svo_submit_export_ar_occluded", seqs, n, style, occlusion, meshes, n_meshes, instances, first, n_instances, dst, mem);
}

extern "C" int svo_export_ar_occluded(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_occlusion* occlusion,
                                      const svo_ar_mesh* meshes, int n_meshes, const svo_ar_instance* instances, const int* first, int n_instances,
                                      const svo_ar_dst* dst, int mem) {
    const int rc = svo_submit_export_ar_occluded(c, seqs, n, style, occlusion, meshes, n_meshes, instances, first, n_instances, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_export_ar(svo_ctx* c, const int* seqs, int n, const svo_ar_style* style, const svo_ar_mesh* meshes, int n_meshes,
                             const svo_ar_instance* instances, const int* first, int n_instances, const svo_ar_dst* dst, int mem) {
    const int rc = svo_submit_export_ar(c, seqs, n, style, meshes, n_meshes, instances, first, n_instances, dst, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_map_size(svo_ctx* ctx, int seq, int from_keyframe, int* keyframes, int64_t* points_bound) {
    if (from_keyframe < 0) return svo_set_error(SVO_ERR_INVALID, "svo_map_size: from_keyframe %d", from_keyframe);
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    grp_map_size(g, s, from_keyframe, keyframes, points_bound);
    return SVO_OK;
}

extern "C" int svo_submit_save(svo_ctx* c, const int* seqs, int n, svo_snapshot* snaps, int mem) {
    if (const int rc = check_snapshot_call(c, "svo_submit_save", seqs, n, snaps, mem)) return rc;
    for (int i = 0; i < n; i++)
        if (!snaps[i].host || snaps[i].host_capacity < (int64_t)sizeof(struct svo_snapshot_info) || snaps[i].data_capacity < 0 ||
            (!snaps[i].data && snaps[i].data_capacity > 0))
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_save: snapshot %d: the host part needs room for its header, the data part its memory", i);
    if (c->failed.load()) return reject_failed(c, "svo_submit_save");
    const NamedSlots slots{seqs, n};
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::Save job;
        slots.each_in(w.first, w.count, [&](int i, int local) { job.seqs.push_back(local); job.snaps.push_back(snaps[i]); });
        if (job.seqs.empty()) continue;
        job.mem = mem;
        worker_submit(w, std::move(job));
    }
    return SVO_OK;
}

extern "C" int svo_save_sequences(svo_ctx* c, const int* seqs, int n, svo_snapshot* snaps, int mem) {
    const int rc = svo_submit_save(c, seqs, n, snaps, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_load(svo_ctx* c, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    if (const int rc = check_snapshot_call(c, "svo_submit_load", seqs, n, snaps, mem)) return rc;
    // every snapshot is parsed and checked before any group gets work
    std::vector<SnapshotLoad> loads((size_t)n);
    for (int i = 0; i < n; i++) {
        loads[i].seq = seqs[i];
        loads[i].data = snaps[i].data;
        if (const int rc = grp_check_snapshot(c->workers[0]->g.get(), &c->rigs[c->slot_rig[seqs[i]]].cam, &snaps[i], &loads[i].host))
            return rc;                           // (every group has the same size and capacity; the settings: the slot's rig's)
    }
    if (c->failed.load()) return reject_failed(c, "svo_submit_load");
    const NamedSlots slots{seqs, n};
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::Load job;
        slots.each_in(w.first, w.count, [&](int i, int local) {
            loads[i].seq = local;
            job.loads.push_back(std::move(loads[i]));
        });
        if (job.loads.empty()) continue;
        job.mem = mem;
        worker_submit(w, std::move(job));
    }
    return SVO_OK;
}

extern "C" int svo_load_sequences(svo_ctx* c, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    const int rc = svo_submit_load(c, seqs, n, snaps, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_submit_pose_updates(svo_ctx* c, const int* seqs, const int* counts, int n, const svo_pose_sample* samples,
                                       float* filtered) {
    if (!c || !counts || (seqs && n < 0)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: bad arguments");
    if (!seqs) n = c->B;
    const NamedSlots slots{seqs, n};
    const int bad = slots.first_bad(c->B, true);
    std::vector<int64_t> first((size_t)n + 1, 0);     // sample offsets of the named slots
    for (int i = 0; i < n; i++) {                // (a slot's name is checked before its count)
        if (i == bad)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: sequence %d is out of range or named twice", slots.at(i));
        if (counts[i] < 0) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: sequence %d: negative count", slots.at(i));
        first[i + 1] = first[i] + counts[i];
    }
    const int64_t total = first[n];
    if (total > (1 << 24)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: %lld samples in one call", (long long)total);
    if (total > 0 && !samples) return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: no samples");
    for (int64_t k = 0; k < total; k++)
        if (samples[k].flags & ~(uint32_t)SVO_POSE_SAMPLE_CHAIN)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_pose_updates: sample %lld: unknown flag bits 0x%x", (long long)k, samples[k].flags);
    if (c->failed.load()) return reject_failed(c, "svo_submit_pose_updates");
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::PoseUpdates u;
        slots.each_in(w.first, w.count, [&](int i, int local) {
            if (counts[i] == 0) return;
            u.seqs.push_back(local);
            u.counts.push_back(counts[i]);
            u.samples.insert(u.samples.end(), samples + first[i], samples + first[i + 1]);
            u.filtered.push_back(filtered ? filtered + first[i] * 6 : nullptr);
        });
        if (!u.seqs.empty()) worker_submit(w, std::move(u));
    }
    return SVO_OK;
}

extern "C" int svo_update_poses(svo_ctx* c, const int* seqs, const int* counts, int n, const svo_pose_sample* samples,
                                float* filtered) {
    const int rc = svo_submit_pose_updates(c, seqs, counts, n, samples, filtered);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_snapshot_size(svo_ctx* ctx, int seq, int64_t* host_bytes, int64_t* data_bytes) {
    svo_group* g; int s;
    if (const int rc = ctx_seq(ctx, seq, &g, &s)) return rc;
    return grp_snapshot_size(g, s, host_bytes, data_bytes);
}

extern "C" int svo_drop_finished_runs(svo_ctx* c, int seq) {
    if (!c || seq >= c->B) return svo_set_error(SVO_ERR_INVALID, "bad ctx / sequence index");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    for (auto& w : c->workers) {
        if (seq < 0) grp_drop_finished_runs(w->g.get(), -1);
        else if (seq >= w->first && seq < w->first + w->count) grp_drop_finished_runs(w->g.get(), seq - w->first);
    }
    return SVO_OK;
}

extern "C" int svo_ctx_get_memory(svo_ctx* c, svo_memory* out) {
    if (!c || !out) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_get_memory: bad arguments");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    std::memset(out, 0, sizeof(*out));
    for (auto& w : c->workers) {
        const svo_memory m = grp_memory(w->g.get());
        out->device_bytes += m.device_bytes; out->klt_cache_bytes += m.klt_cache_bytes;
        out->image_sets += m.image_sets; out->image_sets_free += m.image_sets_free;
        out->keyframe_slabs += m.keyframe_slabs; out->keyframe_slabs_free += m.keyframe_slabs_free;
    }
    out->device_bytes += (int64_t)c->rig_map_bytes();
    return SVO_OK;
}

extern "C" int svo_wait(svo_ctx* c) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "svo_wait: bad ctx");
    return ctx_drain(c);
}

extern "C" int svo_new_images(svo_ctx* c, const uint8_t* const* left, const uint8_t* const* right,
                              int stride, const float* time_stamps, int mem) {
    const int rc = svo_submit_images(c, left, right, stride, time_stamps, mem);
    return rc ? rc : svo_wait(c);
}

extern "C" int svo_new_image(svo_ctx* c, const uint8_t* left, int left_stride, const uint8_t* right,
                             int right_stride, int width, int height, float time_stamp) {
    if (!c || c->B != 1) return svo_set_error(SVO_ERR_INVALID, "svo_new_image needs a 1-sequence ctx");
    if (width != c->width || height != c->height || (!c->one_buffer() && left_stride != right_stride))
        return svo_set_error(SVO_ERR_INVALID, "svo_new_image: image size / stride mismatch");
    return grp_new_images(c->workers[0]->g.get(), &left, &right, left_stride, &time_stamp, SVO_MEM_HOST);
}

extern "C" int svo_ctx_set_input_format(svo_ctx* c, int format) {
    if (!c || !svo::ingest_format(format))
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_set_input_format: unknown format %d", format);
    const int rc = ctx_drain(c);                  // (the groups are idle from here on)
    if (rc) return rc;
    // a group that cannot get its image table keeps the old format, and so does the ctx: the groups before it go back
    for (size_t i = 0; i < c->workers.size(); i++) {
        const int e = grp_set_input_format(c->workers[i]->g.get(), format);
        if (e == SVO_OK) continue;
        for (size_t k = 0; k < i; k++) (void)grp_set_input_format(c->workers[k]->g.get(), c->input_format);
        return e;
    }
    c->input_format = format;
    return SVO_OK;
}

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
    if (!c || (given != 0 && given != 4) || (mem != SVO_MEM_HOST && mem != SVO_MEM_DEVICE))
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

}  // namespace

namespace {

// the checks both ways of adding rigs share: the ten floats, all four maps or none, mem, _reserved
int check_rigs(const char* who, const svo_rig* rigs, int n) {
    for (int i = 0; i < n; i++) {
        const svo_rig& r = rigs[i];
        const float v[10] = {r.baseline, r.fx, r.fy, r.cx, r.cy, r.k1, r.k2, r.k3, r.p1, r.p2};
        for (float x : v)
            if (!std::isfinite(x)) return svo_set_error(SVO_ERR_INVALID, "%s: rig %d has a value that is not finite", who, i);
        if (!(r.fx > 0) || !(r.fy > 0)) return svo_set_error(SVO_ERR_INVALID, "%s: rig %d: fx and fy must be positive", who, i);
        const int given = (r.left_map_x != nullptr) + (r.left_map_y != nullptr) + (r.right_map_x != nullptr) + (r.right_map_y != nullptr);
        if ((given != 0 && given != 4) || (given == 4 && r.mem != SVO_MEM_HOST && r.mem != SVO_MEM_DEVICE) || r._reserved != 0)
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
    for (int i = 0; i < n; i++) {                // (a slot's name is checked before its rig)
        if (i == bad)
            return svo_set_error(SVO_ERR_INVALID, "svo_ctx_assign_rigs: sequence %d out of range", seqs[i]);
        if (!rig_exists(c, rigs[i])) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_assign_rigs: rig %d does not exist", rigs[i]);
    }
    if (c->failed.load()) return reject_failed(c, "svo_ctx_assign_rigs");
    const size_t map_bytes = svo::remap_map_bytes(c->width, c->height);
    for (auto& wp : c->workers) {
        svo_ctx::Worker& w = *wp;
        svo_ctx::RigAssign job;
        slots.each_in(w.first, w.count, [&](int i, int local) {
            const svo_ctx::Rig& r = c->rigs[rigs[i]];
            const uint8_t* base = r.maps.get();
            job.seqs.push_back(local);
            job.bindings.push_back(RigBinding{rigs[i], r.cam, {base, base ? base + map_bytes : nullptr}});
        });
        if (!job.seqs.empty()) worker_submit(w, std::move(job));
    }
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

extern "C" int svo_ctx_set_exact_pinv(svo_ctx* c, int on);
extern "C" int svo_ctx_set_fast_solver(svo_ctx* c, int on) { return svo_ctx_set_exact_pinv(c, on == 0); }

extern "C" int svo_ctx_set_exact_pinv(svo_ctx* c, int on) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "bad ctx");
    const int rc = ctx_drain(c);
    if (!rc)
        for (auto& w : c->workers) grp_set_exact_pinv(w->g.get(), on);
    return rc;
}

extern "C" int svo_ctx_enable_timing(svo_ctx* c, int on) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "bad ctx");
    const int rc = ctx_drain(c);
    if (!rc)
        for (auto& w : c->workers) grp_enable_timing(w->g.get(), on);
    return rc;
}

extern "C" int svo_get_totals(svo_ctx* c, svo_totals* out) {
    if (!c || !out) return svo_set_error(SVO_ERR_INVALID, "svo_get_totals: bad arguments");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    std::memset(out, 0, sizeof(*out));
    for (auto& w : c->workers) {
        const svo_totals t = grp_totals(w->g.get());
        out->frames += t.frames; out->keyframes += t.keyframes; out->keypoints += t.keypoints;
        out->gn_gradient_calls += t.gn_gradient_calls; out->gn_cost_calls += t.gn_cost_calls;
        for (int i = 0; i < 8; i++) out->stage_ms[i] += t.stage_ms[i];
        out->wall_ms = std::max(out->wall_ms, t.wall_ms);
        out->launches += t.launches;
        out->image_sets += t.image_sets;
    }
    out->n_groups = (int)c->workers.size();
    return SVO_OK;
}

extern "C" int svo_ctx_get_launch_shapes(svo_ctx* c, svo_launch_shape* out, int max, int* n) {
    if (!c || !n || max < 0 || (max > 0 && !out)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_get_launch_shapes: bad arguments");
    const int rc = ctx_drain(c);
    if (rc) return rc;
    std::vector<svo_launch_shape> all;
    for (auto& w : c->workers)
        for (const svo_launch_shape& e : grp_launch_shapes(w->g.get())) {
            auto it = std::find_if(all.begin(), all.end(), [&e](const svo_launch_shape& a) {
                return a.kernel == e.kernel && a.waves == e.waves && a.mode == e.mode && a.cap == e.cap;
            });
            if (it == all.end()) all.push_back(e);
            else it->launches += e.launches;
        }
    std::sort(all.begin(), all.end(), [](const svo_launch_shape& a, const svo_launch_shape& b) {
        if (a.kernel != b.kernel) return a.kernel < b.kernel;
        if (a.waves != b.waves) return a.waves < b.waves;
        if (a.mode != b.mode) return a.mode < b.mode;
        return a.cap < b.cap;
    });
    *n = (int)all.size();
    for (int i = 0; i < std::min(max, *n); i++) out[i] = all[i];
    return SVO_OK;
}

// ------------------------------------------------------------------ per-sequence getters of the C ABI
// (each one starts at ctx_seq: the queues have drained, so the group's state is read between two steps)

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
