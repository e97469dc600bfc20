// svo_ctx.hip — the public svo_ctx of the C ABI (svo_ctx_state.hpp): a set of sequence groups (svo_group.hpp), each
// on its own stream and host thread, with a queue of submitted jobs. Here: creation, the queue and svo_wait, the
// frame sets, restarts and keyframe trims, and the ctx-wide settings and read-outs. The other entry points of the ctx:
// svo_ctx_export.hip (the export jobs), svo_ctx_voxel.hip (the voxel maps), svo_ctx_snapshot.hip (save, load, pose
// updates), svo_ctx_rigs.hip (calibration, rectification, rigs), svo_ctx_get.hip (the per-sequence getters).
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <new>

#include "svo_ctx_state.hpp"

namespace {

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
    return grp_export_disparity(g, j.what, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.check_ptr(), j.sgm_ptr(), &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::CloudExport& j) {
    return grp_export_cloud(g, j.what, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.check_ptr(), &j.dst, j.sgm_ptr());
}
int run_job(svo_group* g, int seq0, const svo_ctx::SceneExport& j) {
    return grp_export_scenes_clouds(g, j.mem, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.cameras.data(), &j.dst,
                                    j.has_clouds ? &j.clouds : nullptr, j.extra.empty() ? nullptr : j.extra.data(), j.sgm_ptr());
}
int run_job(svo_group* g, int seq0, const svo_ctx::ArExport& j) {
    return grp_export_ar_occluded(g, j.mem, j.seqs.data(), j.seg.data(), j.inst0.data(), j.inst1.data(), (int)j.seqs.size(), seq0, j.job.get(), &j.dst,
                                  j.occluded ? &j.occlusion : nullptr, j.sgm_ptr());
}
int run_job(svo_group* g, int, const svo_ctx::Save& j) { return grp_save(g, j.seqs.data(), (int)j.seqs.size(), j.snaps.data(), j.mem); }
int run_job(svo_group* g, int, const svo_ctx::Load& j) { return grp_load(g, j.loads.data(), (int)j.loads.size(), j.mem); }
int run_job(svo_group* g, int, const svo_ctx::PoseUpdates& j) {
    return grp_pose_updates(g, j.seqs.data(), j.counts.data(), (int)j.seqs.size(), j.samples.data(), j.filtered.data());
}
int run_job(svo_group* g, int seq0, const svo_ctx::FuseClouds& j) {
    return grp_fuse_clouds(g, j.what, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.style, j.check_ptr(), j.stamp, j.info, j.sgm_ptr());
}
int run_job(svo_group* g, int seq0, const svo_ctx::VoxelExport& j) {
    return grp_export_voxel_maps(g, j.mem, j.seqs.data(), j.seg.data(), j.regions.data(), (int)j.seqs.size(), seq0, &j.filter, &j.dst);
}
int run_job(svo_group* g, int, const svo_ctx::VoxelClear& j) { return grp_clear_voxel_maps(g, j.seqs.data(), (int)j.seqs.size()); }
int run_job(svo_group* g, int seq0, const svo_ctx::VoxelPrune& j) {
    if (j.has_carve)
        return grp_carve_voxel_maps(g, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.cloud, j.sgm_ptr(), j.check_ptr(), &j.carve, &j.keep,
                                    j.center_mode, j.centers.data(), j.carve_info);
    return grp_prune_voxel_maps(g, j.seqs.data(), j.seg.data(), (int)j.seqs.size(), seq0, &j.keep, j.center_mode, j.centers.data(), j.info);
}

int run_job(svo_group* g, int seq0, const svo_ctx::VoxelSave& j) {
    return grp_save_voxel_maps(g, j.mem, j.seqs.data(), j.seg.data(), j.regions.data(), (int)j.seqs.size(), seq0, &j.filter, &j.dst);
}
int run_job(svo_group* g, int seq0, const svo_ctx::VoxelLoad& j) {
    return grp_load_voxel_maps(g, j.mode, j.mem, j.seqs.data(), j.seg.data(), j.spans.data(), (int)j.seqs.size(), seq0, j.info);
}

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

}  // namespace

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

int reject_failed(svo_ctx* c, const char* name) {
    const int rc = ctx_drain(c);
    return rc ? rc : svo_set_error(SVO_ERR_INVALID, "%s: an earlier frame of this ctx failed; create a new ctx", name);
}

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

extern "C" int svo_wait(svo_ctx* c) {
    if (!c) return svo_set_error(SVO_ERR_INVALID, "svo_wait: bad ctx");
    return ctx_drain(c);
}

// ------------------------------------------------------------------ frame sets

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

extern "C" int svo_new_images(svo_ctx* c, const uint8_t* const* left, const uint8_t* const* right,
                              int stride, const float* time_stamps, int mem) {
    return then_wait(c, svo_submit_images(c, left, right, stride, time_stamps, mem));
}

extern "C" int svo_new_image(svo_ctx* c, const uint8_t* left, int left_stride, const uint8_t* right,
                             int right_stride, int width, int height, float time_stamp) {
    if (!c || c->B != 1) return svo_set_error(SVO_ERR_INVALID, "svo_new_image needs a 1-sequence ctx");
    if (width != c->width || height != c->height || (!c->one_buffer() && left_stride != right_stride))
        return svo_set_error(SVO_ERR_INVALID, "svo_new_image: image size / stride mismatch");
    return grp_new_images(c->workers[0]->g.get(), &left, &right, left_stride, &time_stamp, SVO_MEM_HOST);
}

// ------------------------------------------------------------------ restarts, keyframe trims

extern "C" int svo_ctx_restart_sequences(svo_ctx* c, const int* seqs, int n) {
    if (!c || n < 0 || (n > 0 && !seqs)) return svo_set_error(SVO_ERR_INVALID, "svo_ctx_restart_sequences: bad arguments");
    const NamedSlots slots{seqs, n};
    if (const int bad = slots.first_bad(c->B, false); bad >= 0)   // (a slot may be named twice)
        return svo_set_error(SVO_ERR_INVALID, "svo_ctx_restart_sequences: sequence %d out of range", slots.at(bad));
    if (c->failed.load()) return reject_failed(c, "svo_ctx_restart_sequences");
    submit_shares<svo_ctx::Restart>(c, slots, every_slot, nothing_more);
    return SVO_OK;
}

extern "C" int svo_submit_trim_keyframes(svo_ctx* c, const int* seqs, const int* below, int n) {
    if (!c || !naming_ok(seqs, n)) return svo_set_error(SVO_ERR_INVALID, "svo_submit_trim_keyframes: bad arguments");
    const NamedSlots slots = ctx_slots(c, seqs, n);
    if (const int rc = check_slots(c, "svo_submit_trim_keyframes", slots)) return rc;
    if (c->failed.load()) return reject_failed(c, "svo_submit_trim_keyframes");
    submit_shares<svo_ctx::Trim>(c, slots, [&](svo_ctx::Trim& job, int i, int) {
        job.below.push_back(below ? below[i] : INT_MAX);         // (NULL: everything retired)
        return true;
    }, nothing_more);
    return SVO_OK;
}

extern "C" int svo_trim_keyframes(svo_ctx* c, const int* seqs, const int* below, int n) {
    return then_wait(c, svo_submit_trim_keyframes(c, seqs, below, n));
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

// ------------------------------------------------------------------ ctx-wide settings and read-outs

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
