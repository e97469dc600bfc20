// svo_group_step.hip — the step of a sequence group (grp_new_images): one frame of every sequence that got
// images, as its phases, select_sequences ... book_frame. A tracked frame is nine launches on the group's stream,
// one blocking read-back of the result block, and (only when a keyframe is due) a second batch of five launches.
// The state is svo_group_state.hpp; storage and the deferred pose-filter update are svo_group.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

// one call of the step: its input and what its phases hand on
struct Step {
    const uint8_t* const* left;
    const uint8_t* const* right;
    int stride, mem;
    const float* time_stamps;
    std::vector<int> act;        // the sequences that take part, in slot order: they get pyramids
    std::vector<int> trk;        // of these, the ones with a previous frame: they run the tracked frame's kernels
    std::vector<int> start;      // [B] 1: this is frame 0 of the sequence (the slot was empty): no tracking, a keyframe
    std::vector<int> need;       // [B] 1: the sequence makes a keyframe in this step
    int pyr_stream = -1;         // row block of the row-streaming pyramid kernel, 0: some frame does not fit it
    // rectification: the active sequences whose rig has maps, in slot order (the storage of their two maps, their
    // left and right table entries); once packed: do they all share their maps (then the single-map launch), else
    // the chunks of the multi-map launch and whether every chunk is one image
    struct Remap { const uint8_t* map[2]; RemapImg left, right; };
    std::vector<Remap> remap;
    bool remap_shared = true, remap_single = false;
    int remap_chunks = 0;
    bool copy_right = false;     // some sequence's right image is copied by the pyramid launch
    float stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t0, lap_start;
};

hipError_t mark(svo_group* c, int i) {
    return c->timing ? hipEventRecord(c->ev[i].get(), c->stream.get()) : hipSuccess;
}

void lap(svo_group* c, Step& s, int phase) {
    const auto now = std::chrono::steady_clock::now();
    c->host_ms[phase] += std::chrono::duration<double, std::milli>(now - s.lap_start).count();
    s.lap_start = now;
}

// Sequences whose image pointers are NULL sit this step out (their state is untouched; an empty slot stays
// empty): a ctx can hold sequences of different lengths. An empty slot that gets a frame starts a sequence
// with it. The sequences of a launch are packed into the first slots of its argument arrays, so every
// launch covers exactly the sequences it is for.
int select_sequences(svo_group* c, Step& s) {
    s.act.reserve(c->B);
    s.trk.reserve(c->B);
    s.start.assign(c->B, 0);
    s.need.assign(c->B, 0);
    const bool one_buffer = c->fmt->buffers == 1;
    for (int q = 0; q < c->B; q++)
        if (s.left[q] && (one_buffer || s.right[q])) {
            s.act.push_back(q);
            if (c->seqs[q].frame_id < 0) s.start[q] = 1;
            else s.trk.push_back(q);
        } else if (!one_buffer && (s.left[q] != nullptr) != (s.right[q] != nullptr)) {
            return svo_set_error(SVO_ERR_INVALID, "svo_new_images: sequence %d has only one image", q);
        }
    return SVO_OK;
}

// host-resident frames into the staging buffer: slots 0..B-1 left frames, B..2B-1 right frames (a one-buffer
// input format: slots 0..B-1, one side only)
int stage_host_frames(svo_group* c, const Step& s) {
    const int B = c->B;
    const size_t row_bytes = (size_t)ingest_row_pixels(*c->fmt, c->width) * c->fmt->channels;
    const size_t used = (size_t)(c->height - 1) * s.stride + row_bytes;     // bytes of one frame that are read
    const size_t fb = align_up((size_t)c->height * s.stride, 256);
    if (fb > c->stage_frame_bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        const int rc = dev_alloc(c, &c->d_stage_in, fb * 2 * B);    // (an outgrown buffer is freed with the group)
        if (rc) return rc;
        c->stage_frame_bytes = fb;
    }
    // host frames that follow each other at exactly one frame's distance (one [B][H][stride] block per
    // side) go as ONE 2D copy: a "row" is a whole frame
    const size_t spacing = (size_t)c->height * s.stride;
    for (int side = 0; side < c->fmt->buffers; side++) {
        const uint8_t* const* src = side ? s.right : s.left;
        int s0 = 0;
        while (s0 < B) {
            if (!src[s0]) { s0++; continue; }
            int s1 = s0 + 1;
            while (s1 < B && src[s1] && src[s1] == src[s1 - 1] + spacing) s1++;
            uint8_t* dst = c->d_stage_in + (size_t)(side * B + s0) * c->stage_frame_bytes;
            if (s1 - s0 > 1) {
                HIP_TRY(hipMemcpy2DAsync(dst, c->stage_frame_bytes, src[s0], spacing, spacing, s1 - s0,
                                         hipMemcpyHostToDevice, c->stream.get()));
            } else {
                HIP_TRY(hipMemcpyAsync(dst, src[s0], used, hipMemcpyHostToDevice, c->stream.get()));
            }
            s0 = s1;
        }
    }
    return SVO_OK;
}

// the storage of the two maps that rectify the slot's frames (its rig's; rig 0: the ctx's), or nulls
void slot_maps(const svo_group* c, const Seq& q, const uint8_t* maps[2]) {
    for (int side = 0; side < 2; side++)
        maps[side] = q.rig ? q.rig_maps[side] : c->rect ? reinterpret_cast<const uint8_t*>(c->rect[side].xy) : nullptr;
}

// the image table of the step's remap launch, and for maps that differ its chunk table
void pack_remap(svo_group* c, Step& s) {
    const int R = (int)s.remap.size();
    for (const Step::Remap& r : s.remap)
        s.remap_shared = s.remap_shared && r.map[0] == s.remap[0].map[0] && r.map[1] == s.remap[0].map[1];
    std::vector<int> order((size_t)R);
    for (int k = 0; k < R; k++) order[k] = k;
    if (!s.remap_shared) {
        // a rig's two maps are one allocation: the left map's address names the rig
        std::vector<const uint8_t*> rigs;
        for (const Step::Remap& r : s.remap) rigs.push_back(r.map[0]);
        std::sort(rigs.begin(), rigs.end());
        rigs.erase(std::unique(rigs.begin(), rigs.end()), rigs.end());
        std::vector<int> map_of((size_t)R);
        for (int k = 0; k < R; k++) map_of[k] = (int)(std::lower_bound(rigs.begin(), rigs.end(), s.remap[k].map[0]) - rigs.begin());
        std::vector<RemapChunkSpan> spans;
        s.remap_single = remap_chunks(map_of.data(), R, order, spans) == 1;
        s.remap_chunks = (int)spans.size();                    // (<= R <= B: the table's size)
        for (int k = 0; k < s.remap_chunks; k++) {
            const Step::Remap& r = s.remap[order[spans[k].first]];
            c->args.remap_chunk.h[k] = RemapChunk{{r.map[0], r.map[1]}, spans[k].first, spans[k].count};
        }
    }
    for (int k = 0; k < R; k++) {
        c->remap_img.h[k] = s.remap[order[k]].left;
        c->remap_img.h[R + k] = s.remap[order[k]].right;
    }
}

// every active sequence takes a fresh image set; its pyramid arguments
int pack_pyramids(svo_group* c, Step& s) {
    bool any_rect = false;
    for (int seq : s.act) {
        const uint8_t* maps[2];
        slot_maps(c, c->seqs[seq], maps);
        any_rect = any_rect || maps[0] != nullptr;
    }
    if (converts(c->input_format) && any_rect && !c->d_raw_gray) {
        c->raw_plane_bytes = align_up(align_up((size_t)c->width, 64) * c->height, 256);
        const int rc = dev_alloc(c, &c->d_raw_gray, c->raw_plane_bytes * 2 * c->B, false);
        if (rc) return rc;
    }
    for (int j = 0; j < (int)s.act.size(); j++) {
        const int seq = s.act[j];
        Seq& q = c->seqs[seq];
        release_set(q, q.prev_set);
        q.prev_set = q.cur_set;
        const int rc = acquire_set(c, q, &q.cur_set);
        if (rc) return rc;
        ImageSet* is = q.cur_set;
        PyrArgs& hs = clear(c->args.pyr.h[j]);
        hs.n_levels = c->cam.max_pyramid_levels;
        // the sequence's buffers on the device (in place, or in the staging buffer), and its two gray images in them
        const bool host = s.mem == SVO_MEM_HOST;
        const uint8_t* buf[2];
        buf[0] = host ? c->d_stage_in + (size_t)seq * c->stage_frame_bytes : s.left[seq];
        buf[1] = c->fmt->buffers == 1 ? buf[0] : host ? c->d_stage_in + (size_t)(c->B + seq) * c->stage_frame_bytes : s.right[seq];
        const uint8_t* src_l = buf[c->fmt->left.buffer] + (size_t)c->fmt->left.start * c->width;    // (gray formats; unused
        const uint8_t* src_r = buf[c->fmt->right.buffer] + (size_t)c->fmt->right.start * c->width;  //  when the format converts)
        const int M = (int)s.act.size();
        const uint8_t* maps[2];
        slot_maps(c, q, maps);
        const bool rect = maps[0] != nullptr;
        if (converts(c->input_format)) {
            // the ingest launch makes the gray images: straight into the set's own level 0 and right image, or,
            // with rectification on, into the group's raw planes, which the remap then reads (dense rows of the
            // aligned width). The pyramids are built from the set's own images (no ingest of theirs).
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            ImgView gray_l = is->own_left0, gray_r = is->own_right;
            if (rect) {
                const int pitch = (int)align_up((size_t)c->width, 64);
                gray_l = ImgView{c->d_raw_gray + (size_t)seq * c->raw_plane_bytes, c->width, c->height, pitch};
                gray_r = ImgView{c->d_raw_gray + (size_t)(c->B + seq) * c->raw_plane_bytes, c->width, c->height, pitch};
                s.remap.push_back({{maps[0], maps[1]}, RemapImg{gray_l, is->own_left0}, RemapImg{gray_r, is->own_right}});
            }
            c->ingest_img.h[j] = ingest_image(*c->fmt, 0, buf[c->fmt->left.buffer], s.stride, gray_l);
            c->ingest_img.h[M + j] = ingest_image(*c->fmt, 1, buf[c->fmt->right.buffer], s.stride, gray_r);
            hs.src_left = is->left[0];
        } else if (rect) {
            // rectification: the raw frames (in place, or from the staging buffer) are remapped into the
            // set's own level 0 and right image, then the pyramids are built from there (no ingest)
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            s.remap.push_back({{maps[0], maps[1]}, RemapImg{ImgView{src_l, c->width, c->height, s.stride}, is->own_left0},
                               RemapImg{ImgView{src_r, c->width, c->height, s.stride}, is->own_right}});
            hs.src_left = is->left[0];
        } else if (s.mem == SVO_MEM_DEVICE_BORROW) {
            // level 0 of both pyramids and the right image ARE the caller's images (like the
            // reference's shallow cv::Mat alias, stereo_slam.cpp:115): nothing is copied
            is->left[0] = ImgView{src_l, c->width, c->height, s.stride};
            is->right = ImgView{src_r, c->width, c->height, s.stride};
            hs.src_left = is->left[0];
        } else {
            // frames are ingested by the pyramid kernel itself (one launch for all sequences instead of
            // 2 copies per sequence); host-resident ones come through the staging buffer
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            hs.src_left = ImgView{src_l, c->width, c->height, s.stride};
            hs.src_right = ImgView{src_r, c->width, c->height, s.stride};
            hs.dst_right = is->right;
            s.copy_right = true;
        }
        is->lk[0] = is->left[0];
        for (int l = 0; l < hs.n_levels; l++) hs.level[l] = is->left[l];
        hs.n_lk = c->n_lk;
        for (int l = 0; l < c->n_lk; l++) hs.lk[l] = is->lk[l];
        const int rows = pyr_stream_rows(hs);
        s.pyr_stream = (s.pyr_stream == 0 || rows == 0) ? 0 : std::max(s.pyr_stream, rows);
    }
    if (!s.remap.empty()) pack_remap(c, s);
    return SVO_OK;
}

// compaction of the sequence's current keypoint set into the other one, which becomes current
// (mode 0: remove_outliers, 1: find_bad_keypoints)
CompactArgs& pack_compact(svo_group* c, Seq& q, int slot, int mode) {
    CompactArgs& ca = clear(c->args.compact.h[slot]);
    ca.src = q.kps[q.cur]; ca.dst = q.kps[q.cur ^ 1]; ca.mode = mode;
    q.cur ^= 1;
    return ca;
}

// disparity search on the current keypoints: tracked frames clamp to half the window, keyframes
// search from the first new keypoint on (first_ptr)
void pack_ssd(svo_group* c, const Seq& q, int slot, int clamp_half, const int* first_ptr) {
    SsdArgs& sa = clear(c->args.ssd.h[slot]);
    const KpsDev& k = q.kps[q.cur];
    sa.left = q.cur_set->left[0]; sa.right = q.cur_set->right;
    sa.n_ptr = k.n; sa.kps2d = k.kps2d; sa.disparity = q.disparity;
    sa.win = c->cam.window_size_depth_calculator; sa.search_x = c->cam.search_x;
    sa.search_y = c->cam.search_y; sa.clamp_half = clamp_half;
    sa.first = 0; sa.first_ptr = first_ptr;
}

// arguments of the tracked frame's kernels: tracked sequence j in slot j
void pack_tracking_args(svo_group* c, const Step& st) {
    ArgBlocks& a = c->args;
    for (int slot = 0; slot < (int)st.trk.size(); slot++) {
        const int s = st.trk[slot];
        Seq& q = c->seqs[s];
        FrameResult* dr = c->d_res + s;
        // predicted pose = kf.statePre (stereo_slam.cpp:183-192)
        // (== statePost while the previous frame's filter update is still pending, dt = 0)
        for (int i = 0; i < 6; i++) a.guess.h[s][i] = q.pending ? q.kf.statePost[i] : q.kf.statePre[i];
        pack_compact(c, q, slot, 0).min_kf = &dr->min_kf;     // remove_outliers: the result is the frame's keypoints
        const KpsDev& k = q.kps[q.cur];
        SiaArgs& sa = clear(a.sia.h[slot]);
        for (int l = 0; l < c->cam.max_pyramid_levels; l++) {
            sa.prev[l] = q.prev_set->left[l];
            sa.cur[l] = q.cur_set->left[l];
        }
        sa.cam = q.cam; sa.n_ptr = k.n; sa.kps2d = k.kps2d; sa.kps3d = k.kps3d; sa.flags = k.flags;
        sa.pose_guess = a.guess.d[s]; sa.pose_out = dr->pose_sia; sa.cost_out = &dr->sia_cost;
        sa.trace = dr->sia_trace; sa.kp_ws = q.sia_kpws;
        sa.rec_ws = q.sia_rec; sa.rec_cap = c->rec_cap;
        sa.mats_out = q.sia_mats;
        sa.dbg_H = nullptr; sa.dbg_level = -1; sa.cap = c->cap; sa.exact_pinv = c->exact_pinv;
        KltArgs& ka = clear(a.klt.h[slot]);
        ka.kfs = q.d_kfs; ka.kf_mask = c->max_kf - 1; ka.kf_id = k.kf_id; ka.n_cur = c->n_lk;
        for (int l = 0; l < c->n_lk; l++) ka.cur[l] = q.cur_set->lk[l];
        ka.n_ptr = k.n; ka.prev_pts = nullptr; ka.cur_pts = q.tracked; ka.status = q.klt_status;
        ka.err = q.klt_err; ka.win = c->cam.window_size_opt_flow;
        ka.proj_pose = dr->pose_sia; ka.proj_mats = q.sia_mats; ka.kps3d = k.kps3d; ka.proj_out = k.kps2d;
        ka.kp_index = k.kp_index; ka.ref_out = nullptr; ka.cam = q.cam;
        ReprojArgs& ra = clear(a.reproj.h[slot]);
        ra.cam = q.cam; ra.n_ptr = k.n; ra.kps2d = k.kps2d; ra.kps3d = k.kps3d; ra.flags = k.flags;
        ra.tracked = q.tracked; ra.err = q.klt_err; ra.pose_in = dr->pose_sia;
        ra.pose_out = dr->pose_refined; ra.cost_out = &dr->reproj_cost; ra.trace = &dr->reproj_trace;
        ra.exact_pinv = c->exact_pinv;
        ra.zero_out = c->d_inside + s;      // filter_update_kernel adds to it
        pack_ssd(c, q, slot, 1, nullptr);
        fill_filter_table_args(clear(a.filter.h[slot]), q.cam, k, dr->pose_refined, q.disparity, q.d_kfs, c->max_kf - 1,
                               c->width, c->height, c->d_inside + s);
    }
}

// one more launch of `kernel` (SVO_KERNEL_*) in shape `sh`
void count_launch(svo_group* c, int kernel, const LaunchShape& sh) {
    for (svo_launch_shape& e : c->launch_shapes)
        if (e.kernel == kernel && e.waves == sh.waves && e.mode == sh.mode && e.cap == sh.cap) {
            e.launches++;
            return;
        }
    c->launch_shapes.push_back({kernel, sh.waves, sh.mode, sh.cap, 1});
}

// the arguments upload, the pyramids of every sequence with a frame and the tracked frame's kernels for those
// that have a previous one; their inside-counters go back to the host for the keyframe decision
int launch_tracking(svo_group* c, const Step& s) {
    const ArgBlocks& a = c->args;
    hipStream_t st = c->stream.get();
    const int M = (int)s.act.size(), T = (int)s.trk.size();
    HIP_TRY(hipMemcpyAsync(a.dev, a.host.get(), s.remap_chunks ? a.frame_rig_bytes : a.frame_bytes, hipMemcpyHostToDevice, st));
    const bool ingest = converts(c->input_format);
    if (ingest) {
        // both sides of every active sequence in one launch (chunks of the grid's z limit)
        HIP_TRY(hipMemcpyAsync(c->ingest_img.d, c->ingest_img.h, sizeof(IngestImg) * 2 * M, hipMemcpyHostToDevice, st));
        for (int i0 = 0; i0 < 2 * M; i0 += 32768) {
            launch_ingest(c->ingest_img.d + i0, std::min(32768, 2 * M - i0), c->width, c->height, st);
            HIP_TRY(hipGetLastError());
        }
    }
    if (const int R = (int)s.remap.size()) {
        // both sides of every sequence that is rectified in one launch: the single-map kernel while they share their
        // maps (rig 0 only, or one rig for all of them), else a map per chunk (its table went up with the arguments)
        HIP_TRY(hipMemcpyAsync(c->remap_img.d, c->remap_img.h, sizeof(RemapImg) * 2 * R, hipMemcpyHostToDevice, st));
        if (s.remap_shared) {
            RemapLaunch ra;
            for (int side = 0; side < 2; side++)
                ra.map[side] = remap_map_view(const_cast<uint8_t*>(s.remap[0].map[side]), c->width, c->height);
            ra.img = c->remap_img.d; ra.n = R;
            launch_remap(ra, 2, st);
        } else {
            RemapMultiLaunch ra;
            clear(ra);
            ra.chunks = a.remap_chunk.d; ra.img = c->remap_img.d; ra.n = R;
            launch_remap_multi(ra, c->width, c->height, s.remap_chunks, s.remap_single, 2, st);
        }
        HIP_TRY(hipGetLastError());
    }
    launch_pyr_fused(a.pyr.d, M, c->width, c->height, s.copy_right, std::max(s.pyr_stream, 0), st);
    HIP_TRY(hipGetLastError());   // (every launch is checked on its own: a later success must not mask a failure)
    HIP_TRY(mark(c, 1));
    if (T == 0) {                 // only starting sequences: the stages of a tracked frame are empty
        for (int i = 2; i <= 7; i++) HIP_TRY(mark(c, i));
        return SVO_OK;
    }
    launch_compact(a.compact.d, T, c->cap, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 2));
    // the compaction can only shrink a sequence's keypoint set, so last frame's counts bound the
    // grids and the alignment kernel's LDS working set
    int grid_n = 1;
    for (int seq : s.trk) grid_n = std::max(grid_n, c->seqs[seq].n_host);
    grid_n = std::min(grid_n, c->cap);
    // (the launchers take the ctx's settings: launch_sia and sia_pick_shape read max_pyramid_levels and
    // min_pyramid_level_pose_estimation, launch_klt, launch_ssd and launch_detect are given windows, search ranges and
    // grid sizes: integer settings only, which no rig changes. A slot's intrinsics are in its argument blocks.)
    const LaunchStatus sia_launch =
        launch_sia(a.sia.d, T, c->cam, c->width, c->height, grid_n, c->rec_cap, c->exact_pinv, st);
    HIP_TRY(sia_launch.err);
    if (!sia_launch.shape.fits)
        return svo_set_error(SVO_ERR_CAPACITY, "sparse alignment: %d keypoints exceed the workspaces", grid_n);
    count_launch(c, SVO_KERNEL_SIA_GN, sia_launch.shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 3));
    launch_klt(a.klt.d, T, grid_n, c->cam.window_size_opt_flow, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 4));
    const LaunchStatus reproj_launch = launch_reproj(a.reproj.d, T, grid_n, st);
    HIP_TRY(reproj_launch.err);
    if (!reproj_launch.shape.fits)
        return svo_set_error(SVO_ERR_CAPACITY, "reprojection GN: %d keypoints do not fit LDS", grid_n);
    count_launch(c, SVO_KERNEL_REPROJ_GN, reproj_launch.shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 5));
    launch_ssd(a.ssd.d, T, grid_n, c->cam.window_size_depth_calculator, c->cam.search_y, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 6));
    launch_filter(a.filter.d, T, grid_n, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark(c, 7));
    HIP_TRY(hipMemcpyAsync(c->h_inside, c->d_inside, sizeof(int) * c->B, hipMemcpyDeviceToHost, st));
    return SVO_OK;
}

// keyframe `id` of sequence s on its current image set; its record goes to the pinned staging slot of s
// (it reaches the device inside the KfInitArgs block: no copy per keyframe)
int new_keyframe_storage(svo_group* c, Seq& q, int s, int id) {
    if (id - q.kfs.first() >= c->max_kf)     // (the ring slot of `id` still belongs to keyframe id - max_kf)
        return svo_set_error(SVO_ERR_CAPACITY, "more than %d resident keyframes (svo_trim_keyframes makes room)", c->max_kf);
    KfHost k{};
    if (const int rc = take_kf_slab(c, &k.kps)) return rc;
    k.set = q.cur_set;
    q.cur_set->refs++;
    q.kfs.push_back(k);
    fill_kf_record(c, q, id, k, c->args.kf_record.h[s]);
    return SVO_OK;
}

// arguments of the keyframe kernels for sequence s in `slot`: a new keyframe `id`
int pack_keyframe_args(svo_group* c, int slot, int s, bool first_frame) {
    ArgBlocks& a = c->args;
    Seq& q = c->seqs[s];
    FrameResult* dr = c->d_res + s;
    const int id = (int)q.kfs.size();
    const int rc = new_keyframe_storage(c, q, s, id);
    if (rc) return rc;
    // find_bad_keypoints: cur -> other, then the other set is current
    CompactArgs& ca = pack_compact(c, q, slot, 1);
    ca.width = c->width; ca.height = c->height;
    ca.zero = q.n_det; ca.zero_count = SVO_MAX_PYRAMID_LEVELS;      // (detection counters: cleared by the compaction kernel)
    if (first_frame) {
        // a sequence starts: no keypoints, and the slot's result block as a fresh ctx has it (no stream
        // operation of its own per starting sequence)
        ca.start = 1;
        ca.zero_res = reinterpret_cast<int*>(dr); ca.zero_res_count = (int)(sizeof(FrameResult) / sizeof(int));
    }
    DetectArgs& da = clear(a.detect.h[slot]);
    for (int l = 0; l < c->cam.max_pyramid_levels; l++) da.level[l] = q.cur_set->left[l];
    da.n_levels = c->det_levels; da.grid_w = c->cam.grid_width; da.grid_h = c->cam.grid_height;
    da.out = q.det; da.n_out = q.n_det; da.max_cells = c->max_cells;
    MergeArgs& ma = clear(a.merge.h[slot]);
    ma.cam = q.cam; ma.width = c->width; ma.height = c->height;
    ma.det = q.det; ma.n_det = q.n_det; ma.n_levels = c->det_levels; ma.max_cells = c->max_cells;
    ma.kps = q.kps[q.cur]; ma.cap = c->cap;
    ma.sel = q.sel; ma.sel_level = q.sel_level; ma.sel_cell = q.sel_cell; ma.occupied = q.occupied;
    ma.old_count = &dr->old_count; ma.overflow = &dr->overflow;
    pack_ssd(c, q, slot, 0, &dr->old_count);
    KfInitArgs& ia = clear(a.kf_init.h[slot]);
    ia.cam = q.cam; ia.kps = q.kps[q.cur]; ia.old_count = &dr->old_count;
    ia.disparity = q.disparity; ia.frame_pose = dr->pose_refined;
    ia.first_frame = first_frame ? 1 : 0; ia.new_kf_id = id; ia.kfs = q.d_kfs; ia.kf_mask = c->max_kf - 1;
    ia.color_lcg = q.color_lcg; ia.n_out = &dr->kf_n;
    ia.record = a.kf_record.h[s];
    ia.tmpl_valid_bytes = (int)c->tmpl_valid_bytes;
    // (a trimmed keyframe has no record to take the block away from: its ring slot may be the new keyframe's own)
    ia.evict_id = (c->tmpl_kf > 0 && id - c->tmpl_kf >= q.kfs.first()) ? id - c->tmpl_kf : -1;
    return SVO_OK;
}

// keyframe creation for the sequences flagged in s.need: their argument blocks are
// packed into the first m slots, so the five launches cover exactly those sequences
int enqueue_keyframes(svo_group* c, const Step& s) {
    const ArgBlocks& a = c->args;
    hipStream_t st = c->stream.get();
    int m = 0;
    for (int seq = 0; seq < c->B; seq++) {
        if (!s.need[seq]) continue;
        const int rc = pack_keyframe_args(c, m++, seq, s.start[seq] != 0);
        if (rc) return rc;
    }
    if (m == 0) return SVO_OK;
    HIP_TRY(hipMemcpyAsync(a.dev, a.host.get(), a.bytes, hipMemcpyHostToDevice, st));
    // (a launch that fails must not be masked by the next one that succeeds: checked one by one)
    launch_compact(a.compact.d, m, c->cap, st);
    HIP_TRY(hipGetLastError());
    if (c->det_levels > 0) {
        launch_detect(a.detect.d, m, c->max_cells, c->det_levels, c->cam.grid_width, c->cam.grid_height, st);
        HIP_TRY(hipGetLastError());
    }
    launch_select_merge(a.merge.d, m, c->max_cells, st);
    HIP_TRY(hipGetLastError());
    launch_ssd(a.ssd.d, m, c->cap, c->cam.window_size_depth_calculator, c->cam.search_y, st);
    HIP_TRY(hipGetLastError());
    launch_kf_init(a.kf_init.d, m, st);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

// which sequences make a keyframe (every one that starts, stereo_slam.cpp:141-160) and their launches
int decide_keyframes(svo_group* c, Step& s) {
    // KeyFrameManager::keyframe_needed (keyframe_manager.cpp:66-72)
    const int max_keypoints = (c->width / c->cam.grid_width) * (c->height / c->cam.grid_height);
    bool any = false;
    for (int seq : s.act) {
        s.need[seq] = s.start[seq] || (double)c->h_inside[seq] < 0.66 * max_keypoints ? 1 : 0;
        any = any || s.need[seq];
    }
    return any ? enqueue_keyframes(c, s) : SVO_OK;
}

int read_stage_times(svo_group* c, Step& s) {
    HIP_TRY(mark(c, 8));
    if (!c->timing) return SVO_OK;
    HIP_TRY(hipEventSynchronize(c->ev[8].get()));
    for (int i = 0; i < 8; i++) (void)hipEventElapsedTime(&s.stage_ms[i], c->ev[i].get(), c->ev[i + 1].get());
    return SVO_OK;
}

// Keyframe images are only read for keypoints that came from that keyframe (KLT builds a template from
// them when the cache has none). The frame's keypoints — kept by the compaction at its start, plus what a
// keyframe created in this frame adds — refer to keyframes r.min_kf and younger and, of the next 64, to
// those whose bit is set in r.live_kf: the others hand their image sets back to the sequence's free
// list, so memory stays bounded by the keyframes still in use
// instead of growing with every keyframe (the reference keeps them all). Nothing else of a keyframe goes:
// its keypoint arrays, pose and table record stay for the depth filter and the getters, until the keyframe is
// trimmed (trim_keyframes).
void retire_keyframe_images(svo_group* c, const Step& s) {
    for (int seq : s.trk) {
        Seq& q = c->seqs[seq];
        const FrameResult& r = c->h_res[seq];
        const int newest = (int)q.kfs.size() - 1;                  // (never the newest: a keyframe made in this frame)
        for (; q.kfs_retired < std::min(r.min_kf, newest); q.kfs_retired++) release_set(q, q.kfs[q.kfs_retired].set);
        for (int i = 0; i < 64 && r.min_kf < newest && r.min_kf + i < newest; i++) {
            KfHost& old = q.kfs[r.min_kf + i];
            if (old.set && !((r.live_kf[i >> 5] >> (i & 31)) & 1u)) release_set(q, old.set);
        }
    }
}

// host bookkeeping (stereo_slam.cpp:250-270); the pose filter itself is deferred
int book_frame(svo_group* c, Step& s) {
    int overflow_seq = -1;
    for (int seq : s.act) {
        Seq& q = c->seqs[seq];
        const FrameResult& r = c->h_res[seq];
        const double ts = (double)s.time_stamps[seq];
        const bool first = s.start[seq] != 0;
        q.frame_id++;
        if (first) {
            std::memset(q.pose, 0, sizeof(q.pose));
            q.ts = ts;
            q.trajectory.push_back(svo_pose{});         // (the zero pose)
        } else {
            q.pending = true;
            std::memcpy(q.pending_pose, r.pose_refined, sizeof(q.pending_pose));
            q.pending_ts = ts;
        }
        if (s.need[seq]) {
            KfHost& k = q.kfs.back();
            k.n = r.kf_n;
            if (first) std::memset(k.pose, 0, sizeof(k.pose));
            else std::memcpy(k.pose, r.pose_refined, sizeof(k.pose));
        }
        q.n_host = c->h_n[2 * seq + q.cur];
        svo_frame_stats& st = clear(q.stats);
        st.frame_id = q.frame_id; st.is_keyframe = s.need[seq]; st.n_keypoints = q.n_host;
        st.n_keyframes = (int)q.kfs.size(); st.inside_count = first ? 0 : c->h_inside[seq]; st.overflow = r.overflow;
        std::memcpy(st.pose_sia, r.pose_sia, sizeof(st.pose_sia));
        std::memcpy(st.pose_refined, r.pose_refined, sizeof(st.pose_refined));
        st.sia_cost = r.sia_cost; st.reproj_cost = r.reproj_cost; st.sia_ms = s.stage_ms[2];
        std::memcpy(st.stage_ms, s.stage_ms, sizeof(s.stage_ms));
        std::memcpy(st.sia_trace, r.sia_trace, sizeof(st.sia_trace));
        st.reproj_trace = r.reproj_trace;
        c->totals.frames++;
        c->totals.keyframes += s.need[seq];
        c->totals.keypoints += q.n_host;
        if (!first)
            for (int l = 0; l < SVO_MAX_PYRAMID_LEVELS; l++) {
                c->totals.gn_gradient_calls += r.sia_trace[l].n_gradient;
                c->totals.gn_cost_calls += r.sia_trace[l].n_cost;
            }
        if (r.overflow && overflow_seq < 0) overflow_seq = seq;     // reported after every sequence is booked
    }
    lap(c, s, 6);   // bookkeeping
    c->host_steps++;
    c->totals.launches++;
    for (int i = 0; i < 8; i++) c->totals.stage_ms[i] += s.stage_ms[i];
    c->totals.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - s.t0).count();
    if (overflow_seq >= 0)
        return svo_set_error(SVO_ERR_CAPACITY, "sequence %d: more than %d keypoints", overflow_seq, c->cap);
    return SVO_OK;
}

// One frame of the group, as its phases. SVO_HOST_TIMING laps: args, launch, pose_filter, wait_frame,
// kf_enqueue, wait_kf, bookkeeping.
int step(svo_group* c, Step& s) {
    HIP_TRY(hipSetDevice(c->device));
    s.t0 = s.lap_start = std::chrono::steady_clock::now();
    int rc = select_sequences(c, s);
    if (rc || s.act.empty()) return rc;
    HIP_TRY(mark(c, 0));
    if (s.mem == SVO_MEM_HOST && (rc = stage_host_frames(c, s))) return rc;
    if ((rc = pack_pyramids(c, s))) return rc;
    pack_tracking_args(c, s);
    lap(c, s, 0);
    if ((rc = launch_tracking(c, s))) return rc;
    lap(c, s, 1);
    flush_pending(c);                     // previous frame's pose filter, overlapped with the kernels
    lap(c, s, 2);
    if (!s.trk.empty()) HIP_TRY(hipStreamSynchronize(c->stream.get()));   // the inside-counters
    lap(c, s, 3);
    if ((rc = decide_keyframes(c, s))) return rc;
    lap(c, s, 4);
    HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res, c->readback_bytes, hipMemcpyDeviceToHost, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));   // results + counts
    lap(c, s, 5);
    if ((rc = read_stage_times(c, s))) return rc;
    if (c->retire_kf_images) retire_keyframe_images(c, s);
    if (c->kf_window >= 0)                // svo_ctx_set_keyframe_window: host bookkeeping only
        for (int seq : s.trk) {
            Seq& q = c->seqs[seq];
            if (q.kfs_retired - q.kfs.first() > c->kf_window) trim_keyframes(c, q, q.kfs_retired - c->kf_window);
        }
    return book_frame(c, s);
}

}  // namespace

// A frame that fails half way (HIP error, capacity) leaves the sequences of the group at mixed
// frame ids: the group is marked failed and rejects further frames instead of tracking on.
int grp_new_images(svo_group* c, const uint8_t* const* left, const uint8_t* const* right, int stride,
                   const float* time_stamps, int mem) {
    if (!c || !left || (!right && c->fmt->buffers == 2) || !time_stamps ||
        (long long)stride < (long long)ingest_row_pixels(*c->fmt, c->width) * c->fmt->channels)
        return svo_set_error(SVO_ERR_INVALID, "svo_new_images: bad arguments");
    if (const int rc = reject_if_failed(c, "svo_new_images")) return rc;
    Step s;
    s.left = left; s.right = right; s.stride = stride; s.mem = mem; s.time_stamps = time_stamps;
    const int rc = step(c, s);
    if (rc != SVO_OK) c->failed = true;
    return rc;
}
