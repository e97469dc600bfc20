// svo_group_cloud.hip — the cloud job of a sequence group (svo_submit_export_cloud): dense coloured point clouds of
// the frames or newest keyframes of its named slots. dense.hip's kernel searches the lattice of each slot's planes
// into the group's staging block; cloud.hip's count and write kernels turn the two planes into svo_map_point
// records; and svo_cloud_size. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

constexpr size_t CLOUD_STAGING_BYTES = (size_t)256 << 20;   // the slots of one chunk of a job stage at most so much (one slot always fits)

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// The staging block of a chunk of m slots of `points` lattice points each (include/svo_hip.h states the sum):
//   m x planes | m x (tile counts, pose matrices) | host mode: m x records | kept counts
struct Staging {
    size_t planes, counts, records, slot, total;
    Staging(size_t points, bool host, size_t m)
        : planes(up256(points * 8)), counts(up256((size_t)cloud_tiles((int64_t)points) * 4) + 256), records(host ? points * 16 : 0),
          slot(planes + counts + records), total(m * slot + up256(4 * m)) {}
};

int reserve_cloud(svo_group* c, size_t bytes, size_t slots) {
    if (slots > c->cloud_counts_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        c->cloud_counts_host.reset(); c->cloud_counts_cap = 0;
        HIP_TRY(pinned_malloc(c->cloud_counts_host, sizeof(int) * slots));
        c->cloud_counts_cap = slots;
    }
    return c->d_cloud.reserve(c, bytes);
}

// the style is checked and the ctx's size has a lattice point at its step
int check_style(const svo_camera_settings* cam, int width, int height, const svo_cloud_style* style, const char* who, DenseParams* search,
                CloudParams* out) {
    DenseParams s;
    if (const int rc = cloud_check_style(style, cam, who, &s, out)) return rc;
    if (width / s.step < 1 || height / s.step < 1)
        return svo_set_error(SVO_ERR_INVALID, "%s: %d x %d has no lattice point at step %d", who, width, height, s.step);
    if (search) *search = s;
    return SVO_OK;
}

}  // namespace

extern "C" int svo_cloud_size(const svo_camera_settings* cam, int width, int height, const svo_cloud_style* style, int* cols, int* rows,
                              int64_t* points_per_slot) {
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    DenseParams s;
    if (const int rc = check_style(cam, width, height, style, "svo_cloud_size", &s, nullptr)) return rc;
    if (cols) *cols = width / s.step;
    if (rows) *rows = height / s.step;
    if (points_per_slot) *points_per_slot = (int64_t)(width / s.step) * (height / s.step);
    return SVO_OK;
}

int grp_check_cloud_style(const svo_group* c, const svo_cloud_style* style, const svo_stereo_check* check) {
    const char* who = check ? "svo_submit_export_cloud_checked" : "svo_submit_export_cloud";
    if (const int rc = check_style(&c->cam, c->width, c->height, style, who, nullptr, nullptr)) return rc;
    return lr_check_parse(check, true, who, nullptr);
}

int grp_check_cloud_sgm(const svo_group* c, const svo_cloud_style* style, const svo_sgm_params* sgm, const char* who) {
    DenseParams s;
    if (const int rc = check_style(&c->cam, c->width, c->height, style, who, &s, nullptr)) return rc;
    if (s.search_x + 1 > SGM_MAX_D) return svo_set_error(SVO_ERR_INVALID, "%s: search_x %d: at most %d with a cost volume", who, s.search_x, SGM_MAX_D - 1);
    return sgm_check_params(sgm, who, nullptr);
}

int64_t grp_cloud_points(const svo_group* c, const svo_cloud_style* style) {
    DenseParams s;
    if (cloud_check_style(style, &c->cam, "svo_submit_export_cloud", &s, nullptr) != SVO_OK) return 0;
    return (int64_t)(c->width / s.step) * (c->height / s.step);
}

int64_t grp_cloud_slot_bytes(const svo_group* c, const svo_cloud_style* style, const svo_stereo_check* check, const svo_sgm_params* sgm) {
    DenseParams s;
    if (cloud_check_style(style, &c->cam, "svo_submit_export_cloud", &s, nullptr) != SVO_OK) return 0;
    LrCheck lr;
    if (lr_check_parse(check, true, "svo_submit_export_cloud", &lr) != SVO_OK) return 0;
    const size_t points = (size_t)(c->width / s.step) * (size_t)(c->height / s.step);
    return (int64_t)(Staging(points, false, 1).slot + (lr.on && !sgm ? lr_reverse_bytes(c->width, c->height, s.step) : 0));
}

// The named slots of the group as segments and records (svo_submit_export_cloud). Named slot seg[i] of the job owns
// the records from seg[i] * points on. The slots run in chunks of at most `chunk` (one chunk unless the job stages
// more than CLOUD_STAGING_BYTES): per chunk the search of its delivered slots into the staging block's planes, the
// count and write launches over them (device mode: into the caller's records; host mode: into the block's), one copy
// of the kept counts, and in host mode the copies out: each slot's kept prefix (compact) or every run of slots that
// are consecutive in both (organized). The two image tables share the group's argument blocks, half each.
// A checked job (include/svo_hip.h, "cross-check") has a third table, a third of the blocks each: between the search
// and the count launch the reverse search fills the chunk's reverse planes (the group's d_lr block) and the check
// sets the staged disparity of a failing point to -1, which the count and write launches drop as an invalid point.
// An SGM job (sgm != null; include/svo_hip.h, "sgm cross-check") fills the staged planes with grp_sgm_planes in the
// place of the search, its check in the place of the reverse search and the check (no d_lr block), and the count and
// write launches read the cost plane as the sum of four paths.
int grp_export_cloud(svo_group* c, int what, int mem, const int* seqs, const int* seg, int n, int seq0, const svo_cloud_style* style,
                     const svo_stereo_check* check, const svo_cloud_dst* dst, const svo_sgm_params* sgm) {
    if (const int rc = job_begin(c, "svo_submit_export_cloud")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    DenseParams search;
    CloudParams params;
    if (const int rc = cloud_check_style(style, &c->cam, "svo_submit_export_cloud", &search, &params)) return rc;
    LrCheck lr;
    if (const int rc = lr_check_parse(check, true, "svo_submit_export_cloud", &lr)) return rc;
    SgmParams sgm_params{};
    if (sgm) {
        if (const int rc = sgm_check_params(sgm, "svo_submit_export_cloud_sgm", &sgm_params)) return rc;
        sgm_params.value = SVO_DENSE_DISPARITY;
        sgm_params.cost = 1;
        params.sgm_cost = 1;
    }
    const size_t reverse = lr.on && !sgm ? lr_reverse_bytes(c->width, c->height, search.step) : 0;
    const LrParams lr_params{SVO_DENSE_DISPARITY, search.step, lr.max_lr_diff};
    const int64_t points = (int64_t)(c->width / search.step) * (c->height / search.step);
    const bool organized = params.layout == SVO_CLOUD_ORGANIZED;
    // (SVO_CLOUD_CHUNK_SLOTS: fewer slots per chunk, so that tests reach the chunked path)
    const size_t chunk = table_tiles("SVO_CLOUD_CHUNK_SLOTS", std::max<size_t>(1, CLOUD_STAGING_BYTES / (Staging((size_t)points, host, 1).slot + reverse)));
    const size_t m_max = std::min<size_t>((size_t)n, chunk);
    const Staging sg((size_t)points, host, m_max);
    if (const int rc = reserve_cloud(c, sg.total, m_max)) return rc;
    if (lr.on && !sgm)
        if (const int rc = c->d_lr.reserve(c, m_max * reverse)) return rc;
    uint8_t* const d_planes = c->d_cloud.p;
    uint8_t* const d_counts = d_planes + m_max * sg.planes;
    uint8_t* const d_records = d_counts + m_max * sg.counts;
    int* const d_kept = reinterpret_cast<int*>(c->d_cloud.p + m_max * sg.slot);
    int* const kept = c->cloud_counts_host.get();
    const int cloud_grid = cloud_tiles(points);
    for (int i0 = 0; i0 < n; i0 += (int)m_max) {
        const int m = std::min((int)m_max, n - i0);
        std::vector<const ImageSet*> sets((size_t)m, nullptr);
        int shown = 0;
        for (int j = 0; j < m; j++) {
            const int i = i0 + j;
            const Seq& q = c->seqs[seqs[i]];
            svo_cloud_segment& e = clear(dst->segments[seg[i]]);
            e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.keyframe_id = -1;
            e.time_stamp = (float)q.ts; e.first_point = (int64_t)seg[i] * points; e.status = SVO_CLOUD_NONE;
            e.baseline = q.cam.baseline;
            const ImageSet* set = nullptr;
            if (what == SVO_EXPORT_FRAMES) {
                std::memcpy(e.pose, q.pose, sizeof(e.pose));
                if (q.frame_id >= 0) set = q.cur_set;
            } else if (!q.kfs.empty()) {
                const KfHost& k = q.kfs.back();
                e.keyframe_id = (int)q.kfs.size() - 1;
                std::memcpy(e.pose, k.pose, sizeof(e.pose));
                set = k.set;
            }
            if (!set) continue;
            const ImgView& l = set->left[0];
            const ImgView& r = set->right;
            if (l.w != c->width || l.h != c->height || r.w != l.w || r.h != l.h)
                return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_cloud: the planes are %d x %d and %d x %d, not %d x %d", l.w, l.h, r.w, r.h,
                                     c->width, c->height);
            e.status = SVO_CLOUD_OK;
            sets[(size_t)j] = set;
            shown++;
        }
        if (shown == 0) continue;
        if (sgm) {                                         // (the planes first: it uses the argument blocks itself)
            std::vector<DenseImage> images;
            for (int j = 0; j < m; j++) {
                if (!sets[(size_t)j]) continue;
                const ImgView& l = sets[(size_t)j]->left[0];
                const ImgView& r = sets[(size_t)j]->right;
                images.push_back(DenseImage{l.data, r.data, reinterpret_cast<float*>(d_planes + (size_t)j * sg.planes), l.stride, r.stride, l.w, l.h,
                                            c->seqs[seqs[i0 + j]].cam.baseline, 0});
            }
            if (const int rc = grp_sgm_planes(c, images, search, sgm_params, c->width / search.step, c->height / search.step,
                                              lr.on ? &lr_params : nullptr, -1, true))
                return rc;
        }
        const bool wta_check = lr.on && !sgm;
        // (SVO_CLOUD_TABLE_IMAGES: smaller tables, so that tests reach the chunked launches)
        DenseParams sp = search;
        int dense_grid = 0;
        auto dense = group_tile_table<DenseImage>(c, "SVO_CLOUD_TABLE_IMAGES",
                                                  [&](const DenseImage* d, int k, hipStream_t s) { launch_dense(d, k, dense_grid, sp, s); });
        auto cloud = group_tile_table<CloudImage>(c, "SVO_CLOUD_TABLE_IMAGES",
                                                  [&](const CloudImage* d, int k, hipStream_t s) { launch_cloud(d, k, cloud_grid, params, s); });
        auto checks = group_tile_table<LrImage>(c, "SVO_CLOUD_TABLE_IMAGES", [&](const LrImage* d, int k, hipStream_t s) {
            launch_dense_reverse(d, k, dense_grid, sp, s);
            launch_lr_check(d, k, lr_tiles(points), lr_params, s);
        });
        const size_t half = c->args.bytes / (wta_check ? 3 : 2) / 256 * 256;   // (a third each of a checked job's three tables)
        dense.cap = std::min({dense.cap, half / sizeof(DenseImage), DENSE_MAX_IMAGES});
        cloud.cap = std::min({cloud.cap, half / sizeof(CloudImage), DENSE_MAX_IMAGES});
        cloud.h = reinterpret_cast<CloudImage*>(reinterpret_cast<uint8_t*>(cloud.h) + half);
        cloud.d = reinterpret_cast<CloudImage*>(reinterpret_cast<uint8_t*>(cloud.d) + half);
        checks.h = reinterpret_cast<LrImage*>(reinterpret_cast<uint8_t*>(checks.h) + 2 * half);
        checks.d = reinterpret_cast<LrImage*>(reinterpret_cast<uint8_t*>(checks.d) + 2 * half);
        if (dense.cap < 1 || cloud.cap < 1) return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_cloud: the argument blocks hold no image table");
        // (checked: one cap for all three, so that the tables fill and launch in step: search, check, count and write)
        if (wta_check) dense.cap = cloud.cap = checks.cap = std::min(dense.cap, cloud.cap);
        dense_plan(sp, (long long)dense_tiles(search, c->width, c->height) * (long long)std::min<size_t>((size_t)shown, dense.cap));
        dense_grid = dense_tiles(sp, c->width, c->height);
        for (int j = 0; j < m; j++) {
            if (!sets[(size_t)j]) continue;
            const Seq& q = c->seqs[seqs[i0 + j]];
            const svo_cloud_segment& e = dst->segments[seg[i0 + j]];
            const ImgView& l = sets[(size_t)j]->left[0];
            const ImgView& r = sets[(size_t)j]->right;
            float* planes = reinterpret_cast<float*>(d_planes + (size_t)j * sg.planes);
            uint8_t* counts = d_counts + (size_t)j * sg.counts;
            svo_map_point* out = host ? reinterpret_cast<svo_map_point*>(d_records + (size_t)j * sg.records) : dst->points + e.first_point;
            if (!sgm)
                if (const int rc = dense.add(DenseImage{l.data, r.data, planes, l.stride, r.stride, l.w, l.h, q.cam.baseline, 0})) return rc;
            if (wta_check)
                if (const int rc = checks.add(LrImage{l.data, r.data, reinterpret_cast<float*>(c->d_lr.p + (size_t)j * reverse), planes, nullptr,
                                                      l.stride, r.stride, l.w, l.h, q.cam.baseline, 0}))
                    return rc;
            CloudImage ci{l.data, planes, planes + points, out, reinterpret_cast<int*>(counts), d_kept + j, l.stride, l.w, l.h,
                          q.cam.baseline, q.cam.fx, q.cam.fy, q.cam.cx, q.cam.cy, {}, reinterpret_cast<float*>(counts + sg.counts - 256)};
            std::memcpy(ci.pose, e.pose, sizeof(ci.pose));
            if (const int rc = cloud.add(ci)) return rc;
        }
        if (const int rc = dense.launch(false)) return rc;
        if (const int rc = checks.launch(false)) return rc;
        if (const int rc = cloud.launch(false)) return rc;
        HIP_TRY(hipMemcpyAsync(kept, d_kept, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int j = 0; j < m; j++)
            if (sets[(size_t)j]) dst->segments[seg[i0 + j]].n_points = kept[j];
        for (int j = 0; host && j < m;) {
            if (!sets[(size_t)j]) { j++; continue; }
            int k = j + 1;
            const svo_map_point* from = reinterpret_cast<const svo_map_point*>(d_records + (size_t)j * sg.records);
            svo_map_point* to = dst->points + (int64_t)seg[i0 + j] * points;
            if (organized) {
                while (k < m && sets[(size_t)k] && seg[i0 + k] == seg[i0 + k - 1] + 1) k++;
                HIP_TRY(hipMemcpyAsync(to, from, sizeof(svo_map_point) * (size_t)points * (size_t)(k - j), hipMemcpyDeviceToHost, st));
            } else if (kept[j] > 0) {
                HIP_TRY(hipMemcpyAsync(to, from, sizeof(svo_map_point) * (size_t)kept[j], hipMemcpyDeviceToHost, st));
            }
            j = k;
        }
        HIP_TRY(hipStreamSynchronize(st));   // delivered (svo_wait means that), and the block is free for the next chunk
    }
    return SVO_OK;
}
