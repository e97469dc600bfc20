// svo_group_dense.hip — the disparity job of a sequence group (svo_submit_export_disparity): dense disparity or depth
// maps of the frames or newest keyframes of its named slots, computed by dense.hip's kernel from the left level-0
// plane and the right image of each slot, as segments and float planes; and svo_disparity_size. The state is
// svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

constexpr size_t LR_STAGING_BYTES = (size_t)256 << 20;   // the reverse planes of one chunk of a checked job at most (one slot always fits)
constexpr size_t SGM_STAGING_BYTES = (size_t)512 << 20;  // the sums, volumes and count planes of one chunk of an SGM job at most (likewise)

// the style is checked and the ctx's size has a lattice point at its step
int check_style(const svo_camera_settings* cam, int width, int height, const svo_disparity_style* style, const char* who, DenseParams* out) {
    DenseParams p;
    if (const int rc = dense_check_style(style, cam, who, &p)) return rc;
    if (width / p.step < 1 || height / p.step < 1)
        return svo_set_error(SVO_ERR_INVALID, "%s: %d x %d has no lattice point at step %d", who, width, height, p.step);
    if (out) *out = p;
    return SVO_OK;
}

}  // namespace

// The SGM mode of the job (include/svo_hip.h, "sgm"): per chunk of delivered slots whose sums, volumes and count planes
// fit the group's d_sgm block, the cost-volume launch and the two launches of the paths, which write the slots' planes.
// The two image tables share the group's argument blocks, half each, and fill and launch in step. The stream orders a
// chunk's launches before the next chunk's, so the chunks share the block.
// check ("sgm cross-check"): a slot of the block also holds the sums, volume, count plane and disparity plane of the
// mirrored pair; a chunk of m slots has 2 m entries in the two tables, the mirrored pairs behind the forward ones (the
// mirrored cost-volume launch takes the second half, the launches of the paths all of them), and a third table, a
// third of the blocks each, carries the lattice check, which writes the lr plane (value + lr_plane floats) and masks and
// converts the value plane in place (lr_plane < 0: no lr plane, a cloud job's mask). args_reused: the caller fills the
// argument blocks again, so the last upload must be over on return.
int svo::grp_sgm_planes(svo_group* c, const std::vector<DenseImage>& images, const DenseParams& params, SgmParams sp, int cols, int rows,
                        const LrParams* check, int64_t lr_plane, bool args_reused) {
    if (images.empty()) return SVO_OK;
    const int D = params.search_x + 1;
    const size_t per = check ? 2 : 1;
    const size_t volume = sgm_volume_bytes(cols, rows, D), one = 2 * volume + sgm_count_bytes(cols, rows);
    const size_t slot = sgm_slot_bytes(cols, rows, D, check != nullptr);
    // (SVO_SGM_CHUNK_SLOTS: fewer slots per chunk, so that tests reach the chunked path)
    const size_t chunk = std::min(images.size(), table_tiles("SVO_SGM_CHUNK_SLOTS", std::max<size_t>(1, SGM_STAGING_BYTES / slot)));
    if (const int rc = c->d_sgm.reserve(c, chunk * slot)) return rc;
    DenseParams dp = params;
    int grid = 0;
    auto costs = group_tile_table<CostImage>(c, "SVO_DENSE_TABLE_IMAGES", [&](const CostImage* d, int m, hipStream_t s) {
        launch_dense_cost_volume(d, m / (int)per, grid, dp, sp.cost_cap, s);
        if (check) launch_dense_cost_volume_mirrored(d + m / 2, m / 2, grid, dp, sp.cost_cap, s);
    });
    auto sums = group_tile_table<SgmImage>(c, "SVO_DENSE_TABLE_IMAGES", [&](const SgmImage* d, int m, hipStream_t s) {
        sp.reverse_from = check ? m / 2 : 0;
        launch_sgm(d, m, cols, rows, sp, s);
    });
    auto checks = group_tile_table<LrImage>(c, "SVO_DENSE_TABLE_IMAGES", [&](const LrImage* d, int m, hipStream_t s) {
        launch_lr_check_lattice(d, m, lr_tiles((int64_t)cols * rows), *check, s);
    });
    const size_t part = c->args.bytes / (check ? 3 : 2) / 256 * 256;
    const size_t cap = std::min({costs.cap, part / sizeof(CostImage) / per, part / sizeof(SgmImage) / per, DENSE_MAX_IMAGES / per, chunk,
                                 check ? part / sizeof(LrImage) : chunk});
    sums.h = reinterpret_cast<SgmImage*>(reinterpret_cast<uint8_t*>(sums.h) + part);
    sums.d = reinterpret_cast<SgmImage*>(reinterpret_cast<uint8_t*>(sums.d) + part);
    checks.h = reinterpret_cast<LrImage*>(reinterpret_cast<uint8_t*>(checks.h) + 2 * part);
    checks.d = reinterpret_cast<LrImage*>(reinterpret_cast<uint8_t*>(checks.d) + 2 * part);
    if (cap < 1) return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_disparity_sgm: the argument blocks hold no image table");
    dense_plan(dp, (long long)dense_tiles(params, c->width, c->height) * (long long)std::min(images.size(), cap));
    grid = dense_tiles(dp, c->width, c->height);
    for (size_t i0 = 0; i0 < images.size(); i0 += cap) {
        const size_t m = std::min(cap, images.size() - i0);
        for (size_t k = 0; k < m; k++) {
            const DenseImage& im = images[i0 + k];
            uint8_t* const at = c->d_sgm.p + k * slot;     // sums | volume | count plane [| the same of the mirrored pair | its disparity plane]
            uint16_t* const vol = reinterpret_cast<uint16_t*>(at + volume);
            uint16_t* const count = reinterpret_cast<uint16_t*>(at + 2 * volume);
            costs.h[k] = CostImage{im.left, im.right, vol, count, im.left_stride, im.right_stride, im.w, im.h};
            sums.h[k] = SgmImage{vol, count, reinterpret_cast<uint16_t*>(at), im.out, cols, rows, D, im.baseline};
            if (!check) continue;
            uint16_t* const rvol = reinterpret_cast<uint16_t*>(at + one + volume);
            uint16_t* const rcount = reinterpret_cast<uint16_t*>(at + one + 2 * volume);
            float* const rev = reinterpret_cast<float*>(at + 2 * one);
            costs.h[m + k] = CostImage{im.left, im.right, rvol, rcount, im.left_stride, im.right_stride, im.w, im.h};
            sums.h[m + k] = SgmImage{rvol, rcount, reinterpret_cast<uint16_t*>(at + one), rev, cols, rows, D, im.baseline};
            checks.h[k] = LrImage{im.left, im.right, rev, im.out, lr_plane < 0 ? nullptr : im.out + lr_plane, im.left_stride, im.right_stride, im.w, im.h, im.baseline, 0};
        }
        const bool more = args_reused || i0 + m < images.size();   // (a chunk is full: its launches go first)
        costs.m = sums.m = per * m;
        if (const int rc = costs.launch(more)) return rc;
        if (const int rc = sums.launch(more)) return rc;
        if (check) {
            checks.m = m;
            if (const int rc = checks.launch(more)) return rc;
        }
    }
    return SVO_OK;
}

int grp_check_disparity_sgm(const svo_group* c, const svo_disparity_style* style, const svo_sgm_params* sgm, const char* who) {
    DenseParams p;
    if (const int rc = check_style(&c->cam, c->width, c->height, style, who, &p)) return rc;
    if (p.search_x + 1 > SGM_MAX_D) return svo_set_error(SVO_ERR_INVALID, "%s: search_x %d: at most %d with a cost volume", who, p.search_x, SGM_MAX_D - 1);
    return sgm_check_params(sgm, who, nullptr);
}

extern "C" int svo_disparity_size_checked(const svo_camera_settings* cam, int width, int height, const svo_disparity_style* style,
                                          const svo_stereo_check* check, int* cols, int* rows, int* planes, int64_t* image_bytes) {
    const char* who = check ? "svo_disparity_size_checked" : "svo_disparity_size";
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    DenseParams p;
    if (const int rc = check_style(cam, width, height, style, who, &p)) return rc;
    LrCheck lr;
    if (const int rc = lr_check_parse(check, false, who, &lr)) return rc;
    dense_shape(p, width, height, cols, rows, planes, image_bytes, lr.on);
    return SVO_OK;
}

extern "C" int svo_disparity_size(const svo_camera_settings* cam, int width, int height, const svo_disparity_style* style,
                                  int* cols, int* rows, int* planes, int64_t* image_bytes) {
    return svo_disparity_size_checked(cam, width, height, style, nullptr, cols, rows, planes, image_bytes);
}

int grp_check_disparity_style(const svo_group* c, const svo_disparity_style* style, const svo_stereo_check* check) {
    const char* who = check ? "svo_submit_export_disparity_checked" : "svo_submit_export_disparity";
    if (const int rc = check_style(&c->cam, c->width, c->height, style, who, nullptr)) return rc;
    return lr_check_parse(check, false, who, nullptr);
}

int64_t grp_disparity_bytes(const svo_group* c, const svo_disparity_style* style, const svo_stereo_check* check) {
    DenseParams p;
    int64_t bytes = 0;
    if (dense_check_style(style, &c->cam, "svo_submit_export_disparity", &p) == SVO_OK)
        dense_shape(p, c->width, c->height, nullptr, nullptr, nullptr, &bytes, check && check->lr == 1);
    return bytes;
}

// The named slots of the group as segments and planes (svo_submit_export_disparity). Named slot seg[i] of the job goes
// to byte seg[i] * image_bytes of the caller's values; in host mode the group computes its i-th named slot at byte
// i * image_bytes of its staging block and copies every run of slots that are consecutive in both (and delivered) out
// with one copy: a plain one where the planes fill their image_bytes, else a 2-D one of the planes' bytes per slot, so
// that the bytes between two slots stay untouched. The image table (one entry per delivered slot) goes through the
// group's argument blocks, one launch unless it outgrows them.
// A checked job (include/svo_hip.h, "cross-check") searches disparities whatever the style's value, and then, per
// chunk of delivered slots whose reverse planes fit the group's d_lr block, runs the reverse search and the check,
// which appends the lr plane and masks and converts the value plane in place. The stream orders a chunk's check before
// the next chunk's reverse search, so the chunks share the block without a wait of the host.
// An SGM job (sgm != null) leaves the image table empty and delivers through grp_sgm_planes, its check included (another
// rule, "sgm cross-check": no reverse search of this function and no d_lr block).
int grp_export_disparity(svo_group* c, int what, int mem, const int* seqs, const int* seg, int n, int seq0,
                         const svo_disparity_style* style, const svo_stereo_check* check, const svo_sgm_params* sgm,
                         const svo_disparity_dst* dst) {
    if (const int rc = job_begin(c, "svo_submit_export_disparity")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    DenseParams params;
    if (const int rc = dense_check_style(style, &c->cam, "svo_submit_export_disparity", &params)) return rc;
    LrCheck lr;
    if (const int rc = lr_check_parse(check, false, "svo_submit_export_disparity", &lr)) return rc;
    const LrParams lr_params{params.value, params.step, lr.max_lr_diff};
    if (lr.on) params.value = SVO_DENSE_DISPARITY;
    SgmParams sgm_params{};
    if (sgm) {
        if (const int rc = sgm_check_params(sgm, "svo_submit_export_disparity_sgm", &sgm_params)) return rc;
        sgm_params.value = params.value;
        sgm_params.cost = params.cost;
    }
    std::vector<DenseImage> sgm_images;                    // (an SGM job: the delivered slots, for grp_sgm_planes)
    int cols, rows, planes; int64_t image_bytes;
    dense_shape(params, c->width, c->height, &cols, &rows, &planes, &image_bytes, lr.on);
    const int64_t used = (int64_t)planes * cols * rows * 4;   // bytes of a slot's planes
    int tiles = dense_tiles(params, c->width, c->height);
    if (host)
        if (const int rc = c->d_dense.reserve(c, (size_t)n * (size_t)image_bytes)) return rc;
    // (SVO_DENSE_TABLE_IMAGES: a smaller table, so that tests reach the chunked launches)
    auto table = group_tile_table<DenseImage>(c, "SVO_DENSE_TABLE_IMAGES",
                                              [&](const DenseImage* d, int m, hipStream_t s) { launch_dense(d, m, tiles, params, s); });
    table.cap = std::min(table.cap, DENSE_MAX_IMAGES);
    std::vector<char> shown((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_disparity_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.keyframe_id = -1;
        e.time_stamp = (float)q.ts; e.offset = (int64_t)seg[i] * image_bytes; e.status = SVO_DISPARITY_NONE;
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
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_disparity: the planes are %d x %d and %d x %d, not %d x %d", l.w, l.h, r.w, r.h,
                                 c->width, c->height);
        e.status = SVO_DISPARITY_OK;
        shown[i] = 1;
        uint8_t* out = host ? c->d_dense.p + (int64_t)i * image_bytes : reinterpret_cast<uint8_t*>(dst->values) + e.offset;
        const DenseImage image{l.data, r.data, reinterpret_cast<float*>(out), l.stride, r.stride, l.w, l.h, q.cam.baseline, 0};
        if (sgm) {
            sgm_images.push_back(image);
            continue;
        }
        if (const int rc = table.add(image)) return rc;
    }
    if (sgm)
        if (const int rc = grp_sgm_planes(c, sgm_images, params, sgm_params, cols, rows, lr.on ? &lr_params : nullptr, (int64_t)(planes - 1) * cols * rows, false))
            return rc;
    if (table.m == (size_t)std::count(shown.begin(), shown.end(), 1)) {   // (one launch: sized by what it holds)
        dense_plan(params, (long long)tiles * (long long)table.m);
        tiles = dense_tiles(params, c->width, c->height);
    }
    if (const int rc = table.launch(lr.on)) return rc;    // (checked: the argument blocks are filled again)
    if (lr.on && !sgm) {
        const size_t reverse = lr_reverse_bytes(c->width, c->height, params.step);
        // (SVO_LR_CHUNK_SLOTS: fewer slots per chunk, so that tests reach the chunked path)
        const size_t chunk = std::min<size_t>((size_t)n, table_tiles("SVO_LR_CHUNK_SLOTS", std::max<size_t>(1, LR_STAGING_BYTES / reverse)));
        if (const int rc = c->d_lr.reserve(c, chunk * reverse)) return rc;
        const DenseParams rp = params;
        const int lr_grid = lr_tiles((int64_t)cols * rows);
        auto checks = group_tile_table<LrImage>(c, "SVO_DENSE_TABLE_IMAGES", [&](const LrImage* d, int m, hipStream_t s) {
            launch_dense_reverse(d, m, tiles, rp, s);
            launch_lr_check(d, m, lr_grid, lr_params, s);
        });
        checks.cap = std::min({checks.cap, DENSE_MAX_IMAGES, chunk});
        for (int i = 0; i < n; i++) {
            if (!shown[i]) continue;
            const Seq& q = c->seqs[seqs[i]];
            const ImageSet* set = what == SVO_EXPORT_FRAMES ? q.cur_set : q.kfs.back().set;
            const ImgView& l = set->left[0];
            const ImgView& r = set->right;
            float* out = reinterpret_cast<float*>(host ? c->d_dense.p + (int64_t)i * image_bytes
                                                       : reinterpret_cast<uint8_t*>(dst->values) + dst->segments[seg[i]].offset);
            if (checks.m == checks.cap)                    // (a chunk is full: its launches go first)
                if (const int rc = checks.launch(true)) return rc;
            float* rev = reinterpret_cast<float*>(c->d_lr.p + checks.m * reverse);
            if (const int rc = checks.add(LrImage{l.data, r.data, rev, out, out + (int64_t)(planes - 1) * cols * rows, l.stride, r.stride, l.w, l.h,
                                                  q.cam.baseline, 0}))
                return rc;
        }
        if (const int rc = checks.launch(false)) return rc;
    }
    if (host)
        if (const int rc = copy_out_slots(st, reinterpret_cast<uint8_t*>(dst->values), c->d_dense.p, seg, shown.data(), n, image_bytes, used)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}
