// Stage-level C API (include/svo_hip.h, "sgm"): svo_dense_cost_volume, svo_sgm_aggregate, svo_dense_disparity_sgm, and
// ("sgm cross-check") svo_dense_disparity_sgm_checked and svo_cloud_points_sgm.
// They share one chunked runner over the handle's sgm workspace: a chunk's tables, then per image its block of S
// and, for a whole map, its volume and count plane; with a check the same three of the mirrored pair and its
// disparity plane behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "svo_handle.hpp"

using namespace svo;

namespace {

constexpr size_t SGM_CHUNK_BYTES = (size_t)256 << 20;      // S of a chunk of svo_sgm_aggregate; twice it with volumes
constexpr size_t SGM_IMAGE_BYTES = (size_t)1 << 30;        // S of a single volume at most; twice it with volumes

// what one image of a call needs: its aggregation record (sum, and for `search` vol and count, are set per chunk),
// its search record, and the bytes of one volume and one count plane; for a checked map the aggregation record of
// the mirrored pair (its search record is cost: the mirrored launch swaps the planes), the check's record (out: the
// reverse plane, set per chunk; value and lr: set by the entry) and the bytes of the reverse plane
struct SgmWork {
    SgmImage agg;
    CostImage cost;
    size_t volume_bytes, count_bytes;
    int tiles;
    SgmImage ragg;
    LrImage lr;
    size_t reverse_bytes;
};

// the images of a call in chunks: [first, first + m) whose blocks stay within `budget` and `slots` images
// (SVO_SGM_CHUNK_SLOTS: fewer slots, so that tests reach the chunked path); one image always fits
std::vector<std::pair<size_t, size_t>> sgm_chunks(const std::vector<SgmWork>& work, bool search, bool checked, size_t budget) {
    size_t slots = DENSE_MAX_IMAGES;
    if (const char* e = std::getenv("SVO_SGM_CHUNK_SLOTS")) slots = std::max<long long>(1, std::min<long long>(std::atoll(e), (long long)slots));
    std::vector<std::pair<size_t, size_t>> chunks;
    size_t first = 0, bytes = 0;
    for (size_t i = 0; i < work.size(); i++) {
        size_t b = search ? 2 * work[i].volume_bytes + work[i].count_bytes : work[i].volume_bytes;
        if (checked) b = 2 * b + work[i].reverse_bytes;
        if (i > first && (bytes + b > budget || i - first >= slots)) {
            chunks.emplace_back(first, i - first);
            first = i;
            bytes = 0;
        }
        bytes += b;
    }
    if (first < work.size()) chunks.emplace_back(first, work.size() - first);
    return chunks;
}

// search (with `search`) and aggregation (with `aggregate`) of every image, chunk by chunk; complete on return.
// check (a whole map only; sgm.value is SVO_DENSE_DISPARITY then): the tables of a chunk of m images hold 2 m entries,
// the mirrored pairs behind the forward ones, so that the two launches of the paths carry both; the mirrored search
// and the lattice check are the two launches more.
int sgm_run(svo_handle* h, std::vector<SgmWork>& work, bool search, bool aggregate, DenseParams dense, int cost_cap, SgmParams sgm,
            const char* who, const LrParams* check = nullptr) {
    if (work.empty()) return SVO_OK;
    const bool staged = search && aggregate;               // the volumes live in the workspace
    const bool checked = staged && check;
    const size_t per = checked ? 2 : 1;                    // table entries per image
    const auto chunks = sgm_chunks(work, staged, checked, staged ? 2 * SGM_CHUNK_BYTES : SGM_CHUNK_BYTES);
    size_t images = 0, block = 0;
    for (const auto& c : chunks) {
        size_t b = 0;
        for (size_t i = c.first; i < c.first + c.second; i++)
            b += per * ((aggregate ? work[i].volume_bytes : 0) + (staged ? work[i].volume_bytes + work[i].count_bytes : 0)) +
                 (checked ? work[i].reverse_bytes : 0);
        images = std::max(images, c.second);
        block = std::max(block, b);
    }
    const size_t tables = ((sizeof(SgmImage) + sizeof(CostImage)) * per * images + (checked ? sizeof(LrImage) * images : 0) + 255) / 256 * 256;
    if (const int rc = h->sgm_ws.reserve(tables + block, h->stream)) return rc;
    SgmImage* const d_agg = reinterpret_cast<SgmImage*>(h->sgm_ws.ptr.get());
    CostImage* const d_cost = reinterpret_cast<CostImage*>(d_agg + per * images);
    LrImage* const d_lr = reinterpret_cast<LrImage*>(d_cost + per * images);
    std::vector<SgmImage> agg(per * images);
    std::vector<CostImage> cost(per * images);
    std::vector<LrImage> lrs(checked ? images : 0);
    int rc = SVO_OK;
    for (size_t ci = 0; ci < chunks.size() && rc == SVO_OK; ci++) {
        const size_t i0 = chunks[ci].first, m = chunks[ci].second;
        uint8_t* at = h->sgm_ws.ptr.get() + tables;
        int max_cols = 0, max_rows = 0, grid = 0, lr_grid = 0;
        long long workgroups = 0;
        for (size_t k = 0; k < m; k++) {
            SgmWork& w = work[i0 + k];
            if (aggregate) {
                w.agg.sum = reinterpret_cast<uint16_t*>(at);
                at += w.volume_bytes;
            }
            if (staged) {
                w.cost.vol = reinterpret_cast<uint16_t*>(at);
                at += w.volume_bytes;
                w.cost.count = reinterpret_cast<uint16_t*>(at);
                at += w.count_bytes;
                w.agg.vol = w.cost.vol;
                w.agg.count = w.cost.count;
            }
            agg[k] = w.agg;
            cost[k] = w.cost;
            if (checked) {                                 // sums | volume | count plane | disparity plane of the mirrored pair
                w.ragg.sum = reinterpret_cast<uint16_t*>(at);
                at += w.volume_bytes;
                cost[m + k] = w.cost;
                cost[m + k].vol = reinterpret_cast<uint16_t*>(at);
                at += w.volume_bytes;
                cost[m + k].count = reinterpret_cast<uint16_t*>(at);
                at += w.count_bytes;
                w.ragg.vol = cost[m + k].vol;
                w.ragg.count = cost[m + k].count;
                w.ragg.out = w.lr.out = reinterpret_cast<float*>(at);
                at += w.reverse_bytes;
                agg[m + k] = w.ragg;
                lrs[k] = w.lr;
                lr_grid = std::max(lr_grid, lr_tiles((int64_t)w.agg.cols * w.agg.rows));
            }
            max_cols = std::max(max_cols, w.agg.cols);
            max_rows = std::max(max_rows, w.agg.rows);
            workgroups += w.tiles;
        }
        if (search) {
            DenseParams p = dense;
            dense_plan(p, workgroups);
            for (size_t k = 0; k < m; k++) grid = std::max(grid, dense_tiles(p, cost[k].w, cost[k].h));
            if (hipMemcpyAsync(d_cost, cost.data(), sizeof(CostImage) * per * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
                rc = svo_set_error(SVO_ERR_HIP, "%s: an upload failed", who);
                break;
            }
            launch_dense_cost_volume(d_cost, (int)m, grid, p, cost_cap, h->stream);
            if (checked) launch_dense_cost_volume_mirrored(d_cost + m, (int)m, grid, p, cost_cap, h->stream);
        }
        if (aggregate) {
            if (hipMemcpyAsync(d_agg, agg.data(), sizeof(SgmImage) * per * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
                rc = svo_set_error(SVO_ERR_HIP, "%s: an upload failed", who);
                break;
            }
            sgm.reverse_from = checked ? (int)m : 0;
            launch_sgm(d_agg, (int)(per * m), max_cols, max_rows, sgm, h->stream);
        }
        if (checked) {
            if (hipMemcpyAsync(d_lr, lrs.data(), sizeof(LrImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
                rc = svo_set_error(SVO_ERR_HIP, "%s: an upload failed", who);
                break;
            }
            launch_lr_check_lattice(d_lr, (int)m, lr_grid, *check, h->stream);
        }
        if (hipGetLastError() != hipSuccess) rc = svo_set_error(SVO_ERR_HIP, "%s: a launch failed", who);
        // (the next chunk rewrites agg, cost and the blocks: the uploads and launches must be done with them)
        if (rc == SVO_OK && ci + 1 < chunks.size() && hipStreamSynchronize(h->stream) != hipSuccess)
            rc = svo_set_error(SVO_ERR_HIP, "%s: a launch failed", who);
    }
    const hipError_t e = hipStreamSynchronize(h->stream);    // (the uploads read host memory of this call)
    if (rc) return rc;
    HIP_TRY(e);
    return SVO_OK;
}

// the pairs of a search entry into work records (the lattice in agg, the planes in cost)
int sgm_pairs(int n, const svo_dense_src* src, const DenseParams& params, const char* who, std::vector<SgmWork>* work) {
    work->assign((size_t)n, SgmWork{});
    for (int i = 0; i < n; i++) {
        const svo_image& l = src[i].left;
        const svo_image& r = src[i].right;
        if (!l.data || !r.data || l.width < 1 || l.height < 1 || l.width > (1 << 15) || l.height > (1 << 15) || r.width != l.width ||
            r.height != l.height || l.stride < l.width || r.stride < r.width || src[i]._reserved != 0)
            return svo_set_error(SVO_ERR_INVALID, "%s: image %d: two device planes of one size, 1 .. 32768 pixels a side, stride >= width, _reserved 0", who, i);
        const int cols = l.width / params.step, rows = l.height / params.step, D = params.search_x + 1;
        if (cols < 1 || rows < 1)
            return svo_set_error(SVO_ERR_INVALID, "%s: image %d: %d x %d has no lattice point at step %d", who, i, l.width, l.height, params.step);
        SgmWork& w = (*work)[(size_t)i];
        w.agg = w.ragg = SgmImage{nullptr, nullptr, nullptr, nullptr, cols, rows, D, src[i].baseline};
        w.cost = CostImage{l.data, r.data, nullptr, nullptr, l.stride, r.stride, l.width, l.height};
        w.lr = LrImage{l.data, r.data, nullptr, nullptr, nullptr, l.stride, r.stride, l.width, l.height, src[i].baseline, 0};
        w.volume_bytes = sgm_volume_bytes(cols, rows, D);
        w.count_bytes = sgm_count_bytes(cols, rows);
        w.reverse_bytes = sgm_reverse_bytes(cols, rows);
        w.tiles = dense_tiles(params, l.width, l.height);
    }
    return SVO_OK;
}

int sgm_check_search(const svo_disparity_style* style, const char* who, DenseParams* params) {
    if (const int rc = dense_check_style(style, nullptr, who, params)) return rc;
    if (params->search_x + 1 > SGM_MAX_D) return svo_set_error(SVO_ERR_INVALID, "%s: search_x %d: at most %d with a cost volume", who, params->search_x, SGM_MAX_D - 1);
    return SVO_OK;
}

}  // namespace

extern "C" int svo_dense_cost_volume(svo_handle* h, int n, const svo_dense_src* src, const svo_disparity_style* style, int cost_cap,
                                     const int64_t* volume_offset, const int64_t* count_offset, uint16_t* volumes) {
    const char* const who = "svo_dense_cost_volume";
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !volume_offset || !count_offset))) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments", who);
    DenseParams params;
    if (const int rc = sgm_check_search(style, who, &params)) return rc;
    if (cost_cap < 1 || cost_cap > 65535) return svo_set_error(SVO_ERR_INVALID, "%s: cost_cap %d is not within 1 .. 65535", who, cost_cap);
    if (!volumes || ((uintptr_t)volumes & 1)) return svo_set_error(SVO_ERR_INVALID, "%s: volumes is NULL or not 2-byte aligned", who);
    std::vector<SgmWork> work;
    if (const int rc = sgm_pairs(n, src, params, who, &work)) return rc;
    for (int i = 0; i < n; i++) {
        if (volume_offset[i] < 0 || (volume_offset[i] & 1) || count_offset[i] < 0 || (count_offset[i] & 1))
            return svo_set_error(SVO_ERR_INVALID, "%s: image %d: the offsets must be >= 0 and multiples of 2", who, i);
        work[(size_t)i].cost.vol = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(volumes) + volume_offset[i]);
        work[(size_t)i].cost.count = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(volumes) + count_offset[i]);
    }
    return sgm_run(h, work, true, false, params, cost_cap, SgmParams{}, who);
}

extern "C" int svo_sgm_aggregate(svo_handle* h, int n, const svo_sgm_shape* shapes, const uint16_t* const* volumes,
                                 const uint16_t* const* counts, int value, int cost, const svo_sgm_params* sgm, const int64_t* offset,
                                 float* values) {
    const char* const who = "svo_sgm_aggregate";
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!shapes || !volumes || !offset))) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments", who);
    if (value != SVO_DENSE_DISPARITY && value != SVO_DENSE_DEPTH) return svo_set_error(SVO_ERR_INVALID, "%s: value %d", who, value);
    if (cost != 0 && cost != 1) return svo_set_error(SVO_ERR_INVALID, "%s: cost %d", who, cost);
    SgmParams params;
    if (const int rc = sgm_check_params(sgm, who, &params)) return rc;
    params.value = value;
    params.cost = cost;
    if (!values || ((uintptr_t)values & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: values is NULL or not 16-byte aligned", who);
    std::vector<SgmWork> work((size_t)n);
    for (int i = 0; i < n; i++) {
        const svo_sgm_shape& s = shapes[i];
        if (s.cols < 1 || s.rows < 1 || s.cols > (1 << 15) || s.rows > (1 << 15) || s.D < 1 || s.D > SGM_MAX_D)
            return svo_set_error(SVO_ERR_INVALID, "%s: volume %d: cols and rows 1 .. 32768, D 1 .. %d", who, i, SGM_MAX_D);
        if (!volumes[i] || ((uintptr_t)volumes[i] & 1) || (counts && ((uintptr_t)counts[i] & 1)))
            return svo_set_error(SVO_ERR_INVALID, "%s: volume %d: NULL, or it or its count plane is not 2-byte aligned", who, i);
        if (offset[i] < 0 || (offset[i] & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: volume %d: offset must be >= 0 and a multiple of 16", who, i);
        SgmWork& w = work[(size_t)i];
        w.volume_bytes = sgm_volume_bytes(s.cols, s.rows, s.D);
        if (w.volume_bytes > SGM_IMAGE_BYTES) return svo_set_error(SVO_ERR_CAPACITY, "%s: volume %d: %zu bytes of sums, at most %zu", who, i, w.volume_bytes, SGM_IMAGE_BYTES);
        w.agg = SgmImage{volumes[i], counts ? counts[i] : nullptr, nullptr, reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(values) + offset[i]),
                         s.cols, s.rows, s.D, s.baseline};
    }
    return sgm_run(h, work, false, true, DenseParams{}, 0, params, who);
}

extern "C" int svo_dense_disparity_sgm_checked(svo_handle* h, int n, const svo_dense_src* src, const int64_t* offset,
                                               const svo_disparity_style* style, const svo_sgm_params* sgm, const svo_stereo_check* check,
                                               float* values) {
    LrCheck lr;
    if (const int rc = lr_check_parse(check, false, "svo_dense_disparity_sgm_checked", &lr)) return rc;
    const char* const who = lr.on ? "svo_dense_disparity_sgm_checked" : "svo_dense_disparity_sgm";
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !offset))) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments", who);
    DenseParams params;
    if (const int rc = sgm_check_search(style, who, &params)) return rc;
    SgmParams sp;
    if (const int rc = sgm_check_params(sgm, who, &sp)) return rc;
    const LrParams lr_params{params.value, params.step, lr.max_lr_diff};
    sp.value = lr.on ? SVO_DENSE_DISPARITY : params.value;   // (checked: the check kernel converts the survivors)
    sp.cost = params.cost;
    if (!values || ((uintptr_t)values & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: values is NULL or not 16-byte aligned", who);
    std::vector<SgmWork> work;
    if (const int rc = sgm_pairs(n, src, params, who, &work)) return rc;
    for (int i = 0; i < n; i++) {
        if (offset[i] < 0 || (offset[i] & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: image %d: offset must be >= 0 and a multiple of 16", who, i);
        SgmWork& w = work[(size_t)i];
        if (w.volume_bytes > SGM_IMAGE_BYTES)
            return svo_set_error(SVO_ERR_CAPACITY, "%s: image %d: %zu bytes of volume, at most %zu", who, i, w.volume_bytes, SGM_IMAGE_BYTES);
        w.agg.out = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(values) + offset[i]);
        w.lr.value = w.agg.out;
        w.lr.lr = w.agg.out + (int64_t)(1 + params.cost) * w.agg.cols * w.agg.rows;
    }
    return sgm_run(h, work, true, true, params, sp.cost_cap, sp, who, lr.on ? &lr_params : nullptr);
}

extern "C" int svo_dense_disparity_sgm(svo_handle* h, int n, const svo_dense_src* src, const int64_t* offset,
                                       const svo_disparity_style* style, const svo_sgm_params* sgm, float* values) {
    return svo_dense_disparity_sgm_checked(h, n, src, offset, style, sgm, nullptr, values);
}

// The cloud of an SGM map: per chunk of the image table (SVO_CLOUD_TABLE_IMAGES bounds it, as in svo_cloud_points) the
// SGM disparity and cost planes of its pairs go into the cloud workspace (the runner above, with the check masking the
// disparity plane), then the count and write launches run over them.
extern "C" int svo_cloud_points_sgm(svo_handle* h, int n, const svo_cloud_src* src, const int64_t* first, const svo_cloud_style* style,
                                    const svo_sgm_params* sgm, const svo_stereo_check* check, svo_map_point* points, int32_t* counts) {
    const char* const who = "svo_cloud_points_sgm";
    CHECK_H(h);
    if (n < 0 || (n > 0 && (!src || !first))) return svo_set_error(SVO_ERR_INVALID, "%s: bad arguments", who);
    DenseParams search;
    CloudParams params;
    if (const int rc = cloud_check_style(style, nullptr, who, &search, &params)) return rc;
    if (search.search_x + 1 > SGM_MAX_D) return svo_set_error(SVO_ERR_INVALID, "%s: search_x %d: at most %d with a cost volume", who, search.search_x, SGM_MAX_D - 1);
    SgmParams sp;
    if (const int rc = sgm_check_params(sgm, who, &sp)) return rc;
    LrCheck lr;
    if (const int rc = lr_check_parse(check, true, who, &lr)) return rc;
    const LrParams lr_params{SVO_DENSE_DISPARITY, search.step, lr.max_lr_diff};
    sp.value = SVO_DENSE_DISPARITY;
    sp.cost = 1;
    params.sgm_cost = 1;
    if (!points || ((uintptr_t)points & 15)) return svo_set_error(SVO_ERR_INVALID, "%s: points is NULL or not 16-byte aligned", who);
    if ((uintptr_t)counts & 3) return svo_set_error(SVO_ERR_INVALID, "%s: counts is not 4-byte aligned", who);
    std::vector<svo_dense_src> pairs((size_t)n);
    for (int i = 0; i < n; i++) {
        pairs[(size_t)i] = svo_dense_src{src[i].left, src[i].right, src[i].baseline, src[i]._reserved};
        if (first[i] < 0) return svo_set_error(SVO_ERR_INVALID, "%s: image %d: first must be >= 0", who, i);
    }
    std::vector<SgmWork> all;
    if (const int rc = sgm_pairs(n, pairs.data(), search, who, &all)) return rc;
    for (const SgmWork& w : all)
        if (w.volume_bytes > SGM_IMAGE_BYTES)
            return svo_set_error(SVO_ERR_CAPACITY, "%s: %zu bytes of volume, at most %zu", who, w.volume_bytes, SGM_IMAGE_BYTES);
    if (n == 0) return SVO_OK;
    // per image of a chunk: its two planes, its tile counts and its pose matrices, each rounded up to 256 bytes
    auto planes_bytes = [](size_t pts) { return (pts * 8 + 255) / 256 * 256; };
    auto image_block = [&](size_t pts) { return planes_bytes(pts) + ((size_t)cloud_tiles((int64_t)pts) * 4 + 255) / 256 * 256 + 256; };
    const size_t chunk = table_tiles("SVO_CLOUD_TABLE_IMAGES", std::min<size_t>((size_t)n, DENSE_MAX_IMAGES));
    const size_t tables = (sizeof(CloudImage) * chunk + 255) / 256 * 256;
    size_t block = 0;
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        size_t b = 0;
        for (size_t i = i0; i < std::min(i0 + chunk, (size_t)n); i++) b += image_block((size_t)all[i].agg.cols * (size_t)all[i].agg.rows);
        block = std::max(block, b);
    }
    if (const int rc = h->cloud_ws.reserve(tables + block, h->stream)) return rc;
    CloudImage* const d_cloud = reinterpret_cast<CloudImage*>(h->cloud_ws.ptr.get());
    std::vector<CloudImage> cloud(chunk);
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - i0);
        std::vector<SgmWork> work(all.begin() + (ptrdiff_t)i0, all.begin() + (ptrdiff_t)(i0 + m));
        uint8_t* at = h->cloud_ws.ptr.get() + tables;
        int cloud_grid = 0;
        for (size_t j = 0; j < m; j++) {
            const svo_cloud_src& s = src[i0 + j];
            const size_t pts = (size_t)work[j].agg.cols * (size_t)work[j].agg.rows;
            float* planes = reinterpret_cast<float*>(at);
            int* tile_counts = reinterpret_cast<int*>(at + planes_bytes(pts));
            float* mats = reinterpret_cast<float*>(at + image_block(pts) - 256);
            at += image_block(pts);
            work[j].agg.out = work[j].lr.value = planes;
            CloudImage& c = cloud[j];
            c = CloudImage{s.left.data, planes, planes + pts, points + first[i0 + j], tile_counts, counts ? counts + (i0 + j) : nullptr,
                           s.left.stride, s.left.width, s.left.height, s.baseline, s.fx, s.fy, s.cx, s.cy, {}, mats};
            std::memcpy(c.pose, s.pose, sizeof(c.pose));
            cloud_grid = std::max(cloud_grid, cloud_tiles((int64_t)pts));
        }
        // (complete on return, so the cloud table may be a local of this loop)
        if (const int rc = sgm_run(h, work, true, true, search, sp.cost_cap, sp, who, lr.on ? &lr_params : nullptr)) return rc;
        if (hipMemcpyAsync(d_cloud, cloud.data(), sizeof(CloudImage) * m, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            return svo_set_error(SVO_ERR_HIP, "%s: an upload failed", who);
        }
        launch_cloud(d_cloud, (int)m, cloud_grid, params, h->stream);
        if (const int rc = finish_launch(h)) return rc;
    }
    return SVO_OK;
}
