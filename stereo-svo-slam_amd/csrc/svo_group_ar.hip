// svo_group_ar.hip — the ar job of a sequence group (svo_submit_export_ar): the AR demo's picture of its named slots
// (the job's mesh instances, lit and depth tested, over the left level-0 plane of each slot's current frame, seen
// from the slot's pose through its rig's intrinsics), rendered by ar.hip's two kernels, as segments and pixels; the
// occluded job (svo_submit_export_ar_occluded: the organized camera-frame clouds of the named slots, computed by
// grp_export_cloud in device mode into a block of the group, hide the meshes behind them); and the host-only entry
// points svo_ar_size and svo_ar_camera_of_pose. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

constexpr size_t AR_STAGING_BYTES = (size_t)256 << 20;   // the slots of one chunk of an occluded job stage at most so much (one slot always fits)

size_t pad16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace

extern "C" int svo_ar_size(const svo_camera_settings* cam, int width, int height, const svo_ar_style* style, int64_t* pitch,
                           int64_t* image_bytes) {
    if (const int rc = check_settings(cam, width, height, 1)) return rc;
    if (const int rc = ar_check_style(style, "svo_ar_size")) return rc;
    ar_shape(*style, width, height, pitch, image_bytes);
    return SVO_OK;
}

extern "C" int svo_ar_camera_of_pose(const float pose[6], const svo_camera_settings* cam, svo_ar_camera* camera) {
    if (!pose || !cam || !camera) return svo_set_error(SVO_ERR_INVALID, "svo_ar_camera_of_pose: bad arguments");
    double Rd[9];
    rodrigues_d(pose + 3, Rd);
    float R[9];
    for (int k = 0; k < 9; k++) R[k] = (float)Rd[k];
    for (int k = 0; k < 3; k++) {
        for (int j = 0; j < 3; j++) camera->view[4 * k + j] = R[3 * j + k];
        camera->view[4 * k + 3] = -(((R[k] * pose[0]) + (R[3 + k] * pose[1])) + (R[6 + k] * pose[2]));
    }
    camera->fx = cam->fx; camera->fy = cam->fy; camera->cx = cam->cx; camera->cy = cam->cy;
    return SVO_OK;
}

int64_t grp_ar_bytes(const svo_group* c, const svo_ar_style* style) {
    int64_t bytes = 0;
    ar_shape(*style, c->width, c->height, nullptr, &bytes);
    return bytes;
}

// The named slots of the group as segments and images (svo_submit_export_ar); slot seqs[i] shows the job's instances
// [inst0[i], inst1[i]). Named slot seg[i] of the job goes to byte seg[i] * image_bytes of the caller's pixels; in host
// mode the group renders its i-th named slot at byte i * image_bytes of its staging block and copies every run of
// slots that are consecutive in both (and delivered) out as the views do. The input block holds the job's meshes
// once (vertices | triangles | colours), then a draw per (slot, instance), the image records and the work list of
// the first launch; it goes up in one copy. The tile table goes through the group's argument blocks
// (group_tile_table), one launch unless it outgrows them.
int grp_export_ar(svo_group* c, int mem, const int* seqs, const int* seg, const int* inst0, const int* inst1, int n, int seq0,
                  const ArJob* job, const svo_ar_dst* dst) {
    return grp_export_ar_occluded(c, mem, seqs, seg, inst0, inst1, n, seq0, job, dst, nullptr);
}

int grp_check_ar_occlusion(const svo_group* c, const svo_ar_occlusion* occlusion) {
    const char* who = "svo_submit_export_ar_occluded";
    if (const int rc = ar_check_occlusion(occlusion, who)) return rc;
    if (!occlusion || occlusion->on == 0) return SVO_OK;
    if (const int rc = grp_check_cloud_style(c, &occlusion->cloud, &occlusion->check)) return rc;
    if (occlusion->cloud.frame != SVO_CLOUD_CAMERA || occlusion->cloud.layout != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: cloud.frame %d must be SVO_CLOUD_CAMERA and cloud.layout %d must be 0", who, occlusion->cloud.frame,
                             occlusion->cloud.layout);
    return SVO_OK;
}

// With an occlusion ("ar occlusion"; null: the job above, unchanged) the input block ends with one ArOccluder and one
// pair of counters (zero) per delivered slot, and the slots run in chunks of at most `chunk`. Per chunk: the occluder
// of its slots is grp_export_cloud itself, in device mode, the camera frame and the organized layout, into the group's
// d_ar_occ block (search, check, cloud write: its launches, its blocks); then the first launch over the chunk's
// triangles and the tile kernel over its tiles. Slot i of the job has records i % chunk of the block. The counters of
// every slot come back in one copy after the last chunk. With sgm the occluder is the SGM cloud job's
// (svo_submit_export_ar_occluded_sgm): it fills the argument blocks itself and has left them when it returns, before
// this job's tile table is built.
int grp_export_ar_occluded(svo_group* c, int mem, const int* seqs, const int* seg, const int* inst0, const int* inst1, int n, int seq0,
                           const ArJob* job, const svo_ar_dst* dst, const svo_ar_occlusion* occl, const svo_sgm_params* sgm) {
    if (const int rc = job_begin(c, "svo_submit_export_ar")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    const int cols = c->width, rows = c->height;
    int64_t pitch, image_bytes;
    ar_shape(job->style, cols, rows, &pitch, &image_bytes);
    const int64_t used = (int64_t)rows * pitch;          // bytes of an image
    std::vector<svo_ar_draw> draws;
    std::vector<int> draw_mesh;                          // the job's mesh of each draw
    std::vector<ArImage> images;
    std::vector<ArSetup> setup;
    std::vector<ArTile> tiles;
    std::vector<char> shown((size_t)n, 0);
    struct Placed { int i; size_t draw0, rec0, setup0, tile0; };   // a delivered slot: its first draw, record, work item and tile of the job
    std::vector<Placed> placed;
    std::vector<int> kept;                               // (occluded) the kept count of each named slot's cloud
    const unsigned long long* counters = nullptr;        // (occluded) {covered, hidden} of each delivered slot, once the job is delivered
    size_t records = 0;
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_ar_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.status = SVO_AR_NONE;
        e.n_instances = inst1[i] - inst0[i];
        e.time_stamp = (float)q.ts; e.offset = (int64_t)seg[i] * image_bytes;
        std::memcpy(e.pose, q.pose, sizeof(e.pose));
        if (q.frame_id < 0 || !q.cur_set) continue;
        const ImgView& src = q.cur_set->left[0];
        if (src.w != cols || src.h != rows)
            return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_ar: level 0 is %d x %d, not %d x %d", src.w, src.h, cols, rows);
        e.status = SVO_AR_OK;
        shown[i] = 1;
        placed.push_back({i, draws.size(), records, setup.size(), tiles.size()});
        for (int k = inst0[i]; k < inst1[i]; k++) {
            const svo_ar_instance& in = job->instances[(size_t)k];
            const ArJob::Mesh& m = job->meshes[(size_t)in.mesh];
            svo_ar_draw d;
            std::memcpy(d.model, in.model, sizeof(d.model));
            d.vertices = nullptr; d.triangles = nullptr; d.rgb = nullptr;   // (placed below, once the block is there)
            d.n_vertices = m.n_vertices; d.n_triangles = m.n_triangles;
            d.rgb_all = in.rgb; d._reserved = 0;
            draws.push_back(d);
            draw_mesh.push_back(in.mesh);
        }
        ArImage im;
        svo_ar_camera_of_pose(q.pose, &q.cam, &im.cam);
        im.src = src.data; im.dst = nullptr; im.draws = nullptr; im.records = nullptr;   // (placed below, once the blocks are there)
        im.src_stride = src.stride; im.w = cols; im.h = rows;
        const size_t d0 = placed.back().draw0;
        im.n_records = ar_work((int)images.size(), cols, rows, draws.data() + d0, (int)(draws.size() - d0), setup, tiles);
        e.n_triangles = im.n_records;
        records += (size_t)im.n_records;
        images.push_back(im);
    }
    if (!images.empty()) {
        if (host)
            if (const int rc = c->d_ar.reserve(c, (size_t)n * (size_t)image_bytes)) return rc;
        if (const int rc = c->d_ar_rec.reserve(c, sizeof(ArRecord) * records)) return rc;
        // the input block: vertices | triangles | colours | draws | images | work list
        const size_t v_bytes = pad16(sizeof(float) * job->vertices.size()), t_bytes = pad16(sizeof(int32_t) * job->triangles.size());
        const size_t c_bytes = pad16(sizeof(uint32_t) * job->rgb.size()), d_bytes = pad16(sizeof(svo_ar_draw) * draws.size());
        const size_t i_bytes = pad16(sizeof(ArImage) * images.size()), s_bytes = sizeof(ArSetup) * setup.size();
        const size_t o_bytes = occl ? sizeof(ArOccluder) * images.size() : 0, k_bytes = occl ? 16 * images.size() : 0;   // occluders | counters
        const size_t o_at = v_bytes + t_bytes + c_bytes + d_bytes + i_bytes + s_bytes, k_at = o_at + o_bytes;
        const size_t in_bytes = k_at + k_bytes;
        if (const int rc = c->d_ar_in.reserve(c, align_up(in_bytes, 4096))) return rc;
        uint8_t* dev = c->d_ar_in.p;
        const float* d_vertices = reinterpret_cast<const float*>(dev);
        const int32_t* d_triangles = reinterpret_cast<const int32_t*>(dev + v_bytes);
        const uint32_t* d_rgb = reinterpret_cast<const uint32_t*>(dev + v_bytes + t_bytes);
        const svo_ar_draw* d_draws = reinterpret_cast<const svo_ar_draw*>(dev + v_bytes + t_bytes + c_bytes);
        const ArImage* d_images = reinterpret_cast<const ArImage*>(dev + v_bytes + t_bytes + c_bytes + d_bytes);
        const ArSetup* d_setup = reinterpret_cast<const ArSetup*>(dev + v_bytes + t_bytes + c_bytes + d_bytes + i_bytes);
        for (size_t k = 0; k < draws.size(); k++) {
            const ArJob::Mesh& m = job->meshes[(size_t)draw_mesh[k]];
            draws[k].vertices = d_vertices + m.v0 * 3;
            draws[k].triangles = d_triangles + m.t0 * 3;
            if (m.has_rgb) draws[k].rgb = d_rgb + m.c0;
        }
        for (size_t k = 0; k < placed.size(); k++) {
            const Placed& pl = placed[k];
            images[k].dst = host ? c->d_ar.p + (int64_t)pl.i * image_bytes : dst->pixels + (int64_t)seg[pl.i] * image_bytes;
            images[k].draws = d_draws + pl.draw0;
            images[k].records = reinterpret_cast<ArRecord*>(c->d_ar_rec.p) + pl.rec0;
        }
        // the chunks of an occluded job
        svo_cloud_style cloud_style{};
        const svo_stereo_check* check = nullptr;
        int64_t points = 0;
        size_t m_max = 0;
        std::vector<ArOccluder> occluders;
        if (occl) {
            cloud_style = occl->cloud;
            cloud_style.layout = SVO_CLOUD_ORGANIZED;
            check = occl->check.lr ? &occl->check : nullptr;
            points = grp_cloud_points(c, &cloud_style);
            const size_t rec_bytes = sizeof(svo_map_point) * (size_t)points;
            // (SVO_AR_CHUNK_SLOTS: fewer slots per chunk, so that tests reach the chunked path)
            const size_t per_slot = (size_t)grp_cloud_slot_bytes(c, &cloud_style, check, sgm) + rec_bytes;
            m_max = std::min<size_t>((size_t)n, table_tiles("SVO_AR_CHUNK_SLOTS", std::max<size_t>(1, AR_STAGING_BYTES / std::max<size_t>(per_slot, 1))));
            if (const int rc = c->d_ar_occ.reserve(c, m_max * rec_bytes)) return rc;
            for (size_t k = 0; k < placed.size(); k++)
                occluders.push_back(ArOccluder{reinterpret_cast<const svo_map_point*>(c->d_ar_occ.p) + (int64_t)((size_t)placed[k].i % m_max) * points,
                                               reinterpret_cast<unsigned long long*>(dev + k_at) + 2 * k, cols / cloud_style.step,
                                               rows / cloud_style.step, cloud_style.step, 0});
        }
        uint8_t* h = c->d_ar_in.host.get();
        auto put = [&](size_t at, const void* from, size_t b) { if (b) std::memcpy(h + at, from, b); };
        put(0, job->vertices.data(), sizeof(float) * job->vertices.size());
        put(v_bytes, job->triangles.data(), sizeof(int32_t) * job->triangles.size());
        put(v_bytes + t_bytes, job->rgb.data(), sizeof(uint32_t) * job->rgb.size());
        put(v_bytes + t_bytes + c_bytes, draws.data(), sizeof(svo_ar_draw) * draws.size());
        put(v_bytes + t_bytes + c_bytes + d_bytes, images.data(), sizeof(ArImage) * images.size());
        put(v_bytes + t_bytes + c_bytes + d_bytes + i_bytes, setup.data(), s_bytes);
        put(o_at, occluders.data(), o_bytes);
        if (k_bytes) std::memset(h + k_at, 0, k_bytes);
        HIP_TRY(hipMemcpyAsync(dev, h, in_bytes, hipMemcpyHostToDevice, st));
        const ArParams params = ar_params(job->style);
        if (!occl) {
            launch_ar_setup(d_setup, (int)setup.size(), d_images, params, st);
            HIP_TRY(hipGetLastError());
            // (SVO_AR_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
            auto table = group_tile_table<ArTile>(c, "SVO_AR_TABLE_TILES", [&](const ArTile* d, int m, hipStream_t s) {
                launch_ar(d, m, d_images, params, s);
            });
            for (const ArTile& t : tiles)
                if (const int rc = table.add(t)) return rc;
            if (const int rc = table.launch(false)) return rc;
        } else {
            const ArOccluder* d_occluders = reinterpret_cast<const ArOccluder*>(dev + o_at);
            const ArOcclusion occlusion = ar_occlusion(*occl);
            std::vector<svo_cloud_segment> csegs(m_max);
            std::vector<int> local(m_max);
            for (size_t j = 0; j < m_max; j++) local[j] = (int)j;
            kept.assign((size_t)n, 0);
            size_t k = 0;                                    // the next delivered slot: placed[k], image k
            bool ran = false;
            for (int i0 = 0; i0 < n && k < placed.size(); i0 += (int)m_max) {
                const int m = std::min((int)m_max, n - i0);
                const size_t k0 = k;
                while (k < placed.size() && placed[k].i < i0 + m) k++;
                if (k == k0) continue;                       // (no slot of this chunk is delivered)
                if (ran) HIP_TRY(hipStreamSynchronize(st));  // the records and the argument blocks are free for this chunk
                ran = true;
                const svo_cloud_dst cloud_dst{csegs.data(), reinterpret_cast<svo_map_point*>(c->d_ar_occ.p), (int64_t)m * points};
                if (const int rc = grp_export_cloud(c, SVO_EXPORT_FRAMES, SVO_MEM_DEVICE, seqs + i0, local.data(), m, seq0, &cloud_style, check, &cloud_dst, sgm))
                    return rc;
                for (size_t kk = k0; kk < k; kk++) {
                    const svo_cloud_segment& e = csegs[(size_t)(placed[kk].i - i0)];
                    if (e.status != SVO_CLOUD_OK)
                        return svo_set_error(SVO_ERR_INVALID, "svo_submit_export_ar_occluded: slot %d has a picture and no cloud", e.seq);
                    kept[(size_t)placed[kk].i] = e.n_points;
                }
                const size_t s0 = placed[k0].setup0, s1 = k < placed.size() ? placed[k].setup0 : setup.size();
                const size_t t0 = placed[k0].tile0, t1 = k < placed.size() ? placed[k].tile0 : tiles.size();
                launch_ar_setup(d_setup + s0, (int)(s1 - s0), d_images, params, st);
                HIP_TRY(hipGetLastError());
                auto table = group_tile_table<ArTile>(c, "SVO_AR_TABLE_TILES", [&](const ArTile* d, int count, hipStream_t s) {
                    launch_ar_occluded(d, count, d_images, d_occluders, params, occlusion, s);
                });
                for (size_t t = t0; t < t1; t++)
                    if (const int rc = table.add(tiles[t])) return rc;
                if (const int rc = table.launch(false)) return rc;
            }
            HIP_TRY(hipMemcpyAsync(h + k_at, dev + k_at, k_bytes, hipMemcpyDeviceToHost, st));
            counters = reinterpret_cast<const unsigned long long*>(h + k_at);
        }
    }
    if (host)
        if (const int rc = copy_out_slots(st, dst->pixels, c->d_ar.p, seg, shown.data(), n, image_bytes, used)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    if (occl && occl->info) {
        for (int i = 0; i < n; i++) clear(occl->info[seg[i]]).status = SVO_CLOUD_NONE;
        for (size_t k = 0; k < placed.size(); k++) {
            svo_ar_visibility& v = occl->info[seg[placed[k].i]];
            v.status = SVO_CLOUD_OK; v.occluder_points = kept[(size_t)placed[k].i];
            v.covered = (int64_t)counters[2 * k]; v.hidden = (int64_t)counters[2 * k + 1];
        }
    }
    return SVO_OK;
}
