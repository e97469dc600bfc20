// svo_group_scene.hip — the scene job of a sequence group (svo_submit_export_scenes): the viewer's 3-D picture of the
// maps of its named slots (keyframe points, trajectory, frusta), rendered by scene.hip's kernel, as segments and
// pixels, with dense clouds drawn into them on request (svo_submit_export_scenes_clouds: the splat pass); and the
// host-only entry points svo_scene_size, svo_scene_look_at, svo_scene_frustum. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

void cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// v / |v|; false for a vector without a direction
bool normalize(double v[3]) {
    const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(l > 0) || !std::isfinite(l)) return false;
    for (int k = 0; k < 3; k++) v[k] /= l;
    return true;
}

}  // namespace

extern "C" int svo_scene_size(const svo_scene_style* style, int64_t* pitch, int64_t* image_bytes) {
    if (const int rc = scene_check_style(style, "svo_scene_size")) return rc;
    scene_shape(*style, style->cols, style->rows, pitch, image_bytes);
    return SVO_OK;
}

extern "C" int svo_scene_look_at(const float eye[3], const float centre[3], const float up[3], float fov_y_deg, int cols,
                                 int rows, float near, svo_scene_camera* camera) {
    if (!eye || !centre || !up || !camera || !finite3(eye) || !finite3(centre) || !finite3(up) || !(fov_y_deg > 0) ||
        !(fov_y_deg < 180) || cols < 1 || rows < 1 || !(near > 0) || !std::isfinite(near))
        return svo_set_error(SVO_ERR_INVALID, "svo_scene_look_at: bad arguments");
    double axis[3][3];                                     // x_c, y_c, z_c
    const double neg_up[3] = {-(double)up[0], -(double)up[1], -(double)up[2]};
    for (int k = 0; k < 3; k++) axis[2][k] = (double)centre[k] - (double)eye[k];
    if (!normalize(axis[2])) return svo_set_error(SVO_ERR_INVALID, "svo_scene_look_at: eye and centre coincide");
    cross(neg_up, axis[2], axis[0]);
    if (!normalize(axis[0])) return svo_set_error(SVO_ERR_INVALID, "svo_scene_look_at: up is parallel to the viewing direction");
    cross(axis[2], axis[0], axis[1]);
    svo_scene_camera cam;
    for (int k = 0; k < 3; k++) {
        for (int j = 0; j < 3; j++) cam.view[4 * k + j] = (float)(axis[k][j] + 0.0);   // (+ 0.0: no negative zero)
        cam.view[4 * k + 3] = (float)(-((axis[k][0] * eye[0] + axis[k][1] * eye[1]) + axis[k][2] * eye[2]) + 0.0);
    }
    const double half = (double)fov_y_deg * (3.14159265358979323846 / 180.0) * 0.5;
    cam.f = (float)((rows * 0.5) / std::tan(half));
    cam.cx = (float)(cols * 0.5);
    cam.cy = (float)(rows * 0.5);
    cam.near = near;
    if (const int rc = scene_check_camera(&cam, "svo_scene_look_at", 0)) return rc;
    *camera = cam;
    return SVO_OK;
}

extern "C" int svo_scene_frustum(const float pose[6], const float dims[3], float out[8][6]) {
    if (!pose || !dims || !out) return svo_set_error(SVO_ERR_INVALID, "svo_scene_frustum: bad arguments");
    double Rd[9];
    rodrigues_d(pose + 3, Rd);
    float R[9];
    for (int k = 0; k < 9; k++) R[k] = (float)Rd[k];
    const float w = dims[0], h = dims[1], d = dims[2];
    const float v[5][3] = {{0, 0, 0}, {-w, h, d}, {-w, -h, d}, {w, -h, d}, {w, h, d}};
    float world[5][3];
    for (int i = 0; i < 5; i++)
        for (int k = 0; k < 3; k++)
            world[i][k] = ((R[3 * k] * v[i][0] + R[3 * k + 1] * v[i][1]) + R[3 * k + 2] * v[i][2]) + pose[k];
    static const int edge[8][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 4}, {1, 2}, {2, 3}, {3, 4}, {4, 1}};
    for (int e = 0; e < 8; e++) {
        std::memcpy(out[e], world[edge[e][0]], sizeof(float) * 3);
        std::memcpy(out[e] + 3, world[edge[e][1]], sizeof(float) * 3);
    }
    return SVO_OK;
}

namespace svo {

void scene_frustum_lines(const float pose[6], const float dims[3], uint32_t cls_rgb, std::vector<svo_scene_line>& out) {
    float e[8][6];
    svo_scene_frustum(pose, dims, e);
    for (int i = 0; i < 8; i++) {
        svo_scene_line l;
        std::memcpy(l.a, e[i], sizeof(l.a));
        std::memcpy(l.b, e[i] + 3, sizeof(l.b));
        l.cls_rgb = cls_rgb; l._pad = 0;
        out.push_back(l);
    }
}

}  // namespace svo

int grp_check_scene_clouds(const svo_group* c, const svo_scene_clouds* clouds) {
    const char* who = "svo_submit_export_scenes_clouds";
    if (clouds->live != 0 && clouds->live != 1) return svo_set_error(SVO_ERR_INVALID, "%s: live %d is neither 0 nor 1", who, clouds->live);
    if (clouds->point_size < 1 || clouds->point_size > 16)
        return svo_set_error(SVO_ERR_INVALID, "%s: point_size %d is not within 1 .. 16", who, clouds->point_size);
    if (clouds->_reserved[0] != 0 || clouds->_reserved[1] != 0 || clouds->_reserved[2] != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: a _reserved is not 0", who);
    if (clouds->live == 0) return SVO_OK;
    if (clouds->what != SVO_EXPORT_FRAMES && clouds->what != SVO_EXPORT_LAST_KEYFRAMES)
        return svo_set_error(SVO_ERR_INVALID, "%s: what %d", who, clouds->what);
    if (const int rc = grp_check_cloud_style(c, &clouds->cloud, &clouds->check)) return rc;
    if (clouds->cloud.frame != SVO_CLOUD_WORLD || clouds->cloud.layout != 0)
        return svo_set_error(SVO_ERR_INVALID, "%s: cloud.frame %d must be SVO_CLOUD_WORLD and cloud.layout %d must be 0", who, clouds->cloud.frame,
                             clouds->cloud.layout);
    return SVO_OK;
}

int64_t grp_scene_bytes(const svo_scene_style* style) {
    int64_t bytes = 0;
    scene_shape(*style, style->cols, style->rows, nullptr, &bytes);
    return bytes;
}

// The named slots of the group as segments and images (svo_submit_export_scenes); cameras[i] belongs to seqs[i].
// Named slot seg[i] of the job goes to byte seg[i] * image_bytes of the caller's pixels; in host mode the group
// renders its i-th named slot at byte i * image_bytes of its staging block and copies every run of slots that are
// consecutive in both (and delivered) out as the views do. The lines of every slot (trajectory, keyframe frusta, the
// pose's frustum), the table of its keyframe sets and the image records are built in the pinned input block and go
// up in one copy; the tile table goes through the group's argument blocks (group_tile_table), one launch unless it
// outgrows them.
int grp_export_scenes(svo_group* c, int mem, const int* seqs, const int* seg, int n, int seq0, const svo_scene_style* style,
                      const svo_scene_camera* cameras, const svo_scene_dst* dst) {
    return grp_export_scenes_clouds(c, mem, seqs, seg, n, seq0, style, cameras, dst, nullptr, nullptr);
}

// With clouds ("scene clouds"; null: the job above, unchanged) the delivered slots run in chunks of at most `chunk`
// slots. Per chunk: the live layer of its slots is grp_export_cloud itself, in device mode and the organized layout,
// into the records part of the group's d_scene_cloud block (search, check, cloud write: its launches, its blocks);
// the chunk's key planes, the other part of that block, are cleared to all ones; the pieces of every slot's extra span
// and live records go through the splat pass; then the tile kernel that starts from the planes. The span table takes
// the first half of the group's argument blocks, the tile table the second. Every delivered slot has a plane: one that
// nobody offers to stays all ones, which is the picture without cloud points. With sgm the live layer is the SGM cloud
// job's (svo_submit_export_scenes_clouds_sgm): it fills the argument blocks itself and has left them when it returns,
// before this job's span and tile tables are built.
int grp_export_scenes_clouds(svo_group* c, int mem, const int* seqs, const int* seg, int n, int seq0, const svo_scene_style* style,
                             const svo_scene_camera* cameras, const svo_scene_dst* dst, const svo_scene_clouds* clouds,
                             const svo_scene_span* extra, const svo_sgm_params* sgm) {
    if (const int rc = job_begin(c, "svo_submit_export_scenes")) return rc;
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    const int cols = style->cols, rows = style->rows;
    int64_t pitch, image_bytes;
    scene_shape(*style, cols, rows, &pitch, &image_bytes);
    const int64_t used = (int64_t)rows * pitch;          // bytes of an image
    const float dims[3] = {style->frustum_w, style->frustum_h, style->frustum_d};
    std::vector<svo_scene_line> lines;
    std::vector<SceneSet> sets;
    std::vector<SceneImage> images;
    std::vector<SceneTile> tiles;
    std::vector<char> shown((size_t)n, 0);
    struct Placed { int i; size_t set0, line0; };        // a delivered slot: its first set and line of the job
    std::vector<Placed> placed;
    // (with clouds: the cloud segment of every slot whose live layer was drawn; the others have none)
    svo_cloud_segment no_cloud{};
    no_cloud.keyframe_id = -1; no_cloud.status = SVO_CLOUD_NONE;
    std::vector<svo_cloud_segment> cloud_of(clouds ? (size_t)n : 0, no_cloud);
    for (int i = 0; i < n; i++) {
        const Seq& q = c->seqs[seqs[i]];
        svo_scene_segment& e = clear(dst->segments[seg[i]]);
        e.seq = seq0 + seqs[i]; e.run = q.run; e.frame_id = q.frame_id; e.status = SVO_SCENE_NONE;
        e.n_keyframes = (uint16_t)q.kfs.size(); e.from_keyframe = style->from_keyframe;
        e.time_stamp = (float)q.ts; e.offset = (int64_t)seg[i] * image_bytes;
        std::memcpy(e.pose, q.pose, sizeof(e.pose));
        if (q.frame_id < 0) continue;
        e.status = SVO_SCENE_OK;
        shown[i] = 1;
        SceneImage im;
        im.cam = cameras[i];
        im.dst = nullptr; im.sets = nullptr; im.lines = nullptr;   // (placed below, once the blocks are there)
        im.w = cols; im.h = rows;
        const size_t set0 = sets.size(), line0 = lines.size();
        placed.push_back({i, set0, line0});
        // (the resident keyframes: a trimmed one has neither points nor a frustum)
        const size_t kf0 = std::min<size_t>(std::max<size_t>((size_t)style->from_keyframe, (size_t)q.kfs.first()), q.kfs.size());
        if (style->show & SVO_SCENE_POINTS)
            for (size_t k = kf0; k < q.kfs.size(); k++) {
                sets.push_back(scene_set(q.kfs[k].kps, q.kfs[k].n, (int)k));
                e.n_keypoints += q.kfs[k].n;
            }
        if (style->show & SVO_SCENE_TRAJECTORY) {
            const size_t np = q.trajectory.size();
            const size_t first = style->trajectory_tail > 0 && np > (size_t)style->trajectory_tail ? np - (size_t)style->trajectory_tail : 0;
            e.n_poses = (int)(np - first);
            for (size_t j = first; j + 1 < np; j++) {
                const svo_pose &a = q.trajectory[j], &b = q.trajectory[j + 1];
                lines.push_back(svo_scene_line{{a.x, a.y, a.z}, {b.x, b.y, b.z}, (uint32_t)SVO_SCENE_CLASS_TRAJECTORY << 24 | style->trajectory_rgb, 0});
            }
        }
        if (style->show & SVO_SCENE_KEYFRAMES)
            for (size_t k = kf0; k < q.kfs.size(); k++)
                scene_frustum_lines(q.kfs[k].pose, dims, (uint32_t)SVO_SCENE_CLASS_KEYFRAME << 24 | style->keyframe_rgb, lines);
        if (style->show & SVO_SCENE_POSE)
            scene_frustum_lines(q.pose, dims, (uint32_t)SVO_SCENE_CLASS_POSE << 24 | style->pose_rgb, lines);
        im.n_sets = (int)(sets.size() - set0); im.n_lines = (int)(lines.size() - line0);
        scene_tiles((int)images.size(), cols, rows, tiles);
        images.push_back(im);
    }
    if (!images.empty()) {
        if (host)
            if (const int rc = c->d_scene.reserve(c, (size_t)n * (size_t)image_bytes)) return rc;
        // the input block: lines | sets | images [| the images' key planes]
        const size_t lines_bytes = sizeof(svo_scene_line) * lines.size(), sets_bytes = sizeof(SceneSet) * sets.size();
        const size_t images_bytes = sizeof(SceneImage) * images.size();
        const size_t ptrs_bytes = clouds ? sizeof(unsigned long long*) * images.size() : 0;
        const size_t in_bytes = lines_bytes + sets_bytes + images_bytes + ptrs_bytes;
        if (const int rc = c->d_scene_in.reserve(c, align_up(in_bytes, 4096))) return rc;
        const svo_scene_line* d_lines = reinterpret_cast<const svo_scene_line*>(c->d_scene_in.p);
        const SceneSet* d_sets = reinterpret_cast<const SceneSet*>(c->d_scene_in.p + lines_bytes);
        const SceneImage* d_images = reinterpret_cast<const SceneImage*>(c->d_scene_in.p + lines_bytes + sets_bytes);
        unsigned long long** const d_ptrs = reinterpret_cast<unsigned long long**>(c->d_scene_in.p + lines_bytes + sets_bytes + images_bytes);
        for (size_t k = 0; k < placed.size(); k++) {
            const Placed& pl = placed[k];
            images[k].dst = host ? c->d_scene.p + (int64_t)pl.i * image_bytes : dst->pixels + (int64_t)seg[pl.i] * image_bytes;
            images[k].sets = d_sets + pl.set0;
            images[k].lines = d_lines + pl.line0;
        }
        // the chunks of a job with clouds: slot i of the job has plane and records i % m_max of the block
        const bool live = clouds && clouds->live == 1;
        if (!live) sgm = nullptr;
        const svo_stereo_check* check = live && clouds->check.lr ? &clouds->check : nullptr;
        const int64_t points = live ? grp_cloud_points(c, &clouds->cloud) : 0;
        const size_t key_bytes = scene_key_bytes(cols, rows), rec_bytes = sizeof(svo_map_point) * (size_t)points;
        size_t m_max = 0;
        uint8_t* d_records = nullptr;
        std::vector<unsigned long long*> ptrs;
        if (clouds) {
            // (SVO_SCENE_CHUNK_SLOTS: fewer slots per chunk, so that tests reach the chunked path)
            const char* lower = std::getenv("SVO_SCENE_CHUNK_SLOTS");
            m_max = scene_chunk_slots(key_bytes + (live ? grp_cloud_slot_bytes(c, &clouds->cloud, check, sgm) + rec_bytes : 0), (size_t)n,
                                      lower ? std::atoll(lower) : 0);
            if (const int rc = c->d_scene_cloud.reserve(c, m_max * (key_bytes + rec_bytes))) return rc;
            d_records = c->d_scene_cloud.p + m_max * key_bytes;
            for (const Placed& pl : placed)
                ptrs.push_back(reinterpret_cast<unsigned long long*>(c->d_scene_cloud.p + ((size_t)pl.i % m_max) * key_bytes));
        }
        uint8_t* h = c->d_scene_in.host.get();
        if (lines_bytes) std::memcpy(h, lines.data(), lines_bytes);
        if (sets_bytes) std::memcpy(h + lines_bytes, sets.data(), sets_bytes);
        std::memcpy(h + lines_bytes + sets_bytes, images.data(), images_bytes);
        if (ptrs_bytes) std::memcpy(h + lines_bytes + sets_bytes + images_bytes, ptrs.data(), ptrs_bytes);
        HIP_TRY(hipMemcpyAsync(c->d_scene_in.p, h, in_bytes, hipMemcpyHostToDevice, st));
        const SceneParams params = scene_params(*style);
        if (!clouds) {
            // (SVO_SCENE_TABLE_TILES: a smaller table, so that tests reach the chunked launches)
            auto table = group_tile_table<SceneTile>(c, "SVO_SCENE_TABLE_TILES", [&](const SceneTile* d, int m, hipStream_t s) {
                launch_scene(d, m, d_images, params, s);
            });
            for (const SceneTile& t : tiles)
                if (const int rc = table.add(t)) return rc;
            if (const int rc = table.launch(false)) return rc;
        } else {
            svo_cloud_style cloud_style = clouds->cloud;
            cloud_style.layout = SVO_CLOUD_ORGANIZED;
            std::vector<svo_cloud_segment> csegs(m_max);
            std::vector<int> local(m_max);
            for (size_t j = 0; j < m_max; j++) local[j] = (int)j;
            const size_t tiles_per_image = tiles.size() / images.size();
            const size_t half = c->args.bytes / 2 / 256 * 256;
            std::vector<std::pair<int, int>> chunks;
            scene_each_chunk(n, m_max, [&](int first, int count) { chunks.push_back({first, count}); });
            size_t k = 0;                                    // the next delivered slot: placed[k], image k
            for (const auto& [i0, m] : chunks) {
                if (k == placed.size()) break;
                if (placed[k].i >= i0 + m) continue;         // (no slot of this chunk is delivered)
                if (i0 > 0) HIP_TRY(hipStreamSynchronize(st));   // the block is free for this chunk
                if (live) {
                    const svo_cloud_dst cloud_dst{csegs.data(), reinterpret_cast<svo_map_point*>(d_records), (int64_t)m * points};
                    if (const int rc = grp_export_cloud(c, clouds->what, SVO_MEM_DEVICE, seqs + i0, local.data(), m, seq0, &cloud_style, check, &cloud_dst, sgm))
                        return rc;
                }
                HIP_TRY(hipMemsetAsync(c->d_scene_cloud.p, 0xff, (size_t)m * key_bytes, st));
                // (SVO_SCENE_TABLE_SPANS, SVO_SCENE_TABLE_TILES: smaller tables, so that tests reach the chunked launches)
                auto span_table = group_tile_table<SceneSpan>(c, "SVO_SCENE_TABLE_SPANS", [&](const SceneSpan* d, int count, hipStream_t s) {
                    launch_scene_splat(d, count, d_images, d_ptrs, params, clouds->point_size, s);
                });
                auto tile_table = group_tile_table<SceneTile>(c, "SVO_SCENE_TABLE_TILES", [&](const SceneTile* d, int count, hipStream_t s) {
                    launch_scene_clouds(d, count, d_images, d_ptrs, params, s);
                });
                span_table.cap = std::min(span_table.cap, half / sizeof(SceneSpan));
                tile_table.cap = std::min(tile_table.cap, half / sizeof(SceneTile));
                tile_table.h = reinterpret_cast<SceneTile*>(reinterpret_cast<uint8_t*>(tile_table.h) + half);
                tile_table.d = reinterpret_cast<SceneTile*>(reinterpret_cast<uint8_t*>(tile_table.d) + half);
                if (span_table.cap < 1 || tile_table.cap < 1)
                    return svo_set_error(SVO_ERR_CAPACITY, "svo_submit_export_scenes_clouds: the argument blocks hold no table");
                const size_t k0 = k;
                for (; k < placed.size() && placed[k].i < i0 + m; k++) {
                    const int i = placed[k].i, j = i - i0;
                    int rc = SVO_OK;
                    const auto piece = [&](const svo_map_point* from) {
                        return [&, from](int64_t first, int count) { if (!rc) rc = span_table.add(SceneSpan{from + first, (int)k, count}); };
                    };
                    if (extra) scene_each_piece(extra[i].n, piece(extra[i].points));
                    if (live && csegs[(size_t)j].status == SVO_CLOUD_OK) {
                        scene_each_piece(points, piece(reinterpret_cast<const svo_map_point*>(d_records) + (int64_t)j * points));
                        cloud_of[(size_t)i] = csegs[(size_t)j];
                    }
                    if (rc) return rc;
                }
                if (const int rc = span_table.launch(false)) return rc;
                for (size_t t = k0 * tiles_per_image; t < k * tiles_per_image; t++)
                    if (const int rc = tile_table.add(tiles[t])) return rc;
                if (const int rc = tile_table.launch(false)) return rc;
            }
        }
    }
    if (clouds && clouds->info)
        for (int i = 0; i < n; i++) {
            svo_scene_cloud_info& f = clear(clouds->info[seg[i]]);
            const svo_cloud_segment& e = cloud_of[(size_t)i];
            f.status = e.status; f.keyframe_id = e.keyframe_id; f.live_points = e.n_points;
            f.extra_points = extra ? extra[i].n : 0;
        }
    if (host)
        if (const int rc = copy_out_slots(st, dst->pixels, c->d_scene.p, seg, shown.data(), n, image_bytes, used)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}
