// svo_group_snapshot.hip — snapshots of a sequence group (svo_submit_save / svo_submit_load): the format of
// include/svo_hip.h (layout, sizes, the complete check of a host part), the plan of a save, where the planes of a
// slot's state lie on the device, and save and load themselves, whose planes snapshot.hip's kernel copies; and
// svo_snapshot_info, which needs no GPU. The state is svo_group_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "svo_group_state.hpp"

using namespace svo;

namespace {

using SnapHeader = struct svo_snapshot_info;    // (the tag: svo_snapshot_info alone names the function)
constexpr int KP_PLANES = 12;
constexpr int KP_PLANE_ELEM[KP_PLANES] = {sizeof(svo_kp2d), sizeof(svo_kp3d), 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
constexpr int FIXED_PLANES = KP_PLANES + 2;     // the current keypoint set, the colour generator's word, the device count
constexpr size_t SNAP_FRAME_BYTES = sizeof(double) + sizeof(float) * 6 + sizeof(svo_frame_stats);
static_assert(sizeof(SnapHeader) == 160 && sizeof(PoseFilter) == 4128 && SNAP_FRAME_BYTES == 616 &&
              sizeof(svo_snapshot_keyframe) == 32 && sizeof(svo_snapshot_plane) == 16 && sizeof(svo_pose) == 24,
              "the snapshot format of include/svo_hip.h");

// the arrays of a keypoint set in directory order
void kps_planes(const KpsDev& k, uint8_t* out[KP_PLANES]) {
    void* p[KP_PLANES] = {k.kps2d, k.kps3d, k.flags, k.kf_id, k.kp_index, k.outl, k.inl, k.kfx, k.kfP, k.score, k.level_type, k.color};
    for (int i = 0; i < KP_PLANES; i++) out[i] = static_cast<uint8_t*>(p[i]);
}

struct PlaneDim { int row_bytes, rows; };

// the extent every plane of a snapshot has, in directory order (the header's counts are checked already)
std::vector<PlaneDim> snapshot_plane_dims(const SnapHeader& h, const svo_snapshot_keyframe* kfs) {
    std::vector<PlaneDim> v;
    v.reserve((size_t)h.n_planes);
    for (int i = 0; i < KP_PLANES; i++) v.push_back({KP_PLANE_ELEM[i] * h.n_keypoints, 1});
    v.push_back({4, 1});
    v.push_back({4, 1});
    for (int k = 0; k < h.n_keyframes - h.first_keyframe; k++)     // (kfs: the resident ones)
        for (int i = 0; i < KP_PLANES; i++) v.push_back({KP_PLANE_ELEM[i] * kfs[k].n, 1});
    for (int s = 0; s < h.n_image_sets; s++) {
        for (int l = 0; l < h.pyramid_levels; l++) v.push_back({h.width >> l, h.height >> l});
        v.push_back({h.width, h.height});
        for (int l = 1, w = h.width, ht = h.height; l < h.lk_levels; l++) {
            w = (w + 1) / 2; ht = (ht + 1) / 2;
            v.push_back({w, ht});
        }
    }
    return v;
}

int64_t snapshot_plane_count(const SnapHeader& h) {
    return FIXED_PLANES + (int64_t)KP_PLANES * (h.n_keyframes - h.first_keyframe) + (int64_t)h.n_image_sets * (h.pyramid_levels + h.lk_levels);
}

int64_t snapshot_host_bytes(const SnapHeader& h) {
    return (int64_t)(sizeof(SnapHeader) + sizeof(PoseFilter) + SNAP_FRAME_BYTES) + (int64_t)sizeof(svo_pose) * h.n_trajectory +
           (int64_t)sizeof(svo_snapshot_keyframe) * (h.n_keyframes - h.first_keyframe) + (int64_t)sizeof(svo_snapshot_plane) * h.n_planes;
}

// the sections of a checked host part (an aligned private copy)
struct SnapView {
    const SnapHeader* h;
    const PoseFilter* filter;
    const uint8_t* frame;
    const svo_pose* trajectory;
    const svo_snapshot_keyframe* kfs;      // the resident keyframes: kfs[k] is keyframe first_keyframe + k
    const svo_snapshot_plane* dir;
};

SnapView snapshot_view(const uint8_t* p) {
    SnapView v;
    v.h = reinterpret_cast<const SnapHeader*>(p);
    p += sizeof(SnapHeader);
    v.filter = reinterpret_cast<const PoseFilter*>(p);
    p += sizeof(PoseFilter);
    v.frame = p;
    p += SNAP_FRAME_BYTES;
    v.trajectory = reinterpret_cast<const svo_pose*>(p);
    p += sizeof(svo_pose) * (size_t)v.h->n_trajectory;
    v.kfs = reinterpret_cast<const svo_snapshot_keyframe*>(p);
    p += sizeof(svo_snapshot_keyframe) * (size_t)(v.h->n_keyframes - v.h->first_keyframe);
    v.dir = reinterpret_cast<const svo_snapshot_plane*>(p);
    return v;
}

#define SNAP_BAD(...) return svo_set_error(SVO_ERR_INVALID, "snapshot: " __VA_ARGS__)

// Checks a host part completely and copies it (header only for a header-only part) into `copy`, aligned.
int check_snapshot(const void* host_part, int64_t bytes, std::vector<uint8_t>& copy) {
    if (!host_part || bytes < (int64_t)sizeof(SnapHeader)) SNAP_BAD("the host part is shorter than its header");
    SnapHeader h;
    std::memcpy(&h, host_part, sizeof(h));
    if (h.magic != SVO_SNAPSHOT_MAGIC) SNAP_BAD("bad magic");
    if (h.version != SVO_SNAPSHOT_VERSION) SNAP_BAD("version %u, this library reads version %d", h.version, SVO_SNAPSHOT_VERSION);
    if (h.byte_order != SVO_SNAPSHOT_BYTE_ORDER) SNAP_BAD("not little endian");
    if (h.status != SVO_SNAPSHOT_COMPLETE && h.status != SVO_SNAPSHOT_TOO_SMALL) SNAP_BAD("bad status %u", h.status);
    if (h.width < 16 || h.height < 16 || check_settings(&h.cam, h.width, h.height, 1) != SVO_OK) SNAP_BAD("bad camera settings or size");
    if (h.capacity != keypoint_capacity(h.cam, h.width, h.height)) SNAP_BAD("capacity %d does not follow from the settings", h.capacity);
    if (h.pyramid_levels != h.cam.max_pyramid_levels || h.lk_levels != usable_lk_levels(h.cam, h.width, h.height))
        SNAP_BAD("level counts do not follow from the settings");
    if (h.frame_id < -1 || h.n_trajectory != h.frame_id + 1) SNAP_BAD("frame id %d with %d poses", h.frame_id, h.n_trajectory);
    if (h.n_keypoints < 0 || h.n_keypoints > h.capacity) SNAP_BAD("%d keypoints, capacity %d", h.n_keypoints, h.capacity);
    if (h.n_keyframes < 0) SNAP_BAD("%d keyframes", h.n_keyframes);
    if (h.keyframes_retired < 0 || h.keyframes_retired > std::max(h.n_keyframes - 1, 0)) SNAP_BAD("%d keyframes retired of %d", h.keyframes_retired, h.n_keyframes);
    if (h.first_keyframe < 0 || h.first_keyframe > h.keyframes_retired) SNAP_BAD("first keyframe %d, %d retired", h.first_keyframe, h.keyframes_retired);
    const int resident = h.n_keyframes - h.first_keyframe;
    if (resident > MAX_KEYFRAMES) SNAP_BAD("%d resident keyframes", resident);
    if (h.n_image_sets < 0 || h.n_image_sets > resident + 1) SNAP_BAD("%d image sets for %d keyframes", h.n_image_sets, resident);
    if (h.frame_id < 0 ? (h.n_keypoints || h.n_keyframes || h.n_image_sets) : (h.n_keyframes < 1 || h.n_image_sets < 1))
        SNAP_BAD("counts do not fit frame id %d", h.frame_id);
    if ((int64_t)h.n_planes != snapshot_plane_count(h)) SNAP_BAD("%d planes", h.n_planes);
    if (h.host_bytes != snapshot_host_bytes(h) || h.data_bytes < 0) SNAP_BAD("sizes do not fit the counts");
    if (h.status == SVO_SNAPSHOT_TOO_SMALL) {
        copy.assign(reinterpret_cast<const uint8_t*>(&h), reinterpret_cast<const uint8_t*>(&h) + sizeof(h));
        return SVO_OK;
    }
    if (bytes < h.host_bytes) SNAP_BAD("the host part has %lld bytes of %lld", (long long)bytes, (long long)h.host_bytes);
    copy.assign(static_cast<const uint8_t*>(host_part), static_cast<const uint8_t*>(host_part) + h.host_bytes);
    const SnapView v = snapshot_view(copy.data());
    std::vector<int> refs((size_t)h.n_image_sets, 0);
    for (int k = h.first_keyframe; k < h.n_keyframes; k++) {
        const svo_snapshot_keyframe& kf = v.kfs[k - h.first_keyframe];
        if (kf.n < 0 || kf.n > h.capacity) SNAP_BAD("keyframe %d: %d keypoints, capacity %d", k, kf.n, h.capacity);
        if (kf.image_set < -1 || kf.image_set >= h.n_image_sets || (k < h.keyframes_retired && kf.image_set != -1))
            SNAP_BAD("keyframe %d: image set %d", k, kf.image_set);
        if (kf.image_set >= 0) refs[kf.image_set]++;
    }
    for (int s = 1; s < h.n_image_sets; s++)
        if (!refs[s]) SNAP_BAD("image set %d belongs to no keyframe", s);
    const std::vector<PlaneDim> dims = snapshot_plane_dims(h, v.kfs);
    for (int i = 0; i < h.n_planes; i++) {
        const svo_snapshot_plane& p = v.dir[i];
        if (p.row_bytes != dims[i].row_bytes || p.rows != dims[i].rows)
            SNAP_BAD("plane %d: %d x %d bytes, must be %d x %d", i, p.rows, p.row_bytes, dims[i].rows, dims[i].row_bytes);
        if (p.offset < 0 || p.offset > h.data_bytes || (int64_t)p.row_bytes * p.rows > h.data_bytes - p.offset)
            SNAP_BAD("plane %d lies outside the data part", i);
    }
    return SVO_OK;
}

// what a save of the slot writes: header, keyframe records, directory, and the image sets in saved order
struct SavePlan {
    SnapHeader h;
    std::vector<svo_snapshot_keyframe> kfs;
    std::vector<svo_snapshot_plane> dir;
    std::vector<ImageSet*> sets;
};

void plan_snapshot(const svo_group* c, const Seq& q, SavePlan& p) {
    SnapHeader& h = clear(p.h);
    h.magic = SVO_SNAPSHOT_MAGIC; h.version = SVO_SNAPSHOT_VERSION; h.byte_order = SVO_SNAPSHOT_BYTE_ORDER;
    h.cam = q.cam; h.width = c->width; h.height = c->height; h.capacity = c->cap;
    h.pyramid_levels = c->cam.max_pyramid_levels; h.lk_levels = c->n_lk;
    h.frame_id = q.frame_id;
    if (q.frame_id >= 0) {
        h.n_keypoints = q.n_host; h.n_trajectory = (int)q.trajectory.size();
        h.n_keyframes = (int)q.kfs.size(); h.keyframes_retired = q.kfs_retired; h.first_keyframe = q.kfs.first();
        p.sets.push_back(q.cur_set);
        for (const KfHost& k : q.kfs) {
            svo_snapshot_keyframe r;
            std::memcpy(r.pose, k.pose, sizeof(r.pose));
            r.n = k.n; r.image_set = -1;
            if (k.set) {
                const auto it = std::find(p.sets.begin(), p.sets.end(), k.set);
                r.image_set = (int)(it - p.sets.begin());
                if (it == p.sets.end()) p.sets.push_back(k.set);
            }
            p.kfs.push_back(r);
        }
    }
    h.n_image_sets = (int)p.sets.size();
    h.n_planes = (int)snapshot_plane_count(h);
    int64_t off = 0;
    for (const PlaneDim& d : snapshot_plane_dims(h, p.kfs.data())) {
        p.dir.push_back({off, d.row_bytes, d.rows});
        off += (int64_t)align_up((size_t)d.row_bytes * d.rows, 16);
    }
    h.host_bytes = snapshot_host_bytes(h);
    h.data_bytes = off;
}

// where the planes of a slot's state lie on the device, in directory order: the address and the row pitch
struct DevPlane { uint8_t* p; int64_t pitch; };

std::vector<DevPlane> device_planes(const svo_group* c, const Seq& q, const std::vector<ImageSet*>& sets) {
    std::vector<DevPlane> v;
    uint8_t* a[KP_PLANES];
    kps_planes(q.kps[q.cur], a);
    for (uint8_t* p : a) v.push_back({p, 0});
    v.push_back({reinterpret_cast<uint8_t*>(q.color_lcg), 0});
    v.push_back({reinterpret_cast<uint8_t*>(q.d_n + q.cur), 0});
    for (const KfHost& k : q.kfs) {
        kps_planes(k.kps, a);
        for (uint8_t* p : a) v.push_back({p, 0});
    }
    auto image = [&v](const ImgView& im) { v.push_back({const_cast<uint8_t*>(im.data), im.stride}); };
    for (const ImageSet* s : sets) {
        for (int l = 0; l < c->cam.max_pyramid_levels; l++) image(s->left[l]);
        image(s->right);
        for (int l = 1; l < c->n_lk; l++) image(s->lk[l]);
    }
    return v;
}

// The tile table of a save or a load (group_tile_table: in the group's argument blocks, one launch unless it
// outgrows them; SVO_SNAPSHOT_TABLE_TILES: a smaller table, so that tests reach the chunked launches) and the
// tiles of one plane, cut through `cut`
struct PlaneTable {
    TileTable<CopyTile, decltype(&launch_copy_tiles)> tiles;
    std::vector<CopyTile> cut;
    explicit PlaneTable(svo_group* c) : tiles(group_tile_table<CopyTile>(c, "SVO_SNAPSHOT_TABLE_TILES", &launch_copy_tiles)) {}
    int add(const void* src, void* dst, int64_t row_bytes, int64_t rows, int64_t src_pitch, int64_t dst_pitch) {
        cut.clear();
        cut_copy_tiles(src, dst, row_bytes, rows, src_pitch, dst_pitch, cut);
        for (const CopyTile& t : cut)
            if (const int rc = tiles.add(t)) return rc;
        return SVO_OK;
    }
};

}  // namespace

int grp_snapshot_size(svo_group* c, int s, int64_t* host_bytes, int64_t* data_bytes) {
    flush_one(c->seqs[s]);
    SavePlan p;
    plan_snapshot(c, c->seqs[s], p);
    if (host_bytes) *host_bytes = p.h.host_bytes;
    if (data_bytes) *data_bytes = p.h.data_bytes;
    return SVO_OK;
}

int grp_check_snapshot(const svo_group* c, const svo_camera_settings* slot_cam, const svo_snapshot* snap,
                       std::vector<uint8_t>* host_copy) {
    if (const int rc = check_snapshot(snap->host, snap->host_capacity, *host_copy)) return rc;
    const SnapHeader& h = *reinterpret_cast<const SnapHeader*>(host_copy->data());
    if (h.status != SVO_SNAPSHOT_COMPLETE) SNAP_BAD("only the header was saved (a capacity was too small)");
    if (std::memcmp(&h.cam, slot_cam, sizeof(h.cam)) != 0 || h.width != c->width || h.height != c->height || h.capacity != c->cap)
        SNAP_BAD("camera settings, size or capacity differ from the target slot's");
    if (h.n_keyframes - h.first_keyframe > c->max_kf)
        SNAP_BAD("%d resident keyframes, the ctx's keyframe table holds %d", h.n_keyframes - h.first_keyframe, c->max_kf);
    if (snap->data_capacity < h.data_bytes || (h.data_bytes > 0 && !snap->data))
        SNAP_BAD("the data part has %lld bytes of %lld", (long long)snap->data_capacity, (long long)h.data_bytes);
    return SVO_OK;
}

// One group's share of svo_submit_save, between two steps of the group: slot seqs[i] into snaps[i].
int grp_save(svo_group* c, const int* seqs, int n, const svo_snapshot* snaps, int mem) {
    if (const int rc = reject_if_failed(c, "svo_submit_save")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    std::vector<SavePlan> plans((size_t)n);
    std::vector<size_t> stage_off((size_t)n, 0);
    size_t stage = 0;
    for (int i = 0; i < n; i++) {
        Seq& q = c->seqs[seqs[i]];
        flush_one(q);
        SavePlan& p = plans[i];
        plan_snapshot(c, q, p);
        const svo_snapshot& out = snaps[i];
        if (out.host_capacity < p.h.host_bytes || out.data_capacity < p.h.data_bytes) {
            p.h.status = SVO_SNAPSHOT_TOO_SMALL;
            std::memcpy(out.host, &p.h, sizeof(p.h));
            continue;
        }
        std::vector<uint8_t> part((size_t)p.h.host_bytes);
        uint8_t* w = part.data();
        auto put = [&w](const void* src, size_t bytes) { if (bytes) std::memcpy(w, src, bytes); w += bytes; };
        put(&p.h, sizeof(p.h));
        put(&q.kf, sizeof(PoseFilter));
        put(&q.ts, sizeof(double));
        put(q.pose, sizeof(q.pose));
        put(&q.stats, sizeof(q.stats));
        put(q.trajectory.data(), sizeof(svo_pose) * q.trajectory.size());
        put(p.kfs.data(), sizeof(svo_snapshot_keyframe) * p.kfs.size());
        put(p.dir.data(), sizeof(svo_snapshot_plane) * p.dir.size());
        std::memcpy(out.host, part.data(), part.size());
        stage_off[i] = stage;
        stage += align_up((size_t)p.h.data_bytes, 256);
    }
    if (host && stage > 0) {
        if (const int rc = c->d_snap.reserve(c, stage)) return rc;
        HIP_TRY(hipMemsetAsync(c->d_snap.p, 0, stage, st));     // (the bytes between planes: a host-mode snapshot is all defined)
    }
    PlaneTable table(c);
    for (int i = 0; i < n; i++) {
        const SavePlan& p = plans[i];
        if (p.h.status != SVO_SNAPSHOT_COMPLETE) continue;
        const Seq& q = c->seqs[seqs[i]];
        uint8_t* base = host ? c->d_snap.p + stage_off[i] : static_cast<uint8_t*>(snaps[i].data);
        const std::vector<DevPlane> dev = device_planes(c, q, p.sets);
        for (size_t j = 0; j < dev.size(); j++) {
            const svo_snapshot_plane& e = p.dir[j];
            if (const int rc = table.add(dev[j].p, base + e.offset, e.row_bytes, e.rows, dev[j].pitch, e.row_bytes)) return rc;
        }
    }
    if (const int rc = table.tiles.launch(false)) return rc;
    if (host)
        for (int i = 0; i < n; i++)
            if (plans[i].h.status == SVO_SNAPSHOT_COMPLETE && plans[i].h.data_bytes > 0)
                HIP_TRY(hipMemcpyAsync(snaps[i].data, c->d_snap.p + stage_off[i], (size_t)plans[i].h.data_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));       // delivered: svo_wait means that
    return SVO_OK;
}

// One group's share of svo_submit_load, between two steps of the group. The host parts are checked copies
// (grp_check_snapshot); the data parts are trusted.
int grp_load(svo_group* c, const SnapshotLoad* loads, int n, int mem) {
    if (const int rc = reject_if_failed(c, "svo_submit_load")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream.get();
    const bool host = mem == SVO_MEM_HOST;
    std::vector<size_t> stage_off((size_t)n, 0);
    size_t stage = 0;
    for (int i = 0; i < n; i++) {
        stage_off[i] = stage;
        stage += align_up((size_t)reinterpret_cast<const SnapHeader*>(loads[i].host.data())->data_bytes, 256);
    }
    if (host && stage > 0)
        if (const int rc = c->d_snap.reserve(c, stage)) return rc;
    PlaneTable table(c);
    std::vector<std::vector<KfDev>> records((size_t)n);      // (read by their uploads until the stream is idle)
    for (int i = 0; i < n; i++) {
        const int s = loads[i].seq;
        end_sequence(c, s);
        const SnapView v = snapshot_view(loads[i].host.data());
        const SnapHeader& h = *v.h;
        if (h.frame_id < 0) continue;            // an empty snapshot: a restart
        Seq& q = c->seqs[s];
        // storage from the free lists: image sets (their own level 0 and right image) and keyframe slabs
        std::vector<ImageSet*> sets((size_t)h.n_image_sets, nullptr);
        for (ImageSet*& is : sets) {
            if (const int rc = acquire_set(c, q, &is)) return rc;
            is->left[0] = is->own_left0;
            is->right = is->own_right;
            is->lk[0] = is->left[0];
            is->refs = 0;
        }
        q.cur_set = sets[0];
        q.cur_set->refs = 1;
        q.kfs.clear(h.first_keyframe);           // (the ids go on from the saved slot's)
        for (int k = 0; k < h.n_keyframes - h.first_keyframe; k++) {
            KfHost kf{};
            if (const int rc = take_kf_slab(c, &kf.kps)) return rc;
            std::memcpy(kf.pose, v.kfs[k].pose, sizeof(kf.pose));
            kf.n = v.kfs[k].n;
            if (v.kfs[k].image_set >= 0) {
                kf.set = sets[v.kfs[k].image_set];
                kf.set->refs++;
            }
            q.kfs.push_back(kf);
        }
        q.kfs_retired = h.keyframes_retired;
        // host state
        std::memcpy(&q.kf, v.filter, sizeof(PoseFilter));
        std::memcpy(&q.ts, v.frame, sizeof(double));
        std::memcpy(q.pose, v.frame + sizeof(double), sizeof(q.pose));
        std::memcpy(&q.stats, v.frame + sizeof(double) + sizeof(q.pose), sizeof(q.stats));
        q.trajectory.assign(v.trajectory, v.trajectory + h.n_trajectory);
        q.frame_id = h.frame_id; q.n_host = h.n_keypoints; q.pending = false;
        // the keyframe table. Template cache: the keyframes a fresh run would hold ring blocks for get theirs with
        // the "stored" flags cleared, the others have none (as after their eviction)
        // The records of the resident keyframes, in table order: rec[j] is ring slot j
        std::vector<KfDev>& rec = records[i];
        const int resident = q.kfs.resident(), mask = c->max_kf - 1;
        rec.resize((size_t)std::min(c->max_kf, h.n_keyframes));     // (slots [0, that) cover every resident id's)
        for (int k = h.first_keyframe; k < h.n_keyframes; k++) {
            KfDev& d = rec[(size_t)(k & mask)];
            fill_kf_record(c, q, k, q.kfs[k], d);
            std::memcpy(d.pose, q.kfs[k].pose, sizeof(d.pose));
            d.n = q.kfs[k].n;
            if (c->tmpl_kf > 0) {
                if (k < h.n_keyframes - c->tmpl_kf) d.tmpl = nullptr;
                else HIP_TRY(hipMemsetAsync(d.tmpl_valid, 0, c->tmpl_valid_bytes, st));
            }
        }
        // (one copy while the resident ids do not wrap, else the two ends of the table)
        const int s0 = h.first_keyframe & mask;
        const int run0 = std::min(resident, c->max_kf - s0);
        HIP_TRY(hipMemcpyAsync(q.d_kfs + s0, rec.data() + s0, sizeof(KfDev) * (size_t)run0, hipMemcpyHostToDevice, st));
        if (resident > run0)
            HIP_TRY(hipMemcpyAsync(q.d_kfs, rec.data(), sizeof(KfDev) * (size_t)(resident - run0), hipMemcpyHostToDevice, st));
        // the data part -> device
        const uint8_t* base = static_cast<const uint8_t*>(loads[i].data);
        if (host && h.data_bytes > 0) {
            HIP_TRY(hipMemcpyAsync(c->d_snap.p + stage_off[i], loads[i].data, (size_t)h.data_bytes, hipMemcpyHostToDevice, st));
            base = c->d_snap.p + stage_off[i];
        }
        const std::vector<DevPlane> dev = device_planes(c, q, sets);
        for (size_t j = 0; j < dev.size(); j++) {
            const svo_snapshot_plane& e = v.dir[j];
            if (const int rc = table.add(base + e.offset, dev[j].p, e.row_bytes, e.rows, e.row_bytes, dev[j].pitch)) return rc;
        }
    }
    if (const int rc = table.tiles.launch(false)) return rc;
    HIP_TRY(hipStreamSynchronize(st));       // loaded: svo_wait means that
    return SVO_OK;
}

extern "C" int svo_snapshot_info(const void* host_part, int64_t bytes, struct svo_snapshot_info* out) {
    std::vector<uint8_t> copy;
    if (const int rc = check_snapshot(host_part, bytes, copy)) return rc;
    if (out) std::memcpy(out, copy.data(), sizeof(*out));
    return SVO_OK;
}
