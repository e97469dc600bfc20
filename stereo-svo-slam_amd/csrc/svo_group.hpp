// svo_group.hpp — one group of sequences as the ctx drives it (svo_ctx*.hip): the opaque interface of svo_group.hip
// (creation, settings, restarts), svo_group_step.hip (grp_new_images), svo_group_export.hip (grp_export, grp_capacity),
// svo_group_map.hip (grp_export_map, grp_map_size), svo_group_view.hip (grp_export_views, grp_view_bytes),
// svo_group_scene.hip (grp_export_scenes, grp_scene_bytes), svo_group_ar.hip (grp_export_ar, grp_ar_bytes),
// svo_group_dense.hip (grp_export_disparity, grp_disparity_bytes), svo_group_cloud.hip (grp_export_cloud,
// grp_cloud_points), svo_group_voxel.hip (the voxel maps), svo_group_snapshot.hip (grp_check_snapshot, grp_save,
// grp_load, grp_snapshot_size) and svo_group_pose.hip (grp_pose_updates).
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/svo_hip.h"

namespace svo { struct RemapMap; }
struct svo_group;
struct GroupDelete { void operator()(svo_group* g) const; };   // synchronises the group's stream, then frees all
using Group = std::unique_ptr<svo_group, GroupDelete>;

int grp_create(const svo_camera_settings* cam, int width, int height, int n_sequences, int device, Group* out);
// one frame of every sequence whose two images are not NULL (a one-buffer input format: whose left[s] is not NULL;
// right may then be null); after a failure the group rejects further frames
int grp_new_images(svo_group* g, const uint8_t* const* left, const uint8_t* const* right, int stride,
                   const float* time_stamps, int mem);
// the named sequences (indices in the group) end; their slots are empty until their next frame. Runs between two
// steps of the group, on the thread that drives it. A failed group rejects it.
int grp_restart_sequences(svo_group* g, const int* seqs, int n);
// One group's share of svo_submit_trim_keyframes, between two steps of the group, on the thread that drives it: slot
// seqs[i] (index in the group) drops its keyframes below min(below[i], its retired count). A failed group rejects it.
int grp_trim_keyframes(svo_group* g, const int* seqs, const int* below, int n);
void grp_set_keyframe_window(svo_group* g, int keep);                 // svo_ctx_set_keyframe_window (the queues have drained)
svo_keyframe_range grp_keyframe_range(const svo_group* g, int seq);   // (the queues have drained)
// One group's share of svo_ctx_assign_rigs, between two steps of the group, on the thread that drives it: slot seqs[i]
// (index in the group) ends its sequence like a restart and is bound to b[i]: the rig's id, the full settings of its
// sequences from now on, and the storage of its left and right maps (owned by the ctx, valid while a slot is bound;
// null: none; rig 0: ignored, its maps are grp_set_rectification's). A failed group rejects it.
struct RigBinding {
    int rig;
    svo_camera_settings cam;
    const uint8_t* maps[2];
};
int grp_assign_rigs(svo_group* g, const int* seqs, const RigBinding* b, int n);
// One group's share of svo_submit_export, between two steps of the group, on the thread that drives it:
// seqs[i] (index in the group; ctx slot seq0 + seqs[i]) is segment seg[i] of dst->segments; the group's records
// start at record `base` of the caller's arrays (host or device memory: mem). Delivered on return. A failed group
// rejects it.
int grp_export(svo_group* g, int what, int mem, const int* seqs, const int* seg, int n, int seq0, int64_t base,
               const svo_export_dst* dst);
// One group's share of svo_submit_export_map (svo_group_map.hip), between two steps of the group, on the thread that
// drives it: slot seqs[i] (index in the group; ctx slot seq0 + seqs[i]) fills dst->segments[seg[i]] and goes where
// regions[i] says (host or device points: mem). Delivered on return. A failed group rejects it.
int grp_export_map(svo_group* g, int mem, const int* seqs, const int* seg, const svo_map_region* regions, int n, int seq0,
                   const svo_map_filter* filter, const svo_map_dst* dst);
// One group's share of svo_submit_export_views (svo_group_view.hip), between two steps of the group, on the thread that
// drives it: slot seqs[i] (index in the group; ctx slot seq0 + seqs[i]) fills dst->segments[seg[i]] and its image goes
// to byte seg[i] * image_bytes of dst->pixels (host or device memory: mem). style: checked (grp_check_view_style).
// Delivered on return. A failed group rejects it.
int grp_export_views(svo_group* g, int what, int mem, const int* seqs, const int* seg, int n, int seq0,
                     const svo_view_style* style, const svo_view_dst* dst);
// what svo_submit_export_views checks of a style, and the image_bytes of a checked one (they read only what never
// changes in a group)
int grp_check_view_style(const svo_group* g, const svo_view_style* style);
int64_t grp_view_bytes(const svo_group* g, const svo_view_style* style);
// One group's share of svo_submit_export_scenes (svo_group_scene.hip), between two steps of the group, on the thread
// that drives it: slot seqs[i] (index in the group; ctx slot seq0 + seqs[i]) seen through cameras[i] fills
// dst->segments[seg[i]] and its image goes to byte seg[i] * image_bytes of dst->pixels (host or device memory: mem).
// style and cameras: checked (scene_check_style, scene_check_camera). Delivered on return. A failed group rejects it.
int grp_export_scenes(svo_group* g, int mem, const int* seqs, const int* seg, int n, int seq0, const svo_scene_style* style,
                      const svo_scene_camera* cameras, const svo_scene_dst* dst);
int64_t grp_scene_bytes(const svo_scene_style* style);   // the image_bytes of a checked style
// grp_export_scenes with cloud points (svo_submit_export_scenes_clouds). clouds: checked (grp_check_scene_clouds), its
// extra is not read; extra: null, or the span of every seqs[i], checked; clouds->info[seg[i]] is filled if there is one.
// clouds == null is grp_export_scenes. sgm: checked (grp_check_cloud_sgm); the live layer is then the SGM cloud job's.
int grp_export_scenes_clouds(svo_group* g, int mem, const int* seqs, const int* seg, int n, int seq0, const svo_scene_style* style,
                             const svo_scene_camera* cameras, const svo_scene_dst* dst, const svo_scene_clouds* clouds,
                             const svo_scene_span* extra, const svo_sgm_params* sgm = nullptr);
// what svo_submit_export_scenes_clouds checks of a clouds but for its spans
int grp_check_scene_clouds(const svo_group* g, const svo_scene_clouds* clouds);
// What svo_submit_export_ar copied of its caller's arrays, checked; the jobs of all groups share one (read only).
// The meshes lie back to back: mesh m has vertices [v0, v0 + n_vertices) (3 floats each), triangles [t0, t0 +
// n_triangles) (3 indices each) and, with has_rgb, the colours [c0, c0 + n_triangles).
struct ArJob {
    svo_ar_style style{};
    struct Mesh { size_t v0, t0, c0; int n_vertices, n_triangles; bool has_rgb; };
    std::vector<Mesh> meshes;
    std::vector<float> vertices;
    std::vector<int32_t> triangles;
    std::vector<uint32_t> rgb;
    std::vector<svo_ar_instance> instances;
};
// One group's share of svo_submit_export_ar (svo_group_ar.hip), between two steps of the group, on the thread that
// drives it: slot seqs[i] (index in the group; ctx slot seq0 + seqs[i]) shows the instances [inst0[i], inst1[i]) of
// `job`, fills dst->segments[seg[i]] and its image goes to byte seg[i] * image_bytes of dst->pixels (host or device
// memory: mem). Delivered on return. A failed group rejects it.
int grp_export_ar(svo_group* g, int mem, const int* seqs, const int* seg, const int* inst0, const int* inst1, int n, int seq0,
                  const ArJob* job, const svo_ar_dst* dst);
int64_t grp_ar_bytes(const svo_group* g, const svo_ar_style* style);   // the image_bytes of a checked style
// grp_export_ar hidden behind the slots' dense stereo depth (svo_submit_export_ar_occluded). occlusion: checked
// (grp_check_ar_occlusion) with on == 1; occlusion->info[seg[i]] is filled if there is one. occlusion == null is
// grp_export_ar. sgm: checked (grp_check_cloud_sgm); the occluder is then the SGM cloud job's.
int grp_export_ar_occluded(svo_group* g, int mem, const int* seqs, const int* seg, const int* inst0, const int* inst1, int n, int seq0,
                           const ArJob* job, const svo_ar_dst* dst, const svo_ar_occlusion* occlusion, const svo_sgm_params* sgm = nullptr);
// what svo_submit_export_ar_occluded checks of an occlusion (null: nothing)
int grp_check_ar_occlusion(const svo_group* g, const svo_ar_occlusion* occlusion);
// One group's share of svo_submit_export_disparity (svo_group_dense.hip), between two steps of the group, on the thread
// that drives it: slot seqs[i] (index in the group; ctx slot seq0 + seqs[i]) fills dst->segments[seg[i]] and its planes
// go to byte seg[i] * image_bytes of dst->values (host or device memory: mem). style: checked
// (grp_check_disparity_style). check: the cross-check of a checked job (checked too), or null. Delivered on return. A
// failed group rejects it.
int grp_export_disparity(svo_group* g, int what, int mem, const int* seqs, const int* seg, int n, int seq0,
                         const svo_disparity_style* style, const svo_stereo_check* check, const svo_sgm_params* sgm,
                         const svo_disparity_dst* dst);
// what svo_submit_export_disparity_sgm checks beside the style: the params, and an effective search_x <= 63
int grp_check_disparity_sgm(const svo_group* g, const svo_disparity_style* style, const svo_sgm_params* sgm,
                            const char* who = "svo_submit_export_disparity_sgm");
// what svo_submit_export_disparity checks of a style, and the image_bytes of a checked one (they read only what never
// changes in a group)
int grp_check_disparity_style(const svo_group* g, const svo_disparity_style* style, const svo_stereo_check* check);
int64_t grp_disparity_bytes(const svo_group* g, const svo_disparity_style* style, const svo_stereo_check* check);
// One group's share of svo_submit_export_cloud (svo_group_cloud.hip), as grp_export_disparity: slot seqs[i] fills
// dst->segments[seg[i]] and its records start at record seg[i] * points_per_slot of dst->points. style: checked
// (grp_check_cloud_style). check: as in grp_export_disparity. Delivered on return. A failed group rejects it.
int grp_export_cloud(svo_group* g, int what, int mem, const int* seqs, const int* seg, int n, int seq0, const svo_cloud_style* style,
                     const svo_stereo_check* check, const svo_cloud_dst* dst, const svo_sgm_params* sgm = nullptr);
// what svo_submit_export_cloud checks of a style, and the points_per_slot of a checked one
int grp_check_cloud_style(const svo_group* g, const svo_cloud_style* style, const svo_stereo_check* check);
int64_t grp_cloud_points(const svo_group* g, const svo_cloud_style* style);
// what svo_submit_export_cloud_sgm checks beside the style: the params, and an effective search_x <= 63
int grp_check_cloud_sgm(const svo_group* g, const svo_cloud_style* style, const svo_sgm_params* sgm, const char* who);
// what one slot of a device-mode job with that checked style and check stages in the cloud job's blocks: slot_bytes
// [+ reverse_bytes]; an SGM job (sgm != null) has no reverse block
int64_t grp_cloud_slot_bytes(const svo_group* g, const svo_cloud_style* style, const svo_stereo_check* check,
                             const svo_sgm_params* sgm = nullptr);
// Voxel maps (svo_group_voxel.hip). grp_set_voxel_maps: the named slots (indices in the group) get a cleared map of
// `params` (checked), or with params == null lose theirs; grp_voxel_map_info: false for a slot without a map (both:
// the queues have drained). The three jobs run between two steps of the group, on the thread that drives it, and are
// delivered on return; a failed group rejects them. grp_fuse_clouds: slot seqs[i] fills info[seg[i]];
// grp_export_voxel_maps: slot seqs[i] fills dst->segments[seg[i]] and goes where regions[i] says. grp_fuse_clouds with
// sgm (checked: grp_check_cloud_sgm) fuses the records of the SGM cloud job.
int grp_set_voxel_maps(svo_group* g, const int* seqs, int n, const svo_voxel_params* params);
bool grp_voxel_map_info(svo_group* g, int seq, svo_voxel_map_info* info);
int grp_fuse_clouds(svo_group* g, int what, const int* seqs, const int* seg, int n, int seq0, const svo_cloud_style* style,
                    const svo_stereo_check* check, uint32_t stamp, svo_fuse_info* info, const svo_sgm_params* sgm = nullptr);
int grp_export_voxel_maps(svo_group* g, int mem, const int* seqs, const int* seg, const svo_voxel_region* regions, int n, int seq0,
                          const svo_voxel_filter* filter, const svo_voxel_dst* dst);
int grp_clear_voxel_maps(svo_group* g, const int* seqs, int n);
// the prune job: the maps of the named slots rebuilt from their kept entries. centers: three floats per named slot
// (given mode), not read in pose mode. grp_voxel_edge: the voxel edge of a slot's map (0: no map); it changes only in
// grp_set_voxel_maps, so the submitting thread may read it.
int grp_prune_voxel_maps(svo_group* g, const int* seqs, const int* seg, int n, int seq0, const svo_voxel_keep* keep, int center_mode,
                         const float* centers, svo_prune_info* info);
// the carve job ("voxel carve"): grp_prune_voxel_maps with a carve. The occluder of a slot is grp_export_cloud itself, in
// device mode, the camera frame and the organized layout of the current frame, into the block of the occluded AR job;
// the camera is svo_ar_camera_of_pose of the slot's pose and rig. cloud, sgm and check: checked as for the AR job.
int grp_carve_voxel_maps(svo_group* g, const int* seqs, const int* seg, int n, int seq0, const svo_cloud_style* cloud, const svo_sgm_params* sgm,
                         const svo_stereo_check* check, const svo_voxel_carve_rule* carve, const svo_voxel_keep* keep, int center_mode,
                         const float* centers, svo_carve_info* info);
float grp_voxel_edge(const svo_group* g, int seq);
// Voxel entries ("voxel entries"). grp_save_voxel_maps: grp_export_voxel_maps with entry records. grp_load_voxel_maps:
// spans[i] (entries in `mem`, n, voxel: checked) is offered to the map of slot seqs[i], which fills info[seg[i]]; one
// merge launch for the group's share. grp_resize_voxel_maps (the queues have drained) runs in phases, so that the ctx can
// take every group through one before any enters the next: CHECK changes nothing and answers SVO_ERR_CAPACITY if a named
// slot's entries do not fit log2_capacity; ALLOC makes the new map of every slot that moves; MOVE rehashes into them
// and releases the old maps; ABORT gives back what ALLOC made (after an ALLOC that failed, here or in another group).
int grp_save_voxel_maps(svo_group* g, int mem, const int* seqs, const int* seg, const svo_voxel_region* regions, int n, int seq0,
                        const svo_voxel_filter* filter, const svo_voxel_entry_dst* dst);
int grp_load_voxel_maps(svo_group* g, int mode, int mem, const int* seqs, const int* seg, const svo_voxel_entry_span* spans, int n, int seq0,
                        svo_voxel_load_info* info);
enum { VOXEL_RESIZE_CHECK = 0, VOXEL_RESIZE_ALLOC = 1, VOXEL_RESIZE_MOVE = 2, VOXEL_RESIZE_ABORT = 3 };
int grp_resize_voxel_maps(svo_group* g, const int* seqs, int n, int log2_capacity, int phase);
// what svo_map_size reports of a slot (the queues have drained)
void grp_map_size(const svo_group* g, int seq, int from_keyframe, int* keyframes, int64_t* points_bound, int* from = nullptr);
// Snapshots (svo_submit_save / svo_submit_load). grp_check_snapshot: everything svo_submit_load checks of one
// snapshot, on the caller's thread (it reads only what never changes in a group; slot_cam: the settings of the
// target slot's rig); *host_copy receives the checked host part. grp_save / grp_load: one group's share, between two steps of the group, on the thread that drives it;
// seqs / loads[i].seq are indices in the group; delivered on return. A failed group rejects them.
struct SnapshotLoad {
    int seq;
    std::vector<uint8_t> host;        // the checked host part
    const void* data;                 // the data part (host or device memory: mem)
};
int grp_check_snapshot(const svo_group* g, const svo_camera_settings* slot_cam, const svo_snapshot* snap,
                       std::vector<uint8_t>* host_copy);
int grp_save(svo_group* g, const int* seqs, int n, const svo_snapshot* snaps, int mem);
int grp_load(svo_group* g, const SnapshotLoad* loads, int n, int mem);
int grp_snapshot_size(svo_group* g, int seq, int64_t* host_bytes, int64_t* data_bytes);   // (the queues have drained)
// One group's share of svo_submit_pose_updates (svo_group_pose.hip), between two steps of the group, on the thread
// that drives it: counts[i] > 0 samples for slot seqs[i] (index in the group), `samples` in that order; filtered[i]:
// host memory for the slot's counts[i] filtered poses, or null. Delivered on return. A failed group rejects it.
int grp_pose_updates(svo_group* g, const int* seqs, const int* counts, int n, const svo_pose_sample* samples,
                     float* const* filtered);
int grp_capacity(const svo_group* g);                 // keypoint records a sequence can hold (svo_export_capacity)
void grp_drop_finished_runs(svo_group* g, int seq);   // seq < 0: of every sequence of the group
svo_memory grp_memory(const svo_group* g);
void grp_set_exact_pinv(svo_group* g, int on);
// rectification of every frame from the next one on: maps[0] the left image's, maps[1] the right image's
// (owned by the ctx, device memory that stays valid while set); nullptr: off
void grp_set_rectification(svo_group* g, const svo::RemapMap* maps);
// the input format (SVO_INPUT_*, a valid one) of every frame from the next one on. A format that converts gets its
// image table here, the first time: a failure leaves the group's setting as it was.
int grp_set_input_format(svo_group* g, int format);
void grp_enable_timing(svo_group* g, int on);
svo_totals grp_totals(const svo_group* g);
const std::vector<svo_launch_shape>& grp_launch_shapes(const svo_group* g);   // (svo_ctx_get_launch_shapes)
