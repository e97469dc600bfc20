"""ctypes binding of the product library libsvo_hip.so (C ABI: include/svo_hip.h).

torch is used only as plumbing: device buffers and the current HIP stream.
There is no CPU fallback — a missing library or GPU raises.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.normpath(os.path.join(_HERE, "..", "csrc"))
LIB_PATH = os.environ.get("SVO_HIP_LIB", os.path.join(CSRC, "libsvo_hip.so"))   # override: diagnostic builds
_LIB = None

# every symbol include/svo_hip.h declares
SYMBOLS = (
    "svo_last_error", "svo_version", "svo_handle_create", "svo_handle_destroy",
    "svo_handle_set_stream", "svo_handle_synchronize", "svo_build_pyramid",
    "svo_build_lk_pyramid", "svo_sparse_align", "svo_klt_track", "svo_reproj_gn",
    "svo_ssd_disparity", "svo_depth_filter_update",
    "svo_ctx_create", "svo_ctx_destroy", "svo_new_images", "svo_submit_images", "svo_wait",
    "svo_ctx_get_groups", "svo_new_image", "svo_get_pose",
    "svo_get_frame_keypoints", "svo_get_keyframe_count", "svo_get_keyframe",
    "svo_get_trajectory", "svo_update_pose", "svo_get_frame_stats", "svo_ctx_enable_timing",
    "svo_get_totals", "svo_handle_set_exact_pinv", "svo_ctx_set_exact_pinv",
    "svo_handle_set_fast_solver", "svo_ctx_set_fast_solver",
    "svo_device_malloc", "svo_device_free", "svo_copy_to_device", "svo_copy_to_host",
    "svo_copy_image_to_device", "svo_project_keypoints",
    "svo_ctx_get_launch_shapes", "svo_pick_launch_shapes", "svo_pick_sia_lds_bytes", "svo_pinv6_check",
    "svo_solve6_check", "svo_remap_linear", "svo_ctx_set_rectification",
    "svo_detect_keypoints", "svo_detect_shape",
    "svo_ctx_restart_sequences", "svo_get_finished_runs", "svo_get_finished_run",
    "svo_drop_finished_runs", "svo_ctx_get_memory",
    "svo_input_format_info", "svo_convert_frames", "svo_ctx_set_input_format",
    "svo_export_capacity", "svo_submit_export", "svo_export", "svo_pack_keypoints",
    "svo_snapshot_size", "svo_submit_save", "svo_save_sequences", "svo_submit_load", "svo_load_sequences",
    "svo_snapshot_info", "svo_copy_segments",
    "svo_reproj_gn_batch", "svo_filter_update_batch", "svo_sparse_align_batch",
    "svo_submit_pose_updates", "svo_update_poses", "svo_pose_filter_batch",
    "svo_map_size", "svo_submit_export_map", "svo_export_map", "svo_pack_map_points",
    "svo_view_size", "svo_submit_export_views", "svo_export_views", "svo_render_views",
    "svo_disparity_size", "svo_submit_export_disparity", "svo_export_disparity", "svo_dense_disparity",
    "svo_cloud_size", "svo_submit_export_cloud", "svo_export_cloud", "svo_cloud_points",
    "svo_disparity_size_checked", "svo_submit_export_disparity_checked", "svo_export_disparity_checked",
    "svo_dense_disparity_checked", "svo_submit_export_cloud_checked", "svo_export_cloud_checked",
    "svo_cloud_points_checked",
    "svo_submit_export_disparity_sgm", "svo_export_disparity_sgm",
    "svo_dense_cost_volume", "svo_sgm_aggregate", "svo_dense_disparity_sgm",
    "svo_submit_export_disparity_sgm_checked", "svo_export_disparity_sgm_checked", "svo_dense_disparity_sgm_checked",
    "svo_submit_export_cloud_sgm", "svo_export_cloud_sgm", "svo_cloud_points_sgm",
    "svo_submit_fuse_clouds_sgm", "svo_fuse_clouds_sgm", "svo_submit_export_scenes_clouds_sgm", "svo_export_scenes_clouds_sgm",
    "svo_submit_export_ar_occluded_sgm", "svo_export_ar_occluded_sgm",
    "svo_scene_size", "svo_scene_look_at", "svo_scene_frustum", "svo_submit_export_scenes", "svo_export_scenes",
    "svo_render_scene",
    "svo_submit_export_scenes_clouds", "svo_export_scenes_clouds", "svo_render_scene_clouds",
    "svo_voxel_map_bytes", "svo_voxel_clear", "svo_voxel_fuse", "svo_voxel_info", "svo_voxel_extract",
    "svo_ctx_set_voxel_maps", "svo_get_voxel_map_info", "svo_submit_fuse_clouds", "svo_fuse_clouds",
    "svo_submit_export_voxel_maps", "svo_export_voxel_maps", "svo_submit_clear_voxel_maps",
    "svo_voxel_prune", "svo_submit_prune_voxel_maps", "svo_prune_voxel_maps", "svo_voxel_carve",
    "svo_submit_carve_voxel_maps", "svo_carve_voxel_maps",
    "svo_voxel_pack", "svo_voxel_merge", "svo_voxel_rehash", "svo_submit_save_voxel_maps", "svo_save_voxel_maps",
    "svo_submit_load_voxel_maps", "svo_load_voxel_maps", "svo_ctx_resize_voxel_maps",
    "svo_ar_size", "svo_ar_camera_of_pose", "svo_submit_export_ar", "svo_export_ar", "svo_render_ar",
    "svo_submit_export_ar_occluded", "svo_export_ar_occluded", "svo_render_ar_occluded",
    "svo_remap_linear_multi", "svo_ctx_add_rigs", "svo_ctx_remove_rigs", "svo_ctx_assign_rigs", "svo_ctx_get_slot_rig",
    "svo_ctx_get_rigs",
    "svo_klt_track_batch", "svo_klt_cache_layout",
    "svo_rectify_inverse", "svo_build_rectify_maps", "svo_ctx_add_rigs_calibrated", "svo_ctx_set_calibration",
    "svo_submit_trim_keyframes", "svo_trim_keyframes", "svo_ctx_set_keyframe_window", "svo_get_keyframe_range",
    "svo_keyframe_launch_info", "svo_compact_batch", "svo_keyframe_merge_batch", "svo_keyframe_init_batch",
    "svo_keyframe_record_layout", "svo_ssd_disparity_batch",
    "svo_sparse_align_batch_mats", "svo_pose_mats_layout", "svo_filter_update_table_batch",
    "svo_sia_records_check", "svo_ssd_disparity_check",
)

# svo_ctx_set_input_format / svo_convert_frames: how the buffers of a sequence become its two gray images
INPUT_GRAY_PAIR, INPUT_BGR_PAIR, INPUT_RGB_PAIR, INPUT_SBS_GRAY, INPUT_SBS_BGR, INPUT_SBS_RGB, INPUT_CH3_ECON = range(7)
INPUT_FORMATS = ("gray_pair", "bgr_pair", "rgb_pair", "sbs_gray", "sbs_bgr", "sbs_rgb", "ch3_econ")
INGEST_COPY, INGEST_GRAY = 0, 1
# svo_submit_export: what is exported, and where the arrays live
EXPORT_FRAMES, EXPORT_LAST_KEYFRAMES = 0, 1
EXPORT_WHAT = ("frames", "last_keyframes")
MEM_HOST, MEM_DEVICE = 0, 1


class SvoError(RuntimeError):
    pass


class CameraSettings(C.Structure):
    """svo_camera_settings == CameraSettings, src/include/stereo_slam_types.hpp:16-36."""
    _fields_ = [(n, C.c_float) for n in
                ("baseline", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")] + \
               [(n, C.c_int32) for n in
                ("grid_height", "grid_width", "search_x", "search_y",
                 "window_size_pose_estimator", "window_size_opt_flow",
                 "window_size_depth_calculator", "max_pyramid_levels",
                 "min_pyramid_level_pose_estimation")]

    @classmethod
    def from_dict(cls, d):
        cam = cls()
        for name, _ in cls._fields_:
            setattr(cam, name, d[name])
        return cam


RIG_FLOATS = ("baseline", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")


class Rig(C.Structure):
    """svo_rig (include/svo_hip.h): what differs between two units of one camera model."""
    _fields_ = [(n, C.c_float) for n in RIG_FLOATS] + \
               [(n, C.c_void_p) for n in ("left_map_x", "left_map_y", "right_map_x", "right_map_y")] + \
               [("mem", C.c_int32), ("_reserved", C.c_int32)]

    @classmethod
    def from_dict(cls, d):
        """the ten float settings of a camera-settings dict or CameraSettings (no maps)"""
        get = d.__getitem__ if isinstance(d, dict) else lambda n: getattr(d, n)
        return cls(**{n: get(n) for n in RIG_FLOATS})


assert C.sizeof(Rig) == 80


class CameraCalibration(C.Structure):
    """svo_camera_calibration (include/svo_hip.h): K, D, R, P of one camera as EurocInput reads them
    (src/app/euroc_input.cpp:24-49); D = k1, k2, p1, p2, k3, k4, k5, k6."""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 9)]

    @classmethod
    def from_mats(cls, K, D, R, P):
        """K 3x3; D of 4, 5 or 8 coefficients (the rest 0; more raises); R 3x3 or None (identity); P 3x3, or the
        3x4 of a settings file (its left 3x3 is used)"""
        K, P = np.asarray(K, np.float64), np.asarray(P, np.float64)
        D = np.asarray(D, np.float64).ravel()
        R = np.eye(3) if R is None else np.asarray(R, np.float64)
        if K.shape != (3, 3) or R.shape != (3, 3) or P.shape not in ((3, 3), (3, 4)):
            raise ValueError(f"K, R are 3x3 and P is 3x3 or 3x4, not {K.shape}, {R.shape}, {P.shape}")
        if D.size not in (4, 5, 8):
            raise ValueError(f"D has 4, 5 or 8 coefficients, not {D.size}")
        cal = cls()
        cal.K[:] = K.ravel().tolist()
        cal.D[:] = D.tolist() + [0.0] * (8 - D.size)
        cal.R[:] = R.ravel().tolist()
        cal.P[:] = P[:, :3].ravel().tolist()
        return cal


assert C.sizeof(CameraCalibration) == 280


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("stride", C.c_int32)]


class KltKeyframe(C.Structure):
    """svo_klt_keyframe (include/svo_hip.h): one keyframe of svo_klt_track_batch."""
    _fields_ = [("lk", Image * 3), ("n_lk", C.c_int32), ("n_kps", C.c_int32), ("kps2d", C.c_void_p),
                ("tmpl", C.c_void_p), ("tmpl_valid", C.c_void_p), ("tmpl_bytes", C.c_int64),
                ("tmpl_valid_bytes", C.c_int64), ("tmpl_cap", C.c_int32), ("tmpl_win", C.c_int32)]


class KltSequence(C.Structure):
    """svo_klt_sequence (include/svo_hip.h): one sequence of svo_klt_track_batch."""
    _fields_ = [("kfs", C.POINTER(KltKeyframe)), ("n_kfs", C.c_int32), ("n_cur", C.c_int32), ("cur", Image * 3),
                ("n", C.c_void_p), ("kf_id", C.c_void_p), ("kp_index", C.c_void_p), ("kps3d", C.c_void_p),
                ("pose", C.c_void_p), ("cam", CameraSettings)] + \
               [(n, C.c_void_p) for n in ("tracked", "status", "err", "proj_out", "ref_out")]


assert (C.sizeof(KltKeyframe), C.sizeof(KltSequence)) == (128, 248)


KPS_PLANES = ("kps2d", "kps3d", "flags", "kf_id", "kp_index", "outlier_count", "inlier_count", "kf_inv_depth",
              "kf_variance", "score", "level_type", "color", "n")


class KpsPlanes(C.Structure):
    """svo_kps_planes: the twelve planes of a keypoint set and its count, device addresses"""
    _fields_ = [(name, C.c_void_p) for name in KPS_PLANES]


class CompactSequence(C.Structure):
    _fields_ = [("src", KpsPlanes), ("dst", KpsPlanes), ("mode", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("start", C.c_int32), ("enable", C.c_void_p), ("zero", C.c_void_p), ("zero_res", C.c_void_p),
                ("min_kf", C.c_void_p), ("zero_count", C.c_int32), ("zero_res_count", C.c_int32)]


class MergeSequence(C.Structure):
    _fields_ = [("cam", CameraSettings), ("width", C.c_int32), ("height", C.c_int32), ("det", C.c_void_p),
                ("n_det", C.c_void_p), ("kps", KpsPlanes), ("sel", C.c_void_p), ("sel_level", C.c_void_p),
                ("sel_cell", C.c_void_p), ("occupied", C.c_void_p), ("old_count", C.c_void_p), ("overflow", C.c_void_p),
                ("enable", C.c_void_p), ("occupied_count", C.c_int32), ("pad_", C.c_int32)]


class KfInitSequence(C.Structure):
    _fields_ = [("cam", CameraSettings), ("first_frame", C.c_int32), ("new_kf_id", C.c_int32), ("kf_mask", C.c_int32),
                ("evict_id", C.c_int32), ("kps", KpsPlanes), ("record", KpsPlanes), ("old_count", C.c_void_p),
                ("disparity", C.c_void_p), ("frame_pose", C.c_void_p), ("kfs", C.c_void_p), ("kfs_bytes", C.c_int64),
                ("color_lcg", C.c_void_p), ("n_out", C.c_void_p), ("enable", C.c_void_p), ("tmpl", C.c_void_p),
                ("tmpl_valid", C.c_void_p), ("tmpl_valid_bytes", C.c_int32), ("tmpl_cap", C.c_int32),
                ("tmpl_win", C.c_int32), ("pad_", C.c_int32)]


class SsdSequence(C.Structure):
    _fields_ = [("left", Image), ("right", Image), ("n", C.c_void_p), ("kps2d", C.c_void_p), ("disparity", C.c_void_p),
                ("win", C.c_int32), ("search_x", C.c_int32), ("search_y", C.c_int32), ("clamp_half", C.c_int32),
                ("first", C.c_int32), ("cap", C.c_int32), ("first_ptr", C.c_void_p), ("enable", C.c_void_p)]


class FilterKeyframe(C.Structure):
    """svo_filter_keyframe (include/svo_hip.h): one keyframe of svo_filter_update_table_batch."""
    _fields_ = [("pose", C.c_float * 6)] + \
               [(n, C.c_void_p) for n in ("kps2d", "kps3d", "flags", "outlier_count", "inlier_count")] + \
               [("n", C.c_int32), ("pad_", C.c_int32)]


class FilterTableSequence(C.Structure):
    """svo_filter_table_sequence (include/svo_hip.h): one sequence of svo_filter_update_table_batch."""
    _fields_ = [("cam", CameraSettings), ("kps", KpsPlanes), ("frame_pose", C.c_void_p), ("disparity", C.c_void_p),
                ("kfs", C.POINTER(FilterKeyframe)), ("records", C.c_void_p), ("records_bytes", C.c_int64),
                ("table", C.c_int32), ("kf_mask", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("inside_count", C.c_void_p)]


assert (C.sizeof(KpsPlanes), C.sizeof(CompactSequence), C.sizeof(MergeSequence), C.sizeof(KfInitSequence),
        C.sizeof(SsdSequence), C.sizeof(FilterKeyframe), C.sizeof(FilterTableSequence)) == (104, 264, 272, 400, 112, 72, 248)


def _addr(x):
    """a device address from a tensor, an integer or None"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    assert x.is_cuda
    return C.c_void_p(x.data_ptr())


def _fill(struct, d, skip=()):
    """the fields of a ctypes structure from a dict: addresses for pointer fields, nested dicts for nested
    structures, values as they are otherwise; a missing key is NULL / 0"""
    for name, typ in struct._fields_:
        if name in skip or name not in d or d[name] is None:
            continue
        v = d[name]
        if typ is C.c_void_p:
            setattr(struct, name, _addr(v))
        elif typ is KpsPlanes:
            _fill(getattr(struct, name), v)
        elif typ in (C.c_int32, C.c_int64):
            setattr(struct, name, int(v))
        else:
            setattr(struct, name, v)


class InputSide(C.Structure):
    """svo_input_side (include/svo_hip.h)."""
    _fields_ = [("buffer", C.c_int32), ("start_column", C.c_int32), ("op", C.c_int32), ("channel", C.c_int32),
                ("weight", C.c_int32 * 3)]


class InputLayout(C.Structure):
    """svo_input_layout (include/svo_hip.h)."""
    _fields_ = [("buffers", C.c_int32), ("channels", C.c_int32), ("min_row_pixels", C.c_int32),
                ("left", InputSide), ("right", InputSide)]


GN_TRACE_DTYPE = np.dtype([("level", "<i4"), ("n_gradient", "<i4"), ("n_cost", "<i4"),
                           ("n_accepted", "<i4"), ("exit_small", "<i4"),
                           ("initial_cost", "<f4"), ("final_cost", "<f4"), ("pose", "<f4", (6,))])
assert GN_TRACE_DTYPE.itemsize == 52


DET_CELL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("score", "<f4"), ("type", "<i4")])
assert DET_CELL_DTYPE.itemsize == 16


# svo_export_segment (include/svo_hip.h): one per named slot of an export
EXPORT_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("keyframe_id", "<i4"),
                                 ("is_keyframe", "<i4"), ("n", "<i4"), ("first", "<i8"), ("pose", "<f4", (6,)),
                                 ("time_stamp", "<f4"), ("_pad", "<i4")])
assert EXPORT_SEGMENT_DTYPE.itemsize == 64


class ExportDst(C.Structure):
    """svo_export_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("kps2d", C.c_void_p), ("kps3d", C.c_void_p), ("info", C.c_void_p),
                ("capacity", C.c_int64)]


# map export (svo_submit_export_map, include/svo_hip.h): a point, a keyframe entry, a segment (one per named slot)
MAP_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("color", "u1", (3,)), ("flags", "u1")])
MAP_KEYFRAME_DTYPE = np.dtype([("id", "<i4"), ("n_total", "<i4"), ("n", "<i4"), ("_pad", "<i4"), ("first", "<i8"),
                               ("pose", "<f4", (6,))])
MAP_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("status", "<i4"),
                              ("n_keyframes", "<i4"), ("keyframes_retired", "<i4"), ("from_keyframe", "<i4"),
                              ("n_exported", "<i4"), ("n_points", "<i8"), ("points_bound", "<i8"),
                              ("time_stamp", "<f4"), ("_pad", "<i4", (3,))])      # (_pad[0]: first_keyframe)
# svo_map_region as a numpy record, so that a call's regions are one array
MAP_REGION_DTYPE = np.dtype([("first_point", "<i8"), ("point_capacity", "<i8"), ("first_keyframe_entry", "<i8"),
                             ("keyframe_capacity", "<i4"), ("from_keyframe", "<i4")])
assert (MAP_POINT_DTYPE.itemsize, MAP_KEYFRAME_DTYPE.itemsize, MAP_SEGMENT_DTYPE.itemsize,
        MAP_REGION_DTYPE.itemsize) == (16, 48, 64, 32)
MAP_COMPLETE, MAP_TOO_SMALL = 0, 1


def map_first_keyframe(segment):
    """svo_map_segment.first_keyframe of a MAP_SEGMENT_DTYPE record: the slot's oldest resident keyframe (the C union
    member over _pad[0])"""
    return int(segment["_pad"][0])
IGNORE_DURING_REFINEMENT, IGNORE_COMPLETELY, IGNORE_TEMPORARY = 1, 2, 4


class MapFilter(C.Structure):
    """svo_map_filter (include/svo_hip.h): all zero keeps every keypoint of every keyframe."""
    _fields_ = [("drop_flags", C.c_uint32), ("own_only", C.c_int32), ("min_inliers", C.c_int32),
                ("_reserved", C.c_int32)]


class MapDst(C.Structure):
    """svo_map_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("keyframes", C.c_void_p), ("points", C.c_void_p)]


def map_filter(f):
    """a MapFilter from None (keep everything), a MapFilter or a dict of its fields"""
    if f is None:
        return MapFilter()
    return f if isinstance(f, MapFilter) else MapFilter(**f)


# views (svo_submit_export_views, include/svo_hip.h): the plane, the pixel format, a segment (one per named slot)
PLANE_LEFT, PLANE_RIGHT = 0, 1
PLANES = ("left", "right")
PIXEL_GRAY8, PIXEL_RGB8, PIXEL_RGBA8 = 0, 1, 2
PIXELS = ("gray8", "rgb8", "rgba8")
PIXEL_BYTES = (1, 3, 4)
VIEW_OK, VIEW_NONE = 0, 1
VIEW_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("keyframe_id", "<i4"),
                               ("status", "<i4"), ("n", "<i4"), ("offset", "<i8"), ("pose", "<f4", (6,)),
                               ("time_stamp", "<f4"), ("_pad", "<i4")])
assert VIEW_SEGMENT_DTYPE.itemsize == 64


class ViewStyle(C.Structure):
    """svo_view_style (include/svo_hip.h): what one view job draws."""
    _fields_ = [("plane", C.c_int32), ("level", C.c_int32), ("pixel", C.c_int32), ("markers", C.c_int32),
                ("drop_flags", C.c_uint32), ("size", C.c_int32), ("size_temporary", C.c_int32),
                ("_reserved", C.c_int32)]


class ViewDst(C.Structure):
    """svo_view_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("pixels", C.c_void_p), ("capacity", C.c_int64)]


def view_style(what=EXPORT_FRAMES, plane=PLANE_LEFT, level=0, pixel=PIXEL_GRAY8, markers=False, drop_flags=None,
               size=None, size_temporary=None):
    """a ViewStyle; plane and pixel may be names (PLANES, PIXELS). The defaults of the marker fields follow the
    reference app's window: a frame drops IGNORE_COMPLETELY keypoints and draws 20 / 10 (10 with IGNORE_TEMPORARY),
    a keyframe drops nothing and draws 10 / 10."""
    if isinstance(plane, str):
        plane = PLANES.index(plane)
    if isinstance(pixel, str):
        pixel = PIXELS.index(pixel)
    frames = int(what) == EXPORT_FRAMES
    return ViewStyle(int(plane), int(level), int(pixel), int(bool(markers)),
                     (IGNORE_COMPLETELY if frames else 0) if drop_flags is None else int(drop_flags),
                     (20 if frames else 10) if size is None else int(size),
                     10 if size_temporary is None else int(size_temporary), 0)


def view_size(cam, width, height, style):
    """svo_view_size (host only): (cols, rows, pitch, image_bytes) of one image of a view job with `style`."""
    cols, rows, pitch, nbytes = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
    _check(lib().svo_view_size(C.byref(cam), int(width), int(height), C.byref(style), C.byref(cols), C.byref(rows),
                               C.byref(pitch), C.byref(nbytes)))
    return cols.value, rows.value, pitch.value, nbytes.value


class Keypoints(C.Structure):
    """svo_keypoints (include/svo_types.h): an SoA keypoint set, views onto device memory."""
    _fields_ = [("n", C.c_int32)] + [(name, C.c_void_p) for name in (
        "kps2d", "kps3d", "flags", "keyframe_id", "keypoint_index", "outlier_count", "inlier_count",
        "kf_inv_depth", "kf_variance", "score", "level_type", "color")]


class ViewSrc(C.Structure):
    """svo_view_src (include/svo_hip.h): one image of svo_render_views."""
    _fields_ = [("image", Image), ("kps", Keypoints)]


# dense disparity and depth maps (svo_submit_export_disparity, include/svo_hip.h): the value, a segment (one per named
# slot)
DENSE_DISPARITY, DENSE_DEPTH = 0, 1
DENSE_VALUES = ("disparity", "depth")
DISPARITY_OK, DISPARITY_NONE = 0, 1
DISPARITY_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("keyframe_id", "<i4"),
                                    ("status", "<i4"), ("_pad", "<i4"), ("offset", "<i8"), ("pose", "<f4", (6,)),
                                    ("time_stamp", "<f4"), ("baseline", "<f4")])
assert DISPARITY_SEGMENT_DTYPE.itemsize == 64


class DisparityStyle(C.Structure):
    """svo_disparity_style (include/svo_hip.h): what one disparity job computes."""
    _fields_ = [("value", C.c_int32), ("step", C.c_int32), ("win", C.c_int32), ("search_x", C.c_int32),
                ("search_y", C.c_int32), ("cost", C.c_int32), ("_reserved", C.c_int32 * 2)]


class DisparitySegment(C.Structure):
    """svo_disparity_segment (include/svo_hip.h); DISPARITY_SEGMENT_DTYPE is the same layout for numpy."""
    _fields_ = [("seq", C.c_int32), ("run", C.c_int32), ("frame_id", C.c_int32), ("keyframe_id", C.c_int32),
                ("status", C.c_int32), ("_pad", C.c_int32), ("offset", C.c_int64), ("pose", C.c_float * 6),
                ("time_stamp", C.c_float), ("baseline", C.c_float)]


class DisparityDst(C.Structure):
    """svo_disparity_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("values", C.c_void_p), ("capacity", C.c_int64)]


class DenseSrc(C.Structure):
    """svo_dense_src (include/svo_hip.h): one image pair of svo_dense_disparity."""
    _fields_ = [("left", Image), ("right", Image), ("baseline", C.c_float), ("_reserved", C.c_int32)]


assert (C.sizeof(DisparityStyle), C.sizeof(DisparitySegment), C.sizeof(DisparityDst), C.sizeof(DenseSrc)) == (32, 64, 24, 56)


def disparity_style(value=DENSE_DISPARITY, step=1, win=0, search_x=0, search_y=0, cost=False):
    """a DisparityStyle; value may be a name (DENSE_VALUES); win / search_x / search_y of 0: the ctx's settings"""
    if isinstance(value, str):
        value = DENSE_VALUES.index(value)
    return DisparityStyle(int(value), int(step), int(win), int(search_x), int(search_y), int(bool(cost)))


class StereoCheck(C.Structure):
    """svo_stereo_check (include/svo_hip.h, "cross-check"): the left-right check of a checked disparity or cloud job."""
    _fields_ = [("lr", C.c_int32), ("max_lr_diff", C.c_float), ("_reserved", C.c_int32 * 6)]


assert C.sizeof(StereoCheck) == 32


def stereo_check(lr=True, max_lr_diff=0.0):
    """a StereoCheck; max_lr_diff of 0: report only (the lr plane; a cloud needs a tolerance > 0)"""
    return StereoCheck(int(bool(lr)), float(max_lr_diff))


class SgmParams(C.Structure):
    """svo_sgm_params (include/svo_hip.h, "sgm"): the penalties, the cost cap and the sub-pixel switch of an SGM search."""
    _fields_ = [("paths", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("cost_cap", C.c_int32), ("subpixel", C.c_int32),
                ("_reserved", C.c_int32 * 3)]


class SgmShape(C.Structure):
    """svo_sgm_shape (include/svo_hip.h): the lattice and candidates of one volume of svo_sgm_aggregate."""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32), ("baseline", C.c_float)]


assert (C.sizeof(SgmParams), C.sizeof(SgmShape)) == (32, 16)
# what sgm=True stands for in the Python layers (the C ABI has no defaults): chosen by tools/sgm_sweep.py over the
# numpy statement, profiles/sgm_defaults.json
SGM_DEFAULTS = dict(p1=64, p2=256, cost_cap=4095, subpixel=True)


def sgm_params(p1, p2, cost_cap, subpixel=True):
    """an SgmParams of four paths"""
    return SgmParams(4, int(p1), int(p2), int(cost_cap), int(bool(subpixel)))


def sgm_job(sgm):
    """sgm of submit_disparity / submit_cloud as (SgmParams, StereoCheck or None). None or False: (None, None); True:
    SGM_DEFAULTS; an SgmParams: itself, unchecked; a dict with p1, p2, cost_cap and, if wanted, subpixel and lr_check.
    lr_check is the cross-check of the SGM map (include/svo_hip.h, "sgm cross-check": a second SGM map of the mirrored
    pair, another rule than the top-level lr_check=): None or False: off; True: report only; a number: the tolerance"""
    if sgm is None or sgm is False:
        return None, None
    if isinstance(sgm, SgmParams):
        return sgm, None
    fields = dict(SGM_DEFAULTS if sgm is True else sgm)
    lr = fields.pop("lr_check", None)
    check = None if lr is None or lr is False else stereo_check(True, 0.0 if lr is True else float(lr))
    return sgm_params(**fields), check


def sgm_consumer(sgm, lr_check, where):
    """sgm_job for a consumer of the cloud job (submit_fuse, the dense= dict of submit_scenes, the occlusion= dict of
    submit_ar) whose own lr_check sits beside sgm: the two checks are different rules, so lr_check together with sgm
    raises ValueError; `where` names the place for the message ("dense", "occlusion", "submit_fuse")."""
    params, check = sgm_job(sgm)
    if params is not None and lr_check:
        raise ValueError(f"{where}: lr_check is the cross-check of the winner-takes-all search; with sgm the cross-check is "
                         f"the lr_check key of the sgm dict, e.g. sgm=dict(hip_lib.SGM_DEFAULTS, lr_check=1.0)")
    return params, check


def disparity_size(cam, width, height, style, check=None):
    """svo_disparity_size (host only): (cols, rows, planes, image_bytes) of one slot of a disparity job with `style`;
    check: a StereoCheck (svo_disparity_size_checked), or None."""
    cols, rows, planes, nbytes = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    if check is None:
        _check(lib().svo_disparity_size(C.byref(cam), int(width), int(height), C.byref(style), C.byref(cols),
                                        C.byref(rows), C.byref(planes), C.byref(nbytes)))
    else:
        _check(lib().svo_disparity_size_checked(C.byref(cam), int(width), int(height), C.byref(style), C.byref(check),
                                                C.byref(cols), C.byref(rows), C.byref(planes), C.byref(nbytes)))
    return cols.value, rows.value, planes.value, nbytes.value


# dense point clouds (svo_submit_export_cloud, include/svo_hip.h): the frame, the layout, a segment (one per named
# slot); the records are MAP_POINT_DTYPE
CLOUD_WORLD, CLOUD_CAMERA = 0, 1
CLOUD_FRAMES = ("world", "camera")
CLOUD_COMPACT, CLOUD_ORGANIZED = 0, 1
CLOUD_LAYOUTS = ("compact", "organized")
CLOUD_OK, CLOUD_NONE = 0, 1
CLOUD_DROPPED = 0x80
CLOUD_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("keyframe_id", "<i4"),
                                ("status", "<i4"), ("n_points", "<i4"), ("first_point", "<i8"), ("pose", "<f4", (6,)),
                                ("time_stamp", "<f4"), ("baseline", "<f4")])
assert CLOUD_SEGMENT_DTYPE.itemsize == 64


class CloudStyle(C.Structure):
    """svo_cloud_style (include/svo_hip.h): what one cloud job computes."""
    _fields_ = [("step", C.c_int32), ("win", C.c_int32), ("search_x", C.c_int32), ("search_y", C.c_int32),
                ("frame", C.c_int32), ("layout", C.c_int32), ("min_disparity", C.c_float), ("max_depth", C.c_float),
                ("max_mean_cost", C.c_float), ("_reserved", C.c_int32 * 3)]


class CloudSegment(C.Structure):
    """svo_cloud_segment (include/svo_hip.h); CLOUD_SEGMENT_DTYPE is the same layout for numpy."""
    _fields_ = [("seq", C.c_int32), ("run", C.c_int32), ("frame_id", C.c_int32), ("keyframe_id", C.c_int32),
                ("status", C.c_int32), ("n_points", C.c_int32), ("first_point", C.c_int64), ("pose", C.c_float * 6),
                ("time_stamp", C.c_float), ("baseline", C.c_float)]


class CloudDst(C.Structure):
    """svo_cloud_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("points", C.c_void_p), ("capacity", C.c_int64)]


class CloudSrc(C.Structure):
    """svo_cloud_src (include/svo_hip.h): one image pair of svo_cloud_points."""
    _fields_ = [("left", Image), ("right", Image), ("baseline", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("pose", C.c_float * 6), ("_reserved", C.c_int32)]


assert (C.sizeof(CloudStyle), C.sizeof(CloudSegment), C.sizeof(CloudDst), C.sizeof(CloudSrc)) == (48, 64, 24, 96)


def cloud_style(step=1, win=0, search_x=0, search_y=0, frame=CLOUD_WORLD, layout=CLOUD_COMPACT, min_disparity=0.0,
                max_depth=0.0, max_mean_cost=0.0):
    """a CloudStyle; frame and layout may be names (CLOUD_FRAMES, CLOUD_LAYOUTS); win / search_x / search_y of 0: the
    ctx's settings; a filter value of 0: off"""
    if isinstance(frame, str):
        frame = CLOUD_FRAMES.index(frame)
    if isinstance(layout, str):
        layout = CLOUD_LAYOUTS.index(layout)
    return CloudStyle(int(step), int(win), int(search_x), int(search_y), int(frame), int(layout), float(min_disparity),
                      float(max_depth), float(max_mean_cost))


def cloud_size(cam, width, height, style):
    """svo_cloud_size (host only): (cols, rows, points_per_slot) of one slot of a cloud job with `style`."""
    cols, rows, points = C.c_int(0), C.c_int(0), C.c_int64(0)
    _check(lib().svo_cloud_size(C.byref(cam), int(width), int(height), C.byref(style), C.byref(cols), C.byref(rows),
                                C.byref(points)))
    return cols.value, rows.value, points.value


# scenes (svo_submit_export_scenes, include/svo_hip.h): what is shown, the classes of the key, a line of the stage
# entry, a segment (one per named slot)
SCENE_POINTS, SCENE_TRAJECTORY, SCENE_KEYFRAMES, SCENE_POSE = 1, 2, 4, 8
SCENE_ALL = 15
SCENE_CLASS_POSE, SCENE_CLASS_KEYFRAME, SCENE_CLASS_TRAJECTORY, SCENE_CLASS_POINT = range(4)
SCENE_OK, SCENE_NONE = 0, 1
SCENE_LINE_DTYPE = np.dtype([("a", "<f4", (3,)), ("b", "<f4", (3,)), ("cls_rgb", "<u4"), ("_pad", "<u4")])
SCENE_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("status", "<u2"),
                                ("n_keyframes", "<u2"), ("from_keyframe", "<i4"), ("n_keypoints", "<i4"),
                                ("n_poses", "<i4"), ("time_stamp", "<f4"), ("offset", "<i8"), ("pose", "<f4", (6,))])
assert (SCENE_LINE_DTYPE.itemsize, SCENE_SEGMENT_DTYPE.itemsize) == (32, 64)
# the viewer's camera presets (src/qt-viewer/PointCloudViewer.qml:19-39, 95-96): (eye, centre, up), 45 degrees, 0.1
SCENE_FRONT = ((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0))
SCENE_TOP = ((0.0, -5.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
SCENE_SIDE = ((-5.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0))
SCENE_PRESETS = dict(front=SCENE_FRONT, top=SCENE_TOP, side=SCENE_SIDE)
SCENE_FOV_Y, SCENE_NEAR = 45.0, 0.1


class SceneCamera(C.Structure):
    """svo_scene_camera (include/svo_hip.h): the rows of the 3x4 world -> camera matrix, f, cx, cy, near."""
    _fields_ = [("view", C.c_float * 12), ("f", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("near", C.c_float)]


class SceneStyle(C.Structure):
    """svo_scene_style (include/svo_hip.h): what one scene job draws; colours are r << 16 | g << 8 | b."""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("pixel", C.c_int32), ("point_size", C.c_int32),
                ("background", C.c_uint32), ("trajectory_rgb", C.c_uint32), ("keyframe_rgb", C.c_uint32),
                ("pose_rgb", C.c_uint32), ("frustum_w", C.c_float), ("frustum_h", C.c_float), ("frustum_d", C.c_float),
                ("show", C.c_uint32), ("from_keyframe", C.c_int32), ("trajectory_tail", C.c_int32),
                ("filter", MapFilter), ("_reserved", C.c_int32)]


class SceneDst(C.Structure):
    """svo_scene_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("pixels", C.c_void_p), ("capacity", C.c_int64)]


class SceneSrc(C.Structure):
    """svo_scene_src (include/svo_hip.h): one image of svo_render_scene."""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("n_sets", C.c_int32), ("n_lines", C.c_int32),
                ("sets", C.c_void_p), ("own_id", C.c_void_p), ("lines", C.c_void_p)]


assert (C.sizeof(SceneCamera), C.sizeof(SceneStyle)) == (64, 76)


def scene_style(cols=256, rows=256, pixel=PIXEL_RGB8, point_size=3, background=0xffffff, trajectory_rgb=0xff0000,
                keyframe_rgb=0x0000ff, pose_rgb=0x00ff00, frustum=(0.1, 0.08, 0.07), show=SCENE_ALL, from_keyframe=0,
                trajectory_tail=0, filter=None):
    """a SceneStyle; the defaults are the viewer's (white, red trajectory, blue keyframes, a green current pose, its
    frustum). pixel may be a name (PIXELS); filter: None, a MapFilter or a dict of its fields"""
    if isinstance(pixel, str):
        pixel = PIXELS.index(pixel)
    return SceneStyle(int(cols), int(rows), int(pixel), int(point_size), int(background), int(trajectory_rgb),
                      int(keyframe_rgb), int(pose_rgb), float(frustum[0]), float(frustum[1]), float(frustum[2]),
                      int(show), int(from_keyframe), int(trajectory_tail), map_filter(filter), 0)


def scene_size(style):
    """svo_scene_size (host only): (pitch, image_bytes) of one image of a scene job with `style`."""
    pitch, nbytes = C.c_int64(0), C.c_int64(0)
    _check(lib().svo_scene_size(C.byref(style), C.byref(pitch), C.byref(nbytes)))
    return pitch.value, nbytes.value


def scene_look_at(eye, centre, up, fov_y_deg=SCENE_FOV_Y, cols=256, rows=256, near=SCENE_NEAR):
    """svo_scene_look_at (host only): the SceneCamera at `eye` looking at `centre` for a cols x rows image."""
    v3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    out = SceneCamera()
    _check(lib().svo_scene_look_at(v3(eye), v3(centre), v3(up), float(fov_y_deg), int(cols), int(rows), float(near),
                                   C.byref(out)))
    return out


def scene_preset(name, cols=256, rows=256):
    """the viewer's "front", "top" or "side" camera for a cols x rows image"""
    return scene_look_at(*SCENE_PRESETS[name], SCENE_FOV_Y, cols, rows, SCENE_NEAR)


def scene_frustum(pose, dims=(0.1, 0.08, 0.07)):
    """svo_scene_frustum (host only): float32 [8, 6], the world lines (a, b) of the frustum of `pose`."""
    out = np.zeros((8, 6), np.float32)
    _check(lib().svo_scene_frustum((C.c_float * 6)(*[float(x) for x in pose]), (C.c_float * 3)(*[float(x) for x in dims]),
                                   out.ctypes.data_as(C.c_void_p)))
    return out


# scene clouds (svo_submit_export_scenes_clouds, include/svo_hip.h): dense clouds drawn in the scene picture
SCENE_CLASS_CLOUD = 4
SCENE_CLOUD_INFO_DTYPE = np.dtype([("status", "<i4"), ("keyframe_id", "<i4"), ("live_points", "<i4"), ("_pad", "<i4"),
                                   ("extra_points", "<i8"), ("_pad2", "<i8")])


class SceneSpan(C.Structure):
    """svo_scene_span (include/svo_hip.h): n svo_map_point records in device memory."""
    _fields_ = [("points", C.c_void_p), ("n", C.c_int64)]


class SceneCloudInfo(C.Structure):
    """svo_scene_cloud_info (include/svo_hip.h); SCENE_CLOUD_INFO_DTYPE is the same layout for numpy."""
    _fields_ = [("status", C.c_int32), ("keyframe_id", C.c_int32), ("live_points", C.c_int32), ("_pad", C.c_int32),
                ("extra_points", C.c_int64), ("_pad2", C.c_int64)]


class SceneClouds(C.Structure):
    """svo_scene_clouds (include/svo_hip.h): the live layer and the extra spans of a scene job. sgm (Python only): None,
    or the SgmParams the job goes through svo_submit_export_scenes_clouds_sgm with; `check` is then the SGM map's own."""
    sgm = None
    _fields_ = [("live", C.c_int32), ("what", C.c_int32), ("cloud", CloudStyle), ("check", StereoCheck),
                ("point_size", C.c_int32), ("_reserved", C.c_int32 * 3), ("extra", C.c_void_p), ("info", C.c_void_p)]


assert (C.sizeof(SceneSpan), C.sizeof(SceneCloudInfo), C.sizeof(SceneClouds), SCENE_CLOUD_INFO_DTYPE.itemsize) == (16, 32, 120, 32)


def scene_span(records):
    """a SceneSpan of `records`: None, a device tensor holding MAP_POINT_DTYPE records, or (address, n)"""
    if records is None:
        return SceneSpan(None, 0)
    if isinstance(records, torch.Tensor):
        n = records.numel() * records.element_size() // MAP_POINT_DTYPE.itemsize
        return SceneSpan(records.data_ptr() if n else None, n)
    ptr, n = records
    return SceneSpan(int(ptr) if ptr else None, int(n))


def scene_clouds(live=False, what=0, step=1, win=0, search_x=0, search_y=0, min_disparity=0.0, max_depth=0.0,
                 max_mean_cost=0.0, lr_check=0.0, point_size=1, extra=None, info=None, sgm=None):
    """a SceneClouds and what it points to, as (clouds, keep): keep the second alive until the job is delivered.
    live: draw the dense cloud of `what` (0: frames, 1: newest keyframes) of every named slot, searched with step, win,
    search_x, search_y (0: the ctx's), filtered by min_disparity, max_depth, max_mean_cost (0: off) and, with
    lr_check > 0, by the left-right check at that tolerance. extra: None, or per named slot what scene_span takes.
    info: None, or a numpy array of SCENE_CLOUD_INFO_DTYPE, one per named slot. sgm: what sgm_job takes: the live layer
    is the cloud of the SGM map (clouds.sgm holds the params, clouds.check the SGM map's own check, the lr_check key of
    the sgm dict; lr_check beside sgm: ValueError)."""
    lr_check = float(lr_check or 0.0)
    sgm, sgm_check = sgm_consumer(sgm, lr_check, "dense")
    check = stereo_check(lr_check > 0, lr_check) if live else StereoCheck()
    if sgm is not None and live:
        check = sgm_check if sgm_check is not None else StereoCheck()
    spans = None
    if extra is not None:
        spans = (SceneSpan * max(len(extra), 1))(*[scene_span(e) for e in extra])
    c = SceneClouds(int(bool(live)), int(what), cloud_style(step, win, search_x, search_y, CLOUD_WORLD, CLOUD_COMPACT,
                                                           min_disparity, max_depth, max_mean_cost),
                    check, int(point_size), (C.c_int32 * 3)(), C.cast(spans, C.c_void_p) if spans is not None else None,
                    info.ctypes.data if info is not None else None)
    c.sgm = sgm
    return c, (spans, extra, info)


# voxel maps (include/svo_hip.h): svo_map_point records fused into a sparse voxel grid in device memory
VOXEL_LOG2_MIN, VOXEL_LOG2_MAX = 6, 26


class VoxelParams(C.Structure):
    """svo_voxel_params (include/svo_hip.h): what a map is cleared with."""
    _fields_ = [("voxel", C.c_float), ("log2_capacity", C.c_int32), ("drop_flags", C.c_uint32), ("_reserved", C.c_int32)]


class VoxelMap(C.Structure):
    """svo_voxel_map (include/svo_hip.h): a map in device memory and its params."""
    _fields_ = [("data", C.c_void_p), ("params", VoxelParams)]


class VoxelSpan(C.Structure):
    """svo_voxel_span (include/svo_hip.h): n records for map `map` of a call, fused with `stamp`."""
    _fields_ = [("points", C.c_void_p), ("n", C.c_int64), ("map", C.c_int32), ("stamp", C.c_uint32)]


class VoxelMapInfo(C.Structure):
    """svo_voxel_map_info (include/svo_hip.h): the params and counters of a map's header."""
    _fields_ = [("voxel", C.c_float), ("log2_capacity", C.c_int32), ("drop_flags", C.c_uint32), ("_pad", C.c_int32),
                ("n_voxels", C.c_int64), ("n_fused", C.c_int64), ("n_outside", C.c_int64), ("overflow", C.c_int64)]


class VoxelFilter(C.Structure):
    """svo_voxel_filter (include/svo_hip.h): which entries an extraction keeps."""
    _fields_ = [("min_count", C.c_uint32), ("min_stamp", C.c_uint32), ("_reserved", C.c_int32 * 2)]


assert (C.sizeof(VoxelParams), C.sizeof(VoxelMap), C.sizeof(VoxelSpan), C.sizeof(VoxelMapInfo), C.sizeof(VoxelFilter)) == (16, 24, 24, 48, 16)


class VoxelKeep(C.Structure):
    """svo_voxel_keep (include/svo_hip.h, "voxel prune"): which entries a prune keeps."""
    _fields_ = [("min_count", C.c_uint32), ("min_stamp", C.c_uint32), ("center", C.c_float * 3), ("radius", C.c_int32),
                ("_reserved", C.c_int32 * 2)]


class VoxelPruneResult(C.Structure):
    """svo_voxel_prune_result (include/svo_hip.h)."""
    _fields_ = [("n_before", C.c_int64), ("n_kept", C.c_int64), ("center_voxel", C.c_int32 * 3), ("_pad", C.c_int32)]


assert (C.sizeof(VoxelKeep), C.sizeof(VoxelPruneResult)) == (32, 32)


class VoxelCarve(C.Structure):
    """svo_voxel_carve_rule (include/svo_hip.h, "voxel carve"): the guards of a carve."""
    _fields_ = [("margin", C.c_float), ("near", C.c_float), ("max_last", C.c_uint32), ("drop_flags", C.c_uint32), ("ring", C.c_int32),
                ("_reserved", C.c_int32 * 3)]


class VoxelCarveResult(C.Structure):
    """svo_voxel_carve_result (include/svo_hip.h)."""
    _fields_ = [("n_before", C.c_int64), ("n_kept", C.c_int64), ("n_tested", C.c_int64), ("n_carved", C.c_int64)]


assert (C.sizeof(VoxelCarve), C.sizeof(VoxelCarveResult)) == (32, 32)

# svo_voxel_entry (include/svo_hip.h, "voxel entries"): a raw entry of a map; acc = count, sx, sy, sz, sr, sg, sb, last
VOXEL_ENTRY_DTYPE = np.dtype([("key", "<u8"), ("acc", "<u4", (8,))])


class VoxelEntrySpan(C.Structure):
    """svo_voxel_entry_span (include/svo_hip.h): n entry records for map `map` of a call, keys made with `voxel`."""
    _fields_ = [("entries", C.c_void_p), ("n", C.c_int64), ("map", C.c_int32), ("voxel", C.c_float)]


class VoxelMergeResult(C.Structure):
    """svo_voxel_merge_result (include/svo_hip.h): what a merge did to one map."""
    _fields_ = [("n_offered", C.c_int64), ("n_merged", C.c_int64), ("n_skipped", C.c_int64), ("n_claimed", C.c_int64)]


assert (VOXEL_ENTRY_DTYPE.itemsize, C.sizeof(VoxelEntrySpan), C.sizeof(VoxelMergeResult)) == (40, 24, 32)
# the ctx's save and load jobs: svo_submit_save_voxel_maps (the export's regions and segments), svo_submit_load_voxel_maps
VOXEL_LOAD_REPLACE, VOXEL_LOAD_MERGE = 0, 1
VOXEL_LOADED, VOXEL_LOAD_NO_MAP, VOXEL_LOAD_FULL = 0, 1, 2
VOXEL_ENTRY_SPAN_DTYPE = np.dtype([("entries", "<u8"), ("n", "<i8"), ("map", "<i4"), ("voxel", "<f4")])
VOXEL_LOAD_INFO_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("status", "<i4"), ("_pad", "<i4"), ("n_offered", "<i8"), ("n_merged", "<i8"),
                                  ("n_skipped", "<i8"), ("n_claimed", "<i8"), ("n_voxels", "<i8"), ("_pad2", "<i8")])


class VoxelEntryDst(C.Structure):
    """svo_voxel_entry_dst (include/svo_hip.h)"""
    _fields_ = [("segments", C.c_void_p), ("entries", C.c_void_p)]


assert (VOXEL_ENTRY_SPAN_DTYPE.itemsize, VOXEL_LOAD_INFO_DTYPE.itemsize, C.sizeof(VoxelEntryDst)) == (24, 64, 16)
# the ctx's carve job: svo_submit_carve_voxel_maps (the centre modes are the prune job's)
CARVE_OK, CARVE_NO_MAP, CARVE_NO_POSE, CARVE_TOO_LARGE, CARVE_NONE = range(5)
CARVE_INFO_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("status", "<i4"), ("n_before", "<i8"), ("n_kept", "<i8"),
                             ("n_tested", "<i4"), ("n_carved", "<i4"), ("pose", "<f4", (6,))])
assert CARVE_INFO_DTYPE.itemsize == 64
# the ctx's prune job: svo_submit_prune_voxel_maps
PRUNE_OK, PRUNE_NO_MAP, PRUNE_NO_POSE, PRUNE_TOO_LARGE = range(4)
PRUNE_CENTER_GIVEN, PRUNE_CENTER_POSE = 0, 1
PRUNE_INFO_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("status", "<i4"), ("n_before", "<i8"), ("n_kept", "<i8"),
                             ("center", "<f4", (3,)), ("center_voxel", "<i4", (3,)), ("_pad", "<i4", (2,))])
assert PRUNE_INFO_DTYPE.itemsize == 64


# the ctx's voxel maps: svo_submit_fuse_clouds, svo_submit_export_voxel_maps
FUSE_OK, FUSE_NONE, FUSE_NO_MAP, FUSE_FULL = range(4)
VOXEL_OK, VOXEL_NO_MAP, VOXEL_TOO_SMALL = range(3)
FUSE_INFO_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("keyframe_id", "<i4"), ("status", "<i4"),
                            ("n_offered", "<i4"), ("n_fused", "<i4"), ("n_outside", "<i4"), ("n_voxels", "<i8"), ("pose", "<f4", (6,))])
VOXEL_REGION_DTYPE = np.dtype([("first_point", "<i8"), ("point_capacity", "<i8"), ("min_stamp", "<u4"), ("_reserved", "<i4", (3,))])
VOXEL_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("status", "<i4"), ("first_point", "<i8"),
                                ("n_points", "<i8"), ("n_voxels", "<i8"), ("n_fused", "<i8"), ("voxel", "<f4"),
                                ("log2_capacity", "<i4"), ("_pad", "<i8")])


class VoxelDst(C.Structure):
    """svo_voxel_dst (include/svo_hip.h)"""
    _fields_ = [("segments", C.c_void_p), ("points", C.c_void_p)]


assert (FUSE_INFO_DTYPE.itemsize, VOXEL_REGION_DTYPE.itemsize, VOXEL_SEGMENT_DTYPE.itemsize, C.sizeof(VoxelDst)) == (64, 32, 64, 16)


def voxel_map_bytes(log2_capacity):
    """svo_voxel_map_bytes: the device bytes of a map of 1 << log2_capacity entries (needs no GPU)"""
    n = lib().svo_voxel_map_bytes(int(log2_capacity))
    if n <= 0:
        raise SvoError(f"log2_capacity {log2_capacity} is outside {VOXEL_LOG2_MIN} .. {VOXEL_LOG2_MAX}")
    return n


def voxel_params(voxel, log2_capacity, drop_flags=0):
    return VoxelParams(float(voxel), int(log2_capacity), int(drop_flags), 0)


def voxel_keep(min_count=0, min_stamp=0, center=(0.0, 0.0, 0.0), radius=-1):
    """a VoxelKeep: count >= max(1, min_count), last >= min_stamp and, with radius >= 0 (in voxels), the box of
    2 radius + 1 voxels per axis around the voxel that holds `center`"""
    return VoxelKeep(int(min_count), int(min_stamp), (C.c_float * 3)(*[float(c) for c in center]), int(radius), (C.c_int32 * 2)(0, 0))


def voxel_carve(margin, near=0.01, ring=1, max_last=0xFFFFFFFF, drop_flags=0):
    """a VoxelCarve: an entry is carved when the occluder measures a surface more than `margin` behind it along its
    ray; entries nearer than `near` or fused after stamp `max_last` are kept; ring = 1 asks the entry's lattice cell
    and its neighbours, ring = 0 the cell alone"""
    return VoxelCarve(float(margin), float(near), int(max_last), int(drop_flags), int(ring), (C.c_int32 * 3)(0, 0, 0))


def _voxel_map(m):
    """a VoxelMap of (device tensor or address, VoxelParams)"""
    data, params = m
    return VoxelMap(data.data_ptr() if isinstance(data, torch.Tensor) else int(data), params)


# ar pictures (svo_submit_export_ar, include/svo_hip.h): lit meshes over each slot's camera image
AR_OK, AR_NONE = 0, 1
AR_MAX_TRIANGLES = 65536
AR_SEGMENT_DTYPE = np.dtype([("seq", "<i4"), ("run", "<i4"), ("frame_id", "<i4"), ("status", "<u2"), ("_pad", "<u2"),
                             ("n_instances", "<i4"), ("n_triangles", "<i4"), ("time_stamp", "<f4"), ("_pad2", "<i4"),
                             ("offset", "<i8"), ("pose", "<f4", (6,))])
assert AR_SEGMENT_DTYPE.itemsize == 64
# the demo (src/ar-app/): near plane 0.01, a directional light along +z, the object half a metre in front of the
# first camera (AnimatedEntity.qml:56). The demo's light has no ambient term of its own (Qt3D's phong default adds
# a small one); 0.25 is this binding's choice, so that a face turned away from the light keeps a visible colour.
AR_NEAR, AR_LIGHT, AR_AMBIENT, AR_AT = 0.01, (0.0, 0.0, 1.0), 0.25, (0.0, 0.0, 0.5)


class ArCamera(C.Structure):
    """svo_ar_camera (include/svo_hip.h): the rows of the 3x4 world -> camera matrix, fx, fy, cx, cy."""
    _fields_ = [("view", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class ArMesh(C.Structure):
    """svo_ar_mesh (include/svo_hip.h): host arrays of one mesh."""
    _fields_ = [("vertices", C.c_void_p), ("triangles", C.c_void_p), ("rgb", C.c_void_p), ("n_vertices", C.c_int32),
                ("n_triangles", C.c_int32), ("_reserved", C.c_int64)]


class ArInstance(C.Structure):
    """svo_ar_instance (include/svo_hip.h): a mesh placed in the world."""
    _fields_ = [("model", C.c_float * 12), ("mesh", C.c_int32), ("rgb", C.c_uint32), ("_reserved", C.c_int32 * 2)]


class ArStyle(C.Structure):
    """svo_ar_style (include/svo_hip.h)."""
    _fields_ = [("pixel", C.c_int32), ("light", C.c_float * 3), ("ambient", C.c_float), ("near", C.c_float),
                ("_reserved", C.c_int32 * 2)]


class ArDst(C.Structure):
    """svo_ar_dst (include/svo_hip.h)."""
    _fields_ = [("segments", C.c_void_p), ("pixels", C.c_void_p), ("capacity", C.c_int64)]


class ArDraw(C.Structure):
    """svo_ar_draw (include/svo_hip.h): an instanced mesh in device memory, of svo_render_ar."""
    _fields_ = [("model", C.c_float * 12), ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("rgb", C.c_void_p),
                ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("rgb_all", C.c_uint32), ("_reserved", C.c_int32)]


class ArSrc(C.Structure):
    """svo_ar_src (include/svo_hip.h): one image of svo_render_ar."""
    _fields_ = [("image", Image), ("draws", C.c_void_p), ("n_draws", C.c_int32), ("_reserved", C.c_int32)]


assert (C.sizeof(ArCamera), C.sizeof(ArMesh), C.sizeof(ArInstance), C.sizeof(ArStyle), C.sizeof(ArDraw)) == (64, 40, 64, 32, 88)


def ar_style(pixel=PIXEL_RGB8, light=AR_LIGHT, ambient=AR_AMBIENT, near=AR_NEAR):
    """an ArStyle; the defaults are the demo's near plane (0.01) and light (0, 0, 1), and ambient = 0.25 (this
    binding's choice: the demo states none). pixel may be a name (PIXELS)"""
    if isinstance(pixel, str):
        pixel = PIXELS.index(pixel)
    return ArStyle(int(pixel), (C.c_float * 3)(*[float(x) for x in light]), float(ambient), float(near))


def ar_size(cam, width, height, style):
    """svo_ar_size (host only): (pitch, image_bytes) of one image of an ar job in a ctx of these settings."""
    pitch, nbytes = C.c_int64(0), C.c_int64(0)
    _check(lib().svo_ar_size(C.byref(cam), int(width), int(height), C.byref(style), C.byref(pitch), C.byref(nbytes)))
    return pitch.value, nbytes.value


def ar_camera_of_pose(pose, cam):
    """svo_ar_camera_of_pose (host only): the ArCamera of a slot at `pose` (t, r) with the intrinsics of `cam`."""
    out = ArCamera()
    _check(lib().svo_ar_camera_of_pose((C.c_float * 6)(*[float(x) for x in pose]), C.byref(cam), C.byref(out)))
    return out


def ar_model(at=(0.0, 0.0, 0.0), scale=1.0, rot=None):
    """float32 [12]: the rows of the 3x4 mesh -> world matrix `scale * rot` (rot: 3x3, default identity) then + at"""
    m = np.zeros((3, 4), np.float32)
    m[:, :3] = (np.eye(3) if rot is None else np.asarray(rot, np.float64)) * float(scale)
    m[:, 3] = at
    return m.ravel()


def ar_box(size=1.0):
    """the stock object: an axis-aligned cube of edge `size` about the origin as (vertices float32 [8, 3], triangles
    int32 [12, 3]), two triangles a face"""
    h = 0.5 * float(size)
    v = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], np.float32)
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5],
                  [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, t


def ar_instance(model, mesh=0, rgb=0xc08040):
    """an ArInstance of mesh index `mesh` at `model` (12 floats, ar_model) with colour r << 16 | g << 8 | b"""
    return ArInstance((C.c_float * 12)(*[float(x) for x in np.asarray(model).ravel()]), int(mesh), int(rgb))


# ar occlusion (svo_submit_export_ar_occluded, include/svo_hip.h): meshes hidden behind the dense stereo depth
AR_HIDDEN_DROP, AR_HIDDEN_DIM = 0, 1
AR_HIDDEN = ("drop", "dim")
AR_VISIBILITY_DTYPE = np.dtype([("status", "<i4"), ("occluder_points", "<i4"), ("covered", "<i8"), ("hidden", "<i8"),
                                ("_pad", "<i8")])


class ArOcclusion(C.Structure):
    """svo_ar_occlusion (include/svo_hip.h): how an ar job hides its meshes behind the slots' dense stereo depth. sgm
    (Python only): None, or the SgmParams the job goes through svo_submit_export_ar_occluded_sgm with; `check` is then
    the SGM map's own."""
    sgm = None
    _fields_ = [("on", C.c_int32), ("hidden", C.c_int32), ("alpha", C.c_int32), ("margin", C.c_float),
                ("drop_flags", C.c_uint32), ("_reserved", C.c_int32 * 3), ("cloud", CloudStyle), ("check", StereoCheck),
                ("info", C.c_void_p), ("_reserved2", C.c_int64)]


class ArOccluder(C.Structure):
    """svo_ar_occluder (include/svo_hip.h): the organized lattice of one image of svo_render_ar_occluded."""
    _fields_ = [("records", C.c_void_p), ("cols", C.c_int32), ("rows", C.c_int32), ("step", C.c_int32),
                ("_reserved", C.c_int32)]


assert (C.sizeof(ArOcclusion), C.sizeof(ArOccluder), AR_VISIBILITY_DTYPE.itemsize) == (128, 24, 32)


def ar_occlusion(on=True, step=4, hidden=AR_HIDDEN_DROP, alpha=128, margin=0.0, drop_flags=0, win=0, search_x=0, search_y=0,
                 min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0, lr_check=0.0, info=None, sgm=None):
    """an ArOcclusion. hidden may be a name (AR_HIDDEN); step, win, search_x, search_y, min_disparity, max_depth,
    max_mean_cost: the cloud that occludes (cloud_style; 0: the ctx's settings / off); lr_check > 0: the left-right
    check at that tolerance; info: None, or a numpy array of AR_VISIBILITY_DTYPE, one per named slot, that must stay
    alive until the job is delivered. sgm: what sgm_job takes: the occluder is the cloud of the SGM map (the result's
    sgm holds the params, its check the SGM map's own check, the lr_check key of the sgm dict; lr_check beside sgm:
    ValueError)."""
    if isinstance(hidden, str):
        hidden = AR_HIDDEN.index(hidden)
    lr_check = float(lr_check or 0.0)
    sgm, sgm_check = sgm_consumer(sgm, lr_check, "occlusion")
    check = stereo_check(lr_check > 0, lr_check)
    if sgm is not None:
        check = sgm_check if sgm_check is not None else StereoCheck()
    o = ArOcclusion(int(bool(on)), int(hidden), int(alpha), float(margin), int(drop_flags), (C.c_int32 * 3)(),
                    cloud_style(step, win, search_x, search_y, CLOUD_CAMERA, CLOUD_COMPACT, min_disparity, max_depth,
                                max_mean_cost),
                    check, info.ctypes.data if info is not None else None, 0)
    o.sgm = sgm
    return o


def ar_occluder(records, cols=0, rows=0, step=1):
    """an ArOccluder of `records`: None (the image has none), a device tensor holding cols * rows MAP_POINT_DTYPE
    records, or a raw device address"""
    if records is None:
        return ArOccluder(None, 0, 0, 0, 0)
    ptr = records.data_ptr() if isinstance(records, torch.Tensor) else int(records)
    return ArOccluder(ptr, int(cols), int(rows), int(step), 0)


class SnapshotInfo(C.Structure):
    """struct svo_snapshot_info (include/svo_hip.h): the header of a snapshot's host part."""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("byte_order", C.c_uint32), ("status", C.c_uint32),
                ("host_bytes", C.c_int64), ("data_bytes", C.c_int64), ("cam", CameraSettings)] + \
               [(n, C.c_int32) for n in
                ("width", "height", "capacity", "pyramid_levels", "lk_levels", "frame_id", "n_keypoints",
                 "n_trajectory", "n_keyframes", "keyframes_retired", "n_image_sets", "n_planes", "_reserved")]


    @property
    def first_keyframe(self):
        """the oldest keyframe in the snapshot: the ones below were trimmed (the C field of that name)"""
        return self._reserved


assert C.sizeof(SnapshotInfo) == 160


class KeyframeRange(C.Structure):
    """svo_keyframe_range (include/svo_hip.h): keyframes [first, count) of a slot are resident, those below `retired`
    are final; `table`: resident keyframes a slot can hold."""
    _fields_ = [(n, C.c_int32) for n in ("first", "retired", "count", "table")]

    def __repr__(self):
        return f"KeyframeRange(first={self.first}, retired={self.retired}, count={self.count}, table={self.table})"


assert C.sizeof(KeyframeRange) == 16
SNAPSHOT_COMPLETE, SNAPSHOT_TOO_SMALL = 0, 1


class SnapshotBuffers(C.Structure):
    """svo_snapshot (include/svo_hip.h): the two buffers of one snapshot."""
    _fields_ = [("host", C.c_void_p), ("host_capacity", C.c_int64), ("data", C.c_void_p), ("data_capacity", C.c_int64)]


class CopySegment(C.Structure):
    """svo_copy_segment (include/svo_hip.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64), ("rows", C.c_int64),
                ("src_pitch", C.c_int64), ("dst_pitch", C.c_int64)]


# svo_pose_sample (include/svo_types.h): one StereoSlam::update_pose call of svo_submit_pose_updates
POSE_SAMPLE_DTYPE = np.dtype([("pose", "<f4", (6,)), ("speed", "<f4", (6,)), ("pose_var", "<f4", (6,)),
                              ("speed_var", "<f4", (6,)), ("dt", "<f8"), ("flags", "<u4"), ("_pad", "<u4")])
assert POSE_SAMPLE_DTYPE.itemsize == 112
POSE_SAMPLE_CHAIN = 1
# svo_pose_filter_batch: floats of a filter state going in (statePost | errorCovPost) and coming out
# (statePre | statePost | errorCovPre | errorCovPost | gain)
POSE_FILTER_IN_FLOATS, POSE_FILTER_OUT_FLOATS = 156, 456


def lib():
    """Load libsvo_hip.so; fail loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SvoError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _LIB = C.CDLL(LIB_PATH)
        _LIB.svo_last_error.restype = C.c_char_p
        _LIB.svo_voxel_map_bytes.restype = C.c_int64
        for name in ("svo_submit_fuse_clouds", "svo_fuse_clouds"):
            getattr(_LIB, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        # (the SGM forms of the cloud's consumers; an older diagnostic build may lack them, as below)
        p, i = C.c_void_p, C.c_int
        for names, argtypes in ((("svo_submit_fuse_clouds_sgm", "svo_fuse_clouds_sgm"), [p, i, p, i, p, p, p, C.c_uint32, p]),
                                (("svo_submit_export_scenes_clouds_sgm", "svo_export_scenes_clouds_sgm"), [p, p, i, p, p, p, p, p, i]),
                                (("svo_submit_export_ar_occluded_sgm", "svo_export_ar_occluded_sgm"), [p, p, i, p, p, p, p, i, p, p, i, p, i])):
            for name in names:
                if hasattr(_LIB, name):
                    getattr(_LIB, name).argtypes = argtypes
        for name in ("svo_submit_export_voxel_maps", "svo_export_voxel_maps"):     # (regions: a numpy array's address)
            getattr(_LIB, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _LIB.svo_ctx_set_voxel_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        # (centers, info: a numpy array's address. An older diagnostic build named by SVO_HIP_LIB may lack the entries:
        # calling one then fails by name, as every missing entry does)
        for name in ("svo_submit_prune_voxel_maps", "svo_prune_voxel_maps"):
            if hasattr(_LIB, name):
                getattr(_LIB, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(_LIB, "svo_voxel_prune"):
            _LIB.svo_voxel_prune.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("svo_submit_carve_voxel_maps", "svo_carve_voxel_maps"):
            if hasattr(_LIB, name):
                getattr(_LIB, name).argtypes = [p, p, i, p, p, p, p, p, i, p, p]
        if hasattr(_LIB, "svo_voxel_carve"):
            _LIB.svo_voxel_carve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name, argtypes in (("svo_voxel_pack", [p, p, p, p, C.c_int64, p]), ("svo_voxel_merge", [p, i, p, i, p, p]),
                               ("svo_voxel_rehash", [p, p, p, i]), ("svo_submit_save_voxel_maps", [p, p, i, p, p, p, i]),
                               ("svo_save_voxel_maps", [p, p, i, p, p, p, i]), ("svo_submit_load_voxel_maps", [p, p, i, p, i, i, p]),
                               ("svo_load_voxel_maps", [p, p, i, p, i, i, p]), ("svo_ctx_resize_voxel_maps", [p, p, i, i])):
            if hasattr(_LIB, name):
                getattr(_LIB, name).argtypes = argtypes
        _LIB.svo_submit_clear_voxel_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _LIB.svo_get_voxel_map_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for name in ("svo_submit_pose_updates", "svo_update_poses"):
            getattr(_LIB, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _LIB.svo_scene_look_at.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_float,
                                           C.c_void_p]
        _LIB.svo_pose_filter_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    return _LIB


def _check(rc):
    if rc != 0:
        raise SvoError(f"libsvo_hip error {rc}: {lib().svo_last_error().decode()}")


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device, contiguous tensors only"
    return C.c_void_p(t.data_ptr())


def _img(t):
    assert t.dtype == torch.uint8 and t.dim() == 2 and t.is_cuda and t.stride(1) == 1
    return Image(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0))


def detect_shape(width, height, n_levels, grid_width, grid_height):
    """svo_detect_shape (host only): (max_cells, cell_width, cell_height, list_capacity) of the detection
    launch for levels that halve from width x height."""
    out = [C.c_int(0) for _ in range(4)]
    _check(lib().svo_detect_shape(width, height, n_levels, grid_width, grid_height, *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def klt_cache_layout(win):
    """svo_klt_cache_layout (host only): (record_bytes, header_offset, header_bytes, levels) of a keyframe's KLT
    template cache for window `win`."""
    rec, off, hb, lv = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
    _check(lib().svo_klt_cache_layout(int(win), C.byref(rec), C.byref(off), C.byref(hb), C.byref(lv)))
    return rec.value, off.value, hb.value, lv.value


def keyframe_launch_info(cap, max_cells, tmpl_cap):
    """svo_keyframe_launch_info (host only): (threads of the compaction launch for sets of `cap`, threads of the
    select + merge launch for `max_cells`, bytes of "stored" flags of a template cache of tmpl_cap keypoints)"""
    a, b, v = C.c_int(0), C.c_int(0), C.c_int64(0)
    _check(lib().svo_keyframe_launch_info(int(cap), int(max_cells), int(tmpl_cap), C.byref(a), C.byref(b), C.byref(v)))
    return a.value, b.value, v.value


def keyframe_record_layout():
    """svo_keyframe_record_layout (host only): dict of a keyframe table record's size (`bytes`) and the offsets of
    n, pose, tmpl, tmpl_valid, tmpl_cap, tmpl_win and `planes` (name -> offset of that plane's pointer)"""
    names = ("bytes", "n", "pose", "tmpl", "tmpl_valid", "tmpl_cap", "tmpl_win")
    out = [C.c_int64(0) for _ in names]
    planes = (C.c_int64 * 12)()
    _check(lib().svo_keyframe_record_layout(*[C.byref(o) for o in out], planes))
    d = {k: o.value for k, o in zip(names, out)}
    d["planes"] = dict(zip(KPS_PLANES[:12], planes))
    return d


def pose_mats_layout():
    """svo_pose_mats_layout (host only): dict of the size (`bytes`) of the block of rotation matrices that the
    alignment kernel leaves for the KLT launch, and of its members name -> (offset, numpy dtype, count): Rd, R, Ri, t"""
    out = [C.c_int64(0) for _ in range(5)]
    _check(lib().svo_pose_mats_layout(*[C.byref(o) for o in out]))
    size, rd, r, ri, t = (o.value for o in out)
    return dict(bytes=size, Rd=(rd, np.float64, 9), R=(r, np.float32, 9), Ri=(ri, np.float32, 9), t=(t, np.float32, 3))


def rectify_inverse(cal):
    """svo_rectify_inverse (host only): ir[9] of the calibration, the inverse of P R in the arithmetic of the maps;
    SvoError for a calibration the library rejects."""
    ir = (C.c_double * 9)()
    _check(lib().svo_rectify_inverse(C.byref(cal), ir))
    return np.array(ir, np.float64)


def export_capacity(cam, width, height):
    """svo_export_capacity (host only): the records one slot of an export can take at most."""
    out = C.c_int(0)
    _check(lib().svo_export_capacity(C.byref(cam), int(width), int(height), C.byref(out)))
    return out.value


def snapshot_info(host_part):
    """svo_snapshot_info (host only): checks the host part of a snapshot (bytes-like) and returns its header;
    SvoError for a bad one."""
    buf = bytes(host_part)
    out = SnapshotInfo()
    _check(lib().svo_snapshot_info(buf, len(buf), C.byref(out)))
    return out


def input_format_info(fmt, width):
    """svo_input_format_info (host only): the InputLayout of input format `fmt` for images of `width` pixels."""
    out = InputLayout()
    _check(lib().svo_input_format_info(int(fmt), int(width), C.byref(out)))
    return out


def _raw_img(t, channels):
    """a uint8 device buffer [H, W] (one byte per pixel) or [H, W, 3] (interleaved) as an svo_image: width and
    height in pixels, stride in bytes"""
    assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == (3 if channels == 3 else 2) and t.stride(-1) == 1
    if channels == 3:
        assert t.shape[2] == 3 and t.stride(1) == 3
    return Image(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0))


def _imgs(ts, n=None):
    arr = (Image * max(n or len(ts), 1))()
    for i, t in enumerate(ts):
        arr[i] = _img(t)
    return arr


class Handle:
    """svo_handle: one per (GPU, caller)."""

    def __init__(self, device=0, max_keypoints=4096):
        if not torch.cuda.is_available():
            raise SvoError("no GPU visible: libsvo_hip has no CPU fallback")
        self.device = torch.device("cuda", device)
        self._h = C.c_void_p()
        _check(lib().svo_handle_create(device, max_keypoints, C.byref(self._h)))
        self.use_current_stream()

    def use_current_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().svo_handle_set_stream(self._h, C.c_void_p(s)))

    def synchronize(self):
        _check(lib().svo_handle_synchronize(self._h))

    def set_fast_solver(self, on=True):
        """svo_handle_set_fast_solver: off (default) = the reference's row-by-row normal equations +
        SVD pseudo-inverse; on = tree sums + LDL^T."""
        _check(lib().svo_handle_set_fast_solver(self._h, int(on)))

    def set_exact_pinv(self, on=True):
        self.set_fast_solver(not on)

    def close(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.svo_handle_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- P1 ---------------------------------------------------------------
    def build_pyramid(self, img, n_levels):
        """createImgPyramid (src/lib/stereo_slam.cpp:112-121): list of uint8 device tensors."""
        levels = [img]
        h, w = img.shape
        for _ in range(1, n_levels):
            h //= 2
            w //= 2
            levels.append(torch.empty((h, w), dtype=torch.uint8, device=img.device))
        arr = _imgs(levels)
        _check(lib().svo_build_pyramid(self._h, n_levels, arr))
        return levels

    # -- F2 ---------------------------------------------------------------
    def detect_keypoints(self, levels, grid_width, grid_height, max_cells=None):
        """CornerDetector::detect_keypoints on every level (uint8 device tensors or views with unit column
        stride; level l uses the cell (grid_width >> l) x (grid_height >> l)). Returns (cells, counts):
        cells [n_levels, max_cells] device bytes viewed as DET_CELL_DTYPE by detect_to_numpy, counts [n_levels]
        int32 device."""
        n = len(levels)
        if max_cells is None:
            max_cells = max([1] + [(t.shape[1] // max(grid_width >> l, 1)) * (t.shape[0] // max(grid_height >> l, 1))
                                   for l, t in enumerate(levels)])
        dev = levels[0].device
        cells = torch.zeros((n, max_cells, DET_CELL_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
        _check(lib().svo_detect_keypoints(self._h, n, _imgs(levels), grid_width, grid_height, max_cells,
                                          _ptr(cells), _ptr(counts)))
        return cells, counts

    # -- R ----------------------------------------------------------------
    def remap_linear(self, srcs, map_x, map_y):
        """cv::remap(src, dst, map_x, map_y, INTER_LINEAR), constant 0 border (src/app/euroc_input.cpp:69-70)
        of every uint8 device image in `srcs` through one map (float32 [H, W] device tensors): a list of
        uint8 [H, W] device tensors, bit-exact to OpenCV's fixed-point remap."""
        assert map_x.shape == map_y.shape and map_x.dim() == 2
        assert map_x.dtype == torch.float32 and map_y.dtype == torch.float32
        h, w = map_x.shape
        map_x, map_y = map_x.contiguous(), map_y.contiguous()
        outs = [torch.empty((h, w), dtype=torch.uint8, device=map_x.device) for _ in srcs]
        _check(lib().svo_remap_linear(self._h, len(srcs), _imgs(srcs), _imgs(outs), _ptr(map_x), _ptr(map_y)))
        return outs

    def remap_linear_multi(self, srcs, maps_x, maps_y, map_of_image):
        """svo_remap_linear_multi: image i of `srcs` through map map_of_image[i] of maps_x / maps_y (lists of float32
        [H, W] device tensors of one size), in any order; a list of uint8 [H, W] device tensors. The arithmetic is
        remap_linear's."""
        assert len(maps_x) == len(maps_y) and len(map_of_image) == len(srcs)
        maps_x = [m.contiguous() for m in maps_x]
        maps_y = [m.contiguous() for m in maps_y]
        h, w = maps_x[0].shape
        for m in maps_x + maps_y:
            assert m.dtype == torch.float32 and tuple(m.shape) == (h, w) and m.is_cuda
        outs = [torch.empty((h, w), dtype=torch.uint8, device=maps_x[0].device) for _ in srcs]
        n_maps = len(maps_x)
        px = (C.c_void_p * n_maps)(*[m.data_ptr() for m in maps_x])
        py = (C.c_void_p * n_maps)(*[m.data_ptr() for m in maps_y])
        idx = (C.c_int * max(len(srcs), 1))(*[int(i) for i in map_of_image])
        _check(lib().svo_remap_linear_multi(self._h, len(srcs), _imgs(srcs), _imgs(outs), n_maps, px, py, idx))
        return outs

    # -- M ----------------------------------------------------------------
    def build_rectify_maps(self, cals, width, height, out=None):
        """svo_build_rectify_maps: cv::initUndistortRectifyMap (src/app/euroc_input.cpp:48-49) of every
        CameraCalibration in `cals` in one launch: a list of (map_x, map_y) float32 [height, width] device tensors
        (out: such a list to write into)."""
        n = len(cals)
        if out is None:
            out = [tuple(torch.empty((height, width), dtype=torch.float32, device=self.device) for _ in range(2))
                   for _ in range(n)]
        for mx, my in out:
            for m in (mx, my):
                assert m.dtype == torch.float32 and tuple(m.shape) == (height, width) and m.is_cuda and m.is_contiguous()
        arr = (CameraCalibration * max(n, 1))(*cals)
        px = (C.c_void_p * max(n, 1))(*[m[0].data_ptr() for m in out])
        py = (C.c_void_p * max(n, 1))(*[m[1].data_ptr() for m in out])
        _check(lib().svo_build_rectify_maps(self._h, n, arr, int(width), int(height), px, py))
        return out

    # -- I ----------------------------------------------------------------
    def convert_frames(self, fmt, src_a, src_b, width=None, lefts=None, rights=None):
        """svo_convert_frames: the buffers src_a[i] (and src_b[i] for the pair formats, else None) of input format
        `fmt` (uint8 device tensors, [H, W'] or [H, W', 3], unit stride inside a row) into gray images: two lists
        (left, right) of uint8 [H, width] device tensors (made here unless lefts / rights are given). width: of the
        images (default: of the buffer, halved for the side-by-side formats)."""
        info = input_format_info(fmt, 1)
        if width is None:
            width = src_a[0].shape[1] // info.min_row_pixels
        n, hgt = len(src_a), src_a[0].shape[0]
        if lefts is None:
            lefts = [torch.empty((hgt, width), dtype=torch.uint8, device=src_a[0].device) for _ in range(n)]
            rights = [torch.empty((hgt, width), dtype=torch.uint8, device=src_a[0].device) for _ in range(n)]
        arr_a = (Image * n)(*[_raw_img(t, info.channels) for t in src_a])
        arr_b = (Image * n)(*[_raw_img(t, info.channels) for t in src_b]) if info.buffers == 2 else None
        _check(lib().svo_convert_frames(self._h, int(fmt), n, arr_a, arr_b, _imgs(lefts), _imgs(rights)))
        return lefts, rights

    # -- export -----------------------------------------------------------
    def pack_keypoints(self, sets, first, kps2d=None, kps3d=None, info=None):
        """svo_pack_keypoints: SoA keypoint sets into AoS records. sets: a list of (n, {field of svo_keypoints:
        device tensor or raw device address}); first[i]: the record set i starts at; kps2d / kps3d / info: device
        tensors that receive the records (None: skipped)."""
        arr = (Keypoints * max(len(sets), 1))()
        for i, (n, fields) in enumerate(sets):
            arr[i].n = int(n)
            for name, v in fields.items():
                setattr(arr[i], name, v.data_ptr() if isinstance(v, torch.Tensor) else int(v))
        firsts = (C.c_int64 * max(len(sets), 1))(*[int(f) for f in first])
        _check(lib().svo_pack_keypoints(self._h, len(sets), arr, firsts, _ptr(kps2d), _ptr(kps3d), _ptr(info)))

    def pack_map_points(self, regions, first, filter=None, points=None, counts=None):
        """svo_pack_map_points: the keypoints of SoA sets that pass `filter` (map_filter's forms) as dense 16-byte
        points. regions: per region a list of (n, own keyframe id, {field of svo_keypoints: device tensor or raw
        device address}) sets; first[r]: the record region r starts at; points: uint8 [records, 16] device tensor
        or None (counts only); counts: int32 [sets] device tensor (the kept points of every set, in call order) or
        None. Complete on return."""
        sets = [s for r in regions for s in r]
        arr = (Keypoints * max(len(sets), 1))()
        for i, (n, _, fields) in enumerate(sets):
            arr[i].n = int(n)
            for name, v in fields.items():
                setattr(arr[i], name, v.data_ptr() if isinstance(v, torch.Tensor) else int(v))
        begin = (C.c_int32 * (len(regions) + 1))(*np.cumsum([0] + [len(r) for r in regions]).tolist())
        own = (C.c_int32 * max(len(sets), 1))(*[int(s[1]) for s in sets])
        firsts = (C.c_int64 * max(len(regions), 1))(*[int(f) for f in first])
        _check(lib().svo_pack_map_points(self._h, len(regions), begin, arr, own, firsts, C.byref(map_filter(filter)),
                                         _ptr(points), _ptr(counts)))

    def render_views(self, srcs, offsets, style, pixels):
        """svo_render_views: gray planes as images of `style` (a ViewStyle) with a marker per keypoint. srcs: per
        image ((data address or uint8 device tensor [H, W]), width, height, stride) and (n, {field of svo_keypoints:
        device tensor or raw device address}) or None; offsets[i]: the byte of `pixels` (a uint8 device tensor, or a
        raw device address) image i starts at. Complete on return."""
        arr = (ViewSrc * max(len(srcs), 1))()
        for i, (img, kps) in enumerate(srcs):
            data, w, h, stride = img
            arr[i].image = Image(data.data_ptr() if isinstance(data, torch.Tensor) else int(data), int(w), int(h), int(stride))
            if kps is not None:
                arr[i].kps.n = int(kps[0])
                for name, v in kps[1].items():
                    setattr(arr[i].kps, name, v.data_ptr() if isinstance(v, torch.Tensor) else int(v))
        offs = (C.c_int64 * max(len(srcs), 1))(*[int(o) for o in offsets])
        p = pixels.data_ptr() if isinstance(pixels, torch.Tensor) else int(pixels)
        _check(lib().svo_render_views(self._h, len(srcs), arr, offs, C.byref(style), C.c_void_p(p)))

    def pack_dense(self, srcs, offsets):
        """the argument arrays of dense_disparity, built once (keeps Python out of a timed loop)"""
        arr = (DenseSrc * max(len(srcs), 1))()
        for i, (left, right, baseline) in enumerate(srcs):
            for name, (data, w, h, stride) in (("left", left), ("right", right)):
                setattr(arr[i], name, Image(data.data_ptr() if isinstance(data, torch.Tensor) else int(data), int(w), int(h), int(stride)))
            arr[i].baseline = float(baseline)
        return len(srcs), arr, (C.c_int64 * max(len(srcs), 1))(*[int(o) for o in offsets]), srcs

    def dense_disparity_packed(self, packed, style, values, check=None):
        p = values.data_ptr() if isinstance(values, torch.Tensor) else int(values)
        if check is None:
            _check(lib().svo_dense_disparity(self._h, packed[0], packed[1], packed[2], C.byref(style), C.c_void_p(p)))
        else:
            _check(lib().svo_dense_disparity_checked(self._h, packed[0], packed[1], packed[2], C.byref(style),
                                                     C.byref(check), C.c_void_p(p)))

    def dense_disparity(self, srcs, offsets, style, values, check=None):
        """svo_dense_disparity: dense disparity or depth planes of `style` (a DisparityStyle with win, search_x and
        search_y given). srcs: per image pair (left, right, baseline) with left / right ((data address or uint8
        device tensor [H, W]), width, height, stride); offsets[i]: the byte of `values` (a float32 device tensor, or
        a raw device address) the planes of pair i start at. check: a StereoCheck (svo_dense_disparity_checked: the
        lr plane follows the others), or None. Complete on return."""
        self.dense_disparity_packed(self.pack_dense(srcs, offsets), style, values, check)

    def dense_cost_volume(self, srcs, style, cost_cap, volume_offsets, count_offsets, volumes):
        """svo_dense_cost_volume: the uint16 cost volume [rows, cols, search_x + 1] and count plane [rows, cols] of every
        pair of srcs (as in dense_disparity) at the bytes volume_offsets[i] / count_offsets[i] of `volumes` (a uint16
        or int16 device tensor, or a raw device address). Complete on return."""
        n, arr, _, _ = self.pack_dense(srcs, volume_offsets)
        vo = (C.c_int64 * max(n, 1))(*[int(o) for o in volume_offsets])
        co = (C.c_int64 * max(n, 1))(*[int(o) for o in count_offsets])
        p = volumes.data_ptr() if isinstance(volumes, torch.Tensor) else int(volumes)
        _check(lib().svo_dense_cost_volume(self._h, n, arr, C.byref(style), int(cost_cap), vo, co, C.c_void_p(p)))

    def sgm_aggregate(self, shapes, volumes, counts, value, cost, sgm, offsets, values):
        """svo_sgm_aggregate: the four paths and the value rule over the caller's volumes. shapes: per volume (cols,
        rows, D, baseline); volumes: per volume a device tensor or raw device address of uint16 [rows, cols, D];
        counts: None, or per volume a device tensor / address of uint16 [rows, cols] or None; value: DENSE_*; cost:
        the second plane; sgm: an SgmParams; offsets[i]: the byte of `values` (a float32 device tensor or raw device
        address) the planes of volume i start at. Complete on return."""
        n = len(shapes)
        addr = lambda v: 0 if v is None else (v.data_ptr() if isinstance(v, torch.Tensor) else int(v))
        sh = (SgmShape * max(n, 1))(*[SgmShape(int(c), int(r), int(d), float(b)) for c, r, d, b in shapes])
        vols = (C.c_void_p * max(n, 1))(*[addr(v) for v in volumes])
        cnts = None if counts is None else (C.c_void_p * max(n, 1))(*[addr(v) for v in counts])
        offs = (C.c_int64 * max(n, 1))(*[int(o) for o in offsets])
        _check(lib().svo_sgm_aggregate(self._h, n, sh, vols, cnts, int(value), int(bool(cost)), C.byref(sgm), offs,
                                       C.c_void_p(addr(values))))

    def dense_disparity_sgm_packed(self, packed, style, sgm, values, check=None):
        p = values.data_ptr() if isinstance(values, torch.Tensor) else int(values)
        if check is None:
            _check(lib().svo_dense_disparity_sgm(self._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(sgm), C.c_void_p(p)))
        else:
            _check(lib().svo_dense_disparity_sgm_checked(self._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(sgm),
                                                         C.byref(check), C.c_void_p(p)))

    def dense_disparity_sgm(self, srcs, offsets, style, sgm, values, check=None):
        """svo_dense_disparity_sgm: dense_disparity with semi-global aggregation and sub-pixel values (sgm: an
        SgmParams; style.search_x <= 63). check: a StereoCheck (svo_dense_disparity_sgm_checked: the cross-check of
        the SGM map, the lr plane appended), or None. Complete on return."""
        self.dense_disparity_sgm_packed(self.pack_dense(srcs, offsets), style, sgm, values, check)

    def pack_cloud(self, srcs, first):
        """the argument arrays of cloud_points, built once (keeps Python out of a timed loop)"""
        arr = (CloudSrc * max(len(srcs), 1))()
        for i, (left, right, rig, pose) in enumerate(srcs):
            for name, (data, w, h, stride) in (("left", left), ("right", right)):
                setattr(arr[i], name, Image(data.data_ptr() if isinstance(data, torch.Tensor) else int(data), int(w), int(h), int(stride)))
            for k in ("baseline", "fx", "fy", "cx", "cy"):
                setattr(arr[i], k, float(rig[k]))
            arr[i].pose = (C.c_float * 6)(*[float(v) for v in pose])
        return len(srcs), arr, (C.c_int64 * max(len(srcs), 1))(*[int(o) for o in first]), srcs

    def cloud_points_packed(self, packed, style, points, counts=None, check=None):
        p = points.data_ptr() if isinstance(points, torch.Tensor) else int(points)
        c = None if counts is None else C.c_void_p(counts.data_ptr() if isinstance(counts, torch.Tensor) else int(counts))
        if check is None:
            _check(lib().svo_cloud_points(self._h, packed[0], packed[1], packed[2], C.byref(style), C.c_void_p(p), c))
        else:
            _check(lib().svo_cloud_points_checked(self._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(check),
                                                  C.c_void_p(p), c))

    def cloud_points(self, srcs, first, style, points, counts=None, check=None):
        """svo_cloud_points: the coloured 3-D points of `style` (a CloudStyle with win, search_x and search_y given).
        srcs: per image pair (left, right, rig, pose) with left / right ((data address or uint8 device tensor [H, W]),
        width, height, stride), rig a mapping with baseline, fx, fy, cx, cy and pose six floats; first[i]: the record
        of `points` (a device tensor of 16-byte records, or a raw device address) the records of pair i start at;
        counts: an int32 device tensor [n] (or address) for the kept counts, or None. check: a StereoCheck
        (svo_cloud_points_checked: failing points are dropped), or None. Complete on return."""
        self.cloud_points_packed(self.pack_cloud(srcs, first), style, points, counts, check)

    def cloud_points_sgm_packed(self, packed, style, sgm, points, counts=None, check=None):
        p = points.data_ptr() if isinstance(points, torch.Tensor) else int(points)
        c = None if counts is None else C.c_void_p(counts.data_ptr() if isinstance(counts, torch.Tensor) else int(counts))
        _check(lib().svo_cloud_points_sgm(self._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(sgm),
                                          None if check is None else C.byref(check), C.c_void_p(p), c))

    def cloud_points_sgm(self, srcs, first, style, sgm, points, counts=None, check=None):
        """svo_cloud_points_sgm: cloud_points over SGM maps (sgm: an SgmParams; style.search_x <= 63; max_mean_cost
        bounds the aggregated cost over its four paths). check: a StereoCheck with a tolerance (the cross-check of the
        SGM map: failing points are dropped), or None. Complete on return."""
        self.cloud_points_sgm_packed(self.pack_cloud(srcs, first), style, sgm, points, counts, check)

    # -- voxel maps ---------------------------------------------------------
    def voxel_new(self, params, device="cuda"):
        """a cleared map of `params` (a VoxelParams) in a device tensor of its own, as the (tensor, params) pair the
        other voxel_* methods take"""
        data = torch.empty(voxel_map_bytes(params.log2_capacity), dtype=torch.uint8, device=device)
        self.voxel_clear((data, params))
        return data, params

    def voxel_clear(self, m):
        """svo_voxel_clear: m = (uint8 device tensor or address of svo_voxel_map_bytes bytes, VoxelParams)"""
        vm = _voxel_map(m)
        _check(lib().svo_voxel_clear(self._h, C.c_void_p(vm.data), C.byref(vm.params)))

    def voxel_fuse(self, spans, maps):
        """svo_voxel_fuse: spans = [(records, map index, stamp)] with records a device tensor of 16-byte
        MAP_POINT_DTYPE records, (address, n) or None; maps = [(tensor or address, VoxelParams)]. One launch; raises
        (SVO_ERR_CAPACITY, nothing written) when a load bound fails. Complete on return."""
        arr = (VoxelSpan * max(len(spans), 1))()
        for i, (records, mi, stamp) in enumerate(spans):
            sp = scene_span(records)
            arr[i] = VoxelSpan(sp.points, sp.n, int(mi), int(stamp))
        marr = (VoxelMap * max(len(maps), 1))(*[_voxel_map(m) for m in maps])
        _check(lib().svo_voxel_fuse(self._h, len(spans), arr, len(maps), marr))

    def voxel_info(self, m):
        """svo_voxel_info: the header of a map as a dict (voxel, log2_capacity, drop_flags, n_voxels, n_fused,
        n_outside, overflow). m: (tensor or address, params), a tensor or an address."""
        data = m[0] if isinstance(m, tuple) else m
        info = VoxelMapInfo()
        _check(lib().svo_voxel_info(self._h, C.c_void_p(data.data_ptr() if isinstance(data, torch.Tensor) else int(data)), C.byref(info)))
        return {n: getattr(info, n) for n, _ in VoxelMapInfo._fields_ if n != "_pad"}

    def voxel_count(self, m, min_count=0, min_stamp=0):
        """svo_voxel_extract with points == NULL: how many entries the filter keeps"""
        n = C.c_int64(-1)
        _check(lib().svo_voxel_extract(self._h, C.byref(_voxel_map(m)), C.byref(VoxelFilter(int(min_count), int(min_stamp))), None,
                                       C.c_int64(0), C.byref(n)))
        return n.value

    def voxel_extract(self, m, min_count=0, min_stamp=0, points=None, capacity=None):
        """svo_voxel_extract: the kept entries in ascending key order as MAP_POINT_DTYPE records. points: a device
        tensor (or address, with `capacity` records) that receives them, or None: one of exactly the kept count is
        made. Returns (points, n)."""
        if points is None:
            capacity = self.voxel_count(m, min_count, min_stamp)
            points = torch.empty((max(capacity, 1), 16), dtype=torch.uint8, device="cuda")
        elif capacity is None:
            capacity = points.numel() * points.element_size() // MAP_POINT_DTYPE.itemsize
        n = C.c_int64(-1)
        p = points.data_ptr() if isinstance(points, torch.Tensor) else int(points)
        _check(lib().svo_voxel_extract(self._h, C.byref(_voxel_map(m)), C.byref(VoxelFilter(int(min_count), int(min_stamp))),
                                       C.c_void_p(p), C.c_int64(int(capacity)), C.byref(n)))
        return points, n.value

    def voxel_prune(self, m, keep):
        """svo_voxel_prune: the map reduced in place to the entries `keep` (a VoxelKeep, see voxel_keep) names. Returns
        a dict: n_before, n_kept, center_voxel. Complete on return."""
        out = VoxelPruneResult()
        _check(lib().svo_voxel_prune(self._h, C.byref(_voxel_map(m)), C.byref(keep) if keep is not None else None, C.byref(out)))
        return {"n_before": out.n_before, "n_kept": out.n_kept, "center_voxel": tuple(out.center_voxel)}

    def voxel_carve(self, m, camera, width, height, occluder, carve, keep=None):
        """svo_voxel_carve: the map reduced in place to the entries that `keep` (a VoxelKeep, or None: all) keeps and
        that the occluder does not contradict. camera: an ArCamera; occluder: an ArOccluder, or what ar_occluder takes
        as a tuple (None: no evidence, a plain prune); carve: a VoxelCarve (see voxel_carve). Returns a dict: n_before,
        n_kept, n_tested, n_carved. Complete on return."""
        occ = occluder if isinstance(occluder, ArOccluder) else ar_occluder(*(occluder if isinstance(occluder, (tuple, list)) else (occluder,)))
        out = VoxelCarveResult()
        _check(lib().svo_voxel_carve(self._h, C.byref(_voxel_map(m)), C.byref(camera) if camera is not None else None, int(width), int(height),
                                     C.byref(occ), C.byref(carve) if carve is not None else None,
                                     C.byref(keep) if keep is not None else None, C.byref(out)))
        return {n: getattr(out, n) for n, _ in VoxelCarveResult._fields_}

    def voxel_pack(self, m, min_count=0, min_stamp=0, entries=None, capacity=None):
        """svo_voxel_pack: the kept entries in ascending key order as VOXEL_ENTRY_DTYPE records, accumulators verbatim.
        entries: a device tensor (or address, with `capacity` records) that receives them, or None: a uint8 tensor
        [kept, 40] of exactly the kept count is made. Returns (entries, n)."""
        vm, f = _voxel_map(m), VoxelFilter(int(min_count), int(min_stamp))
        n = C.c_int64(-1)
        if entries is None:
            _check(lib().svo_voxel_pack(self._h, C.byref(vm), C.byref(f), None, C.c_int64(0), C.byref(n)))
            capacity = n.value
            entries = torch.empty((max(capacity, 1), VOXEL_ENTRY_DTYPE.itemsize), dtype=torch.uint8, device="cuda")[:capacity]
        elif capacity is None:
            capacity = entries.numel() * entries.element_size() // VOXEL_ENTRY_DTYPE.itemsize
        p = entries.data_ptr() if isinstance(entries, torch.Tensor) else int(entries)
        _check(lib().svo_voxel_pack(self._h, C.byref(vm), C.byref(f), C.c_void_p(p), C.c_int64(int(capacity)), C.byref(n)))
        return entries, n.value

    def voxel_merge(self, spans, maps):
        """svo_voxel_merge: spans = [(entries, map index, voxel)] with entries a device tensor of 40-byte
        VOXEL_ENTRY_DTYPE records, (address, n) or None, and voxel the edge their keys were made with; maps = [(tensor
        or address, VoxelParams)]. One launch; raises (SVO_ERR_CAPACITY, nothing written) when a load bound fails.
        Returns per map a dict: n_offered, n_merged, n_skipped, n_claimed. Complete on return."""
        arr = (VoxelEntrySpan * max(len(spans), 1))()
        for i, (entries, mi, voxel) in enumerate(spans):
            if entries is None:
                ptr, n = None, 0
            elif isinstance(entries, torch.Tensor):
                n = entries.numel() * entries.element_size() // VOXEL_ENTRY_DTYPE.itemsize
                ptr = entries.data_ptr() if n else None
            else:
                ptr, n = entries
            arr[i] = VoxelEntrySpan(int(ptr) if ptr else None, int(n), int(mi), float(voxel))
        marr = (VoxelMap * max(len(maps), 1))(*[_voxel_map(m) for m in maps])
        res = (VoxelMergeResult * max(len(maps), 1))()
        _check(lib().svo_voxel_merge(self._h, len(spans), arr, len(maps), marr, res))
        return [{n: getattr(res[i], n) for n, _ in VoxelMergeResult._fields_} for i in range(len(maps))]

    def voxel_rehash(self, m, log2_capacity):
        """svo_voxel_rehash: the entries, n_voxels and cumulative counters of map m in a new map of 1 << log2_capacity
        entries with the same voxel and drop_flags, in a device tensor of its own; m is only read. Raises
        (SVO_ERR_CAPACITY) when the entries exceed the new load limit. Returns the (tensor, params) pair."""
        vm = _voxel_map(m)
        nbytes = voxel_map_bytes(log2_capacity)
        device = m[0].device if isinstance(m[0], torch.Tensor) else "cuda"
        data = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _check(lib().svo_voxel_rehash(self._h, C.byref(vm), C.c_void_p(data.data_ptr()), int(log2_capacity)))
        return data, VoxelParams(vm.params.voxel, int(log2_capacity), vm.params.drop_flags, 0)

    def render_scene(self, srcs, cameras, offsets, style, pixels):
        """svo_render_scene: the viewer's scene of keyframe sets and lines as images of `style` (a SceneStyle). srcs:
        per image (cols, rows, sets, lines) with sets a list of (n, own_id, {field of svo_keypoints: device tensor or
        raw device address}) and lines a device tensor holding SCENE_LINE_DTYPE records (16-byte aligned) or None;
        cameras: a SceneCamera per image; offsets[i]: the byte of `pixels` (a uint8 device tensor, or a raw device
        address) image i starts at. Complete on return."""
        self.render_scene_packed(self.pack_scene(srcs, cameras, offsets), style, pixels)

    def pack_scene(self, srcs, cameras, offsets):
        """the argument arrays of render_scene, built once (keeps Python out of a timed call); pass the result to
        render_scene_packed. The device tensors of `srcs` must stay alive."""
        n = len(srcs)
        arr = (SceneSrc * max(n, 1))()
        cams = (SceneCamera * max(n, 1))(*cameras)
        keep = []
        for i, (cols, rows, sets, lines) in enumerate(srcs):
            ks = (Keypoints * max(len(sets), 1))()
            own = (C.c_int32 * max(len(sets), 1))()
            for j, (m, own_id, planes) in enumerate(sets):
                ks[j].n, own[j] = int(m), int(own_id)
                for name, v in planes.items():
                    setattr(ks[j], name, v.data_ptr() if isinstance(v, torch.Tensor) else int(v))
            keep += [ks, own]
            n_lines = 0 if lines is None else lines.numel() * lines.element_size() // SCENE_LINE_DTYPE.itemsize
            arr[i] = SceneSrc(int(cols), int(rows), len(sets), n_lines, C.cast(ks, C.c_void_p), C.cast(own, C.c_void_p),
                              lines.data_ptr() if n_lines else None)
        offs = (C.c_int64 * max(n, 1))(*[int(o) for o in offsets])
        return n, arr, cams, offs, keep

    def render_scene_packed(self, packed, style, pixels):
        """svo_render_scene of the arrays of pack_scene"""
        n, arr, cams, offs, _ = packed
        p = pixels.data_ptr() if isinstance(pixels, torch.Tensor) else int(pixels)
        _check(lib().svo_render_scene(self._h, n, arr, cams, offs, C.byref(style), C.c_void_p(p)))

    def render_scene_clouds(self, srcs, spans, cameras, offsets, style, point_size, pixels):
        """svo_render_scene_clouds: render_scene with cloud points. spans: per image a list of what scene_span takes
        (device tensors of MAP_POINT_DTYPE records, or (address, n)); point_size: the cloud points' square."""
        packed = self.pack_scene(srcs, cameras, offsets)
        self.render_scene_clouds_packed(packed, self.pack_scene_spans(spans), style, point_size, pixels)

    def pack_scene_spans(self, spans):
        """the span arrays of render_scene_clouds, built once; the device tensors must stay alive"""
        flat = [scene_span(e) for per_image in spans for e in per_image]
        arr = (SceneSpan * max(len(flat), 1))(*flat)
        counts = (C.c_int32 * max(len(spans), 1))(*[len(per_image) for per_image in spans])
        return arr, counts, spans

    def render_scene_clouds_packed(self, packed, packed_spans, style, point_size, pixels):
        """svo_render_scene_clouds of the arrays of pack_scene and pack_scene_spans"""
        n, arr, cams, offs, _ = packed
        p = pixels.data_ptr() if isinstance(pixels, torch.Tensor) else int(pixels)
        _check(lib().svo_render_scene_clouds(self._h, n, arr, packed_spans[0], packed_spans[1], cams, offs, C.byref(style),
                                             C.c_int32(int(point_size)), C.c_void_p(p)))

    def render_ar(self, srcs, cameras, offsets, style, pixels, occluders=None, occlusion=None):
        """svo_render_ar: lit meshes over gray planes as images of `style` (an ArStyle). srcs: per image
        ((data address or uint8 device tensor, width, height, stride), draws) with draws a list of (model of 12
        floats, vertices float32 device tensor [V, 3], triangles int32 device tensor [T, 3], rgb uint32 / int32 device
        tensor [T] or None, the instance's colour); cameras: an ArCamera per image; offsets[i]: the byte of `pixels`
        (a uint8 device tensor, or a raw device address) image i starts at. Complete on return.
        With occlusion (an ArOcclusion; only its scalar fields are read) the call is svo_render_ar_occluded: occluders
        is one ArOccluder, or what ar_occluder takes as a tuple, per image, and the visibility of every image is
        returned (AR_VISIBILITY_DTYPE [n]); without it None is returned."""
        return self.render_ar_packed(self.pack_ar(srcs, cameras, offsets), style, pixels, occluders, occlusion)

    def pack_ar(self, srcs, cameras, offsets):
        """the argument arrays of render_ar, built once (keeps Python out of a timed call); pass the result to
        render_ar_packed. The device tensors of `srcs` must stay alive."""
        n = len(srcs)
        arr = (ArSrc * max(n, 1))()
        cams = (ArCamera * max(n, 1))(*cameras)
        keep = []
        for i, (img, draws) in enumerate(srcs):
            data, w, h, stride = img
            ds = (ArDraw * max(len(draws), 1))()
            for j, (model, vertices, triangles, rgb, rgb_all) in enumerate(draws):
                ds[j] = ArDraw((C.c_float * 12)(*[float(x) for x in np.asarray(model).ravel()]), vertices.data_ptr(),
                               triangles.data_ptr(), None if rgb is None else rgb.data_ptr(), vertices.numel() // 3,
                               triangles.numel() // 3, int(rgb_all), 0)
            keep.append(ds)
            arr[i] = ArSrc(Image(data.data_ptr() if isinstance(data, torch.Tensor) else int(data), int(w), int(h), int(stride)),
                           C.cast(ds, C.c_void_p), len(draws), 0)
        offs = (C.c_int64 * max(n, 1))(*[int(o) for o in offsets])
        return n, arr, cams, offs, keep

    def pack_ar_occluders(self, occluders):
        """the occluder array of render_ar_packed, built once; the device tensors must stay alive"""
        occ = [o if isinstance(o, ArOccluder) else ar_occluder(*(o if isinstance(o, (tuple, list)) else (o,)))
               for o in occluders]
        return (ArOccluder * max(len(occ), 1))(*occ)

    def render_ar_packed(self, packed, style, pixels, occluders=None, occlusion=None):
        """svo_render_ar of the arrays of pack_ar; with occlusion svo_render_ar_occluded (occluders: as in render_ar,
        or the array of pack_ar_occluders), which returns the visibilities"""
        n, arr, cams, offs, _ = packed
        p = pixels.data_ptr() if isinstance(pixels, torch.Tensor) else int(pixels)
        if occlusion is None:
            _check(lib().svo_render_ar(self._h, n, arr, cams, offs, C.byref(style), C.c_void_p(p)))
            return None
        if occluders is not None and not isinstance(occluders, C.Array):
            occluders = self.pack_ar_occluders(occluders)
        vis = np.zeros(max(n, 1), AR_VISIBILITY_DTYPE)
        _check(lib().svo_render_ar_occluded(self._h, n, arr, cams, offs, C.byref(style), C.byref(occlusion), occluders,
                                            C.c_void_p(p), C.c_void_p(vis.ctypes.data)))
        return vis[:n]

    def copy_segments(self, segs):
        """svo_copy_segments: 2-D byte segments, device to device. segs: (src address, dst address, row_bytes,
        rows, src_pitch, dst_pitch) each. Complete on return."""
        arr = (CopySegment * max(len(segs), 1))(*[CopySegment(*[int(x) for x in g]) for g in segs])
        _check(lib().svo_copy_segments(self._h, len(segs), arr))

    # -- pose filter --------------------------------------------------------
    def pose_filter_batch(self, state_in, start_pose, first, samples, state_out, filtered=None):
        """svo_pose_filter_batch: the 12-state pose filter of len(state_in) states in one launch. Device tensors:
        state_in float32 [B, 156] (statePost | errorCovPost), start_pose float32 [B, 6], first int32 [B + 1]
        (sample offsets), samples uint8 [total, 112] (POSE_SAMPLE_DTYPE records), state_out float32 [B, 456]
        (statePre | statePost | errorCovPre | errorCovPost | gain; written for states with samples only), filtered
        float32 [total, 6] or None."""
        b, total = state_in.shape[0], samples.shape[0]
        assert state_in.shape == (b, POSE_FILTER_IN_FLOATS) and state_out.shape == (b, POSE_FILTER_OUT_FLOATS)
        assert start_pose.shape == (b, 6) and first.shape == (b + 1,) and first.dtype == torch.int32
        assert samples.dtype == torch.uint8 and samples.shape == (total, POSE_SAMPLE_DTYPE.itemsize)
        assert filtered is None or filtered.shape == (total, 6)
        for t in (state_in, start_pose, state_out, filtered):
            assert t is None or t.dtype == torch.float32
        _check(lib().svo_pose_filter_batch(self._h, b, _ptr(state_in), _ptr(start_pose), _ptr(first), total,
                                           _ptr(samples), _ptr(state_out), _ptr(filtered)))

    # -- P2 ---------------------------------------------------------------
    def build_lk_pyramid(self, img, win, max_levels=3):
        levels = [img]
        h, w = img.shape
        for _ in range(1, max_levels):
            h = (h + 1) // 2
            w = (w + 1) // 2
            levels.append(torch.empty((h, w), dtype=torch.uint8, device=img.device))
        arr = _imgs(levels)
        n = C.c_int(0)
        _check(lib().svo_build_lk_pyramid(self._h, max_levels, win, arr, C.byref(n)))
        return levels[:n.value]

    # -- A ----------------------------------------------------------------
    def sparse_align(self, prev_pyr, cur_pyr, kps2d, kps3d, flags, cam, pose_guess,
                     dbg_level=-1):
        """PoseEstimator::estimate_pose. Returns (pose[6], cost, trace, dbg) as device/np."""
        dev = kps2d.device
        n = kps2d.shape[0]
        pose_out = torch.zeros(6, dtype=torch.float32, device=dev)
        cost = torch.zeros(1, dtype=torch.float32, device=dev)
        trace = torch.zeros(8 * GN_TRACE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        dbg = torch.zeros(48, dtype=torch.float32, device=dev) if dbg_level >= 0 else None
        _check(lib().svo_sparse_align(
            self._h, _imgs(prev_pyr, 8), _imgs(cur_pyr, 8), _ptr(kps2d), _ptr(kps3d), _ptr(flags),
            n, C.byref(cam), _ptr(pose_guess), _ptr(pose_out), _ptr(cost), _ptr(trace), _ptr(dbg),
            dbg_level))
        return pose_out, cost, trace, dbg

    def sparse_align_batch(self, n, n_bound, kps2d, kps3d, flags, prev_pyrs, cur_pyrs, cam, pose_guess, dbg_level=-1,
                           ws_fill=0, outputs=None, mats_out=None):
        """Diagnostic: svo_sparse_align of len(n) sequences in one launch. n: int32 [batch] device; the keypoint
        arrays are [batch, stride, ..] device tensors; prev_pyrs / cur_pyrs: per sequence the list of its level
        images (uint8 device tensors or views with unit column stride); pose_guess [batch, 6]. outputs: (pose_out
        [batch, 6], cost [batch], trace [batch, 8 * 52] bytes, dbg [batch, 48] or None) to write into, made here if
        None. mats_out: None, or a device tensor of at least batch blocks of pose_mats_layout()["bytes"] that receives
        every sequence's block of rotation matrices (svo_sparse_align_batch_mats). Returns (pose_out, cost, trace, dbg,
        (waves, mode, cap))."""
        batch, stride = kps2d.shape[0], kps2d.shape[1]
        dev = kps2d.device
        levels = cam.max_pyramid_levels
        if outputs is None:
            outputs = (torch.zeros((batch, 6), dtype=torch.float32, device=dev),
                       torch.zeros(batch, dtype=torch.float32, device=dev),
                       torch.zeros((batch, 8 * GN_TRACE_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                       torch.zeros((batch, 48), dtype=torch.float32, device=dev) if dbg_level >= 0 else None)
        pose_out, cost, trace, dbg = outputs
        pp, cp = (Image * (batch * levels))(), (Image * (batch * levels))()
        for b in range(batch):
            for l in range(levels):
                pp[b * levels + l], cp[b * levels + l] = _img(prev_pyrs[b][l]), _img(cur_pyrs[b][l])
        waves, mode, cap = C.c_int(0), C.c_int(0), C.c_int(0)
        args = (self._h, batch, stride, _ptr(n), int(n_bound), _ptr(kps2d), _ptr(kps3d), _ptr(flags), pp, cp, C.byref(cam),
                _ptr(pose_guess), int(dbg_level), C.c_uint32(ws_fill), _ptr(pose_out), _ptr(cost), _ptr(trace), _ptr(dbg),
                C.byref(waves), C.byref(mode), C.byref(cap))
        if mats_out is None:
            _check(lib().svo_sparse_align_batch(*args))
        else:
            assert mats_out.numel() * mats_out.element_size() >= batch * pose_mats_layout()["bytes"]
            _check(lib().svo_sparse_align_batch_mats(*args, _ptr(mats_out)))
        return pose_out, cost, trace, dbg, (waves.value, mode.value, cap.value)

    def sia_records_check(self, n, n_bound, kps2d, flags, prev_pyrs, cam, rec_cap=None, ws_fill=0, want_records=False, want_ref=False):
        """Diagnostic: the alignment records of len(n) sequences by the records kernel and by the one-lane-per-pixel
        kernel it replaced (svo_sia_records_check). n: int32 [batch] device; kps2d [batch, stride, 2] float32, flags
        [batch, stride] int32 / uint32 or None, device; prev_pyrs: per sequence the list of its max_pyramid_levels
        level images (uint8 device tensors or views with unit column stride). Returns (number of differing 32-bit
        words, index of the first or -1, the kernel's records [batch, levels used, 68, rec_cap] float32 or None); with
        want_ref a fourth value: the replaced kernel's records."""
        batch, stride = kps2d.shape[0], kps2d.shape[1]
        levels = cam.max_pyramid_levels
        if rec_cap is None:
            rec_cap = (max(int(n_bound), 1) + 255) // 256 * 256
        used = levels - cam.min_pyramid_level_pose_estimation
        rec = torch.empty((batch, used, 68, rec_cap), dtype=torch.float32, device=kps2d.device) if want_records else None
        ref = torch.empty((batch, used, 68, rec_cap), dtype=torch.float32, device=kps2d.device) if want_ref else None
        pp = (Image * (batch * levels))()
        for b in range(batch):
            for l in range(levels):
                pp[b * levels + l] = _img(prev_pyrs[b][l])
        n_diff, first = C.c_int64(0), C.c_int64(0)
        _check(lib().svo_sia_records_check(self._h, batch, stride, _ptr(n), int(n_bound), _ptr(kps2d), _ptr(flags), pp,
                                           C.byref(cam), int(rec_cap), C.c_uint32(ws_fill), _ptr(rec), _ptr(ref), C.byref(n_diff),
                                           C.byref(first)))
        return (n_diff.value, first.value, rec, ref) if want_ref else (n_diff.value, first.value, rec)

    # -- A3 ---------------------------------------------------------------
    def project_keypoints(self, pose, kps3d, cam):
        """project_keypoints (src/lib/transform_keypoints.cpp:11-48): pose [6] and kps3d device tensors."""
        n = kps3d.shape[0]
        out = torch.zeros((n, 2), dtype=torch.float32, device=kps3d.device)
        _check(lib().svo_project_keypoints(self._h, _ptr(pose), _ptr(kps3d), n, C.byref(cam), _ptr(out)))
        return out

    # -- B2 ---------------------------------------------------------------
    def klt_track(self, prev_lk, cur_lk, prev_pts, cur_pts, win):
        """OpticalFlow::calculate_optical_flow. cur_pts is updated in place."""
        n = prev_pts.shape[0]
        dev = prev_pts.device
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        err = torch.zeros(n, dtype=torch.float32, device=dev)
        nl = min(len(prev_lk), len(cur_lk))
        _check(lib().svo_klt_track(self._h, _imgs(prev_lk), _imgs(cur_lk), nl, _ptr(prev_pts),
                                   _ptr(cur_pts), n, win, _ptr(status), _ptr(err)))
        return cur_pts, status, err

    def klt_track_batch(self, seqs, n_bound, win, use_mats):
        """Diagnostic: svo_klt_track_batch, the KLT launch as the tracker makes it, over len(seqs) sequences. A
        sequence is a dict of device tensors: kfs (list of keyframes: dict(lk=[levels], kps2d float32 [m, 2],
        tmpl / valid uint8 tensors or None, tmpl_cap, tmpl_win)), cur ([levels]), n (int32 [1]), kf_id (int32 [n]
        or None), kp_index (int32 [n]), kps3d (float32 [n, 3]), pose (float32 [6]), cam (CameraSettings), and the
        outputs tracked, status, err, proj_out, ref_out (or None), which are written in place. Complete on return."""
        arr = (KltSequence * len(seqs))()
        keep = []
        for b, s in enumerate(seqs):
            kfs = (KltKeyframe * len(s["kfs"]))()
            keep.append(kfs)
            for k, f in enumerate(s["kfs"]):
                for l, im in enumerate(f["lk"]):
                    kfs[k].lk[l] = _img(im)
                tm, va = f.get("tmpl"), f.get("valid")
                kfs[k].n_lk, kfs[k].n_kps, kfs[k].kps2d = len(f["lk"]), f["kps2d"].shape[0], _ptr(f["kps2d"])
                kfs[k].tmpl, kfs[k].tmpl_valid = _ptr(tm), _ptr(va)
                kfs[k].tmpl_bytes = 0 if tm is None else tm.numel() * tm.element_size()
                kfs[k].tmpl_valid_bytes = 0 if va is None else va.numel() * va.element_size()
                kfs[k].tmpl_cap, kfs[k].tmpl_win = int(f.get("tmpl_cap", 0)), int(f.get("tmpl_win", 0))
            a = arr[b]
            a.kfs, a.n_kfs, a.n_cur = kfs, len(s["kfs"]), len(s["cur"])
            for l, im in enumerate(s["cur"]):
                a.cur[l] = _img(im)
            assert s["n"].dtype == torch.int32 and s["kp_index"].dtype == torch.int32
            assert s.get("kf_id") is None or s["kf_id"].dtype == torch.int32
            a.n, a.kf_id, a.kp_index, a.kps3d, a.pose = (_ptr(s["n"]), _ptr(s.get("kf_id")), _ptr(s["kp_index"]),
                                                         _ptr(s["kps3d"]), _ptr(s["pose"]))
            a.cam = s["cam"]
            a.tracked, a.status, a.err, a.proj_out, a.ref_out = (_ptr(s["tracked"]), _ptr(s["status"]), _ptr(s["err"]),
                                                                 _ptr(s["proj_out"]), _ptr(s.get("ref_out")))
        _check(lib().svo_klt_track_batch(self._h, len(seqs), arr, int(n_bound), int(win), int(bool(use_mats))))

    # -- B1 + B3 ----------------------------------------------------------
    def pinv6_check(self, H, impl):
        """Diagnostic: pinv of n 6x6 systems H[n, 36] (float32, device) through the solvers' Jacobi
        SVD, impl 0 = sequential reference, 1 = lane-parallel. Returns (out[n, 114] float32 =
        Hinv, W, Vt, U^T per system, sweeps[n] int32)."""
        n = H.shape[0]
        out = torch.empty((n, 114), dtype=torch.float32, device=H.device)
        sweeps = torch.empty(n, dtype=torch.int32, device=H.device)
        _check(lib().svo_pinv6_check(self._h, _ptr(H), n, _ptr(out), _ptr(sweeps), int(impl)))
        return out, sweeps

    def solve6_check(self, H, b, impl):
        """Diagnostic: the exact Gauss-Newton solve delta = pinv(H) b of n systems H[n, 36], b[n, 6]
        (float32, device), impl 0 = round-4 solve (wave-uniform finish), 1 = lane-resident solve of the
        kernels. Returns (out[n, 120] float32 = Hinv, W, Vt, U^T, delta per system, sweeps[n] int32)."""
        n = H.shape[0]
        out = torch.empty((n, 120), dtype=torch.float32, device=H.device)
        sweeps = torch.empty(n, dtype=torch.int32, device=H.device)
        _check(lib().svo_solve6_check(self._h, _ptr(H), _ptr(b), n, _ptr(out), _ptr(sweeps), int(impl)))
        return out, sweeps

    def reproj_gn(self, kps2d, kps3d, flags, cam, pose_in, tracked=None, err=None):
        dev = kps2d.device
        n = kps2d.shape[0]
        pose_out = torch.zeros(6, dtype=torch.float32, device=dev)
        cost = torch.zeros(1, dtype=torch.float32, device=dev)
        trace = torch.zeros(GN_TRACE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        _check(lib().svo_reproj_gn(self._h, _ptr(kps2d), _ptr(kps3d), _ptr(flags), n, C.byref(cam),
                                   _ptr(tracked), _ptr(err), _ptr(pose_in), _ptr(pose_out),
                                   _ptr(cost), _ptr(trace)))
        return pose_out, cost, trace

    def reproj_gn_batch(self, n, n_bound, kps2d, kps3d, flags, cam, pose_in, tracked=None, err=None, zero_out=None):
        """Diagnostic: svo_reproj_gn of len(n) sequences in one launch. n: int32 [batch] device; the keypoint
        arrays are [batch, stride, ..] device tensors (kps2d and flags are updated in place). Returns (pose_out
        [batch, 6], cost [batch], trace [batch] bytes, waves, cap)."""
        batch, stride = kps2d.shape[0], kps2d.shape[1]
        dev = kps2d.device
        pose_out = torch.zeros((batch, 6), dtype=torch.float32, device=dev)
        cost = torch.zeros(batch, dtype=torch.float32, device=dev)
        trace = torch.zeros((batch, GN_TRACE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        waves, cap = C.c_int(0), C.c_int(0)
        _check(lib().svo_reproj_gn_batch(self._h, batch, stride, _ptr(n), int(n_bound), _ptr(kps2d), _ptr(kps3d),
                                         _ptr(flags), C.byref(cam), _ptr(tracked), _ptr(err), _ptr(pose_in),
                                         _ptr(pose_out), _ptr(cost), _ptr(trace), _ptr(zero_out), C.byref(waves),
                                         C.byref(cap)))
        return pose_out, cost, trace, waves.value, cap.value

    # -- C1 ---------------------------------------------------------------
    def ssd_disparity(self, left, right, kps2d, win, search_x, search_y, clamp_half=1):
        n = kps2d.shape[0]
        out = torch.zeros(n, dtype=torch.float32, device=kps2d.device)
        a, b = _img(left), _img(right)
        _check(lib().svo_ssd_disparity(self._h, C.byref(a), C.byref(b), _ptr(kps2d), n, win,
                                       search_x, search_y, clamp_half, _ptr(out)))
        return out

    # -- C2 + D1 ----------------------------------------------------------
    def depth_filter_update(self, kps2d, kps3d, flags, cam, frame_pose, disparity, ref3d, ref2d,
                            kf_pose, outlier, inlier, kf_x, kf_p, do_outlier_check=1, do_update=1):
        n = kps2d.shape[0]
        _check(lib().svo_depth_filter_update(
            self._h, _ptr(kps2d), _ptr(kps3d), _ptr(flags), n, C.byref(cam), _ptr(frame_pose),
            _ptr(disparity), _ptr(ref3d), _ptr(ref2d), _ptr(kf_pose), _ptr(outlier), _ptr(inlier),
            _ptr(kf_x), _ptr(kf_p), do_outlier_check, do_update))

    def filter_update_batch(self, n, n_bound, kps2d, kps3d, flags, cam, frame_pose, disparity, ref3d, ref2d, kf_pose,
                            outlier, inlier, kf_x, kf_p, do_outlier_check, do_update, do_flags, do_reproject, width,
                            height, inside_count):
        """Diagnostic: svo_depth_filter_update of len(n) sequences in one launch, with the flag write-back, the
        reprojection and the inside counter of the tracker's launch. The keypoint arrays are [batch, stride, ..]
        device tensors, updated in place; inside_count int32 [batch], zeroed by the caller."""
        batch, stride = kps2d.shape[0], kps2d.shape[1]
        _check(lib().svo_filter_update_batch(
            self._h, batch, stride, _ptr(n), int(n_bound), _ptr(kps2d), _ptr(kps3d), _ptr(flags), C.byref(cam),
            _ptr(frame_pose), _ptr(disparity), _ptr(ref3d), _ptr(ref2d), _ptr(kf_pose), _ptr(outlier), _ptr(inlier),
            _ptr(kf_x), _ptr(kf_p), int(do_outlier_check), int(do_update), int(do_flags), int(do_reproject),
            int(width), int(height), _ptr(inside_count)))

    def filter_update_table_batch(self, seqs, n_bound, do_outlier_check=1, do_update=1, do_flags=1, do_reproject=1):
        """Diagnostic: svo_filter_update_table_batch, the depth filter launch as the tracker makes it for a tracked
        frame, over len(seqs) sequences. A sequence is a dict with the fields of svo_filter_table_sequence: cam
        (CameraSettings), kps (dict of the planes KPS_PLANES), frame_pose, disparity, kfs (a list of `table` dicts with
        the fields of svo_filter_keyframe; pose: six numbers), records / records_bytes, kf_mask, width, height,
        inside_count; addresses as device tensors or integers. The frame's and the keyframes' arrays are updated in
        place. Complete on return."""
        arr = (FilterTableSequence * len(seqs))()
        keep = []
        for a, s in zip(arr, seqs):
            kfs = (FilterKeyframe * max(len(s["kfs"]), 1))()
            keep.append(kfs)
            for k, f in zip(kfs, s["kfs"]):
                _fill(k, f, skip=("pose",))
                k.pose[:] = [float(v) for v in f["pose"]]
            _fill(a, s, skip=("kfs", "table"))
            a.kfs, a.table = kfs, int(s.get("table", len(s["kfs"])))
        _check(lib().svo_filter_update_table_batch(self._h, len(seqs), arr, int(n_bound), int(do_outlier_check),
                                                   int(do_update), int(do_flags), int(do_reproject)))

    # -- keyframe path bookkeeping -------------------------------------------
    def compact_batch(self, seqs, cap):
        """Diagnostic: svo_compact_batch over len(seqs) sequences, each a dict with the fields of
        svo_compact_sequence (src / dst: dicts of the planes KPS_PLANES; addresses as device tensors or integers).
        Returns the workgroup size of the launch. Complete on return."""
        arr = (CompactSequence * len(seqs))()
        for a, s in zip(arr, seqs):
            _fill(a, s)
        threads = C.c_int(0)
        _check(lib().svo_compact_batch(self._h, len(seqs), arr, int(cap), C.byref(threads)))
        return threads.value

    def keyframe_merge_batch(self, seqs, n_levels, max_cells, cap):
        """Diagnostic: svo_keyframe_merge_batch; seqs: dicts with the fields of svo_merge_sequence (cam: CameraSettings).
        Returns the workgroup size of the launch."""
        arr = (MergeSequence * len(seqs))()
        for a, s in zip(arr, seqs):
            _fill(a, s)
        threads = C.c_int(0)
        _check(lib().svo_keyframe_merge_batch(self._h, len(seqs), arr, int(n_levels), int(max_cells), int(cap),
                                              C.byref(threads)))
        return threads.value

    def keyframe_init_batch(self, seqs, cap):
        """Diagnostic: svo_keyframe_init_batch; seqs: dicts with the fields of svo_kf_init_sequence."""
        arr = (KfInitSequence * len(seqs))()
        for a, s in zip(arr, seqs):
            _fill(a, s)
        _check(lib().svo_keyframe_init_batch(self._h, len(seqs), arr, int(cap)))

    def ssd_disparity_batch(self, seqs, n_bound, win, search_y):
        """Diagnostic: svo_ssd_disparity_batch; seqs: dicts with the fields of svo_ssd_sequence (left / right: uint8
        device tensors or views). Returns the largest window of the kernel shape the launch chose."""
        arr = (SsdSequence * len(seqs))()
        for a, s in zip(arr, seqs):
            _fill(a, s, skip=("left", "right"))
            a.left, a.right = _img(s["left"]), _img(s["right"])
        max_win = C.c_int(0)
        _check(lib().svo_ssd_disparity_batch(self._h, len(seqs), arr, int(n_bound), int(win), int(search_y),
                                             C.byref(max_win)))
        return max_win.value

    def ssd_disparity_check(self, seqs, n_bound, win, search_y, stride, fill=0):
        """Diagnostic: svo_ssd_disparity_check, the one-wave SSD kernel against the four-wave kernel it replaced on
        the sequences of ssd_disparity_batch (their `disparity` is not written and may be missing). Returns (number
        of differing 32-bit words, index of the first or -1, the kernel's array [batch, stride] float32 whose
        unwritten words hold `fill`, the replaced kernel's array)."""
        arr = (SsdSequence * len(seqs))()
        for a, s in zip(arr, seqs):
            _fill(a, s, skip=("left", "right"))
            a.left, a.right = _img(s["left"]), _img(s["right"])
        out = torch.empty((len(seqs), int(stride)), dtype=torch.float32, device=self.device)
        ref = torch.empty_like(out)
        n_diff, first = C.c_int64(0), C.c_int64(0)
        _check(lib().svo_ssd_disparity_check(self._h, len(seqs), arr, int(n_bound), int(win), int(search_y), int(stride),
                                             C.c_uint32(fill), _ptr(out), _ptr(ref), C.byref(n_diff), C.byref(first)))
        return n_diff.value, first.value, out, ref


def detect_to_numpy(cells, counts):
    """Per level the structured array (DET_CELL_DTYPE) of its cells, from Handle.detect_keypoints' outputs."""
    c = cells.cpu().numpy().view(DET_CELL_DTYPE)[..., 0]
    return [c[l, :k].copy() for l, k in enumerate(counts.cpu().numpy())]


def trace_to_numpy(t):
    return t.cpu().numpy().view(GN_TRACE_DTYPE)
