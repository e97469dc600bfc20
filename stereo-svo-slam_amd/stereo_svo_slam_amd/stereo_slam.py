"""Host-side mirror of the reference's user API on top of the C ABI.

`StereoSlam` has the live surface of the reference's Python wrapper
(src/python/wrapper/slam_accelerator.pyx:50-91: ctor(CameraSettings),
new_image(left, right, time_stamp), get_frame(), get_keyframe(), get_keyframes())
and of the C++ class (src/include/stereo_slam.hpp:35-62: + get_trajectory,
update_pose).  `StereoSlamBatch` drives B independent sequences through the same
kernel launches (one svo_ctx).  No compute happens in Python.  The objects its
submit_* methods return live in jobs.py and are importable from here as well.
"""
import ctypes as C

import numpy as np
import torch

from . import hip_lib
from .hip_lib import POSE_SAMPLE_CHAIN, POSE_SAMPLE_DTYPE, CameraSettings, SvoError, _check, lib
from .jobs import (KP_INFO_DTYPE, ArPictures, Clouds, Disparities, Export, Carve, Frame, Fusion, MapExport, Prune,  # noqa: F401
                   Scenes, Snapshot, Views, VoxelLoads, VoxelMaps, VoxelSaves, caller_memory, int_array, named_slots)


class GnTrace(C.Structure):
    _fields_ = [("level", C.c_int32), ("n_gradient", C.c_int32), ("n_cost", C.c_int32),
                ("n_accepted", C.c_int32), ("exit_small", C.c_int32),
                ("initial_cost", C.c_float), ("final_cost", C.c_float), ("pose", C.c_float * 6)]


class FrameStats(C.Structure):
    """svo_frame_stats (include/svo_hip.h)."""
    _fields_ = [("frame_id", C.c_int32), ("is_keyframe", C.c_int32), ("n_keypoints", C.c_int32),
                ("n_keyframes", C.c_int32), ("inside_count", C.c_int32), ("overflow", C.c_int32),
                ("pose_sia", C.c_float * 6), ("pose_refined", C.c_float * 6),
                ("sia_cost", C.c_float), ("reproj_cost", C.c_float), ("sia_ms", C.c_float),
                ("stage_ms", C.c_float * 8),
                ("sia_trace", GnTrace * 8), ("reproj_trace", GnTrace)]


class Totals(C.Structure):
    """svo_totals (include/svo_hip.h)."""
    _fields_ = [("frames", C.c_int64), ("keyframes", C.c_int64), ("keypoints", C.c_int64),
                ("gn_gradient_calls", C.c_int64), ("gn_cost_calls", C.c_int64),
                ("stage_ms", C.c_double * 8), ("wall_ms", C.c_double),
                ("launches", C.c_int64), ("n_groups", C.c_int32), ("image_sets", C.c_int32)]


class LaunchShape(C.Structure):
    """svo_launch_shape (include/svo_hip.h)."""
    _fields_ = [("kernel", C.c_int32), ("waves", C.c_int32), ("mode", C.c_int32), ("cap", C.c_int32),
                ("launches", C.c_int64)]


class RunInfo(C.Structure):
    """svo_run_info (include/svo_hip.h): what stays of a sequence that a restart ended."""
    _fields_ = [("seq", C.c_int32), ("run", C.c_int32), ("frames", C.c_int32), ("keyframes", C.c_int32),
                ("last_time_stamp", C.c_float), ("pose", C.c_float * 6)]


class Memory(C.Structure):
    """svo_memory (include/svo_hip.h)."""
    _fields_ = [("device_bytes", C.c_int64), ("klt_cache_bytes", C.c_int64),
                ("image_sets", C.c_int32), ("image_sets_free", C.c_int32),
                ("keyframe_slabs", C.c_int32), ("keyframe_slabs_free", C.c_int32)]


KERNEL_NAMES = ("sia_gn_kernel", "reproj_gn_kernel")     # svo_launch_shape.kernel


def _shape_key(e):
    """(kernel name, waves, mode, cap) of a svo_launch_shape"""
    return (KERNEL_NAMES[e.kernel], e.waves, e.mode, e.cap)


def pick_launch_shapes(cfg, batch, n_bound, rec_cap=1 << 20, exact=True):
    """svo_pick_launch_shapes: the (kernel, waves, mode, cap) the alignment and the reprojection GN
    launch for `batch` sequences of at most n_bound keypoints of camera preset `cfg` (a host decision:
    no GPU needed); None for a kernel whose workspaces the keypoints exceed."""
    out = (LaunchShape * 2)()
    _check(lib().svo_pick_launch_shapes(C.byref(CameraSettings.from_dict(cfg)), cfg["width"], cfg["height"],
                                        batch, n_bound, rec_cap, int(exact), out))
    return tuple(_shape_key(e) if e.launches else None for e in out)


def pick_sia_lds_bytes(cfg, batch, n_bound, rec_cap=1 << 20, exact=True):
    """svo_pick_sia_lds_bytes: the dynamic LDS per workgroup of the alignment launch pick_launch_shapes
    describes (a host decision: no GPU needed)."""
    out = C.c_int64(0)
    _check(lib().svo_pick_sia_lds_bytes(C.byref(CameraSettings.from_dict(cfg)), cfg["width"], cfg["height"],
                                        batch, n_bound, rec_cap, int(exact), C.byref(out)))
    return out.value


class StereoSlamBatch:
    def __init__(self, camera_settings, width, height, n_sequences=1, device=0):
        if isinstance(camera_settings, dict):
            camera_settings = CameraSettings.from_dict(camera_settings)
        if not torch.cuda.is_available():
            raise SvoError("no GPU visible: libsvo_hip has no CPU fallback")
        self.cam = camera_settings
        self.width, self.height, self.n = width, height, n_sequences
        self.device = torch.device("cuda", device)
        self._fuse_stamp = 0             # submit_fuse: the automatic stamp
        self._fused_keyframe = {}        # fuse_new_keyframes: slot -> newest keyframe id it fused
        self._ctx = C.c_void_p()
        _check(lib().svo_ctx_create(C.byref(self.cam), width, height, n_sequences, device,
                                    C.byref(self._ctx)))

    def close(self):
        if getattr(self, "_ctx", None) and hip_lib._LIB is not None:
            hip_lib._LIB.svo_ctx_destroy(self._ctx)
        self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_fast_solver(self, on=True):
        """svo_ctx_set_fast_solver: off (default) = reference-order Gauss-Newton (bit-exact traces);
        on = tree sums + LDL^T solve."""
        self._fast = bool(on)
        if self._ctx:
            _check(lib().svo_ctx_set_fast_solver(self._ctx, int(on)))

    def set_exact_pinv(self, on=True):
        self.set_fast_solver(not on)

    def set_rectification(self, left_maps, right_maps):
        """svo_ctx_set_rectification: from the next frame on the images are RAW and are remapped on the GPU
        (cv::remap INTER_LINEAR, constant 0 border, bit-exact) before tracking. left_maps / right_maps:
        (map_x, map_y) of the library's left / right image, float32 [H, W] numpy arrays or CUDA tensors
        (EurocInput: left <- RIGHT.* calibration, right <- LEFT.*); None, None turns it off."""
        if left_maps is None and right_maps is None:
            self._rect = None
        else:
            maps = [*left_maps, *right_maps]
            on_dev = isinstance(maps[0], torch.Tensor)
            if on_dev:
                maps = [m.to(dtype=torch.float32).contiguous() for m in maps]
            else:
                maps = [np.ascontiguousarray(m, np.float32) for m in maps]
            self._rect = (maps, on_dev)
        if self._ctx:                      # (StereoSlam creates its ctx with the first image)
            self._apply_rectification()

    def _apply_rectification(self):
        rect = getattr(self, "_rect", None)
        if rect is None:
            _check(lib().svo_ctx_set_rectification(self._ctx, None, None, None, None, 0))
            return
        if isinstance(rect[0], hip_lib.CameraCalibration):
            _check(lib().svo_ctx_set_calibration(self._ctx, C.byref(rect[0]), C.byref(rect[1])))
            return
        maps, on_dev = rect
        for m in maps:
            assert tuple(m.shape) == (self.height, self.width), "a rectification map has the ctx size"
        if on_dev:
            assert all(m.is_cuda and m.device == self.device for m in maps), "maps on the ctx's GPU"
            ptrs = [C.c_void_p(m.data_ptr()) for m in maps]
        else:
            ptrs = [m.ctypes.data_as(C.c_void_p) for m in maps]
        _check(lib().svo_ctx_set_rectification(self._ctx, *ptrs, caller_memory(self.device, on_dev)))

    def set_calibration(self, left, right):
        """svo_ctx_set_calibration: set_rectification with the maps of two CameraCalibrations (the cameras behind the
        library's left / right image; EurocInput: left <- RIGHT.*, right <- LEFT.*), built on the GPU straight in the
        remap's fixed-point form; None, None turns rectification off."""
        if (left is None) != (right is None):
            raise ValueError("give both calibrations or none")
        self._rect = None if left is None else (left, right)
        if self._ctx:                      # (StereoSlam creates its ctx with the first image)
            self._apply_rectification()

    @staticmethod
    def build_rectify_maps(cals, width, height, device=0):
        """svo_build_rectify_maps: [(map_x, map_y)] float32 [height, width] CUDA tensors, one pair per
        CameraCalibration, all in one launch (the float maps set_rectification / add_rigs take)"""
        h = hip_lib.Handle(device, 1)
        try:
            out = h.build_rectify_maps(cals, width, height)
            h.synchronize()
        finally:
            h.close()
        return out

    def set_input_format(self, fmt):
        """svo_ctx_set_input_format: from the next frame on the frames are buffers of input format `fmt`
        (hip_lib.INPUT_*, or its name in hip_lib.INPUT_FORMATS) and become gray images on the GPU (cvtColor's
        15-bit fixed point, channel extract, the halves of a side-by-side frame). The pair formats take
        [H, W, 3] lefts and rights; the one-buffer formats take ONE list of [H, >= 2W] (sbs_gray),
        [H, >= 2W, 3] (sbs_bgr / sbs_rgb) or [H, W, 3] (ch3_econ) frames as `lefts` (rights: None)."""
        if isinstance(fmt, str):
            fmt = hip_lib.INPUT_FORMATS.index(fmt)
        hip_lib.input_format_info(fmt, self.width or 1)      # (raises for an unknown format)
        self._format = int(fmt)
        if self._ctx:                      # (StereoSlam creates its ctx with the first image)
            _check(lib().svo_ctx_set_input_format(self._ctx, self._format))

    def _frame_layout(self):
        """(buffers per sequence, the shape a buffer has at least, bytes per pixel) of the input format in force"""
        if not getattr(self, "_format", 0):        # (the default asks the library nothing)
            return 2, (self.height, self.width), 1
        info = hip_lib.input_format_info(self._format, self.width)
        shape = (self.height, info.min_row_pixels) + ((3,) if info.channels == 3 else ())
        return info.buffers, shape, info.channels

    @staticmethod
    def _fits(arr, shape, channels):
        """a frame buffer: the rows and channels of `shape`, at least its columns, pixels and channels dense"""
        sh = tuple(arr.shape)
        if len(sh) != len(shape) or sh[0] != shape[0] or sh[1] < shape[1] or sh[2:] != shape[2:]:
            return False
        strides = arr.stride() if isinstance(arr, torch.Tensor) else arr.strides
        return strides[-1] == 1 and (channels == 1 or strides[1] == 3)

    def enable_timing(self, on=True):
        self._timing = bool(on)
        if self._ctx:                      # (StereoSlam creates its ctx with the first image)
            _check(lib().svo_ctx_enable_timing(self._ctx, int(on)))

    def new_images(self, lefts, rights, time_stamps):
        """lefts/rights: per sequence a uint8 [H, W] numpy array (host) or torch CUDA tensor; None for
        a sequence that has no frame at this step (it sits the step out: sequences of a ctx may have
        different lengths; an empty slot starts its sequence with the first frame it gets)."""
        buffers, shape, channels = self._frame_layout()
        assert len(lefts) == self.n and (buffers == 1 or len(rights) == self.n)
        if all(x is None for x in lefts):
            return
        on_dev = isinstance(next(x for x in lefts if x is not None), torch.Tensor)
        ptrs_l = (C.c_void_p * self.n)()
        ptrs_r = (C.c_void_p * self.n)()
        keep = []
        stride = None
        for s in range(self.n):
            if lefts[s] is None:
                continue
            for arr, dst in ((lefts[s], ptrs_l), (rights[s], ptrs_r))[:buffers]:
                if on_dev:
                    assert arr.is_cuda and arr.dtype == torch.uint8
                    st, p = arr.stride(0), arr.data_ptr()
                else:
                    arr = np.ascontiguousarray(arr, dtype=np.uint8)
                    st, p = arr.strides[0], arr.ctypes.data
                assert self._fits(arr, shape, channels), (tuple(arr.shape), shape)
                assert stride is None or stride == st
                stride = st
                keep.append(arr)
                dst[s] = p
        ts = (C.c_float * self.n)(*[float(t) for t in time_stamps])
        _check(lib().svo_new_images(self._ctx, ptrs_l, ptrs_r, stride, ts, caller_memory(self.device, on_dev)))

    def pack_images(self, lefts, rights, time_stamps, borrow=False):
        """Pre-build the argument arrays of one step (keeps Python out of a timed loop); pass the
        result to new_images_packed / submit_packed. The frames are torch uint8 tensors, all on
        the GPU (SVO_MEM_DEVICE; with borrow=True SVO_MEM_DEVICE_BORROW: used in place, the caller
        keeps them alive and unchanged) or all in host memory (SVO_MEM_HOST; pinned for full PCIe rate).
        With a one-buffer input format (set_input_format) `lefts` holds the frames and `rights` is ignored."""
        buffers, shape, channels = self._frame_layout()
        ptrs_l = (C.c_void_p * self.n)()
        ptrs_r = (C.c_void_p * self.n)()
        some = next(x for x in lefts if x is not None)
        stride = some.stride(0)
        on_dev = some.is_cuda
        for s in range(self.n):
            if lefts[s] is None:                            # the sequence sits this step out
                continue
            for arr, dst in ((lefts[s], ptrs_l), (rights[s], ptrs_r))[:buffers]:
                assert arr.is_cuda == on_dev and arr.dtype == torch.uint8
                assert self._fits(arr, shape, channels) and arr.stride(0) == stride, (tuple(arr.shape), shape)
                dst[s] = arr.data_ptr()
        ts = (C.c_float * self.n)(*[float(t) for t in time_stamps])
        return ptrs_l, ptrs_r, stride, ts, (lefts, rights), (2 if borrow else 1) if on_dev else 0

    def new_images_packed(self, packed):
        _check(lib().svo_new_images(self._ctx, packed[0], packed[1], packed[2], packed[3], packed[5]))

    def submit_packed(self, packed):
        """Pipelined form (svo_submit_images): queues the frame set on every sequence group and
        returns; `packed` (and its device images) must stay alive until wait()."""
        _check(lib().svo_submit_images(self._ctx, packed[0], packed[1], packed[2], packed[3], packed[5]))

    def wait(self):
        _check(lib().svo_wait(self._ctx))

    def export_capacity(self):
        """svo_export_capacity: the records one slot of an export can take at most."""
        return hip_lib.export_capacity(self.cam, self.width, self.height)

    def submit_export(self, what="frames", seqs=None, device=False, fields=("kps2d", "kps3d", "info")):
        """svo_submit_export: queue the export of the current frames (what="frames") or newest keyframes
        ("last_keyframes") of the slots `seqs` (None: all, in order) behind the frame sets and restarts submitted
        so far; nothing is waited for. Returns an Export, valid after its wait() (or the ctx's); its submit()
        queues the same export again into the same buffers."""
        if isinstance(what, str):
            what = hip_lib.EXPORT_WHAT.index(what)
        return Export(self, int(what), seqs, device, fields).submit()

    def export_frames(self, seqs=None, device=False, fields=("kps2d", "kps3d", "info")):
        return self.submit_export("frames", seqs, device, fields).wait()

    def export_last_keyframes(self, seqs=None, device=False, fields=("kps2d", "kps3d", "info")):
        return self.submit_export("last_keyframes", seqs, device, fields).wait()

    def map_size(self, seq, from_keyframe=0):
        """svo_map_size: (keyframes, points_bound) an export of the slot's map from `from_keyframe` on needs right
        now (waits)."""
        k, p = C.c_int(0), C.c_int64(0)
        _check(lib().svo_map_size(self._ctx, int(seq), int(from_keyframe), C.byref(k), C.byref(p)))
        return k.value, p.value

    def submit_map(self, seqs=None, from_keyframe=None, filter=None, device=False, point_capacity=None,
                   keyframe_capacity=None, regions=None):
        """svo_submit_export_map: queue the export of every keyframe (from `from_keyframe` on: None = 0, an int, or
        one per slot) of the slots `seqs` (None: all, in order) as compacted points behind what was submitted so
        far. filter: None (everything), a hip_lib.MapFilter or a dict of its fields. Returns a MapExport, valid
        after its wait(). point_capacity / keyframe_capacity (an int or one per slot): room for what the frames
        still queued may add, nothing is waited for then and a slot that outgrew them comes back MAP_TOO_SMALL;
        default: what the slots need right now (map_size: waits for the queues). regions: a
        hip_lib.MAP_REGION_DTYPE array that places every slot itself."""
        if regions is None and (point_capacity is None or keyframe_capacity is None):
            named = named_slots(self, seqs, explicit=True)[0]
            frm = np.broadcast_to(0 if from_keyframe is None else from_keyframe, (len(named),))
            sizes = [self.map_size(s, f) for s, f in zip(named, frm)]
            if keyframe_capacity is None:
                keyframe_capacity = [k for k, _ in sizes]
            if point_capacity is None:
                point_capacity = [p for _, p in sizes]
        return MapExport(self, seqs, from_keyframe, filter, device, point_capacity, keyframe_capacity, regions).submit()

    def export_map(self, seqs=None, from_keyframe=None, filter=None, device=False):
        """the map of the slots `seqs`: regions sized from map_size, submit + wait; a slot that came back
        MAP_TOO_SMALL gets the capacities its segment asks for and the export runs once more."""
        m = self.submit_map(seqs, from_keyframe, filter, device).wait()
        if m.grow():
            m.submit().wait()
        return m

    def view_size(self, style):
        """svo_view_size: (cols, rows, pitch, image_bytes) of one image of a view job with `style` in this ctx"""
        return hip_lib.view_size(self.cam, self.width, self.height, style)

    def submit_views(self, what="frames", seqs=None, plane="left", level=0, pixel="gray8", markers=False,
                     drop_flags=None, size=None, size_temporary=None, device=False, style=None):
        """svo_submit_export_views: queue a view of the current frames (what="frames") or newest keyframes
        ("last_keyframes") of the slots `seqs` (None: all, in order) behind what was submitted so far; nothing is
        waited for. plane "left" (level 0 .. max_pyramid_levels - 1) or "right"; pixel "gray8", "rgb8" or "rgba8";
        markers: one marker per keypoint as the reference app's window draws them (hip_lib.view_style has the
        defaults of drop_flags and the two sizes); style: a hip_lib.ViewStyle instead of all these. Returns a Views,
        valid after its wait() (or the ctx's); its submit() queues the same job again into the same buffers."""
        if isinstance(what, str):
            what = hip_lib.EXPORT_WHAT.index(what)
        if style is None:
            style = hip_lib.view_style(what, plane, level, pixel, markers, drop_flags, size, size_temporary)
        return Views(self, what, seqs, style, device).submit()

    def export_views(self, what="frames", seqs=None, **kw):
        """submit_views + wait"""
        return self.submit_views(what, seqs, **kw).wait()

    def disparity_size(self, style, check=None):
        """svo_disparity_size: (cols, rows, planes, image_bytes) of one slot of a disparity job with `style` (and
        `check`, a hip_lib.StereoCheck or None) in this ctx"""
        return hip_lib.disparity_size(self.cam, self.width, self.height, style, check)

    @staticmethod
    def _stereo_check(lr_check):
        """lr_check of submit_disparity / submit_cloud as a hip_lib.StereoCheck: None or False: off (the unchecked
        entry); True: report only; a number: the tolerance max_lr_diff"""
        if lr_check is None or lr_check is False:
            return None
        return hip_lib.stereo_check(True, 0.0 if lr_check is True else float(lr_check))

    @staticmethod
    def _sgm_params(sgm):
        """sgm of submit_disparity / submit_cloud as (hip_lib.SgmParams, hip_lib.StereoCheck or None): hip_lib.sgm_job"""
        return hip_lib.sgm_job(sgm)

    def submit_disparity(self, what="frames", seqs=None, value="disparity", step=1, win=0, search_x=0, search_y=0,
                         cost=False, device=False, style=None, lr_check=None, sgm=None):
        """svo_submit_export_disparity: queue a dense disparity (value="disparity") or depth ("depth") map of the
        current frames (what="frames") or newest keyframes ("last_keyframes") of the slots `seqs` (None: all, in
        order) behind what was submitted so far; nothing is waited for. step: the lattice (1 .. 16); win, search_x,
        search_y: 0 takes the ctx's settings; cost: a second plane with the minimum SSD; style: a
        hip_lib.DisparityStyle instead of all these; lr_check: the left-right cross-check (True: the lr plane is
        appended; a tolerance: values that differ by more are set invalid as well; default off); sgm: semi-global
        aggregation and sub-pixel values (True: hip_lib.SGM_DEFAULTS; or dict(p1=, p2=, cost_cap=, subpixel=,
        lr_check=); search_x <= 63; the cost plane then holds the aggregated cost; the dict's lr_check (None, True or a
        tolerance, as the top-level one) is the cross-check of the SGM map, a second SGM map of the mirrored pair, e.g.
        sgm=dict(hip_lib.SGM_DEFAULTS, lr_check=1.0); the top-level lr_check together with sgm: ValueError; default off).
        Returns a Disparities, valid after its wait() (or the ctx's); its submit() queues the same job again into the
        same buffers."""
        if isinstance(what, str):
            what = hip_lib.EXPORT_WHAT.index(what)
        if style is None:
            style = hip_lib.disparity_style(value, step, win, search_x, search_y, cost)
        return Disparities(self, what, seqs, style, device, self._stereo_check(lr_check), *self._sgm_params(sgm)).submit()

    def export_disparity(self, what="frames", seqs=None, **kw):
        """submit_disparity + wait"""
        return self.submit_disparity(what, seqs, **kw).wait()

    def cloud_size(self, style):
        """svo_cloud_size: (cols, rows, points_per_slot) of one slot of a cloud job with `style` in this ctx"""
        return hip_lib.cloud_size(self.cam, self.width, self.height, style)

    def submit_cloud(self, what="frames", seqs=None, step=1, win=0, search_x=0, search_y=0, frame="world", layout="compact",
                     min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0, device=False, style=None, lr_check=None, sgm=None):
        """svo_submit_export_cloud: queue a dense coloured point cloud of the current frames (what="frames") or newest
        keyframes ("last_keyframes") of the slots `seqs` (None: all, in order) behind what was submitted so far;
        nothing is waited for. step, win, search_x, search_y: as submit_disparity; frame: "world" or "camera";
        layout: "compact" or "organized"; min_disparity, max_depth, max_mean_cost: the filter (0: off); style: a
        hip_lib.CloudStyle instead of all these; lr_check: a tolerance > 0 drops the points that fail the left-right
        cross-check (default off); sgm: as submit_disparity: the cloud of the SGM map (max_mean_cost then bounds the
        aggregated cost over its four paths; the dict's lr_check, a tolerance > 0, drops the points that fail the SGM
        map's cross-check; the top-level lr_check together with sgm: ValueError; default off). Returns a Clouds, valid after its wait() (or the ctx's); its submit()
        queues the same job again into the same buffers."""
        if isinstance(what, str):
            what = hip_lib.EXPORT_WHAT.index(what)
        if style is None:
            style = hip_lib.cloud_style(step, win, search_x, search_y, frame, layout, min_disparity, max_depth, max_mean_cost)
        return Clouds(self, what, seqs, style, device, self._stereo_check(lr_check), *self._sgm_params(sgm)).submit()

    def export_cloud(self, what="frames", seqs=None, **kw):
        """submit_cloud + wait"""
        return self.submit_cloud(what, seqs, **kw).wait()

    def submit_scenes(self, seqs=None, camera="front", device=False, style=None, dense=None, clouds=None, **kw):
        """svo_submit_export_scenes: queue the viewer's 3-D picture (keyframe points, trajectory, a frustum per
        keyframe and at the current pose) of the slots `seqs` (None: all, in order) behind what was submitted so far;
        nothing is waited for. camera: a preset name ("front", "top", "side"), one hip_lib.SceneCamera for all, or a
        list with one per named slot; style: a hip_lib.SceneStyle, or its fields as keywords (hip_lib.scene_style:
        cols, rows, pixel, point_size, colours, show, from_keyframe, trajectory_tail, filter). dense: None, or a dict
        (any of what, step, win, search_x, search_y, min_disparity, max_depth, max_mean_cost, lr_check, point_size, sgm;
        live=False: only point_size counts, for `clouds`; sgm: as submit_cloud's: the live layer is the cloud of the SGM
        map, its check the lr_check key of the sgm dict, and lr_check beside sgm is a ValueError) that draws the dense cloud of every named slot's frame (what="frames") or newest keyframe ("last_keyframes")
        into its picture, the cloud submit_cloud(layout="organized") with these values would deliver; clouds: None,
        or per named slot a device tensor of hip_lib.MAP_POINT_DTYPE bytes, (address, n) or None: records of the
        caller's drawn as well (they stay alive and unchanged until the job is delivered). Returns a Scenes, valid
        after its wait() (or the ctx's); its submit() queues the same job again into the same buffers."""
        if style is None:
            style = hip_lib.scene_style(**kw)
        if isinstance(camera, str):
            camera = hip_lib.scene_preset(camera, style.cols, style.rows)
        return Scenes(self, seqs, style, camera, device, dense, clouds).submit()

    def export_scenes(self, seqs=None, **kw):
        """submit_scenes + wait"""
        return self.submit_scenes(seqs, **kw).wait()

    def submit_ar(self, meshes, instances, seqs=None, first=None, device=False, style=None, occlusion=None, **kw):
        """svo_submit_export_ar: queue the AR demo's picture (the instanced meshes, lit and depth tested, over the
        left image of each named slot's current frame, seen from its pose through its rig's intrinsics) of the named
        slots (None: all), ordered with the frame sets; nothing is waited for. meshes, instances, first: see
        ArPictures; style: a hip_lib.ArStyle, or its fields as keywords (hip_lib.ar_style: pixel, light, ambient,
        near). occlusion: None, a hip_lib.ArOcclusion, or a dict (step, hidden = "drop" | "dim", alpha, margin,
        drop_flags, win, search_x, search_y, min_disparity, max_depth, max_mean_cost, lr_check, sgm): the job is
        svo_submit_export_ar_occluded, the meshes are hidden behind the dense, checked stereo depth of the frame and
        ArPictures.visibility counts the covered and hidden pixels. sgm in the dict (as submit_cloud's): the depth is
        the SGM map's (svo_submit_export_ar_occluded_sgm), its check the lr_check key of the sgm dict, and lr_check
        beside sgm is a ValueError. Returns an ArPictures, valid after wait()."""
        if style is None:
            style = hip_lib.ar_style(**kw)
        return ArPictures(self, seqs, style, meshes, instances, first, device, occlusion).submit()

    def export_ar(self, meshes, instances, seqs=None, **kw):
        """submit_ar + wait"""
        return self.submit_ar(meshes, instances, seqs, **kw).wait()

    def snapshot_size(self, seq):
        """svo_snapshot_size: (host_bytes, data_bytes) a save of the slot needs right now (waits)."""
        hb, db = C.c_int64(0), C.c_int64(0)
        _check(lib().svo_snapshot_size(self._ctx, int(seq), C.byref(hb), C.byref(db)))
        return hb.value, db.value

    def _snapshot_call(self, fn, seqs, snaps):
        seqs, n, seq_arr = named_slots(self, seqs)
        assert n == len(snaps)
        device = [s.device_mode for s in snaps]
        assert all(device) or not any(device), "snapshots of one call are all in host or all in device memory"
        arr = (hip_lib.SnapshotBuffers * max(n, 1))(*[s._buffers() for s in snaps])
        _check(fn(self._ctx, seq_arr, n, arr, caller_memory(self.device, any(device))))

    def new_snapshot(self, host_bytes, data_bytes, device=False):
        """zeroed buffers for a save (zeroed: the bytes between the planes of a device-mode data part are not
        written)"""
        return Snapshot(np.zeros(host_bytes, np.uint8),
                        torch.zeros(data_bytes, dtype=torch.uint8, device=self.device) if device
                        else np.zeros(data_bytes, np.uint8))

    def submit_save(self, seqs=None, device=False, snapshots=None):
        """svo_submit_save: queue the save of the slots `seqs` (None: all) behind what was submitted so far.
        Returns the Snapshots, valid after wait(). snapshots: buffers to save into (new_snapshot), with room for
        what the frames still queued may add; nothing is waited for then, and a save whose capacity turns out too
        small gives a header-only snapshot (info.status == SNAPSHOT_TOO_SMALL, with the sizes needed). Default:
        made here with the sizes the slots need, after a wait for the queues."""
        seqs = named_slots(self, seqs, explicit=True)[0]
        if snapshots is None:
            snapshots = [self.new_snapshot(*self.snapshot_size(s), device) for s in seqs]
        self._snapshot_call(lib().svo_submit_save, seqs, snapshots)
        return snapshots

    def save(self, seqs=None, device=False):
        """submit_save + wait: the Snapshots of the slots `seqs` (None: all)"""
        snaps = self.submit_save(seqs, device)
        self.wait()
        return snaps

    def submit_load(self, seqs, snapshots):
        """svo_submit_load: queue the load of snapshots[i] into slot seqs[i]; the slot's current sequence ends as
        with restart(). A bad snapshot raises SvoError here and nothing is queued. The data parts stay alive and
        unchanged until wait()."""
        self._snapshot_call(lib().svo_submit_load, seqs, list(snapshots))

    def load(self, seqs, snapshots):
        self.submit_load(seqs, snapshots)
        self.wait()

    def restart(self, seqs):
        """svo_ctx_restart_sequences: the named slots end their sequences (ordered with the submitted frame
        sets, does not wait); the next frame a slot gets is frame 0 of a new sequence."""
        seqs, n, arr = named_slots(self, [seqs] if np.isscalar(seqs) else seqs)
        _check(lib().svo_ctx_restart_sequences(self._ctx, arr, n))
        self._forget_fused(seqs)                # (the new run's keyframes are new)

    # -- trimming retired keyframes ------------------------------------------------------------------------
    def trim_keyframes(self, seqs=None, below=None, wait=True):
        """svo_submit_trim_keyframes: the slots `seqs` (None: all, in order) drop their keyframes with an id below
        min(below, retired) (below: None = everything retired, an int, or one per slot), ordered with the submitted
        frame sets like restart(). wait=False: queued only. Ids never move; the storage returns to the ctx."""
        _, n, arr = named_slots(self, [seqs] if np.isscalar(seqs) else seqs)
        lim = None if below is None else int_array([int(b) for b in np.broadcast_to(below, (n,))])
        fn = lib().svo_trim_keyframes if wait else lib().svo_submit_trim_keyframes
        _check(fn(self._ctx, arr, lim, n))

    def set_keyframe_window(self, keep):
        """svo_ctx_set_keyframe_window: keep >= 0: after each step a slot keeps at most `keep` retired keyframes;
        -1 (the default): slots never trim on their own. Waits for the queues."""
        _check(lib().svo_ctx_set_keyframe_window(self._ctx, int(keep)))

    def keyframe_range(self, seq=0):
        """svo_get_keyframe_range: a hip_lib.KeyframeRange (first, retired, count, table) of the slot (waits)."""
        r = hip_lib.KeyframeRange()
        _check(lib().svo_get_keyframe_range(self._ctx, int(seq), C.byref(r)))
        return r

    # -- camera rigs ---------------------------------------------------------------------------------------
    def add_rigs(self, rigs):
        """svo_ctx_add_rigs / svo_ctx_add_rigs_calibrated: every rig is a dict (or CameraSettings) with the ten float
        settings baseline, fx, fy, cx, cy, k1, k2, k3, p1, p2, and optionally (dict only) its rectification in one of
        two forms: "left_maps" and "right_maps", (map_x, map_y) of the library's left / right image as in
        set_rectification, float32 [H, W] numpy arrays or CUDA tensors (both or neither); or "left_calibration" and
        "right_calibration", two CameraCalibrations as in set_calibration (both or neither; not with maps). A list
        may mix the forms: each form goes to its entry in one call. Waits for queued work. Returns the ids in the
        order of `rigs` (>= 1; rig 0 is the ctx's own settings and set_rectification's maps)."""
        arr = (hip_lib.Rig * max(len(rigs), 1))()
        keep, cals = [], {}
        for i, r in enumerate(rigs):
            arr[i] = hip_lib.Rig.from_dict(r)
            is_dict = isinstance(r, dict)
            cal = (r.get("left_calibration"), r.get("right_calibration")) if is_dict else (None, None)
            maps = [*r["left_maps"], *r["right_maps"]] if is_dict and r.get("left_maps") is not None else None
            if (cal[0] is None) != (cal[1] is None):
                raise ValueError(f"rig {i}: give both calibrations or none")
            if cal[0] is not None:
                if maps is not None or r.get("right_maps") is not None:
                    raise ValueError(f"rig {i}: calibrations or maps, not both")
                cals[i] = cal
                continue
            if maps is None:
                continue
            on_dev = isinstance(maps[0], torch.Tensor)
            maps = [m.to(dtype=torch.float32).contiguous() if on_dev else np.ascontiguousarray(m, np.float32) for m in maps]
            for m in maps:
                assert tuple(m.shape) == (self.height, self.width), "a rectification map has the ctx size"
            keep.append(maps)
            ptrs = [m.data_ptr() if on_dev else m.ctypes.data for m in maps]
            arr[i].left_map_x, arr[i].left_map_y, arr[i].right_map_x, arr[i].right_map_y = ptrs
            arr[i].mem = caller_memory(self.device, on_dev)
        plain = [i for i in range(len(rigs)) if i not in cals]
        out = [None] * len(rigs)
        added = []
        try:
            for idx, calibrated in ((plain, False), (sorted(cals), True)):
                if not idx and (calibrated or cals):
                    continue
                n = len(idx)
                sub = (hip_lib.Rig * max(n, 1))(*[arr[i] for i in idx])
                ids = (C.c_int * max(n, 1))()
                if calibrated:
                    left = (hip_lib.CameraCalibration * n)(*[cals[i][0] for i in idx])
                    right = (hip_lib.CameraCalibration * n)(*[cals[i][1] for i in idx])
                    _check(lib().svo_ctx_add_rigs_calibrated(self._ctx, sub, left, right, n, ids))
                else:
                    _check(lib().svo_ctx_add_rigs(self._ctx, sub, n, ids))
                for k, i in enumerate(idx):
                    out[i] = ids[k]
                added += list(ids[:n])
        except SvoError:
            if added:                             # (a mixed list is all or nothing, like each entry)
                _check(lib().svo_ctx_remove_rigs(self._ctx, int_array(added), len(added)))
            raise
        for i in range(len(rigs)):                # (find_rig: the full settings of every rig added here)
            cam = CameraSettings.from_buffer_copy(self.cam)
            for name in hip_lib.RIG_FLOATS:
                setattr(cam, name, getattr(arr[i], name))
            self._rig_settings()[out[i]] = bytes(cam)
        return out

    def _rig_settings(self):
        if getattr(self, "_rig_cams", None) is None:
            self._rig_cams = {0: bytes(self.cam)}
        return self._rig_cams

    def remove_rigs(self, ids):
        """svo_ctx_remove_rigs: waits; SvoError (nothing removed) for rig 0 or while a slot is bound to one of them"""
        ids = [int(i) for i in ([ids] if np.isscalar(ids) else ids)]
        _check(lib().svo_ctx_remove_rigs(self._ctx, int_array(ids), len(ids)))
        for i in ids:
            self._rig_settings().pop(i, None)

    def assign_rigs(self, seqs, rigs):
        """svo_ctx_assign_rigs: slot seqs[i] ends its sequence like restart() and is bound to rig rigs[i] (ordered with
        the submitted frame sets, does not wait); its next frame is frame 0 of a new sequence under that rig."""
        (_, n, seq_arr), rigs = named_slots(self, seqs), [int(r) for r in rigs]
        assert n == len(rigs)
        _check(lib().svo_ctx_assign_rigs(self._ctx, seq_arr, int_array(rigs), n))

    def slot_rig(self, seq):
        """svo_ctx_get_slot_rig: (rig id, CameraSettings the slot tracks with)"""
        rig, cam = C.c_int(0), CameraSettings()
        _check(lib().svo_ctx_get_slot_rig(self._ctx, seq, C.byref(rig), C.byref(cam)))
        return rig.value, cam

    def rigs(self):
        """svo_ctx_get_rigs: (rigs of the ctx, rig 0 included; device bytes of the added rigs' maps)"""
        n, b = C.c_int(0), C.c_int64(0)
        _check(lib().svo_ctx_get_rigs(self._ctx, C.byref(n), C.byref(b)))
        return n.value, b.value

    def find_rig(self, cam, add=False):
        """the id of a rig this object has added (or rig 0) whose settings equal `cam` (CameraSettings) byte for byte;
        add: a rig without maps is added when there is none. None otherwise."""
        for rid, b in self._rig_settings().items():
            if b == bytes(cam):
                return rid
        return self.add_rigs([cam])[0] if add else None

    def finished_runs(self, seq):
        """The kept records of the slot's ended sequences, oldest first: [(RunInfo, trajectory[n, 6])]."""
        n = C.c_int(0)
        _check(lib().svo_get_finished_runs(self._ctx, seq, C.byref(n)))
        out = []
        for i in range(n.value):
            info, m = RunInfo(), C.c_int(0)
            _check(lib().svo_get_finished_run(self._ctx, seq, i, C.byref(info), None, 0, C.byref(m)))
            traj = np.zeros((m.value, 6), np.float32)
            _check(lib().svo_get_finished_run(self._ctx, seq, i, None, traj.ctypes.data_as(C.c_void_p), m.value, None))
            out.append((info, traj))
        return out

    def drop_finished_runs(self, seq=-1):
        _check(lib().svo_drop_finished_runs(self._ctx, seq))

    # -- voxel maps: the slots' dense clouds fused into one bounded map per slot -----------------------------------
    def _forget_fused(self, seqs):
        """fuse_new_keyframes fuses the newest keyframe of these slots (None: all) again"""
        for s in (range(self.n) if seqs is None else seqs):
            self._fused_keyframe.pop(s, None)

    def set_voxel_maps(self, voxel, log2_capacity=20, seqs=None, drop_flags=0):
        """svo_ctx_set_voxel_maps: every slot of `seqs` (None: all) gets an empty voxel map of edge `voxel` and
        1 << log2_capacity entries (10 .. 26); voxel=None takes the maps away. Waits for the queues."""
        seqs, n, arr = named_slots(self, seqs)
        params = None if voxel is None else C.byref(hip_lib.voxel_params(voxel, log2_capacity, drop_flags))
        _check(lib().svo_ctx_set_voxel_maps(self._ctx, arr, n, params))
        self._forget_fused(seqs)

    def voxel_map_info(self, seq=0):
        """svo_get_voxel_map_info as a dict (waits); None for a slot without a map"""
        info = hip_lib.VoxelMapInfo()
        if lib().svo_get_voxel_map_info(self._ctx, int(seq), C.byref(info)) != 0:
            return None
        return {n: getattr(info, n) for n, _ in hip_lib.VoxelMapInfo._fields_ if n != "_pad"}

    def submit_fuse(self, what="last_keyframes", seqs=None, stamp=None, lr_check=None, step=4, win=0, search_x=0, search_y=0,
                    min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0, sgm=None):
        """svo_submit_fuse_clouds: queue the fusion of the dense world-frame cloud of the newest keyframes (or,
        what="frames", the current frames) of the slots `seqs` (None: all) into their voxel maps, behind what was
        submitted so far; nothing is waited for. The cloud is submit_cloud's (step, win, search_x, search_y, the
        filter, lr_check, sgm: with sgm the job is svo_submit_fuse_clouds_sgm and fuses the cloud of the SGM map, whose
        check is the lr_check key of the sgm dict; the top-level lr_check together with sgm: ValueError); stamp: a u32
        the reached voxels are raised to (None: a counter of this object, one more per job). Returns a Fusion, valid
        after its wait() (or the ctx's)."""
        if isinstance(what, str):
            what = hip_lib.EXPORT_WHAT.index(what)
        sgm = hip_lib.sgm_consumer(sgm, lr_check, "submit_fuse")
        if stamp is None:
            self._fuse_stamp += 1
            stamp = self._fuse_stamp
        style = hip_lib.cloud_style(step, win, search_x, search_y, "world", "compact", min_disparity, max_depth, max_mean_cost)
        return Fusion(self, what, seqs, style, self._stereo_check(lr_check), stamp, *sgm).submit()

    def fuse_clouds(self, what="last_keyframes", seqs=None, grow=None, **kw):
        """submit_fuse + wait. grow=N: the maps of the slots that came back FUSE_FULL are resized (resize_voxel_maps)
        one step of log2_capacity at a time, up to N, and each is fused once more with the same stamp at the same queue
        position (nothing else was submitted in between); the returned Fusion holds the second answer for them. A slot
        still FUSE_FULL at N stays so. grow=None: the one job, as ever."""
        job = self.submit_fuse(what, seqs, **kw).wait()
        return job if grow is None else self._grow_and_fuse_again(job, grow)

    def _grow_and_fuse_again(self, job, grow):
        """fuse_clouds(grow=) on a delivered Fusion: resize what came back FUSE_FULL, fuse it again, keep the second answer"""
        named = list(range(self.n)) if job.seqs is None else job.seqs
        full = [i for i, f in enumerate(job.info) if int(f["status"]) == hip_lib.FUSE_FULL]
        while full:
            log2 = {i: self.voxel_map_info(named[i])["log2_capacity"] for i in full}
            full = [i for i in full if log2[i] < int(grow)]
            if not full:
                break
            for lg in sorted(set(log2[i] for i in full)):
                self.resize_voxel_maps(lg + 1, [named[i] for i in full if log2[i] == lg])
            again = Fusion(self, job.what, [named[i] for i in full], job.style, None if job.sgm is not None else job.check, job.stamp, job.sgm,
                           job.check if job.sgm is not None else None).submit().wait()
            for j, i in enumerate(full):
                job.info[i] = again.info[j]
            full = [i for i in full if int(job.info[i]["status"]) == hip_lib.FUSE_FULL]
        return job

    def fuse_new_keyframes(self, seqs=None, prune=None, carve=None, grow=None, **kw):
        """fuse_clouds("last_keyframes") of only those slots whose newest keyframe changed since this method last fused
        them (the bookkeeping is here, on the host: it waits for the queues to read the keyframe counts). Returns the
        Fusion, or None when no slot has a new keyframe. prune: a dict of submit_prune's keywords; the prune of the
        fused slots is queued behind the fuse (and waited for with it; the Prune is the Fusion's `.prune`).
        keep_stamps=N in it stands for min_stamp = stamp - N + 1 with `stamp` this fuse's: what the last N fuses of
        this object reached stays. carve: a dict of submit_carve's keywords (margin at least); the carve of the fused
        slots by their current frames is queued in FRONT of the fuse, so that what the camera sees through leaves before
        the new cloud arrives (the Carve is the Fusion's `.carve`). grow=N: as fuse_clouds(grow=N); the second fuse of a
        slot that was full then runs behind this call's prune."""
        named = named_slots(self, seqs, explicit=True)[0]
        self.wait()
        fresh = []
        for s in named:
            r = self.keyframe_range(s)
            newest = r.count - 1
            if r.count > 0 and self._fused_keyframe.get(s) != newest:
                fresh.append((s, newest))
        if not fresh:
            return None
        carved = None if carve is None else self.submit_carve(seqs=[s for s, _ in fresh], **dict(carve))
        job = self.submit_fuse("last_keyframes", [s for s, _ in fresh], **kw)
        job.prune, job.carve = None, carved
        if prune is not None:
            prune = dict(prune)
            keep_stamps = prune.pop("keep_stamps", None)
            if keep_stamps is not None:
                prune["min_stamp"] = max(0, job.stamp - int(keep_stamps) + 1)
            job.prune = self.submit_prune([s for s, _ in fresh], **prune)
        job.wait()
        if grow is not None:
            self._grow_and_fuse_again(job, grow)
        for (s, newest), f in zip(fresh, job.info):
            if int(f["status"]) == hip_lib.FUSE_OK:
                self._fused_keyframe[s] = newest
        return job

    def submit_voxel_maps(self, seqs=None, min_count=0, min_stamp=0, device=False, capacities=None):
        """svo_submit_export_voxel_maps: queue the export of the voxel maps of the slots `seqs` (None: all) as
        MAP_POINT_DTYPE records in key order. capacities: the records each slot's region holds (an int or one per
        slot; nothing is waited for then, and a slot that outgrew it comes back VOXEL_TOO_SMALL); default: what the
        maps hold right now (waits for the queues). Returns a VoxelMaps, valid after its wait()."""
        if capacities is None:
            named = named_slots(self, seqs, explicit=True)[0]
            capacities = [(self.voxel_map_info(s) or {"n_voxels": 0})["n_voxels"] for s in named]
        return VoxelMaps(self, seqs, capacities, min_count, min_stamp, device).submit()

    def export_voxel_maps(self, seqs=None, **kw):
        """submit_voxel_maps + wait"""
        return self.submit_voxel_maps(seqs, **kw).wait()

    def submit_save_voxel_maps(self, seqs=None, min_count=0, min_stamp=0, device=False, capacities=None):
        """svo_submit_save_voxel_maps: queue the save of the voxel maps of the slots `seqs` (None: all) as their raw
        entries (hip_lib.VOXEL_ENTRY_DTYPE: key, counts, sums and stamps verbatim) in key order: what load_voxel_maps
        takes, and nothing is lost on the way. capacities, min_count, min_stamp, device: as submit_voxel_maps. Returns
        a VoxelSaves, valid after its wait()."""
        if capacities is None:
            named = named_slots(self, seqs, explicit=True)[0]
            capacities = [(self.voxel_map_info(s) or {"n_voxels": 0})["n_voxels"] for s in named]
        return VoxelSaves(self, seqs, capacities, min_count, min_stamp, device).submit()

    def save_voxel_maps(self, seqs=None, **kw):
        """submit_save_voxel_maps + wait"""
        return self.submit_save_voxel_maps(seqs, **kw).wait()

    def submit_load_voxel_maps(self, seqs, saves, merge=False, voxel=None):
        """svo_submit_load_voxel_maps: queue a load into the voxel maps of the slots `seqs` (None: all), behind what was
        submitted so far. saves: a delivered VoxelSaves (its named slot i goes to seqs[i]; a slot that had no map when it
        was saved is left out of the job, whose `seqs` then names the others), or per slot entry records
        (numpy hip_lib.VOXEL_ENTRY_DTYPE, a uint8 [n, 40] tensor, None) with voxel= the edge their keys were made with
        (one, or one per slot). merge=False: a map is cleared first and then holds exactly the entries; merge=True: they
        are added to what it holds, to the bit as if their records had been fused. The edge must be the map's own, bit
        for bit. Returns a VoxelLoads, valid after its wait(): `info` says per slot what happened (VOXEL_LOAD_FULL: the
        map is too small and unchanged: resize_voxel_maps)."""
        if isinstance(saves, VoxelSaves):
            named = named_slots(self, seqs, explicit=True)[0]
            if len(named) != len(saves.segments):
                raise ValueError(f"a VoxelSaves of {len(saves.segments)} slots for {len(named)} slots")
            small = [i for i in range(len(named)) if saves.status(i) == hip_lib.VOXEL_TOO_SMALL]
            if small:
                raise ValueError(f"slots {small} of the VoxelSaves came back VOXEL_TOO_SMALL: they hold no entries")
            ok = [i for i in range(len(named)) if saves.status(i) == hip_lib.VOXEL_OK]     # (a slot that had no map is left out of the job)
            seqs, voxel, saves = [named[i] for i in ok], [saves.voxel(i) for i in ok], [saves.entries(i) for i in ok]
        elif voxel is None:
            raise ValueError("entries without a VoxelSaves need voxel=")
        return VoxelLoads(self, seqs, list(saves), voxel, merge).submit()

    def load_voxel_maps(self, seqs, saves, **kw):
        """submit_load_voxel_maps + wait"""
        return self.submit_load_voxel_maps(seqs, saves, **kw).wait()

    def resize_voxel_maps(self, log2_capacity, seqs=None):
        """svo_ctx_resize_voxel_maps: the voxel maps of the slots `seqs` (None: all; slots without a map are skipped) move
        into tables of 1 << log2_capacity entries (10 .. 26) with every entry, count, sum, stamp and counter kept. Waits
        for the queues. Raises (SVO_ERR_CAPACITY, nothing changed) when a slot's entries do not fit."""
        seqs, n, arr = named_slots(self, seqs)
        _check(lib().svo_ctx_resize_voxel_maps(self._ctx, arr, n, int(log2_capacity)))

    def submit_prune(self, seqs=None, min_count=0, min_stamp=0, radius=None, center="pose"):
        """svo_submit_prune_voxel_maps: queue a prune of the voxel maps of the slots `seqs` (None: all) behind what was
        submitted so far; nothing is waited for. An entry stays iff count >= max(1, min_count), last >= min_stamp and,
        with a radius, it lies in the box around the centre. radius: metres (None: no box), turned into voxels per
        slot as floor(radius / voxel) with that slot's voxel edge in double, so the box never reaches further than
        `radius` from the centre voxel's faces; slots whose maps differ in their edge go as one job per edge (the
        edges are read from the ctx: with a radius this waits for the queues once). center: "pose" (each slot's
        camera centre when the job runs), one xyz for all, or an array of one xyz per named slot. Returns a Prune,
        valid after its wait() (or the ctx's); with several edges a list of them."""
        if radius is None:                                   # no box: no centre is read, and no pose is asked for
            return Prune(self, seqs, hip_lib.voxel_keep(min_count, min_stamp), None).submit()
        named = named_slots(self, seqs, explicit=True)[0]
        by_radius, no_map = {}, []
        for i, s in enumerate(named):
            info = self.voxel_map_info(s)
            if info is None:
                no_map.append(i)                              # (PRUNE_NO_MAP whatever the radius: it goes with the first job)
            else:
                by_radius.setdefault(int(np.floor(float(radius) / float(np.float32(info["voxel"])))), []).append(i)
        first = next(iter(by_radius), 0)
        by_radius[first] = sorted(by_radius.get(first, []) + no_map)
        per_slot = None if isinstance(center, str) else np.broadcast_to(np.asarray(center, np.float32), (len(named), 3))
        jobs = [Prune(self, [named[i] for i in idx], hip_lib.voxel_keep(min_count, min_stamp, radius=r),
                      center if per_slot is None else per_slot[idx]).submit() for r, idx in by_radius.items()]
        return jobs[0] if len(jobs) == 1 else jobs

    def prune_voxel_maps(self, seqs=None, **kw):
        """submit_prune + wait"""
        job = self.submit_prune(seqs, **kw)
        self.wait()
        return job

    def submit_carve(self, margin, seqs=None, near=0.01, ring=1, max_last=0xFFFFFFFF, drop_flags=0, keep=None, lr_check=None, step=4, win=0,
                     search_x=0, search_y=0, min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0, sgm=None):
        """svo_submit_carve_voxel_maps: queue a carve of the voxel maps of the slots `seqs` (None: all) behind what was
        submitted so far; nothing is waited for. An entry leaves when the dense depth of the slot's current frame (the
        occluder of export_ar's occlusion: submit_cloud's step, win, search_x, search_y, the filter, lr_check, sgm, in the
        camera frame) measures a surface more than `margin` behind it along its ray, in its lattice cell and, with
        ring = 1, in every neighbour of the cell; entries nearer than `near`, fused after stamp `max_last` or without
        complete evidence stay. keep: a dict of min_count, min_stamp, radius (in voxels) and center ("pose" or xyz)
        for a keep rule of the prune applied with it; None: none. Returns a Carve, valid after its wait() (or the
        ctx's)."""
        sgm = hip_lib.sgm_consumer(sgm, lr_check, "submit_carve")
        style = hip_lib.cloud_style(step, win, search_x, search_y, "camera", "compact", min_disparity, max_depth, max_mean_cost)
        keep = dict(keep or {})
        center = keep.pop("center", "pose")
        radius = keep.pop("radius", None)
        rule = None if not keep and radius is None else hip_lib.voxel_keep(radius=-1 if radius is None else int(radius), **keep)
        params, check = sgm if sgm[0] is not None else (None, self._stereo_check(lr_check))
        return Carve(self, seqs, style, check, params, hip_lib.voxel_carve(margin, near, ring, max_last, drop_flags), rule,
                     center if radius is not None else None).submit()

    def carve_voxel_maps(self, margin, seqs=None, **kw):
        """submit_carve + wait"""
        job = self.submit_carve(margin, seqs, **kw)
        self.wait()
        return job

    def clear_voxel_maps(self, seqs=None, wait=True):
        """svo_submit_clear_voxel_maps: queued; the maps of the slots `seqs` (None: all) become empty"""
        seqs, n, arr = named_slots(self, seqs)
        _check(lib().svo_submit_clear_voxel_maps(self._ctx, arr, n))
        self._forget_fused(seqs)
        if wait:
            self.wait()

    def memory(self):
        m = Memory()
        _check(lib().svo_ctx_get_memory(self._ctx, C.byref(m)))
        return m

    def groups(self):
        n = C.c_int(0)
        _check(lib().svo_ctx_get_groups(self._ctx, C.byref(n)))
        return n.value

    def totals(self):
        t = Totals()
        _check(lib().svo_get_totals(self._ctx, C.byref(t)))
        return t

    def launch_shapes(self):
        """svo_ctx_get_launch_shapes: {(kernel name, waves, mode, cap): launches} of the alignment
        and reprojection-GN kernels, summed over the groups since creation."""
        n = C.c_int(0)
        _check(lib().svo_ctx_get_launch_shapes(self._ctx, None, 0, C.byref(n)))
        out = (LaunchShape * max(n.value, 1))()
        _check(lib().svo_ctx_get_launch_shapes(self._ctx, out, n.value, C.byref(n)))
        return {_shape_key(e): e.launches for e in out[:n.value]}

    def pose(self, seq=0):
        p = np.zeros(6, np.float32)
        _check(lib().svo_get_pose(self._ctx, seq, p.ctypes.data_as(C.c_void_p)))
        return p

    def stats(self, seq=0):
        st = FrameStats()
        _check(lib().svo_get_frame_stats(self._ctx, seq, C.byref(st)))
        return st

    def get_frame(self, seq=0):
        n = C.c_int(0)
        _check(lib().svo_get_frame_keypoints(self._ctx, seq, None, None, None, 0, C.byref(n)))
        k2 = np.zeros((n.value, 2), np.float32)
        k3 = np.zeros((n.value, 3), np.float32)
        info = np.zeros(n.value, KP_INFO_DTYPE)
        _check(lib().svo_get_frame_keypoints(self._ctx, seq, k2.ctypes.data_as(C.c_void_p),
                                             k3.ctypes.data_as(C.c_void_p),
                                             info.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return Frame(self.pose(seq), k2, k3, info)

    def num_keyframes(self, seq=0):
        n = C.c_int(0)
        _check(lib().svo_get_keyframe_count(self._ctx, seq, C.byref(n)))
        return n.value

    def get_keyframe(self, kid=None, seq=0):
        if kid is None:
            kid = self.num_keyframes(seq) - 1
        n = C.c_int(0)
        pose = np.zeros(6, np.float32)
        _check(lib().svo_get_keyframe(self._ctx, seq, kid, None, None, None,
                                      pose.ctypes.data_as(C.c_void_p), 0, C.byref(n)))
        k2 = np.zeros((n.value, 2), np.float32)
        k3 = np.zeros((n.value, 3), np.float32)
        info = np.zeros(n.value, KP_INFO_DTYPE)
        _check(lib().svo_get_keyframe(self._ctx, seq, kid, k2.ctypes.data_as(C.c_void_p),
                                      k3.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p),
                                      pose.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return Frame(pose, k2, k3, info)

    def get_keyframes(self, seq=0):
        """the resident keyframes, oldest first: ids keyframe_range(seq).first .. num_keyframes(seq) - 1"""
        return [self.get_keyframe(i, seq) for i in range(self.keyframe_range(seq).first, self.num_keyframes(seq))]

    def get_trajectory(self, seq=0):
        n = C.c_int(0)
        _check(lib().svo_get_trajectory(self._ctx, seq, None, 0, C.byref(n)))
        out = np.zeros((n.value, 6), np.float32)
        _check(lib().svo_get_trajectory(self._ctx, seq, out.ctypes.data_as(C.c_void_p), n.value,
                                        C.byref(n)))
        return out

    def update_pose(self, pose, speed, pose_variance, speed_variance, dt, seq=0):
        out = np.zeros(6, np.float32)
        arrs = [np.ascontiguousarray(a, np.float32) for a in (pose, speed, pose_variance, speed_variance)]
        _check(lib().svo_update_pose(self._ctx, seq, *[a.ctypes.data_as(C.c_void_p) for a in arrs],
                                     C.c_double(dt), out.ctypes.data_as(C.c_void_p)))
        return out


    # -- batched pose-filter updates ----------------------------------------
    IMU_RATE = 104.0                              # samples per second of the Econ camera's IMU thread (slam_app.cpp:127)

    def submit_pose_updates(self, seqs, samples_per_seq):
        """svo_submit_pose_updates: queue the pose-filter updates of the slots `seqs` (None: all, in order) behind
        what was submitted so far; nothing is waited for. samples_per_seq[i]: the POSE_SAMPLE_DTYPE records of slot
        seqs[i] in the order they are applied (an empty array or None: the slot is left alone). Returns the filtered
        poses, float32 [total, 6] in sample order, valid after wait()."""
        _, n, seq_arr = named_slots(self, seqs)
        assert len(samples_per_seq) == n
        per = [np.zeros(0, POSE_SAMPLE_DTYPE) if a is None else np.ascontiguousarray(a, POSE_SAMPLE_DTYPE).reshape(-1)
               for a in samples_per_seq]
        counts = int_array([len(a) for a in per])
        samples = np.concatenate(per) if per else np.zeros(0, POSE_SAMPLE_DTYPE)
        filtered = np.zeros((len(samples), 6), np.float32)
        _check(lib().svo_submit_pose_updates(self._ctx, seq_arr, counts, n, samples.ctypes.data if len(samples) else None,
                                             filtered.ctypes.data if len(samples) else None))
        return filtered                            # (the worker writes into it: the caller keeps it until wait())

    def update_poses(self, seqs, samples_per_seq):
        """submit_pose_updates + wait: the filtered poses [total, 6]"""
        out = self.submit_pose_updates(seqs, samples_per_seq)
        self.wait()
        return out

    @classmethod
    def gyro_samples(cls, gyro_deg_s, dt):
        """SlamApp::update_pose_from_imu (slam_app.cpp:111-135) of one frame interval as chained samples: at most
        IMU_RATE * dt of the gyro rates ([n, 3] degrees per second, x y z) as the speed measurement with the app's
        variances, each one update of 1 / IMU_RATE (the double)"""
        gyro = np.asarray(gyro_deg_s, np.float32).reshape(-1, 3)
        n = min(len(gyro), int(np.float32(cls.IMU_RATE) * np.float32(dt)))     # std::min<size_t>(size, f * dt): truncated
        out = np.zeros(n, POSE_SAMPLE_DTYPE)
        out["speed"][:, 3:] = (gyro[:n].astype(np.float64) / 180.0 * np.pi).astype(np.float32)
        out["pose_var"] = 1000.0
        out["speed_var"] = np.array([100.0, 100.0, 100.0, 0.1, 0.1, 0.1], np.float32)
        out["dt"] = 1.0 / cls.IMU_RATE
        out["flags"] = POSE_SAMPLE_CHAIN
        return out

    def submit_poses_from_gyro(self, gyro_per_seq, dt, seqs=None):
        """gyro_samples of every named slot (gyro_per_seq[i]: [n_i, 3] or None) as one submit_pose_updates"""
        return self.submit_pose_updates(seqs, [None if g is None else self.gyro_samples(g, dt) for g in gyro_per_seq])

    def update_poses_from_gyro(self, gyro_per_seq, dt, seqs=None):
        """the app's IMU loop between two frames for many slots in one call, without a round trip per sample:
        submit_poses_from_gyro + wait. Returns the filtered poses [total, 6]."""
        out = self.submit_poses_from_gyro(gyro_per_seq, dt, seqs)
        self.wait()
        return out


class StereoSlam(StereoSlamBatch):
    """One sequence: the reference's StereoSlam."""

    def __init__(self, camera_settings, width=None, height=None, device=0):
        self._pending = (camera_settings, device)
        self._ctx = None
        self.ar_visibility = None          # get_ar with occlusion: the last picture's counts
        if width is not None:
            super().__init__(camera_settings, width, height, 1, device)

    def set_input_format(self, fmt):
        if self._ctx is None:              # (kept until the first frame makes the ctx)
            self._format = hip_lib.INPUT_FORMATS.index(fmt) if isinstance(fmt, str) else int(fmt)
            hip_lib.input_format_info(self._format, 1)
        else:
            super().set_input_format(fmt)

    def set_keyframe_window(self, keep):
        if self._ctx is None:              # (kept until the first frame makes the ctx)
            self._window = int(keep)
        else:
            super().set_keyframe_window(keep)

    def new_image(self, left, right=None, time_stamp=0.0):
        """one frame; with a one-buffer input format `left` is the frame and `right` is ignored"""
        if self._ctx is None:   # the reference learns the image size from the first frame
            cam, device = self._pending
            h, w = left.shape[:2]
            if getattr(self, "_format", 0):
                w //= hip_lib.input_format_info(self._format, 1).min_row_pixels   # (side by side: half the frame)
            super().__init__(cam, w, h, 1, device)
            if getattr(self, "_format", 0):
                super().set_input_format(self._format)
            if getattr(self, "_fast", False):
                self.set_fast_solver(True)
            if getattr(self, "_timing", False):
                self.enable_timing(True)
            if getattr(self, "_rect", None) is not None:
                self._apply_rectification()
            if getattr(self, "_window", -1) >= 0:
                super().set_keyframe_window(self._window)
        self.new_images([left], [right], [time_stamp])

    def _get(self, export, pick, *args, **kw):
        """what the get_* share: None without a ctx; else the host-mode job `export` of the one slot, and a copy of what
        `pick` takes from it (None when there is none)"""
        if self._ctx is None:
            return None
        kw["device"] = False
        out = pick(export(*args, **kw))
        return None if out is None else out.copy()

    def get_image(self, what="frames", **kw):
        """the image of the current frame (or, what="last_keyframes", of the newest keyframe) as a numpy array
        (export_views of the one slot: plane, level, pixel, markers, ...); None when there is none"""
        return self._get(self.export_views, lambda job: job.image(0), what, None, **kw)

    def get_disparity(self, what="frames", **kw):
        """the dense disparity (or, value="depth", depth) map of the current frame (or, what="last_keyframes", of the
        newest keyframe) as a numpy array [planes, rows, cols] (export_disparity of the one slot: value, step, win,
        search_x, search_y, cost); None when there is none"""
        return self._get(self.export_disparity, lambda job: job.planes(0), what, None, **kw)

    def get_cloud(self, what="frames", **kw):
        """the dense coloured point cloud of the current frame (or, what="last_keyframes", of the newest keyframe) as
        a numpy array of hip_lib.MAP_POINT_DTYPE (export_cloud of the one slot: step, frame, layout, the filter, ...;
        layout="organized": [rows, cols]); None when there is none"""
        def pick(job):
            return job.organized(0) if job.style.layout == hip_lib.CLOUD_ORGANIZED else job.points(0)
        return self._get(self.export_cloud, pick, what, None, **kw)

    def prune_voxel_map(self, **kw):
        """prune_voxel_maps of the one slot (min_count, min_stamp, radius in metres, center="pose" or xyz): its record
        of hip_lib.PRUNE_INFO_DTYPE"""
        return self.prune_voxel_maps([0], **kw).info[0].copy()

    def carve_voxel_map(self, margin, **kw):
        """carve_voxel_maps of the one slot (margin, near, ring, max_last, keep, step, sgm, lr_check, ...): its record of
        hip_lib.CARVE_INFO_DTYPE"""
        return self.carve_voxel_maps(margin, [0], **kw).info[0].copy()

    def get_voxel_map(self, **kw):
        """the slot's voxel map as a numpy array of hip_lib.MAP_POINT_DTYPE in key order (export_voxel_maps of the one
        slot: min_count, min_stamp); None without a map"""
        return self._get(self.export_voxel_maps, lambda job: job.points(0), None, **kw)

    def save_voxel_map(self, **kw):
        """the slot's voxel map as a VoxelSaves (save_voxel_maps of the one slot): entries(0), tobytes(0)"""
        return self.save_voxel_maps([0], **kw)

    def load_voxel_map(self, save, merge=False, **kw):
        """load_voxel_maps of the one slot from a VoxelSaves (or entry records with voxel=): its record of
        hip_lib.VOXEL_LOAD_INFO_DTYPE"""
        return self.load_voxel_maps([0], save if isinstance(save, VoxelSaves) else [save], merge=merge, **kw).info[0].copy()

    def resize_voxel_map(self, log2_capacity):
        """resize_voxel_maps of the one slot"""
        self.resize_voxel_maps(log2_capacity, [0])

    def get_scene(self, camera="front", **kw):
        """the viewer's 3-D picture of the map as a numpy array [rows, cols, 3 | 4] (export_scenes of the one slot:
        camera, cols, rows, pixel, show, ...; dense=dict(...) draws the current frame's dense cloud into it); None before
        the first frame"""
        return self._get(self.export_scenes, lambda job: job.image(0), None, camera=camera, **kw)

    def get_ar(self, objects, **kw):
        """the AR demo's picture of the current frame as a numpy array [height, width, 3 | 4] (export_ar of the one
        slot: pixel, light, ambient, near). objects: (vertices, triangles, model of 12 floats, rgb) each, e.g.
        (*hip_lib.ar_box(0.2), hip_lib.ar_model(hip_lib.AR_AT), 0xc08040). occlusion = dict(...) (submit_ar) hides
        the objects behind the frame's dense stereo depth. None before the first frame"""
        meshes = [(v, t) for v, t, _, _ in objects]
        instances = [(model, i, rgb) for i, (_, _, model, rgb) in enumerate(objects)]

        def pick(job):
            # (with occlusion: the picture's hip_lib.AR_VISIBILITY_DTYPE record, for whoever wants the counts)
            self.ar_visibility = None if job.visibility is None else job.visibility[0].copy()
            return job.image(0)
        return self._get(self.export_ar, pick, meshes, instances, None, **kw)
