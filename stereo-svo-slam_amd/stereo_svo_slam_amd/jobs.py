"""The objects behind the ctx's queued jobs (svo_submit_*, include/svo_hip.h): each owns the buffers the library writes
until the job is delivered, and queues the same job again with submit(). `Job` is what they share, the way
csrc/svo_ctx_state.hpp is for the entries they call: the named slots, the per-slot records, the destination in pinned or
device memory, submit() and wait(). `Frame` and `Snapshot` are the plain values of the getters and of save / load.
StereoSlamBatch (stereo_slam.py) makes all of them. No compute happens in Python.
"""
import ctypes as C

import numpy as np
import torch

from . import hip_lib
from .hip_lib import SvoError, _check, lib

KP_INFO_DTYPE = np.dtype([
    ("score", "<f4"), ("level", "<i4"), ("type", "<i4"), ("keyframe_id", "<i4"),
    ("keypoint_index", "<i4"), ("color", "u1", (3,)), ("ignore_during_refinement", "u1"),
    ("ignore_completely", "u1"), ("ignore_temporary", "u1"), ("_pad", "u1", (2,)),
    ("outlier_count", "<i4"), ("inlier_count", "<i4"), ("kf_inv_depth", "<f4"),
    ("kf_variance", "<f4")], align=False)
assert KP_INFO_DTYPE.itemsize == 44


def int_array(values):
    """a C int array of `values` (one element at least, so that an empty list still has an address)"""
    return (C.c_int * max(len(values), 1))(*values)


def named_slots(slam, seqs, explicit=False):
    """(seqs, n, array) of a call that names slots of `slam`: seqs as a list of ints, their number and the C int array the
    entry takes. seqs=None stands for every slot in order: (None, slam.n, None), or with explicit=True the list
    0 .. slam.n - 1 spelled out."""
    if seqs is None:
        if not explicit:
            return None, slam.n, None
        seqs = range(slam.n)
    seqs = [int(s) for s in seqs]
    return seqs, len(seqs), int_array(seqs)


def caller_memory(device, on_device):
    """the SVO_MEM_* constant for buffers of the caller's in device (on_device) or host memory; for device memory the
    caller's current stream is synchronised first, so that nothing of theirs is still using the tensors"""
    if on_device:
        torch.cuda.current_stream(device).synchronize()
        return hip_lib.MEM_DEVICE
    return hip_lib.MEM_HOST


class Frame:
    """Frame / KeyFrame (src/include/stereo_slam_types.hpp:117-131) without images."""

    def __init__(self, pose, kps2d, kps3d, info):
        self.pose = pose
        self.kps2d = kps2d
        self.kps3d = kps3d
        self.info = info


class Job:
    """What the queued jobs share. A subclass names its slots with _name(), makes its buffers and gives _call(ctx, mem):
    the one library call of the job."""

    EXPLICIT_SLOTS = False             # seqs=None travels as NULL, not as the list 0 .. n - 1

    def _name(self, slam, seqs, device=False):
        """_slam, device_mode and the named slots (seqs, _n, _seq_arr); returns their number"""
        self._slam, self.device_mode = slam, bool(device)
        self.seqs, self._n, self._seq_arr = named_slots(slam, seqs, self.EXPLICIT_SLOTS)
        return self._n

    def _per_slot(self, dtype):
        """(array, view) of one zeroed record per named slot: the array has one record at least (its address goes to
        the library), the view exactly the named ones"""
        a = np.zeros(max(self._n, 1), dtype)
        return a, a[:self._n]

    def _segments(self, dtype):
        self._seg, self.segments = self._per_slot(dtype)

    def _alloc(self, shape, dtype, make=torch.zeros):
        """the destination: on the ctx's device in device mode, pinned host memory otherwise"""
        if self.device_mode:
            return make(shape, dtype=dtype, device=self._slam.device)
        return make(shape, dtype=dtype, pin_memory=True)

    def submit(self):
        """queue the job (again: the same slots into the same buffers, once the previous one is delivered)"""
        _check(self._call(self._slam._ctx, caller_memory(self._slam.device, self.device_mode)))
        return self

    def wait(self):
        self._slam.wait()
        return self


class PictureJob(Job):
    """A job of one picture per named slot: `pixels` is the whole buffer, a numpy uint8 view of pinned memory in host
    mode, a torch uint8 tensor on the ctx's device in device mode. A subclass sets cols, rows, pitch, image_bytes and
    channels before _pictures(), and OK: the status of a slot that has a picture."""

    GRAY_IS_2D = False                 # one channel: [rows, cols, 1] (True: [rows, cols])

    def _pictures(self, seg_dtype, dst_type):
        self.capacity = self._n * self.image_bytes
        self._segments(seg_dtype)
        self._buf = self._alloc(max(self.capacity, 4), torch.uint8)
        self._dst = dst_type(self._seg.ctypes.data, self._buf.data_ptr(), self.capacity)

    @property
    def pixels(self):
        return self._buf if self.device_mode else self._buf.numpy()

    def image(self, i):
        """the image of named slot i: [rows, cols, channels] (a Views' gray8: [rows, cols]), a view of `pixels` (numpy in
        host mode, a torch tensor in device mode); None for a slot whose status is not OK (it has no picture)"""
        e = self.segments[i]
        if int(e["status"]) != self.OK:
            return None
        lo = int(e["offset"])
        shape = (self.rows, self.cols) + (() if self.channels == 1 and self.GRAY_IS_2D else (self.channels,))
        return self.pixels[lo:lo + self.rows * self.pitch].reshape(shape)


class PointJob(Job):
    """A job that delivers hip_lib.MAP_POINT_DTYPE records: `points_buffer` is a uint8 [capacity, 16] tensor, pinned
    memory in host mode, on the ctx's device in device mode."""

    def _points(self, make=torch.zeros):
        self.points_buffer = self._alloc((max(self.capacity, 1), hip_lib.MAP_POINT_DTYPE.itemsize), torch.uint8, make)

    def _records(self, lo, n):
        """records [lo, lo + n) as numpy (device mode copies them to the host)"""
        a = self.points_buffer[lo:lo + n]
        a = a.cpu().numpy() if self.device_mode else a.numpy()
        return a.view(hip_lib.MAP_POINT_DTYPE)[:, 0]


class Export(Job):
    """One svo_submit_export: keeps the buffers the library writes alive. After wait(): `segments`
    (hip_lib.EXPORT_SEGMENT_DTYPE, one per named slot) and the record arrays kps2d [capacity, 2] float32,
    kps3d [capacity, 3] float32 and info — numpy views of pinned memory (info: KP_INFO_DTYPE [capacity]) in host
    mode, torch tensors on the ctx's device (info: uint8 [capacity, 44]) in device mode; None for a field that
    was not asked for. Slot i's keypoints are records [segments[i].first, + segments[i].n) of every array.
    Unlike the other jobs' its segments live in a torch tensor, and its record arrays start uninitialised."""

    def __init__(self, slam, what, seqs, device, fields):
        n = self._name(slam, seqs, device)
        self.what = what
        self.capacity = n * slam.export_capacity()
        self._seg = torch.zeros(max(n, 1) * hip_lib.EXPORT_SEGMENT_DTYPE.itemsize, dtype=torch.uint8)
        self.segments = self._seg.numpy().view(hip_lib.EXPORT_SEGMENT_DTYPE)[:n]
        shapes = {"kps2d": ((self.capacity, 2), torch.float32), "kps3d": ((self.capacity, 3), torch.float32),
                  "info": ((self.capacity, KP_INFO_DTYPE.itemsize), torch.uint8)}
        assert set(fields) <= set(shapes), fields
        self._bufs = {name: self._alloc(*shapes[name], make=torch.empty) for name in fields}
        self._dst = hip_lib.ExportDst(self._seg.data_ptr(), *[
            self._bufs[name].data_ptr() if name in self._bufs else None for name in ("kps2d", "kps3d", "info")],
            self.capacity)

    def _field(self, name):
        t = self._bufs.get(name)
        if t is None or self.device_mode:
            return t
        a = t.numpy()
        return a.view(KP_INFO_DTYPE)[:, 0] if name == "info" else a

    kps2d = property(lambda self: self._field("kps2d"))
    kps3d = property(lambda self: self._field("kps3d"))
    info = property(lambda self: self._field("info"))

    def _call(self, ctx, mem):
        return lib().svo_submit_export(ctx, self.what, self._seq_arr, self._n, C.byref(self._dst), mem)

    def frame(self, i):
        """segment i as a Frame (what get_frame / get_keyframe return); a field that was not exported is None.
        Device mode copies the segment's records to the host."""
        e = self.segments[i]
        lo, hi = int(e["first"]), int(e["first"]) + int(e["n"])
        out = []
        for name in ("kps2d", "kps3d", "info"):
            a = self._field(name)
            if a is not None:
                a = a[lo:hi]
                if self.device_mode:
                    a = a.cpu().numpy()
                    if name == "info":
                        a = a.view(KP_INFO_DTYPE)[:, 0]
                a = a.copy()
            out.append(a)
        return Frame(np.array(e["pose"], np.float32), *out)


class MapExport(PointJob):
    """One svo_submit_export_map: owns the buffers the library writes. `regions` (hip_lib.MAP_REGION_DTYPE, one per
    named slot: where the slot goes and from which keyframe on) are laid out here, densely in named order, from the
    capacities given, unless an array of them is passed. After wait(): `segments` (hip_lib.MAP_SEGMENT_DTYPE, one
    per named slot), keyframes(i), points(i) and points_of_keyframe(i, k). The points are a numpy view
    (hip_lib.MAP_POINT_DTYPE) of pinned memory in host mode, `points_buffer` a uint8 [capacity, 16] tensor on the
    ctx's device in device mode (points(i) then copies the slot's records to the host). The points start
    uninitialised, like an Export's records."""

    EXPLICIT_SLOTS = True              # (`seqs` is always the list: the regions go with it, one by one)

    def __init__(self, slam, seqs=None, from_keyframe=None, filter=None, device=False, point_capacity=0,
                 keyframe_capacity=0, regions=None):
        self._name(slam, seqs, device)
        self.filter = hip_lib.map_filter(filter)
        self.regions = self._per_slot(hip_lib.MAP_REGION_DTYPE)[1]
        if regions is not None:
            self.regions[:] = regions
        else:
            self.regions["from_keyframe"] = 0 if from_keyframe is None else from_keyframe
            self.regions["point_capacity"] = point_capacity
            self.regions["keyframe_capacity"] = keyframe_capacity
            self._place()
        self._segments(hip_lib.MAP_SEGMENT_DTYPE)
        self._allocate()

    def _place(self):
        """every slot behind the one named before it"""
        r = self.regions
        r["first_point"] = np.cumsum(r["point_capacity"]) - r["point_capacity"]
        r["first_keyframe_entry"] = np.cumsum(r["keyframe_capacity"]) - r["keyframe_capacity"]

    def _allocate(self):
        r = self.regions
        self.capacity = int((r["first_point"] + r["point_capacity"]).max()) if self._n else 0
        entries = int((r["first_keyframe_entry"] + r["keyframe_capacity"]).max()) if self._n else 0
        self._kfs = np.zeros(max(entries, 1), hip_lib.MAP_KEYFRAME_DTYPE)
        self._points(torch.empty)
        self._dst = hip_lib.MapDst(self._seg.ctypes.data, self._kfs.ctypes.data if entries else None,
                                   self.points_buffer.data_ptr() if self.capacity else None)

    def _call(self, ctx, mem):
        return lib().svo_submit_export_map(ctx, self._seq_arr, self._n, self.regions.ctypes.data_as(C.c_void_p),
                                           C.byref(self.filter), C.byref(self._dst), mem)

    def grow(self):
        """after wait(): every slot that came back MAP_TOO_SMALL gets the capacities its segment asks for, the regions
        are laid out again and new buffers made. False: every slot was delivered and nothing changed."""
        small = self.segments["status"] == hip_lib.MAP_TOO_SMALL
        if not small.any():
            return False
        r = self.regions
        r["point_capacity"] = np.where(small, np.maximum(r["point_capacity"], self.segments["points_bound"]), r["point_capacity"])
        r["keyframe_capacity"] = np.where(small, np.maximum(r["keyframe_capacity"], self.segments["n_exported"]), r["keyframe_capacity"])
        self._place()
        self._allocate()
        return True

    def keyframes(self, i):
        """the svo_map_keyframe entries (hip_lib.MAP_KEYFRAME_DTYPE) of named slot i; none for a slot that was not delivered"""
        e, r = self.segments[i], self.regions[i]
        n = int(e["n_exported"]) if e["status"] == hip_lib.MAP_COMPLETE else 0
        return self._kfs[int(r["first_keyframe_entry"]):int(r["first_keyframe_entry"]) + n]

    def first_keyframe(self, i):
        """svo_map_segment.first_keyframe of named slot i: its oldest resident keyframe when the job ran"""
        return hip_lib.map_first_keyframe(self.segments[i])

    def points(self, i):
        """the kept points of named slot i (hip_lib.MAP_POINT_DTYPE), keyframe after keyframe"""
        return self._records(int(self.regions[i]["first_point"]), int(self.segments[i]["n_points"]))

    def points_of_keyframe(self, i, k):
        """the kept points of the k-th exported keyframe of named slot i"""
        kf = self.keyframes(i)[k]
        return self._records(int(kf["first"]), int(kf["n"]))


class Views(PictureJob):
    """One svo_submit_export_views: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.VIEW_SEGMENT_DTYPE, one per named slot), image(i) and `pixels` (PictureJob). cols, rows, pitch,
    image_bytes: the shape of every image of the job (svo_view_size); channels: 1, 3 or 4."""

    OK, GRAY_IS_2D = hip_lib.VIEW_OK, True

    def __init__(self, slam, what, seqs, style, device):
        self._name(slam, seqs, device)
        self.what, self.style = int(what), style
        self.cols, self.rows, self.pitch, self.image_bytes = slam.view_size(style)
        self.channels = hip_lib.PIXEL_BYTES[style.pixel]
        self._pictures(hip_lib.VIEW_SEGMENT_DTYPE, hip_lib.ViewDst)

    def _call(self, ctx, mem):
        return lib().svo_submit_export_views(ctx, self.what, self._seq_arr, self._n, C.byref(self.style), C.byref(self._dst), mem)


SGM_AND_LR_CHECK = ("lr_check= is the cross-check of the winner-takes-all search; the cross-check of an SGM job is the "
                    "lr_check key of its sgm dict, e.g. sgm=dict(hip_lib.SGM_DEFAULTS, lr_check=1.0)")


def _check_that_is_on(check):
    """a hip_lib.StereoCheck that is on, or None: a job without one goes through the unchecked entry"""
    return check if check is not None and check.lr else None


class Disparities(Job):
    """One svo_submit_export_disparity: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.DISPARITY_SEGMENT_DTYPE, one per named slot), `values` [slots, planes, rows, cols] float32 (a strided view
    of the buffer: numpy over pinned memory in host mode, a torch tensor on the ctx's device in device mode; a slot
    whose status is DISPARITY_NONE keeps what the buffer held) and planes(i). cols, rows, planes, image_bytes: the shape
    of every slot of the job (svo_disparity_size). A checked job (check: a hip_lib.StereoCheck that is on) goes through
    svo_submit_export_disparity_checked; its last plane is the lr plane, lr(i). An SGM job (sgm: a hip_lib.SgmParams)
    goes through svo_submit_export_disparity_sgm: the same planes with semi-global aggregation and sub-pixel values;
    with sgm_check (a StereoCheck that is on: the cross-check of the SGM map, the lr_check key of the sgm dict) through
    svo_submit_export_disparity_sgm_checked, and lr(i) is its lr plane. sgm together with a top-level check that is
    on raises ValueError: the two checks are different rules."""

    def __init__(self, slam, what, seqs, style, device, check=None, sgm=None, sgm_check=None):
        n = self._name(slam, seqs, device)
        self.what, self.style, self.check, self.sgm = int(what), style, _check_that_is_on(check), sgm
        if self.check is not None and sgm is not None:
            raise ValueError(SGM_AND_LR_CHECK)
        if sgm is not None:
            self.check = _check_that_is_on(sgm_check)
        self.cols, self.rows, self.n_planes, self.image_bytes = slam.disparity_size(style, self.check)
        self.capacity = n * self.image_bytes
        self._segments(hip_lib.DISPARITY_SEGMENT_DTYPE)
        self._buf = self._alloc(max(self.capacity // 4, 4), torch.float32)
        self._dst = hip_lib.DisparityDst(self._seg.ctypes.data, self._buf.data_ptr(), self.capacity)

    @property
    def values(self):
        plane = self.rows * self.cols
        v = torch.as_strided(self._buf, (self._n, self.n_planes, self.rows, self.cols), (self.image_bytes // 4, plane, self.cols, 1))
        return v if self.device_mode else v.numpy()

    def _call(self, ctx, mem):
        if self.sgm is not None and self.check is not None:
            return lib().svo_submit_export_disparity_sgm_checked(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                                                 C.byref(self.sgm), C.byref(self.check), C.byref(self._dst), mem)
        if self.sgm is not None:
            return lib().svo_submit_export_disparity_sgm(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                                         C.byref(self.sgm), C.byref(self._dst), mem)
        if self.check is None:
            return lib().svo_submit_export_disparity(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                                     C.byref(self._dst), mem)
        return lib().svo_submit_export_disparity_checked(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                                         C.byref(self.check), C.byref(self._dst), mem)

    def planes(self, i):
        """the planes of named slot i: [planes, rows, cols], a view of `values`; None for a slot whose status is
        DISPARITY_NONE"""
        if int(self.segments[i]["status"]) != hip_lib.DISPARITY_OK:
            return None
        return self.values[i]

    def lr(self, i):
        """the lr plane of named slot i of a checked job ([rows, cols]: -1 invalid, -2 no way back, else the
        left-right difference); None for an unchecked job or a slot whose status is DISPARITY_NONE"""
        planes = self.planes(i)
        return None if planes is None or self.check is None else planes[-1]


class Clouds(PointJob):
    """One svo_submit_export_cloud: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.CLOUD_SEGMENT_DTYPE, one per named slot), points(i) and, in the organized layout, organized(i).
    `points_buffer`: PointJob (points(i) / organized(i) copy a device-mode slot's records to the host). cols, rows,
    points_per_slot: the lattice of every slot of the job (svo_cloud_size). A checked job (check: a hip_lib.StereoCheck
    that is on) goes through svo_submit_export_cloud_checked. An SGM job (sgm: a hip_lib.SgmParams; sgm_check: the
    cross-check of the SGM map, or None) goes through svo_submit_export_cloud_sgm; sgm together with a top-level check
    that is on raises ValueError."""

    def __init__(self, slam, what, seqs, style, device, check=None, sgm=None, sgm_check=None):
        n = self._name(slam, seqs, device)
        self.what, self.style, self.check, self.sgm = int(what), style, _check_that_is_on(check), sgm
        if self.check is not None and sgm is not None:
            raise ValueError(SGM_AND_LR_CHECK)
        if sgm is not None:
            self.check = _check_that_is_on(sgm_check)
        self.cols, self.rows, self.points_per_slot = slam.cloud_size(style)
        self.capacity = n * self.points_per_slot
        self._segments(hip_lib.CLOUD_SEGMENT_DTYPE)
        self._points()
        self._dst = hip_lib.CloudDst(self._seg.ctypes.data, self.points_buffer.data_ptr(), self.capacity)

    def _call(self, ctx, mem):
        if self.sgm is not None:
            return lib().svo_submit_export_cloud_sgm(ctx, self.what, self._seq_arr, self._n, C.byref(self.style), C.byref(self.sgm),
                                                     None if self.check is None else C.byref(self.check), C.byref(self._dst), mem)
        if self.check is None:
            return lib().svo_submit_export_cloud(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                                 C.byref(self._dst), mem)
        return lib().svo_submit_export_cloud_checked(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                                     C.byref(self.check), C.byref(self._dst), mem)

    def points(self, i):
        """the kept points of named slot i (hip_lib.MAP_POINT_DTYPE) in row-major lattice order; None for a slot whose
        status is CLOUD_NONE. In the organized layout: the records without CLOUD_DROPPED, a copy."""
        e = self.segments[i]
        if int(e["status"]) != hip_lib.CLOUD_OK:
            return None
        if self.style.layout == hip_lib.CLOUD_ORGANIZED:
            r = self._records(int(e["first_point"]), self.points_per_slot)
            return r[(r["flags"] & hip_lib.CLOUD_DROPPED) == 0]
        return self._records(int(e["first_point"]), int(e["n_points"]))

    def organized(self, i):
        """the records of named slot i as [rows, cols] (organized layout only); None for a slot whose status is
        CLOUD_NONE"""
        if self.style.layout != hip_lib.CLOUD_ORGANIZED:
            raise ValueError("organized(): the job's layout is compact")
        e = self.segments[i]
        if int(e["status"]) != hip_lib.CLOUD_OK:
            return None
        return self._records(int(e["first_point"]), self.points_per_slot).reshape(self.rows, self.cols)


class Fusion(Job):
    """One svo_submit_fuse_clouds: owns the info the library writes. After wait(): `info` (hip_lib.FUSE_INFO_DTYPE, one
    per named slot). Its submit() queues the same job again (the same slots, style and stamp). Nothing of the caller's
    goes in or out on the device: it is a host-mode job, and its submit() never synchronises a stream. An SGM job (sgm:
    a hip_lib.SgmParams; sgm_check: the cross-check of the SGM map, or None) goes through svo_submit_fuse_clouds_sgm;
    sgm together with a top-level check that is on raises ValueError."""

    def __init__(self, slam, what, seqs, style, check, stamp, sgm=None, sgm_check=None):
        self._name(slam, seqs)
        self.what, self.style, self.stamp, self.check, self.sgm = int(what), style, int(stamp), _check_that_is_on(check), sgm
        if self.check is not None and sgm is not None:
            raise ValueError(SGM_AND_LR_CHECK)
        if sgm is not None:
            self.check = _check_that_is_on(sgm_check)
        self._info, self.info = self._per_slot(hip_lib.FUSE_INFO_DTYPE)

    def _call(self, ctx, mem):
        if self.sgm is not None:
            return lib().svo_submit_fuse_clouds_sgm(ctx, self.what, self._seq_arr, self._n, C.byref(self.style), C.byref(self.sgm),
                                                    None if self.check is None else C.byref(self.check), self.stamp,
                                                    self._info.ctypes.data)
        return lib().svo_submit_fuse_clouds(ctx, self.what, self._seq_arr, self._n, C.byref(self.style),
                                            None if self.check is None else C.byref(self.check), self.stamp, self._info.ctypes.data)


class Prune(Job):
    """One svo_submit_prune_voxel_maps: owns the info the library writes and the centres it reads at the call. After
    wait(): `info` (hip_lib.PRUNE_INFO_DTYPE, one per named slot). keep: a hip_lib.VoxelKeep (its center is used where
    `centers` is None); centers: "pose" (each slot's camera centre when the job runs) or one xyz per named slot. Its
    submit() queues the same job again. A host-mode job: its submit() never synchronises a stream."""

    def __init__(self, slam, seqs, keep, centers):
        n = self._name(slam, seqs)
        self.keep = keep
        self.center_mode = hip_lib.PRUNE_CENTER_POSE if isinstance(centers, str) else hip_lib.PRUNE_CENTER_GIVEN
        if isinstance(centers, str) and centers != "pose":
            raise ValueError(f"centers is 'pose' or coordinates, not {centers!r}")
        self.centers = None
        if self.center_mode == hip_lib.PRUNE_CENTER_GIVEN and centers is not None:
            self.centers = np.ascontiguousarray(np.broadcast_to(np.asarray(centers, np.float32), (n, 3)))
        self._info, self.info = self._per_slot(hip_lib.PRUNE_INFO_DTYPE)

    def _call(self, ctx, mem):
        centers = None if self.centers is None or not len(self.centers) else self.centers.ctypes.data
        return lib().svo_submit_prune_voxel_maps(ctx, self._seq_arr, self._n, C.byref(self.keep), self.center_mode, centers,
                                                 self._info.ctypes.data)


class Carve(Prune):
    """One svo_submit_carve_voxel_maps: a Prune carrying a carve. The occluder of every named slot is the organized
    camera-frame cloud of its current frame under `style` (a hip_lib.CloudStyle), `check` (a StereoCheck or None) and
    `sgm` (an SgmParams or None: winner-takes-all); carve: a hip_lib.VoxelCarve; keep: a VoxelKeep or None (every entry
    is kept by the keep rule). After wait(): `info` (hip_lib.CARVE_INFO_DTYPE, one per named slot)."""

    def __init__(self, slam, seqs, style, check, sgm, carve, keep, centers):
        super().__init__(slam, seqs, keep, centers)
        self.style, self.check, self.sgm, self.carve = style, check, sgm, carve
        self._info, self.info = self._per_slot(hip_lib.CARVE_INFO_DTYPE)

    def _call(self, ctx, mem):
        centers = None if self.centers is None or not len(self.centers) else self.centers.ctypes.data
        ref = lambda x: None if x is None else C.byref(x)
        return lib().svo_submit_carve_voxel_maps(ctx, self._seq_arr, self._n, C.byref(self.style), ref(self.sgm), ref(self.check),
                                                 ref(self.carve), ref(self.keep), self.center_mode, centers, self._info.ctypes.data)


class VoxelMaps(PointJob):
    """One svo_submit_export_voxel_maps: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.VOXEL_SEGMENT_DTYPE, one per named slot) and points(i); `points_buffer`: PointJob. capacities: the records
    each named slot's region holds, back to back."""

    def __init__(self, slam, seqs, capacities, min_count, min_stamp, device):
        n = self._name(slam, seqs, device)
        caps = [int(c) for c in np.broadcast_to(capacities, (n,))]
        self.regions = self._per_slot(hip_lib.VOXEL_REGION_DTYPE)[0]
        self.regions["point_capacity"][:n] = caps
        self.regions["first_point"][:n] = np.cumsum([0] + caps[:-1]) if n else []
        self.regions["min_stamp"][:n] = np.broadcast_to(min_stamp, (n,))
        self.capacity = sum(caps)
        self._filter = hip_lib.VoxelFilter(int(min_count), 0)
        self._segments(hip_lib.VOXEL_SEGMENT_DTYPE)
        self._points()
        self._dst = hip_lib.VoxelDst(self._seg.ctypes.data, self.points_buffer.data_ptr())

    def _call(self, ctx, mem):
        return lib().svo_submit_export_voxel_maps(ctx, self._seq_arr, self._n, self.regions.ctypes.data_as(C.c_void_p),
                                                  C.byref(self._filter), C.byref(self._dst), mem)

    def span(self, i):
        """(device address, n) of named slot i's records (device mode): what a scene job's extra span takes"""
        e = self.segments[i]
        n = int(e["n_points"]) if int(e["status"]) == hip_lib.VOXEL_OK else 0
        return (self.points_buffer.data_ptr() + 16 * int(e["first_point"]) if n else None, n)

    def points(self, i):
        """the records of named slot i (hip_lib.MAP_POINT_DTYPE) in key order; None unless its status is VOXEL_OK"""
        e = self.segments[i]
        if int(e["status"]) != hip_lib.VOXEL_OK:
            return None
        return self._records(int(e["first_point"]), int(e["n_points"]))


# the 64-byte header of VoxelSaves.tobytes, little endian; the records follow
VOXEL_SAVE_MAGIC, VOXEL_SAVE_VERSION = 0x45585653, 1       # "SVXE"
VOXEL_SAVE_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("voxel_bits", "<u4"), ("drop_flags", "<u4"), ("log2_capacity", "<i4"),
                                    ("_pad", "<i4"), ("n", "<i8"), ("n_fused", "<i8"), ("n_outside", "<i8"), ("overflow", "<i8"), ("_pad2", "<i8")])
assert VOXEL_SAVE_HEADER_DTYPE.itemsize == 64


class VoxelSaves(Job):
    """One svo_submit_save_voxel_maps: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.VOXEL_SEGMENT_DTYPE, one per named slot; n_points counts entries), status(i), entries(i), info(i) and
    tobytes(i). `entries_buffer`: a uint8 [capacity, 40] tensor of hip_lib.VOXEL_ENTRY_DTYPE records, pinned memory in
    host mode, on the ctx's device in device mode. capacities: the records each named slot's region holds, back to
    back. `maps`: per named slot what svo_get_voxel_map_info says at this job's own wait() (None for a slot without a
    map, and for every slot until then: the ctx's wait() does not fill it). tobytes takes from it what the segment does
    not carry: drop_flags, and n_outside and overflow, which are the map's at that wait and not at the job's queue
    position (n, n_fused and the records are the job's); without it tobytes raises."""

    def __init__(self, slam, seqs, capacities, min_count, min_stamp, device):
        n = self._name(slam, seqs, device)
        caps = [int(c) for c in np.broadcast_to(capacities, (n,))]
        self.regions = self._per_slot(hip_lib.VOXEL_REGION_DTYPE)[0]
        self.regions["point_capacity"][:n] = caps
        self.regions["first_point"][:n] = np.cumsum([0] + caps[:-1]) if n else []
        self.regions["min_stamp"][:n] = np.broadcast_to(min_stamp, (n,))
        self.capacity = sum(caps)
        self._filter = hip_lib.VoxelFilter(int(min_count), 0)
        self._segments(hip_lib.VOXEL_SEGMENT_DTYPE)
        self.entries_buffer = self._alloc((max(self.capacity, 1), hip_lib.VOXEL_ENTRY_DTYPE.itemsize), torch.uint8)
        self._dst = hip_lib.VoxelEntryDst(self._seg.ctypes.data, self.entries_buffer.data_ptr())
        self.maps = [None] * n

    def _call(self, ctx, mem):
        return lib().svo_submit_save_voxel_maps(ctx, self._seq_arr, self._n, self.regions.ctypes.data_as(C.c_void_p),
                                                C.byref(self._filter), C.byref(self._dst), mem)

    def wait(self):
        super().wait()
        if self._slam is not None:
            named = range(self._slam.n) if self.seqs is None else self.seqs
            self.maps = [self._slam.voxel_map_info(s) for s in named]
        return self

    def status(self, i):
        return int(self.segments[i]["status"])

    def info(self, i):
        """the segment of named slot i"""
        return self.segments[i]

    def voxel(self, i):
        """the voxel edge the keys of named slot i were made with (float32)"""
        return np.float32(self.segments[i]["voxel"])

    def entries(self, i):
        """the records of named slot i in key order, a view: numpy hip_lib.VOXEL_ENTRY_DTYPE in host mode, a uint8 [n, 40]
        tensor on the device in device mode; None unless its status is VOXEL_OK"""
        e = self.segments[i]
        if int(e["status"]) != hip_lib.VOXEL_OK:
            return None
        a = self.entries_buffer[int(e["first_point"]):int(e["first_point"]) + int(e["n_points"])]
        return a if self.device_mode else a.numpy().view(hip_lib.VOXEL_ENTRY_DTYPE)[:, 0]

    def tobytes(self, i):
        """named slot i as bytes: a VOXEL_SAVE_HEADER_DTYPE header (magic, version, the voxel edge's bits, drop_flags, the
        source's log2_capacity, n, and the map's three cumulative counters) and the n records"""
        ent = self.entries(i)
        if ent is None:
            raise ValueError(f"slot {i} of the job holds no entries (status {self.status(i)})")
        if self.maps[i] is None:
            raise ValueError(f"slot {i}: tobytes needs the map's drop_flags and counters, which this job's own wait() reads "
                             "(the ctx's wait() delivers the entries only)")
        ent = ent.cpu().numpy().view(hip_lib.VOXEL_ENTRY_DTYPE)[:, 0] if self.device_mode else ent
        e, m = self.segments[i], self.maps[i]
        head = np.zeros((), VOXEL_SAVE_HEADER_DTYPE)
        head["magic"], head["version"] = VOXEL_SAVE_MAGIC, VOXEL_SAVE_VERSION
        head["voxel_bits"] = np.float32(e["voxel"]).view(np.uint32)
        head["drop_flags"], head["log2_capacity"], head["n"] = m["drop_flags"], e["log2_capacity"], len(ent)
        head["n_fused"], head["n_outside"], head["overflow"] = e["n_fused"], m["n_outside"], m["overflow"]
        return head.tobytes() + ent.tobytes()

    @classmethod
    def frombytes(cls, b):
        """the VoxelSaves of one slot that tobytes wrote: host mode, bound to no ctx (it cannot be submitted); `header`
        holds the file's header"""
        if len(b) < 64:
            raise ValueError("not a saved voxel map: shorter than its header")
        head = np.frombuffer(b[:64], VOXEL_SAVE_HEADER_DTYPE)[0]
        n = int(head["n"])
        if int(head["magic"]) != VOXEL_SAVE_MAGIC or int(head["version"]) != VOXEL_SAVE_VERSION or n < 0 or len(b) != 64 + 40 * n:
            raise ValueError("not a saved voxel map: bad magic, version or length")
        self = cls.__new__(cls)
        self._slam, self.device_mode, self.seqs, self._n, self._seq_arr = None, False, [0], 1, None
        self.header = head.copy()
        self._segments(hip_lib.VOXEL_SEGMENT_DTYPE)
        e = self.segments[0]
        e["status"], e["n_points"], e["n_voxels"], e["n_fused"] = hip_lib.VOXEL_OK, n, n, head["n_fused"]
        e["voxel"], e["log2_capacity"] = np.uint32(head["voxel_bits"]).view(np.float32), head["log2_capacity"]
        self.capacity = n
        self.entries_buffer = torch.zeros((max(n, 1), 40), dtype=torch.uint8)
        self.entries_buffer[:n] = torch.frombuffer(bytearray(b[64:]), dtype=torch.uint8).reshape(n, 40) if n else self.entries_buffer[:0]
        self.maps = [{"drop_flags": int(head["drop_flags"]), "n_outside": int(head["n_outside"]), "overflow": int(head["overflow"])}]
        return self

    def submit(self):
        if self._slam is None:
            raise ValueError("a VoxelSaves read from bytes belongs to no ctx")
        return super().submit()


class VoxelLoads(Job):
    """One svo_submit_load_voxel_maps: owns the spans and keeps the entries alive until the job is delivered. After wait():
    `info` (hip_lib.VOXEL_LOAD_INFO_DTYPE, one per named slot). sources: per named slot entry records (a numpy array of
    hip_lib.VOXEL_ENTRY_DTYPE, a uint8 [n, 40] tensor on the host or on the ctx's device, or None: no records); voxels:
    the voxel edge of each. All on the host or all on the device."""

    def __init__(self, slam, seqs, sources, voxels, merge):
        n = self._name(slam, seqs)
        if len(sources) != n:
            raise ValueError(f"{len(sources)} sources for {n} slots")
        on_device = {isinstance(s, torch.Tensor) and s.is_cuda for s in sources if s is not None and len(s)}
        if len(on_device) > 1:
            raise ValueError("the entries of one load job lie all on the host or all on the device")
        self.device_mode = bool(on_device and on_device.pop())
        self.mode = hip_lib.VOXEL_LOAD_MERGE if merge else hip_lib.VOXEL_LOAD_REPLACE
        self._spans = np.zeros(max(n, 1), hip_lib.VOXEL_ENTRY_SPAN_DTYPE)
        self._keep = []
        for i, (src, voxel) in enumerate(zip(sources, np.broadcast_to(np.asarray(voxels, np.float32), (n,)))):
            self._spans[i]["voxel"] = voxel
            if src is None or not len(src):
                continue
            if isinstance(src, torch.Tensor):
                src = src.contiguous()
                count, ptr = src.numel() * src.element_size() // 40, src.data_ptr()
            else:
                src = np.ascontiguousarray(src, hip_lib.VOXEL_ENTRY_DTYPE)
                count, ptr = len(src), src.ctypes.data
            self._keep.append(src)
            self._spans[i]["entries"], self._spans[i]["n"] = ptr, count
        self._info, self.info = self._per_slot(hip_lib.VOXEL_LOAD_INFO_DTYPE)

    def _call(self, ctx, mem):
        return lib().svo_submit_load_voxel_maps(ctx, self._seq_arr, self._n, self._spans.ctypes.data, self.mode, mem, self._info.ctypes.data)

    def status(self, i):
        return int(self.info[i]["status"])


class Scenes(PictureJob):
    """One svo_submit_export_scenes: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.SCENE_SEGMENT_DTYPE, one per named slot), image(i) and `pixels` (PictureJob). cols, rows, pitch,
    image_bytes: the shape of every image of the job (svo_scene_size); channels: 3 or 4. With dense or clouds
    (StereoSlamBatch.submit_scenes) the job is svo_submit_export_scenes_clouds and `cloud_info`
    (hip_lib.SCENE_CLOUD_INFO_DTYPE, one per named slot) says what was drawn; without them cloud_info is None. With the
    key sgm in dense (what hip_lib.sgm_job takes) the job is svo_submit_export_scenes_clouds_sgm: the live layer is the
    cloud of the SGM map, `sgm` its params, and the lr_check key of the sgm dict its check."""

    OK = hip_lib.SCENE_OK
    DENSE_DEFAULTS = dict(live=True, what="frames", step=2, win=0, search_x=0, search_y=0, min_disparity=0.0, max_depth=0.0,
                          max_mean_cost=0.0, lr_check=0.0, point_size=1, sgm=None)

    def __init__(self, slam, seqs, style, cameras, device, dense=None, clouds=None):
        n = self._name(slam, seqs, device)
        self.style = style
        self.cols, self.rows = style.cols, style.rows
        self.pitch, self.image_bytes = hip_lib.scene_size(style)
        self.channels = hip_lib.PIXEL_BYTES[style.pixel]
        if isinstance(cameras, hip_lib.SceneCamera):
            cameras = [cameras] * n                       # one view of all
        if len(cameras) != n:
            raise ValueError(f"{len(cameras)} cameras for {n} named slots: one per named slot, or a single one for all")
        self._cams = (hip_lib.SceneCamera * max(n, 1))(*cameras)
        self._pictures(hip_lib.SCENE_SEGMENT_DTYPE, hip_lib.SceneDst)
        self.cloud_info = self._clouds = self.sgm = None
        if dense is not None or clouds is not None:
            d = dict(self.DENSE_DEFAULTS)
            unknown = set(dense or {}) - set(d)
            if unknown:
                raise ValueError(f"dense: unknown keys {sorted(unknown)}")
            d.update(dense or {})
            if isinstance(d["what"], str):
                d["what"] = hip_lib.EXPORT_WHAT.index(d["what"])
            d["lr_check"] = float(d["lr_check"] or 0.0)
            if clouds is not None and len(clouds) != n:
                raise ValueError(f"{len(clouds)} clouds for {n} named slots: one per named slot")
            self._info, self.cloud_info = self._per_slot(hip_lib.SCENE_CLOUD_INFO_DTYPE)
            live = dense is not None and bool(d.pop("live"))
            d.pop("live", None)
            self._clouds = hip_lib.scene_clouds(live=live, extra=clouds, info=self._info, **d)
            self.sgm = self._clouds[0].sgm

    def _call(self, ctx, mem):
        if self.sgm is not None:
            return lib().svo_submit_export_scenes_clouds_sgm(ctx, self._seq_arr, self._n, C.byref(self.style),
                                                             C.byref(self._clouds[0]), C.byref(self.sgm), self._cams,
                                                             C.byref(self._dst), mem)
        if self._clouds is None:
            return lib().svo_submit_export_scenes(ctx, self._seq_arr, self._n, C.byref(self.style), self._cams,
                                                  C.byref(self._dst), mem)
        return lib().svo_submit_export_scenes_clouds(ctx, self._seq_arr, self._n, C.byref(self.style),
                                                     C.byref(self._clouds[0]), self._cams, C.byref(self._dst), mem)


class ArPictures(PictureJob):
    """One svo_submit_export_ar: owns the buffers the library writes. After wait(): `segments`
    (hip_lib.AR_SEGMENT_DTYPE, one per named slot), image(i) and `pixels` (PictureJob). cols, rows, pitch,
    image_bytes: the shape of every image of the job (svo_ar_size); channels: 3 or 4. meshes: (vertices [V, 3],
    triangles [T, 3][, rgb [T] or None]) each; instances: hip_lib.ArInstance, or (model of 12 floats, mesh index,
    rgb) each; first: None (every slot shows every instance) or n + 1 ascending offsets into the instances.
    With occlusion (StereoSlamBatch.submit_ar) the job is svo_submit_export_ar_occluded and `visibility`
    (hip_lib.AR_VISIBILITY_DTYPE, one per named slot) says how much of the meshes is hidden; without it visibility
    is None. With the key sgm in occlusion (what hip_lib.sgm_job takes; or an ArOcclusion whose sgm is set) the job is
    svo_submit_export_ar_occluded_sgm: the occluder is the cloud of the SGM map, `sgm` its params, and the lr_check key
    of the sgm dict its check."""

    OK = hip_lib.AR_OK
    OCCLUSION_DEFAULTS = dict(step=4, hidden="drop", alpha=128, margin=0.0, drop_flags=0, win=0, search_x=0, search_y=0,
                              min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0, lr_check=0.0, sgm=None)

    def __init__(self, slam, seqs, style, meshes, instances, first, device, occlusion=None):
        n = self._name(slam, seqs, device)
        self.style = style
        self.cols, self.rows = slam.width, slam.height
        self.pitch, self.image_bytes = hip_lib.ar_size(slam.cam, slam.width, slam.height, style)
        self.channels = hip_lib.PIXEL_BYTES[style.pixel]
        self._keep = []
        self._meshes = (hip_lib.ArMesh * max(len(meshes), 1))()
        for i, m in enumerate(meshes):
            v = np.ascontiguousarray(m[0], np.float32).reshape(-1, 3)
            t = np.ascontiguousarray(m[1], np.int32).reshape(-1, 3)
            rgb = None if len(m) < 3 or m[2] is None else np.ascontiguousarray(m[2], np.uint32).reshape(-1)
            if rgb is not None and len(rgb) != len(t):
                raise ValueError(f"mesh {i}: {len(rgb)} colours for {len(t)} triangles")
            self._keep += [v, t, rgb]
            self._meshes[i] = hip_lib.ArMesh(v.ctypes.data if len(v) else None, t.ctypes.data if len(t) else None,
                                             None if rgb is None else rgb.ctypes.data, len(v), len(t), 0)
        self._n_meshes = len(meshes)
        inst = [x if isinstance(x, hip_lib.ArInstance) else hip_lib.ar_instance(*x) for x in instances]
        self._inst = (hip_lib.ArInstance * max(len(inst), 1))(*inst)
        self._n_inst = len(inst)
        self._first = None if first is None else (C.c_int * (n + 1))(*[int(f) for f in first])
        self._pictures(hip_lib.AR_SEGMENT_DTYPE, hip_lib.ArDst)
        self.visibility = self._occlusion = self.sgm = None
        if occlusion is not None:
            if isinstance(occlusion, hip_lib.ArOcclusion):
                self._occlusion = hip_lib.ArOcclusion.from_buffer_copy(occlusion)
                self._occlusion.sgm = occlusion.sgm
            else:
                d = dict(self.OCCLUSION_DEFAULTS)
                unknown = set(occlusion) - set(d)
                if unknown:
                    raise ValueError(f"occlusion: unknown keys {sorted(unknown)}")
                d.update(occlusion)
                self._occlusion = hip_lib.ar_occlusion(True, **d)
            self._vis, self.visibility = self._per_slot(hip_lib.AR_VISIBILITY_DTYPE)
            self._occlusion.info = self._vis.ctypes.data
            self.sgm = self._occlusion.sgm

    def _call(self, ctx, mem):
        if self.sgm is not None:
            return lib().svo_submit_export_ar_occluded_sgm(ctx, self._seq_arr, self._n, C.byref(self.style),
                                                           C.byref(self._occlusion), C.byref(self.sgm), self._meshes,
                                                           self._n_meshes, self._inst, self._first, self._n_inst,
                                                           C.byref(self._dst), mem)
        if self._occlusion is None:
            return lib().svo_submit_export_ar(ctx, self._seq_arr, self._n, C.byref(self.style), self._meshes, self._n_meshes,
                                              self._inst, self._first, self._n_inst, C.byref(self._dst), mem)
        return lib().svo_submit_export_ar_occluded(ctx, self._seq_arr, self._n, C.byref(self.style),
                                                   C.byref(self._occlusion), self._meshes, self._n_meshes, self._inst,
                                                   self._first, self._n_inst, C.byref(self._dst), mem)


class Snapshot:
    """The sequence state of one slot (svo_submit_save / svo_submit_load): `host` (numpy uint8, the host part) and
    `data` (the data part: numpy uint8, or a torch uint8 tensor on the ctx's device in device mode). Valid after
    the wait() that follows its save. `info`: the checked header (hip_lib.SnapshotInfo). tobytes() / frombytes():
    one self-contained blob for a file."""

    def __init__(self, host, data):
        self.host, self.data = host, data

    @property
    def device_mode(self):
        return isinstance(self.data, torch.Tensor)

    @property
    def info(self):
        return hip_lib.snapshot_info(self.host)

    def trimmed(self):
        """the two parts cut to the sizes the header states (a save is given capacities)"""
        i = self.info
        return Snapshot(self.host[:i.host_bytes], self.data[:i.data_bytes])

    def tobytes(self):
        """host part, then data part (their sizes are in the header)"""
        t = self.trimmed()
        data = t.data.cpu().numpy() if t.device_mode else t.data
        return t.host.tobytes() + data.tobytes()

    @classmethod
    def frombytes(cls, blob, device=None):
        """from tobytes(); device: a torch device for a device-mode snapshot (default: host mode)"""
        i = hip_lib.snapshot_info(blob)
        if i.status != hip_lib.SNAPSHOT_COMPLETE or len(blob) < i.host_bytes + i.data_bytes:
            raise SvoError("snapshot: incomplete")
        a = np.frombuffer(blob, np.uint8)
        host, data = a[:i.host_bytes].copy(), a[i.host_bytes:i.host_bytes + i.data_bytes].copy()
        return cls(host, torch.from_numpy(data).to(device) if device is not None else data)

    def _buffers(self):
        if self.device_mode:
            assert self.data.is_cuda and self.data.dtype == torch.uint8 and self.data.is_contiguous()
            data, n = self.data.data_ptr(), self.data.numel()
        else:
            assert self.data.dtype == np.uint8 and self.data.flags.c_contiguous
            data, n = self.data.ctypes.data, self.data.size
        assert self.host.dtype == np.uint8 and self.host.flags.c_contiguous
        return hip_lib.SnapshotBuffers(self.host.ctypes.data, self.host.size, data if n else None, n)
