"""The Python job objects themselves (Export, MapExport, Views, Disparities, Clouds, Fusion, VoxelMaps, Scenes,
ArPictures): what a freshly made one holds, the library call its submit() makes, and what a second submit() does.
The other suites check what the jobs deliver; the tables here were written from the source of the nine stand-alone
classes that stereo_slam.py held before they moved to jobs.py over one base, and passed against those first.

One ctx of the `tiny` configuration, 3 slots, two frames played, a voxel map of 1 << 10 entries on every slot, one box
for the AR jobs. Per class: every slot (seqs=None), [2, 0] and the empty list (every entry takes one), host and device
mode, and both entries of the four classes that have two.

The call is taken by a wrapper over the entry in hip_lib.lib() that forwards to the real one. It is compared as: the
entry's name, None and numbers as they are, the bytes of an int array, every structure field by field, and every
address as (the job's buffer it points into, offset). An address that points into none of them fails."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import (KP_INFO_DTYPE, ArPictures, Clouds, Disparities, Export, Frame, Fusion, MapExport,
                                             Scenes, StereoSlam, StereoSlamBatch, Views, VoxelMaps)

pytestmark = pytest.mark.gpu

N_SLOTS = 3
NAMINGS = (None, [2, 0], [])
HOST, DEVICE = hip_lib.MEM_HOST, hip_lib.MEM_DEVICE
VOXEL, LOG2 = 0.05, 10


@pytest.fixture(scope="module")
def ctx():
    """(batch, cfg): every slot has a frame, a keyframe and an (empty) voxel map"""
    seqs = [synth.make_sequence_gpu("tiny", 2, seed, motion_scale=4.0) for seed in (1, 11, 12)]
    torch.cuda.synchronize()
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], N_SLOTS)
    for k in range(2):
        batch.new_images([s[1][k] for s in seqs], [s[2][k] for s in seqs], [float(s[4][k]) for s in seqs])
    batch.set_voxel_maps(VOXEL, LOG2)
    assert all(batch.num_keyframes(s) >= 1 and batch.stats(s).frame_id == 1 for s in range(N_SLOTS))
    yield batch, cfg
    batch.close()


# ------------------------------------------------------------------------------------------------ the attribute tables

class T:
    """a row of an attribute table: the exact type, and for an array its dtype, shape, place ("pinned", "host", "cuda";
    None: not a tensor) and whether it is all zero"""

    def __init__(self, kind, dtype=None, shape=None, place=None, zero=False):
        self.kind, self.dtype, self.shape, self.place, self.zero = kind, dtype, shape, place, zero


ND, TT = np.ndarray, torch.Tensor


def _check_rows(tag, job, device, rows):
    """every row of the table; a value that is no T is compared as it is"""
    for attr, want in rows.items():
        got = getattr(job, attr)
        where = (tag, attr)
        if not isinstance(want, T):
            assert type(got) is type(want) and got == want, (where, got, want)
            continue
        assert type(got) is want.kind, (where, type(got))
        if want.dtype is not None:
            assert got.dtype == want.dtype, (where, got.dtype)
        if want.shape is not None:
            assert tuple(got.shape) == tuple(want.shape), (where, tuple(got.shape))
        if want.place == "cuda":
            assert got.is_cuda and got.device == device, where
        elif want.place is not None:
            assert not got.is_cuda and got.is_pinned() == (want.place == "pinned"), where
        if want.zero:
            assert not (got if isinstance(got, ND) else got.cpu().numpy()).view(np.uint8).any(), where


def _names(n, seqs):
    """the rows every class with optional naming shares"""
    return {"seqs": seqs, "_n": n, "_seq_arr": None if seqs is None else T(C.c_int * max(n, 1))}


# ------------------------------------------------------------------------------------------------ the recorded call

class Where:
    """addresses as (name of a job's buffer, offset); `raw` keeps them as they were"""

    def __init__(self, buffers):
        self.spans, self.raw = [], []
        for name, b in buffers.items():
            if b is None:
                continue
            if isinstance(b, TT):
                lo, size = b.data_ptr(), b.numel() * b.element_size()
            elif isinstance(b, ND):
                lo, size = b.ctypes.data, b.nbytes
            else:
                lo, size = C.addressof(b), C.sizeof(b)
            if lo and size:
                self.spans.append((name, lo, size))

    def __call__(self, addr):
        if not addr:
            return None
        self.raw.append(addr)
        for name, lo, size in self.spans:
            if lo <= addr < lo + size:
                return (name, addr - lo)
        raise AssertionError(f"address {addr:#x} points into none of the job's buffers")


def _plain(v, where=lambda address: address or None):
    """a ctypes value as Python values; addresses through `where` (default: as they are, NULL as None)"""
    if isinstance(v, C.Structure):
        return {name: where(getattr(v, name)) if typ is C.c_void_p else _plain(getattr(v, name), where)
                for name, typ in v._fields_}
    if isinstance(v, C.Array):
        return [_plain(x, where) for x in v]
    return v


def _arg(a, ctx, where):
    if a is ctx:
        return "ctx"
    if a is None or isinstance(a, float):
        return a
    if isinstance(a, int):
        return where(a) if a >> 32 else a                  # (an address that travels as a Python int)
    if isinstance(a, C.c_void_p):
        return where(a.value)
    if isinstance(a, C.Array):
        return bytes(a) if issubclass(a._type_, C._SimpleCData) else _plain(a, where)
    if hasattr(a, "_obj"):                                  # byref
        return _plain(a._obj, where)
    raise AssertionError(f"argument of type {type(a)}")


class Recorder:
    """forwarding wrappers over entries of hip_lib.lib(), and a counter of the stream synchronisations"""

    def __init__(self, monkeypatch, names):
        self.calls, self.syncs = [], 0
        lib = hip_lib.lib()
        for name in names:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))
        real = torch.cuda.current_stream
        rec = self

        class Stream:
            def __init__(self, s):
                self._s = s

            def synchronize(self):
                rec.syncs += 1
                self._s.synchronize()

        monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream(real(device)))

    def _wrap(self, name, real):
        def entry(*args):
            self.calls.append((name, args))
            return real(*args)
        return entry

    def submit(self, job, buffers):
        """job.submit().wait(): the one call it made as (comparable, raw addresses), and the synchronisations"""
        self.calls.clear()
        self.syncs = 0
        assert job.submit() is job
        assert job.wait() is job
        assert len(self.calls) == 1, [c[0] for c in self.calls]
        name, args = self.calls[0]
        where = Where(buffers)
        return [name] + [_arg(a, job._slam._ctx, where) for a in args], where.raw, self.syncs


def _ints(values):
    return None if values is None else struct.pack(f"<{max(len(values), 1)}i", *(values or [0]))


def _submit_twice(tag, rec, job, buffers, want, syncs):
    """the call against `want`; a second submit of the delivered job makes the same call with the same addresses"""
    call, raw, n_sync = rec.submit(job, buffers(job))
    assert call == want, (tag, call, want)
    assert n_sync == syncs, (tag, n_sync)
    again, raw2, n_sync2 = rec.submit(job, buffers(job))
    assert again == call and raw2 == raw and n_sync2 == syncs, tag
    return call


def _cases(namings=NAMINGS):
    for seqs in namings:
        for device in (False, True):
            yield seqs, (N_SLOTS if seqs is None else len(seqs)), device


def _place(device):
    return "cuda" if device else "pinned"


# ------------------------------------------------------------------------------------------------ the nine classes

def test_export(ctx, monkeypatch):
    batch, _ = ctx
    rec = Recorder(monkeypatch, ["svo_submit_export"])
    cap1 = batch.export_capacity()
    shapes = {"kps2d": (torch.float32, 2), "kps3d": (torch.float32, 3), "info": (torch.uint8, 44)}
    for fields in (("kps2d", "kps3d", "info"), ("kps3d",)):
        for seqs, n, device in _cases():
            for what in (0, 1):
                tag = ("Export", fields, seqs, device, what)
                job = Export(batch, what, seqs, device, fields)
                cap = n * cap1
                rows = dict(_names(n, seqs), what=what, device_mode=device, capacity=cap,
                            _seg=T(TT, torch.uint8, (max(n, 1) * 64,), "host", zero=True),
                            segments=T(ND, hip_lib.EXPORT_SEGMENT_DTYPE, (n,)), _bufs=T(dict), _dst=T(hip_lib.ExportDst))
                for name, (dtype, width) in shapes.items():
                    if name not in fields:
                        rows[name] = None
                    elif device:
                        rows[name] = T(TT, dtype, (cap, width), "cuda")
                    elif name == "info":
                        rows[name] = T(ND, KP_INFO_DTYPE, (cap,))
                    else:
                        rows[name] = T(ND, np.float32, (cap, width))
                _check_rows(tag, job, batch.device, rows)
                assert sorted(job._bufs) == sorted(fields), tag
                for name in fields:                          # (torch.empty: only shape, dtype and place)
                    b = job._bufs[name]
                    assert type(b) is TT and b.dtype == shapes[name][0] and tuple(b.shape) == (cap, shapes[name][1]), tag
                    assert (b.is_cuda and b.device == batch.device) if device else (b.is_pinned() or cap == 0), tag     # (nothing to pin)
                assert job.segments.base is not None and not job.segments.flags.owndata, tag
                ptr = lambda name: (name, 0) if name in fields and cap else None
                want = ["svo_submit_export", "ctx", what, _ints(seqs), n,
                        dict(segments=("segments", 0), kps2d=ptr("kps2d"), kps3d=ptr("kps3d"), info=ptr("info"), capacity=cap),
                        DEVICE if device else HOST]
                _submit_twice(tag, rec, job, lambda j: dict(j._bufs, segments=j._seg), want, 1 if device else 0)
                for i in range(n):
                    f = job.frame(i)
                    assert type(f) is Frame and f.pose.dtype == np.float32 and f.pose.shape == (6,), tag
                    m = int(job.segments[i]["n"])
                    assert m > 0 and int(job.segments[i]["seq"]) == (i if seqs is None else seqs[i]), tag
                    for name, (dtype, width) in shapes.items():
                        a = getattr(f, name)
                        if name not in fields:
                            assert a is None, tag
                        else:
                            assert type(a) is ND and a.flags.owndata and len(a) == m, tag
                            assert a.dtype == (KP_INFO_DTYPE if name == "info" else np.float32), tag


def _map_buffers(j):
    return dict(segments=j._seg, keyframes=j._kfs, points=j.points_buffer, regions=j.regions.base)


def test_map_export(ctx, monkeypatch):
    batch, _ = ctx
    rec = Recorder(monkeypatch, ["svo_submit_export_map"])
    for seqs, n, device in _cases():
        tag = ("MapExport", seqs, device)
        job = MapExport(batch, seqs, None, dict(own_only=1), device, 4096, 2)
        named = list(range(N_SLOTS)) if seqs is None else seqs
        rows = dict(seqs=named, _n=n, _seq_arr=T(C.c_int * max(n, 1)), device_mode=device, capacity=4096 * n,
                    filter=T(hip_lib.MapFilter), regions=T(ND, hip_lib.MAP_REGION_DTYPE, (n,)),
                    _seg=T(ND, hip_lib.MAP_SEGMENT_DTYPE, (max(n, 1),), zero=True), segments=T(ND, hip_lib.MAP_SEGMENT_DTYPE, (n,)),
                    _kfs=T(ND, hip_lib.MAP_KEYFRAME_DTYPE, (max(2 * n, 1),), zero=True),
                    points_buffer=T(TT, torch.uint8, (max(4096 * n, 1), 16), _place(device)),     # (torch.empty)
                    _dst=T(hip_lib.MapDst))
        _check_rows(tag, job, batch.device, rows)
        assert bytes(job._seq_arr) == _ints(named), tag              # (always an explicit list)
        assert [int(x) for x in job.regions["first_point"]] == [4096 * i for i in range(n)], tag
        assert [int(x) for x in job.regions["first_keyframe_entry"]] == [2 * i for i in range(n)], tag
        assert job.filter.own_only == 1, tag
        want = ["svo_submit_export_map", "ctx", _ints(named), n, ("regions", 0),
                dict(drop_flags=0, own_only=1, min_inliers=0, _reserved=0),
                dict(segments=("segments", 0), keyframes=("keyframes", 0) if n else None, points=("points", 0) if n else None),
                DEVICE if device else HOST]
        _submit_twice(tag, rec, job, _map_buffers, want, 1 if device else 0)
        assert not job.grow(), tag
        for i in range(n):
            assert int(job.segments[i]["status"]) == hip_lib.MAP_COMPLETE, tag
            kfs, pts = job.keyframes(i), job.points(i)
            assert type(kfs) is ND and kfs.dtype == hip_lib.MAP_KEYFRAME_DTYPE and len(kfs) >= 1, tag
            assert type(pts) is ND and pts.dtype == hip_lib.MAP_POINT_DTYPE and pts.shape == (int(job.segments[i]["n_points"]),), tag
            assert job.points_of_keyframe(i, 0).shape == (int(kfs[0]["n"]),) and type(job.first_keyframe(i)) is int, tag


def test_map_export_grow_makes_new_buffers(ctx, monkeypatch):
    batch, _ = ctx
    rec = Recorder(monkeypatch, ["svo_submit_export_map"])
    for device in (False, True):
        job = MapExport(batch, [2, 0], None, None, device, 1, 1)
        _, raw, _ = rec.submit(job, _map_buffers(job))
        assert (job.segments["status"] == hip_lib.MAP_TOO_SMALL).all()
        old = (job._kfs, job.points_buffer)                      # (kept: a freed block could be handed out again)
        assert job.grow()
        assert job._kfs is not old[0] and job.points_buffer.data_ptr() != old[1].data_ptr()
        assert job.capacity == int(job.segments["points_bound"].sum()) > 2
        assert job.points_buffer.shape == (job.capacity, 16) and job.points_buffer.is_cuda == device
        call, raw2, _ = rec.submit(job, _map_buffers(job))
        assert raw2 != raw and call[6] == dict(segments=("segments", 0), keyframes=("keyframes", 0), points=("points", 0))
        assert (job.segments["status"] == hip_lib.MAP_COMPLETE).all() and not job.grow()
        assert len(job.points(0)) == int(job.segments[0]["n_points"]) > 0


def _picture_rows(n, device, image_bytes, seg_dtype):
    cap = n * image_bytes
    return dict(device_mode=device, capacity=cap, _seg=T(ND, seg_dtype, (max(n, 1),), zero=True), segments=T(ND, seg_dtype, (n,)),
                _buf=T(TT, torch.uint8, (max(cap, 4),), _place(device), zero=True),
                pixels=T(TT, torch.uint8, (max(cap, 4),), "cuda") if device else T(ND, np.uint8, (max(cap, 4),)))


def _check_images(tag, job, n, device, shape):
    """image(i) of a delivered picture job: a view of `pixels`"""
    for i in range(n):
        img = job.image(i)
        assert type(img) is (TT if device else ND) and tuple(img.shape) == shape and img.dtype == (torch.uint8 if device else np.uint8), tag
        lo = int(job.segments[i]["offset"])
        if device:
            assert img.data_ptr() == job._buf.data_ptr() + lo, tag
        else:
            assert img.ctypes.data == job._buf.data_ptr() + lo and not img.flags.owndata, tag


def test_views(ctx, monkeypatch):
    batch, cfg = ctx
    rec = Recorder(monkeypatch, ["svo_submit_export_views"])
    for pixel, markers in (("gray8", False), ("rgba8", True)):
        for seqs, n, device in _cases():
            tag = ("Views", pixel, seqs, device)
            style = hip_lib.view_style(0, "left", 0, pixel, markers)
            want_style = _plain(hip_lib.view_style(0, "left", 0, pixel, markers))
            cols, rows_, pitch, image_bytes = batch.view_size(style)
            job = Views(batch, 0, seqs, style, device)
            ch = 1 if pixel == "gray8" else 4
            rows = dict(_names(n, seqs), what=0, cols=cfg["width"], rows=cfg["height"], pitch=pitch, image_bytes=image_bytes, channels=ch,
                        _dst=T(hip_lib.ViewDst), **_picture_rows(n, device, image_bytes, hip_lib.VIEW_SEGMENT_DTYPE))
            _check_rows(tag, job, batch.device, rows)
            assert job.style is style and (cols, rows_) == (cfg["width"], cfg["height"]), tag
            want = ["svo_submit_export_views", "ctx", 0, _ints(seqs), n, want_style,
                    dict(segments=("segments", 0), pixels=("buffer", 0), capacity=n * image_bytes), DEVICE if device else HOST]
            _submit_twice(tag, rec, job, lambda j: dict(segments=j._seg, buffer=j._buf), want, 1 if device else 0)
            assert (job.segments["status"] == hip_lib.VIEW_OK).all(), tag
            _check_images(tag, job, n, device, (cfg["height"], cfg["width"]) + ((ch,) if ch > 1 else ()))


def test_disparities(ctx, monkeypatch):
    batch, _ = ctx
    plain, checked = "svo_submit_export_disparity", "svo_submit_export_disparity_checked"
    rec = Recorder(monkeypatch, [plain, checked])
    for check in (None, hip_lib.stereo_check(False), hip_lib.stereo_check(True, 0.0)):
        on = check is not None and bool(check.lr)
        for seqs, n, device in _cases():
            tag = ("Disparities", on, check is None, seqs, device)
            style = hip_lib.disparity_style("disparity", 4, cost=True)
            want_style = _plain(hip_lib.disparity_style("disparity", 4, cost=True))
            cols, rows_, planes, image_bytes = batch.disparity_size(style, check if on else None)
            assert planes == (3 if on else 2) and image_bytes >= 4 * planes * rows_ * cols
            job = Disparities(batch, 1, seqs, style, device, check)
            floats = max(n * image_bytes // 4, 4)
            rows = dict(_names(n, seqs), what=1, device_mode=device, cols=cols, rows=rows_, n_planes=planes, image_bytes=image_bytes,
                        capacity=n * image_bytes, _seg=T(ND, hip_lib.DISPARITY_SEGMENT_DTYPE, (max(n, 1),), zero=True),
                        segments=T(ND, hip_lib.DISPARITY_SEGMENT_DTYPE, (n,)),
                        _buf=T(TT, torch.float32, (floats,), _place(device), zero=True), _dst=T(hip_lib.DisparityDst),
                        values=T(TT, torch.float32, (n, planes, rows_, cols), "cuda") if device else T(ND, np.float32, (n, planes, rows_, cols)))
            _check_rows(tag, job, batch.device, rows)
            assert job.style is style and (job.check is check if on else job.check is None), tag
            v = job.values                                        # a strided view of the buffer
            strides = (image_bytes // 4, rows_ * cols, cols, 1)
            if device:
                assert n == 0 or (tuple(v.stride()) == strides and v.data_ptr() == job._buf.data_ptr()), tag
            else:
                assert n == 0 or (v.strides == tuple(4 * s for s in strides) and v.ctypes.data == job._buf.data_ptr()), tag
            dst = dict(segments=("segments", 0), values=("buffer", 0), capacity=n * image_bytes)
            mem = DEVICE if device else HOST
            want = ([checked, "ctx", 1, _ints(seqs), n, want_style, _plain(hip_lib.stereo_check(True, 0.0)), dst, mem] if on
                    else [plain, "ctx", 1, _ints(seqs), n, want_style, dst, mem])
            _submit_twice(tag, rec, job, lambda j: dict(segments=j._seg, buffer=j._buf), want, 1 if device else 0)
            for i in range(n):
                assert int(job.segments[i]["status"]) == hip_lib.DISPARITY_OK, tag
                p, lr = job.planes(i), job.lr(i)
                assert type(p) is (TT if device else ND) and tuple(p.shape) == (planes, rows_, cols), tag
                assert (tuple(lr.shape) == (rows_, cols)) if on else lr is None, tag


def _check_records(tag, job, n, ok, counted=True):
    """points(i) of a delivered point-record job: a numpy array of MAP_POINT_DTYPE, a copy in device mode"""
    for i in range(n):
        assert int(job.segments[i]["status"]) == ok, tag
        pts = job.points(i)
        assert type(pts) is ND and pts.dtype == hip_lib.MAP_POINT_DTYPE and pts.ndim == 1, tag
        assert not counted or len(pts) == int(job.segments[i]["n_points"]), tag


def test_clouds(ctx, monkeypatch):
    batch, _ = ctx
    plain, checked = "svo_submit_export_cloud", "svo_submit_export_cloud_checked"
    rec = Recorder(monkeypatch, [plain, checked])
    for check, layout in ((None, "compact"), (hip_lib.stereo_check(False), "organized"), (hip_lib.stereo_check(True, 1.0), "compact")):
        on = check is not None and bool(check.lr)
        for seqs, n, device in _cases():
            tag = ("Clouds", on, layout, seqs, device)
            style = hip_lib.cloud_style(4, layout=layout)
            want_style = _plain(hip_lib.cloud_style(4, layout=layout))
            cols, rows_, per_slot = batch.cloud_size(style)
            job = Clouds(batch, 0, seqs, style, device, check)
            rows = dict(_names(n, seqs), what=0, device_mode=device, cols=cols, rows=rows_, points_per_slot=per_slot,
                        capacity=n * per_slot, _seg=T(ND, hip_lib.CLOUD_SEGMENT_DTYPE, (max(n, 1),), zero=True),
                        segments=T(ND, hip_lib.CLOUD_SEGMENT_DTYPE, (n,)),
                        points_buffer=T(TT, torch.uint8, (max(n * per_slot, 1), 16), _place(device), zero=True), _dst=T(hip_lib.CloudDst))
            _check_rows(tag, job, batch.device, rows)
            assert job.style is style and (job.check is check if on else job.check is None), tag
            dst = dict(segments=("segments", 0), points=("buffer", 0), capacity=n * per_slot)
            mem = DEVICE if device else HOST
            want = ([checked, "ctx", 0, _ints(seqs), n, want_style, _plain(hip_lib.stereo_check(True, 1.0)), dst, mem] if on
                    else [plain, "ctx", 0, _ints(seqs), n, want_style, dst, mem])
            _submit_twice(tag, rec, job, lambda j: dict(segments=j._seg, buffer=j.points_buffer), want, 1 if device else 0)
            _check_records(tag, job, n, hip_lib.CLOUD_OK, layout == "compact")
            for i in range(n):
                if layout == "organized":
                    assert job.organized(i).shape == (rows_, cols) and job.organized(i).dtype == hip_lib.MAP_POINT_DTYPE, tag
                else:
                    with pytest.raises(ValueError, match=r"organized\(\): the job's layout is compact"):
                        job.organized(i)


def test_fusion(ctx, monkeypatch):
    batch, _ = ctx
    rec = Recorder(monkeypatch, ["svo_submit_fuse_clouds"])
    for check in (None, hip_lib.stereo_check(False), hip_lib.stereo_check(True, 1.0)):
        on = check is not None and bool(check.lr)
        for seqs in NAMINGS:
            n = N_SLOTS if seqs is None else len(seqs)
            tag = ("Fusion", on, seqs)
            style = hip_lib.cloud_style(16, max_depth=40.0)
            want_style = _plain(hip_lib.cloud_style(16, max_depth=40.0))
            job = Fusion(batch, 1, seqs, style, check, 7)
            rows = dict(_names(n, seqs), what=1, stamp=7, _info=T(ND, hip_lib.FUSE_INFO_DTYPE, (max(n, 1),), zero=True),
                        info=T(ND, hip_lib.FUSE_INFO_DTYPE, (n,)))
            _check_rows(tag, job, batch.device, rows)
            assert job.style is style and (job.check is check if on else job.check is None), tag
            want = ["svo_submit_fuse_clouds", "ctx", 1, _ints(seqs), n, want_style,
                    _plain(hip_lib.stereo_check(True, 1.0)) if on else None, 7, ("info", 0)]
            _submit_twice(tag, rec, job, lambda j: dict(info=j._info), want, 0)     # (never synchronises the stream)
            assert all(int(s) in (hip_lib.FUSE_OK, hip_lib.FUSE_FULL) for s in job.info["status"]), tag
            assert [int(s) for s in job.info["seq"]] == (list(range(N_SLOTS)) if seqs is None else seqs), tag


def test_voxel_maps(ctx, monkeypatch):
    batch, _ = ctx
    batch.fuse_clouds("last_keyframes", None, step=16, max_depth=40.0)            # (something to export)
    rec = Recorder(monkeypatch, ["svo_submit_export_voxel_maps"])
    for seqs, n, device in _cases():
        tag = ("VoxelMaps", seqs, device)
        caps = [1024, 1040, 1024][:n]
        job = VoxelMaps(batch, seqs, caps if n else 1024, 1, 0, device)
        rows = dict(_names(n, seqs), device_mode=device, capacity=sum(caps), regions=T(ND, hip_lib.VOXEL_REGION_DTYPE, (max(n, 1),)),
                    _filter=T(hip_lib.VoxelFilter), _seg=T(ND, hip_lib.VOXEL_SEGMENT_DTYPE, (max(n, 1),), zero=True),
                    segments=T(ND, hip_lib.VOXEL_SEGMENT_DTYPE, (n,)),
                    points_buffer=T(TT, torch.uint8, (max(sum(caps), 1), 16), _place(device), zero=True), _dst=T(hip_lib.VoxelDst))
        _check_rows(tag, job, batch.device, rows)
        assert [int(x) for x in job.regions["point_capacity"][:n]] == caps, tag
        assert [int(x) for x in job.regions["first_point"][:n]] == [sum(caps[:i]) for i in range(n)], tag
        want = ["svo_submit_export_voxel_maps", "ctx", _ints(seqs), n, ("regions", 0), dict(min_count=1, min_stamp=0, _reserved=[0, 0]),
                dict(segments=("segments", 0), points=("buffer", 0)), DEVICE if device else HOST]
        _submit_twice(tag, rec, job, lambda j: dict(segments=j._seg, buffer=j.points_buffer, regions=j.regions), want, 1 if device else 0)
        _check_records(tag, job, n, hip_lib.VOXEL_OK)
        for i in range(n):
            m, lo = int(job.segments[i]["n_points"]), int(job.segments[i]["first_point"])
            assert job.span(i) == ((job.points_buffer.data_ptr() + 16 * lo, m) if m else (None, 0)), tag


def test_scenes(ctx, monkeypatch):
    batch, _ = ctx
    plain, clouds = "svo_submit_export_scenes", "svo_submit_export_scenes_clouds"
    rec = Recorder(monkeypatch, [plain, clouds])
    for dense in (None, dict(step=4, max_depth=40.0)):
        for seqs, n, device in _cases():
            tag = ("Scenes", dense is not None, seqs, device)
            style = hip_lib.scene_style(cols=64, rows=48, pixel="rgb8")
            want_style = _plain(hip_lib.scene_style(cols=64, rows=48, pixel="rgb8"))
            pitch, image_bytes = hip_lib.scene_size(style)
            cams = [hip_lib.scene_preset(name, 64, 48) for name in ("front", "top", "side")][:n]
            job = Scenes(batch, seqs, style, cams if n != 2 else cams[0], device, dense)     # (one camera stands for all)
            want_cams = [_plain(c) for c in ([cams[0]] * 2 if n == 2 else cams)] or [_plain(hip_lib.SceneCamera())]
            rows = dict(_names(n, seqs), cols=64, rows=48, pitch=pitch, image_bytes=image_bytes, channels=3,
                        _cams=T(hip_lib.SceneCamera * max(n, 1)), _dst=T(hip_lib.SceneDst),
                        **_picture_rows(n, device, image_bytes, hip_lib.SCENE_SEGMENT_DTYPE))
            if dense is None:
                rows.update(cloud_info=None, _clouds=None)
            else:
                rows.update(cloud_info=T(ND, hip_lib.SCENE_CLOUD_INFO_DTYPE, (n,), zero=True), _clouds=T(tuple),
                            _info=T(ND, hip_lib.SCENE_CLOUD_INFO_DTYPE, (max(n, 1),), zero=True))
            _check_rows(tag, job, batch.device, rows)
            assert job.style is style and (dense is None or type(job._clouds[0]) is hip_lib.SceneClouds), tag
            dst = dict(segments=("segments", 0), pixels=("buffer", 0), capacity=n * image_bytes)
            mem = DEVICE if device else HOST
            if dense is None:
                want = [plain, "ctx", _ints(seqs), n, want_style, want_cams, dst, mem]
            else:
                layer = dict(live=1, what=0, cloud=_plain(hip_lib.cloud_style(4, 0, 0, 0, "world", "compact", 0.0, 40.0, 0.0)),
                             check=_plain(hip_lib.StereoCheck()), point_size=1, _reserved=[0, 0, 0], extra=None, info=("info", 0))
                want = [clouds, "ctx", _ints(seqs), n, want_style, layer, want_cams, dst, mem]
            _submit_twice(tag, rec, job, lambda j: dict(segments=j._seg, buffer=j._buf, info=getattr(j, "_info", None)), want,
                          1 if device else 0)
            assert (job.segments["status"] == hip_lib.SCENE_OK).all(), tag
            _check_images(tag, job, n, device, (48, 64, 3))
    front = hip_lib.scene_preset("front", 64, 48)
    with pytest.raises(ValueError, match="2 cameras for 3 named slots: one per named slot, or a single one for all"):
        Scenes(batch, None, style, [front, front], False)
    with pytest.raises(ValueError, match=r"dense: unknown keys \['stride'\]"):
        Scenes(batch, None, style, front, False, dict(stride=2))
    with pytest.raises(ValueError, match="1 clouds for 3 named slots: one per named slot"):
        Scenes(batch, None, style, front, False, None, [None])


def test_ar_pictures(ctx, monkeypatch):
    batch, cfg = ctx
    plain, occluded = "svo_submit_export_ar", "svo_submit_export_ar_occluded"
    rec = Recorder(monkeypatch, [plain, occluded])
    box = hip_lib.ar_box(0.2)
    model = hip_lib.ar_model(hip_lib.AR_AT)
    W, H = cfg["width"], cfg["height"]
    for occlusion in (None, dict(step=8, hidden="dim", max_depth=40.0)):
        for seqs, n, device in _cases():
            first = [0, 1, 1] if n == 2 else None
            tag = ("ArPictures", occlusion is not None, seqs, device)
            style = hip_lib.ar_style("rgba8")
            want_style = _plain(hip_lib.ar_style("rgba8"))
            pitch, image_bytes = hip_lib.ar_size(batch.cam, W, H, style)
            job = ArPictures(batch, seqs, style, [box], [(model, 0, 0x40c080)], first, device, occlusion)
            rows = dict(_names(n, seqs), cols=W, rows=H, pitch=pitch, image_bytes=image_bytes, channels=4, _dst=T(hip_lib.ArDst),
                        _meshes=T(hip_lib.ArMesh * 1), _n_meshes=1, _inst=T(hip_lib.ArInstance * 1), _n_inst=1,
                        _first=None if first is None else T(C.c_int * 3), **_picture_rows(n, device, image_bytes, hip_lib.AR_SEGMENT_DTYPE))
            if occlusion is None:
                rows.update(visibility=None, _occlusion=None)
            else:
                rows.update(visibility=T(ND, hip_lib.AR_VISIBILITY_DTYPE, (n,), zero=True), _occlusion=T(hip_lib.ArOcclusion))
            _check_rows(tag, job, batch.device, rows)
            assert job.style is style, tag
            meshes = [dict(vertices=("vertices", 0), triangles=("triangles", 0), rgb=None, n_vertices=8, n_triangles=12, _reserved=0)]
            inst = [_plain(hip_lib.ar_instance(model, 0, 0x40c080))]
            dst = dict(segments=("segments", 0), pixels=("buffer", 0), capacity=n * image_bytes)
            mem = DEVICE if device else HOST
            if occlusion is None:
                want = [plain, "ctx", _ints(seqs), n, want_style, meshes, 1, inst, _ints(first), 1, dst, mem]
            else:
                hide = dict(_plain(hip_lib.ar_occlusion(True, step=8, hidden="dim", max_depth=40.0)), info=("visibility", 0))
                want = [occluded, "ctx", _ints(seqs), n, want_style, hide, meshes, 1, inst, _ints(first), 1, dst, mem]
            buffers = lambda j: dict(segments=j._seg, buffer=j._buf, vertices=j._keep[0], triangles=j._keep[1],
                                     visibility=getattr(j, "_vis", None))
            _submit_twice(tag, rec, job, buffers, want, 1 if device else 0)
            assert (job.segments["status"] == hip_lib.AR_OK).all(), tag
            _check_images(tag, job, n, device, (H, W, 4))
    with pytest.raises(ValueError, match="mesh 0: 2 colours for 12 triangles"):
        ArPictures(batch, None, style, [(box[0], box[1], [1, 2])], [], None, False)
    with pytest.raises(ValueError, match=r"occlusion: unknown keys \['stride'\]"):
        ArPictures(batch, None, style, [box], [], None, False, dict(stride=2))


# ------------------------------------------------------------------------------------------------ StereoSlam.get_*

def _getters(slam):
    objects = [(*hip_lib.ar_box(0.2), hip_lib.ar_model(hip_lib.AR_AT), 0xc08040)]
    return dict(image=lambda: slam.get_image("frames", pixel="rgb8"), disparity=lambda: slam.get_disparity("frames", step=4),
                cloud=lambda: slam.get_cloud("frames", step=4), organized=lambda: slam.get_cloud("frames", step=4, layout="organized"),
                voxel_map=lambda: slam.get_voxel_map(min_count=1), scene=lambda: slam.get_scene("top", cols=64, rows=48),
                ar=lambda: slam.get_ar(objects), ar_occluded=lambda: slam.get_ar(objects, occlusion=dict(step=8)))


def test_getters_of_one_sequence():
    cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", 2, 1)
    torch.cuda.synchronize()
    slam = StereoSlam(cfg)
    for name, get in _getters(slam).items():
        assert get() is None, name                           # no ctx yet
    assert slam.ar_visibility is None
    slam.new_image(L[0], R[0], float(ts[0]))
    slam.set_voxel_maps(VOXEL, LOG2)
    slam.fuse_clouds("last_keyframes", None, step=16)
    W, H = cfg["width"], cfg["height"]
    shapes = dict(image=(H, W, 3), scene=(48, 64, 3), ar=(H, W, 3), ar_occluded=(H, W, 3))
    ndims = dict(disparity=3, organized=2)
    dtypes = dict(image=np.uint8, disparity=np.float32, scene=np.uint8, ar=np.uint8, ar_occluded=np.uint8)
    for name, get in _getters(slam).items():
        a = get()
        assert type(a) is ND and a.base is None and a.flags.owndata, name          # its own memory, not the job's
        assert a.dtype == dtypes.get(name, hip_lib.MAP_POINT_DTYPE), name
        if name in shapes:
            assert a.shape == shapes[name], (name, a.shape)
        else:
            assert a.ndim == ndims.get(name, 1) and a.size > 0, name
        if name == "ar":
            assert slam.ar_visibility is None
        if name == "ar_occluded":
            assert slam.ar_visibility.dtype == hip_lib.AR_VISIBILITY_DTYPE and slam.ar_visibility.shape == ()
    slam.close()
