"""Every svo_submit_* entry of the ctx, called through raw ctypes with its smallest valid arguments and one thing
wrong (or two, which pins the order of the checks): the return code and the text of svo_last_error() are compared with
a table that was written by reading the entries' source, not recorded from a run. One ctx of the `tiny` configuration,
4 slots in 2 groups, two frames played. Nothing of it is queued: afterwards a further frame set steps all four slots and
export_frames() equals the getters.

A second ctx is failed the way test_failure_in_one_group_latches_the_ctx (test_tracker_gpu.py) does it, on the host: a
frame set that hands one sequence only one of its two images. There the same table holds (the check of the failed ctx is
every entry's last), and a valid call of every entry returns "<entry>: an earlier frame of this ctx failed; create a new
ctx"."""
import ctypes as C

import numpy as np
import pytest

from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch
from test_export_gpu import _check_frames, _frame_set, _getter_state, _sequences

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -4
N_SLOTS = 4
NAMED = (0, 2)                     # one slot of each group
TWICE, RANGE = (2, 2), (0, N_SLOTS)


def _ints(values):
    return None if values is None else (C.c_int * max(len(values), 1))(*values)


def _arg(v):
    """a Python value as a ctypes argument: structures by reference, numpy arrays and addresses as pointers"""
    if isinstance(v, C.Structure):
        return C.byref(v)
    if isinstance(v, np.ndarray):
        return C.c_void_p(v.ctypes.data)
    return v


class Addr(int):
    """an address (an int would travel as a C int)"""


def _call(name, *args):
    fn = getattr(hip_lib.lib(), name)
    rc = fn(*[C.c_void_p(int(a)) if isinstance(a, Addr) else _arg(a) for a in args])
    return rc, hip_lib.lib().svo_last_error().decode()


class Entry:
    """one entry point: the order of its arguments and a valid call's values; (seqs, n) come from `seqs` (a tuple, or
    None for every slot) unless `n` is given"""

    def __init__(self, name, order, **base):
        self.name, self.order, self.base = name, order, base

    def __call__(self, **over):
        a = dict(self.base, **over)
        if "n" not in a:
            a["n"] = 0 if a["seqs"] is None else len(a["seqs"])
        a["seqs"] = _ints(a["seqs"])
        return _call(self.name, *[a[k] for k in self.order])


def _slot(name, s):
    return (INVALID, f"{name}: sequence {s} is out of range or named twice")


def _table(batch, cfg, saved=None):
    """[(label, (rc, text) got, (rc, text) expected)] of the rejected calls (they are made here), and [(the entry as its
    messages spell it, a valid call of it)] (not made here); saved: snapshots of the slots NAMED for svo_submit_load's"""
    ctx, cam, W, H = batch._ctx, batch.cam, cfg["width"], cfg["height"]
    out, valid = [], []

    def case(label, got, rc, text):
        out.append((label, got, (rc, text)))

    def slots(entry, name, bad_arguments):
        """the naming checks every entry with (seqs, n) makes alike; bad_arguments: what the entry says to n < 0"""
        case(f"{name} n < 0", entry(seqs=NAMED, n=-1), *bad_arguments)
        case(f"{name} out of range", entry(seqs=RANGE), *_slot(name, N_SLOTS))
        case(f"{name} negative slot", entry(seqs=(-1, 1)), *_slot(name, -1))
        case(f"{name} named twice", entry(seqs=TWICE), *_slot(name, 2))
        case(f"{name} twice before range", entry(seqs=(1, 1, 7)), *_slot(name, 1))

    # one block of memory for every destination: nothing is written, but a call accepted by mistake stays inside it
    seg = np.zeros(64 * N_SLOTS + 64, np.uint8)
    view_style, disp_style, cloud_style = hip_lib.view_style(), hip_lib.disparity_style(), hip_lib.cloud_style()
    lr1_disp, lr1_cloud = hip_lib.stereo_check(True, 0.0), hip_lib.stereo_check(True, 1.0)
    scene_style, ar_style = hip_lib.scene_style(cols=32, rows=32), hip_lib.ar_style()
    cap = batch.export_capacity()
    view_bytes = batch.view_size(view_style)[3]
    disp_bytes, disp_bytes_lr = batch.disparity_size(disp_style)[3], batch.disparity_size(disp_style, lr1_disp)[3]
    cloud_points = batch.cloud_size(cloud_style)[2]
    scene_bytes = hip_lib.scene_size(scene_style)[1]
    ar_bytes = hip_lib.ar_size(cam, W, H, ar_style)[1]
    room = np.zeros(2 * max(cap * 44, view_bytes, disp_bytes_lr, cloud_points * 16, scene_bytes, ar_bytes) + 128, np.uint8)
    S = Addr((seg.ctypes.data + 63) // 64 * 64)
    M = Addr((room.ctypes.data + 63) // 64 * 64)
    off = lambda k: Addr(M + k)

    # ---------------------------------------------------------------- svo_submit_images
    name = "svo_submit_images"
    ptrs, ts = (C.c_void_p * N_SLOTS)(), (C.c_float * N_SLOTS)()
    e = Entry(name, ("ctx", "left", "right", "stride", "ts", "mem"), ctx=ctx, left=ptrs, right=ptrs, stride=W, ts=ts, mem=0,
              seqs=None)
    valid.append((name, e))
    for label, over in (("NULL ctx", dict(ctx=None)), ("NULL left", dict(left=None)), ("NULL right", dict(right=None)),
                        ("NULL time stamps", dict(ts=None)), ("NULL ctx, short stride", dict(ctx=None, stride=W - 1))):
        case(f"{name} {label}", e(**over), INVALID, f"{name}: bad arguments")
    case(f"{name} short stride", e(stride=W - 1), INVALID, f"{name}: stride {W - 1} is below the row's bytes")
    case(f"{name} NULL left, short stride", e(left=None, stride=0), INVALID, f"{name}: bad arguments")

    # ---------------------------------------------------------------- svo_submit_trim_keyframes
    name = "svo_submit_trim_keyframes"
    e = Entry(name, ("ctx", "seqs", "below", "n"), ctx=ctx, seqs=NAMED, below=None)
    valid.append((name, e))
    case(f"{name} NULL ctx", e(ctx=None), INVALID, f"{name}: bad arguments")
    case(f"{name} NULL ctx, bad slot", e(ctx=None, seqs=RANGE), INVALID, f"{name}: bad arguments")
    slots(e, name, (INVALID, f"{name}: bad arguments"))

    # ---------------------------------------------------------------- svo_submit_export
    name = "svo_submit_export"
    dst = lambda **kw: hip_lib.ExportDst(**dict(dict(segments=S, kps2d=None, kps3d=None, info=M, capacity=2 * cap), **kw))
    e = Entry(name, ("ctx", "what", "seqs", "n", "dst", "mem"), ctx=ctx, what=0, seqs=NAMED, dst=dst(), mem=0)
    valid.append((name, e))
    bad = lambda what=0, mem=0: (INVALID, f"{name}: bad arguments (what {what}, mem {mem})")
    case(f"{name} NULL ctx", e(ctx=None), *bad())
    case(f"{name} NULL dst", e(dst=None), *bad())
    case(f"{name} NULL segments", e(dst=dst(segments=None)), *bad())
    case(f"{name} bad what", e(what=2), *bad(what=2))
    case(f"{name} bad mem", e(mem=2), *bad(mem=2))
    slots(e, name, bad())
    case(f"{name} misaligned", e(dst=dst(info=off(2))), INVALID, f"{name}: an array is not 4-byte aligned")
    short = (CAPACITY, f"{name}: 2 slots need arrays of {2 * cap} records, capacity {2 * cap - 1}")
    case(f"{name} short capacity", e(dst=dst(capacity=2 * cap - 1)), *short)
    case(f"{name} every slot, short capacity", e(seqs=None, n=-3, dst=dst(capacity=N_SLOTS * cap - 1)), CAPACITY,
         f"{name}: {N_SLOTS} slots need arrays of {N_SLOTS * cap} records, capacity {N_SLOTS * cap - 1}")
    case(f"{name} bad what, bad slot", e(what=-1, seqs=RANGE), *bad(what=-1))
    case(f"{name} bad slot, misaligned", e(seqs=TWICE, dst=dst(kps2d=off(1))), *_slot(name, 2))
    case(f"{name} bad slot, short capacity", e(seqs=RANGE, dst=dst(capacity=0)), *_slot(name, N_SLOTS))
    case(f"{name} misaligned, short capacity", e(dst=dst(kps3d=off(3), capacity=0)), INVALID, f"{name}: an array is not 4-byte aligned")

    # ---------------------------------------------------------------- svo_submit_export_map
    name = "svo_submit_export_map"
    regions = lambda *rows: np.array(list(rows), hip_lib.MAP_REGION_DTYPE)
    good = (0, 0, 0, 0, 0)
    dst = lambda **kw: hip_lib.MapDst(**dict(dict(segments=S, keyframes=None, points=None), **kw))
    e = Entry(name, ("ctx", "seqs", "n", "regions", "filter", "dst", "mem"), ctx=ctx, seqs=NAMED, regions=regions(good, good),
              filter=None, dst=dst(), mem=0)
    valid.append((name, e))
    bad = lambda mem=0: (INVALID, f"{name}: bad arguments (mem {mem})")
    case(f"{name} NULL ctx", e(ctx=None), *bad())
    case(f"{name} NULL dst", e(dst=None), *bad())
    case(f"{name} NULL segments", e(dst=dst(segments=None)), *bad())
    case(f"{name} bad mem", e(mem=3), *bad(mem=3))
    slots(e, name, bad())
    case(f"{name} no regions", e(regions=None), INVALID, f"{name}: no regions")
    case(f"{name} every slot, no regions", e(seqs=None, regions=None), INVALID, f"{name}: no regions")
    flags = (INVALID, f"{name}: drop_flags 0x8 has unknown bits, or _reserved is not 0")
    case(f"{name} unknown flag", e(filter=hip_lib.MapFilter(8, 0, 0, 0)), *flags)
    case(f"{name} filter _reserved", e(filter=hip_lib.MapFilter(1, 0, 0, 5)), INVALID,
         f"{name}: drop_flags 0x1 has unknown bits, or _reserved is not 0")
    case(f"{name} misaligned", e(dst=dst(points=off(8))), INVALID, f"{name}: points is not 16-byte aligned")
    case(f"{name} negative field", e(regions=regions(good, (0, 0, 0, 0, -1))), INVALID, f"{name}: region 1 has a negative field")
    case(f"{name} capacity without array", e(regions=regions((0, 1, 0, 0, 0), good)), INVALID,
         f"{name}: region 0 has a capacity, but its array is NULL")
    case(f"{name} keyframe capacity without array", e(regions=regions(good, (0, 0, 0, 1, 0)), dst=dst(points=M)), INVALID,
         f"{name}: region 1 has a capacity, but its array is NULL")
    case(f"{name} bad filter, bad slot", e(seqs=RANGE, filter=hip_lib.MapFilter(8, 0, 0, 0)), *flags)
    case(f"{name} misaligned, bad slot", e(seqs=RANGE, dst=dst(points=off(4))), INVALID, f"{name}: points is not 16-byte aligned")
    case(f"{name} bad name at 1, bad region at 0", e(seqs=RANGE, regions=regions((-1, 0, 0, 0, 0), good)), INVALID,
         f"{name}: region 0 has a negative field")
    case(f"{name} bad name at 1, bad region at 1", e(seqs=RANGE, regions=regions(good, (-1, 0, 0, 0, 0))), *_slot(name, N_SLOTS))
    case(f"{name} bad name at 0, bad region at 0", e(seqs=(-1, 0), regions=regions((-1, 0, 0, 0, 0), good)), *_slot(name, -1))

    # ---------------------------------------------------------------- views, disparity, clouds
    def image_entry(entry, name, quiet, args, style_who, field, align, align_text, per_slot, units):
        """entry: the symbol called; name: the entry its messages spell (the checked entries report under the unchecked
        one's); style_who: the name a bad style is reported under"""
        make = {"svo_submit_export_views": hip_lib.ViewDst, "svo_submit_export_disparity": hip_lib.DisparityDst,
                "svo_submit_export_cloud": hip_lib.CloudDst}[name]
        dst = lambda **kw: make(**dict({"segments": S, field: M, "capacity": 2 * per_slot}, **kw))
        e = Entry(entry, ("ctx", "what", "seqs", "n", "style") + (("check",) if "check" in args else ()) + ("dst", "mem"),
                  ctx=ctx, what=0, seqs=NAMED, dst=dst(), mem=0, **args)
        valid.append((name, e))
        bad = lambda what=0, mem=0: (INVALID, f"{name}: bad arguments (what {what}, mem {mem})")
        tag = f"{entry}{quiet}"
        case(f"{tag} NULL ctx", e(ctx=None), *bad())
        case(f"{tag} NULL dst", e(dst=None), *bad())
        case(f"{tag} NULL segments", e(dst=dst(segments=None)), *bad())
        case(f"{tag} bad what", e(what=2), *bad(what=2))
        case(f"{tag} bad mem", e(mem=2), *bad(mem=2))
        case(f"{tag} n < 0", e(n=-1), *bad())
        case(f"{tag} NULL style", e(style=None), INVALID, f"{style_who}: no style")
        case(f"{tag} NULL {field}", e(dst=dst(**{field: None})), INVALID, f"{name}: {field} is NULL or not {align_text} aligned")
        case(f"{tag} misaligned", e(dst=dst(**{field: off(align // 2)})), INVALID, f"{name}: {field} is NULL or not {align_text} aligned")
        case(f"{tag} out of range", e(seqs=RANGE), *_slot(name, N_SLOTS))
        case(f"{tag} named twice", e(seqs=TWICE), *_slot(name, 2))
        short = lambda n: (CAPACITY, f"{name}: {n} slots need {n * per_slot} {units}, capacity {n * per_slot - 1}")
        case(f"{tag} short capacity", e(dst=dst(capacity=2 * per_slot - 1)), *short(2))
        case(f"{tag} every slot, short capacity", e(seqs=None, dst=dst(capacity=N_SLOTS * per_slot - 1)), *short(N_SLOTS))
        case(f"{tag} bad style, bad slot", e(style=None, seqs=RANGE), INVALID, f"{style_who}: no style")
        case(f"{tag} bad mem, bad style", e(mem=-1, style=None), *bad(mem=-1))
        case(f"{tag} misaligned, bad slot", e(seqs=TWICE, dst=dst(**{field: off(1)})), INVALID,
             f"{name}: {field} is NULL or not {align_text} aligned")
        case(f"{tag} bad slot, short capacity", e(seqs=RANGE, dst=dst(capacity=0)), *_slot(name, N_SLOTS))
        return e

    image_entry("svo_submit_export_views", "svo_submit_export_views", "", dict(style=view_style), "svo_submit_export_views",
                "pixels", 4, "4-byte", view_bytes, "bytes")
    name = "svo_submit_export_disparity"
    off_check, bad_off_check = hip_lib.StereoCheck(0, 0.0), hip_lib.StereoCheck(0, -1.0)
    image_entry(name, name, "", dict(style=disp_style), name, "values", 16, "16-byte", disp_bytes, "bytes")
    image_entry(name + "_checked", name, " (no check)", dict(style=disp_style, check=None), name, "values", 16, "16-byte", disp_bytes, "bytes")
    image_entry(name + "_checked", name, " (check off)", dict(style=disp_style, check=off_check), name, "values", 16, "16-byte", disp_bytes, "bytes")
    e = image_entry(name + "_checked", name, " (check on)", dict(style=disp_style, check=lr1_disp), name + "_checked", "values", 16,
                    "16-byte", disp_bytes_lr, "bytes")
    # (a check that is off is checked first of all, under the entry's own name; one that is on with the style)
    text = f"{name}_checked: check: max_lr_diff is negative or not finite"
    case(f"{name}_checked bad off check", e(check=bad_off_check), INVALID, text)
    case(f"{name}_checked bad off check, NULL ctx", e(check=bad_off_check, ctx=None), INVALID, text)
    case(f"{name}_checked bad off check, bad slot", e(check=bad_off_check, seqs=RANGE), INVALID, text)
    case(f"{name}_checked bad on check", e(check=hip_lib.StereoCheck(2, 0.0)), INVALID, f"{name}_checked: check: lr 2")
    case(f"{name}_checked bad on check, NULL ctx", e(check=hip_lib.StereoCheck(2, 0.0), ctx=None), INVALID,
         f"{name}: bad arguments (what 0, mem 0)")
    case(f"{name}_checked bad on check, bad slot", e(check=hip_lib.StereoCheck(1, -1.0), seqs=RANGE), INVALID,
         f"{name}_checked: check: max_lr_diff is negative or not finite")
    name = "svo_submit_export_cloud"
    image_entry(name, name, "", dict(style=cloud_style), name, "points", 16, "16-byte", cloud_points, "records")
    image_entry(name + "_checked", name, " (no check)", dict(style=cloud_style, check=None), name, "points", 16, "16-byte", cloud_points, "records")
    image_entry(name + "_checked", name, " (check off)", dict(style=cloud_style, check=off_check), name, "points", 16, "16-byte", cloud_points, "records")
    e = image_entry(name + "_checked", name, " (check on)", dict(style=cloud_style, check=lr1_cloud), name + "_checked", "points", 16,
                    "16-byte", cloud_points, "records")
    text = f"{name}_checked: check: max_lr_diff is negative or not finite"
    case(f"{name}_checked bad off check", e(check=bad_off_check), INVALID, text)
    case(f"{name}_checked bad off check, NULL ctx", e(check=bad_off_check, ctx=None), INVALID, text)
    case(f"{name}_checked bad off check, bad slot", e(check=bad_off_check, seqs=RANGE), INVALID, text)
    case(f"{name}_checked check without tolerance", e(check=lr1_disp), INVALID, f"{name}_checked: check: a cloud needs max_lr_diff > 0")
    case(f"{name}_checked check without tolerance, bad slot", e(check=lr1_disp, seqs=RANGE), INVALID,
         f"{name}_checked: check: a cloud needs max_lr_diff > 0")
    case(f"{name}_checked bad on check, NULL dst", e(check=lr1_disp, dst=None), INVALID, f"{name}: bad arguments (what 0, mem 0)")

    # ---------------------------------------------------------------- svo_submit_fuse_clouds
    name = "svo_submit_fuse_clouds"
    info = np.zeros(N_SLOTS, hip_lib.FUSE_INFO_DTYPE)
    e = Entry(name, ("ctx", "what", "seqs", "n", "style", "check", "stamp", "info"), ctx=ctx, what=1, seqs=NAMED, style=cloud_style,
              check=None, stamp=1, info=info)
    valid.append((name, e))
    bad = lambda what=1: (INVALID, f"{name}: bad arguments (what {what})")
    case(f"{name} NULL ctx", e(ctx=None), *bad())
    case(f"{name} NULL info", e(info=None), *bad())
    case(f"{name} bad what", e(what=2), *bad(what=2))
    slots(e, name, bad())
    case(f"{name} NULL style", e(style=None), INVALID, "svo_submit_export_cloud: no style")
    case(f"{name} NULL style, check on", e(style=None, check=lr1_cloud), INVALID, "svo_submit_export_cloud_checked: no style")
    frame = (INVALID, f"{name}: frame must be SVO_CLOUD_WORLD and layout 0")
    case(f"{name} camera frame", e(style=hip_lib.cloud_style(frame="camera")), *frame)
    case(f"{name} organized layout", e(style=hip_lib.cloud_style(layout="organized")), *frame)
    case(f"{name} bad off check", e(check=bad_off_check), INVALID, f"{name}: check: max_lr_diff is negative or not finite")
    case(f"{name} bad off check, NULL ctx", e(check=bad_off_check, ctx=None), INVALID, f"{name}: check: max_lr_diff is negative or not finite")
    case(f"{name} check without tolerance", e(check=lr1_disp), INVALID, "svo_submit_export_cloud_checked: check: a cloud needs max_lr_diff > 0")
    case(f"{name} bad what, bad slot", e(what=7, seqs=RANGE), *bad(what=7))
    case(f"{name} bad style, bad slot", e(style=None, seqs=RANGE), INVALID, "svo_submit_export_cloud: no style")
    case(f"{name} camera frame, bad slot", e(style=hip_lib.cloud_style(frame="camera"), seqs=TWICE), *frame)

    # ---------------------------------------------------------------- svo_submit_export_voxel_maps
    name = "svo_submit_export_voxel_maps"
    regions = lambda *rows: np.array(list(rows), hip_lib.VOXEL_REGION_DTYPE)
    good = (0, 0, 0, (0, 0, 0))
    dst = lambda **kw: hip_lib.VoxelDst(**dict(dict(segments=S, points=None), **kw))
    e = Entry(name, ("ctx", "seqs", "n", "regions", "filter", "dst", "mem"), ctx=ctx, seqs=NAMED, regions=regions(good, good),
              filter=None, dst=dst(), mem=0)
    valid.append((name, e))
    bad = lambda mem=0: (INVALID, f"{name}: bad arguments (mem {mem})")
    case(f"{name} NULL ctx", e(ctx=None), *bad())
    case(f"{name} NULL dst", e(dst=None), *bad())
    case(f"{name} NULL segments", e(dst=dst(segments=None)), *bad())
    case(f"{name} bad mem", e(mem=2), *bad(mem=2))
    slots(e, name, bad())
    case(f"{name} no regions", e(regions=None), INVALID, f"{name}: no regions")
    reserved = hip_lib.VoxelFilter(0, 0, (C.c_int32 * 2)(0, 1))
    case(f"{name} filter _reserved", e(filter=reserved), INVALID, f"{name}: a _reserved is not 0")
    case(f"{name} misaligned", e(dst=dst(points=off(8))), INVALID, f"{name}: points is not 16-byte aligned")
    field = lambda i: (INVALID, f"{name}: region {i} has a negative field or a non-zero _reserved")
    case(f"{name} negative field", e(regions=regions(good, (0, -1, 0, (0, 0, 0)))), *field(1))
    case(f"{name} region _reserved", e(regions=regions((0, 0, 0, (0, 0, 1)), good)), *field(0))
    case(f"{name} capacity without array", e(regions=regions(good, (0, 1, 0, (0, 0, 0)))), INVALID,
         f"{name}: region 1 has a capacity, but points is NULL")
    case(f"{name} bad filter, bad slot", e(seqs=RANGE, filter=reserved), INVALID, f"{name}: a _reserved is not 0")
    case(f"{name} no regions, bad filter", e(regions=None, filter=reserved), INVALID, f"{name}: no regions")
    case(f"{name} bad name at 1, bad region at 0", e(seqs=RANGE, regions=regions((-1, 0, 0, (0, 0, 0)), good)), *field(0))
    case(f"{name} bad name at 1, bad region at 1", e(seqs=RANGE, regions=regions(good, (-1, 0, 0, (0, 0, 0)))), *_slot(name, N_SLOTS))

    # ---------------------------------------------------------------- svo_submit_clear_voxel_maps
    name = "svo_submit_clear_voxel_maps"
    e = Entry(name, ("ctx", "seqs", "n"), ctx=ctx, seqs=NAMED)
    valid.append((name, e))
    case(f"{name} NULL ctx", e(ctx=None), INVALID, f"{name}: bad arguments")
    case(f"{name} NULL ctx, bad slot", e(ctx=None, seqs=TWICE), INVALID, f"{name}: bad arguments")
    slots(e, name, (INVALID, f"{name}: bad arguments"))

    # ---------------------------------------------------------------- svo_submit_export_scenes, _scenes_clouds
    name = "svo_submit_export_scenes"
    camera = hip_lib.scene_preset("front", 32, 32)
    blind = hip_lib.SceneCamera.from_buffer_copy(camera)
    blind.f = 0.0
    cameras = lambda *c: (hip_lib.SceneCamera * len(c))(*c)
    dst = lambda **kw: hip_lib.SceneDst(**dict(dict(segments=S, pixels=M, capacity=2 * scene_bytes), **kw))
    bad = lambda mem=0: (INVALID, f"{name}: bad arguments (mem {mem})")
    pixels = (INVALID, f"{name}: pixels is NULL or not 4-byte aligned")
    view = lambda i: (INVALID, f"{name}: camera {i}: an entry is not finite, or f or near is not > 0")
    short = (CAPACITY, f"{name}: 2 slots need {2 * scene_bytes} bytes, capacity {2 * scene_bytes - 1}")
    nothing = hip_lib.scene_clouds()[0]
    for entry, args in ((name, {}), (name + "_clouds", dict(clouds=None)), (name + "_clouds", dict(clouds=nothing))):
        order = ("ctx", "seqs", "n", "style") + (("clouds",) if args else ()) + ("cameras", "dst", "mem")
        e = Entry(entry, order, ctx=ctx, seqs=NAMED, style=scene_style, cameras=cameras(camera, camera), dst=dst(), mem=0, **args)
        valid.append((name, e))
        tag = entry + (" (nothing to draw)" if args.get("clouds") is not None else "")
        case(f"{tag} NULL ctx", e(ctx=None), *bad())
        case(f"{tag} NULL dst", e(dst=None), *bad())
        case(f"{tag} NULL segments", e(dst=dst(segments=None)), *bad())
        case(f"{tag} NULL cameras", e(cameras=None), *bad())
        case(f"{tag} bad mem", e(mem=2), *bad(mem=2))
        case(f"{tag} n < 0", e(n=-2), *bad())
        case(f"{tag} NULL style", e(style=None), INVALID, f"{name}: no style")
        case(f"{tag} NULL pixels", e(dst=dst(pixels=None)), *pixels)
        case(f"{tag} misaligned", e(dst=dst(pixels=off(2))), *pixels)
        case(f"{tag} out of range", e(seqs=RANGE), *_slot(name, N_SLOTS))
        case(f"{tag} named twice", e(seqs=TWICE), *_slot(name, 2))
        case(f"{tag} bad camera", e(cameras=cameras(camera, blind)), *view(1))
        case(f"{tag} short capacity", e(dst=dst(capacity=2 * scene_bytes - 1)), *short)
        case(f"{tag} bad style, bad slot", e(style=None, seqs=RANGE), INVALID, f"{name}: no style")
        case(f"{tag} misaligned, bad slot", e(dst=dst(pixels=off(1)), seqs=RANGE), *pixels)
        case(f"{tag} bad slot, short capacity", e(seqs=RANGE, dst=dst(capacity=0)), *_slot(name, N_SLOTS))
        case(f"{tag} bad camera, short capacity", e(cameras=cameras(blind, camera), dst=dst(capacity=0)), *view(0))
        case(f"{tag} bad name at 1, bad camera at 0", e(seqs=RANGE, cameras=cameras(blind, camera)), *view(0))
        case(f"{tag} bad name at 1, bad camera at 1", e(seqs=RANGE, cameras=cameras(camera, blind)), *_slot(name, N_SLOTS))
    # (clouds with nothing to draw are checked before anything else, unless the ctx is NULL; others after the cameras)
    who = name + "_clouds"
    thick = hip_lib.scene_clouds(point_size=17)[0]
    size = (INVALID, f"{who}: point_size 17 is not within 1 .. 16")
    case(f"{who} nothing to draw, bad size", e(clouds=thick), *size)
    case(f"{who} nothing to draw, bad size, NULL dst", e(clouds=thick, dst=None), *size)
    case(f"{who} nothing to draw, bad size, bad slot", e(clouds=thick, seqs=RANGE), *size)
    case(f"{who} nothing to draw, bad size, NULL ctx", e(clouds=thick, ctx=None), *bad())
    live = hip_lib.scene_clouds(live=True, what=2)[0]
    case(f"{who} live, bad what", e(clouds=live), INVALID, f"{who}: what 2")
    case(f"{who} live, bad what, NULL dst", e(clouds=live, dst=None), *bad())
    case(f"{who} live, bad what, bad slot", e(clouds=live, seqs=RANGE), *_slot(name, N_SLOTS))
    case(f"{who} live, bad what, bad camera", e(clouds=live, cameras=cameras(blind, camera)), *view(0))
    case(f"{who} live, bad what, short capacity", e(clouds=live, dst=dst(capacity=0)), INVALID, f"{who}: what 2")
    spans, keep = hip_lib.scene_clouds(extra=[None, (0, 0)])
    keep[0][1].n = -1
    span = (INVALID, f"{who}: span 1: n -1 must be >= 0 and its records device memory, 16-byte aligned")
    case(f"{who} bad span", e(clouds=spans), *span)
    case(f"{who} bad span, short capacity", e(clouds=spans, dst=dst(capacity=0)), *span)
    case(f"{who} bad span, bad slot", e(clouds=spans, seqs=TWICE), *_slot(name, 2))
    spans2, keep2 = hip_lib.scene_clouds(extra=[None, (0, 0)])
    case(f"{who} spans, short capacity", e(clouds=spans2, dst=dst(capacity=2 * scene_bytes - 1)), *short)
    valid.append((name, lambda e=e: e(clouds=spans2)))

    # ---------------------------------------------------------------- svo_submit_export_ar, _ar_occluded
    vertices, triangles = hip_lib.ar_box()
    wrong = triangles.copy()
    wrong[0, 1] = 8
    mesh = lambda t: (hip_lib.ArMesh * 1)(hip_lib.ArMesh(vertices.ctypes.data, t.ctypes.data, None, len(vertices), len(t)))
    instances = lambda m: (hip_lib.ArInstance * 1)(hip_lib.ar_instance(hip_lib.ar_model(), mesh=m))
    dst = lambda **kw: hip_lib.ArDst(**dict(dict(segments=S, pixels=M, capacity=2 * ar_bytes), **kw))
    occlusion_off = hip_lib.ar_occlusion(on=False)
    occlusion_bad = hip_lib.ar_occlusion(on=False)
    occlusion_bad.on = 2
    for name, args in (("svo_submit_export_ar", {}), ("svo_submit_export_ar_occluded", dict(occlusion=None)),
                       ("svo_submit_export_ar_occluded", dict(occlusion=occlusion_off))):
        order = ("ctx", "seqs", "n", "style") + (("occlusion",) if args else ()) + ("meshes", "n_meshes", "instances", "first",
                                                                                   "n_instances", "dst", "mem")
        e = Entry(name, order, ctx=ctx, seqs=NAMED, style=ar_style, meshes=None, n_meshes=0, instances=None, first=None, n_instances=0,
                  dst=dst(), mem=0, **args)
        valid.append((name, e))
        tag = name + (" (occlusion off)" if args.get("occlusion") is not None else "")
        bad = lambda mem=0, meshes=0, inst=0: (INVALID, f"{name}: bad arguments (mem {mem}, {meshes} meshes, {inst} instances)")
        pixels = (INVALID, f"{name}: pixels is NULL or not 4-byte aligned")
        case(f"{tag} NULL ctx", e(ctx=None), *bad())
        case(f"{tag} NULL dst", e(dst=None), *bad())
        case(f"{tag} NULL segments", e(dst=dst(segments=None)), *bad())
        case(f"{tag} bad mem", e(mem=2), *bad(mem=2))
        case(f"{tag} n < 0", e(n=-1), *bad())
        case(f"{tag} meshes < 0", e(n_meshes=-1), *bad(meshes=-1))
        case(f"{tag} NULL meshes", e(n_meshes=1), *bad(meshes=1))
        case(f"{tag} NULL instances", e(n_instances=3), *bad(inst=3))
        case(f"{tag} NULL style", e(style=None), INVALID, f"{name}: no style")
        case(f"{tag} NULL pixels", e(dst=dst(pixels=None)), *pixels)
        case(f"{tag} misaligned", e(dst=dst(pixels=off(2))), *pixels)
        case(f"{tag} out of range", e(seqs=RANGE), *_slot(name, N_SLOTS))
        case(f"{tag} named twice", e(seqs=TWICE), *_slot(name, 2))
        case(f"{tag} first ends early", e(first=_ints((0, 0, 0)), meshes=mesh(triangles), n_meshes=1, instances=instances(0), n_instances=1),
             INVALID, f"{name}: first starts at 0 and ends at 0, not at >= 0 and 1")
        case(f"{tag} first descends", e(first=_ints((1, 0, 1)), meshes=mesh(triangles), n_meshes=1, instances=instances(0), n_instances=1),
             INVALID, f"{name}: first does not ascend at 0")
        vertex = (INVALID, f"{name}: mesh 0: triangle 0 names vertex 8 of 8")
        case(f"{tag} bad triangle", e(meshes=mesh(wrong), n_meshes=1), *vertex)
        case(f"{tag} bad instance", e(meshes=mesh(triangles), n_meshes=1, instances=instances(1), n_instances=1), INVALID,
             f"{name}: instance 0: a model entry that is not finite, mesh 1 of 1, a colour with a top byte, or a _reserved that is not 0")
        case(f"{tag} short capacity", e(dst=dst(capacity=2 * ar_bytes - 1)), CAPACITY,
             f"{name}: 2 slots need {2 * ar_bytes} bytes, capacity {2 * ar_bytes - 1}")
        case(f"{tag} bad style, bad slot", e(style=None, seqs=RANGE), INVALID, f"{name}: no style")
        case(f"{tag} misaligned, bad slot", e(dst=dst(pixels=off(3)), seqs=RANGE), *pixels)
        case(f"{tag} bad slot, short capacity", e(seqs=RANGE, dst=dst(capacity=0)), *_slot(name, N_SLOTS))
        case(f"{tag} bad slot, bad triangle", e(seqs=TWICE, meshes=mesh(wrong), n_meshes=1), *_slot(name, 2))
        case(f"{tag} bad triangle, short capacity", e(meshes=mesh(wrong), n_meshes=1, dst=dst(capacity=0)), *vertex)
    on = (INVALID, "svo_submit_export_ar_occluded: occlusion: on 2 is neither 0 nor 1")
    case("svo_submit_export_ar_occluded bad occlusion", e(occlusion=occlusion_bad), *on)
    case("svo_submit_export_ar_occluded bad occlusion, bad slot", e(occlusion=occlusion_bad, seqs=RANGE), *on)
    case("svo_submit_export_ar_occluded bad occlusion, NULL pixels", e(occlusion=occlusion_bad, dst=dst(pixels=None)), *on)
    case("svo_submit_export_ar_occluded bad style, bad occlusion", e(style=None, occlusion=occlusion_bad), INVALID,
         "svo_submit_export_ar_occluded: no style")

    # ---------------------------------------------------------------- svo_submit_save, svo_submit_load
    header = C.sizeof(hip_lib.SnapshotInfo)
    host = np.zeros(2 * header, np.uint8)
    snaps = lambda *s: (hip_lib.SnapshotBuffers * len(s))(*[hip_lib.SnapshotBuffers(*x) for x in s])
    good = (host.ctypes.data, header, None, 0)
    for name in ("svo_submit_save", "svo_submit_load"):
        e = Entry(name, ("ctx", "seqs", "n", "snaps", "mem"), ctx=ctx, seqs=NAMED, snaps=snaps(good, good), mem=0)
        bad = lambda mem=0: (INVALID, f"{name}: bad arguments (mem {mem})")
        case(f"{name} NULL ctx", e(ctx=None), *bad())
        case(f"{name} NULL snapshots", e(snaps=None), *bad())
        case(f"{name} NULL seqs", e(seqs=None, n=2), *bad())
        case(f"{name} bad mem", e(mem=2), *bad(mem=2))
        slots(e, name, bad())
        case(f"{name} bad mem, bad slot", e(mem=5, seqs=RANGE), *bad(mem=5))
    if saved is not None:                        # (a load parses its snapshots before it looks at the ctx's state)
        real = (hip_lib.SnapshotBuffers * len(saved))(*[s._buffers() for s in saved])
        valid.append((name, lambda e=e: e(snaps=real)))
    name = "svo_submit_save"
    e = Entry(name, ("ctx", "seqs", "n", "snaps", "mem"), ctx=ctx, seqs=NAMED, snaps=snaps(good, good), mem=0)
    valid.append((name, e))
    part = lambda i: (INVALID, f"{name}: snapshot {i}: the host part needs room for its header, the data part its memory")
    case(f"{name} NULL host part", e(snaps=snaps(good, (None, header, None, 0))), *part(1))
    case(f"{name} short host part", e(snaps=snaps((host.ctypes.data, header - 1, None, 0), good)), *part(0))
    case(f"{name} data capacity without memory", e(snaps=snaps(good, (host.ctypes.data, header, None, 1))), *part(1))
    case(f"{name} bad slot, short host part", e(seqs=RANGE, snaps=snaps((host.ctypes.data, header - 1, None, 0), good)), *_slot(name, N_SLOTS))

    # ---------------------------------------------------------------- svo_submit_pose_updates
    name = "svo_submit_pose_updates"
    samples = np.zeros(2, hip_lib.POSE_SAMPLE_DTYPE)
    samples["dt"] = 0.05
    flagged = samples.copy()
    flagged["flags"][1] = 2
    e = Entry(name, ("ctx", "seqs", "counts", "n", "samples", "filtered"), ctx=ctx, seqs=NAMED, counts=_ints((1, 1)), samples=samples,
              filtered=None)
    valid.append((name, e))
    case(f"{name} NULL ctx", e(ctx=None), INVALID, f"{name}: bad arguments")
    case(f"{name} NULL counts", e(counts=None), INVALID, f"{name}: bad arguments")
    slots(e, name, (INVALID, f"{name}: bad arguments"))
    count = lambda s: (INVALID, f"{name}: sequence {s}: negative count")
    case(f"{name} negative count", e(counts=_ints((1, -1))), *count(2))
    case(f"{name} too many samples", e(counts=_ints((1 << 24, 1)), samples=None), INVALID, f"{name}: 16777217 samples in one call")
    case(f"{name} no samples", e(samples=None), INVALID, f"{name}: no samples")
    case(f"{name} unknown flag", e(samples=flagged), INVALID, f"{name}: sample 1: unknown flag bits 0x2")
    case(f"{name} NULL counts, bad slot", e(counts=None, seqs=RANGE), INVALID, f"{name}: bad arguments")
    case(f"{name} bad name at 1, bad count at 0", e(seqs=RANGE, counts=_ints((-1, 1))), *count(0))
    case(f"{name} bad name at 1, bad count at 1", e(seqs=RANGE, counts=_ints((1, -1))), *_slot(name, N_SLOTS))
    case(f"{name} bad slot, no samples", e(seqs=TWICE, samples=None), *_slot(name, 2))
    case(f"{name} negative count, no samples", e(counts=_ints((1, -1)), samples=None), *count(2))
    return out, valid, (seg, room, host, info, keep, keep2, saved)


def test_rejected_calls_return_what_the_table_says(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = _sequences("tiny", (1, 11), 3)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], N_SLOTS)
    assert batch.groups() == 2
    slots = list(range(N_SLOTS))
    for t in range(2):
        batch.new_images(*_frame_set(N_SLOTS, {s: (seqs[s % 2], t) for s in slots}))
    before = _getter_state(batch)
    table, _, keep = _table(batch, cfg)
    assert len({label for label, _, _ in table}) == len(table)
    wrong = [(label, got, want) for label, got, want in table if got != want]
    assert not wrong, (len(wrong), wrong[:8])
    # nothing was queued: the slots are where they were, a further frame set steps all four, and the export equals the getters
    assert _getter_state(batch) == before
    batch.new_images(*_frame_set(N_SLOTS, {s: (seqs[s % 2], 2) for s in slots}))
    state = _getter_state(batch)
    assert [state[s]["frame_id"] for s in slots] == [2] * N_SLOTS
    _check_frames("after the rejected calls", batch.export_frames(), state, slots, {s: (0, seqs[s % 2][2][2]) for s in slots})
    batch.close()
    del keep


def test_a_failed_ctx_rejects_valid_calls_last(monkeypatch):
    import torch
    from stereo_svo_slam_amd import synth
    from stereo_svo_slam_amd.hip_lib import SvoError
    monkeypatch.setenv("SVO_GROUPS", "2")
    seqs = [synth.make_sequence("tiny", 2, 30 + s, device="cpu") for s in range(N_SLOTS)]
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], N_SLOTS)
    assert batch.groups() == 2
    dl = [[s[1][k].cuda() for s in seqs] for k in range(2)]
    dr = [[s[2][k].cuda() for s in seqs] for k in range(2)]
    torch.cuda.synchronize()
    batch.new_images_packed(batch.pack_images(dl[0], dr[0], [0.0] * N_SLOTS))
    saved = batch.save(list(NAMED))
    bad = batch.pack_images(dl[1], dr[1], [0.05] * N_SLOTS)
    bad[1][3] = None                                   # sequence 3 (second group): right image missing
    batch.submit_packed(bad)
    with pytest.raises(SvoError, match="only one image"):
        batch.wait()
    frames = batch.totals().frames
    table, valid, keep = _table(batch, cfg, saved)
    wrong = [(label, got, want) for label, got, want in table if got != want]
    assert not wrong, (len(wrong), wrong[:8])
    assert len(valid) == 26 and "svo_submit_load" in [name for name, _ in valid]
    got = [(name, call()) for name, call in valid]
    wrong = [(name, g) for name, g in got if g != (INVALID, f"{name}: an earlier frame of this ctx failed; create a new ctx")]
    assert not wrong, wrong[:8]
    assert batch.totals().frames == frames
    batch.close()
    del keep
