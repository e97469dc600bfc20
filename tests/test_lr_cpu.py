"""The left-right cross-check without a GPU: the numpy statement (tests/lr_ref.py) against the oracle's per-keypoint
search on the mirrored planes of the crafted pairs (tests/lr_cases.py), what keeps those pairs honest, the layout of
svo_stereo_check against the Python type, svo_disparity_size_checked and what it rejects, and the kept set of a checked
cloud. Bit for bit throughout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import dense_ref as DR
import lr_cases as LC
import lr_ref as LR
import oracle_py as O
from stereo_svo_slam_amd import hip_lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = hip_lib.CameraSettings.from_dict(synth.CONFIGS["tiny"])
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_lr_plane(left, right, win, sx, sy, step, disp):
    """the lr plane from the oracle: oracle_py.ssd_disparity on the mirrored planes at the keypoints (W - 1 - xr, y) of
    the lattice points that have a matched column inside the image"""
    h, w = left.shape
    cols, rows, xs, ys = DR.lattice(w, h, step)
    lm, rm = LR.mirrored(left, right)
    out = np.where(disp < 0, F(LR.INVALID), F(LR.NO_WAY_BACK)).astype(F)
    at, kps = [], []
    for iy in range(rows):
        for ix in range(cols):
            if disp[iy, ix] >= 0:
                xr = LR.matched_column(xs[ix], disp[iy, ix])
                if xr <= w - 1:
                    at.append((iy, ix))
                    kps.append((w - 1 - xr, ys[iy]))
    rd = np.asarray(O.ssd_disparity(lm, rm, np.asarray(kps, F).reshape(-1, 2), win, sx, sy, 1), F)
    for (iy, ix), r in zip(at, rd):
        if r >= 0:
            out[iy, ix] = np.abs(F(disp[iy, ix]) - r)
    return out


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_statement_equals_the_oracle(name):
    left, right, win, sx, sy, step = LC.cases()[name]
    want = oracle_lr_plane(left, right, win, sx, sy, step, LC.forward(name)[0])
    assert np.array_equal(_bits(LC.reference(name)), _bits(want))


def test_the_cases_reach_what_they_are_for():
    """Each of -1, -2, a zero and a value above the tolerance occurs; the shares at max_lr_diff = 1 lie within 0.05 of
    the issue's table. The half-occluded band of `occl`: the issue names columns 34 .. 39 (left of the foreground
    block). In this project's convention a match lies at x + d in the right image, so the background that the block
    hides in the right image is what the left image shows in columns 60 .. 65, right of the block (left x is hidden
    iff 49 <= x + 3 <= 68 and x is not in 40 .. 59). Measured with the statement: 0.000 of columns 34 .. 39 and 0.896
    of columns 60 .. 65 of rows 8 .. 31 fail at step 1. The band is asserted where it lies."""
    seen = set()
    for name in sorted(LC.cases()):
        lr = LC.reference(name)
        assert np.array_equal(lr == LR.INVALID, LC.forward(name)[0] < 0), name
        assert ((lr >= 0) | (lr == LR.INVALID) | (lr == LR.NO_WAY_BACK)).all(), name
        seen |= {k for k, m in (("-1", lr == -1), ("-2", lr == -2), ("0", lr == 0), (">1", lr > 1)) if m.any()}
        if name in LC.SHARES:
            fails = LR.fails(lr, 1.0)
            got = (float((~fails).mean()), float((lr == -2).mean()), float((lr > 1).mean()))
            print(name, "kept %.3f, -2 %.3f, > 1 %.3f" % got)
            for g, w in zip(got, LC.SHARES[name]):
                assert abs(g - w) <= 0.05, (name, got, LC.SHARES[name])
    assert seen == {"-1", "-2", "0", ">1"}
    assert abs(float((LC.forward("f")[0] < 0).mean()) - 0.600) <= 0.05
    band = LR.fails(LC.reference("occl1"), 1.0)[8:32, 60:66]
    print("occl1: the half-occluded band fails at %.3f" % float(band.mean()))
    assert float(band.mean()) > 0.5
    # a seam of the mirrored column tiles lies inside `wide` at both windows (a tile spans 257 - win columns)
    for name in ("wide1", "wide2"):
        left, _, win, _, _, _ = LC.cases()[name]
        assert 257 - win < left.shape[1] <= 2 * (257 - win) and left.shape[1] % 2 == 1


def test_checked_planes_and_the_clouds_kept_set():
    """masking and depth of the checked planes, and: the kept set of a checked cloud (the filter of "clouds" on the
    masked disparity plane) is cloud_ref.kept_mask & ~fails"""
    rig = dict(fx=212.0, fy=212.0, cx=48.0, cy=20.0, baseline=23.5)
    for name in ("occl1", "f", "b"):
        left, right, win, sx, sy, step = LC.cases()[name]
        h, w = left.shape
        fwd, lr = LC.forward(name), LC.reference(name)
        fails = LR.fails(lr, 1.0)
        report = LR.checked_planes(fwd, lr, DR.DISPARITY, True, max_lr_diff=0.0)
        assert report.shape[0] == 3 and np.array_equal(_bits(report[:2]), _bits(fwd)) and np.array_equal(_bits(report[2]), _bits(lr))
        masked = LR.checked_planes(fwd, lr, DR.DISPARITY, False, max_lr_diff=1.0)
        assert masked.shape[0] == 2 and (masked[0][fails] == -1).all() and np.array_equal(_bits(masked[0][~fails]), _bits(fwd[0][~fails]))
        depth = LR.checked_planes(fwd, lr, DR.DEPTH, True, baseline=20.0, max_lr_diff=1.0)
        assert (depth[0][fails] == 0).all() and np.array_equal(_bits(depth[0][~fails]), _bits(F(20.0) / fwd[0][~fails]))
        assert np.array_equal(_bits(depth[1]), _bits(fwd[1]))
        z = CR.local_points(fwd, w, h, step, rig)[2]
        kw = dict(min_disparity=1.0, max_depth=2000.0, max_mean_cost=900.0)
        plain = CR.kept_mask(fwd, w, h, win, step, z, **kw)
        planes = np.stack([masked[0], fwd[1]])
        checked = CR.kept_mask(planes, w, h, win, step, CR.local_points(planes, w, h, step, rig)[2], **kw)
        assert np.array_equal(checked, plain & ~fails), name
        assert 0 < checked.sum() < plain.sum(), name


def test_struct_layout_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    cls, name = hip_lib.StereoCheck, "svo_stereo_check"
    lines = [f'  printf("{name} %zu\\n", sizeof({name}));\n']
    lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    assert c[name] == [C.sizeof(cls)] == [32]
    for f in cls._fields_:
        assert c[f"{name}.{f[0]}"] == [getattr(cls, f[0]).offset], f[0]
    assert [f[0] for f in cls._fields_] == ["lr", "max_lr_diff", "_reserved"] and C.sizeof(C.c_int32 * 6) == 24
    lib = hip_lib.lib()
    for sym in ("svo_disparity_size_checked", "svo_submit_export_disparity_checked", "svo_export_disparity_checked",
                "svo_dense_disparity_checked", "svo_submit_export_cloud_checked", "svo_export_cloud_checked", "svo_cloud_points_checked"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)
    ck = hip_lib.stereo_check()
    assert (ck.lr, ck.max_lr_diff, list(ck._reserved)) == (1, 0.0, [0] * 6)
    ck = hip_lib.stereo_check(False, 1.5)
    assert (ck.lr, ck.max_lr_diff) == (0, 1.5)


def _style(value=0, step=1, win=0, sx=0, sy=0, cost=0):
    return hip_lib.DisparityStyle(value, step, win, sx, sy, cost)


def _check(lr=1, diff=0.0, reserved=None):
    ck = hip_lib.StereoCheck(lr, diff)
    if reserved is not None:
        ck._reserved[reserved] = 1
    return ck


def test_disparity_size_checked():
    for step in (1, 3, 16):
        for cost in (0, 1):
            for w, h in ((320, 240), (752, 480), (97, 53)):
                plain = hip_lib.disparity_size(CAM, w, h, _style(step=step, cost=cost))
                assert hip_lib.disparity_size(CAM, w, h, _style(step=step, cost=cost), _check(0, 2.0)) == plain     # off: the unchecked shape
                for diff in (0.0, 1.0):
                    cols, rows, planes, nbytes = hip_lib.disparity_size(CAM, w, h, _style(step=step, cost=cost), _check(1, diff))
                    assert (cols, rows, planes) == (w // step, h // step, 2 + cost) == (*plain[:2], plain[2] + 1)
                    assert nbytes == (planes * cols * rows * 4 + 255) // 256 * 256
    assert hip_lib.disparity_size(CAM, 320, 240, _style(), _check()) == (320, 240, 2, 614400)
    lib = hip_lib.lib()
    nbytes, planes = C.c_int64(0), C.c_int(0)
    assert lib.svo_disparity_size_checked(C.byref(CAM), 320, 240, C.byref(_style(step=3, cost=1)), None, None, None, C.byref(planes), C.byref(nbytes)) == 0
    assert (planes.value, nbytes.value) == (2, (2 * 106 * 80 * 4 + 255) // 256 * 256)                                 # NULL: the unchecked entry
    assert lib.svo_disparity_size_checked(C.byref(CAM), 320, 240, C.byref(_style()), C.byref(_check()), None, None, None, None) == 0


def test_disparity_size_checked_rejects():
    bad = [_check(2), _check(-1), _check(1, -1.0), _check(1, float("inf")), _check(1, float("nan")), _check(1, -0.5),
           _check(0, -1.0), _check(0, float("nan")), _check(2, 1.0)] + [_check(lr, 1.0, r) for lr in (0, 1) for r in range(6)]
    for ck in bad:
        with pytest.raises(hip_lib.SvoError):
            hip_lib.disparity_size(CAM, 320, 240, _style(), ck)
    # everything the unchecked entry rejects, with a good check
    for st in (_style(value=2), _style(step=0), _style(step=17), _style(cost=2), _style(win=36), _style(sx=65), _style(sy=9)):
        with pytest.raises(hip_lib.SvoError):
            hip_lib.disparity_size(CAM, 320, 240, st, _check(1, 1.0))
    with pytest.raises(hip_lib.SvoError):
        hip_lib.disparity_size(CAM, 15, 240, _style(step=16), _check())
    lib = hip_lib.lib()
    assert lib.svo_disparity_size_checked(C.byref(CAM), 320, 240, None, C.byref(_check()), None, None, None, None) == -1
    assert lib.svo_disparity_size_checked(None, 320, 240, C.byref(_style()), C.byref(_check()), None, None, None, None) == -1
    # the calls that need a ctx or a handle reject a missing one
    ddst, cdst = hip_lib.DisparityDst(None, None, 0), hip_lib.CloudDst(None, None, 0)
    cst = hip_lib.cloud_style(win=7, search_x=9, search_y=2)
    assert lib.svo_submit_export_disparity_checked(None, 0, None, 0, C.byref(_style()), C.byref(_check()), C.byref(ddst), 0) == -1
    assert lib.svo_export_disparity_checked(None, 0, None, 0, C.byref(_style()), C.byref(_check()), C.byref(ddst), 0) == -1
    assert lib.svo_dense_disparity_checked(None, 0, None, None, C.byref(_style(win=7, sx=9, sy=2)), C.byref(_check()), None) == -1
    assert lib.svo_submit_export_cloud_checked(None, 0, None, 0, C.byref(cst), C.byref(_check(1, 1.0)), C.byref(cdst), 0) == -1
    assert lib.svo_export_cloud_checked(None, 0, None, 0, C.byref(cst), C.byref(_check(1, 1.0)), C.byref(cdst), 0) == -1
    assert lib.svo_cloud_points_checked(None, 0, None, None, C.byref(cst), C.byref(_check(1, 1.0)), None, None) == -1
    assert hip_lib.lib().svo_last_error()
