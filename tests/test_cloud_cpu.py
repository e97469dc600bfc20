"""The dense point cloud without a GPU: the numpy statement (tests/cloud_ref.py) against the oracle's per-keypoint
search and keypoint initialisation on the lattice points of the crafted cases (tests/cloud_cases.py), what keeps those
cases honest, the struct layouts of the C header against the Python types, svo_cloud_size and what it rejects. Bit for
bit throughout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_cases as CC
import cloud_ref as CR
import dense_ref as DR
import oracle_py as O
from stereo_svo_slam_amd import hip_lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = synth.CONFIGS["tiny"]
CAM = hip_lib.CameraSettings.from_dict(CFG)
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_points(c, pose):
    """the kps3d the oracle gives new keypoints at the lattice points of a case: its disparity search feeds its
    keypoint initialisation; float32 [rows * cols, 3] in row-major order"""
    h, w = c["left"].shape
    kps = DR.lattice_keypoints(w, h, c["step"])
    disp = np.asarray(O.ssd_disparity(c["left"], c["right"], kps, c["win"], c["search_x"], c["search_y"], 1), F)
    cam = O.make_camera(**{k: float(c["rig"][k]) for k in CR.RIG_KEYS})
    k3, _, _ = O.depth_init(cam, np.asarray(pose, F), kps, disp, 0, 0, 12345)
    return disp, k3


@pytest.mark.parametrize("name", sorted(CC.cases()))
def test_statement_equals_the_oracle(name):
    c = CC.cases()[name]
    h, w = c["left"].shape
    planes = CC.planes(name)
    valid = (planes[0] >= 0).reshape(-1)
    local = CR.local_points(planes, w, h, c["step"], c["rig"])
    disp, k3 = oracle_points(c, c["pose"])
    assert np.array_equal(_bits(disp), _bits(planes[0].reshape(-1)))
    world = np.stack([p.reshape(-1) for p in CR.world_points(local, c["pose"])], 1)
    assert np.array_equal(_bits(world[valid]), _bits(k3[valid])), name
    # the camera frame is the world frame at the zero pose
    _, k3_zero = oracle_points(c, CC.POSE_ZERO)
    camera = np.stack([p.reshape(-1) for p in local], 1)
    assert np.array_equal(_bits(camera[valid]), _bits(k3_zero[valid])), name
    # ... and the records carry exactly these bits, in row-major order, with the gray of the left plane
    for frame, want in ((CR.WORLD, world), (CR.CAMERA, camera)):
        rec, n = CC.reference(name, frame, CR.ORGANIZED)
        kept = (rec["flags"] == 0)
        assert n == int(kept.sum()) and rec.shape == (valid.size,)
        got = np.stack([rec["x"], rec["y"], rec["z"]], 1)
        assert np.array_equal(_bits(got[kept]), _bits(want[kept])) and not (kept & ~valid).any()
        assert (_bits(got[~kept]) == 0).all() and (rec["flags"][~kept] == CR.DROPPED).all()
        cols, rows, xs, ys = DR.lattice(w, h, c["step"])
        gray = c["left"][np.repeat(ys, cols), np.tile(xs, rows)]
        assert all(np.array_equal(rec["color"][:, k], gray) for k in range(3))
        compact, n2 = CC.reference(name, frame, CR.COMPACT)
        assert n2 == n and compact.tobytes() == rec[kept].tobytes()


def test_the_cases_reach_what_they_are_for():
    cases = CC.cases()
    frac = {}
    for name in sorted(cases):
        planes = CC.planes(name)
        valid = int((planes[0] >= 0).sum())
        assert valid > 0, name
        frac[name] = CC.reference(name, CR.WORLD, CR.COMPACT)[1] / valid
    for name in CC.FILTERED:
        assert any(v != 0 for v in cases[name]["filter"].values())
        assert 0.10 <= frac[name] <= 0.90, (name, frac[name])          # neither side of the predicate goes untested
    assert set(CC.FILTERED) == {n for n in cases if 0 < frac[n] < 1}
    assert frac["all"] == 1 and frac["invalid"] == 1 and frac["none"] == 0
    assert cases["none"]["filter"]["min_disparity"] > cases["none"]["search_x"]
    # in "three" the cost term and the two depth terms (disp < m is z > baseline / m: one of them implies the other)
    # each drop points that the other does not
    c = cases["three"]
    h, w = c["left"].shape
    z = CR.local_points(CC.planes("three"), w, h, c["step"], c["rig"])[2]
    every = CR.kept_mask(CC.planes("three"), w, h, c["win"], c["step"], z, **c["filter"])
    for off in (dict(max_mean_cost=0.0), dict(min_disparity=0.0, max_depth=0.0)):
        without = CR.kept_mask(CC.planes("three"), w, h, c["win"], c["step"], z, **dict(c["filter"], **off))
        assert int(without.sum()) > int(every.sum()), off
    # points that sit exactly on a threshold stay
    d = CC.planes("disparity")[0]
    assert int((d == F(cases["disparity"]["filter"]["min_disparity"])).sum()) > 0
    c = cases["depth"]
    h, w = c["left"].shape
    z = CR.local_points(CC.planes("depth"), w, h, c["step"], c["rig"])[2]
    assert int((z[CC.planes("depth")[0] >= 0] == F(c["filter"]["max_depth"])).sum()) > 0
    # more than one tile and a count that is no multiple of 256; and one that is
    points = {n: CC.planes(n)[0].size for n in cases}
    assert points["all"] > 256 and points["all"] % 256 != 0
    assert points["ties"] > 256 and points["ties"] % 256 == 0
    assert any(p < 256 for p in points.values())
    # disparities clamped to 0.5, fractional disparities, invalid points, costs beyond 2^24
    assert float((CC.planes("clamped")[0] == F(0.5)).mean()) > 0.5
    t = CC.planes("ties")[0]
    assert float((t != np.round(t)).mean()) > 0.05
    assert 0.3 < float((CC.planes("invalid")[0] < 0).mean()) < 0.9
    assert float((CC.planes("cost")[1] >= 2.0**24).mean()) >= 0.5
    # both cameras and both poses are used, the skewed camera is what it is said to be
    assert {tuple(c["rig"].items()) for c in cases.values()} == {tuple(CC.RIG_CENTRED.items()), tuple(CC.RIG_SKEWED.items())}
    assert {c["pose"] for c in cases.values()} == {CC.POSE_ZERO, CC.POSE_GENERAL} and all(v != 0 for v in CC.POSE_GENERAL)
    assert CC.RIG_SKEWED["fx"] != CC.RIG_SKEWED["fy"]
    for c in cases.values():
        h, w = c["left"].shape
        if c["rig"] is CC.RIG_SKEWED:
            assert abs(c["rig"]["cx"] - w / 2) > 1 and abs(c["rig"]["cy"] - h / 2) > 1


def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_cloud_style": hip_lib.CloudStyle, "svo_cloud_segment": hip_lib.CloudSegment,
                 "svo_cloud_dst": hip_lib.CloudDst, "svo_cloud_src": hip_lib.CloudSrc}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in cls._fields_]
    lines.append('  printf("enums %d %d %d %d %d %d %d\\n", SVO_CLOUD_WORLD, SVO_CLOUD_CAMERA, SVO_CLOUD_COMPACT, '
                 'SVO_CLOUD_ORGANIZED, SVO_CLOUD_OK, SVO_CLOUD_NONE, SVO_CLOUD_DROPPED);\n')
    lines.append('  printf("ignore %d\\n", (int)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY));\n')
    lines.append('  printf("point %zu\\n", sizeof(svo_map_point));\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_cloud_style": 48, "svo_cloud_segment": 64, "svo_cloud_dst": 24, "svo_cloud_src": 96}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f in cls._fields_:
            assert c[f"{name}.{f[0]}"] == [getattr(cls, f[0]).offset], (name, f[0])
    seg = hip_lib.CLOUD_SEGMENT_DTYPE
    assert seg.itemsize == 64 and list(seg.names) == [f[0] for f in hip_lib.CloudSegment._fields_]
    for f in seg.names:
        assert seg.fields[f][1] == getattr(hip_lib.CloudSegment, f).offset, f
    assert c["enums"] == [hip_lib.CLOUD_WORLD, hip_lib.CLOUD_CAMERA, hip_lib.CLOUD_COMPACT, hip_lib.CLOUD_ORGANIZED, hip_lib.CLOUD_OK,
                          hip_lib.CLOUD_NONE, hip_lib.CLOUD_DROPPED] == [0, 1, 0, 1, 0, 1, 0x80]
    assert c["ignore"][0] & hip_lib.CLOUD_DROPPED == 0                      # the dropped bit is no SVO_IGNORE_* bit
    assert c["point"] == [16] == [hip_lib.MAP_POINT_DTYPE.itemsize] == [CR.POINT.itemsize] and CR.POINT == hip_lib.MAP_POINT_DTYPE
    assert (CR.WORLD, CR.CAMERA, CR.COMPACT, CR.ORGANIZED, CR.DROPPED) == (0, 1, 0, 1, hip_lib.CLOUD_DROPPED)
    lib = hip_lib.lib()
    for sym in ("svo_cloud_size", "svo_submit_export_cloud", "svo_export_cloud", "svo_cloud_points"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def _style(step=1, win=0, sx=0, sy=0, frame=0, layout=0, min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0, reserved=(0, 0, 0)):
    st = hip_lib.CloudStyle(step, win, sx, sy, frame, layout, min_disparity, max_depth, max_mean_cost)
    st._reserved[0], st._reserved[1], st._reserved[2] = reserved
    return st


def test_cloud_size():
    for step in (1, 3, 16):
        for w, h in ((320, 240), (752, 480), (97, 53)):
            cols, rows, points = hip_lib.cloud_size(CAM, w, h, _style(step=step))
            assert (cols, rows) == (w // step, h // step) == DR.lattice(w, h, step)[:2] and points == cols * rows
            # the lattice is the disparity job's
            assert (cols, rows) == hip_lib.disparity_size(CAM, w, h, hip_lib.disparity_style(step=step))[:2]
    assert hip_lib.cloud_size(CAM, 320, 240, _style()) == (320, 240, 76800)                  # style zeros: the ctx's settings
    assert hip_lib.cloud_size(CAM, 320, 240, _style(16, 35, 64, 8, 1, 1, 3.0, 50.0, 1e4)) == (20, 15, 300)
    assert hip_lib.cloud_size(CAM, 320, 240, hip_lib.cloud_style(4, frame="camera", layout="organized", max_depth=9.0)) == (80, 60, 4800)
    lib = hip_lib.lib()
    points = C.c_int64(0)
    assert lib.svo_cloud_size(C.byref(CAM), 320, 240, C.byref(_style(step=3)), None, None, C.byref(points)) == 0
    assert points.value == 106 * 80
    assert lib.svo_cloud_size(C.byref(CAM), 320, 240, C.byref(_style()), None, None, None) == 0


def test_cloud_size_rejects():
    bad = [_style(step=0), _style(step=17), _style(step=-1), _style(win=36), _style(win=-1), _style(sx=65), _style(sx=-1),
           _style(sy=9), _style(sy=-1), _style(frame=2), _style(frame=-1), _style(layout=2), _style(layout=-1),
           _style(min_disparity=-1.0), _style(max_depth=-0.5), _style(max_mean_cost=-1e-3),
           _style(min_disparity=float("nan")), _style(max_depth=float("inf")), _style(max_mean_cost=float("nan")),
           _style(max_mean_cost=float("-inf")),
           _style(reserved=(1, 0, 0)), _style(reserved=(0, 1, 0)), _style(reserved=(0, 0, 1))]
    for st in bad:
        with pytest.raises(hip_lib.SvoError):
            hip_lib.cloud_size(CAM, 320, 240, st)
    with pytest.raises(hip_lib.SvoError):
        hip_lib.cloud_size(CAM, 15, 240, _style(step=16))         # cols of 0
    with pytest.raises(hip_lib.SvoError):
        hip_lib.cloud_size(CAM, 320, 15, _style(step=16))         # rows of 0
    with pytest.raises(hip_lib.SvoError):
        hip_lib.cloud_size(CAM, 0, 240, _style())                 # settings svo_ctx_create rejects
    lib = hip_lib.lib()
    assert lib.svo_cloud_size(C.byref(CAM), 320, 240, None, None, None, None) == -1
    assert lib.svo_cloud_size(None, 320, 240, C.byref(_style()), None, None, None) == -1
    # the calls that need a ctx or a handle reject a missing one before anything else
    dst = hip_lib.CloudDst(None, None, 0)
    assert lib.svo_submit_export_cloud(None, 0, None, 0, C.byref(_style()), C.byref(dst), 0) == -1
    assert lib.svo_export_cloud(None, 0, None, 0, C.byref(_style()), C.byref(dst), 0) == -1
    assert lib.svo_cloud_points(None, 0, None, None, C.byref(_style(win=7, sx=9, sy=2)), None, None) == -1
    assert hip_lib.lib().svo_last_error()
