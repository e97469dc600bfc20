"""The AR picture without a GPU: the struct layouts of the C header against the Python types, svo_ar_size and what it
rejects, svo_ar_camera_of_pose bit for bit against the restatement (tests/ar_ref.py) and against the oracle's
project_keypoints, and the restatement against the properties the header claims: no drawing order, no holes along a
shared edge, depth > 0, nothing for A == 0, both windings alike."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ar_ref as AR
import oracle_py as O
from stereo_svo_slam_amd import hip_lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CFG = synth.CONFIGS["tiny"]
CAM = hip_lib.CameraSettings.from_dict(CFG)


def _style(**kw):
    reserved = kw.pop("reserved", (0, 0))
    st = hip_lib.ar_style(**kw)
    st._reserved[0], st._reserved[1] = reserved
    return st


def test_struct_layouts(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_ar_camera": hip_lib.ArCamera, "svo_ar_mesh": hip_lib.ArMesh, "svo_ar_instance": hip_lib.ArInstance,
                 "svo_ar_style": hip_lib.ArStyle, "svo_ar_dst": hip_lib.ArDst, "svo_ar_draw": hip_lib.ArDraw,
                 "svo_ar_src": hip_lib.ArSrc}
    names = {name: [f[0] for f in cls._fields_] for name, cls in ctypes_of.items()}
    names["svo_ar_segment"] = list(hip_lib.AR_SEGMENT_DTYPE.names)
    lines = []
    for name, fields in names.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in fields]
    lines.append('  printf("enums %d %d %d\\n", SVO_AR_OK, SVO_AR_NONE, SVO_AR_MAX_TRIANGLES);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_ar_camera": 64, "svo_ar_mesh": 40, "svo_ar_instance": 64, "svo_ar_style": 32, "svo_ar_dst": 24, "svo_ar_draw": 88,
            "svo_ar_src": 40}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f in names[name]:
            assert c[f"{name}.{f}"] == [getattr(cls, f).offset], (name, f)
    assert c["svo_ar_segment"] == [hip_lib.AR_SEGMENT_DTYPE.itemsize] == [64]
    for f in names["svo_ar_segment"]:
        assert c[f"svo_ar_segment.{f}"] == [hip_lib.AR_SEGMENT_DTYPE.fields[f][1]], f
    assert c["enums"] == [hip_lib.AR_OK, hip_lib.AR_NONE, hip_lib.AR_MAX_TRIANGLES] == [0, 1, 65536]
    assert (AR.RGB8, AR.RGBA8) == (hip_lib.PIXEL_RGB8, hip_lib.PIXEL_RGBA8)
    lib = hip_lib.lib()
    for sym in ("svo_ar_size", "svo_ar_camera_of_pose", "svo_submit_export_ar", "svo_export_ar", "svo_render_ar"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def test_ar_size_against_the_restatement():
    for pixel in (AR.RGB8, AR.RGBA8):
        for w, h in ((320, 240), (752, 480), (64, 64), (200, 120)):
            got = hip_lib.ar_size(CAM, w, h, _style(pixel=pixel))
            assert got == AR.size(w, h, pixel), (pixel, w, h)
            assert got[1] % 256 == 0 and 0 <= got[1] - h * got[0] < 256
    lib = hip_lib.lib()
    st, nbytes = _style(), C.c_int64(0)
    assert lib.svo_ar_size(C.byref(CAM), 320, 240, C.byref(st), None, C.byref(nbytes)) == 0 and nbytes.value == 230400
    assert lib.svo_ar_size(C.byref(CAM), 320, 240, C.byref(st), None, None) == 0


def test_ar_size_rejects():
    hip_lib.ar_size(CAM, 320, 240, _style(pixel="rgba8", light=(0.0, 0.0, 0.0), ambient=0.0, near=1e-30))   # the limits are fine
    hip_lib.ar_size(CAM, 320, 240, _style(light=(-3e38, 3e38, 1.0), ambient=1.0, near=3e38))
    inf, nan = float("inf"), float("nan")
    bad = [_style(pixel=0), _style(pixel=3), _style(pixel=-1), _style(light=(inf, 0, 1)), _style(light=(0, nan, 1)),
           _style(light=(0, 0, -inf)), _style(ambient=-0.01), _style(ambient=1.01), _style(ambient=nan), _style(ambient=inf),
           _style(near=0.0), _style(near=-1.0), _style(near=nan), _style(near=inf), _style(reserved=(1, 0)), _style(reserved=(0, 1))]
    for st in bad:
        with pytest.raises(hip_lib.SvoError):
            hip_lib.ar_size(CAM, 320, 240, st)
    with pytest.raises(hip_lib.SvoError):
        hip_lib.ar_size(CAM, 0, 240, _style())              # settings svo_ctx_create rejects
    lib = hip_lib.lib()
    assert lib.svo_ar_size(C.byref(CAM), 320, 240, None, None, None) == -1
    assert lib.svo_ar_size(None, 320, 240, C.byref(_style()), None, None) == -1


def _poses():
    pi = np.pi
    poses = [np.zeros(6)]
    for axis in range(3):
        for angle in (0.5, -0.5, pi / 2, 1.0, 3.0, pi - 1e-3, -(pi - 1e-5), 1e-3, 1e-7, 1e-17, 1e-30):
            p = np.zeros(6)
            p[3 + axis] = angle
            p[:3] = (0.25 * axis, -1.5, 2.0 + axis)
            poses.append(p)
    rng = np.random.default_rng(5)
    for scale in (1e-9, 1e-4, 0.3, 1.0, 1.8):
        for _ in range(4):
            poses.append(np.concatenate([rng.normal(0, 3, 3), rng.uniform(-1, 1, 3) * scale]))
    return [p.astype(F) for p in poses]


def test_camera_of_pose_is_bit_equal_to_the_restatement():
    for pose in _poses():
        got = np.frombuffer(bytes(hip_lib.ar_camera_of_pose(pose, CAM)), F)
        want = AR.camera_of_pose(pose, CFG["fx"], CFG["fy"], CFG["cx"], CFG["cy"])
        assert got.tobytes() == want.tobytes(), pose
    cam = hip_lib.ar_camera_of_pose([1, 2, 3, 0, 0, 0], CAM)
    assert list(cam.view) == [1, 0, 0, -1, 0, 1, 0, -2, 0, 0, 1, -3] and (cam.fx, cam.fy, cam.cx, cam.cy) == (200, 200, 160, 120)
    lib = hip_lib.lib()
    assert lib.svo_ar_camera_of_pose(None, C.byref(CAM), C.byref(cam)) == -1
    assert lib.svo_ar_camera_of_pose((C.c_float * 6)(), None, C.byref(cam)) == -1


# The float32 view matrix against the oracle's project_keypoints (which subtracts the translation and rotates by -r
# with its own rounding), on the distortion-free settings of "tiny", over the poses above and points 1 .. 8 m in front
# of each camera inside a 90-degree cone. Measured on the CPU: the largest pixel difference is CAMERA_MEASURED; the
# bound is four times that.
CAMERA_MEASURED = 1.6021729e-04
CAMERA_BOUND = 4 * CAMERA_MEASURED


def test_camera_of_pose_agrees_with_the_oracle_projection():
    cam_o = O.make_camera(**{k: CFG[k] for k in synth.CAMERA_FIELDS})
    rng = np.random.default_rng(11)
    worst = 0.0
    for pose in _poses():
        R = O.rodrigues(pose[3:6])                                    # camera -> world
        z = rng.uniform(1.0, 8.0, 64)
        pc = np.stack([rng.uniform(-1, 1, 64) * z * 0.7, rng.uniform(-1, 1, 64) * z * 0.5, z], 1)
        world = (pc @ R.T + pose[:3].astype(np.float64)).astype(F)
        want = O.project_keypoints(pose, world, cam_o)
        cam = np.frombuffer(bytes(hip_lib.ar_camera_of_pose(pose, CAM)), F)
        for p, uv in zip(world, want):
            c = AR.transform(cam[:12], p)
            u, v = (cam[12] * c[0]) / c[2] + cam[14], (cam[13] * c[1]) / c[2] + cam[15]
            worst = max(worst, abs(float(u) - float(uv[0])), abs(float(v) - float(uv[1])))
    print(f"largest pixel difference {worst:.7e} (measured {CAMERA_MEASURED:.7e}, bound {CAMERA_BOUND:.7e})")
    assert worst <= CAMERA_BOUND


# ---- the restatement against its own properties
H, W = 20, 70


def _rec(pts, c2=(1.0, 1.0, 1.0), colour=0x102030):
    """a screen record of sub-pixel points [(X, Y)] * 3"""
    p = np.asarray(pts, np.int64)
    return p[:, 0].copy(), p[:, 1].copy(), np.asarray(c2, F), colour


def _quad(rng):
    """a convex quad in sub-pixel units: four points of an ellipse at ascending angles, in and around the image"""
    a = np.sort(rng.uniform(0, 2 * np.pi, 4))
    cx, cy = rng.uniform(-5, W + 5), rng.uniform(-5, H + 5)
    rx, ry = rng.uniform(0.3, 40), rng.uniform(0.3, 15)
    return np.stack([np.floor((cx + rx * np.cos(a)) * 16), np.floor((cy + ry * np.sin(a)) * 16)], 1).astype(np.int64)


def _plane(recs):
    keys = np.full((H, W), AR.EMPTY, np.uint64)
    for r in recs:
        AR.offer(keys, r)
    return keys


def test_shuffled_order_gives_the_same_bytes():
    rng = np.random.default_rng(1)
    recs = []
    for i in range(60):
        q = _quad(rng)
        recs.append(_rec(q[:3], rng.uniform(0.5, 3, 3), int(rng.integers(0, 1 << 24))))
    recs += [_rec(np.stack(recs[0][:2], 1), recs[0][2], 0x000001)]     # equal depth, another colour
    want = _plane(recs)
    assert (want != AR.EMPTY).sum() > 100
    for seed in range(5):
        order = np.random.default_rng(seed).permutation(len(recs))
        assert np.array_equal(_plane([recs[i] for i in order]), want)


def test_a_split_quad_has_no_hole_along_either_diagonal():
    rng = np.random.default_rng(2)
    py, px = np.mgrid[0:H, 0:W]
    Px, Py = 16 * px + 8, 16 * py + 8
    holes = interior = 0
    for _ in range(2000):
        q = _quad(rng)
        # strictly inside the convex quad: the four edge functions agree in sign
        e = [(q[(k + 1) % 4, 0] - q[k, 0]) * (Py - q[k, 1]) - (q[(k + 1) % 4, 1] - q[k, 1]) * (Px - q[k, 0]) for k in range(4)]
        inside = np.all([x > 0 for x in e], 0) | np.all([x < 0 for x in e], 0)
        planes = [_plane([_rec(q[[0, 1, 2]]), _rec(q[[0, 2, 3]])]), _plane([_rec(q[[0, 1, 3]]), _rec(q[[1, 2, 3]])])]
        for p in planes:
            holes += int((inside & (p == AR.EMPTY)).sum())
        interior += int(inside.sum())
    assert interior > 100000 and holes == 0


def test_depth_stays_positive():
    rng = np.random.default_rng(3)
    lowest, covered = np.inf, 0
    for _ in range(3000):
        q = _quad(rng)
        z = rng.uniform(0.1, 20, 4) if rng.random() < 0.8 else F(10.0) ** rng.uniform(-30, 30, 4)
        keys = np.full((H, W), AR.EMPTY, np.uint64)
        depth = np.full((H, W), np.inf, F)
        covered += AR.offer(keys, _rec(q[[0, 1, 2]], z[[0, 1, 2]]), depth) + AR.offer(keys, _rec(q[[0, 2, 3]], z[[0, 2, 3]]), depth)
        hit = keys != AR.EMPTY
        if hit.any():
            lowest = min(lowest, float(depth[hit].min()))
            assert ((keys[hit] >> np.uint64(63)) == 0).all()                     # the sign bit: the bits order as the values
    print(f"{covered} covered pixels, lowest depth {lowest:.3e}")
    assert covered > 100000 and lowest > 0


def test_zero_area_draws_nothing():
    for pts in ([(16, 16), (160, 160), (320, 320)], [(40, 40), (40, 40), (200, 90)], [(8, 8), (8, 8), (8, 8)],
                [(8, 8), (808, 8), (408, 8)], [(24, 8), (24, 300), (24, 100)]):
        assert (_plane([_rec(pts)]) == AR.EMPTY).all(), pts


def test_both_windings_draw_the_same_pixels():
    rng = np.random.default_rng(4)
    for _ in range(300):
        q = _quad(rng)
        z = rng.uniform(0.5, 3, 3)
        a, b = _plane([_rec(q[[0, 1, 2]], z)]), _plane([_rec(q[[0, 2, 1]], z[[0, 2, 1]])])
        assert np.array_equal(a != AR.EMPTY, b != AR.EMPTY)
        assert np.array_equal(a & np.uint64(0xFFFFFF), b & np.uint64(0xFFFFFF))


def test_the_inclusive_rule_on_centres_and_edges():
    # a vertex exactly on a pixel centre and an edge through centres are covered
    keys = _plane([_rec([(8, 8), (8 + 16 * 4, 8), (8, 8 + 16 * 4)])])
    hit = keys != AR.EMPTY
    assert hit[0, 0] and hit[0, 4] and hit[4, 0] and hit[2, 2] and not hit[3, 3] and not hit[0, 5]
    assert hit.sum() == 15
    # a sliver thinner than a pixel covers only the centres it contains
    keys = _plane([_rec([(0, 7), (16 * 10, 7), (16 * 10, 9)])])
    hit = keys != AR.EMPTY
    assert hit[0].sum() >= 1 and not hit[1:].any() and hit[0, 9] and not hit[0, 0]
    keys = _plane([_rec([(0, 1), (16 * 10, 1), (16 * 10, 3)])])
    assert (keys == AR.EMPTY).all()


def test_shading():
    w = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], F)                          # normal (0, 0, 1)
    assert AR.shade_colour(w, 0x804020, (0, 0, 1), 0.0) == 0x804020
    assert AR.shade_colour(w, 0x804020, (0, 0, -1), 0.0) == 0x804020            # both faces are lit alike
    assert AR.shade_colour(w, 0x804020, (1, 0, 0), 0.0) == 0                    # a light parallel to the face
    assert AR.shade_colour(w, 0x804020, (1, 0, 0), 1.0) == 0x804020
    assert AR.shade_colour(w, 0x804020, (1, 0, 0), 0.5) == 0x402010
    assert AR.shade_colour(w, 0xffffff, (0, 0, 5), 0.25) == 0xffffff            # s is capped at 1
    assert AR.shade_colour(np.zeros((3, 3), F), 0x804020, (0, 0, 1), 0.25) == 0x201008   # q == 0: s = 0
