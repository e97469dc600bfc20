"""The scene without a GPU: svo_scene_size and its rejected styles against the restatement (tests/scene_ref.py), the
struct layouts of the C header against the Python types, svo_scene_frustum bit for bit and svo_scene_look_at within
a float32 ulp of a float64 statement, the restatement's depth-buffer loop against the "smallest key wins" formulation
that the kernel computes, and the line rule."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_ref as MR
import scene_ref as SR
from stereo_svo_slam_amd import hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _style(**kw):
    reserved = kw.pop("reserved", 0)
    st = hip_lib.scene_style(**kw)
    st._reserved = reserved
    return st


def test_scene_size_against_the_restatement():
    for pixel in (SR.RGB8, SR.RGBA8):
        for cols, rows in ((1, 1), (3, 2), (5, 17), (64, 16), (65, 17), (256, 256), (752, 480), (4096, 4096), (4096, 1), (1, 4096)):
            got = hip_lib.scene_size(_style(cols=cols, rows=rows, pixel=pixel))
            assert got == SR.size(cols, rows, pixel), (pixel, cols, rows)
            assert got[1] % 256 == 0 and 0 <= got[1] - rows * got[0] < 256
    lib = hip_lib.lib()
    st, nbytes = _style(cols=7, rows=3), C.c_int64(0)
    assert lib.svo_scene_size(C.byref(st), None, C.byref(nbytes)) == 0 and nbytes.value == 256
    assert lib.svo_scene_size(C.byref(st), None, None) == 0


def test_scene_size_rejects():
    hip_lib.scene_size(_style(cols=4096, rows=4096, pixel=SR.RGBA8, point_size=16, show=15, from_keyframe=2**31 - 1,
                              trajectory_tail=2**31 - 1, background=0, trajectory_rgb=0xffffff,
                              filter=dict(drop_flags=7, own_only=1, min_inliers=-5), frustum=(0.0, -1.0, 1e30)))   # the limits are fine
    hip_lib.scene_size(_style(cols=1, rows=1, point_size=1, show=0))
    inf, nan = float("inf"), float("nan")
    bad = [_style(cols=0), _style(cols=4097), _style(cols=-1), _style(rows=0), _style(rows=4097), _style(pixel=0), _style(pixel=3),
           _style(pixel=-1), _style(point_size=0), _style(point_size=17), _style(point_size=-1), _style(background=0x1000000),
           _style(trajectory_rgb=0x80000000), _style(keyframe_rgb=0x1000000), _style(pose_rgb=0xff000000),
           _style(frustum=(inf, 0.08, 0.07)), _style(frustum=(0.1, nan, 0.07)), _style(frustum=(0.1, 0.08, -inf)),
           _style(show=16), _style(show=0x80000000), _style(from_keyframe=-1), _style(trajectory_tail=-1),
           _style(filter=dict(drop_flags=8)), _style(filter=dict(drop_flags=0x80000000)), _style(filter=dict(_reserved=1)),
           _style(reserved=1)]
    for st in bad:
        with pytest.raises(hip_lib.SvoError):
            hip_lib.scene_size(st)
    assert hip_lib.lib().svo_scene_size(None, None, None) == -1


def test_struct_layouts(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    names = {"svo_scene_camera": [f[0] for f in hip_lib.SceneCamera._fields_],
             "svo_scene_style": [f[0] for f in hip_lib.SceneStyle._fields_],
             "svo_scene_line": list(hip_lib.SCENE_LINE_DTYPE.names),
             "svo_scene_segment": list(hip_lib.SCENE_SEGMENT_DTYPE.names),
             "svo_scene_dst": [f[0] for f in hip_lib.SceneDst._fields_],
             "svo_scene_src": [f[0] for f in hip_lib.SceneSrc._fields_]}
    lines = []
    for name, fields in names.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in fields]
    lines.append('  printf("enums %d %d %d %d %d %d %d %d %d %d\\n", SVO_SCENE_POINTS, SVO_SCENE_TRAJECTORY, SVO_SCENE_KEYFRAMES,'
                 ' SVO_SCENE_POSE, SVO_SCENE_CLASS_POSE, SVO_SCENE_CLASS_KEYFRAME, SVO_SCENE_CLASS_TRAJECTORY,'
                 ' SVO_SCENE_CLASS_POINT, SVO_SCENE_OK, SVO_SCENE_NONE);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    assert c["svo_scene_camera"] == [C.sizeof(hip_lib.SceneCamera)] == [64]
    assert c["svo_scene_style"] == [C.sizeof(hip_lib.SceneStyle)]
    assert c["svo_scene_line"] == [hip_lib.SCENE_LINE_DTYPE.itemsize] == [32]
    assert c["svo_scene_segment"] == [hip_lib.SCENE_SEGMENT_DTYPE.itemsize] == [64]
    assert c["svo_scene_dst"] == [C.sizeof(hip_lib.SceneDst)]
    assert c["svo_scene_src"] == [C.sizeof(hip_lib.SceneSrc)]
    for cls, name in ((hip_lib.SceneCamera, "svo_scene_camera"), (hip_lib.SceneStyle, "svo_scene_style"),
                      (hip_lib.SceneDst, "svo_scene_dst"), (hip_lib.SceneSrc, "svo_scene_src")):
        for f in names[name]:
            assert c[f"{name}.{f}"] == [getattr(cls, f).offset], (name, f)
    for name, dt in (("svo_scene_line", hip_lib.SCENE_LINE_DTYPE), ("svo_scene_segment", hip_lib.SCENE_SEGMENT_DTYPE)):
        for f in names[name]:
            assert c[f"{name}.{f}"] == [dt.fields[f][1]], (name, f)
    assert c["enums"] == [hip_lib.SCENE_POINTS, hip_lib.SCENE_TRAJECTORY, hip_lib.SCENE_KEYFRAMES, hip_lib.SCENE_POSE,
                          hip_lib.SCENE_CLASS_POSE, hip_lib.SCENE_CLASS_KEYFRAME, hip_lib.SCENE_CLASS_TRAJECTORY,
                          hip_lib.SCENE_CLASS_POINT, hip_lib.SCENE_OK, hip_lib.SCENE_NONE] == [1, 2, 4, 8, 0, 1, 2, 3, 0, 1]
    assert (SR.POINTS, SR.TRAJECTORY, SR.KEYFRAMES, SR.POSE, SR.RGB8, SR.RGBA8) == (1, 2, 4, 8, hip_lib.PIXEL_RGB8, hip_lib.PIXEL_RGBA8)
    lib = hip_lib.lib()
    for sym in ("svo_scene_size", "svo_scene_look_at", "svo_scene_frustum", "svo_submit_export_scenes", "svo_export_scenes",
                "svo_render_scene"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def _crafted_poses():
    pi = np.pi
    poses = [np.zeros(6)]
    for axis in range(3):
        for angle in (0.5, -0.5, pi / 2, -pi / 2, 1.0, 3.0, pi - 1e-3, pi - 1e-7, float(F(pi)), -(pi - 1e-5), pi + 1e-3, 2 * pi - 1e-3,
                      1e-3, 1e-7, 1e-12, 1e-17, -1e-20, 1e-30):
            p = np.zeros(6)
            p[3 + axis] = angle
            p[:3] = (0.25 * axis, -1.5, 2.0 + axis)
            poses.append(p)
    rng = np.random.default_rng(5)
    for scale in (1e-9, 1e-4, 0.3, 1.0, 1.8):                # general axes; 1.8 * sqrt(3) is near pi
        for _ in range(4):
            poses.append(np.concatenate([rng.normal(0, 3, 3), rng.uniform(-1, 1, 3) * scale]))
    poses.append(np.array([1.0, 2.0, 3.0, pi / np.sqrt(3), pi / np.sqrt(3), pi / np.sqrt(3)]))
    return [p.astype(F) for p in poses]


def test_frustum_is_bit_equal_to_the_restatement():
    for pose in _crafted_poses():
        for dims in (SR.VIEWER_DIMS, (0.3, 0.7, 1.9), (0.0, 0.0, 0.0), (-0.1, 0.08, -0.07)):
            got, want = hip_lib.scene_frustum(pose, dims), SR.frustum(pose, dims)
            assert got.tobytes() == want.tobytes(), (pose, dims)
    f = hip_lib.scene_frustum([1, 2, 3, 0, 0, 0])
    w, h, d = (F(v) for v in SR.VIEWER_DIMS)
    apex = [F(1), F(2), F(3)]
    assert f[0].tolist() == apex + [F(1) - w, F(2) + h, F(3) + d]                  # 0 -> 1
    assert f[7].tolist() == [F(1) + w, F(2) + h, F(3) + d, F(1) - w, F(2) + h, F(3) + d]   # 4 -> 1
    assert all(f[e, :3].tolist() == apex for e in range(4))
    lib = hip_lib.lib()
    assert lib.svo_scene_frustum(None, None, None) == -1


def test_look_at_against_float64():
    rng = np.random.default_rng(9)
    cases = [SR.PRESETS[k] + (45.0, 256, 256, 0.1) for k in ("front", "top", "side")]
    cases += [((1, 2, 3), (-2, 0.5, 7), (0.1, -1, 0.2), 60.0, 752, 480, 0.05), ((0, 0, 0), (0, 1e-3, 1), (0, 1, 0), 1.0, 1, 1, 1e-6),
              ((5, 5, 5), (5, 5, 6), (1, 0, 0), 179.0, 4096, 3, 10.0)]
    for _ in range(20):
        cases.append((tuple(rng.normal(0, 5, 3)), tuple(rng.normal(0, 5, 3)), tuple(rng.normal(0, 1, 3)), float(rng.uniform(5, 170)),
                      int(rng.integers(1, 4097)), int(rng.integers(1, 4097)), float(rng.uniform(1e-3, 2))))
    for eye, centre, up, fov, cols, rows, near in cases:
        eye, centre, up = (np.asarray(v, F) for v in (eye, centre, up))          # (the C entry takes floats)
        cam = hip_lib.scene_look_at(eye, centre, up, fov, cols, rows, near)
        view, f, cx, cy, _ = SR.look_at(eye, centre, up, F(fov), cols, rows, near)
        got = np.array(list(cam.view), F).reshape(3, 4)
        # both sides round double results that may differ in the last double bit: one float32 ulp of the row's largest
        # magnitude is the whole margin
        for k in range(3):
            ulp = np.spacing(F(np.abs(view[k]).max()))
            assert np.all(np.abs(got[k].astype(np.float64) - view[k]) <= ulp), (eye, centre, up, k)
        assert abs(np.float64(cam.f) - f) <= np.spacing(F(f)) and cam.cx == F(cols / 2) and cam.cy == F(rows / 2) and cam.near == F(near)
        R = got[:, :3].astype(np.float64)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)                          # rows orthonormal
        assert np.linalg.det(R) > 0.99                                             # right-handed: x right, y down, z forward
        scale = max(1.0, float(np.abs(eye).max()))
        assert np.allclose(R @ eye.astype(np.float64) + got[:, 3], 0, atol=4e-6 * scale)   # the eye maps to the origin
        z = (centre - eye).astype(np.float64)
        assert np.allclose(R @ z, [0, 0, np.sqrt(z @ z)], atol=4e-6 * max(1.0, np.sqrt(z @ z)))   # the centre lies straight ahead


def test_presets():
    front = hip_lib.scene_preset("front", 640, 480)
    assert list(front.view) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1]               # the identity rotation exactly
    assert (front.cx, front.cy, front.near) == (320.0, 240.0, F(0.1)) and front.f == F(240 / np.tan(np.deg2rad(22.5)))
    assert list(hip_lib.scene_preset("top").view) == [1, 0, 0, 0, 0, 0, -1, 0, 0, 1, 0, 5]
    assert list(hip_lib.scene_preset("side").view) == [0, 0, -1, 0, 0, 1, 0, 0, 1, 0, 0, 5]
    assert hip_lib.SCENE_PRESETS == {k: tuple(tuple(float(x) for x in v) for v in p) for k, p in SR.PRESETS.items()}
    st = hip_lib.scene_style()                                                     # the viewer's colours and frustum
    assert (st.background, st.trajectory_rgb, st.keyframe_rgb, st.pose_rgb) == (0xffffff, 0xff0000, 0x0000ff, 0x00ff00)
    assert (st.frustum_w, st.frustum_h, st.frustum_d) == tuple(F(v) for v in SR.VIEWER_DIMS) and st.show == 15


def test_look_at_rejects():
    ok = dict(eye=(0, 0, -1), centre=(0, 0, 0), up=(0, -1, 0), fov_y_deg=45.0, cols=8, rows=8, near=0.1)
    hip_lib.scene_look_at(**ok)
    nan, inf = float("nan"), float("inf")
    for change in (dict(centre=(0, 0, -1)), dict(up=(0, 0, 1)), dict(up=(0, 0, -2)), dict(up=(0, 0, 0)), dict(eye=(nan, 0, 0)),
                   dict(centre=(0, inf, 0)), dict(up=(0, nan, 0)), dict(fov_y_deg=0.0), dict(fov_y_deg=180.0), dict(fov_y_deg=-3.0),
                   dict(fov_y_deg=nan), dict(cols=0), dict(rows=0), dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf)):
        with pytest.raises(hip_lib.SvoError):
            hip_lib.scene_look_at(**dict(ok, **change))


def _random_scene(rng, n_points, n_lines):
    """points on few depths and few centres (ties, coincidence), lines that cross them; some elements not drawable"""
    depths = np.array([1.0, 1.5, 2.0, 2.0, 3.0], F)
    k3 = np.zeros((n_points, 3), F)
    z = depths[rng.integers(0, len(depths), n_points)]
    k3[:, 0] = rng.integers(-3, 4, n_points).astype(F) * F(0.25) * z
    k3[:, 1] = rng.integers(-3, 4, n_points).astype(F) * F(0.25) * z
    k3[:, 2] = z
    k3[::13] = F([np.nan, 0, 1])
    k3[5::17, 2] = F(-1.0)
    planes = {"flags": rng.integers(0, 8, n_points).astype(np.uint32), "keyframe_id": rng.integers(0, 3, n_points).astype(np.uint32),
              "inlier_count": rng.integers(0, 12, n_points).astype(np.uint32), "color": rng.integers(0, 2**24, n_points).astype(np.uint32)}
    sets = [(n_points // 2, 1, k3[:n_points // 2], {k: v[:n_points // 2] for k, v in planes.items()}),
            (n_points - n_points // 2, 2, k3[n_points // 2:], {k: v[n_points // 2:] for k, v in planes.items()})]
    lines = []
    for _ in range(n_lines):
        a = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), depths[rng.integers(0, 5)] if rng.random() < 0.7 else rng.uniform(-1, 3)], F)
        b = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), depths[rng.integers(0, 5)] if rng.random() < 0.7 else rng.uniform(-1, 3)], F)
        lines.append((a, b, int(rng.integers(0, 3)) << 24 | int(rng.integers(0, 2**24))))
    return sets, lines


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_depth_buffer_loop_equals_smallest_key(seed):
    rng = np.random.default_rng(seed)
    cols, rows = 41, 29
    cam = SR.camera(np.eye(3, 4), 20.0, cols / 2, rows / 2, 0.5)
    sets, lines = _random_scene(rng, 120, 30)
    for pixel, size, filt in ((SR.RGB8, 1, MR.KEEP_ALL), (SR.RGBA8, 4, dict(drop_flags=2, own_only=1, min_inliers=3)), (SR.RGB8, 7, MR.KEEP_ALL)):
        a = SR.render(cols, rows, pixel, cam, sets, lines, filt, size, 0x102030)
        b = SR.render_smallest_key(cols, rows, pixel, cam, sets, lines, filt, size, 0x102030, rng=rng)
        assert a.tobytes() == b.tobytes(), (pixel, size)
        bg = np.all(a[:, :, :3] == np.array([0x10, 0x20, 0x30], np.uint8), axis=2)
        assert bg.any() and not bg.all()
        if pixel == SR.RGBA8:
            assert (a[:, :, 3] == 255).all()


def test_hand_written_picture():
    """one point of size 3, one line behind it and one in front of it, pixel by pixel"""
    cam = SR.camera(np.eye(3, 4), 4.0, 4.0, 3.0, 0.5)
    k3 = np.array([[0.5, 0.0, 2.0]], F)                   # u = 4 * 0.5 / 2 + 4 = 5, v = 3: pixels 4 .. 6 x 2 .. 4
    sets = [(1, 0, k3, {"flags": np.zeros(1, np.uint32), "keyframe_id": np.zeros(1, np.uint32), "inlier_count": np.zeros(1, np.uint32),
                        "color": np.array([0x030201], np.uint32)})]                      # r 1, g 2, b 3
    lines = [(F([-1.0, 0.0, 1.0]), F([1.0, 0.0, 1.0]), 2 << 24 | 0x0a0b0c),    # y = 3, x 0 .. 8, nearer than the point
             (F([0.75, -3.0, 4.0]), F([0.75, 3.0, 4.0]), 1 << 24 | 0x0d0e0f)]  # x = 4 + 0.75 = 4, y 0 .. 6, behind the point
    img = SR.render(9, 7, SR.RGB8, cam, sets, lines, MR.KEEP_ALL, 3, 0xffffff)
    for y in range(7):
        for x in range(9):
            want = (10, 11, 12) if y == 3 else (1, 2, 3) if 4 <= x <= 6 and 2 <= y <= 4 else (13, 14, 15) if x == 4 else (255, 255, 255)
            assert tuple(img[y, x]) == want, (x, y)


def test_the_line_rule():
    rng = np.random.default_rng(3)
    ends = [(0, 0, 0, 0), (0, 0, 7, 0), (0, 0, 0, -7), (3, 4, 10, 11), (3, 4, -4, 11), (0, 0, 10, 3), (0, 0, -10, 3), (0, 0, 3, -10),
            (5, 5, 4, 5), (0, 0, 2, 1), (0, 0, 1, 2), (-32767, -32767, 32767, 32767), (32767, -32767, -32767, 32766), (0, 0, 65534, 1)]
    ends += [tuple(int(v) for v in rng.integers(-300, 300, 4)) for _ in range(300)]
    for X0, Y0, X1, Y1 in ends:
        pix = SR.line_pixels(X0, Y0, X1, Y1)
        dx, dy = X1 - X0, Y1 - Y0
        n = max(abs(dx), abs(dy))
        assert len(pix) == n + 1 and pix[0] == (X0, Y0) and pix[-1] == (X1, Y1)
        major = 0 if abs(dx) >= abs(dy) else 1
        step = np.sign(dx if major == 0 else dy)
        for (xa, ya), (xb, yb) in zip(pix, pix[1:]):
            assert max(abs(xb - xa), abs(yb - ya)) == 1                              # 8-connected
            assert (xb - xa, yb - ya)[major] == step                                 # the major axis strictly monotone
    assert SR.line_pixels(0, 0, 4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]   # halves round up ...
    assert SR.line_pixels(0, 0, 4, -2) == [(0, 0), (1, 0), (2, -1), (3, -1), (4, -2)]   # ... toward +infinity, whatever the direction
    assert SR.rdiv(-3, 2) == -1 and SR.rdiv(3, 2) == 2 and SR.rdiv(-1, 2) == 0 and SR.rdiv(1, 2) == 1
