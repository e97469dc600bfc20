"""The views without a GPU: svo_view_size and its rejected arguments against the restatement (tests/view_ref.py), the
struct layouts of the C header against the Python types, and the restatement's painter's loop against the "highest
covering index wins" formulation that the kernel computes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import view_ref as VR
from stereo_svo_slam_amd import hip_lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE_ALL = 7


def _cam(config):
    cfg = synth.CONFIGS[config]
    return cfg, hip_lib.CameraSettings.from_dict(cfg)


def _style(plane=0, level=0, pixel=0, markers=0, drop_flags=0, size=10, size_temporary=10, reserved=0):
    return hip_lib.ViewStyle(plane, level, pixel, markers, drop_flags, size, size_temporary, reserved)


@pytest.mark.parametrize("config", ["tiny", "euroc", "hd"])
def test_view_size_against_the_restatement(config):
    cfg, cam = _cam(config)
    w, h = cfg["width"], cfg["height"]
    for pixel in (VR.GRAY8, VR.RGB8, VR.RGBA8):
        for level in range(cfg["max_pyramid_levels"]):
            got = hip_lib.view_size(cam, w, h, _style(VR.PLANE_LEFT, level, pixel))
            assert got == VR.size(w, h, VR.PLANE_LEFT, level, pixel), (pixel, level)
            assert got[3] % 256 == 0 and 0 <= got[3] - got[1] * got[2] < 256
        got = hip_lib.view_size(cam, w, h, _style(VR.PLANE_RIGHT, 0, pixel))
        assert got == VR.size(w, h, VR.PLANE_RIGHT, 0, pixel) == (w, h, w * VR.BYTES[pixel], (w * h * VR.BYTES[pixel] + 255) // 256 * 256)
    if config == "euroc" and cfg["max_pyramid_levels"] > 5:
        assert VR.size(w, h, 0, 4, VR.RGB8)[0] == 47 and VR.size(w, h, 0, 5, VR.RGB8)[0] == 23


def test_view_size_out_pointers_may_be_null():
    cfg, cam = _cam("tiny")
    st = _style()
    rows = C.c_int(0)
    assert hip_lib.lib().svo_view_size(C.byref(cam), cfg["width"], cfg["height"], C.byref(st), None, C.byref(rows), None, None) == 0
    assert rows.value == cfg["height"]


def test_view_size_rejects():
    cfg, cam = _cam("tiny")
    w, h, levels = cfg["width"], cfg["height"], cfg["max_pyramid_levels"]
    hip_lib.view_size(cam, w, h, _style(0, levels - 1, VR.RGBA8, 1, IGNORE_ALL, 64, 0))          # the limits are fine
    bad = [_style(plane=2), _style(plane=-1), _style(level=levels), _style(level=-1), _style(plane=1, level=1),
           _style(pixel=3), _style(pixel=-1), _style(markers=2), _style(markers=-1),
           _style(markers=1, pixel=VR.GRAY8), _style(plane=1, markers=1, pixel=VR.RGB8),
           _style(drop_flags=8), _style(drop_flags=0x80000000), _style(size=65), _style(size=-1),
           _style(size_temporary=65), _style(size_temporary=-1), _style(reserved=1)]
    for st in bad:
        with pytest.raises(hip_lib.SvoError):
            hip_lib.view_size(cam, w, h, st)
    out = C.c_int(0)
    lib = hip_lib.lib()
    assert lib.svo_view_size(C.byref(cam), w, h, None, C.byref(out), None, None, None) == -1
    assert lib.svo_view_size(None, w, h, C.byref(_style()), C.byref(out), None, None, None) == -1
    assert lib.svo_view_size(C.byref(cam), 8, h, C.byref(_style()), C.byref(out), None, None, None) == -1   # (svo_ctx_create's rule)


def test_struct_layouts(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    names = {"svo_view_style": [f[0] for f in hip_lib.ViewStyle._fields_],
             "svo_view_segment": list(hip_lib.VIEW_SEGMENT_DTYPE.names),
             "svo_view_dst": [f[0] for f in hip_lib.ViewDst._fields_],
             "svo_view_src": ["image", "kps"]}
    lines = []
    for name, fields in names.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in fields]
    lines.append('  printf("enums %d %d %d %d %d %d %d\\n", SVO_PLANE_LEFT, SVO_PLANE_RIGHT, SVO_PIXEL_GRAY8, SVO_PIXEL_RGB8,'
                 ' SVO_PIXEL_RGBA8, SVO_VIEW_OK, SVO_VIEW_NONE);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    assert c["svo_view_style"] == [C.sizeof(hip_lib.ViewStyle)] == [32]
    assert c["svo_view_segment"] == [hip_lib.VIEW_SEGMENT_DTYPE.itemsize] == [64]
    assert c["svo_view_dst"] == [C.sizeof(hip_lib.ViewDst)]
    assert c["svo_view_src"] == [C.sizeof(hip_lib.ViewSrc)]
    for cls, name in ((hip_lib.ViewStyle, "svo_view_style"), (hip_lib.ViewDst, "svo_view_dst"), (hip_lib.ViewSrc, "svo_view_src")):
        for f in names[name]:
            assert c[f"{name}.{f}"] == [getattr(cls, f).offset], (name, f)
    for f in names["svo_view_segment"]:
        assert c[f"svo_view_segment.{f}"] == [hip_lib.VIEW_SEGMENT_DTYPE.fields[f][1]], f
    assert c["enums"] == [hip_lib.PLANE_LEFT, hip_lib.PLANE_RIGHT, hip_lib.PIXEL_GRAY8, hip_lib.PIXEL_RGB8,
                          hip_lib.PIXEL_RGBA8, hip_lib.VIEW_OK, hip_lib.VIEW_NONE] == [0, 1, 0, 1, 2, 0, 1]
    assert (VR.GRAY8, VR.RGB8, VR.RGBA8, VR.IGNORE_TEMPORARY) == (0, 1, 2, hip_lib.IGNORE_TEMPORARY)
    lib = hip_lib.lib()
    for sym in ("svo_view_size", "svo_submit_export_views", "svo_export_views", "svo_render_views"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def test_default_styles_follow_the_app():
    f = hip_lib.view_style(hip_lib.EXPORT_FRAMES, "left", 0, "rgb8", True)
    k = hip_lib.view_style(hip_lib.EXPORT_LAST_KEYFRAMES, "left", 0, "rgba8", True)
    assert (f.drop_flags, f.size, f.size_temporary, f.pixel, f.markers) == (hip_lib.IGNORE_COMPLETELY, 20, 10, 1, 1)
    assert (k.drop_flags, k.size, k.size_temporary, k.pixel, k.markers) == (0, 10, 10, 2, 1)


def test_hand_written_markers():
    """one cross and one square, pixel by pixel"""
    gray = np.full((9, 12), 7, np.uint8)
    k2 = np.float32([[3.9, 4.2], [8.0, 4.0]])
    img = VR.render(gray, VR.RGB8, k2, [0, 0], [0, 1], [[1, 2, 3], [4, 5, 6]], 0, 0, 4, 4)
    cross = {(x, 4) for x in range(1, 6)} | {(3, y) for y in range(2, 7)}
    square = {(x, y) for x in (7, 9) for y in (3, 4, 5)} | {(8, 3), (8, 5)}            # s' = 3, half 1
    for y in range(9):
        for x in range(12):
            want = (1, 2, 3) if (x, y) in cross else (4, 5, 6) if (x, y) in square else (7, 7, 7)
            assert tuple(img[y, x]) == want, (x, y)
    assert VR.centre(-0.5, -0.99, 0) == (0, 0) and VR.centre(-1.0, 5.9, 0) == (-1, 5)
    assert VR.centre(13.0, 7.0, 2) == (3, 1) and VR.centre(-7.0, 7.9, 2) == (-1, 1)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e10, -1e10, 32768.0, -32768.0):
        assert VR.centre(bad, 1.0, 0) is None and VR.centre(1.0, bad, 0) is None
    assert VR.centre(32767.9, -32767.9, 0) == (32767, -32767)
    assert VR.centre(65536.0, 0.0, 1) is None and VR.centre(65535.0, 0.0, 1) == (32767, 0)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_painters_loop_equals_highest_covering_index(seed):
    """seeded random sets with heavy overlap (many markers on few centres, both types, every flag combination, sizes
    up to 64, centres outside): drawing in order equals taking the highest covering index"""
    rng = np.random.default_rng(seed)
    rows, cols = 37, 53
    gray = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    n = 300
    centres = rng.integers(-12, 66, (12, 2)).astype(np.float32)
    k2 = centres[rng.integers(0, 12, n)] * (1 << (seed % 3)) + rng.random((n, 2)).astype(np.float32) * 0.9
    k2[::17] = np.float32([np.nan, 3.0])
    flags = rng.integers(0, 8, n)
    types = rng.integers(0, 2, n)
    colors = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    for pixel in (VR.RGB8, VR.RGBA8):
        for drop, s, st in ((0, 10, 20), (2, 64, 1), (5, 0, 33), (7, 20, 10)):
            a = VR.render(gray, pixel, k2, flags, types, colors, seed % 3, drop, s, st)
            b = VR.render_highest_index(gray, pixel, k2, flags, types, colors, seed % 3, drop, s, st)
            assert a.tobytes() == b.tobytes(), (pixel, drop)
            if drop != 7:
                assert (a[:, :, :3] != gray[:, :, None]).any()
            if pixel == VR.RGBA8:
                assert (a[:, :, 3] == 255).all()
