"""The dense disparity map without a GPU: the numpy statement (tests/dense_ref.py) against the oracle's per-keypoint
search on the lattice points of the crafted pairs (tests/dense_cases.py), what keeps those pairs honest, the struct
layouts of the C header against the Python types, svo_disparity_size and what it rejects. Bit for bit throughout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dense_cases as DC
import dense_ref as DR
import oracle_py as O
from stereo_svo_slam_amd import hip_lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = synth.CONFIGS["tiny"]
CAM = hip_lib.CameraSettings.from_dict(CFG)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_plane(left, right, win, sx, sy, step):
    """the oracle's disparity at every lattice point: float32 [rows, cols]"""
    h, w = left.shape
    cols, rows, _, _ = DR.lattice(w, h, step)
    kps = DR.lattice_keypoints(w, h, step)
    return np.asarray(O.ssd_disparity(left, right, kps, win, sx, sy, 1), np.float32).reshape(rows, cols)


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_statement_equals_the_oracle(name):
    left, right, win, sx, sy, step = DC.cases()[name]
    assert np.array_equal(_bits(DC.reference(name)[0]), _bits(oracle_plane(left, right, win, sx, sy, step)))


def test_the_cases_reach_what_they_are_for():
    for name in sorted(DC.cases()):
        value, cost = DC.reference(name)
        invalid = float((value < 0).mean())
        assert ((value < 0) == (cost < 0)).all(), name
        if name == "f":
            assert 0.3 < invalid < 0.9, (name, invalid)
        else:
            assert invalid == 0, (name, invalid)
        if name != "c":
            assert len(np.unique(value)) >= 4, name
    assert float((DC.reference("e")[1] >= 2.0**24).mean()) >= 0.5
    c = DC.reference("c")[0]
    assert float((c != np.round(c)).mean()) >= 0.5
    # the depth plane: baseline / disparity in float where valid, 0 elsewhere
    left, right, win, sx, sy, step = DC.cases()["f"]
    z = DR.planes(left, right, win, sx, sy, step, DR.DEPTH, False, baseline=20.0)[0]
    d = DC.reference("f")[0]
    assert np.array_equal(z == 0, d < 0)
    assert np.array_equal(_bits(z[d >= 0]), _bits(np.float32(20.0) / d[d >= 0]))


def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_disparity_style": hip_lib.DisparityStyle, "svo_disparity_segment": hip_lib.DisparitySegment,
                 "svo_disparity_dst": hip_lib.DisparityDst, "svo_dense_src": hip_lib.DenseSrc}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in cls._fields_]
    lines.append('  printf("enums %d %d %d %d\\n", SVO_DENSE_DISPARITY, SVO_DENSE_DEPTH, SVO_DISPARITY_OK, SVO_DISPARITY_NONE);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_disparity_style": 32, "svo_disparity_segment": 64, "svo_disparity_dst": 24, "svo_dense_src": 56}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f in cls._fields_:
            assert c[f"{name}.{f[0]}"] == [getattr(cls, f[0]).offset], (name, f[0])
    seg = hip_lib.DISPARITY_SEGMENT_DTYPE
    assert seg.itemsize == 64 and list(seg.names) == [f[0] for f in hip_lib.DisparitySegment._fields_]
    for f in seg.names:
        assert seg.fields[f][1] == getattr(hip_lib.DisparitySegment, f).offset, f
    assert c["enums"] == [hip_lib.DENSE_DISPARITY, hip_lib.DENSE_DEPTH, hip_lib.DISPARITY_OK, hip_lib.DISPARITY_NONE] == [0, 1, 0, 1]
    assert (DR.DISPARITY, DR.DEPTH) == (hip_lib.DENSE_DISPARITY, hip_lib.DENSE_DEPTH)
    lib = hip_lib.lib()
    for sym in ("svo_disparity_size", "svo_submit_export_disparity", "svo_export_disparity", "svo_dense_disparity"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def _style(value=0, step=1, win=0, sx=0, sy=0, cost=0, reserved=(0, 0)):
    st = hip_lib.DisparityStyle(value, step, win, sx, sy, cost)
    st._reserved[0], st._reserved[1] = reserved
    return st


def test_disparity_size():
    for step in (1, 3, 16):
        for cost in (0, 1):
            for w, h in ((320, 240), (752, 480), (97, 53)):
                cols, rows, planes, nbytes = hip_lib.disparity_size(CAM, w, h, _style(step=step, cost=cost))
                assert (cols, rows, planes) == (w // step, h // step, 1 + cost) == (*DR.lattice(w, h, step)[:2], 1 + cost)
                assert nbytes % 256 == 0 and 0 <= nbytes - planes * cols * rows * 4 < 256, (step, cost, w, h)
    assert hip_lib.disparity_size(CAM, 320, 240, _style()) == (320, 240, 1, 307200)          # style zeros: the ctx's settings
    assert hip_lib.disparity_size(CAM, 320, 240, _style(value=1, step=16, win=35, sx=64, sy=8, cost=1)) == (20, 15, 2, 2560)
    assert hip_lib.disparity_size(CAM, 320, 240, _style(win=1, sx=1, sy=1)) == (320, 240, 1, 307200)
    lib = hip_lib.lib()
    nbytes = C.c_int64(0)
    assert lib.svo_disparity_size(C.byref(CAM), 320, 240, C.byref(_style(step=3)), None, None, None, C.byref(nbytes)) == 0
    assert nbytes.value == (106 * 80 * 4 + 255) // 256 * 256
    assert lib.svo_disparity_size(C.byref(CAM), 320, 240, C.byref(_style()), None, None, None, None) == 0


def test_disparity_size_rejects():
    bad = [_style(value=2), _style(value=-1), _style(step=0), _style(step=17), _style(step=-1), _style(cost=2), _style(cost=-1),
           _style(win=36), _style(win=-1), _style(sx=65), _style(sx=-1), _style(sy=9), _style(sy=-1),
           _style(reserved=(1, 0)), _style(reserved=(0, 1))]
    for st in bad:
        with pytest.raises(hip_lib.SvoError):
            hip_lib.disparity_size(CAM, 320, 240, st)
    with pytest.raises(hip_lib.SvoError):
        hip_lib.disparity_size(CAM, 15, 240, _style(step=16))     # cols of 0
    with pytest.raises(hip_lib.SvoError):
        hip_lib.disparity_size(CAM, 320, 15, _style(step=16))     # rows of 0
    with pytest.raises(hip_lib.SvoError):
        hip_lib.disparity_size(CAM, 0, 240, _style())             # settings svo_ctx_create rejects
    lib = hip_lib.lib()
    assert lib.svo_disparity_size(C.byref(CAM), 320, 240, None, None, None, None, None) == -1
    assert lib.svo_disparity_size(None, 320, 240, C.byref(_style()), None, None, None, None) == -1
    # the calls that need a ctx or a handle reject a missing one before anything else
    dst = hip_lib.DisparityDst(None, None, 0)
    assert lib.svo_submit_export_disparity(None, 0, None, 0, C.byref(_style()), C.byref(dst), 0) == -1
    assert lib.svo_export_disparity(None, 0, None, 0, C.byref(_style()), C.byref(dst), 0) == -1
    assert lib.svo_dense_disparity(None, 0, None, None, C.byref(_style(win=7, sx=9, sy=2)), None) == -1
    assert hip_lib.lib().svo_last_error()
