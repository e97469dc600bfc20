"""The bulk export without a GPU: the restatement (tests/export_ref.py) pinned on hand-written records, the struct
layouts of the C header against the Python dtypes, and svo_export_capacity."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import export_ref as ER
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import CameraSettings
from stereo_svo_slam_amd.stereo_slam import KP_INFO_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_layout(tmp_path):
    """sizeof and offsetof of the export structs as a C compiler sees include/svo_hip.h"""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    names = [f[0] for f in ER.SEGMENT_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n'
        '  printf("segment %zu\\n", sizeof(svo_export_segment));\n'
        '  printf("info %zu\\n", sizeof(svo_kp_info));\n'
        '  printf("dst %zu %zu %zu %zu %zu %zu\\n", sizeof(svo_export_dst), offsetof(svo_export_dst, segments),\n'
        '         offsetof(svo_export_dst, kps2d), offsetof(svo_export_dst, kps3d), offsetof(svo_export_dst, info),\n'
        '         offsetof(svo_export_dst, capacity));\n' +
        "".join(f'  printf("{n} %zu\\n", offsetof(svo_export_segment, {n}));\n' for n in names) +
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}


def test_struct_layouts(tmp_path):
    c = _c_layout(tmp_path)
    assert c["segment"] == [64] == [hip_lib.EXPORT_SEGMENT_DTYPE.itemsize] == [ER.SEGMENT_BYTES]
    assert c["info"] == [44] == [KP_INFO_DTYPE.itemsize] == [ER.INFO_BYTES]
    for name, offset, kind, count in ER.SEGMENT_FIELDS:
        assert c[name] == [offset], name
        dt, off = hip_lib.EXPORT_SEGMENT_DTYPE.fields[name][:2]
        assert off == offset and dt.base == np.dtype(kind) and int(np.prod(dt.shape, dtype=int)) == count, name
    assert set(hip_lib.EXPORT_SEGMENT_DTYPE.names) == {f[0] for f in ER.SEGMENT_FIELDS}
    for name, offset, kind, count in ER.INFO_FIELDS:
        dt, off = KP_INFO_DTYPE.fields[name][:2]
        assert off == offset and dt.base == np.dtype(kind) and int(np.prod(dt.shape, dtype=int)) == count, name
    d = hip_lib.ExportDst
    assert c["dst"] == [C.sizeof(d), d.segments.offset, d.kps2d.offset, d.kps3d.offset, d.info.offset, d.capacity.offset]


@pytest.mark.parametrize("config", ["tiny", "euroc", "hd"])
def test_export_capacity(config):
    cfg = synth.CONFIGS[config]
    cam = CameraSettings.from_dict(cfg)
    got = hip_lib.export_capacity(cam, cfg["width"], cfg["height"])
    cells = (cfg["width"] // cfg["grid_width"]) * (cfg["height"] // cfg["grid_height"])
    assert got == (2 * cells + 128 + 63) // 64 * 64 == ER.capacity(cfg)
    assert got % 4 == 0


def test_export_capacity_of_the_euroc_grid():
    cfg = dict(synth.CONFIGS["euroc"], grid_width=54, grid_height=48)
    assert (cfg["width"], cfg["height"]) == (752, 480)
    assert hip_lib.export_capacity(CameraSettings.from_dict(cfg), 752, 480) == 448


def test_export_capacity_rejects_bad_arguments():
    cfg = synth.CONFIGS["tiny"]
    cam = CameraSettings.from_dict(cfg)
    out = C.c_int(-7)
    lib = hip_lib.lib()
    assert lib.svo_export_capacity(None, cfg["width"], cfg["height"], C.byref(out)) == -1
    assert lib.svo_export_capacity(C.byref(cam), cfg["width"], cfg["height"], None) == -1
    assert lib.svo_export_capacity(C.byref(cam), 8, cfg["height"], C.byref(out)) == -1
    bad = CameraSettings.from_dict(dict(cfg, grid_width=0))
    assert lib.svo_export_capacity(C.byref(bad), cfg["width"], cfg["height"], C.byref(out)) == -1
    assert out.value == -7
    with pytest.raises(hip_lib.SvoError):
        hip_lib.export_capacity(bad, cfg["width"], cfg["height"])


def _planes(**kw):
    base = {k: np.zeros(1, np.uint32) for k in ER.PLANES}
    for k, v in kw.items():
        base[k] = np.array([v]).astype(np.float32).view(np.uint32) if isinstance(v, float) else np.array([v], np.uint32)
    return base


def test_hand_written_records():
    """svo_kp_info by hand (struct.pack of its fields in order) against the restatement"""
    rec = ER.info_records(_planes(score=37.5, level_type=2 | 1 << 8, keyframe_id=7, keypoint_index=311, color=0x00CCBBAA,
                                  flags=ER.IGNORE_DURING_REFINEMENT | ER.IGNORE_TEMPORARY, outlier_count=3, inlier_count=9,
                                  kf_inv_depth=0.25, kf_variance=1.5))
    want = struct.pack("<fiiii3B3B2xiiff", 37.5, 2, 1, 7, 311, 0xAA, 0xBB, 0xCC, 1, 0, 1, 3, 9, 0.25, 1.5)
    assert len(want) == 44 and rec.tobytes() == want
    v = rec.view(KP_INFO_DTYPE)[0, 0]
    assert (v["level"], v["type"], tuple(v["color"])) == (2, 1, (0xAA, 0xBB, 0xCC))
    # the colour's top byte, flag bits beyond the three, level | type beyond 16 bits: not part of a record
    rec = ER.info_records(_planes(color=0xFF010203, flags=0xfffffff8 | ER.IGNORE_COMPLETELY, level_type=0x00ab0305))
    want = struct.pack("<fiiii3B3B2xiiff", 0.0, 5, 3, 0, 0, 3, 2, 1, 0, 1, 0, 0, 0, 0.0, 0.0)
    assert rec.tobytes() == want
    # negative counters and float bit patterns pass through unchanged
    rec = ER.info_records(_planes(outlier_count=np.uint32(0xffffffff), kf_variance=np.uint32(0x7fc00001), score=np.uint32(0x80000000)))
    assert rec[0, 28:32].tobytes() == b"\xff" * 4 and rec[0, 40:44].tobytes() == struct.pack("<I", 0x7fc00001)
    assert rec[0, 0:4].tobytes() == struct.pack("<I", 0x80000000)


def test_placement_rule():
    # one group: dense, every first a multiple of 4
    assert ER.placement([0, 1, 2, 3], [5, 0, 4, 3], [(0, 4)], 64) == [0, 8, 8, 12]
    # three groups of 2: a group starts at (named slots of earlier groups) * capacity; named order inside a group
    groups = ER.group_ranges(6, 3)
    assert groups == [(0, 2), (2, 2), (4, 2)]
    assert ER.placement([0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6], groups, 64) == [0, 4, 128, 132, 256, 264]
    assert ER.placement([5, 0, 4, 1], [6, 1, 5, 2], groups, 64) == [128, 0, 136, 4]
    assert ER.group_ranges(66, 3) == [(0, 22), (22, 22), (44, 22)] and ER.group_ranges(5, 2) == [(0, 3), (3, 2)]


def test_pack_leaves_the_rest_alone():
    rng = np.random.default_rng(3)
    sets = []
    for n in (3, 0, 5):
        planes = {k: rng.integers(0, 2**32, n, dtype=np.uint32) for k in ER.PLANES}
        sets.append((n, rng.random((n, 2), np.float32), rng.random((n, 3), np.float32), planes))
    first = ER.placement([0, 1, 2], [3, 0, 5], [(0, 3)], 64)
    assert first == [0, 4, 4]
    o2, o3, oi = ER.pack(sets, first, 16)
    assert np.all(o2[3] == 0xA5) and np.all(oi[3] == 0xA5) and np.all(o3[9:] == 0xA5)
    assert o2[4:9].tobytes() == sets[2][1].tobytes() and o3[:3].tobytes() == sets[0][2].tobytes()
    assert oi[4:9].tobytes() == ER.info_records(sets[2][3]).tobytes()
