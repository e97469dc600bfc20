"""The map export without a GPU: the struct layouts of the C header against the Python types, the restatement
(tests/map_ref.py) pinned on hand-written sets, and wire.keyframes_messages on a fake export."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np

import map_ref as MR
from stereo_svo_slam_amd import hip_lib, wire
from stereo_svo_slam_amd.stereo_slam import Frame, KP_INFO_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = (("svo_map_point", MR.POINT_FIELDS, MR.POINT_BYTES), ("svo_map_filter", MR.FILTER_FIELDS, MR.FILTER_BYTES),
           ("svo_map_keyframe", MR.KEYFRAME_FIELDS, MR.KEYFRAME_BYTES), ("svo_map_segment", MR.SEGMENT_FIELDS, MR.SEGMENT_BYTES),
           ("svo_map_region", MR.REGION_FIELDS, MR.REGION_BYTES))


def _c_layout(tmp_path):
    """sizeof and offsetof of the map structs as a C compiler sees include/svo_hip.h"""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    lines = []
    for name, fields, _ in STRUCTS:
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in fields]
    lines.append('  printf("svo_map_dst %zu %zu %zu %zu\\n", sizeof(svo_map_dst), offsetof(svo_map_dst, segments),\n'
                 '         offsetof(svo_map_dst, keyframes), offsetof(svo_map_dst, points));\n')
    lines.append('  printf("status %d %d\\n", SVO_MAP_COMPLETE, SVO_MAP_TOO_SMALL);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}


def _check_dtype(dtype, fields, size):
    assert dtype.itemsize == size and set(dtype.names) == {f[0] for f in fields}
    for name, offset, kind, count in fields:
        dt, off = dtype.fields[name][:2]
        assert off == offset and dt.base == np.dtype(kind) and int(np.prod(dt.shape, dtype=int)) == count, name


def test_struct_layouts(tmp_path):
    c = _c_layout(tmp_path)
    assert [size for _, _, size in STRUCTS] == [16, 16, 48, 64, 32]
    for name, fields, size in STRUCTS:
        assert c[name] == [size], name
        for f in fields:
            assert c[f"{name}.{f[0]}"] == [f[1]], (name, f[0])
    _check_dtype(hip_lib.MAP_POINT_DTYPE, MR.POINT_FIELDS, 16)
    _check_dtype(hip_lib.MAP_KEYFRAME_DTYPE, MR.KEYFRAME_FIELDS, 48)
    _check_dtype(hip_lib.MAP_SEGMENT_DTYPE, MR.SEGMENT_FIELDS, 64)
    _check_dtype(hip_lib.MAP_REGION_DTYPE, MR.REGION_FIELDS, 32)
    f = hip_lib.MapFilter
    assert C.sizeof(f) == 16
    assert [getattr(f, n[0]).offset for n in MR.FILTER_FIELDS] == [n[1] for n in MR.FILTER_FIELDS]
    d = hip_lib.MapDst
    assert c["svo_map_dst"] == [C.sizeof(d), d.segments.offset, d.keyframes.offset, d.points.offset]
    assert c["status"] == [hip_lib.MAP_COMPLETE, hip_lib.MAP_TOO_SMALL] == [MR.COMPLETE, MR.TOO_SMALL]
    assert (hip_lib.IGNORE_DURING_REFINEMENT, hip_lib.IGNORE_COMPLETELY, hip_lib.IGNORE_TEMPORARY) == (1, 2, 4)
    assert "svo_pack_map_points" in hip_lib.SYMBOLS and "svo_submit_export_map" in hip_lib.SYMBOLS
    lib = hip_lib.lib()
    for sym in ("svo_map_size", "svo_submit_export_map", "svo_export_map", "svo_pack_map_points"):
        getattr(lib, sym)


# ---------------------------------------------------------------------------------- map_ref on hand-written sets

def _set(own_id, rows):
    """rows: (x, y, z, flags, keyframe_id, inlier_count, colour word) per keypoint"""
    k3 = np.array([r[:3] for r in rows], np.float32).reshape(-1, 3)
    planes = {name: np.array([np.uint32(r[3 + i] & 0xffffffff) for r in rows], np.uint32) for i, name in enumerate(MR.PLANES)}
    return (len(rows), own_id, k3, planes)


SET_A = _set(0, [(1.0, 2.0, 3.0, 0, 0, 9, 0x00332211),
                 (4.0, 5.0, 6.0, MR.IGNORE_COMPLETELY, 0, 1, 0xFF665544),
                 (7.0, 8.0, 9.0, MR.IGNORE_TEMPORARY | 0xfffffff8, 0, 8, 0x00998877)])
SET_B = _set(1, [(1.5, 2.5, 3.5, 0, 0, 9, 0x00332211),          # a stale copy of keyframe 0's point
                 (-1.0, -2.0, -3.0, 0, 1, 7, 0x00010203),
                 (0.5, 0.25, 0.125, MR.IGNORE_DURING_REFINEMENT, 1, -1, 0x00a0b0c0)])


def _pt(x, y, z, r, g, b, flags):
    return struct.pack("<fff4B", x, y, z, r, g, b, flags)


def test_hand_written_points():
    rec = MR.point_records(SET_A[2], SET_A[3])
    assert rec.shape == (3, 16)
    assert rec[0].tobytes() == _pt(1.0, 2.0, 3.0, 0x11, 0x22, 0x33, 0)
    assert rec[1].tobytes() == _pt(4.0, 5.0, 6.0, 0x44, 0x55, 0x66, 2)       # the colour's top byte is no part of a point
    assert rec[2].tobytes() == _pt(7.0, 8.0, 9.0, 0x77, 0x88, 0x99, 4)       # nor flag bits beyond the three
    assert rec.view(hip_lib.MAP_POINT_DTYPE)[1, 0]["flags"] == 2
    # any bit pattern of kps3d passes through, NaNs included
    bits = np.array([[0x7fc00001, 0xffffffff, 0x80000000]], np.uint32)
    rec = MR.point_records(bits, {"flags": np.zeros(1, np.uint32), "color": np.zeros(1, np.uint32)})
    assert rec[0, :12].tobytes() == struct.pack("<3I", 0x7fc00001, 0xffffffff, 0x80000000)


def _kept(filt):
    return [MR.keep_mask(s[3], s[1], filt).tolist() for s in (SET_A, SET_B)]


def test_every_filter_field():
    assert _kept({}) == [[True, True, True], [True, True, False]]          # (inlier_count -1 < 0)
    assert _kept(dict(min_inliers=-1)) == [[True] * 3, [True] * 3]
    assert _kept(dict(drop_flags=MR.IGNORE_COMPLETELY, min_inliers=-1)) == [[True, False, True], [True, True, True]]
    assert _kept(dict(drop_flags=MR.IGNORE_TEMPORARY | MR.IGNORE_DURING_REFINEMENT, min_inliers=-1)) == [[True, True, False], [True, True, False]]
    assert _kept(dict(own_only=1, min_inliers=-1)) == [[True] * 3, [False, True, True]]
    assert _kept(dict(own_only=7, min_inliers=-1)) == [[True] * 3, [False, True, True]]      # any value but 0 is "on"
    assert _kept(dict(min_inliers=8)) == [[True, False, True], [True, False, False]]
    assert _kept(dict(min_inliers=10)) == [[False] * 3, [False] * 3]
    assert _kept(dict(drop_flags=MR.IGNORE_COMPLETELY, own_only=1, min_inliers=8)) == [[True, False, True], [False, False, False]]


def test_pack_is_dense_and_leaves_the_rest_alone():
    empty = _set(5, [])
    regions = [[SET_A, empty, SET_B], [], [SET_B]]
    first = [2, 9, 11]
    points, counts = MR.pack(regions, first, dict(own_only=1, min_inliers=-1), 16)
    assert counts == [3, 0, 2, 2]
    a, b = MR.point_records(SET_A[2], SET_A[3]), MR.point_records(SET_B[2], SET_B[3])
    assert points[2:5].tobytes() == a.tobytes() and points[5:7].tobytes() == b[1:].tobytes()
    assert points[11:13].tobytes() == b[1:].tobytes()
    untouched = np.ones(16, bool)
    untouched[2:7] = untouched[11:13] = False
    assert np.all(points[untouched] == 0xA5)
    points, counts = MR.pack(regions, first, dict(min_inliers=100), 16)
    assert counts == [0, 0, 0, 0] and np.all(points == 0xA5)
    # a set's n bounds what is read of its planes
    points, counts = MR.pack([[(2,) + SET_A[1:]]], [0], dict(min_inliers=-1), 4)
    assert counts == [2] and points[:2].tobytes() == a[:2].tobytes() and np.all(points[2:] == 0xA5)


# ---------------------------------------------------------------------------------- wire

class _FakeSlam:
    """keyframes per slot as (pose, kps3d, colours); the getters of StereoSlamBatch that keyframes_message uses and
    an export_map that answers with a numpy-built export of MapExport's interface"""

    def __init__(self, slots):
        self.slots = slots
        self.n = len(slots)
        self.map_exports = 0

    def num_keyframes(self, seq=0):
        return len(self.slots[seq])

    def get_keyframe(self, kid=None, seq=0):
        pose, k3, col = self.slots[seq][kid]
        info = np.zeros(len(k3), KP_INFO_DTYPE)
        info["color"] = col
        return Frame(pose, np.zeros((len(k3), 2), np.float32), k3, info)

    def export_map(self, seqs=None, from_keyframe=None, filter=None, device=False):
        assert from_keyframe is None and filter is None
        self.map_exports += 1
        return _FakeMapExport(self, list(range(self.n)) if seqs is None else list(seqs))


class _FakeMapExport:
    def __init__(self, slam, seqs):
        regions, first, at = [], [], 3
        self._kfs, self.segments = [], np.zeros(len(seqs), hip_lib.MAP_SEGMENT_DTYPE)
        for i, s in enumerate(seqs):
            sets, kfs = [], np.zeros(len(slam.slots[s]), hip_lib.MAP_KEYFRAME_DTYPE)
            n_points = 0
            for k, (pose, k3, col) in enumerate(slam.slots[s]):
                word = col[:, 0].astype(np.uint32) | col[:, 1].astype(np.uint32) << 8 | col[:, 2].astype(np.uint32) << 16
                z = np.zeros(len(k3), np.uint32)
                sets.append((len(k3), k, k3, {"flags": z, "keyframe_id": z + k, "inlier_count": z, "color": word}))
                kfs[k] = (k, len(k3), len(k3), 0, at + n_points, pose)
                n_points += len(k3)
            regions.append(sets)
            first.append(at)
            self._kfs.append(kfs)
            self.segments[i]["seq"], self.segments[i]["n_exported"], self.segments[i]["n_points"] = s, len(kfs), n_points
            self.segments[i]["frame_id"] = 0 if len(kfs) else -1
            at += n_points + 2
        self._points = MR.pack(regions, first, MR.KEEP_ALL, at)[0].view(hip_lib.MAP_POINT_DTYPE)[:, 0]

    def keyframes(self, i):
        return self._kfs[i]

    def points_of_keyframe(self, i, k):
        kf = self._kfs[i][k]
        return self._points[int(kf["first"]):int(kf["first"]) + int(kf["n"])]


def test_keyframes_messages_equal_keyframes_message():
    rng = np.random.default_rng(5)

    def kf(n):
        pose = rng.normal(size=6).astype(np.float32)
        return (pose, rng.normal(size=(n, 3)).astype(np.float32) * 10, rng.integers(0, 256, (n, 3)).astype(np.uint8))

    slam = _FakeSlam([[kf(4), kf(0), kf(7)], [], [kf(1)]])          # a keyframe with no keypoints, an empty slot
    for seqs in (None, [2, 0], [1]):
        texts = wire.keyframes_messages(slam, seqs)
        named = range(3) if seqs is None else seqs
        assert texts == [wire.keyframes_message(slam, s) for s in named]
    assert slam.map_exports == 3
    assert wire.keyframes_messages(slam, [1]) == ["[]"]
    assert '"keypoints":[]' in wire.keyframes_messages(slam, [0])[0]
