"""Snapshots without a GPU: svo_snapshot_info accepts the host part an independent statement of the format writes
(tests/snapshot_ref.py) and rejects every single-field corruption of it; the struct layouts of the C header
against the binding."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import snapshot_ref as SR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import SvoError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = synth.CONFIGS["tiny"]


def _valid():
    """frame 2 of a sequence with three keyframes: one retired, one with a set of its own, one on the current frame"""
    return SR.host_part(CFG, frame_id=2, n_keypoints=40, keyframes=[(33, -1), (50, 1), (44, 0)], n_sets=2, retired=1)


def _rejected(part, why):
    with pytest.raises(SvoError, match="snapshot"):
        hip_lib.snapshot_info(part)
        pytest.fail(f"accepted: {why}")


def test_struct_layouts(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n'
        '  printf("%zu %zu %zu %zu %zu\\n", sizeof(struct svo_snapshot_info), sizeof(svo_snapshot_keyframe),\n'
        '         sizeof(svo_snapshot_plane), sizeof(svo_snapshot), sizeof(svo_copy_segment));\n'
        '  printf("%zu %zu %zu %zu %zu\\n", offsetof(struct svo_snapshot_info, host_bytes), offsetof(struct svo_snapshot_info, cam),\n'
        '         offsetof(struct svo_snapshot_info, width), offsetof(struct svo_snapshot_info, frame_id),\n'
        '         offsetof(struct svo_snapshot_info, n_planes));\n'
        '  printf("%zu %zu\\n", sizeof(svo_frame_stats), sizeof(svo_pose));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    info = hip_lib.SnapshotInfo
    assert rows[0] == [SR.HEADER.size, SR.KEYFRAME.size, SR.PLANE.size, C.sizeof(hip_lib.SnapshotBuffers), C.sizeof(hip_lib.CopySegment)]
    assert rows[0][0] == C.sizeof(info)
    assert rows[1] == [info.host_bytes.offset, info.cam.offset, info.width.offset, info.frame_id.offset, info.n_planes.offset]
    assert rows[1] == [struct.calcsize("<4I"), struct.calcsize("<4I2q"), struct.calcsize("<4I2q10f9i"),
                       struct.calcsize("<4I2q10f9i5i"), struct.calcsize("<4I2q10f9i11i")]
    assert rows[2] == [SR.STATS_BYTES, SR.POSE.size]


def test_valid_parts_are_accepted():
    part, sections, fields = _valid()
    assert len(part) == sections["end"] == fields["host_bytes"]
    info = hip_lib.snapshot_info(part)
    for name in ("magic", "version", "byte_order", "status", "host_bytes", "data_bytes") + SR.COUNTS:
        assert getattr(info, name) == fields[name], name
    for name in SR.CAM_FLOATS + SR.CAM_INTS:
        assert getattr(info.cam, name) == CFG[name], name
    assert info.capacity == hip_lib.export_capacity(hip_lib.CameraSettings.from_dict(CFG), CFG["width"], CFG["height"])
    assert SR.parse(part)["directory"][-1][1:] == (80, 60)          # the last plane: LK level 2 of set 1
    assert hip_lib.snapshot_info(part + b"\x00" * 7).host_bytes == len(part)      # more bytes than needed: fine
    # an empty slot, and a header-only part (a save whose capacity was too small)
    empty, _, f = SR.host_part(CFG)
    info = hip_lib.snapshot_info(empty)
    assert (info.frame_id, info.n_planes, info.n_keyframes, info.data_bytes) == (-1, 14, 0, 32)
    small = SR.with_header(part, fields, status=SR.TOO_SMALL)[:SR.HEADER.size]
    assert hip_lib.snapshot_info(small).status == hip_lib.SNAPSHOT_TOO_SMALL


HEADER_CORRUPTIONS = [
    dict(magic=SR.MAGIC ^ 1), dict(version=2), dict(version=0), dict(byte_order=0x04030201), dict(status=2),
    dict(host_bytes=-1), dict(_reserved=1),
    dict(width=CFG["width"] + 40), dict(height=8), dict(capacity=SR.capacity(CFG) + 64), dict(pyramid_levels=3),
    dict(lk_levels=2), dict(max_pyramid_levels=9), dict(grid_width=0), dict(window_size_pose_estimator=5),
    dict(frame_id=-2), dict(frame_id=3), dict(n_trajectory=2), dict(n_keypoints=SR.capacity(CFG) + 1), dict(n_keypoints=-1),
    dict(n_keyframes=SR.MAX_KEYFRAMES + 1), dict(n_keyframes=2), dict(n_keyframes=-1), dict(keyframes_retired=3),
    dict(keyframes_retired=-1), dict(n_image_sets=5), dict(n_image_sets=1), dict(n_image_sets=0), dict(n_planes=13),
    dict(data_bytes=-16),
]


@pytest.mark.parametrize("change", HEADER_CORRUPTIONS, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_header_corruptions_are_rejected(change):
    part, _, fields = _valid()
    _rejected(SR.with_header(part, fields, **change), change)


def test_sizes_are_checked():
    part, _, fields = _valid()
    for delta in (-16, -1, 1, 16):
        _rejected(SR.with_header(part, fields, host_bytes=fields["host_bytes"] + delta), f"host_bytes {delta:+d}")
    # a data part too short for the directory: every size from "the last plane ends past it" down
    last = SR.parse(part)["directory"][-1]
    end = last[0] + last[1] * last[2]
    assert hip_lib.snapshot_info(SR.with_header(part, fields, data_bytes=end)).data_bytes == end
    for short in (end - 1, last[0], 16, 0):
        _rejected(SR.with_header(part, fields, data_bytes=short), f"data_bytes {short}")


def test_keyframe_and_directory_corruptions_are_rejected():
    part, sections, fields = _valid()

    def patched(offset, fmt, *values):
        b = bytearray(part)
        struct.pack_into(fmt, b, offset, *values)
        return bytes(b)

    kf = lambda i: sections["keyframes"] + SR.KEYFRAME.size * i
    _rejected(patched(kf(1) + 24, "<i", SR.capacity(CFG) + 1), "a keyframe's count above the capacity")
    _rejected(patched(kf(1) + 24, "<i", -1), "a negative keyframe count")
    _rejected(patched(kf(1) + 24, "<i", 49), "a keyframe count that the directory does not match")
    _rejected(patched(kf(2) + 28, "<i", 2), "an image set that does not exist")
    _rejected(patched(kf(2) + 28, "<i", -2), "image set -2")
    _rejected(patched(kf(0) + 28, "<i", 0), "a retired keyframe with images")
    _rejected(patched(kf(1) + 28, "<i", 0), "image set 1 without a keyframe")
    n = fields["n_planes"]
    entry = lambda i: sections["directory"] + SR.PLANE.size * i
    for i in (0, 13, 14, n - 1):
        off, row_bytes, rows = SR.parse(part)["directory"][i]
        _rejected(patched(entry(i), "<q", fields["data_bytes"] - row_bytes * rows + 1), f"plane {i} ends past the data part")
        _rejected(patched(entry(i), "<q", 1 << 62), f"plane {i} far past the end")
        _rejected(patched(entry(i), "<q", -16), f"plane {i} at a negative offset")
        _rejected(patched(entry(i) + 8, "<i", row_bytes + 4), f"plane {i}: row_bytes")
        _rejected(patched(entry(i) + 12, "<i", rows + 1), f"plane {i}: rows")
        _rejected(patched(entry(i) + 12, "<i", -rows), f"plane {i}: negative rows")


def test_truncation_at_every_section_boundary():
    part, sections, _ = _valid()
    for name, at in sections.items():
        for size in {max(at - 1, 0), at, at + 1} - {len(part), len(part) + 1}:
            _rejected(part[:size], f"truncated to {size} bytes ({name})")
    _rejected(b"", "no bytes")
