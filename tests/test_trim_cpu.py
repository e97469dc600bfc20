"""Trimmed keyframes without a GPU: the layout of svo_keyframe_range and of the fields a trimmed slot reports against
the binding, trimmed host parts of a snapshot through svo_snapshot_info (built here from the helpers of
tests/snapshot_ref.py, which states the untrimmed format), and the host logic that passes a keyframe window on
(multi_seq.play_queue, replay's flag)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import snapshot_ref as SR
from stereo_svo_slam_amd import hip_lib, multi_seq, replay, synth
from stereo_svo_slam_amd.hip_lib import SvoError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = synth.CONFIGS["tiny"]


def test_struct_layouts(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n'
        '  printf("%zu %zu %zu %zu %zu\\n", sizeof(svo_keyframe_range), offsetof(svo_keyframe_range, first),\n'
        '         offsetof(svo_keyframe_range, retired), offsetof(svo_keyframe_range, count), offsetof(svo_keyframe_range, table));\n'
        '  printf("%zu %zu %zu\\n", sizeof(svo_map_segment), offsetof(svo_map_segment, time_stamp), offsetof(svo_map_segment, first_keyframe));\n'
        '  printf("%zu %zu\\n", sizeof(struct svo_snapshot_info), offsetof(struct svo_snapshot_info, first_keyframe));\n'
        '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    r = hip_lib.KeyframeRange
    assert rows[0] == [C.sizeof(r), r.first.offset, r.retired.offset, r.count.offset, r.table.offset] == [16, 0, 4, 8, 12]
    seg = hip_lib.MAP_SEGMENT_DTYPE
    assert rows[1] == [seg.itemsize, seg.fields["time_stamp"][1], seg.fields["_pad"][1]] == [64, 48, 52]
    rec = np.zeros(1, seg)
    rec["_pad"][0] = (9, 0, 0)
    assert hip_lib.map_first_keyframe(rec[0]) == 9
    info = hip_lib.SnapshotInfo
    assert rows[2] == [C.sizeof(info), info._reserved.offset] == [160, 156]
    i = info()
    i._reserved = 7
    assert i.first_keyframe == 7


# ---------------------------------------------------------------------------------------------- trimmed host parts

KEYFRAMES = [(33, -1), (21, -1), (50, 1), (44, 0)]       # four keyframes, two retired; frame 5


def _untrimmed():
    return SR.host_part(CFG, frame_id=5, n_keypoints=40, keyframes=KEYFRAMES, n_sets=2, retired=2)


def _trimmed(first, n_keyframes=len(KEYFRAMES), retired=2, keep_planes=False):
    """The host part of the same slot with keyframes [0, first) trimmed: the helper writes the sections of the resident
    keyframes (keep_planes: and, wrongly, the directory of all of them), the header then states the absolute counts."""
    resident = KEYFRAMES[max(first, 0):]
    part, sections, fields = SR.host_part(CFG, frame_id=5, n_keypoints=40, keyframes=resident, n_sets=2, retired=0)
    if keep_planes:
        full, fsec, ffields = _untrimmed()
        directory = full[fsec["directory"]:fsec["end"]]
        part = part[:sections["directory"]] + directory
        fields = dict(fields, n_planes=ffields["n_planes"], host_bytes=len(part), data_bytes=ffields["data_bytes"])
    return SR.with_header(part, fields, n_keyframes=n_keyframes, keyframes_retired=retired, _reserved=first), fields


def _rejected(part, why):
    with pytest.raises(SvoError, match="snapshot"):
        hip_lib.snapshot_info(part)
        pytest.fail(f"accepted: {why}")


def test_an_untrimmed_part_still_validates():
    part, _, fields = _untrimmed()
    info = hip_lib.snapshot_info(part)
    assert info.first_keyframe == 0 and info.n_keyframes == 4 and info.n_planes == 14 + 12 * 4 + 2 * (info.pyramid_levels + info.lk_levels)
    assert info.host_bytes == len(part) == fields["host_bytes"]


@pytest.mark.parametrize("first", (1, 2))
def test_a_trimmed_part_is_accepted(first):
    part, fields = _trimmed(first)
    full, _, ffields = _untrimmed()
    info = hip_lib.snapshot_info(part)
    assert (info.first_keyframe, info.n_keyframes, info.keyframes_retired) == (first, 4, 2)
    assert info.n_planes == 14 + 12 * (4 - first) + 2 * (info.pyramid_levels + info.lk_levels) == ffields["n_planes"] - 12 * first
    assert info.host_bytes == len(part) == len(full) - first * (SR.KEYFRAME.size + 12 * SR.PLANE.size)
    gone = sum((e * n + 15) // 16 * 16 for n, _ in KEYFRAMES[:first] for e in SR.KP_ELEM)
    assert info.data_bytes == ffields["data_bytes"] - gone


def test_bad_trimmed_parts_are_rejected():
    _rejected(_trimmed(3)[0], "first_keyframe 3 > keyframes_retired 2: a live keyframe was trimmed")
    part, fields = _trimmed(1)
    _rejected(SR.with_header(part, dict(fields, n_keyframes=4, keyframes_retired=2), _reserved=-1), "a negative first_keyframe")
    _rejected(_trimmed(1, keep_planes=True)[0], "the directory still carries the trimmed keyframe's planes")
    _rejected(_trimmed(1, n_keyframes=5)[0], "one keyframe more than the sections hold")
    # the resident count is what the table bounds: ids beyond it are fine, 4097 resident keyframes are not
    _rejected(SR.with_header(part, dict(fields, keyframes_retired=2), n_keyframes=SR.MAX_KEYFRAMES + 2, _reserved=1), "4097 resident keyframes")
    # a retired keyframe among the resident ones must not name an image set
    bad = _trimmed(1)[0]
    at = SR.host_part(CFG, frame_id=5, n_keypoints=40, keyframes=KEYFRAMES[1:], n_sets=2)[1]["keyframes"]
    bad = bad[:at] + SR.KEYFRAME.pack(*[0.0] * 6, 21, 1) + bad[at + SR.KEYFRAME.size:]
    _rejected(bad, "keyframe 1 is retired and names image set 1")


def test_ids_far_beyond_the_table_are_accepted():
    """a long run: 100 000 keyframes made, the last two resident"""
    resident = [(50, 1), (44, 0)]
    part, _, fields = SR.host_part(CFG, frame_id=5, n_keypoints=40, keyframes=resident, n_sets=2, retired=0)
    part = SR.with_header(part, fields, n_keyframes=100000, keyframes_retired=99998, _reserved=99998)
    info = hip_lib.snapshot_info(part)
    assert (info.first_keyframe, info.n_keyframes, info.n_planes) == (99998, 100000, fields["n_planes"])


# ------------------------------------------------------------------------------------------------- host logic

class _FakeSlam:
    """what play_queue touches of a ctx"""

    def __init__(self, n):
        self.n, self.calls = n, []

    def set_keyframe_window(self, keep):
        self.calls.append(("window", keep))

    def restart(self, slots):
        self.calls.append(("restart", tuple(slots)))

    def new_images(self, L, R, ts):
        self.calls.append(("frames", tuple(x is not None for x in L)))


def _play(**kw):
    slam = _FakeSlam(2)
    frame = np.zeros((4, 4), np.uint8)
    where, frames = multi_seq.play_queue(slam, lambda s, k: (frame, frame), [2, 1, 2], **kw)
    return slam.calls, where, frames


def test_play_queue_passes_the_window_on():
    plain, where, frames = _play()
    assert frames == 5 and not any(c[0] == "window" for c in plain)
    for keep in (0, 3, -1):
        calls, where_k, frames_k = _play(keyframe_window=keep)
        assert calls[0] == ("window", keep) and calls[1:] == plain and (where_k, frames_k) == (where, frames)
    for bad in (-2, 1.5, "3"):
        with pytest.raises((ValueError, TypeError)):
            _play(keyframe_window=bad)


def test_replay_flag():
    ap = replay.build_parser()
    assert ap.parse_args(["--synthetic", "tiny"]).keyframe_window is None
    assert ap.parse_args(["--synthetic", "tiny", "--keyframe-window", "0"]).keyframe_window == 0
    assert ap.parse_args(["--synthetic", "tiny", "--keyframe-window", "12"]).keyframe_window == 12
    for bad in ("-1", "many"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--synthetic", "tiny", "--keyframe-window", bad])
