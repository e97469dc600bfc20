"""replay --dump-cloud: one well-formed PLY per keyframe, each with the vertices of export_cloud of a twin tracker at
the frame that made the keyframe (synthetic frames are fed as they are), byte for byte."""
import os

import numpy as np
import pytest

from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam

pytestmark = pytest.mark.gpu


def test_dump_cloud_writes_a_ply_per_keyframe(tmp_path):
    frames, step, max_depth = 6, 8, 6.0
    out = tmp_path / "cloud"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-cloud", str(out), "--cloud-step", str(step),
                 "--cloud-max-depth", str(max_depth)])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    twin = StereoSlam(cfg)
    want, newest = {}, -1
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        kf = int(twin.stats().n_keyframes) - 1
        if kf != newest:
            newest = kf
            job = twin.export_cloud("last_keyframes", None, step=step, max_depth=max_depth)
            assert int(job.segments[0]["status"]) == hip_lib.CLOUD_OK and int(job.segments[0]["keyframe_id"]) == kf
            want[kf] = job.points(0).copy()
    twin.close()
    assert 0 in want and sorted(os.listdir(out)) == [f"kf{kf:06d}_cloud.ply" for kf in sorted(want)]
    for kf, points in want.items():
        raw = (out / f"kf{kf:06d}_cloud.ply").read_bytes()
        head, body = raw.split(b"end_header\n", 1)
        assert head.decode("ascii").split("\n") == [
            "ply", "format binary_little_endian 1.0", f"element vertex {len(points)}", "property float x", "property float y",
            "property float z", "property uchar red", "property uchar green", "property uchar blue", ""]
        assert len(points) > 100 and len(body) == 15 * len(points)
        v = np.frombuffer(body, replay.PLY_VERTEX)
        assert all(v[k].tobytes() == points[k].tobytes() for k in ("x", "y", "z"))
        assert all(np.array_equal(v[k], points["color"][:, i]) for i, k in enumerate(("red", "green", "blue")))
        assert np.array_equal(replay.read_ply(out / f"kf{kf:06d}_cloud.ply"), v)
        cols, rows = cfg["width"] // step, cfg["height"] // step
        assert len(points) < cols * rows                                    # the depth filter and the invalid border drop some
