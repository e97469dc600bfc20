"""replay --dump-disparity --disparity-sgm: the stacked file holds the value and aggregated-cost planes that the SGM job
delivers of the same frame, bit for bit, and they are the numpy statement's (tests/sgm_ref.py)."""
import os

import numpy as np
import pytest

import dense_ref as DR
import sgm_ref as SR
from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu


def test_disparity_sgm_writes_the_jobs_planes(tmp_path):
    frames, step, p1, p2, cap = 2, 16, 16, 128, 2047
    out = tmp_path / "disp"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-disparity", str(out), "--disparity-step", str(step),
                 "--disparity-sgm", f"{p1},{p2},{cap}"])
    assert sorted(os.listdir(out)) == [f"{k:06d}_disparity.npy" for k in range(frames)]
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    cols, rows, _, _ = DR.lattice(cfg["width"], cfg["height"], step)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    for k in range(frames):
        batch.new_images([L[k].cuda()], [R[k].cuda()], [float(ts[k])])
        got = np.load(out / f"{k:06d}_disparity.npy")
        assert got.dtype == np.float32 and got.shape == (2, rows, cols)
        job = batch.export_disparity("frames", None, step=step, cost=True, sgm=dict(p1=p1, p2=p2, cost_cap=cap))
        assert got.tobytes() == np.ascontiguousarray(job.planes(0)).tobytes(), k
    batch.close()
    win, sx, sy = cfg["window_size_depth_calculator"], cfg["search_x"], cfg["search_y"]
    want = SR.planes_fast(L[-1].numpy(), R[-1].numpy(), win, sx, sy, step, p1, p2, cap)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[0] != np.floor(got[0])).any()
    # two arguments: the cost cap of the defaults
    short = tmp_path / "short"
    replay.main(["--synthetic", "tiny", "--frames", "1", "--dump-disparity", str(short), "--disparity-step", str(step), "--disparity-sgm", "32,256"])
    want = SR.planes_fast(L[0].numpy(), R[0].numpy(), win, sx, sy, step, 32, 256, hip_lib.SGM_DEFAULTS["cost_cap"])
    assert np.array_equal(np.load(short / "000000_disparity.npy").view(np.uint32), want.view(np.uint32))
