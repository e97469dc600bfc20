"""replay --dump-disparity: the files it writes, and one of them against the oracle's per-keypoint search on that frame's
planes (synthetic frames are fed as they are: no rectification, no conversion), bit for bit."""
import os

import numpy as np
import pytest

import dense_ref as DR
from stereo_svo_slam_amd import replay, synth
from test_dense_cpu import oracle_plane

pytestmark = pytest.mark.gpu


def test_dump_disparity_writes_the_maps(tmp_path):
    frames, step = 3, 16
    out = tmp_path / "disp"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-disparity", str(out), "--disparity-step", str(step)])
    assert sorted(os.listdir(out)) == [f"{k:06d}_disparity.npy" for k in range(frames)]
    cfg, L, R, _, _ = synth.make_sequence("tiny", frames, 0, device="cpu")
    cols, rows, _, _ = DR.lattice(cfg["width"], cfg["height"], step)
    k = 2
    got = np.load(out / f"{k:06d}_disparity.npy")
    assert got.dtype == np.float32 and got.shape == (rows, cols)
    want = oracle_plane(L[k].numpy(), R[k].numpy(), cfg["window_size_depth_calculator"], cfg["search_x"], cfg["search_y"], step)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got >= 0.5).mean() > 0.5 and len(np.unique(got)) > 4
    # depth: baseline / disparity where there is one, 0 elsewhere
    depth = tmp_path / "depth"
    replay.main(["--synthetic", "tiny", "--frames", "1", "--dump-disparity", str(depth), "--disparity-step", str(step), "--disparity-depth"])
    z, d = np.load(depth / "000000_disparity.npy"), np.load(out / "000000_disparity.npy")
    valid = d >= 0
    assert np.array_equal(z == 0, ~valid)
    assert np.array_equal(z[valid].view(np.uint32), (np.float32(cfg["baseline"]) / d[valid]).view(np.uint32))
