"""replay --dump-disparity --disparity-lr and --dump-cloud --cloud-lr: the stacked file has the lr plane and equals the
checked job's planes of the same frame and the numpy statement (tests/lr_ref.py), bit for bit; the cloud loses points."""
import os

import numpy as np
import pytest

import dense_ref as DR
import lr_ref as LR
from stereo_svo_slam_amd import replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu


def test_disparity_lr_stacks_the_plane(tmp_path):
    frames, step, diff = 2, 16, 1.0
    out = tmp_path / "disp"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-disparity", str(out), "--disparity-step", str(step),
                 "--disparity-lr", str(diff)])
    assert sorted(os.listdir(out)) == [f"{k:06d}_disparity.npy" for k in range(frames)]
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    cols, rows, _, _ = DR.lattice(cfg["width"], cfg["height"], step)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    for k in range(frames):
        batch.new_images([L[k].cuda()], [R[k].cuda()], [float(ts[k])])
        got = np.load(out / f"{k:06d}_disparity.npy")
        assert got.dtype == np.float32 and got.shape == (3, rows, cols)
        job = batch.export_disparity("frames", None, step=step, cost=True, lr_check=diff)
        assert got.tobytes() == np.ascontiguousarray(job.planes(0)).tobytes(), k
        assert got[2].tobytes() == np.ascontiguousarray(job.lr(0)).tobytes()
    batch.close()
    k = frames - 1
    win, sx, sy = cfg["window_size_depth_calculator"], cfg["search_x"], cfg["search_y"]
    fwd = DR.planes(L[k].numpy(), R[k].numpy(), win, sx, sy, step, DR.DISPARITY, True)
    lr = LR.lr_plane(L[k].numpy(), R[k].numpy(), win, sx, sy, step, fwd[0])
    want = LR.checked_planes(fwd, lr, DR.DISPARITY, True, max_lr_diff=diff)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    fails = LR.fails(lr, diff)
    assert fails.any() and not fails.all() and (got[0][fails] == -1).all()


def test_cloud_lr_drops_points(tmp_path):
    plain, checked = tmp_path / "plain", tmp_path / "checked"
    args = ["--synthetic", "tiny", "--frames", "2", "--cloud-step", "8"]
    replay.main(args + ["--dump-cloud", str(plain)])
    replay.main(args + ["--dump-cloud", str(checked), "--cloud-lr", "1.0"])
    assert sorted(os.listdir(plain)) == sorted(os.listdir(checked)) and os.listdir(plain)
    for name in os.listdir(plain):
        assert 0 < os.path.getsize(checked / name) < os.path.getsize(plain / name), name
