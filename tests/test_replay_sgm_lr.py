"""replay --dump-disparity --disparity-sgm --disparity-lr and --dump-cloud --cloud-sgm [--cloud-lr]: the stacked file
holds value, aggregated cost and lr of the checked SGM job of the same frame and of the numpy statement
(tests/sgm_lr_ref.py), bit for bit; the PLYs hold the vertices of the SGM cloud job of a twin tracker."""
import os

import numpy as np
import pytest

import dense_ref as DR
import lr_ref as LR
import sgm_lr_ref as SLR
from stereo_svo_slam_amd import replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu

P1, P2, CAP = 16, 128, 2047


def test_disparity_sgm_lr_stacks_three_planes(tmp_path):
    frames, step, diff = 2, 16, 1.0
    out = tmp_path / "disp"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-disparity", str(out), "--disparity-step", str(step),
                 "--disparity-sgm", f"{P1},{P2},{CAP}", "--disparity-lr", str(diff)])
    assert sorted(os.listdir(out)) == [f"{k:06d}_disparity.npy" for k in range(frames)]
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    cols, rows, _, _ = DR.lattice(cfg["width"], cfg["height"], step)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    for k in range(frames):
        batch.new_images([L[k].cuda()], [R[k].cuda()], [float(ts[k])])
        got = np.load(out / f"{k:06d}_disparity.npy")
        assert got.dtype == np.float32 and got.shape == (3, rows, cols)
        job = batch.export_disparity("frames", None, step=step, cost=True, sgm=dict(p1=P1, p2=P2, cost_cap=CAP, lr_check=diff))
        assert got.tobytes() == np.ascontiguousarray(job.planes(0)).tobytes(), k
        assert got[2].tobytes() == np.ascontiguousarray(job.lr(0)).tobytes()
    batch.close()
    win, sx, sy = cfg["window_size_depth_calculator"], cfg["search_x"], cfg["search_y"]
    want = SLR.checked_planes(L[-1].numpy(), R[-1].numpy(), win, sx, sy, step, P1, P2, CAP, max_lr_diff=diff, fast=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    fails = LR.fails(want[2], diff)
    assert not fails.all() and (got[0][fails] == -1).all()
    # tolerance 0 only reports
    report = tmp_path / "report"
    replay.main(["--synthetic", "tiny", "--frames", "1", "--dump-disparity", str(report), "--disparity-step", str(step),
                 "--disparity-sgm", f"{P1},{P2},{CAP}", "--disparity-lr", "0"])
    want = SLR.checked_planes(L[0].numpy(), R[0].numpy(), win, sx, sy, step, P1, P2, CAP, max_lr_diff=0.0, fast=True)
    assert np.array_equal(np.load(report / "000000_disparity.npy").view(np.uint32), want.view(np.uint32))


def test_cloud_sgm_writes_the_jobs_vertices(tmp_path):
    frames, step = 2, 8
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    for lr in (None, 1.0):
        out = tmp_path / f"cloud{lr}"
        replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-cloud", str(out), "--cloud-step", str(step),
                     "--cloud-sgm", f"{P1},{P2},{CAP}"] + ([] if lr is None else ["--cloud-lr", str(lr)]))
        names = sorted(os.listdir(out))
        assert names and names[0] == "kf000000_cloud.ply"
        batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
        batch.new_images([L[0].cuda()], [R[0].cuda()], [float(ts[0])])
        job = batch.export_cloud("last_keyframes", None, step=step, sgm=dict(p1=P1, p2=P2, cost_cap=CAP, lr_check=lr))
        want = job.points(0)
        got = replay.read_ply(out / "kf000000_cloud.ply")
        assert len(got) == len(want) > 0
        for k in ("x", "y", "z"):
            assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (lr, k)
        batch.close()
