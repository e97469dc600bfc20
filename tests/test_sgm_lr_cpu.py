"""The cross-check of SGM maps without a GPU: the two formulations of tests/sgm_lr_ref.py agree, the check does what it
is for on the occlusion scene, the crafted cases of tests/sgm_lr_cases.py reach what they were made for, the SGM form of
max_mean_cost both drops and keeps, and the Python surface parses the sgm dict's lr_check.

One thing the cases cannot reach: lr = -2 by an invalid reverse point under a valid forward point. A point is invalid by
its row (the same row for both maps) or by x11 >= W - 1, which needs window 1 and the pixel x' = W - 1; the looked-up
cell has x' <= (W - 1 - xr) + step / 2 <= W - 2, because xr >= x + 1 and x >= step / 2. The branch is kept (a caller's
own planes may hold anything) and is tested here on planes made by hand."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import lr_ref as LR
import sgm_lr_cases as LC
import sgm_lr_ref as SLR
import sgm_ref as SR
from stereo_svo_slam_amd import hip_lib, jobs

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_two_formulations_agree(name):
    left, step = LC.cases()[name][0], LC.cases()[name][5]
    fwd, rev = LC.forward(name)[0], LC.reverse(name)
    want = SLR.lr_plane(fwd, rev, left.shape[1], step)
    assert want.dtype == F and np.array_equal(want.view(np.uint32), LC.reference(name).view(np.uint32))


def test_small_case_from_the_first_formulation_of_sgm():
    """the whole statement point by point (sgm_ref's first formulation too) on the smallest case, both values"""
    left, right, win, sx, sy, step, p1, p2, cap = LC.cases()["thin"]
    for value, diff in ((SR.DISPARITY, 0.0), (SR.DEPTH, 1.0)):
        slow = SLR.checked_planes(left, right, win, sx, sy, step, p1, p2, cap, True, value, True, 17.5, diff, fast=False)
        fast = SLR.checked_planes(left, right, win, sx, sy, step, p1, p2, cap, True, value, True, 17.5, diff, fast=True)
        assert slow.shape == (3, 12, 40) and np.array_equal(slow.view(np.uint32), fast.view(np.uint32))


def test_invalid_reverse_point_by_hand():
    fwd = np.array([[1.0, 2.25, -1.0, 0.5]], F)
    rev = np.array([[-1.0, 2.0, -1.0, 3.0]], F)            # W = 4, step 1: x = 0 -> xr 1 -> cell 2 (invalid); x = 1 -> xr 3 -> cell 0 (invalid)
    want = np.array([[-2.0, -2.0, -1.0, -2.0]], F)         # x = 3 -> xr 4 > W - 1
    assert np.array_equal(SLR.lr_plane(fwd, rev, 4, 1), want) and np.array_equal(SLR.lr_plane_fast(fwd, rev, 4, 1), want)
    rev[0, 2] = 1.5
    assert SLR.lr_plane(fwd, rev, 4, 1)[0, 0] == F(0.5) == SLR.lr_plane_fast(fwd, rev, 4, 1)[0, 0]


def _shares(seed, step):
    name = f"occl{seed}s{step}"
    s = LC.SCENE
    truth = LC.occlusion_scene(seed)[2]
    cols, rows = s["w"] // step, s["h"] // step
    xs, ys = np.arange(cols) * step + step // 2, np.arange(rows) * step + step // 2
    t = truth[ys][:, xs]
    fwd = LC.forward(name)[0]
    fails = LR.fails(LC.reference(name), 1.0)
    valid = fwd >= 0
    wrong = valid & (np.abs(fwd - t) > 1.0)
    band = np.zeros_like(valid)
    band[np.ix_((ys >= s["y0"]) & (ys < s["y1"]), (xs >= s["b"]) & (xs < s["b"] + s["dfg"] - s["dbg"]))] = True
    good = valid & ~wrong & ~band
    return float(fails[wrong].mean()), float(fails[good].mean()), int(wrong.sum()), int(good.sum())


@pytest.mark.parametrize("step", LC.STEPS)
@pytest.mark.parametrize("seed", LC.SEEDS)
def test_what_the_check_is_for(seed, step):
    """of the valid points more than 1 px from the truth at least 0.75 fail at tolerance 1; of those within 1 px and
    outside the half-occluded band at most 0.08. Measured with this reference: 0.81 - 0.93 and 0.029 - 0.050"""
    wrong_fail, good_fail, n_wrong, n_good = _shares(seed, step)
    print(f"seed {seed} step {step}: {wrong_fail:.3f} of {n_wrong} wrong points fail, {good_fail:.3f} of {n_good} good points")
    assert n_wrong > 0 and n_good > 0
    assert wrong_fail >= 0.75
    assert good_fail <= 0.08


def test_cases_reach_what_they_are_for():
    seen = set()
    for name in sorted(LC.cases()):
        lr = LC.reference(name)
        left, step = LC.cases()[name][0], LC.cases()[name][5]
        w = left.shape[1]
        fwd = LC.forward(name)[0]
        assert ((lr >= 0) | (lr == LR.INVALID) | (lr == LR.NO_WAY_BACK)).all(), name
        assert ((lr == LR.INVALID) == (fwd < 0)).all(), name
        xs = (np.arange(fwd.shape[1]) * step + step // 2)[None, :]
        xr = xs + (np.maximum(fwd, 0).astype(F) + F(0.5)).astype(np.int32)
        outside = (fwd >= 0) & (xr > w - 1)
        assert (lr[outside] == LR.NO_WAY_BACK).all() and (lr[(fwd >= 0) & ~outside] >= 0).all(), name   # (the docstring's proof)
        seen |= {k for k, m in (("-1", lr == -1), ("outside", outside), ("0", lr == 0), (">1", lr > 1), ("j0 = 0", fwd == F(0.5))) if m.any()}
    assert seen == {"-1", "outside", "0", ">1", "j0 = 0"}
    # the clamp: step 8, W % 8 == 7, a valid point at ix = 0 whose matched column lies beyond the mirrored lattice's last cell
    left, _, _, _, _, step, *_ = LC.cases()["clamp"]
    w, cols = left.shape[1], left.shape[1] // step
    assert step == 8 and w % 8 == 7
    d = LC.forward("clamp")[0][:, 0]
    xr = np.array([LR.matched_column(step // 2, v) for v in d])
    reached = (d >= 0) & (w - 1 - xr >= cols * step)
    assert reached.any() and all(SLR.mirrored_cell(w, step, cols, int(v)) == cols - 1 for v in xr[reached])
    assert (LC.reference("clamp")[:, 0][reached] >= 0).all()
    # j0 = 0: disp = 0.5 is matched to xr = x + 1
    assert LR.matched_column(7, F(0.5)) == 8
    thin = LC.forward("thin")[0]
    assert (thin[:, -1] == -1).all() and (thin[-1, :] == -1).all() and (thin[:-1, :16] == F(0.5)).mean() > 0.9


def test_max_mean_cost_of_sgm_planes_drops_and_keeps():
    """best > max_mean_cost * 4.0f, restated here, against sgm_lr_ref.cloud: both outcomes in one case, and another kept
    set than the template-area rule of cloud_ref gives"""
    name = "occl3s4"
    left, right, win, sx, sy, step, *_ = LC.cases()[name]
    planes = LC.forward(name)
    bound = float(np.median(planes[1][planes[1] >= 0])) / 4.0
    rig = dict(fx=90.0, fy=91.0, cx=48.0, cy=20.0, baseline=0.12)
    want = (planes[0] >= 0) & ~(planes[1].astype(F) > F(bound) * F(4.0))
    assert 0 < int(want.sum()) < int((planes[0] >= 0).sum())
    recs, n = SLR.cloud(left, planes, step, rig, np.zeros(6, F), CR.CAMERA, CR.ORGANIZED, max_mean_cost=bound)
    assert n == int(want.sum()) and np.array_equal((recs["flags"] == 0).reshape(want.shape), want)
    area = CR.kept_mask(planes, left.shape[1], left.shape[0], win, step, np.zeros_like(planes[0]), max_mean_cost=bound)
    assert not np.array_equal(area, want)
    masked = SLR.masked(planes, LC.reference(name), 1.0)
    assert (masked[0] < 0).sum() > (planes[0] < 0).sum() and np.array_equal(masked[1], planes[1])


def test_python_surface():
    p, check = hip_lib.sgm_job(dict(hip_lib.SGM_DEFAULTS, lr_check=1.0))
    assert isinstance(p, hip_lib.SgmParams) and (p.paths, p.p1, p.p2, p.cost_cap, p.subpixel) == (4, 64, 256, 4095, 1)
    assert isinstance(check, hip_lib.StereoCheck) and (check.lr, check.max_lr_diff) == (1, 1.0)
    assert hip_lib.sgm_job(dict(p1=32, p2=256, cost_cap=4095, lr_check=True))[1].max_lr_diff == 0.0
    for spec in (True, dict(p1=32, p2=256, cost_cap=4095), dict(hip_lib.SGM_DEFAULTS, lr_check=None), dict(hip_lib.SGM_DEFAULTS, lr_check=False), p):
        got, none = hip_lib.sgm_job(spec)
        assert isinstance(got, hip_lib.SgmParams) and none is None
    assert hip_lib.sgm_job(None) == (None, None) == hip_lib.sgm_job(False)
    assert "lr_check" not in hip_lib.SGM_DEFAULTS

    class Slam:                                            # what a job reads of its ctx before it checks the combination
        n = 2

    top = hip_lib.stereo_check(True, 1.0)
    for job in (jobs.Disparities, jobs.Clouds):
        with pytest.raises(ValueError, match="lr_check key of its sgm dict"):
            job(Slam(), 0, None, None, False, top, p, None)
    for sym in ("svo_submit_export_disparity_sgm_checked", "svo_export_disparity_sgm_checked", "svo_dense_disparity_sgm_checked",
                "svo_submit_export_cloud_sgm", "svo_export_cloud_sgm", "svo_cloud_points_sgm"):
        assert sym in hip_lib.SYMBOLS
        getattr(hip_lib.lib(), sym)


def test_header_declares_the_entries(tmp_path):
    """the new prototypes compile as C and take the arguments the Python layer passes"""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header"
    src = tmp_path / "protos.c"
    src.write_text('#include "svo_hip.h"\n'
                   "int (*a)(svo_handle *, int, const svo_dense_src *, const int64_t *, const svo_disparity_style *, const svo_sgm_params *,\n"
                   "         const svo_stereo_check *, float *) = svo_dense_disparity_sgm_checked;\n"
                   "int (*b)(svo_handle *, int, const svo_cloud_src *, const int64_t *, const svo_cloud_style *, const svo_sgm_params *,\n"
                   "         const svo_stereo_check *, svo_map_point *, int32_t *) = svo_cloud_points_sgm;\n"
                   "int (*c)(svo_ctx *, int, const int *, int, const svo_disparity_style *, const svo_sgm_params *, const svo_stereo_check *,\n"
                   "         const svo_disparity_dst *, int) = svo_submit_export_disparity_sgm_checked;\n"
                   "int (*d)(svo_ctx *, int, const int *, int, const svo_cloud_style *, const svo_sgm_params *, const svo_stereo_check *,\n"
                   "         const svo_cloud_dst *, int) = svo_export_cloud_sgm;\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "protos.o")])
    assert C.sizeof(hip_lib.StereoCheck) == 32
