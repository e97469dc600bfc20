"""The SGM forms of the cloud's consumers without a GPU: what they are for, measured on the references
alone (tests/sgm_consumer_cases.py), and the Python surface: how sgm= travels from the keyword and the dicts to the job
objects, the ValueErrors, and the six symbols of the built library."""
import ctypes as C

import numpy as np
import pytest
import torch

import sgm_consumer_cases as SC
from stereo_svo_slam_amd import hip_lib, jobs, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch


# ------------------------------------------------------------------ (1) what it is for
@pytest.fixture(scope="module")
def measured():
    """per seed: the disparity errors of the two maps and, per voxel edge, the fused depth errors"""
    out = {}
    for seed in SC.SEEDS:
        left, right = SC.plane_pair(seed)
        wta, sgm = SC.planes(left, right)
        a, b = SC.clouds(left, wta, sgm)
        out[seed] = (SC.disparity_error(wta[0]), SC.disparity_error(sgm[0]),
                     {v: (SC.fused_depth_error(a, v), SC.fused_depth_error(b, v)) for v in SC.VOXELS})
    return out


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_sgm_depth_fuses_into_a_map_five_times_closer_to_the_plane(measured, seed):
    """Measured with the references: the winner-takes-all disparity is off by 0.260 px in the mean (0.46 of its points
    within 0.25 px), the sub-pixel SGM disparity by 0.048 - 0.051 px (all within 0.25 px); the RMS depth error of the
    fused voxel points is 0.345 against 0.065 - 0.067, a ratio of 0.189 - 0.195, over 154 - 156 points per map."""
    (wta_err, wta_near), (sgm_err, sgm_near), fused = measured[seed]
    print(f"seed {seed}: disparity error winner-takes-all {wta_err:.3f} ({wta_near:.2f} within 0.25), SGM {sgm_err:.3f} ({sgm_near:.2f})")
    assert sgm_err <= 0.10 and wta_err >= 0.20
    for voxel, ((wta_rms, wta_n), (sgm_rms, sgm_n)) in fused.items():
        print(f"  voxel {voxel}: RMS depth error {wta_rms:.3f} ({wta_n} points) against {sgm_rms:.3f} ({sgm_n}): {sgm_rms / wta_rms:.3f}")
        assert sgm_rms / wta_rms <= 0.30, (voxel, sgm_rms, wta_rms)
        assert wta_n >= 150 and sgm_n >= 150, (voxel, wta_n, sgm_n)


def test_the_generator_is_the_stated_one():
    left, right = SC.plane_pair(3)
    again = SC.plane_pair(3)
    assert left.shape == right.shape == (SC.H, SC.W) and left.dtype == np.uint8
    assert left.tobytes() == again[0].tobytes() and right.tobytes() == again[1].tobytes()
    assert SC.plane_pair(4)[0].tobytes() != left.tobytes()
    assert SC.K == (SC.D1 - SC.D0) / SC.W and SC.D0 + SC.K * SC.W == SC.D1


# ------------------------------------------------------------------ (2) the Python surface
PARAMS = dict(p1=32, p2=200, cost_cap=1000, subpixel=False)


def _fields(p):
    return (p.paths, p.p1, p.p2, p.cost_cap, p.subpixel)


def _as_sgm_job(sgm, got_params, got_check):
    """what a consumer carries is what hip_lib.sgm_job parses"""
    want_params, want_check = hip_lib.sgm_job(sgm)
    assert (got_params is None) == (want_params is None)
    if want_params is not None:
        assert _fields(got_params) == _fields(want_params)
    want = (0, 0.0) if want_check is None else (want_check.lr, want_check.max_lr_diff)
    assert (got_check.lr, got_check.max_lr_diff) == want


SGM_FORMS = (True, hip_lib.sgm_params(32, 200, 1000), dict(PARAMS), dict(PARAMS, lr_check=1.5), dict(hip_lib.SGM_DEFAULTS, lr_check=None))


@pytest.mark.parametrize("sgm", SGM_FORMS)
def test_scene_clouds_and_ar_occlusion_hand_the_params_on(sgm):
    clouds, keep = hip_lib.scene_clouds(live=True, step=4, sgm=sgm)
    _as_sgm_job(sgm, clouds.sgm, clouds.check)
    occlusion = hip_lib.ar_occlusion(step=4, sgm=sgm)
    _as_sgm_job(sgm, occlusion.sgm, occlusion.check)
    # without a live layer the check stays off, as it does without sgm
    clouds, keep = hip_lib.scene_clouds(live=False, sgm=sgm)
    assert clouds.sgm is not None and (clouds.check.lr, clouds.check.max_lr_diff) == (0, 0.0)


def test_without_sgm_nothing_changes():
    for sgm in (None, False):
        clouds, _ = hip_lib.scene_clouds(live=True, step=4, lr_check=1.5, sgm=sgm)
        occlusion = hip_lib.ar_occlusion(step=4, lr_check=1.5, sgm=sgm)
        assert clouds.sgm is None and occlusion.sgm is None
        assert (clouds.check.lr, clouds.check.max_lr_diff, occlusion.check.lr, occlusion.check.max_lr_diff) == (1, 1.5, 1, 1.5)
    assert bytes(hip_lib.scene_clouds(live=True, step=4, lr_check=1.5)[0]) == bytes(hip_lib.scene_clouds(live=True, step=4, lr_check=1.5, sgm=None)[0])
    assert bytes(hip_lib.ar_occlusion(lr_check=1.5)) == bytes(hip_lib.ar_occlusion(lr_check=1.5, sgm=None))
    assert hip_lib.SceneClouds().sgm is None and hip_lib.ArOcclusion().sgm is None


def test_a_sibling_lr_check_beside_sgm_is_refused():
    with pytest.raises(ValueError, match="dense: .*sgm dict"):
        hip_lib.scene_clouds(live=True, lr_check=1.0, sgm=True)
    with pytest.raises(ValueError, match="occlusion: .*sgm dict"):
        hip_lib.ar_occlusion(lr_check=1.0, sgm=dict(PARAMS))
    with pytest.raises(ValueError, match="submit_fuse: .*sgm dict"):
        hip_lib.sgm_consumer(True, 1.0, "submit_fuse")
    assert hip_lib.sgm_consumer(None, 1.0, "submit_fuse") == (None, None)
    with pytest.raises(TypeError):
        hip_lib.scene_clouds(live=True, sgm=dict(PARAMS, paths=8))          # (sgm_params takes no such key)


class _Slam:
    """what the job objects read of a StereoSlamBatch before anything is submitted"""
    n, device = 3, "cpu"
    width, height = synth.CONFIGS["tiny"]["width"], synth.CONFIGS["tiny"]["height"]
    cam = hip_lib.CameraSettings.from_dict(synth.CONFIGS["tiny"])


@pytest.fixture()
def unpinned(monkeypatch):
    """the jobs' buffers in plain host memory: nothing here is submitted"""
    monkeypatch.setattr(jobs.Job, "_alloc", lambda self, shape, dtype, make=torch.zeros: make(shape, dtype=dtype))


@pytest.mark.parametrize("sgm", SGM_FORMS)
def test_the_job_objects_keep_the_params(unpinned, sgm):
    slam = _Slam()
    params, check = hip_lib.sgm_job(sgm)
    style = hip_lib.cloud_style(4)
    fuse = jobs.Fusion(slam, 1, None, style, None, 7, params, check)
    _as_sgm_job(sgm, fuse.sgm, fuse.check if fuse.check is not None else hip_lib.StereoCheck())
    scene = jobs.Scenes(slam, None, hip_lib.scene_style(cols=32, rows=16), hip_lib.scene_preset("front", 32, 16), False,
                        dict(step=4, sgm=sgm))
    _as_sgm_job(sgm, scene.sgm, scene._clouds[0].check)
    box = hip_lib.ar_box(1.0)
    inst = [(hip_lib.ar_model((0.0, 0.0, 4.0)), 0, 0xffffff)]
    for occlusion in (dict(step=4, sgm=sgm), hip_lib.ar_occlusion(step=4, sgm=sgm)):
        ar = jobs.ArPictures(slam, None, hip_lib.ar_style(), [box], inst, None, False, occlusion)
        _as_sgm_job(sgm, ar.sgm, ar._occlusion.check)
    # and without sgm the jobs are the ones they were
    assert jobs.Fusion(slam, 1, None, style, hip_lib.stereo_check(True, 1.0), 7).sgm is None
    assert jobs.Scenes(slam, None, hip_lib.scene_style(cols=32, rows=16), hip_lib.scene_preset("front", 32, 16), False, dict(step=4)).sgm is None
    assert jobs.ArPictures(slam, None, hip_lib.ar_style(), [box], inst, None, False, dict(step=4)).sgm is None


def test_the_job_objects_refuse_both_checks(unpinned):
    slam = _Slam()
    with pytest.raises(ValueError, match="sgm dict"):
        jobs.Fusion(slam, 1, None, hip_lib.cloud_style(4), hip_lib.stereo_check(True, 1.0), 7, hip_lib.sgm_params(32, 200, 1000))
    with pytest.raises(ValueError, match="dense: .*sgm dict"):
        jobs.Scenes(slam, None, hip_lib.scene_style(cols=32, rows=16), hip_lib.scene_preset("front", 32, 16), False,
                    dict(step=4, lr_check=1.0, sgm=True))
    with pytest.raises(ValueError, match="occlusion: .*sgm dict"):
        jobs.ArPictures(slam, None, hip_lib.ar_style(), [hip_lib.ar_box(1.0)], [], None, False, dict(lr_check=1.0, sgm=True))


def test_submit_fuse_parses_sgm_and_refuses_a_top_level_lr_check(monkeypatch):
    made = []
    monkeypatch.setattr(jobs.Fusion, "submit", lambda self: made.append(self) or self)
    batch = object.__new__(StereoSlamBatch)
    batch.n, batch._fuse_stamp = 2, 0
    job = batch.submit_fuse("frames", [1], sgm=dict(PARAMS, lr_check=2.0), step=8)
    assert made == [job] and _fields(job.sgm) == (4, 32, 200, 1000, 0) and (job.check.lr, job.check.max_lr_diff) == (1, 2.0)
    assert (job.what, job.stamp, job.style.step) == (0, 1, 8)
    assert batch.submit_fuse(sgm=True).check is None and _fields(made[-1].sgm) == _fields(hip_lib.sgm_job(True)[0])
    plain = batch.submit_fuse(lr_check=1.5)
    assert plain.sgm is None and (plain.check.lr, plain.check.max_lr_diff) == (1, 1.5)
    with pytest.raises(ValueError, match="submit_fuse: .*sgm dict"):
        batch.submit_fuse(lr_check=1.5, sgm=True)
    assert batch._fuse_stamp == 3                                          # (the refused call took no stamp)


ENTRIES = {"svo_submit_fuse_clouds_sgm": 9, "svo_fuse_clouds_sgm": 9, "svo_submit_export_scenes_clouds_sgm": 9,
           "svo_export_scenes_clouds_sgm": 9, "svo_submit_export_ar_occluded_sgm": 13, "svo_export_ar_occluded_sgm": 13}


def test_the_library_exports_the_six_entries():
    lib = hip_lib.lib()
    for name, n_args in ENTRIES.items():
        assert name in hip_lib.SYMBOLS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args, name
    # a NULL ctx is answered, not followed: the entries check their arguments like the ones they extend
    p = hip_lib.sgm_params(32, 200, 1000)
    info = np.zeros(1, hip_lib.FUSE_INFO_DTYPE)
    style = hip_lib.cloud_style(4)
    assert lib.svo_submit_fuse_clouds_sgm(None, 0, None, 0, C.byref(style), C.byref(p), None, 1, info.ctypes.data) == -1
    assert b"svo_submit_fuse_clouds_sgm" in lib.svo_last_error()
    assert lib.svo_submit_fuse_clouds_sgm(None, 0, None, 0, C.byref(style), None, None, 1, info.ctypes.data) == -1
    assert b"svo_submit_fuse_clouds:" in lib.svo_last_error()               # (sgm == NULL is the existing entry)
    bad = hip_lib.sgm_params(32, 200, 1000)
    bad.paths = 8
    assert lib.svo_submit_export_scenes_clouds_sgm(None, None, 0, None, None, C.byref(bad), None, None, 0) == -1
    assert b"svo_submit_export_scenes_clouds_sgm" in lib.svo_last_error()
