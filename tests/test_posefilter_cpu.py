"""The batched pose-filter updates without a GPU: the numpy restatement (tests/posefilter_cases.py) against the
oracle's update_pose bit for bit, the layout of svo_pose_sample in the C header, the Python dtype and the
restatement, the branches the crafted states reach, and the rejections that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py as O
import posefilter_cases as PC
from stereo_svo_slam_amd import hip_lib, stereo_slam, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = dict(pose_var=1000.0, speed_var=(100.0, 100.0, 100.0, 0.1, 0.1, 0.1))
FRAME = dict(pose_var=0.1, speed_var=1.0)


def _oracle():
    cfg = synth.CONFIGS["tiny"]
    return O.Slam(O.make_camera(**{k: cfg[k] for k in synth.CAMERA_FIELDS}))


@pytest.mark.parametrize("variances,dt,chain", [
    (APP, 1.0 / 104, True), (APP, 1.0 / 104, False), (APP, 0.05, True), (APP, 0.0, False),
    (FRAME, 0.0, False), (FRAME, 0.0, True), (FRAME, 1.0 / 104, False), (FRAME, 0.05, True)])
def test_restatement_equals_the_oracle(variances, dt, chain):
    """chains of 10 samples from a fresh filter: every filtered pose has the oracle's bits (the state feeds forward,
    so a difference anywhere in the filter shows in a later pose)"""
    rng = np.random.default_rng(int(dt * 1000) + 7 * chain + (3 if variances is APP else 0))
    slam, f = _oracle(), PC.Filter()
    pose = slam.pose()                                    # a fresh filter's pose: zeros
    assert not pose.any()
    for k in range(10):
        sm = PC.sample(pose=rng.uniform(-1, 1, 6).astype(np.float32), speed=rng.uniform(-1, 1, 6).astype(np.float32), dt=dt,
                       chain=chain, **variances)
        z = pose if chain else sm["pose"]
        want = slam.update_pose(z, sm["speed"], sm["pose_var"], sm["speed_var"], dt)
        pose = f.update(z, sm["speed"], sm["pose_var"], sm["speed_var"], dt)
        assert pose.tobytes() == want.tobytes(), k
    slam.close()


def test_run_chains_like_the_loop():
    """run() with CHAIN measures the previous filtered pose (first: the start pose), as the app's loop does"""
    rng = np.random.default_rng(5)
    samples = np.array([PC.app_sample(rng, chain=True) for _ in range(4)], PC.SAMPLE_DTYPE)
    start = rng.uniform(-1, 1, 6).astype(np.float32)
    out, filtered = PC.run(PC.fresh_state(), start, samples)
    slam = _oracle()
    pose = start
    for k, sm in enumerate(samples):
        pose = slam.update_pose(pose, sm["speed"], sm["pose_var"], sm["speed_var"], float(sm["dt"]))
        assert filtered[k].tobytes() == pose.tobytes()
    assert out[12:18].tobytes() == pose.tobytes() and out.shape == (PC.OUT_FLOATS,)
    slam.close()


def test_crafted_states_reach_the_branches():
    """the two launches of the GPU test take the skip branch of the solve, both signs of beta and several sweeps"""
    for name in ("first", "second"):
        cases, refs, trace = PC.reference(name)
        assert trace.skipped >= 3 and trace.beta_neg > 0 and trace.beta_pos > 0 and max(trace.sweeps) >= 5
        assert all((r is None) == (len(c[2]) == 0) for c, r in zip(cases, refs))
        for r in refs:
            assert r is None or (np.isfinite(r[0]).all() and np.isfinite(r[1]).all())
    assert [len(c[2]) for c in PC.reference("first")[0]] == [1, 0, 7, 3, 0, 2]
    assert [len(c[2]) for c in PC.reference("second")[0]] == [i % 5 for i in range(70)]
    # chained and unchained samples inside one slot
    flags = PC.reference("first")[0][2][2]["flags"]
    assert 0 < int((flags & PC.CHAIN).sum()) < len(flags)
    # the coupled covariance: symmetric, condition ~1e6
    cov = PC.coupled_state()[12:].reshape(12, 12).astype(np.float64)
    assert np.array_equal(cov, cov.T) and 1e5 < np.linalg.cond(cov) < 1e7


def test_sample_layout(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    names = [f[0] for f in PC.SAMPLE_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(svo_pose_sample));\n  printf("chain %d\\n", (int)SVO_POSE_SAMPLE_CHAIN);\n' +
                   "".join(f'  printf("{n} %zu\\n", offsetof(svo_pose_sample, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}
    assert c["size"] == 112 == hip_lib.POSE_SAMPLE_DTYPE.itemsize == PC.SAMPLE_BYTES == PC.SAMPLE_DTYPE.itemsize
    assert c["chain"] == hip_lib.POSE_SAMPLE_CHAIN == PC.CHAIN == 1
    assert stereo_slam.POSE_SAMPLE_DTYPE is hip_lib.POSE_SAMPLE_DTYPE
    for name, offset, kind, count in PC.SAMPLE_FIELDS:
        assert c[name] == offset, name
        for dtype in (hip_lib.POSE_SAMPLE_DTYPE, PC.SAMPLE_DTYPE):
            dt, off = dtype.fields[name][:2]
            assert off == offset and dt.base == np.dtype(kind) and int(np.prod(dt.shape, dtype=int)) == count, name
    assert set(hip_lib.POSE_SAMPLE_DTYPE.names) == set(names)
    assert (hip_lib.POSE_FILTER_IN_FLOATS, hip_lib.POSE_FILTER_OUT_FLOATS) == (PC.IN_FLOATS, PC.OUT_FLOATS) == (156, 456)


def test_gyro_samples_are_the_apps_loop():
    """StereoSlamBatch.gyro_samples: the app's variances, truncation and double 1.0 / 104, chained"""
    gyro = np.arange(15, dtype=np.float32).reshape(5, 3) * 3 - 10
    s = stereo_slam.StereoSlamBatch.gyro_samples(gyro, 1 / 30.0)
    assert len(s) == 3 == int(np.float32(104.0) * np.float32(1 / 30.0))           # min(samples, 104 * images_read / 30)
    assert len(stereo_slam.StereoSlamBatch.gyro_samples(gyro[:2], 1 / 30.0)) == 2
    assert len(stereo_slam.StereoSlamBatch.gyro_samples(gyro, 0.0)) == 0
    assert np.all(s["flags"] == 1) and np.all(s["dt"] == 1.0 / 104.0) and np.all(s["pose_var"] == 1000.0)
    assert np.array_equal(s["speed_var"][0], np.array([100, 100, 100, 0.1, 0.1, 0.1], np.float32))
    assert not s["speed"][:, :3].any()
    assert np.array_equal(s["speed"][:, 3:], (gyro[:3].astype(np.float64) / 180.0 * np.pi).astype(np.float32))


def test_rejections_without_a_device():
    lib = hip_lib.lib()
    invalid, no_device = -1, -3                            # SVO_ERR_INVALID, SVO_ERR_NO_DEVICE
    counts = (C.c_int * 1)(1)
    sample = np.zeros(1, hip_lib.POSE_SAMPLE_DTYPE)
    out = np.full(6, 7, np.float32)
    for fn in (lib.svo_submit_pose_updates, lib.svo_update_poses):
        assert fn(None, None, counts, 1, sample.ctypes.data, out.ctypes.data) == invalid
        assert b"svo_submit_pose_updates" in lib.svo_last_error()
    assert np.all(out == 7)
    assert lib.svo_pose_filter_batch(None, 0, None, None, None, 0, None, None, None) == invalid
    import torch
    if not torch.cuda.is_available():                      # (as every entry that needs the GPU does here)
        h = C.c_void_p()
        assert lib.svo_handle_create(0, 64, C.byref(h)) == no_device
