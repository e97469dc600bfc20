"""The sequence of the C++ facade tests and the oracle's run over it: the `tiny` preset (320x240), 14 frames,
motion_scale 4, with the app's IMU loop (SlamApp::update_pose_from_imu: three gyro samples through update_pose,
variances 1000 / (100, 100, 100, 0.1, 0.1, 0.1), dt = 1/104) after some of the frames. test_facade_cpu.py pins the
seed from the oracle alone; test_facade_gpu.py plays the same frames through hostcpp/ and compares."""
import functools
import math

import numpy as np

import ingest_ref as IR
import oracle_py as O
from stereo_svo_slam_amd import synth
import util

PRESET, FRAMES, MOTION = "tiny", 14, 4.0
# the first seed at which the oracle makes at least three keyframes (seeds 0 .. 25 give one or two in 14 frames) and a
# later frame holds live keypoints of two keyframe ids
# (test_facade_cpu.py::test_the_sequence_reaches_three_keyframes_and_mixed_frames)
SEED = 26
IMU_AFTER = (1, 4, 5, 9)                  # frames followed by an IMU loop of three samples
POSE_VAR = np.full(6, 1000.0, np.float32)
SPEED_VAR = np.array([100.0, 100.0, 100.0, 0.1, 0.1, 0.1], np.float32)
DT = 1.0 / 104.0

# one record of <dir>/samples.bin as tests/cpp/facade_sequence.cpp reads it (88 bytes, packed)
SAMPLE_FILE_DTYPE = np.dtype([("after_frame", "<i4"), ("first", "<i4"), ("speed", "<f4", (6,)), ("pose_var", "<f4", (6,)),
                              ("speed_var", "<f4", (6,)), ("dt", "<f8")])
assert SAMPLE_FILE_DTYPE.itemsize == 88

GRAY_MODES = ("pair", "fast", "fast_late")
COLOUR_MODES = ("sbs", "econ", "bgr")
FORMAT_OF = {"sbs": "sbs_gray", "econ": "ch3_econ", "bgr": "bgr_pair"}


@functools.lru_cache(maxsize=None)
def sequence(seed=SEED, n_frames=FRAMES):
    """(cfg, lefts [n, H, W], rights, time stamps) rendered on the CPU; shared, read-only"""
    cfg, L, R, poses, ts = synth.make_sequence(PRESET, n_frames, seed, device="cpu", motion_scale=MOTION)
    L, R = np.stack([x.numpy() for x in L]), np.stack([x.numpy() for x in R])
    L.setflags(write=False); R.setflags(write=False)
    return cfg, L, R, [float(t) for t in ts]


@functools.lru_cache(maxsize=None)
def colour_frames(seed=SEED, n_frames=FRAMES):
    """genuinely coloured left / right frames [n, H, W, 3] (B, G, R) of the sequence, as test_ingest_gpu.py makes them"""
    cfg, L, R, ts = sequence(seed, n_frames)
    lc = np.stack([IR.colourize(L[k], 2 * k) for k in range(n_frames)])
    rc = np.stack([IR.colourize(R[k], 2 * k + 1) for k in range(n_frames)])
    lc.setflags(write=False); rc.setflags(write=False)
    return lc, rc


def buffers(mode, k, seed=SEED, n_frames=FRAMES):
    """the buffers (a, b) of frame k as the program's mode takes them; b is None for the one-buffer modes"""
    cfg, L, R, ts = sequence(seed, n_frames)
    if mode in GRAY_MODES:
        return L[k], R[k]
    lc, rc = colour_frames(seed, n_frames)
    return IR.pack(FORMAT_OF[mode], lc[k], rc[k])


def gray_frames(mode, k, seed=SEED, n_frames=FRAMES):
    """the (left, right) 8-bit images that the tracker has to see of frame k: the statement of tests/ingest_ref.py"""
    a, b = buffers(mode, k, seed, n_frames)
    if mode in GRAY_MODES:
        return a, b
    return IR.convert(FORMAT_OF[mode], a, b)


@functools.lru_cache(maxsize=None)
def imu_samples():
    """the samples of every IMU loop, in order: SAMPLE_FILE_DTYPE records"""
    rng = np.random.default_rng(2024)
    out = np.zeros(3 * len(IMU_AFTER), SAMPLE_FILE_DTYPE)
    for i, rec in enumerate(out):
        rec["after_frame"], rec["first"] = IMU_AFTER[i // 3], 1 if i % 3 == 0 else 0
        rec["speed"][3:] = (rng.uniform(-40, 40, 3) / 180.0 * math.pi).astype(np.float32)
        rec["pose_var"], rec["speed_var"], rec["dt"] = POSE_VAR, SPEED_VAR, DT
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(colour=False, seed=SEED, n_frames=FRAMES, imu=True):
    """oracle_py.Slam over the sequence (colour: over the gray images of the coloured frames; the three colour modes
    carry the same ones). Per frame a dict(made, kps2d, kps3d, info, pose, n_keyframes, updates [m, 6]); then the
    keyframes (kps2d, kps3d, info, pose) and the trajectory, which is the pose of every frame. Shared: leave unchanged."""
    cfg, L, R, ts = sequence(seed, n_frames)
    ref = O.Slam(util.oracle_camera(cfg))
    samples = imu_samples() if imu else imu_samples()[:0]
    frames = []
    for k in range(n_frames):
        left, right = gray_frames("sbs" if colour else "pair", k, seed, n_frames)
        made = ref.new_image(left, right, ts[k])
        k2, k3, info = ref.keypoints()
        pose = ref.pose().copy()
        updates, prev = [], pose
        for sm in samples[samples["after_frame"] == k]:
            prev = ref.update_pose(pose if sm["first"] else prev, sm["speed"], sm["pose_var"], sm["speed_var"], float(sm["dt"]))
            updates.append(prev)
        frames.append(dict(made=made, kps2d=k2, kps3d=k3, info=info, pose=pose, n_keyframes=ref.num_keyframes(),
                           updates=np.array(updates, np.float32).reshape(-1, 6)))
    keyframes = [ref.keyframe(kid) for kid in range(ref.num_keyframes())]
    ref.close()
    return frames, keyframes, np.stack([f["pose"] for f in frames])


def stage_frame(frames):
    """the frame the stage classes run on: the one after the first frame that holds keypoints of two keyframes"""
    return mixed_frames(frames)[0] + 1


def mixed_frames(frames):
    """frames (index >= 1) whose live keypoints (not ignore_completely) come from two or more keyframe ids"""
    out = []
    for k, f in enumerate(frames):
        live = f["info"]["ignore_completely"] == 0
        if k >= 1 and len(np.unique(f["info"]["keyframe_id"][live])) >= 2:
            out.append(k)
    return out
