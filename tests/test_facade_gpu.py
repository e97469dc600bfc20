"""The C++ facade classes with the reference's names (hostcpp/: StereoSlam, PoseEstimator,
project_keypoints, PoseRefiner + OpticalFlow, DepthFilter; reference:
src/include/pose_estimator.hpp:19-27, pose_refinement.hpp:22-32, optical_flow.hpp:26-30,
depth_filter.hpp:14-20) built with g++ against libsvo_hip.so and run on the GPU; their results
must equal, bit for bit, what the ctypes binding gets from the same C entry points; and StereoSlam itself over a
whole sequence (tests/facade_cases.py), in every way frames can be handed to it, against oracle_py.Slam."""
import ctypes as C
import os
import shutil
import subprocess
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import KP_INFO_DTYPE, StereoSlam
import facade_cases as FC
import oracle_py as O
import size_cases
import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-svo-slam_amd", "csrc")


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    gxx = shutil.which("g++")
    assert gxx
    subprocess.check_call([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-o", exe, "-L" + CSRC, "-lsvo_hip", "-Wl,-rpath," + CSRC,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_facade_smoke_runs_on_the_gpu(tmp_path):
    exe = _build(tmp_path, "facade_smoke")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "keypoints" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("exact", [False, True])
def test_facade_stage_classes_equal_the_ctypes_path(tmp_path, exact):
    _stage_classes_on_two_frames(tmp_path, exact, *synth.make_sequence("tiny", 2, 0, device="cpu"))


@pytest.mark.parametrize("exact", [False, True])
def test_facade_stage_classes_at_an_odd_size(tmp_path, exact):
    """the same comparison at the smallest odd case of tests/size_cases.py (61x47, two alignment levels, one LK
    level): make_stereo_image's floor and ceil halvings differ, and opt_flow is cut to the levels the LK pyramid has"""
    name = min((n for n, c in size_cases.CASES.items() if size_cases.config(n)["width"] % 2 and size_cases.config(n)["height"] % 2),
               key=lambda n: size_cases.config(n)["width"] * size_cases.config(n)["height"])
    c = size_cases.CASES[name]
    cfg, L, R, poses, ts = synth.make_sequence(c["preset"], 2, c["seed"], device="cpu", motion_scale=c["motion"],
                                               overrides=c["overrides"])
    assert name == "lk1_61" and (cfg["width"], cfg["height"]) == (61, 47)
    lk_levels = _stage_classes_on_two_frames(tmp_path, exact, cfg, L, R, poses, ts)
    assert lk_levels == 1                                            # (SVO_LK_LEVELS is 3)
    assert size_cases.floor_dims(cfg)[1] != size_cases.ceil_dims(cfg, 2)[1]


def _stage_classes_on_two_frames(tmp_path, exact, cfg, L, R, poses, ts):
    L = [x.numpy() for x in L]
    R = [x.numpy() for x in R]
    w, h = cfg["width"], cfg["height"]
    cam = hip_lib.CameraSettings.from_dict(cfg)
    for name, img in (("l0", L[0]), ("r0", R[0]), ("l1", L[1]), ("r1", R[1])):
        img.tofile(str(tmp_path / (name + ".raw")))
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(bytes(cam))
    exe = _build(tmp_path, "facade_stages")
    r = subprocess.run([exe, str(tmp_path), str(w), str(h)] + ([] if exact else ["fast"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(str(tmp_path / "out.bin"), dtype=np.uint8)
    n = int(raw[:4].view(np.int32)[0])
    fl = raw[4:].view(np.float32)
    o = 0

    def take(k):
        nonlocal o
        v = fl[o:o + k]
        o += k
        return v

    pose_sia, sia_cost = take(6), take(1)[0]
    pose_ref, ref_cost = take(6), take(1)[0]
    projected = take(2 * n).reshape(n, 2)
    merged = take(2 * n).reshape(n, 2)
    updated = take(3 * n).reshape(n, 3)
    rec = take(5 * n).reshape(n, 5)
    dims = fl[o:].view(np.int32).tolist()                          # StereoImage::left and ::opt_flow of frame 1
    n_left, left_dims = dims[0], list(zip(dims[1:1 + 2 * dims[0]:2], dims[2:2 + 2 * dims[0]:2]))
    dims = dims[1 + 2 * n_left:]
    n_lk, lk_dims = dims[0], list(zip(dims[1:1 + 2 * dims[0]:2], dims[2:2 + 2 * dims[0]:2]))
    assert len(dims) == 1 + 2 * n_lk
    assert n_left == cfg["max_pyramid_levels"] and left_dims == size_cases.floor_dims(cfg)        # halfSample: floor
    assert n_lk == len(O.build_lk_pyramid(L[1], cfg["window_size_opt_flow"])) and lk_dims == size_cases.ceil_dims(cfg, n_lk)

    # the same steps through the ctypes binding
    slam = StereoSlam(cfg)
    slam.new_image(L[0], R[0], 0.0)
    f0 = slam.get_frame()
    assert len(f0.kps2d) == n
    H = hip_lib.Handle(0, 4096)
    H.set_exact_pinv(exact)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nl = cfg["max_pyramid_levels"]
    win = cfg["window_size_opt_flow"]
    p0, p1 = H.build_pyramid(dev(L[0]), nl), H.build_pyramid(dev(L[1]), nl)
    k2, k3 = dev(f0.kps2d), dev(f0.kps3d)
    flags = dev(util.flags_of(f0.info))
    g_pose, g_cost, _, _ = H.sparse_align(p0, p1, k2, k3, flags, cam, dev(np.zeros(6, np.float32)))
    assert np.array_equal(g_pose.cpu().numpy(), pose_sia) and float(g_cost.cpu()) == sia_cost
    g_proj = H.project_keypoints(g_pose, k3, cam)
    assert np.array_equal(g_proj.cpu().numpy(), projected)
    lk0, lk1 = H.build_lk_pyramid(dev(L[0]), win), H.build_lk_pyramid(dev(L[1]), win)
    cur = g_proj.clone()
    _, st, err = H.klt_track(lk0, lk1, k2, cur, win)       # one keyframe: every point tracks against it
    g_k2 = g_proj.clone()
    g_fl = flags.clone()
    g_ref, g_rcost, _ = H.reproj_gn(g_k2, k3, g_fl, cam, g_pose, cur, err)
    assert np.array_equal(g_ref.cpu().numpy(), pose_ref) and float(g_rcost.cpu()) == ref_cost
    assert np.array_equal(g_k2.cpu().numpy(), merged)
    disp = H.ssd_disparity(dev(L[1]), dev(R[1]), g_k2, cfg["window_size_depth_calculator"], cfg["search_x"],
                           cfg["search_y"], 1)
    g3 = k3.clone()
    outl = dev(f0.info["outlier_count"].astype(np.int32))
    inl = dev(f0.info["inlier_count"].astype(np.int32))
    kx, kP = dev(f0.info["kf_inv_depth"].copy()), dev(f0.info["kf_variance"].copy())
    kf_pose = dev(np.zeros((n, 6), np.float32))
    H.depth_filter_update(g_k2, g3, g_fl, cam, g_ref, disp, k3, k2, kf_pose, outl, inl, kx, kP)
    assert np.array_equal(g3.cpu().numpy(), updated)
    assert np.array_equal(g_fl.cpu().numpy().astype(np.float32), rec[:, 0])
    assert np.array_equal(outl.cpu().numpy().astype(np.float32), rec[:, 1])
    assert np.array_equal(inl.cpu().numpy().astype(np.float32), rec[:, 2])
    assert np.array_equal(kx.cpu().numpy(), rec[:, 3]) and np.array_equal(kP.cpu().numpy(), rec[:, 4])
    assert np.linalg.norm(pose_ref[:3] - poses[1][:3]) < 0.05        # and it is a sensible pose
    H.close()
    return n_lk


# ---------------------------------------------------------------- StereoSlam over a whole sequence

NULL_TEXT = "libsvo_hip: bad ctx / sequence index"       # ctx_seq (csrc/svo_ctx.hip) rejects a NULL ctx; check() throws it
INFO_FIELDS = [f for f in KP_INFO_DTYPE.names if f != "_pad"]


def _write_sequence(d, mode="pair"):
    cfg, L, R, ts = FC.sequence()
    with open(d / "cam.bin", "wb") as f:
        f.write(bytes(hip_lib.CameraSettings.from_dict(cfg)))
    samples = np.ascontiguousarray(FC.imu_samples())
    np.array([FC.FRAMES, cfg["width"], cfg["height"], len(samples)], np.int32).tofile(str(d / "meta.bin"))
    np.array(ts, np.float32).tofile(str(d / "ts.bin"))
    samples.tofile(str(d / "samples.bin"))
    with open(d / "frames.bin", "wb") as f:
        for k in range(FC.FRAMES):
            for buf in FC.buffers(mode, k):
                if buf is not None:
                    f.write(np.ascontiguousarray(buf).tobytes())
    return cfg, ts


class _Reader:
    def __init__(self, path):
        self.raw, self.o = np.fromfile(path, np.uint8), 0

    def take(self, dtype, count=1):
        n = np.dtype(dtype).itemsize * count
        assert self.o + n <= len(self.raw), "out.bin ends early"
        v = self.raw[self.o:self.o + n].view(dtype)
        self.o += n
        return v

    def i32(self):
        return int(self.take(np.int32)[0])

    def keypoints(self):
        n = self.i32()
        return (self.take(np.float32, 2 * n).reshape(n, 2), self.take(np.float32, 3 * n).reshape(n, 3),
                self.take(KP_INFO_DTYPE, n))

    def keyframe(self):
        kid, pose = self.i32(), self.take(np.float32, 6)
        k2, k3, info = self.keypoints()
        return SimpleNamespace(id=kid, pose=pose, kps2d=k2, kps3d=k3, info=info)


def _read_sequence_output(path, n_frames):
    r = _Reader(path)
    before = r.i32()
    frames = []
    for _ in range(n_frames):
        got, fid, stamp, pose = r.i32(), r.i32(), float(r.take(np.float64)[0]), r.take(np.float32, 6)
        k2, k3, info = r.keypoints()
        n_kf, m = r.i32(), r.i32()
        frames.append(SimpleNamespace(got=got, id=fid, time_stamp=stamp, pose=pose, kps2d=k2, kps3d=k3, info=info,
                                      n_keyframes=n_kf, updates=r.take(np.float32, 6 * m).reshape(m, 6)))
    keyframes = [r.keyframe() for _ in range(r.i32())]
    last = r.keyframe()
    n = r.i32()
    trajectory = r.take(np.float32, 6 * n).reshape(n, 6)
    assert r.o == len(r.raw), "out.bin holds more than the records"
    return before, frames, keyframes, last, trajectory


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_keypoints(tag, got, k2, k3, info):
    assert _same(got.kps2d, k2), f"{tag}: kps2d"
    assert _same(got.kps3d, k3), f"{tag}: kps3d"
    assert len(got.info) == len(info), f"{tag}: info count"
    for name in INFO_FIELDS:
        assert _same(got.info[name], info[name]), f"{tag}: info.{name}"


def _same_frame(tag, got, want):
    assert _same(got.pose, want["pose"]), (tag, got.pose, want["pose"])
    _same_keypoints(tag, got, want["kps2d"], want["kps3d"], want["info"])
    assert _same(got.updates, want["updates"]), (tag, "update_pose", got.updates, want["updates"])


@pytest.mark.parametrize("mode", ["pair", "sbs", "econ", "bgr", "fast", "fast_late"])
def test_stereo_slam_over_a_sequence_equals_the_oracle(tmp_path, mode):
    """hostcpp's StereoSlam over the 14 frames of tests/facade_cases.py with the app's IMU loop after four of them,
    frames handed over as the mode says (tests/cpp/facade_sequence.cpp), against oracle_py.Slam fed the gray frames
    (the colour and packed modes: the gray images tests/ingest_ref.py makes of the same buffers). Default solver:
    every pose, keypoint array, info field, update_pose return, keyframe and the trajectory on bits. Fast solver:
    poses within the project's 1e-4; fast_late switches after the third frame, frames 0-2 stay on bits."""
    cfg, ts = _write_sequence(tmp_path, mode)
    exe = _build(tmp_path, "facade_sequence")
    t0 = time.perf_counter()
    r = subprocess.run([exe, str(tmp_path), mode], capture_output=True, text=True, timeout=120)
    print(f"facade_sequence {mode}: {time.perf_counter() - t0:.2f} s")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    for call in ("get_keyframe", "get_keyframes", "get_trajectory", "update_pose"):     # before the first image
        assert f"null {call}: {NULL_TEXT}" in lines, (call, lines)
    before, frames, keyframes, last, trajectory = _read_sequence_output(str(tmp_path / "out.bin"), FC.FRAMES)
    assert before == 0                                                                   # get_frame: false, no ctx yet

    want_frames, want_keyframes, want_trajectory = FC.oracle_run(colour=mode in FC.COLOUR_MODES)
    exact_until = {"fast": 0, "fast_late": 3}.get(mode, FC.FRAMES)
    for k, (got, want) in enumerate(zip(frames, want_frames)):
        tag = f"{mode} frame {k}"
        assert got.got == 1 and got.id == k and got.time_stamp == float(np.float32(ts[k])), (tag, got.id, got.time_stamp)
        assert got.n_keyframes == want["n_keyframes"], (tag, got.n_keyframes, want["n_keyframes"])
        assert len(got.updates) == len(want["updates"]) == (3 if k in FC.IMU_AFTER else 0), tag
        if k < exact_until:
            _same_frame(tag, got, want)
        else:
            assert np.max(np.abs(got.pose - want["pose"])) < 1e-4, (tag, got.pose, want["pose"])
            assert len(got.kps2d) == len(want["kps2d"]) and np.isfinite(got.updates).all(), tag
    assert len(keyframes) == len(want_keyframes) >= 3 and [kf.id for kf in keyframes] == list(range(len(keyframes)))
    assert last.id == len(keyframes) - 1
    assert _same(last.pose, keyframes[-1].pose)
    _same_keypoints(f"{mode} get_keyframe", last, keyframes[-1].kps2d, keyframes[-1].kps3d, keyframes[-1].info)
    assert trajectory.shape == want_trajectory.shape
    if exact_until == FC.FRAMES:
        for kid, (got, (k2, k3, info, pose)) in enumerate(zip(keyframes, want_keyframes)):
            assert _same(got.pose, pose), (mode, "keyframe", kid, got.pose, pose)
            _same_keypoints(f"{mode} keyframe {kid}", got, k2, k3, info)
        assert _same(trajectory, want_trajectory), (mode, "trajectory")
    else:
        for kid, (got, (k2, k3, info, pose)) in enumerate(zip(keyframes, want_keyframes)):
            assert np.max(np.abs(got.pose - pose)) < 1e-4 and len(got.kps2d) == len(k2), (mode, "keyframe", kid)
        assert np.max(np.abs(trajectory - want_trajectory)) < 1e-4
        assert _same(trajectory[:exact_until], want_trajectory[:exact_until])


@pytest.mark.parametrize("exact", [False, True])
def test_facade_stage_classes_with_two_keyframes(tmp_path, exact):
    """PoseRefiner and DepthFilter on a frame whose keypoints come from two keyframes (the frame after the first
    mixed one of tests/facade_cases.py): the grouping by keyframe id, the scatter back and the per-keypoint keyframe
    look-ups, against the same C entries through the ctypes binding, one klt_track call per keyframe's group."""
    cfg, ts = _write_sequence(tmp_path, "pair")
    _, L, R, _ = FC.sequence()
    want_frames, _, _ = FC.oracle_run()
    K = FC.stage_frame(want_frames)
    exe = _build(tmp_path, "facade_stages_seq")
    t0 = time.perf_counter()
    r = subprocess.run([exe, str(tmp_path), str(K)] + ([] if exact else ["fast"]), capture_output=True, text=True, timeout=120)
    print(f"facade_stages_seq: {time.perf_counter() - t0:.2f} s")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rd = _Reader(str(tmp_path / "stages.bin"))
    made_on = rd.take(np.int32, rd.i32()).tolist()
    n = rd.i32()
    pose_sia, sia_cost = rd.take(np.float32, 6), rd.take(np.float32)[0]
    pose_ref, ref_cost = rd.take(np.float32, 6), rd.take(np.float32)[0]
    projected, merged = rd.take(np.float32, 2 * n).reshape(n, 2), rd.take(np.float32, 2 * n).reshape(n, 2)
    updated, rec = rd.take(np.float32, 3 * n).reshape(n, 3), rd.take(np.float32, 5 * n).reshape(n, 5)
    assert rd.o == len(rd.raw)
    assert made_on == [k for k in range(K) if want_frames[k]["made"]] and len(made_on) >= 2

    # the same steps through the ctypes binding
    cam = hip_lib.CameraSettings.from_dict(cfg)
    slam = StereoSlam(cfg)
    for k in range(K):
        slam.new_image(L[k], R[k], ts[k])
    prev = slam.get_frame()
    kfs = [slam.get_keyframe(i) for i in range(slam.num_keyframes())]
    assert len(prev.kps2d) == n and len(kfs) == len(made_on)
    kf_id, kp_index = prev.info["keyframe_id"], prev.info["keypoint_index"]
    groups = [int(g) for g in np.unique(kf_id)]                       # ascending, as the std::map walks them
    assert len(groups) >= 2 and min(int((kf_id == g).sum()) for g in groups) >= 1
    H = hip_lib.Handle(0, 4096)
    H.set_exact_pinv(exact)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared frames are read-only)
    nl, win = cfg["max_pyramid_levels"], cfg["window_size_opt_flow"]
    p_prev, p_cur = H.build_pyramid(dev(L[K - 1]), nl), H.build_pyramid(dev(L[K]), nl)
    k2, k3 = dev(prev.kps2d), dev(prev.kps3d)
    flags = dev(util.flags_of(prev.info))
    g_pose, g_cost, _, _ = H.sparse_align(p_prev, p_cur, k2, k3, flags, cam, dev(prev.pose))
    assert np.array_equal(g_pose.cpu().numpy(), pose_sia) and float(g_cost.cpu()) == sia_cost
    g_proj = H.project_keypoints(g_pose, k3, cam)
    assert np.array_equal(g_proj.cpu().numpy(), projected)
    lk_cur = H.build_lk_pyramid(dev(L[K]), win)
    tracked, err = g_proj.clone(), torch.zeros(n, dtype=torch.float32, device="cuda")
    for g in groups:
        idx = torch.from_numpy(np.flatnonzero(kf_id == g)).cuda()
        ref = dev(kfs[g].kps2d[kp_index[kf_id == g]])
        cur = g_proj[idx].clone()
        torch.cuda.synchronize()
        _, st, e = H.klt_track(H.build_lk_pyramid(dev(L[made_on[g]]), win), lk_cur, ref, cur, win)
        torch.cuda.synchronize()
        tracked[idx], err[idx] = cur, e                                # scattered back in Python
    torch.cuda.synchronize()
    g_k2, g_fl = g_proj.clone(), flags.clone()
    g_ref, g_rcost, _ = H.reproj_gn(g_k2, k3, g_fl, cam, g_pose, tracked, err)
    assert np.array_equal(g_ref.cpu().numpy(), pose_ref) and float(g_rcost.cpu()) == ref_cost
    assert np.array_equal(g_k2.cpu().numpy(), merged)
    disp = H.ssd_disparity(dev(L[K]), dev(R[K]), g_k2, cfg["window_size_depth_calculator"], cfg["search_x"],
                           cfg["search_y"], 1)
    g3 = k3.clone()
    outl, inl = dev(prev.info["outlier_count"].astype(np.int32)), dev(prev.info["inlier_count"].astype(np.int32))
    kx, kP = dev(prev.info["kf_inv_depth"].copy()), dev(prev.info["kf_variance"].copy())
    ref3d = dev(np.stack([kfs[g].kps3d[i] for g, i in zip(kf_id, kp_index)]))
    ref2d = dev(np.stack([kfs[g].kps2d[i] for g, i in zip(kf_id, kp_index)]))
    kf_pose = dev(np.stack([kfs[g].pose for g in kf_id]).astype(np.float32))
    H.depth_filter_update(g_k2, g3, g_fl, cam, g_ref, disp, ref3d, ref2d, kf_pose, outl, inl, kx, kP)
    assert np.array_equal(g3.cpu().numpy(), updated)
    assert np.array_equal(g_fl.cpu().numpy().astype(np.float32), rec[:, 0])
    assert np.array_equal(outl.cpu().numpy().astype(np.float32), rec[:, 1])
    assert np.array_equal(inl.cpu().numpy().astype(np.float32), rec[:, 2])
    assert np.array_equal(kx.cpu().numpy(), rec[:, 3]) and np.array_equal(kP.cpu().numpy(), rec[:, 4])
    assert len({tuple(p) for p in kf_pose.cpu().numpy()}) >= 2         # the keyframe poses differ: a wrong look-up shows
    H.close()
    slam.close()
