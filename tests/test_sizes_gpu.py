"""The whole tracker ctx at image sizes that nothing divides (tests/size_cases.py): odd widths and heights, levels
where halfSample's floor and pyrDown's ceil disagree, rows that are no whole number of dwords, borrowed frames
whose base and stride are off a dword, partial grid cells, fewer than SVO_LK_LEVELS LK levels. Every comparison
is the one the suite already makes at 320x240, 752x480 and 1920x1080: bit for bit against the oracle for the
tracker, byte for byte against the numpy statements (view_ref, dense_ref, cloud_ref, ar_ref, snapshot_ref,
rectify_ref, rigcal_ref, ingest_ref) for the jobs and the raw input."""
import os

import numpy as np
import pytest
import torch

import ar_ref as AR
import cloud_ref as CR
import dense_ref as DR
import ingest_ref as IR
import rectify_ref as RR
import rigcal_ref as RC
import size_cases as S
import snapshot_ref as SR
import util
import view_ref as VR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import CameraCalibration
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch, pick_launch_shapes
import test_ar_gpu as TA
import test_cloud_gpu as TC
import test_dense_gpu as TD
import test_export_gpu as TE
import test_ingest_gpu as TI
import test_rectify_gpu as TR
import test_view_gpu as TV
from test_tracker_gpu import _batch_against_oracle, _oracle_frames, _run

pytestmark = pytest.mark.gpu


def _batch(cfg, n_slots, groups):
    """a ctx of n_slots slots in `groups` sequence groups"""
    old = os.environ.get("SVO_GROUPS")
    os.environ["SVO_GROUPS"] = str(groups)
    try:
        b = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    finally:
        if old is None:
            del os.environ["SVO_GROUPS"]
        else:
            os.environ["SVO_GROUPS"] = old
    assert b.groups() == groups
    return b


def _gpu_sequences(name, seeds, n_frames):
    """the case's sequences of `seeds` rendered on the GPU: [(cfg, lefts [n, H, W], rights, poses, time stamps)]"""
    c = S.CASES[name]
    out = [synth.make_sequence_gpu(c["preset"], n_frames, seed, motion_scale=c["motion"], overrides=c["overrides"])
           for seed in seeds]
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------- a. a lone ctx, every case

# frames per case: the case's own count, cut behind its second keyframe after frame 0 where it comes earlier
LONE_FRAMES = dict(odd323=25, half322=30, cells321=29, dense327=21, lk2_167=13, lk1_61=14, euroc749=8)


@pytest.mark.parametrize("name", list(S.CASES))
def test_lone_ctx_equals_the_oracle(name):
    """host frames, the default (reference-order) solver: every frame's keyframe decision, index lists, flags,
    counters, score, pose, keypoints and GN traces, then the keyframes and the trajectory"""
    c = S.CASES[name]
    gpu, ref, same = _run(c["preset"], LONE_FRAMES[name], c["seed"], motion_scale=c["motion"], exact=True,
                          overrides=c["overrides"])
    assert same == 1.0
    if name != "euroc749":
        assert ref.num_keyframes() >= 3, "the case lost its keyframes"
    gpu.close()


# ---------------------------------------------------------------------------------- b. input layouts

LAYOUT_FRAMES = 8


def _layout_frames(form, L, R):
    """the frames of one sequence as the tensors of an input form, and whether they are borrowed"""
    n, H, W = L.shape
    if form == "host":
        return [torch.from_numpy(L[k].copy()) for k in range(n)], [torch.from_numpy(R[k].copy()) for k in range(n)], False
    if form in ("copied", "borrowed"):
        dl, dr = torch.from_numpy(L.copy()).cuda(), torch.from_numpy(R.copy()).cuda()
        return [dl[k] for k in range(n)], [dr[k] for k in range(n)], form == "borrowed"
    wide_l = torch.full((n, H, W + 13), 0xEE, dtype=torch.uint8, device="cuda")
    wide_r = torch.full((n, H, W + 13), 0x11, dtype=torch.uint8, device="cuda")
    wide_l[:, :, 5:5 + W], wide_r[:, :, 5:5 + W] = torch.from_numpy(L.copy()).cuda(), torch.from_numpy(R.copy()).cuda()
    return [wide_l[k, :, 5:5 + W] for k in range(n)], [wide_r[k, :, 5:5 + W] for k in range(n)], True


@pytest.mark.parametrize("form", ["host", "copied", "borrowed", "slice"])
@pytest.mark.parametrize("name", ["odd323", "cells321"])
def test_input_layouts_equal_the_oracle(name, form):
    """the same sequence through pack_images / submit_packed as a host tensor, a contiguous device tensor that is
    copied, the same tensor borrowed (stride = the odd width) and a borrowed slice [:, 5:5+W] of a [H, W+13] tensor
    (base off a dword): every frame equals the oracle's"""
    cfg, L, R, ts = S.sequence(name, LAYOUT_FRAMES)
    frames, _ = S.oracle_run(name, LAYOUT_FRAMES)
    lefts, rights, borrow = _layout_frames(form, L, R)
    if borrow:                                             # level 0 of every kernel takes its byte path
        assert all((t.data_ptr() | t.stride(0)) & 3 for t in lefts + rights)
    torch.cuda.synchronize()
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    for k in range(LAYOUT_FRAMES):
        batch.submit_packed(batch.pack_images([lefts[k]], [rights[k]], [float(ts[k])], borrow=borrow))
        batch.wait()
        made, k2, k3, info, pose, ost = frames[k]
        st = batch.stats(0)
        assert st.is_keyframe == made, f"{name} {form} frame {k}: keyframe decision"
        util.compare_frame(f"{name} {form} frame {k}", batch.get_frame(0), k2, k3, info, pose, 0.0)
        if k > 0:
            assert util.same_trace(st, ost, cfg), f"{name} {form} frame {k}: GN trace differs from the oracle's"
    assert np.array_equal(batch.get_trajectory(0), np.array([f[4] for f in frames]))
    batch.close()


# ---------------------------------------------------------------------------------- c. batched launches

DENSE_BATCH = dict(n_seq=34, n_frames=12, first_seed=3)


@pytest.fixture(scope="module")
def dense_batch():
    """34 `dense327` sequences (seeds 3, 4, ...) of 12 frames and the oracle's frames of each"""
    p = DENSE_BATCH
    rendered = _gpu_sequences("dense327", range(p["first_seed"], p["first_seed"] + p["n_seq"]), p["n_frames"])
    cfg = rendered[0][0]
    oracle = _oracle_frames(rendered, cfg)
    assert any(f[0] for o in oracle for f in o[1:]), "a keyframe inside the run"
    assert max(len(f[1]) for o in oracle for f in o) > 128, "some set passes 128 keypoints"
    return rendered, cfg, oracle


def _predicted_shapes(cfg, oracle, groups):
    """{(kernel, waves, mode, cap): launches} of a run that waits after every frame set: a group's launch of step k
    is sized by the largest keypoint count its sequences had after step k - 1 (a host decision:
    svo_pick_launch_shapes), and every group launches once per step"""
    cap = SR.capacity(cfg)
    rec_cap = (cap + 511) // 512 * 512
    want = {}
    for lo, hi in groups:
        for k in range(1, len(oracle[0])):
            n_bound = min(max(len(o[k - 1][1]) for o in oracle[lo:hi]), cap)
            for key in pick_launch_shapes(cfg, hi - lo, n_bound, rec_cap=rec_cap):
                assert key is not None
                want[key] = want.get(key, 0) + 1
    return want


def test_batched_launch_at_an_odd_size_equals_the_oracle(monkeypatch, dense_batch):
    """34 sequences of 327x241 in one group, borrowed frames (odd stride, odd bases): one launch holds the 32
    sequences at which sia.hip and reproj.hip switch shape; bit for bit against the oracle on every frame, and the
    launch shapes are the ones the host decision predicts"""
    rendered, cfg, oracle = dense_batch
    monkeypatch.setenv("SVO_GROUPS", "1")
    shapes = _batch_against_oracle(rendered, cfg, oracle, 1)
    print("dense327 batched launch shapes:", shapes)
    want = _predicted_shapes(cfg, oracle, [(0, len(rendered))])
    assert shapes == want, (shapes, want)
    assert all(k[2] == 2 for k in shapes if k[0] == "sia_gn_kernel"), shapes       # records and taps from L2
    assert any(k[3] > 128 for k in shapes if k[0] == "sia_gn_kernel"), shapes


def test_batched_launch_with_two_lk_levels_equals_the_oracle(monkeypatch):
    """4 `lk2_167` sequences in 2 groups, 8 frames, borrowed frames: n_lk = 2 in a batched launch"""
    rendered = _gpu_sequences("lk2_167", (1, 2, 3, 4), 8)
    cfg = rendered[0][0]
    assert SR.lk_levels(cfg) == 2
    oracle = _oracle_frames(rendered, cfg)
    assert any(f[0] for o in oracle for f in o[1:]), "a keyframe inside the run"
    monkeypatch.setenv("SVO_GROUPS", "2")
    shapes = _batch_against_oracle(rendered, cfg, oracle, 2)
    print("lk2_167 batched launch shapes:", shapes)


# ---------------------------------------------------------------------------------- d. jobs behind an odd-size ctx

JOB_SEEDS, JOB_FRAMES = (1, 11, 12), 5


@pytest.fixture(scope="module")
def odd_jobs():
    """`odd323`, 3 slots in 2 groups after 5 borrowed frames: (ctx, cfg, per slot the host frames (lefts, rights),
    per slot the index of the frame its newest keyframe shows)"""
    rendered = _gpu_sequences("odd323", JOB_SEEDS, JOB_FRAMES)
    cfg = rendered[0][0]
    batch = _batch(cfg, 3, 2)
    kf = [0] * 3
    for k in range(JOB_FRAMES):
        batch.submit_packed(batch.pack_images([r[1][k] for r in rendered], [r[2][k] for r in rendered],
                                              [float(r[4][k]) for r in rendered], borrow=True))
        batch.wait()
        for s in range(3):
            if batch.stats(s).is_keyframe:
                kf[s] = k
    host = [(r[1].cpu().numpy(), r[2].cpu().numpy()) for r in rendered]
    yield batch, cfg, host, kf
    batch.close()
    del rendered


def test_views_at_an_odd_size(odd_jobs):
    """every left level (floor halving), the right plane, and RGB8 / RGBA8 marker views against view_ref"""
    batch, cfg, host, kf = odd_jobs
    W, H, levels = cfg["width"], cfg["height"], cfg["max_pyramid_levels"]
    slots = [0, 1, 2]
    for what in (TV.FRAMES, TV.KEYFRAMES):
        left, right = TV._gray_views(batch, what)
        for s in slots:
            src = JOB_FRAMES - 1 if what == TV.FRAMES else kf[s]
            chain = TV._chain(host[s][0][src], levels)
            for l in range(levels):
                assert (left[l].cols, left[l].rows, left[l].pitch, left[l].image_bytes) == VR.size(W, H, VR.PLANE_LEFT, l, VR.GRAY8)
                img = left[l].image(s)
                assert img.shape == (H >> l, W >> l), (what, s, l)
                assert img.tobytes() == chain[l].tobytes(), (what, s, l)
                TV._check_segment((what, s, l), left[l].segments[s], batch, what, s)
            assert right.image(s).tobytes() == host[s][1][src].tobytes(), (what, s)
        for level in (0, 1, levels - 1):
            for pixel in ("rgb8", "rgba8"):
                v = batch.export_views(what, level=level, pixel=pixel, markers=True)
                assert (v.cols, v.rows, v.pitch, v.image_bytes) == VR.size(W, H, VR.PLANE_LEFT, level, v.style.pixel)
                TV._check_marker_views((what, level, pixel), batch, what, slots, v, left[level])
                assert any(v.image(i)[:, :, :3].tobytes() != np.repeat(left[level].image(i)[:, :, None], 3, 2).tobytes()
                           for i in slots)
        for device in (False, True):                       # unexpanded planes in device mode too, plain RGB included
            v = batch.export_views(what, [2, 0], level=1, pixel="rgb8", device=device)
            for i, s in enumerate((2, 0)):
                src = JOB_FRAMES - 1 if what == TV.FRAMES else kf[s]
                want = VR.expand(TV._chain(host[s][0][src], 2)[1], VR.RGB8)
                assert TV._np(v.image(i)).tobytes() == want.tobytes(), (what, s, device)


# the job's window and search ranges where dense_ref walks a whole lattice (every point walks its own candidates)
DENSE_STEP1 = dict(win=3, search_x=2, search_y=1)
DENSE_STEP3 = dict(win=7, search_x=9, search_y=2)


@pytest.mark.parametrize("step,win", [(1, DENSE_STEP1), (3, DENSE_STEP3)], ids=["step1", "step3"])
def test_disparity_at_an_odd_size(odd_jobs, step, win):
    """disparity and cost planes of every slot's current frame at lattice step 1 (323 x 245 points) and 3
    (107 x 81: the last columns and rows of the image hold no point) against dense_ref, bit for bit"""
    batch, cfg, host, kf = odd_jobs
    W, H = cfg["width"], cfg["height"]
    job = batch.submit_disparity("frames", None, step=step, cost=True, **win)
    job.wait()
    job._buf.fill_(float(TD.GUARD))
    job.submit().wait()
    assert (job.cols, job.rows, job.n_planes) == (W // step, H // step, 2)
    for s in range(3):
        left, right = host[s][0][JOB_FRAMES - 1], host[s][1][JOB_FRAMES - 1]
        seg = job.segments[s]
        assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"])) == (s, hip_lib.DISPARITY_OK, JOB_FRAMES - 1)
        assert int(seg["offset"]) == s * job.image_bytes
        got = job.planes(s)
        if s == 0:                                         # the statement itself: value and cost
            want = DR.planes(left, right, win["win"], win["search_x"], win["search_y"], step, DR.DISPARITY, True)
            assert np.array_equal(TD._bits(got[0]), TD._bits(want[0])), (s, int((TD._bits(got[0]) != TD._bits(want[0])).sum()))
            assert np.array_equal(TD._bits(got[1]), TD._bits(want[1])), (s, int((TD._bits(got[1]) != TD._bits(want[1])).sum()))
            assert len(np.unique(want[0])) > 2
        TD._check_slot(("odd", step), job, s, s, batch, "frames")      # (the oracle's search on the ctx's own views)
    flat = TD._bits(job._buf)
    guard = TD._bits(np.full(1, TD.GUARD))[0]
    used = job.n_planes * job.rows * job.cols
    assert all((flat[s * job.image_bytes // 4 + used:(s + 1) * job.image_bytes // 4] == guard).all() for s in range(3))
    if step == 3:                                          # the newest keyframes, as depth, in device memory
        job = batch.export_disparity("last_keyframes", [2, 0], value="depth", step=3, device=True, **win)
        for i, s in ((0, 2), (1, 0)):
            TD._check_slot("keyframes", job, i, s, batch, "last_keyframes")


_CLOUD_PLANES = {}          # dense_ref's planes of the fixture's views, per (what, slot): computed once, never changed


@pytest.mark.parametrize("layout,frame", [("compact", "world"), ("organized", "camera")])
def test_cloud_at_an_odd_size(odd_jobs, layout, frame):
    """compact and organized clouds of frames and newest keyframes against cloud_ref over dense_ref's planes"""
    batch, cfg, host, kf = odd_jobs
    played = (batch, _CLOUD_PLANES)
    for what in ("frames", "last_keyframes"):
        job = batch.submit_cloud(what, None, step=TC.STEP, frame=frame, layout=layout, **TC.WIN, **TC.FILTER)
        job.wait()
        job.points_buffer.fill_(TC.GUARD)
        job.submit().wait()
        assert (job.cols, job.rows) == (cfg["width"] // TC.STEP, cfg["height"] // TC.STEP)
        for s in range(3):
            src = JOB_FRAMES - 1 if what == "frames" else kf[s]
            n, planes = TC._check_slot((what, layout), job, s, s, played, what)
            assert played[1][(what, s)][0].tobytes() == host[s][0][src].tobytes()      # the plane it walked is the frame given
            assert 0 < n < (planes[0] >= 0).sum()
    job = batch.submit_cloud("frames", [1], step=5, layout=layout, device=True, win=5, search_x=6, search_y=1)
    job.wait()
    left, right = host[1][0][JOB_FRAMES - 1], host[1][1][JOB_FRAMES - 1]
    planes = DR.planes(left, right, 5, 6, 1, 5, DR.DISPARITY, True)
    rig = {k: cfg[k] for k in CR.RIG_KEYS}
    ref, n = CR.cloud(left, planes, 5, 5, rig, job.segments[0]["pose"], CR.WORLD, TC.LAYOUTS[layout])
    assert int(job.segments[0]["n_points"]) == n
    raw = TC._np(job.points_buffer[:job.points_per_slot])
    assert raw[:len(ref)].tobytes() == ref.tobytes()


@pytest.mark.parametrize("device", (False, True))
def test_ar_picture_at_an_odd_size(odd_jobs, device):
    """the lit boxes over every slot's 323 x 245 camera image against ar_ref (rows of 969 and 1292 bytes)"""
    batch, cfg, host, kf = odd_jobs
    for pixel in ("rgb8", "rgba8"):
        job = batch.submit_ar(TA.MESHES, TA.INSTANCES, None, device=device, pixel=pixel)
        job.wait()
        job._buf.fill_(TA.FILL)
        job.submit().wait()
        assert (job.pitch, job.image_bytes) == AR.size(cfg["width"], cfg["height"], job.style.pixel)
        for s in range(3):
            TA._check_slot(pixel, job, s, s, batch, TA.INSTANCES)
        px = job.pixels.cpu().numpy() if device else job.pixels
        used = job.rows * job.pitch
        assert all((px[s * job.image_bytes + used:(s + 1) * job.image_bytes] == TA.FILL).all() for s in range(3))


def test_bulk_export_at_an_odd_size(odd_jobs):
    """frames and newest keyframes of all slots in one launch against the getters"""
    batch, cfg, host, kf = odd_jobs
    slots = [0, 1, 2]
    state = TE._getter_state(batch)
    for device in (False, True):
        frames = batch.export_frames(device=device)
        keyframes = batch.export_last_keyframes(device=device)
        ts = (JOB_FRAMES - 1) / 20.0
        TE._check_frames(f"device {device}", frames, state, slots, {s: (0, np.float32(ts)) for s in slots})
        TE._check_keyframes(f"device {device}", keyframes, state, slots)
        TE._check_placement(frames, batch, slots)
        TE._check_placement(keyframes, batch, slots)
    assert batch.export_capacity() == SR.capacity(cfg)


def test_snapshot_with_two_lk_levels_moves_between_ctxs():
    """`lk2_167`: saved after frame 6 in a 1-slot ctx, loaded into slot 2 of a 3-slot ctx in 2 groups; the header's
    plane directory is snapshot_ref's (floor dims for the alignment pyramid, ceil dims for the one further LK
    level), the image planes are the frames given, and frames 7 .. 12 equal the uninterrupted run (the oracle's)"""
    n, k_save = 13, 6
    cfg, L, R, ts = S.sequence("lk2_167", n)
    frames, _ = S.oracle_run("lk2_167", n)
    made = [k for k in range(n) if frames[k][0]]
    assert any(0 < k <= k_save for k in made) and any(k > k_save for k in made), made
    levels = cfg["max_pyramid_levels"]

    def check(tag, batch, slot, k):
        mk, k2, k3, info, pose, ost = frames[k]
        st = batch.stats(slot)
        assert st.frame_id == k and st.is_keyframe == mk, tag
        util.compare_frame(tag, batch.get_frame(slot), k2, k3, info, pose, 0.0)
        assert k == 0 or util.same_trace(st, ost, cfg), tag

    src = _batch(cfg, 1, 1)
    for k in range(k_save + 1):
        src.new_images([L[k]], [R[k]], [float(ts[k])])
    check("source", src, 0, k_save)
    snap = src.save([0])[0]
    ref = SR.parse(snap.host)
    assert (ref["width"], ref["height"], ref["lk_levels"], ref["pyramid_levels"]) == (167, 123, 2, levels)
    assert ref["capacity"] == SR.capacity(cfg) and ref["frame_id"] == k_save
    want = SR.plane_dims(cfg, ref["n_keypoints"], [kn for _, kn, _ in ref["keyframes"]], ref["n_image_sets"])
    assert [(rb, rows) for _, rb, rows in ref["directory"]] == want
    assert want[-1] == (84, 62) and (cfg["width"] >> 1, cfg["height"] >> 1) == (83, 61)
    left, right = TV._snapshot_planes(snap, cfg, "frame")
    for l, img in enumerate(TV._chain(L[k_save], levels)):
        assert left[l].tobytes() == img.tobytes(), l
    assert right.tobytes() == R[k_save].tobytes()
    state = (src.get_frame(0), src.get_trajectory(0).tobytes(), src.num_keyframes(0))
    src.close()

    dst = _batch(cfg, 3, 2)
    dst.load([2], [snap])
    f = dst.get_frame(2)
    assert (f.pose.tobytes(), f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes()) == \
           (state[0].pose.tobytes(), state[0].kps2d.tobytes(), state[0].kps3d.tobytes(), state[0].info.tobytes())
    assert dst.get_trajectory(2).tobytes() == state[1] and dst.num_keyframes(2) == state[2]
    for k in range(k_save + 1, n):                         # slot 0 plays the sequence from its start beside it
        j = k - k_save - 1
        dst.new_images([L[j], None, L[k]], [R[j], None, R[k]], [float(ts[j]), 0.0, float(ts[k])])
        check(f"resumed frame {k}", dst, 2, k)
        check(f"beside it, frame {j}", dst, 0, j)
    assert np.array_equal(dst.get_trajectory(2), np.array([f[4] for f in frames]))
    assert dst.num_keyframes(2) == len(made)
    again = dst.save([2])[0]
    assert SR.parse(again.host)["lk_levels"] == 2
    dst.close()


# ---------------------------------------------------------------------------------- e. raw input at an odd size

RAW_FRAMES = 4


@pytest.fixture(scope="module")
def odd_raw():
    """`odd323`, 2 sequences of 4 frames on the GPU (raw frames of the tests below)"""
    return _gpu_sequences("odd323", (21, 22), RAW_FRAMES)


def _odd_maps(W, H):
    """a small rotation plus radial term at the `tiny` focal lengths, as test_rectify_gpu.py builds its maps"""
    return (RR.euroc_like_maps(W, H, angle=0.012, shift=(1.5, -2.0), f_p=190.0, f_k=200.0),
            RR.euroc_like_maps(W, H, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068, f_p=190.0, f_k=200.0))


def _remapped(rendered, maps):
    """the sequences with every frame replaced by the statement's remap of it (device tensors again)"""
    out = []
    for cfg, L, R, poses, ts in rendered:
        l = np.stack([RR.remap_linear(x, *maps[0]) for x in L.cpu().numpy()])
        r = np.stack([RR.remap_linear(x, *maps[1]) for x in R.cpu().numpy()])
        out.append((cfg, torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda(), poses, ts))
    torch.cuda.synchronize()
    return out


def test_rectification_with_float_maps_at_an_odd_size(odd_raw):
    """set_rectification (host arrays and device tensors of 323 floats a row) on raw frames == a ctx fed
    rectify_ref's remap of them: per frame pose, keypoints, info and stats, at the end trajectories and keyframes;
    host, device and borrowed frames"""
    cfg = odd_raw[0][0]
    W, H = cfg["width"], cfg["height"]
    maps = _odd_maps(W, H)
    ref_frames, ref_final, _ = TR._run_batch(_remapped(odd_raw, maps), "device")
    for mode in ("host", "device", "borrow"):
        frames, final, _ = TR._run_batch(odd_raw, mode, maps=maps)
        assert frames == ref_frames and final == ref_final, mode
    dev_maps = tuple(tuple(torch.from_numpy(m).cuda() for m in side) for side in maps)
    frames, final, _ = TR._run_batch(odd_raw, "device", maps=dev_maps)
    assert frames == ref_frames and final == ref_final
    # and what the tracker worked on is the statement's image
    one = StereoSlamBatch(cfg, W, H, 1)
    one.set_rectification(*maps)
    one.new_images([odd_raw[0][1][0]], [odd_raw[0][2][0]], [0.0])
    assert one.export_views("frames").image(0).tobytes() == RR.remap_linear(odd_raw[0][1][0].cpu().numpy(), *maps[0]).tobytes()
    assert one.export_views("frames", plane="right").image(0).tobytes() == RR.remap_linear(odd_raw[0][2][0].cpu().numpy(), *maps[1]).tobytes()
    one.close()


def _odd_calibration(seed, W, H):
    """an EuRoC-like camera of the odd size as (rigcal_ref's tuple, CameraCalibration)"""
    s = float(seed)
    K = np.array([[208.0 + s, 0, W / 2.0 + 1.0 - 0.5 * s], [0, 207.25 + 0.5 * s, H / 2.0 - 3.5 + s], [0, 0, 1]], np.float64)
    D = np.array([-0.28 + 0.01 * s, 0.07, 2.0e-4 * s, -1.5e-4, 0.0, 0.0, 0.0, 0.0], np.float64)
    R = RC.rotation(0.003 * s, -0.002, 0.001 * s)
    P = np.array([[200.0, 0, (W - 1) / 2.0], [0, 200.0, (H - 1) / 2.0], [0, 0, 1]], np.float64)
    return (K, D, R, P), CameraCalibration.from_mats(K, D, R, P)


def test_calibration_maps_built_on_the_gpu_at_an_odd_size(odd_raw):
    """set_calibration (the fused map kernel: 323 is no multiple of its 4-column step) on raw frames == a ctx fed
    rectify_ref's remap through rigcal_ref's maps; and svo_build_rectify_maps gives those maps bit for bit"""
    cfg = odd_raw[0][0]
    W, H = cfg["width"], cfg["height"]
    (left_t, left_c), (right_t, right_c) = _odd_calibration(1, W, H), _odd_calibration(2, W, H)
    maps = (RC.maps(left_t, W, H), RC.maps(right_t, W, H))
    built = StereoSlamBatch.build_rectify_maps([left_c, right_c], W, H)
    for got, want in zip(built, maps):
        for axis in (0, 1):
            assert RC.same_bits(got[axis].cpu().numpy(), want[axis]), axis
    ref_frames, ref_final, _ = TR._run_batch(_remapped(odd_raw, maps), "device")
    n_seq = len(odd_raw)
    slam = StereoSlamBatch(cfg, W, H, n_seq)
    slam.set_calibration(left_c, right_c)
    for k in range(RAW_FRAMES):
        slam.new_images([r[1][k] for r in odd_raw], [r[2][k] for r in odd_raw], [k / 20.0] * n_seq)
        assert {s: TR._snapshot(slam, s) for s in range(n_seq)} == ref_frames[k], k
    assert [TR._final(slam, s) for s in range(n_seq)] == ref_final
    assert slam.export_views("frames", [0]).image(0).tobytes() == \
           RR.remap_linear(odd_raw[0][1][RAW_FRAMES - 1].cpu().numpy(), *maps[0]).tobytes()
    slam.close()


@pytest.mark.parametrize("fmt", ["sbs_gray", "sbs_bgr", "bgr_pair"])
def test_packed_input_formats_at_an_odd_size(odd_raw, fmt):
    """side-by-side gray (the right half starts at byte 323), side-by-side colour and BGR pairs (rows of 969
    bytes) == the default format on ingest_ref's gray images, in the three memory modes"""
    cfg = odd_raw[0][0]
    n_seq = len(odd_raw)
    colour, gray = TI._colour_frames(odd_raw)
    for s in range(n_seq):                                 # the statement's conversion of what is fed, once
        a, b = TI._pack_dev(fmt, colour[s][0, 0], colour[s][0, 1], gray[s][0][0], gray[s][1][0])
        gl, gr = IR.convert(fmt, a.cpu().numpy(), None if b is None else b.cpu().numpy(), width=cfg["width"])
        assert gl.tobytes() == gray[s][0][0].cpu().numpy().tobytes() and gr.tobytes() == gray[s][1][0].cpu().numpy().tobytes()
    feed = TI._feed_of(colour, gray)
    ref_frames, ref_final, _, _ = TI._drive(cfg, n_seq, RAW_FRAMES, feed)
    for mode in ("host", "device", "borrow"):
        frames, final, _, _ = TI._drive(cfg, n_seq, RAW_FRAMES, feed, fmt=fmt, mode=mode)
        assert frames == ref_frames and final == ref_final, (fmt, mode)
