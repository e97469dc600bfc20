"""GPU parity of the whole tracker (svo_ctx = StereoSlam::new_image,
src/lib/stereo_slam.cpp:123-271) against the oracle's restatement, frame by
frame on seeded synthetic sequences: feature index lists bit-exact, poses
within 1e-4 m / rad."""
import numpy as np
import pytest
import torch

import oracle_py as O
from stereo_svo_slam_amd import synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam, StereoSlamBatch
import util
from util import INT_FIELDS, compare_frame as _compare_frame, same_trace as _same_trace


def _free_port():
    """a TCP port nobody listens on right now (the rendezvous of the two-rank tests)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


pytestmark = pytest.mark.gpu

def _run(config, n_frames, seed, on_device=False, motion_scale=1.0, exact=True, tol=None,
         render_device="cpu", overrides=None):
    """Both trackers frame by frame. exact=True (the default here and of the product: the
    reference-order mode): every GN trace must equal the oracle's and the pose is the oracle's bit for
    bit; exact=False (svo_ctx_set_fast_solver): pose within 1e-4. Returns the fraction of
    tracked frames whose GN traces equal the oracle's as the third value. overrides: camera settings (the image
    size among them) that replace the preset's."""
    if tol is None:
        tol = 0.0 if exact else 1e-4
    cfg, L, R, poses, ts = synth.make_sequence(config, n_frames, seed, device=render_device,
                                               motion_scale=motion_scale, overrides=overrides)
    L = [x.cpu() for x in L]
    R = [x.cpu() for x in R]
    cam = util.oracle_camera(cfg)
    ref = O.Slam(cam)
    gpu = StereoSlam(cfg, cfg["width"], cfg["height"])
    if not exact:                      # (exact: nothing is set — the product default is under test)
        gpu.set_fast_solver(True)
    n_kf = 0
    same = 0
    for k in range(n_frames):
        l, r = L[k].numpy(), R[k].numpy()
        made = ref.new_image(l, r, float(ts[k]))
        if on_device:
            gpu.new_image(L[k].cuda(), R[k].cuda(), float(ts[k]))
        else:
            gpu.new_image(l, r, float(ts[k]))
        n_kf += made
        st = gpu.stats()
        assert st.is_keyframe == made, f"frame {k}: keyframe decision"
        ok2, ok3, oinfo = ref.keypoints()
        _compare_frame(f"{config}/{seed} frame {k}", gpu.get_frame(), ok2, ok3, oinfo, ref.pose(), tol)
        if k > 0:
            eq = _same_trace(st, ref.stats(), cfg)
            same += eq
            if exact:
                assert eq, f"{config}/{seed} frame {k}: GN trace differs from the oracle's"
    assert gpu.num_keyframes() == ref.num_keyframes() == n_kf
    for kid in range(n_kf):
        k2, k3, info, pose = ref.keyframe(kid)
        g = gpu.get_keyframe(kid)
        assert np.array_equal(g.kps2d, k2) or np.max(np.abs(g.kps2d - k2)) < 5e-2
        for f in INT_FIELDS + ("color",):
            assert np.array_equal(g.info[f], info[f]), f"keyframe {kid} info.{f}"
        assert np.array_equal(g.info["score"], info["score"]), f"keyframe {kid} score"
        assert np.max(np.abs(g.pose - pose)) < 1e-4
    traj = gpu.get_trajectory()
    assert traj.shape == (n_frames, 6)
    return gpu, ref, same / max(n_frames - 1, 1)


def test_first_frame_keyframe_bit_exact():
    """Frame 0: FAST/edgelet grid detection, merge, SSD depth: all integer work."""
    for config, seed in (("tiny", 0), ("euroc", 0), ("blender", 1), ("econ", 2)):
        cfg, L, R, poses, ts = synth.make_sequence(config, 1, seed, device="cpu")
        ref = O.Slam(util.oracle_camera(cfg))
        ref.new_image(L[0].numpy(), R[0].numpy(), 0.0)
        gpu = StereoSlam(cfg)
        gpu.new_image(L[0].numpy(), R[0].numpy(), 0.0)
        f = gpu.get_frame()
        k2, k3, info = ref.keypoints()
        assert np.array_equal(f.kps2d, k2), config            # detected positions: exact
        assert np.array_equal(f.info["score"], info["score"])
        for fld in INT_FIELDS:
            assert np.array_equal(f.info[fld], info[fld]), (config, fld)
        assert np.array_equal(f.info["color"], info["color"])
        # same float expressions on the same integers: depth init is reproduced exactly
        assert np.array_equal(f.kps3d, k3), config
        assert np.array_equal(f.info["kf_inv_depth"], info["kf_inv_depth"])
        gpu.close()


def test_first_frame_real_image():
    left, right = util.real_pair()
    cfg = dict(synth.CONFIGS["econ"])
    ref = O.Slam(util.oracle_camera(cfg))
    ref.new_image(left, right, 0.0)
    gpu = StereoSlam(cfg)
    gpu.new_image(left, right, 0.0)
    f = gpu.get_frame()
    k2, k3, info = ref.keypoints()
    assert np.array_equal(f.kps2d, k2)
    assert np.array_equal(f.info["type"], info["type"])
    assert np.array_equal(f.kps3d, k3)


@pytest.mark.parametrize("config,n_frames,seed", [("tiny", 12, 0), ("tiny", 12, 3), ("euroc", 8, 0),
                                                  ("econ", 5, 1), ("hd", 3, 0)])
@pytest.mark.parametrize("exact", [False, True])
def test_sequence_matches_oracle(config, n_frames, seed, exact):
    _run(config, n_frames, seed, exact=exact)


def test_sequence_with_keyframe_creation():
    """Fast motion so that keyframe_needed fires inside the sequence (product default solver)."""
    gpu, ref, same = _run("tiny", 30, 1, motion_scale=4.0)
    assert same == 1.0
    assert ref.num_keyframes() >= 2


def test_long_sequence_with_keyframes_at_full_size():
    """Stress case: 60 frames of the C2 configuration at 3x the motion, several keyframes inside the
    sequence. Default (reference-order) mode: feature index lists, flags, counters, poses and points
    equal the oracle's on every frame, every GN trace too."""
    gpu, ref, same = _run("euroc", 60, 5, motion_scale=3.0, exact=True, render_device="cuda")
    assert ref.num_keyframes() >= 3 and same == 1.0


def test_drift_over_300_frames():
    """trajectory drift against the restatement over 300 frames of the C2
    configuration <= 1 mm / 0.01 deg, identical accept / reject trace on >= 99 % of the frames.
    Default mode: no drift at all and every trace identical (asserted frame by frame in _run).
    Fast-solver mode: the drift bound holds; its traces are its own (reported, not asserted)."""
    n = 300
    for exact in (True, False):
        gpu, ref, same = _run("euroc", n, 7, exact=exact, render_device="cuda")
        d = np.abs(gpu.get_trajectory() - np.array([ref.pose()]))[-1]
        drift_t, drift_r = float(np.max(d[:3])), float(np.max(d[3:]))
        print(f"300 frames, exact={exact}: drift {drift_t * 1e3:.4f} mm / {np.degrees(drift_r):.5f} deg, "
              f"{same:.4f} of the frames with the oracle's GN trace, {ref.num_keyframes()} keyframes")
        assert drift_t <= 1e-3 and drift_r <= np.radians(0.01)
        if exact:
            assert same == 1.0 and drift_t == 0.0 and drift_r == 0.0
        gpu.close()


def test_device_resident_input():
    _run("tiny", 5, 2, on_device=True)


def test_batch_equals_single():
    """B sequences through one ctx give the same results as B separate contexts."""
    seqs = [synth.make_sequence("tiny", 6, s, device="cpu") for s in (0, 1, 2)]
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 3)
    singles = [StereoSlam(cfg) for _ in seqs]
    for k in range(6):
        batch.new_images([s[1][k].numpy() for s in seqs], [s[2][k].numpy() for s in seqs],
                         [float(s[4][k]) for s in seqs])
        for i, s in enumerate(seqs):
            singles[i].new_image(s[1][k].numpy(), s[2][k].numpy(), float(s[4][k]))
            a, b = batch.get_frame(i), singles[i].get_frame()
            assert np.array_equal(a.pose, b.pose)
            assert np.array_equal(a.kps2d, b.kps2d) and np.array_equal(a.kps3d, b.kps3d)
            assert np.array_equal(a.info, b.info)


def test_batched_launch_shapes_equal_single(monkeypatch):
    """From 32 sequences per group on, the alignment kernel changes shape (records, per-keypoint
    values and image taps from L2, half as many waves): same arithmetic in the same order, so a
    sequence inside such a group ends bit for bit like a ctx of its own (which the other tests pin
    to the oracle). (Default solver: the fast solver's tree sums depend on the number of waves.)"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n_seq, n_frames = 34, 5
    six = [synth.make_sequence("tiny", n_frames, 40 + s, device="cpu") for s in range(6)]
    seqs = [six[s % 6] for s in range(n_seq)]
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_seq)
    assert batch.groups() == 1
    for k in range(n_frames):
        batch.new_images([s[1][k].numpy() for s in seqs], [s[2][k].numpy() for s in seqs],
                         [float(s[4][k]) for s in seqs])
    for i in (0, 5, 33):
        one = StereoSlam(cfg)
        for k in range(n_frames):
            one.new_image(seqs[i][1][k].numpy(), seqs[i][2][k].numpy(), float(seqs[i][4][k]))
        a, b = batch.get_frame(i), one.get_frame()
        assert np.array_equal(a.pose, b.pose), (i, a.pose, b.pose)
        assert np.array_equal(a.kps2d, b.kps2d) and np.array_equal(a.kps3d, b.kps3d)
        assert np.array_equal(a.info, b.info)
        assert np.array_equal(batch.get_trajectory(i), one.get_trajectory())
        one.close()
    batch.close()


def _oracle_frames(rendered, cfg):
    """The oracle over every rendered sequence, frame by frame, in a thread pool (the oracle's ctypes calls
    release the GIL): per sequence a list of (keyframe made, kps2d, kps3d, info, pose, stats) per frame."""
    from concurrent.futures import ThreadPoolExecutor
    cam = util.oracle_camera(cfg)
    host = [(r[1].cpu().numpy() if torch.is_tensor(r[1]) else np.stack([x.numpy() for x in r[1]]),
             r[2].cpu().numpy() if torch.is_tensor(r[2]) else np.stack([x.numpy() for x in r[2]]),
             r[4]) for r in rendered]

    def one(seq):
        L, R, ts = seq
        ref = O.Slam(cam)
        out = []
        for k in range(len(ts)):
            made = ref.new_image(L[k], R[k], float(ts[k]))
            ok2, ok3, oinfo = ref.keypoints()
            out.append((made, ok2, ok3, oinfo, ref.pose().copy(), ref.stats()))
        ref.close()
        return out

    with ThreadPoolExecutor(min(16, len(host))) as ex:
        return list(ex.map(one, host))


def _batch_against_oracle(rendered, cfg, oracle, n_groups, fast=False):
    """All sequences in one ctx of n_groups groups, borrowed device frames queued with svo_submit_images, one
    frame set at a time. Every sequence on every frame: keyframe decision, feature index lists, flags, counters,
    score, and (reference-order mode) pose, keypoints and GN traces bit for bit; the fast solver: pose within
    1e-4, keypoints within the _compare_frame bounds. Returns the ctx's launch shapes."""
    n_seq, n_frames = len(rendered), len(rendered[0][4])
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_seq)
    assert batch.groups() == n_groups
    if fast:
        batch.set_fast_solver(True)
    torch.cuda.synchronize()
    packs = [batch.pack_images([r[1][k] for r in rendered], [r[2][k] for r in rendered],
                               [float(r[4][k]) for r in rendered], borrow=True) for k in range(n_frames)]
    tol = 1e-4 if fast else 0.0
    for k in range(n_frames):
        batch.submit_packed(packs[k])
        batch.wait()
        for i in range(n_seq):
            made, ok2, ok3, oinfo, pose, ost = oracle[i][k]
            st = batch.stats(i)
            assert st.is_keyframe == made, f"seq {i} frame {k}: keyframe decision"
            _compare_frame(f"seq {i} frame {k}", batch.get_frame(i), ok2, ok3, oinfo, pose, tol)
            if k > 0 and not fast:
                assert _same_trace(st, ost, cfg), f"seq {i} frame {k}: GN trace differs from the oracle's"
    for i in range(n_seq):
        traj = np.array([f[4] for f in oracle[i]])
        if fast:
            assert np.max(np.abs(batch.get_trajectory(i) - traj)) < 1e-4, i
        else:
            assert np.array_equal(batch.get_trajectory(i), traj), i
        assert batch.num_keyframes(i) == sum(f[0] for f in oracle[i]), i
    shapes = batch.launch_shapes()
    batch.close()
    return shapes


def _sia_shapes(shapes):
    return {k[1:]: v for k, v in shapes.items() if k[0] == "sia_gn_kernel"}


def _reproj_shapes(shapes):
    return {k[1:]: v for k, v in shapes.items() if k[0] == "reproj_gn_kernel"}


# C2 in the shape of the headline run: 72 `euroc` sequences in 2 groups of 36, 10 frames at 8x the motion,
# so that keyframes fire inside the run (the sets pass 128 keypoints) after frames whose sets all stay below
C2_BATCH = dict(n_seq=72, groups=2, n_frames=10, motion_scale=8.0)


@pytest.fixture(scope="module")
def c2_batch():
    """rendered sequences and the oracle's frames of the C2 batched run (shared by the exact and fast legs)"""
    p = C2_BATCH
    rendered = [synth.make_sequence_gpu("euroc", p["n_frames"], 100 + s, motion_scale=p["motion_scale"])
                for s in range(p["n_seq"])]
    cfg = rendered[0][0]
    oracle = _oracle_frames(rendered, cfg)
    per_group = p["n_seq"] // p["groups"]
    for g in range(p["groups"]):          # a keyframe inside the run in every group
        assert any(f[0] for o in oracle[g * per_group:(g + 1) * per_group] for f in o[1:]), g
    return rendered, cfg, oracle


def test_batched_c2_shape_in_groups_equals_the_oracle(monkeypatch, c2_batch):
    """The launch shape the headline number runs, pinned to the oracle DIRECTLY: 72 `euroc` sequences in
    2 groups of 36 (sia_gn_kernel<1,2>: one wave per sequence, records and image taps from L2, with cap 128
    and 192, i.e. two and three staging chunks; reproj_gn_kernel<1> with cap 192: three staging steps),
    several groups on their own streams, borrowed device frames queued with svo_submit_images. Every
    sequence's pose, keypoints, flags, counters, GN traces and trajectory equal the oracle's bit for bit
    on every frame."""
    rendered, cfg, oracle = c2_batch
    monkeypatch.setenv("SVO_GROUPS", str(C2_BATCH["groups"]))
    shapes = _batch_against_oracle(rendered, cfg, oracle, C2_BATCH["groups"])
    sia, rp = _sia_shapes(shapes), _reproj_shapes(shapes)
    print("C2 batched launch shapes:", shapes)
    assert set(sia) <= {(1, 2, 64), (1, 2, 128), (1, 2, 192)}, sia
    assert (1, 2, 128) in sia and (1, 2, 192) in sia, sia
    assert all(w == 1 for w, _, _ in rp) and any(cap >= 192 for _, _, cap in rp), rp


def test_batched_c2_fast_solver_stays_with_the_oracle(monkeypatch):
    """The batched C2 shape with the fast solver (tree sums whose order depends on the wave count): 72
    `euroc` sequences in 2 groups at the motion of the earlier form of the C2 test, 6 frames; every pose
    within 1e-4 m / rad of the oracle's, feature index lists equal, on every frame. (The 8x motion of the
    reference-order test above is beyond the fast solver's bound in any shape: one of its sequences ends
    3e-4 away from the oracle in a ctx of its own too. That run pins the reference-order mode only.)"""
    monkeypatch.setenv("SVO_GROUPS", "2")
    rendered = [synth.make_sequence_gpu("euroc", 6, 100 + s, motion_scale=1.5) for s in range(72)]
    cfg = rendered[0][0]
    shapes = _batch_against_oracle(rendered, cfg, _oracle_frames(rendered, cfg), 2, fast=True)
    sia = _sia_shapes(shapes)
    print("C2 batched launch shapes, fast solver:", shapes)
    assert sia and all(w == 1 and m == 2 for w, m, _ in sia) and (1, 2, 128) in sia, sia


def test_batched_two_wave_alignment_equals_the_oracle(monkeypatch):
    """sia_gn_kernel<2,2> (a batched launch whose largest set has 193-384 keypoints) and reproj_gn_kernel<4>
    in a batched launch: 36 `euroc` sequences with a 32 x 32 pixel keypoint grid (345 cells), 3 frames,
    one group; bit for bit against the oracle on every frame."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    rendered = [synth.make_sequence_gpu("euroc", 3, 300 + s, motion_scale=1.5,
                                        overrides=dict(grid_width=32, grid_height=32)) for s in range(36)]
    cfg = rendered[0][0]
    shapes = _batch_against_oracle(rendered, cfg, _oracle_frames(rendered, cfg), 1)
    print("C2 dense-grid launch shapes:", shapes)
    sia, rp = _sia_shapes(shapes), _reproj_shapes(shapes)
    assert sia and all(w == 2 and m == 2 for w, m, _ in sia), sia
    assert rp and all(w == 4 for w, _, _ in rp), rp


def test_batched_c3_equals_the_oracle(monkeypatch):
    """C3 (1920x1080, ~2000 keypoints) in a batched launch: 32 `hd` sequences in one group, 2 frames;
    sia_gn_kernel<4,2> and reproj_gn_kernel<4> at C3's caps (1536-2048 keypoints), bit for bit against the oracle."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    rendered = [synth.make_sequence_gpu("hd", 2, 400 + s) for s in range(32)]
    cfg = rendered[0][0]
    shapes = _batch_against_oracle(rendered, cfg, _oracle_frames(rendered, cfg), 1)
    print("C3 batched launch shapes:", shapes)
    sia, rp = _sia_shapes(shapes), _reproj_shapes(shapes)
    assert sia and all(w == 4 and m == 2 and cap >= 1536 for w, m, cap in sia), sia
    assert rp and all(w == 4 and cap >= 1536 for w, _, cap in rp), rp


def test_shape_switch_when_sequences_finish(monkeypatch):
    """34 `tiny` sequences of unequal length in one group: while 34 are active the alignment runs
    sia_gn_kernel<1,2>; once 30 have finished, the 4 that remain run sia_gn_kernel<1,0>. Every sequence
    ends with the oracle's pose, keypoints, flags, counters, trajectory and GN traces."""
    from stereo_svo_slam_amd import multi_seq
    monkeypatch.setenv("SVO_GROUPS", "1")
    lengths = [3] * 30 + [8] * 4
    seqs = [synth.make_sequence("tiny", n, 500 + s, device="cpu", motion_scale=2.0) for s, n in enumerate(lengths)]
    cfg = seqs[0][0]
    seqs = [(c, L, R, p, np.arange(len(L), dtype=np.float32) / 20.0) for c, L, R, p, _ in seqs]   # play_unequal's times
    oracle = _oracle_frames(seqs, cfg)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], len(lengths))
    assert batch.groups() == 1
    done = multi_seq.play_unequal(batch, lambda s, k: (seqs[s][1][k].numpy(), seqs[s][2][k].numpy()), lengths)
    assert done == sum(lengths)
    for s, n in enumerate(lengths):
        made, ok2, ok3, oinfo, pose, ost = oracle[s][-1]
        _compare_frame(f"seq {s}", batch.get_frame(s), ok2, ok3, oinfo, pose, tol=0.0)
        assert _same_trace(batch.stats(s), ost, cfg), s
        assert np.array_equal(batch.get_trajectory(s), np.array([f[4] for f in oracle[s]])), s
        assert batch.num_keyframes(s) == sum(f[0] for f in oracle[s]), s
    sia = _sia_shapes(batch.launch_shapes())
    batch.close()
    print("unequal lengths launch shapes:", sia)
    assert sia.get((1, 2, 64), 0) == 2 and sia.get((1, 0, 64), 0) == 5, sia


def test_groups_and_pipelined_submit_equal_lockstep(monkeypatch):
    """Sequence groups (own stream + host thread each) and svo_submit_images / svo_wait give
    the results of the single-group, call-per-frame form: 5 sequences as 1 group vs 2 groups
    (3 + 2 sequences), the latter with all frames queued before one wait."""
    import torch
    n_frames = 7
    seqs = [synth.make_sequence("tiny", n_frames, s, device="cpu") for s in range(5)]
    cfg = seqs[0][0]
    monkeypatch.setenv("SVO_GROUPS", "1")
    one = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 5)
    monkeypatch.setenv("SVO_GROUPS", "2")
    two = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 5)
    assert one.groups() == 1 and two.groups() == 2
    dev_l = [[s[1][k].cuda() for s in seqs] for k in range(n_frames)]
    dev_r = [[s[2][k].cuda() for s in seqs] for k in range(n_frames)]
    torch.cuda.synchronize()
    packs = [two.pack_images(dev_l[k], dev_r[k], [float(s[4][k]) for s in seqs]) for k in range(n_frames)]
    for k in range(n_frames):
        one.new_images([s[1][k].numpy() for s in seqs], [s[2][k].numpy() for s in seqs],
                       [float(s[4][k]) for s in seqs])
        two.submit_packed(packs[k])
    two.wait()
    t1, t2 = one.totals(), two.totals()
    detail = [(i, len(one.get_frame(i).kps2d), len(two.get_frame(i).kps2d), one.num_keyframes(i), two.num_keyframes(i),
               len(one.get_keyframe(0, i).kps2d), len(two.get_keyframe(0, i).kps2d)) for i in range(5)]
    assert (t1.frames, t1.keyframes, t1.keypoints) == (t2.frames, t2.keyframes, t2.keypoints), detail
    assert t2.n_groups == 2 and t2.launches == 2 * n_frames and t1.launches == n_frames
    for i in range(5):
        a, b = one.get_frame(i), two.get_frame(i)
        assert np.array_equal(a.pose, b.pose)
        assert np.array_equal(a.kps2d, b.kps2d) and np.array_equal(a.kps3d, b.kps3d)
        assert np.array_equal(a.info, b.info)
        assert np.array_equal(one.get_trajectory(i), two.get_trajectory(i))
        assert one.num_keyframes(i) == two.num_keyframes(i)


def test_failure_in_one_group_latches_the_ctx(monkeypatch):
    """A frame that fails in one sequence group (here: a sequence handed only one of its two images)
    fails the ctx: the wait reports the cause, nothing more is queued on ANY group afterwards, so the
    healthy group's sequences do not run ahead on later submits."""
    from stereo_svo_slam_amd.hip_lib import SvoError
    seqs = [synth.make_sequence("tiny", 3, 30 + s, device="cpu") for s in range(4)]
    cfg = seqs[0][0]
    monkeypatch.setenv("SVO_GROUPS", "2")
    ctx = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 4)
    assert ctx.groups() == 2
    dl = [[s[1][k].cuda() for s in seqs] for k in range(3)]
    dr = [[s[2][k].cuda() for s in seqs] for k in range(3)]
    torch.cuda.synchronize()
    ctx.new_images_packed(ctx.pack_images(dl[0], dr[0], [0.0] * 4))
    bad = ctx.pack_images(dl[1], dr[1], [0.05] * 4)
    bad[1][3] = None                                   # sequence 3 (second group): right image missing
    ctx.submit_packed(bad)
    with pytest.raises(SvoError, match="only one image"):
        ctx.wait()
    frames_after_failure = ctx.totals().frames           # group 0 may have run frame 1, group 1 has not
    assert frames_after_failure in (4, 6)
    with pytest.raises(SvoError, match="earlier frame of this ctx failed"):
        ctx.submit_packed(ctx.pack_images(dl[2], dr[2], [0.1] * 4))
    with pytest.raises(SvoError, match="earlier frame of this ctx failed"):
        ctx.new_images_packed(ctx.pack_images(dl[2], dr[2], [0.1] * 4))
    assert ctx.totals().frames == frames_after_failure
    ctx.close()


def test_klt_template_cache_changes_nothing(monkeypatch):
    """The KLT template cache (a keyframe's templates kept in HBM for the sequence's last keyframes)
    only replaces recomputation by a load: with the cache off, with a ring of one keyframe (every
    new keyframe evicts the previous one, whose points are tracked from the images again) and with
    a ring of four (the default is eight), every frame of a sequence with several keyframes is the same."""
    n_frames = 36
    cfg, L, R, poses, ts = synth.make_sequence("tiny", n_frames, 2, device="cpu", motion_scale=4.0)
    runs = {}
    for k in ("0", "1", "4"):
        monkeypatch.setenv("SVO_KLT_CACHE_KF", k)
        ctx = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
        frames = []
        for i in range(n_frames):
            ctx.new_images([L[i].numpy()], [R[i].numpy()], [float(ts[i])])
            f = ctx.get_frame(0)
            frames.append((f.pose.copy(), f.kps2d.copy(), f.kps3d.copy(), f.info.copy()))
        runs[k] = (frames, ctx.num_keyframes(0))
        ctx.close()
    assert runs["0"][1] == runs["1"][1] == runs["4"][1] >= 3
    for k in ("1", "4"):
        for i, (a, b) in enumerate(zip(runs["0"][0], runs[k][0])):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, i)


@pytest.mark.parametrize("win", [21, 35])
def test_klt_ring_of_three_slots_changes_nothing(monkeypatch, win):
    """The same sequence in three slots of one group whose keyframe ids, and so their places in the template ring,
    differ at every step: slot 1 is restarted after 5 frames and slot 2 after 11, then each runs all 36 frames. With
    the ring off (SVO_KLT_CACHE_KF=0), a ring of one keyframe and a ring of two (every slot makes four keyframes, so
    either ring wraps, at a different step in every slot), in both kernel shapes (window 21: 32 columns, 35: 36
    columns): every frame of every slot is the oracle's and the ring-off run's."""
    n_frames, delays = 36, (0, 5, 11)
    cfg, L, R, poses, ts = synth.make_sequence("tiny", n_frames, 2, device="cpu", motion_scale=4.0,
                                               overrides={"window_size_opt_flow": win})
    L, R = [x.numpy() for x in L], [x.numpy() for x in R]
    ref = O.Slam(util.oracle_camera(cfg))
    oracle = []
    for i in range(n_frames):
        ref.new_image(L[i], R[i], float(ts[i]))
        k2, k3, info = ref.keypoints()
        oracle.append((k2, k3, info, ref.pose()))
    n_kf = ref.num_keyframes()
    assert n_kf >= 3, "the sequence stopped making keyframes: the rings never wrap"
    base = None
    for ring in ("0", "1", "2"):
        monkeypatch.setenv("SVO_KLT_CACHE_KF", ring)
        ctx = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 3)
        assert ctx.groups() == 1
        frames = [[None] * n_frames for _ in delays]
        for step in range(n_frames + max(delays)):
            again = [s for s, d in enumerate(delays) if d and step == d]
            if again:
                ctx.restart(again)
            # (a slot plays the sequence from step 0; its restart makes it begin again)
            at = [step - d if step >= d else step for d in delays]
            live = [k < n_frames for k in at]
            ctx.new_images([L[k] if ok else None for k, ok in zip(at, live)], [R[k] if ok else None for k, ok in zip(at, live)],
                           [float(ts[min(k, n_frames - 1)]) for k in at])
            for s, (k, ok) in enumerate(zip(at, live)):
                if ok and step >= delays[s]:
                    f = ctx.get_frame(s)
                    k2, k3, info, pose = oracle[k]
                    _compare_frame(f"window {win} ring {ring} slot {s} frame {k}", f, k2, k3, info, pose, 0.0)
                    frames[s][k] = (f.pose.copy(), f.kps2d.copy(), f.kps3d.copy(), f.info.copy())
        for s in range(len(delays)):
            assert ctx.num_keyframes(s) == n_kf, (ring, s, ctx.num_keyframes(s))
        ctx.close()
        if base is None:
            base = frames[0]
        for s in range(len(delays)):
            for k in range(n_frames):
                assert all(np.array_equal(x, y) for x, y in zip(base[k], frames[s][k])), (win, ring, s, k)


def test_update_pose_matches_oracle():
    cfg = dict(synth.CONFIGS["tiny"])
    gpu = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    ref = O.Slam(util.oracle_camera(cfg))
    rng = np.random.RandomState(0)
    for i in range(5):
        pose = rng.normal(0, 0.1, 6).astype(np.float32)
        speed = rng.normal(0, 0.1, 6).astype(np.float32)
        pv = np.full(6, 0.1, np.float32)
        sv = np.ones(6, np.float32)
        dt = 0.0 if i % 2 == 0 else 0.05
        a = gpu.update_pose(pose, speed, pv, sv, dt)
        b = ref.update_pose(pose, speed, pv, sv, dt)
        assert np.array_equal(a, b)


def test_sequences_of_unequal_length_share_a_ctx():
    """C4 mechanics: sequences of different lengths in ONE ctx. A sequence whose frames ran out sits
    the remaining steps out (NULL image pointers); every sequence ends exactly like a ctx of its own."""
    from stereo_svo_slam_amd import multi_seq
    lengths = [7, 3, 5, 1]
    seqs = [synth.make_sequence("tiny", n, 10 + s, device="cpu") for s, n in enumerate(lengths)]
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], len(lengths))
    done = multi_seq.play_unequal(batch, lambda s, k: (seqs[s][1][k].numpy(), seqs[s][2][k].numpy()), lengths)
    assert done == sum(lengths) and batch.totals().frames == sum(lengths)
    for s, n in enumerate(lengths):
        one = StereoSlam(cfg)
        for k in range(n):
            one.new_image(seqs[s][1][k].numpy(), seqs[s][2][k].numpy(), k / 20.0)
        a, b = batch.get_frame(s), one.get_frame()
        assert np.array_equal(a.pose, b.pose) and np.array_equal(a.kps2d, b.kps2d)
        assert np.array_equal(a.info, b.info)
        assert batch.get_trajectory(s).shape == (n, 6)
        one.close()
    batch.close()


TWO_RANK_WORKER = r"""
import json, os, sys
sys.path[:0] = [os.path.join(ROOT, "stereo-svo-slam_amd")]
import numpy as np, torch
from stereo_svo_slam_amd import multi_seq, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch
rank, local_rank, world = multi_seq.init_distributed("gloo")
device = torch.device("cuda", 0)                    # both ranks share the one GPU of the box
lengths = [6, 4, 5, 3]
mine = multi_seq.assign_longest_first(lengths, world)[rank]
seqs = {s: synth.make_sequence("tiny", lengths[s], 20 + s, device="cpu") for s in mine}
cfg = dict(synth.CONFIGS["tiny"])
slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], len(mine), 0)
my_len = [lengths[s] for s in mine]
multi_seq._barrier(world, None)
frames = multi_seq.play_unequal(slam, lambda i, k: (seqs[mine[i]][1][k].numpy(), seqs[mine[i]][2][k].numpy()), my_len)
local = [[mine[i], my_len[i]] + [float(v) for v in slam.pose(i)] for i in range(len(mine))]
local += [[-1, 0] + [0.0] * 6] * (2 - len(local))    # fixed-size summaries: two rows per rank
allsum = multi_seq.gather_summaries(local, world, None)
if rank == 0:
    print(json.dumps({"summaries": allsum.tolist()}))
"""


def test_two_ranks_share_the_gpu(tmp_path):
    """The multi-rank path with the HIP ctx in it (the CPU twin in tests/test_host_cpu.py drives the
    oracle): two gloo ranks on the one GPU of the box, sequences of unequal length assigned longest
    first, one all_gather of the per-sequence summaries; every pose equals a single-process run."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "worker.py"
    script.write_text(f"ROOT = {root!r}\n" + TWO_RANK_WORKER)
    port = _free_port()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", port, str(script)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    summ = np.array([r for r in res["summaries"] if r[0] >= 0])
    lengths = [6, 4, 5, 3]
    assert sorted(summ[:, 0].astype(int).tolist()) == [0, 1, 2, 3]
    cfg = dict(synth.CONFIGS["tiny"])
    for row in summ:
        s = int(row[0])
        assert int(row[1]) == lengths[s]
        L = synth.make_sequence("tiny", lengths[s], 20 + s, device="cpu")
        one = StereoSlam(cfg)
        for k in range(lengths[s]):
            one.new_image(L[1][k].numpy(), L[2][k].numpy(), k / 20.0)
        assert np.array_equal(np.float32(row[2:]), one.get_frame().pose)
        one.close()


def test_borrowed_device_frames_equal_copied_ones():
    """SVO_MEM_DEVICE_BORROW: level 0 of the pyramids and the right image alias the caller's device
    images (the reference's own shallow cv::Mat alias); results equal the copying SVO_MEM_DEVICE
    path, keyframes (which keep referring to old frames) included."""
    import torch
    n_frames = 14
    cfg, L, R, poses, ts = synth.make_sequence("tiny", n_frames, 1, device="cpu", motion_scale=4.0)
    dl = [x.cuda() for x in L]
    dr = [x.cuda() for x in R]
    torch.cuda.synchronize()
    a = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    b = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    for k in range(n_frames):
        a.new_images_packed(a.pack_images([dl[k]], [dr[k]], [float(ts[k])]))
        b.new_images_packed(b.pack_images([dl[k]], [dr[k]], [float(ts[k])], borrow=True))
        fa, fb = a.get_frame(0), b.get_frame(0)
        assert np.array_equal(fa.pose, fb.pose) and np.array_equal(fa.kps2d, fb.kps2d)
        assert np.array_equal(fa.info, fb.info)
    assert a.num_keyframes(0) == b.num_keyframes(0) >= 2
    a.close(); b.close()


def test_keyframe_images_are_released_when_no_keypoint_needs_them(monkeypatch):
    """A keyframe's image set is only read for keypoints that came from it; once the frame's keypoints refer to
    younger keyframes only it goes back to the sequence's free list (the reference keeps every keyframe's
    images: memory that grows with the run). Same frames, keyframes and trajectory as with
    SVO_KEEP_KEYFRAME_IMAGES=1 and as the oracle's; fewer image sets allocated."""
    n = 160                                       # a steady turn (0.86 deg per frame): what a keyframe saw leaves the image for good
    cfg = dict(synth.CONFIGS["euroc"])
    scene = synth.Scene(0, "cuda")
    poses = np.zeros((n, 6), np.float32)
    poses[:, 4] = 0.015 * np.arange(n)
    seeds = 7919 + 2 * np.arange(n)
    L = [x.cpu() for x in synth.render_frames_gpu(scene, cfg, poses, False, 1.0, seeds)]
    R = [x.cpu() for x in synth.render_frames_gpu(scene, cfg, poses, True, 1.0, seeds + 1)]
    ts = np.arange(n, dtype=np.float32) / 20.0
    ref = O.Slam(util.oracle_camera(cfg))
    runs = {}
    for keep in ("0", "1"):
        monkeypatch.setenv("SVO_KEEP_KEYFRAME_IMAGES", keep)
        gpu = StereoSlam(cfg, cfg["width"], cfg["height"])
        frames = []
        for k in range(n):
            gpu.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
            if keep == "0":
                ref.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
                ok2, ok3, oinfo = ref.keypoints()
                _compare_frame(f"frame {k}", gpu.get_frame(), ok2, ok3, oinfo, ref.pose(), 0.0)
            f = gpu.get_frame()
            frames.append((f.pose.copy(), f.kps2d.copy(), f.kps3d.copy(), f.info.copy()))
        runs[keep] = (frames, gpu.num_keyframes(), gpu.totals().image_sets, gpu.get_trajectory().copy())
        for kid in range(gpu.num_keyframes()):              # every keyframe is still served, images or not
            k2, k3, info, pose = ref.keyframe(kid)
            g = gpu.get_keyframe(kid)
            assert np.array_equal(g.info["color"], info["color"]) and np.max(np.abs(g.pose - pose)) < 1e-4
        gpu.close()
    (fa, kfa, sets_a, ta), (fb, kfb, sets_b, tb) = runs["0"], runs["1"]
    assert kfa == kfb == ref.num_keyframes() and kfa >= 5, kfa
    assert np.array_equal(ta, tb)
    for a, b in zip(fa, fb):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    print(f"{kfa} keyframes in {n} frames: {sets_a} image sets allocated with release, {sets_b} without")
    assert sets_b >= kfa + 2 and sets_a <= sets_b - 2, (sets_a, sets_b)
