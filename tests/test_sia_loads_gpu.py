"""The batched alignment shapes (MODE 2: sia_gn_kernel<1,2>, <4,2>) ask for everything a pass reads of its keypoint at
once and whatever the slot holds: the active flag, the point and the 16 records of a pass of cost() a pass ahead, those
of a pass of get_gradient together with its image taps; one wave keeps the projections in registers between the two.
What was loaded for an inactive or padded slot is dropped. These runs pin that to the oracle with inactive slots
between active ones, passes that hold nothing but padding, and keypoint counts on both sides of a 64-keypoint pass."""
import numpy as np
import pytest
import torch

from stereo_svo_slam_amd import synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam, StereoSlamBatch
from test_tracker_gpu import _batch_against_oracle, _oracle_frames, _sia_shapes

pytestmark = pytest.mark.gpu

# 36 `euroc` sequences in one group, 8 frames at 8x the motion (keyframes fire inside the run, the sets pass 128
# keypoints). Seeds chosen with the oracle alone so that conditions (a)-(c) below hold; rendered on the CPU, whose
# frames the choice was made on.
LOADS_BATCH = dict(seeds=list(range(300, 330)) + [346, 365, 367, 378, 382, 386], n_frames=8, motion_scale=8.0)


def _holes(info_before, n):
    """The flags of the first n keypoints the alignment of a frame is given (the previous frame's, without the ones
    remove_outliers drops): is a keypoint with SVO_IGNORE_TEMPORARY followed by one without?"""
    keep = ~info_before["ignore_completely"].astype(bool)
    temporary = info_before["ignore_temporary"].astype(bool)[keep][:n]
    return bool(temporary.any() and (~temporary[int(np.argmax(temporary)):]).any())


def test_batched_loads_of_inactive_and_padded_slots_equal_the_oracle(monkeypatch):
    """Every (sequence, frame) of the run: keyframe decision, pose, keypoints, info and GN trace equal the oracle's
    bit for bit (_batch_against_oracle of test_tracker_gpu.py, nothing skipped). Before the GPU runs, the ORACLE's
    tracked frames must show that the run exercises the loads: (a) a frame whose first n keypoints (n: what
    estimate_pose is given after remove_outliers) hold one with SVO_IGNORE_TEMPORARY in front of one without — an
    inactive slot between active ones; (b) a launch with a sequence whose n ends a whole 64-keypoint pass or more
    below the launch's cap (the largest set of the sequences' previous frames, in whole passes) — a pass of nothing
    but dropped loads; (c) a frame with n = 0 and one with n = 1 (mod 64)."""
    p = LOADS_BATCH
    rendered = []
    for seed in p["seeds"]:
        cfg, L, R, poses, ts = synth.make_sequence("euroc", p["n_frames"], seed, device="cpu",
                                                   motion_scale=p["motion_scale"])
        rendered.append((cfg, torch.stack(L).cuda(), torch.stack(R).cuda(), poses, ts))
    cfg = rendered[0][0]
    n_seq = len(rendered)
    assert n_seq >= 32
    oracle = _oracle_frames(rendered, cfg)

    tracked = range(1, p["n_frames"])
    n = np.array([[oracle[i][k][5].n_tracked for k in tracked] for i in range(n_seq)])            # [sequence, frame]
    active = np.array([[oracle[i][k][5].n_active for k in tracked] for i in range(n_seq)])
    before = np.array([[len(oracle[i][k - 1][1]) for k in tracked] for i in range(n_seq)])        # sets of frame k - 1
    holes = np.array([[_holes(oracle[i][k - 1][3], oracle[i][k][5].n_tracked) for k in tracked] for i in range(n_seq)])
    caps = (before.max(axis=0) + 63) // 64 * 64
    passes = (n + 63) // 64 * 64
    print("alignment keypoint counts, min / max per frame:", n.min(axis=0), n.max(axis=0), "caps:", caps)
    print("frames with inactive keypoints:", int((active < n).sum()), "of them with one between active ones:",
          int(holes.sum()))
    print("residues mod 64 (count):", {r: int((n % 64 == r).sum()) for r in (0, 1)})
    print("sequences a whole pass or more below their launch's cap, per frame:", (passes + 64 <= caps[None, :]).sum(axis=0))
    assert holes.any(), "(a) no tracked frame with an inactive keypoint in front of an active one"
    assert (passes + 64 <= caps[None, :]).any(), "(b) no sequence ends a whole pass below its launch's cap"
    for r in (0, 1):
        assert (n % 64 == r).any(), f"(c) no tracked frame with n = {r} (mod 64)"

    monkeypatch.setenv("SVO_GROUPS", "1")
    shapes = _batch_against_oracle(rendered, cfg, oracle, 1)
    sia = _sia_shapes(shapes)
    print("launch shapes:", shapes)
    assert sia and set(sia) <= {(1, 2, 128), (1, 2, 192)}, sia


@pytest.mark.parametrize("restart_at", [None, 4], ids=["straight", "restart"])
def test_one_pass_batched_shape_equals_single_contexts(monkeypatch, restart_at):
    """Sets of at most 64 keypoints (one pass, no load a pass ahead) do not occur in `euroc`: 34 `tiny` sequences in
    one group (sia_gn_kernel<1,2>, cap 64) against contexts of their own (the lone-sequence shapes, which read
    LDS and are pinned to the oracle by the other tests), every frame of every distinct sequence bit for bit. With
    restart_at two slots start a new sequence at that step (svo_ctx_restart_sequences), as two fresh contexts do:
    that step's launch holds the 32 others, and the new sequences' first tracked frames run beside sets that have
    been thinned for frames."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n_seq, n_frames, n_distinct = 34, 8, 8
    distinct = [synth.make_sequence("tiny", n_frames, 60 + s, device="cpu") for s in range(n_distinct)]
    seqs = [distinct[s % n_distinct] for s in range(n_seq)]
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_seq)
    assert batch.groups() == 1
    check = list(range(n_distinct)) + [n_seq - 1]
    restarted = [1, n_seq - 1]
    singles = {i: StereoSlam(cfg) for i in check}
    counts = []
    for k in range(n_frames):
        if k == restart_at:
            batch.restart(restarted)
            for i in restarted:
                singles[i].close()
                singles[i] = StereoSlam(cfg)
        batch.new_images([s[1][k].numpy() for s in seqs], [s[2][k].numpy() for s in seqs],
                         [float(s[4][k]) for s in seqs])
        for i in check:
            singles[i].new_image(seqs[i][1][k].numpy(), seqs[i][2][k].numpy(), float(seqs[i][4][k]))
            a, b = batch.get_frame(i), singles[i].get_frame()
            assert np.array_equal(a.pose, b.pose), (i, k, a.pose, b.pose)
            assert np.array_equal(a.kps2d, b.kps2d) and np.array_equal(a.kps3d, b.kps3d), (i, k)
            assert np.array_equal(a.info, b.info), (i, k)
        counts.append([len(batch.get_frame(i).kps2d) for i in check])
    print("keypoints per frame (rows) and checked slot (columns):")
    print(np.array(counts))
    for i in check:
        assert np.array_equal(batch.get_trajectory(i), singles[i].get_trajectory()), i
        singles[i].close()
    sia = _sia_shapes(batch.launch_shapes())
    print("launch shapes:", sia)
    assert sia and set(sia) == {(1, 2, 64)}, sia
    batch.close()
