"""The batched one-wave alignment shape (sia_gn_kernel<1,2>) stages the rows of its ordered accumulation in chunks
of 32 keypoints, two per 64-keypoint pass, every lane staging half of a keypoint's rows. These runs pin it to the
oracle with keypoint counts on both sides of every chunk boundary."""
import numpy as np
import pytest
import torch

from stereo_svo_slam_amd import synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam, StereoSlamBatch
from test_tracker_gpu import _batch_against_oracle, _oracle_frames, _sia_shapes

pytestmark = pytest.mark.gpu

# 36 `euroc` sequences in one group, 10 frames at 8x the motion (keyframes fire inside the run, the sets pass 128
# keypoints). Seeds chosen with the oracle alone so that conditions (a)-(c) below hold; rendered on the CPU, whose
# frames the choice was made on.
CHUNKS_BATCH = dict(n_seq=36, first_seed=300, n_frames=10, motion_scale=8.0)


def test_chunks_of_32_keypoints_in_the_batched_shape_equal_the_oracle(monkeypatch):
    """Every (sequence, frame) of the run: keyframe decision, pose, keypoints, info and GN trace equal the oracle's
    bit for bit (_batch_against_oracle of test_tracker_gpu.py, nothing skipped). Before the GPU runs, the ORACLE's
    keypoint counts n of the tracked frames (what estimate_pose is given after remove_outliers) must show that the
    run exercises the chunking: (a) n = 0, 1 and 31 (mod 32) occur, (b) a launch holds sequences with different
    numbers of 32-keypoint chunks, (c) launches with cap 128 and with cap 192 occur (the cap of a launch is the
    largest set of its sequences' previous frames, in whole 64-keypoint passes)."""
    p = CHUNKS_BATCH
    rendered = []
    for s in range(p["n_seq"]):
        cfg, L, R, poses, ts = synth.make_sequence("euroc", p["n_frames"], p["first_seed"] + s, device="cpu",
                                                   motion_scale=p["motion_scale"])
        rendered.append((cfg, torch.stack(L).cuda(), torch.stack(R).cuda(), poses, ts))
    cfg = rendered[0][0]
    oracle = _oracle_frames(rendered, cfg)

    tracked = range(1, p["n_frames"])
    n = np.array([[oracle[i][k][5].n_tracked for k in tracked] for i in range(p["n_seq"])])      # [sequence, frame]
    before = np.array([[len(oracle[i][k - 1][1]) for k in tracked] for i in range(p["n_seq"])])  # sets of frame k - 1
    caps = (before.max(axis=0) + 63) // 64 * 64
    chunks = (n + 31) // 32
    print("alignment keypoint counts, min / max per frame:", n.min(axis=0), n.max(axis=0))
    print("residues mod 32 (count):", {r: int((n % 32 == r).sum()) for r in (0, 1, 31)})
    print("32-keypoint chunks per launch:", [sorted(set(c)) for c in chunks.T], "caps:", caps)
    for r in (0, 1, 31):
        assert (n % 32 == r).any(), f"(a) no tracked frame with n = {r} (mod 32)"
    assert any(len(set(c)) > 1 for c in chunks.T), "(b) every launch has sequences of one chunk count"
    assert 128 in caps and 192 in caps, f"(c) caps {caps}"

    monkeypatch.setenv("SVO_GROUPS", "1")
    shapes = _batch_against_oracle(rendered, cfg, oracle, 1)
    sia = _sia_shapes(shapes)
    print("launch shapes:", shapes)
    assert set(sia) <= {(1, 2, 128), (1, 2, 192)}, sia
    assert (1, 2, 128) in sia and (1, 2, 192) in sia, sia


def test_one_and_two_chunks_in_the_batched_shape_equal_single_contexts(monkeypatch):
    """Small sets (n <= 64: one or two chunks, the second one short or empty) do not occur in `euroc`: 34 `tiny`
    sequences in one group (sia_gn_kernel<1,2>, cap 64) against contexts of their own (the lone-sequence shapes,
    which stage 64 keypoints at a time and are pinned to the oracle by the other tests), every frame of every
    distinct sequence bit for bit. The counts are printed; no condition is attached to them."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n_seq, n_frames, n_distinct = 34, 8, 8
    distinct = [synth.make_sequence("tiny", n_frames, 60 + s, device="cpu") for s in range(n_distinct)]
    seqs = [distinct[s % n_distinct] for s in range(n_seq)]
    cfg = seqs[0][0]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_seq)
    assert batch.groups() == 1
    check = list(range(n_distinct)) + [n_seq - 1]
    singles = {i: StereoSlam(cfg) for i in check}
    counts = []
    for k in range(n_frames):
        batch.new_images([s[1][k].numpy() for s in seqs], [s[2][k].numpy() for s in seqs],
                         [float(s[4][k]) for s in seqs])
        for i in check:
            singles[i].new_image(seqs[i][1][k].numpy(), seqs[i][2][k].numpy(), float(seqs[i][4][k]))
            a, b = batch.get_frame(i), singles[i].get_frame()
            assert np.array_equal(a.pose, b.pose), (i, k, a.pose, b.pose)
            assert np.array_equal(a.kps2d, b.kps2d) and np.array_equal(a.kps3d, b.kps3d), (i, k)
            assert np.array_equal(a.info, b.info), (i, k)
        counts.append([len(batch.get_frame(i).kps2d) for i in check[:n_distinct]])
    print("keypoints per frame (rows) and distinct sequence (columns):")
    print(np.array(counts))
    for i in check:
        assert np.array_equal(batch.get_trajectory(i), singles[i].get_trajectory()), i
        singles[i].close()
    sia = _sia_shapes(batch.launch_shapes())
    print("launch shapes:", sia)
    assert sia and all((w, m) == (1, 2) for w, m, _ in sia), sia
    batch.close()
