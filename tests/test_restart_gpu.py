"""Sequence lifecycle inside a running ctx (svo_ctx_restart_sequences): a slot that starts late, ends early or
plays one sequence after another gives, for every run, what a fresh tracker gives: compared with one fresh
oracle_py.Slam per run in the default (reference-order) solver, bit for bit (tol = 0.0)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import oracle_py as O
import rectify_ref as RR
import util
from stereo_svo_slam_amd import multi_seq, synth
from stereo_svo_slam_amd.hip_lib import SvoError
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu


def _render(config, n_frames, seed, motion_scale=4.0):
    """(cfg, left frames, right frames, time stamps) of a seeded sequence, numpy / float"""
    cfg, L, R, _, ts = synth.make_sequence(config, n_frames, seed, device="cpu", motion_scale=motion_scale)
    return cfg, [x.numpy() for x in L], [x.numpy() for x in R], [float(t) for t in ts]


def _oracle(seqs, cfg, maps=None):
    """One fresh oracle per sequence: per frame (keyframe made, kps2d, kps3d, info, pose, stats). With maps the
    oracle sees the frames rectified by the restatement (tests/rectify_ref.py)."""
    cam = util.oracle_camera(cfg)

    def one(seq):
        _, L, R, ts = seq
        ref = O.Slam(cam)
        out = []
        for k in range(len(ts)):
            l, r = L[k], R[k]
            if maps is not None:
                l, r = RR.remap_linear(l, *maps[0]), RR.remap_linear(r, *maps[1])
            made = ref.new_image(l, r, ts[k])
            k2, k3, info = ref.keypoints()
            out.append((made, k2, k3, info, ref.pose().copy(), ref.stats()))
        ref.close()
        return out

    with ThreadPoolExecutor(min(16, len(seqs))) as ex:
        return list(ex.map(one, seqs))


def _same_frame(tag, batch, slot, o, k, cfg):
    """slot's current frame == frame k of its run's oracle: keyframe decision, keypoints, info (colours too),
    pose, GN traces"""
    made, k2, k3, info, pose, ost = o[k]
    st = batch.stats(slot)
    assert st.frame_id == k, f"{tag}: frame id {st.frame_id}"
    assert st.is_keyframe == made, f"{tag}: keyframe decision"
    f = batch.get_frame(slot)
    util.compare_frame(tag, f, k2, k3, info, pose, 0.0)
    assert np.array_equal(f.info["color"], info["color"]), f"{tag}: colours"
    if k > 0:
        assert util.same_trace(st, ost, cfg), f"{tag}: GN trace differs from the oracle's"
    return st


def _same_run_end(tag, traj, n_keyframes, o, n):
    assert np.array_equal(traj, np.array([f[4] for f in o[:n]])), f"{tag}: trajectory"
    assert n_keyframes == sum(f[0] for f in o[:n]), f"{tag}: keyframe count"


def _drive(batch, cfg, seqs, oracle, plan, n_steps, ends=None):
    """plan[slot] = [(sequence, first step, frames), ...] in time order. The slot is restarted before the first
    frame of every run but its first, and before step ends[slot] (a run that is not followed by another). Every
    slot with a frame is compared with its run's oracle on every step; at the end every run's trajectory and
    keyframe count: ended runs through finished_runs, the others through the getters.
    Returns per step {slot: (frame_id, is_keyframe)}."""
    ends = ends or {}
    n = batch.n
    record = []
    for t in range(n_steps):
        restart = [slot for slot in range(n) if ends.get(slot) == t or
                   any(j > 0 and first == t for j, (_, first, _) in enumerate(plan[slot]))]
        if restart:
            batch.restart(restart)
        L, R, ts, live = [None] * n, [None] * n, [0.0] * n, {}
        for slot in range(n):
            for s, first, count in plan[slot]:
                if first <= t < first + count:
                    L[slot], R[slot] = seqs[s][1][t - first], seqs[s][2][t - first]
                    ts[slot] = seqs[s][3][t - first]
                    live[slot] = (s, t - first)
        batch.new_images(L, R, ts)
        rec = {}
        for slot, (s, k) in live.items():
            st = _same_frame(f"step {t} slot {slot} seq {s} frame {k}", batch, slot, oracle[s], k, cfg)
            rec[slot] = (st.frame_id, st.is_keyframe)
        record.append(rec)
    for slot in range(n):
        done = batch.finished_runs(slot)
        n_ended = len(plan[slot]) - (0 if slot in ends else 1)
        assert [i.run for i, _ in done] == list(range(n_ended)), (slot, [i.run for i, _ in done])
        for j, (s, first, count) in enumerate(plan[slot]):
            tag = f"slot {slot} run {j} seq {s}"
            if j < n_ended:
                info, traj = done[j]
                assert (info.seq, info.frames) == (slot, count), tag
                assert np.float32(info.last_time_stamp) == np.float32(seqs[s][3][count - 1]), tag
                assert np.array_equal(np.array(info.pose[:], np.float32), oracle[s][count - 1][4]), f"{tag}: final pose"
                _same_run_end(tag, traj, info.keyframes, oracle[s], count)
            else:
                _same_run_end(tag, batch.get_trajectory(slot), batch.num_keyframes(slot), oracle[s], count)
    return record


def _assert_empty(batch, slot):
    """the getters on an empty slot return what a fresh ctx returns"""
    assert np.array_equal(batch.pose(slot), np.zeros(6, np.float32))
    assert len(batch.get_frame(slot).kps2d) == 0 and batch.num_keyframes(slot) == 0
    assert batch.get_trajectory(slot).shape == (0, 6)
    assert bytes(batch.stats(slot)) == bytes(len(bytes(batch.stats(slot))))


def test_mixed_step(monkeypatch):
    """One group, 5 slots: slot 0 runs through, slot 1 is restarted mid-run and plays another sequence, slot 2
    starts at step 3, slot 3 ends early and stays empty, slot 4 is restarted twice. The restarts of slots 1
    and 4 fall on a step at which slot 0 (the sequence of test_sequence_with_keyframe_creation) creates a
    keyframe, so one keyframe batch holds a tracked and two starting slots."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    N = 30
    seqs = [_render("tiny", N, seed) for seed in (1, 11, 12, 13, 14, 15, 16, 17)]
    cfg = seqs[0][0]
    oracle = _oracle(seqs, cfg)
    kf_steps = [k for k in range(2, N - 8) if oracle[0][k][0]]
    assert kf_steps, "the oracle creates a keyframe inside sequence 0"
    T = kf_steps[0]
    plan = [[(0, 0, N)],
            [(1, 0, T), (2, T, N - T)],
            [(3, 3, N - 3)],
            [(4, 0, 5)],
            [(5, 0, T), (6, T, 4), (7, T + 4, N - T - 4)]]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 5)
    assert batch.groups() == 1
    record = _drive(batch, cfg, seqs, oracle, plan, N, ends={3: 5})
    assert record[T][0] == (T, 1) and record[T][1] == (0, 1) and record[T][4] == (0, 1), record[T]
    _assert_empty(batch, 3)
    assert batch.totals().frames == sum(c for p in plan for _, _, c in p)
    batch.close()


def test_batched_shape_across_a_restart(monkeypatch):
    """36 slots in one group; at step 3 six of them start a new sequence, so that step's tracked-frame launches
    hold 30 slots and take the lone shape while every other tracked step holds 36 (sia_gn_kernel<1,2>)."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n_slots, n_steps, at = 36, 6, 3
    seqs = [_render("tiny", n_steps, 500 + s, motion_scale=2.0) for s in range(n_slots + 6)]
    cfg = seqs[0][0]
    oracle = _oracle(seqs, cfg)
    plan = [[(s, 0, n_steps)] for s in range(n_slots)]
    for j, slot in enumerate(range(0, n_slots, 6)):
        plan[slot] = [(slot, 0, at), (n_slots + j, at, n_steps - at)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 1
    _drive(batch, cfg, seqs, oracle, plan, n_steps)
    sia = {k[1:]: v for k, v in batch.launch_shapes().items() if k[0] == "sia_gn_kernel"}
    batch.close()
    print("launch shapes across a restart:", sia)
    # steps 1, 2, 4, 5: 36 tracked slots; step 3: 30; step 0: none (every slot starts)
    assert sia.get((1, 2, 64), 0) == 4 and sia.get((1, 0, 64), 0) == 1 and sum(sia.values()) == 5, sia


def test_pipelined_queue_over_groups(monkeypatch):
    """Three groups, 9 slots, borrowed device frames: 20 sequences of unequal length through play_queue with every
    frame set and every restart queued before one wait."""
    monkeypatch.setenv("SVO_GROUPS", "3")
    lengths = [3 + (7 * s) % 8 for s in range(20)]
    seqs = [_render("tiny", n, 700 + s, motion_scale=2.0) for s, n in enumerate(lengths)]
    cfg = seqs[0][0]
    oracle = _oracle(seqs, cfg)
    dev = [([torch.from_numpy(x).cuda() for x in q[1]], [torch.from_numpy(x).cuda() for x in q[2]]) for q in seqs]
    torch.cuda.synchronize()
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 9)
    assert batch.groups() == 3
    where, done = multi_seq.play_queue(batch, lambda s, k: (dev[s][0][k], dev[s][1][k]), lengths,
                                       time_of=lambda s, k: seqs[s][3][k], pipelined=True, borrow=True)
    assert done == sum(lengths) == batch.totals().frames and sorted(where) == list(range(20))
    runs_of = {slot: max(r for sl, r in where.values() if sl == slot) for slot, _ in where.values()}
    for s, (slot, run) in where.items():
        tag = f"seq {s} slot {slot} run {run}"
        if run == runs_of[slot]:
            _same_frame(tag, batch, slot, oracle[s], lengths[s] - 1, cfg)
            _same_run_end(tag, batch.get_trajectory(slot), batch.num_keyframes(slot), oracle[s], lengths[s])
        else:
            info, traj = batch.finished_runs(slot)[run]
            assert (info.seq, info.run, info.frames) == (slot, run, lengths[s]), tag
            assert np.array_equal(np.array(info.pose[:], np.float32), oracle[s][-1][4]), tag
            _same_run_end(tag, traj, info.keyframes, oracle[s], lengths[s])
    batch.close()


@pytest.mark.parametrize("cache", ["0", "1", "4", None])
def test_memory_is_bounded_and_stale_cache_entries_are_harmless(monkeypatch, cache):
    """The 36-frame sequence of test_klt_template_cache_changes_nothing (>= 3 keyframes) five times through one
    slot: runs 2-5 repeat run 1 bit for bit whatever the template-cache ring holds from the run before, and the
    ctx owns after each of them what it owned after run 1."""
    if cache is None:
        monkeypatch.delenv("SVO_KLT_CACHE_KF", raising=False)
    else:
        monkeypatch.setenv("SVO_KLT_CACHE_KF", cache)
    n_frames = 36
    cfg, L, R, ts = _render("tiny", n_frames, 2)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    runs, mem = [], []
    for run in range(5):
        frames = []
        for i in range(n_frames):
            batch.new_images([L[i]], [R[i]], [ts[i]])
            f = batch.get_frame(0)
            frames.append((f.pose.copy(), f.kps2d.copy(), f.kps3d.copy(), f.info.copy()))
        assert batch.num_keyframes(0) >= 3
        runs.append((frames, batch.num_keyframes(0), batch.get_trajectory(0)))
        m = batch.memory()
        mem.append((m.device_bytes, m.image_sets, m.keyframe_slabs))
        batch.restart([0])
    for run in range(1, 5):
        assert runs[run][1] == runs[0][1] and np.array_equal(runs[run][2], runs[0][2]), run
        for i, (a, b) in enumerate(zip(runs[0][0], runs[run][0])):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (run, i)
        assert mem[run] == mem[0], (run, mem)
    m = batch.memory()
    assert m.keyframe_slabs_free == m.keyframe_slabs and m.image_sets_free == m.image_sets, \
        (m.keyframe_slabs_free, m.keyframe_slabs, m.image_sets_free, m.image_sets)
    assert m.device_bytes == mem[0][0] and m.klt_cache_bytes <= m.device_bytes
    assert (m.klt_cache_bytes == 0) == (cache == "0")
    assert len(batch.finished_runs(0)) == 5
    batch.close()


def test_borrowed_frames_are_let_go():
    """Borrowed device frames of run A are overwritten with noise once the restart has been processed; run B in
    the same slot equals B's oracle."""
    n = 10
    seqs = [_render("tiny", n, 40), _render("tiny", n, 41)]
    cfg = seqs[0][0]
    oracle = _oracle(seqs, cfg)
    dev = [([torch.from_numpy(x).cuda() for x in q[1]], [torch.from_numpy(x).cuda() for x in q[2]]) for q in seqs]
    torch.cuda.synchronize()
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    submit = lambda L, R, ts: batch.new_images_packed(batch.pack_images(L, R, ts, borrow=True))
    for k in range(n):
        submit([dev[0][0][k]], [dev[0][1][k]], [seqs[0][3][k]])
        _same_frame(f"run A frame {k}", batch, 0, oracle[0], k, cfg)
    assert any(f[0] for f in oracle[0][1:]), "run A has a keyframe of its own besides frame 0"
    batch.restart([0])
    batch.wait()
    for t in dev[0][0] + dev[0][1]:
        t.random_(0, 256)
    torch.cuda.synchronize()
    for k in range(n):
        submit([dev[1][0][k]], [dev[1][1][k]], [seqs[1][3][k]])
        _same_frame(f"run B frame {k}", batch, 0, oracle[1], k, cfg)
    _same_run_end("run B", batch.get_trajectory(0), batch.num_keyframes(0), oracle[1], n)
    batch.close()


def test_restart_with_rectification(monkeypatch):
    """Rectification on: a slot restarted mid-run equals the oracle on rectified frames, the first frame of the
    new run included, next to a slot that tracks on."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n = 10
    seqs = [_render("tiny", n, 60 + s) for s in range(3)]
    cfg = seqs[0][0]
    w, h = cfg["width"], cfg["height"]
    maps = (RR.euroc_like_maps(w, h, angle=0.012, shift=(1.5, -2.0)),
            RR.euroc_like_maps(w, h, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068))
    oracle = _oracle(seqs, cfg, maps)
    batch = StereoSlamBatch(cfg, w, h, 2)
    batch.set_rectification(*maps)
    _drive(batch, cfg, seqs, oracle, [[(0, 0, n)], [(1, 0, 4), (2, 4, n - 4)]], n)
    batch.close()


def test_pose_filter_after_restart():
    """update_pose on a restarted slot runs on a new filter (as test_update_pose_matches_oracle on a fresh ctx)"""
    cfg, L, R, ts = _render("tiny", 4, 5)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    rng = np.random.RandomState(0)

    def updates(ref):
        for i in range(5):
            pose = rng.normal(0, 0.1, 6).astype(np.float32)
            speed = rng.normal(0, 0.1, 6).astype(np.float32)
            pv, sv = np.full(6, 0.1, np.float32), np.ones(6, np.float32)
            dt = 0.0 if i % 2 == 0 else 0.05
            assert np.array_equal(batch.update_pose(pose, speed, pv, sv, dt), ref.update_pose(pose, speed, pv, sv, dt))

    for k in range(4):
        batch.new_images([L[k]], [R[k]], [ts[k]])
    used = batch.update_pose(np.ones(6, np.float32), np.ones(6, np.float32), np.full(6, 0.1, np.float32),
                             np.ones(6, np.float32), 0.05)
    assert np.any(used != 0)                                # the old run's filter has moved
    batch.restart([0])
    updates(O.Slam(util.oracle_camera(cfg)))
    batch.close()


def test_edges(monkeypatch):
    """Bad index, restarts of empty slots, getters on an emptied slot, drop_finished_runs, a failed ctx."""
    monkeypatch.setenv("SVO_GROUPS", "2")
    n = 4
    seqs = [_render("tiny", n, 80 + s) for s in range(4)]
    cfg = seqs[0][0]
    oracle = _oracle(seqs, cfg)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 4)
    assert batch.groups() == 2
    batch.restart([0, 3])                                   # a fresh ctx: every slot is empty
    assert all(batch.finished_runs(s) == [] for s in range(4))
    for bad in ([4], [-1], [0, 99]):
        with pytest.raises(SvoError):
            batch.restart(bad)
    step = lambda k: batch.new_images([q[1][k] for q in seqs], [q[2][k] for q in seqs], [q[3][k] for q in seqs])
    step(0)
    step(1)
    with pytest.raises(SvoError):
        batch.restart([1, 4])                               # nothing queued: slot 1 goes on
    batch.restart([2])
    batch.restart([2])                                      # double restart: one record
    batch.restart([2, 2])
    assert [len(batch.finished_runs(s)) for s in range(4)] == [0, 0, 1, 0]
    _assert_empty(batch, 2)
    mem = batch.memory()
    assert mem.image_sets_free > 0 and mem.keyframe_slabs_free < mem.keyframe_slabs
    batch.new_images([q[1][2] if s != 2 else None for s, q in enumerate(seqs)],
                     [q[2][2] if s != 2 else None for s, q in enumerate(seqs)], [q[3][2] for q in seqs])
    _assert_empty(batch, 2)                                 # NULL images keep it empty
    for s in (0, 1, 3):
        _same_frame(f"slot {s}", batch, s, oracle[s], 2, cfg)
    info, traj = batch.finished_runs(2)[0]
    assert (info.seq, info.run, info.frames) == (2, 0, 2)
    _same_run_end("slot 2 run 0", traj, info.keyframes, oracle[2], 2)
    batch.drop_finished_runs(2)
    assert batch.finished_runs(2) == []
    batch.restart([0])
    batch.drop_finished_runs()
    assert all(batch.finished_runs(s) == [] for s in range(4))
    # a failed ctx rejects restarts (as test_failure_in_one_group_latches_the_ctx fails one)
    dl = [torch.from_numpy(q[1][3]).cuda() for q in seqs]
    dr = [torch.from_numpy(q[2][3]).cuda() for q in seqs]
    torch.cuda.synchronize()
    bad = batch.pack_images(dl, dr, [q[3][3] for q in seqs])
    bad[1][3] = None
    batch.submit_packed(bad)
    with pytest.raises(SvoError, match="only one image"):
        batch.wait()
    with pytest.raises(SvoError, match="earlier frame of this ctx failed"):
        batch.restart([1])
    batch.close()


def test_start_beside_a_tracked_frame_at_euroc_size(monkeypatch):
    """The 752x480 kernel shapes: two slots, 16 steps, slot 1 restarted after 8 frames."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    seqs = [_render("euroc", 16, 0, motion_scale=2.0), _render("euroc", 8, 1, motion_scale=2.0),
            _render("euroc", 8, 2, motion_scale=2.0)]
    cfg = seqs[0][0]
    oracle = _oracle(seqs, cfg)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 2)
    record = _drive(batch, cfg, seqs, oracle, [[(0, 0, 16)], [(1, 0, 8), (2, 8, 8)]], 16)
    assert record[8][0][0] == 8 and record[8][1] == (0, 1)
    batch.close()
