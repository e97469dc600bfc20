"""Save and load of a slot's sequence state (svo_submit_save / svo_submit_load): a sequence saved after frame k
and loaded into another slot, ctx, group layout or template-ring size gives from frame k+1 on the frames of a
fresh oracle_py.Slam that saw the whole sequence, bit for bit (tol = 0.0, traces compared); and the copy kernel
alone (svo_copy_segments) against numpy."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import oracle_py as O
import snapshot_ref as SR
import util
from stereo_svo_slam_amd import hip_lib, multi_seq, synth
from stereo_svo_slam_amd.hip_lib import SvoError
from stereo_svo_slam_amd.stereo_slam import Snapshot, StereoSlamBatch

pytestmark = pytest.mark.gpu

N = 50
MAIN, SIDE = 12, 11                      # seeds: the main sequence, and the one that runs beside it
KEYFRAMES = [0, 6, 14, 21, 28, 35, 41, 48]


class World:
    """The two sequences (numpy frames), their oracles — per frame (keyframe made, kps2d, kps3d, info, pose,
    stats) — and what the tests share."""

    def __init__(self):
        self.seq = {}
        for seed in (MAIN, SIDE):
            cfg, L, R, _, ts = synth.make_sequence("tiny", N, seed, device="cpu", motion_scale=8.0)
            self.seq[seed] = ([x.numpy() for x in L], [x.numpy() for x in R], [float(t) for t in ts])
        self.cfg = cfg
        cam = util.oracle_camera(cfg)

        def one(seed):
            L, R, ts = self.seq[seed]
            ref = O.Slam(cam)
            out = []
            for k in range(N):
                made = ref.new_image(L[k], R[k], ts[k])
                k2, k3, info = ref.keypoints()
                out.append((made, k2, k3, info, ref.pose().copy(), ref.stats()))
            ref.close()
            return out

        with ThreadPoolExecutor(2) as ex:
            self.oracle = dict(zip((MAIN, SIDE), ex.map(one, (MAIN, SIDE))))
        self._saved = {}

    def frames(self, seed, k):
        L, R, ts = self.seq[seed]
        return L[k], R[k], ts[k]

    def saved(self, k, cache=None, monkeypatch=None):
        """(host part, data part) bytes of the main sequence saved after frame k in a 1-slot ctx made under
        SVO_KLT_CACHE_KF = cache, host mode; made once"""
        if (k, cache) not in self._saved:
            _set_cache(monkeypatch, cache)
            src = StereoSlamBatch(self.cfg, self.cfg["width"], self.cfg["height"], 1)
            _play(self, src, {0: MAIN}, 0, k + 1)
            snap = src.save([0])[0]
            src.close()
            self._saved[(k, cache)] = (snap.host.tobytes(), snap.data.tobytes())
        host, data = self._saved[(k, cache)]
        return Snapshot(np.frombuffer(host, np.uint8).copy(), np.frombuffer(data, np.uint8).copy())


@pytest.fixture(scope="module")
def world():
    w = World()
    o = w.oracle[MAIN]
    # what the cases below rely on; a changed renderer fails here instead of leaving a case unreached
    assert [k for k in range(N) if o[k][0]] == KEYFRAMES
    origin = [sorted(set(f[3]["keyframe_id"].tolist())) for f in o]
    assert origin[39] == [0, 1, 2, 3, 4, 5] and origin[40] == [0, 2, 3, 4, 5], "frame 40: keyframe 1 retired while 0 is live"
    assert origin[43] == [0, 2, 3, 4, 5, 6] and all(origin[k] == [2, 3, 4, 5, 6] for k in range(44, 48)), origin[43:48]
    assert all(min(origin[k]) == 2 for k in range(44, N)), "from frame 44 on keyframes 0 and 1 are both gone"
    assert min(len(f[1]) for f in o) >= 33
    return w


def _set_cache(monkeypatch, cache):
    if monkeypatch is None:
        return
    if cache is None:
        monkeypatch.delenv("SVO_KLT_CACHE_KF", raising=False)
    else:
        monkeypatch.setenv("SVO_KLT_CACHE_KF", cache)


def _same_frame(w, tag, batch, slot, seed, k):
    """slot's current frame == frame k of the oracle: keyframe decision, keypoints, info (colours too), pose, traces"""
    made, k2, k3, info, pose, ost = w.oracle[seed][k]
    st = batch.stats(slot)
    assert st.frame_id == k, f"{tag}: frame id {st.frame_id}"
    assert st.is_keyframe == made, f"{tag}: keyframe decision"
    f = batch.get_frame(slot)
    util.compare_frame(tag, f, k2, k3, info, pose, 0.0)
    assert np.array_equal(f.info["color"], info["color"]), f"{tag}: colours"
    if k > 0:
        assert util.same_trace(st, ost, w.cfg), f"{tag}: GN trace differs from the oracle's"


def _same_run_end(w, tag, batch, slot, seed, n):
    o = w.oracle[seed]
    assert np.array_equal(batch.get_trajectory(slot), np.array([f[4] for f in o[:n]])), f"{tag}: trajectory"
    assert batch.num_keyframes(slot) == sum(f[0] for f in o[:n]), f"{tag}: keyframe count"


def _play(w, batch, slots, first, end, check=True, offsets=None, feed=None):
    """frames [first, end) of seed slots[slot] into every slot named (the others get None); offsets[slot]: that
    slot plays frame k - offsets[slot] at step k. Every frame is compared with the oracle."""
    offsets = offsets or {}
    for k in range(first, end):
        L, R, ts = [None] * batch.n, [None] * batch.n, [0.0] * batch.n
        for slot, seed in slots.items():
            if 0 <= k - offsets.get(slot, 0) < N:
                L[slot], R[slot], ts[slot] = w.frames(seed, k - offsets.get(slot, 0))
        (feed or batch.new_images)(L, R, ts)
        for slot, seed in slots.items():
            if check and L[slot] is not None:
                _same_frame(w, f"step {k} slot {slot}", batch, slot, seed, k - offsets.get(slot, 0))


def _state(batch, slot):
    """everything the getters return for the slot, as comparable values"""
    f = batch.get_frame(slot)
    kfs = batch.get_keyframes(slot)
    return dict(pose=batch.pose(slot).tobytes(), stats=bytes(batch.stats(slot)), trajectory=batch.get_trajectory(slot).tobytes(),
                frame=(f.pose.tobytes(), f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes()),
                keyframes=[(k.pose.tobytes(), k.kps2d.tobytes(), k.kps3d.tobytes(), k.info.tobytes()) for k in kfs])


@pytest.mark.parametrize("k", [0, 1, 6, 7, 40, 45])
def test_resume_equals_uninterrupted(world, k):
    """Saved after frame k in a 1-slot ctx (host mode), loaded into slot 2 of a fresh 3-slot ctx: the getters
    return what they returned at the source, and frames k+1 .. 49 equal the oracle's while slot 0 runs another
    sequence from its frame 0 and slot 1 stays empty. k = 0, 6: saved on a keyframe (it shares the current image
    set); 40: keyframe 1 retired while 0 is live; 45: two retired."""
    w = world
    cfg = w.cfg
    src = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    _play(w, src, {0: MAIN}, 0, k + 1, check=False)
    _same_frame(w, f"source frame {k}", src, 0, MAIN, k)
    snap = src.save([0])[0]
    info = snap.info
    ref = SR.parse(snap.host)
    n_kf = sum(1 for f in KEYFRAMES if f <= k)
    assert (info.frame_id, info.n_keyframes, info.n_trajectory) == (k, n_kf, k + 1)
    assert (info.host_bytes, info.data_bytes) == (snap.host.size, snap.data.size) == src.snapshot_size(0)
    assert info.keyframes_retired == {40: 0, 45: 2}.get(k, info.keyframes_retired)
    if k == 40:
        assert [s for _, _, s in ref["keyframes"]].count(-1) == 1 and ref["keyframes"][1][2] == -1 and ref["keyframes"][0][2] > 0
    if k in (0, 6):
        assert ref["keyframes"][-1][2] == 0, "a keyframe made on the current frame shares its image set"
    assert ref["n_image_sets"] == len({s for _, _, s in ref["keyframes"] if s >= 0} | {0})
    assert np.array_equal(ref["trajectory"], src.get_trajectory(0)) and ref["pose"].tobytes() == src.pose(0).tobytes()
    state = _state(src, 0)
    src.close()

    dst = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 3)
    dst.load([2], [snap])
    assert _state(dst, 2) == state
    assert dst.finished_runs(2) == [] and dst.stats(1).frame_id == 0 and dst.num_keyframes(1) == 0
    _play(w, dst, {0: SIDE, 2: MAIN}, k + 1, N, offsets={0: k + 1})
    _same_run_end(w, "restored", dst, 2, MAIN, N)
    _same_run_end(w, "beside it", dst, 0, SIDE, N - k - 1)
    assert dst.get_trajectory(1).shape == (0, 6)
    assert dst.totals().frames == 2 * (N - k - 1)            # frames count where they ran
    dst.close()


def test_device_mode_with_borrowed_frames(world):
    """The source tracks borrowed device frames whose row pitch is not the width; the save goes into a torch
    tensor; the borrowed buffers are overwritten and the source ctx destroyed before the load."""
    w = world
    cfg = w.cfg
    W, H, k = cfg["width"], cfg["height"], 22
    L, R, ts = w.seq[MAIN]

    def on_device(images):
        buf = torch.zeros((len(images), H, W + 24), dtype=torch.uint8, device="cuda")
        buf[:, :, :W] = torch.from_numpy(np.stack(images)).cuda()
        return buf

    bl, br = on_device(L), on_device(R)
    torch.cuda.synchronize()

    def feed_to(batch):
        def feed(Ls, Rs, t):
            i = int(round(t[0] * 20))
            batch.new_images_packed(batch.pack_images([bl[i, :, :W]], [br[i, :, :W]], t, borrow=True))
        return feed

    src = StereoSlamBatch(cfg, W, H, 1)
    _play(w, src, {0: MAIN}, 0, k + 1, feed=feed_to(src))
    snap = src.save([0], device=True)[0]
    assert snap.data.is_cuda and snap.info.frame_id == k
    bl[:k + 1].random_(0, 256)
    br[:k + 1].random_(0, 256)
    torch.cuda.synchronize()
    src.close()
    dst = StereoSlamBatch(cfg, W, H, 1)
    dst.load([0], [snap])
    _same_frame(w, "loaded", dst, 0, MAIN, k)
    snap.data.random_(0, 256)                                  # the slot has its own copies
    _play(w, dst, {0: MAIN}, k + 1, N, feed=feed_to(dst))
    _same_run_end(w, "restored", dst, 0, MAIN, N)
    dst.close()


def test_ordering_in_a_pipelined_multi_group_ctx(world, monkeypatch):
    """6 slots in 3 groups, everything queued: a save between two frame sets holds the frame before it; a load
    queued between two frame sets into running slots ends their runs and the next frame set continues the loaded
    ones."""
    monkeypatch.setenv("SVO_GROUPS", "3")
    w = world
    cfg = w.cfg
    seeds = {s: (MAIN if s % 2 == 0 else SIDE) for s in range(6)}
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 6)
    assert batch.groups() == 3
    dev = {seed: ([torch.from_numpy(x).cuda() for x in w.seq[seed][0]], [torch.from_numpy(x).cuda() for x in w.seq[seed][1]])
           for seed in (MAIN, SIDE)}
    torch.cuda.synchronize()
    frame_of = {s: 0 for s in range(6)}     # the next frame of every slot
    keep = []

    def submit():
        packed = batch.pack_images([dev[seeds[s]][0][frame_of[s]] for s in range(6)], [dev[seeds[s]][1][frame_of[s]] for s in range(6)],
                                   [w.seq[seeds[s]][2][frame_of[s]] for s in range(6)])
        keep.append(packed)
        batch.submit_packed(packed)
        for s in range(6):
            frame_of[s] += 1

    t = 7
    for _ in range(t):
        submit()
    batch.wait()
    sizes = [batch.snapshot_size(s) for s in (1, 4)]
    snaps = [batch.new_snapshot(2 * hb, 2 * db) for hb, db in sizes]       # (room for what frame t adds)
    submit()                                                                # frame t
    batch.submit_save([1, 4], snapshots=snaps)
    submit()
    submit()
    batch.wait()
    assert [s.info.frame_id for s in snaps] == [t, t] and all(s.info.status == hip_lib.SNAPSHOT_COMPLETE for s in snaps)
    for s in range(6):
        _same_frame(w, f"slot {s} after the save", batch, s, seeds[s], t + 2)
    # slot 0 takes on slot 1's saved sequence, slot 5 slot 4's, between two frame sets
    submit()                                                                # frame t + 3
    batch.submit_load([0, 5], [s.trimmed() for s in snaps])
    seeds[0], seeds[5] = seeds[1], seeds[4]
    frame_of[0] = frame_of[5] = t + 1
    for _ in range(4):
        submit()
    batch.wait()
    for s in (0, 5):
        (run, traj), = batch.finished_runs(s)
        old = MAIN if s == 0 else SIDE
        assert (run.seq, run.run, run.frames) == (s, 0, t + 4)
        assert np.array_equal(traj, np.array([f[4] for f in w.oracle[old][:t + 4]])), f"slot {s}: the ended run"
    assert all(batch.finished_runs(s) == [] for s in (1, 2, 3, 4))
    for s in range(6):
        _same_frame(w, f"slot {s} at the end", batch, s, seeds[s], frame_of[s] - 1)
        _same_run_end(w, f"slot {s}", batch, s, seeds[s], frame_of[s])
    batch.close()


CACHES = ["2", "0", None]


@pytest.mark.parametrize("src_cache,dst_cache", [(a, b) for a in CACHES for b in CACHES if a != b])
def test_template_ring_combinations(world, monkeypatch, src_cache, dst_cache):
    """k = 45 (7 keyframes, 5 of them live): saved under one template-ring size, loaded under another."""
    w = world
    cfg = w.cfg
    snap = w.saved(45, src_cache, monkeypatch)
    _set_cache(monkeypatch, dst_cache)
    dst = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    assert (dst.memory().klt_cache_bytes == 0) == (dst_cache == "0")
    dst.load([0], [snap])
    _play(w, dst, {0: MAIN}, 46, N)
    _same_run_end(w, "restored", dst, 0, MAIN, N)
    dst.close()


@pytest.mark.parametrize("table", [None, "3"], ids=["unset", "3"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_round_trip(world, monkeypatch, device, table):
    """save(load(s)) == s byte for byte in both parts; two saves of one state are identical. With
    SVO_SNAPSHOT_TABLE_TILES=3 the at least 14 non-empty planes of frame 45 do not fit the group's tile table, so
    every save and load here goes out as five or more launches over a refilled table."""
    if table:
        monkeypatch.setenv("SVO_SNAPSHOT_TABLE_TILES", table)
    w = world
    cfg = w.cfg
    snap = w.saved(45)
    if device:
        snap = Snapshot(snap.host, torch.from_numpy(snap.data).cuda())
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 2)
    batch.load([1], [snap])
    a, b = batch.save([1], device=device)[0], batch.save([1], device=device)[0]
    as_bytes = lambda s: (s.host.tobytes(), s.data.cpu().numpy().tobytes() if s.device_mode else s.data.tobytes())
    assert as_bytes(a) == as_bytes(b) == as_bytes(snap)
    again = Snapshot.frombytes(a.tobytes(), device="cuda" if device else None)
    assert as_bytes(again) == as_bytes(snap) and again.info.frame_id == 45
    # an empty slot gives a valid snapshot, and loading it is a restart
    empty = batch.save([0])[0]
    assert (empty.info.frame_id, empty.info.n_planes) == (-1, 14)
    batch.load([1], [empty])
    assert batch.stats(1).frame_id == 0 and batch.num_keyframes(1) == 0 and len(batch.finished_runs(1)) == 1
    batch.close()


def test_rejections(world):
    """Every bad call raises, queues nothing and leaves the ctx tracking: slot 0 plays the main sequence through
    all of them."""
    w = world
    cfg = w.cfg
    good = w.saved(7)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 2)
    step = [0]

    def track_on():
        _play(w, batch, {0: MAIN}, step[0], step[0] + 1)
        step[0] += 1

    def rejected(seqs, snaps):
        with pytest.raises(SvoError):
            batch.submit_load(seqs, snaps)
        track_on()

    track_on()
    # a ctx with another keypoint grid
    other = StereoSlamBatch(dict(cfg, grid_width=32), cfg["width"], cfg["height"], 1)
    with pytest.raises(SvoError, match="differ"):
        other.load([0], [good])
    L, R, ts = w.frames(MAIN, 0)
    other.new_images([L], [R], [ts])
    assert other.stats(0).is_keyframe == 1 and other.num_keyframes(0) == 1
    other.close()
    rejected([1], [Snapshot(good.host[:-1], good.data)])                    # truncated host part
    rejected([1], [Snapshot(good.host[:SR.HEADER.size + 10], good.data)])
    rejected([1], [Snapshot(good.host, good.data[:-1])])                    # data part shorter than stated
    rejected([2], [good])                                                   # bad slot
    rejected([-1], [good])
    rejected([1, 1], [good, good])                                          # named twice
    rejected([0, 1], [good, Snapshot(good.host[:-1], good.data)])           # one bad snapshot: slot 0 is not touched either
    with pytest.raises(SvoError):
        batch.submit_save([0, 0], snapshots=[batch.new_snapshot(1 << 16, 1 << 20) for _ in range(2)])
    with pytest.raises(SvoError):
        batch.submit_save([0], snapshots=[batch.new_snapshot(SR.HEADER.size - 1, 1 << 20)])
    track_on()
    assert batch.finished_runs(0) == [] and batch.stats(1).frame_id == 0 and batch.num_keyframes(1) == 0
    # capacities too small: the header alone, with the sizes needed; nothing past it is touched
    for short_host, short_data in ((1, 0), (0, 1), (None, None)):
        need = batch.snapshot_size(0)
        host_cap, data_cap = (SR.HEADER.size, 0) if short_host is None else (need[0] - short_host, need[1] - short_data)
        small = Snapshot(np.full(host_cap, 0xAB, np.uint8), np.full(data_cap, 0xAB, np.uint8))
        batch.submit_save([0], snapshots=[small])
        batch.wait()
        info = small.info
        assert info.status == hip_lib.SNAPSHOT_TOO_SMALL and (info.host_bytes, info.data_bytes) == need
        assert np.all(small.host[SR.HEADER.size:] == 0xAB) and np.all(small.data == 0xAB)
        rejected([1], [small])                                              # and a load refuses it
    exact = batch.save([0])[0]
    assert exact.info.status == hip_lib.SNAPSHOT_COMPLETE and exact.info.frame_id == step[0] - 1
    track_on()
    batch.close()


def test_memory(world):
    """What a load takes from the free lists a restart gives back; rounds of (load, 2 frames, restart) in one
    slot leave the ctx's device memory where the first round left it."""
    w = world
    cfg = w.cfg
    snap = w.saved(45)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    batch.load([0], [snap])                  # (the pools grow to what the state needs, once)
    batch.restart([0])
    before = batch.memory()
    assert before.image_sets_free == before.image_sets and before.keyframe_slabs_free == before.keyframe_slabs
    batch.load([0], [snap])
    loaded = batch.memory()
    info = snap.info
    assert (info.n_keyframes, info.n_image_sets) == (7, 6)
    assert loaded.keyframe_slabs_free == before.keyframe_slabs_free - info.n_keyframes
    assert loaded.image_sets_free == before.image_sets_free - info.n_image_sets
    batch.restart([0])
    after = batch.memory()
    assert (after.image_sets_free, after.keyframe_slabs_free) == (before.image_sets_free, before.keyframe_slabs_free)
    assert (after.image_sets, after.keyframe_slabs, after.device_bytes) == (before.image_sets, before.keyframe_slabs, before.device_bytes)
    first = None
    for r in range(20):
        batch.load([0], [snap])
        _play(w, batch, {0: MAIN}, 46, 48, check=r in (0, 19))
        batch.restart([0])
        m = batch.memory()
        first = first or (m.device_bytes, m.image_sets, m.keyframe_slabs)
        assert (m.device_bytes, m.image_sets, m.keyframe_slabs) == first, r
        assert m.image_sets_free == m.image_sets and m.keyframe_slabs_free == m.keyframe_slabs
    assert len(batch.finished_runs(0)) == 22
    batch.close()


def test_pose_filter_is_carried(world):
    """The same update_pose (a gyro sample) at the source and at the restored slot gives the same output, and the
    next three frames are equal."""
    w = world
    cfg = w.cfg
    src = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    _play(w, src, {0: MAIN}, 0, 8)
    dst = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 2)
    dst.load([1], src.save([0]))
    rng = np.random.RandomState(3)
    for dt in (0.0, 0.05):
        pose, speed = rng.normal(0, 0.05, 6).astype(np.float32), rng.normal(0, 0.05, 6).astype(np.float32)
        args = (pose, speed, np.full(6, 0.1, np.float32), np.ones(6, np.float32), dt)
        a, b = src.update_pose(*args, seq=0), dst.update_pose(*args, seq=1)
        assert np.array_equal(a, b) and np.any(a != 0)
    for k in range(8, 11):
        _play(w, src, {0: MAIN}, k, k + 1, check=False)
        _play(w, dst, {1: MAIN}, k, k + 1, check=False)
        assert _state(src, 0) == _state(dst, 1), k
    assert src.stats(0).frame_id == 10
    src.close()
    dst.close()


@pytest.mark.parametrize("table", [None, "1000"], ids=["one-launch", "chunked"])
def test_copy_segments_alone(monkeypatch, table):
    """svo_copy_segments against numpy: every row length x source offset x destination offset x pitch kind x row
    count in one call, every destination surrounded by canary bytes."""
    if table:
        monkeypatch.setenv("SVO_SNAPSHOT_TABLE_TILES", table)
    rng = np.random.RandomState(5)
    lengths = (0, 1, 3, 4, 15, 16, 17, 255, 256, 4097)
    segs, at = [], 0
    for n in lengths:
        pitches = {"equal": (n + 15) // 16 * 16 + 16, "dense": n}
        for kind in ("equal", "unequal", "dense"):
            sp, dp = (n + 7, n + 13) if kind == "unequal" else (pitches[kind],) * 2
            for rows in (0, 1, 5):
                for so in range(16):
                    for do in range(16):
                        segs.append((at + so, at + 32 + do, n, rows, sp, dp))
                        at += (max(sp, dp) * rows + 64 + 15) // 16 * 16 + 32
    total = at + 64
    src = rng.randint(0, 256, total).astype(np.uint8)
    dst = np.full(total, 0xCD, np.uint8)
    expect = dst.copy()
    for s, d, n, rows, sp, dp in segs:
        for r in range(rows):
            expect[d + r * dp:d + r * dp + n] = src[s + r * sp:s + r * sp + n]
    dsrc, ddst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    assert dsrc.data_ptr() % 16 == 0 and ddst.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    h = hip_lib.Handle(0, 64)
    h.copy_segments([(dsrc.data_ptr() + s, ddst.data_ptr() + d, n, rows, sp, dp) for s, d, n, rows, sp, dp in segs])
    got = ddst.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, (bad[:8], len(segs))
    for seg in ((dsrc.data_ptr(), ddst.data_ptr(), -1, 1, 0, 0), (0, ddst.data_ptr(), 4, 1, 4, 4), (dsrc.data_ptr(), ddst.data_ptr(), 8, 2, 8, 4)):
        with pytest.raises(SvoError):
            h.copy_segments([seg])
    h.copy_segments([])
    h.copy_segments([(0, 0, 0, 5, 0, 0), (0, 0, 7, 0, 7, 7)])              # nothing to copy: no pointer is looked at
    assert np.array_equal(ddst.cpu().numpy(), expect)
    h.close()


def test_move_between_ctxs(world):
    """multi_seq.move: slot 1 of a 2-slot ctx continues as slot 3 of a 4-slot ctx."""
    w = world
    cfg = w.cfg
    src = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 2)
    dst = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 4)
    _play(w, src, {0: SIDE, 1: MAIN}, 0, 16)
    _play(w, dst, {0: SIDE}, 0, 3)
    multi_seq.move(src, [1], dst, [3])
    (run, traj), = src.finished_runs(1)
    assert run.frames == 16 and np.array_equal(traj, np.array([f[4] for f in w.oracle[MAIN][:16]]))
    assert src.stats(1).frame_id == 0 and src.num_keyframes(1) == 0 and src.get_trajectory(1).shape == (0, 6)
    _same_frame(w, "moved", dst, 3, MAIN, 15)
    _play(w, src, {0: SIDE}, 16, 20)
    _play(w, dst, {0: SIDE, 3: MAIN}, 16, 30, offsets={0: 13})
    _same_run_end(w, "moved", dst, 3, MAIN, 30)
    src.close()
    dst.close()
