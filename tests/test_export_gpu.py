"""The bulk export (svo_submit_export / svo_pack_keypoints) on the GPU. The yardsticks are the numpy restatement
(tests/export_ref.py) for the stage entry and the per-sequence getters (get_frame, get_keyframe, stats, pose) for
the ctx: every comparison is on bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import export_ref as ER
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import Handle
from stereo_svo_slam_amd.stereo_slam import KP_INFO_DTYPE, StereoSlamBatch

pytestmark = pytest.mark.gpu

FIELDS = ("kps2d", "kps3d", "info")


# ---------------------------------------------------------------------------------- stage entry

def _device_plane(values, offset, keep):
    """the 4-byte values in device memory at a base that is `offset` bytes past an allocation's start"""
    raw = np.zeros(offset + values.nbytes + 16, np.uint8)
    raw[offset:offset + values.nbytes] = values.view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw).cuda()
    keep.append(t)
    return t.data_ptr() + offset


def _crafted_sets(counts, seed):
    """seeded random SoA sets (every plane any 32-bit pattern) as (host sets for export_ref, device sets for
    Handle.pack_keypoints); plane bases are 4 and 12 bytes past their allocations, alternating; the kps2d / kps3d
    of every other set too"""
    rng = np.random.default_rng(seed)
    host, dev, keep = [], [], []
    for j, n in enumerate(counts):
        k2 = rng.integers(0, 2**32, (n, 2), dtype=np.uint32).view(np.float32)
        k3 = rng.integers(0, 2**32, (n, 3), dtype=np.uint32).view(np.float32)
        planes = {name: rng.integers(0, 2**32, n, dtype=np.uint32) for name in ER.PLANES}
        host.append((n, k2, k3, planes))
        fields = {"kps2d": _device_plane(k2, (4 if j % 2 else 0), keep), "kps3d": _device_plane(k3, (12 if j % 2 else 0), keep)}
        for i, name in enumerate(ER.PLANES):
            fields[name] = _device_plane(planes[name], 4 if (i + j) % 2 else 12, keep)
        dev.append((n, fields))
    return host, dev, keep


COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)


def test_pack_keypoints_on_crafted_sets():
    """every n of the list mixed in one call, in two orders; the result is export_ref's, and every byte outside
    the segments keeps its 0xA5"""
    h = Handle(0, 1024)
    for seed, order in ((1, COUNTS), (2, COUNTS[::-1] + (256, 0, 2))):
        host, dev, keep = _crafted_sets(order, seed)
        first = ER.placement(list(range(len(order))), list(order), [(0, len(order))], 0)
        assert all(f % 4 == 0 for f in first)
        first = [f + 8 for f in first]                       # (records 0..7 stay untouched too)
        records = first[-1] + order[-1] + 9
        want = ER.pack(host, first, records)
        outs = [torch.full((records, w), 0xA5, dtype=torch.uint8, device="cuda") for w in (8, 12, 44)]
        h.pack_keypoints(dev, first, *outs)
        h.synchronize()
        for name, got, exp in zip(FIELDS, outs, want):
            assert got.cpu().numpy().tobytes() == exp.tobytes(), (seed, name)
        del keep
    h.close()


def test_pack_keypoints_skips_null_arrays():
    h = Handle(0, 1024)
    counts = (5, 257, 0, 64)
    host, dev, keep = _crafted_sets(counts, 3)
    first = ER.placement(list(range(4)), list(counts), [(0, 4)], 0)
    records = first[-1] + counts[-1] + 5
    want = ER.pack(host, first, records)
    for given in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        outs = [torch.full((records, w), 0xA5, dtype=torch.uint8, device="cuda") if g else None for w, g in zip((8, 12, 44), given)]
        h.pack_keypoints(dev, first, *outs)
        h.synchronize()
        for name, got, exp in zip(FIELDS, outs, want):
            if got is not None:
                assert got.cpu().numpy().tobytes() == exp.tobytes(), (given, name)
    h.pack_keypoints(dev, first, None, None, None)          # nothing to do
    h.pack_keypoints([], [], torch.zeros(8, dtype=torch.uint8, device="cuda"))
    h.synchronize()
    h.close()


# ---------------------------------------------------------------------------------- the ctx against its getters

def _sequences(config, seeds, n_frames, motion_scale=4.0):
    """[(lefts [n, H, W], rights, time stamps)] rendered on the GPU, and the config"""
    out = []
    for seed in seeds:
        cfg, L, R, _, ts = synth.make_sequence_gpu(config, n_frames, seed, motion_scale=motion_scale)
        out.append((L, R, [float(t) for t in ts]))
    torch.cuda.synchronize()
    return cfg, out


def _frame_set(n, live):
    """live: {slot: (sequence tuple, frame index)} -> lefts, rights, time stamps of new_images / pack_images"""
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for slot, (seq, k) in live.items():
        L[slot], R[slot], ts[slot] = seq[0][k], seq[1][k], seq[2][k]
    return L, R, ts


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _getter_state(batch, slots=None):
    """what the getters say about the slots, as comparable values: per slot (frame n, kps2d, kps3d, info bytes,
    pose bytes, stats frame_id, is_keyframe) and (keyframe count, keyframe n, its three arrays, its pose)"""
    out = {}
    for s in (range(batch.n) if slots is None else slots):
        f, st, nk = batch.get_frame(s), batch.stats(s), batch.num_keyframes(s)
        kf = batch.get_keyframe(None, s) if nk else None
        out[s] = dict(frame=(len(f.kps2d), _bytes(f.kps2d), _bytes(f.kps3d), _bytes(f.info), _bytes(f.pose)),
                      frame_id=st.frame_id, is_keyframe=st.is_keyframe, n_keyframes=nk,
                      keyframe=None if kf is None else (len(kf.kps2d), _bytes(kf.kps2d), _bytes(kf.kps3d), _bytes(kf.info), _bytes(kf.pose)))
    return out


def _segment_arrays(e, i):
    """segment i of an Export as (n, kps2d, kps3d, info bytes, pose bytes), through Export.frame"""
    f = e.frame(i)
    assert f.info.dtype == KP_INFO_DTYPE and f.kps2d.shape[1:] == (2,) and f.kps3d.shape[1:] == (3,)
    return (int(e.segments[i]["n"]), _bytes(f.kps2d), _bytes(f.kps3d), _bytes(f.info), _bytes(f.pose))


def _check_placement(e, batch, seqs):
    groups = ER.group_ranges(batch.n, batch.groups())
    want = ER.placement(seqs, [int(x) for x in e.segments["n"]], groups, batch.export_capacity())
    assert [int(x) for x in e.segments["first"]] == want
    assert e.capacity == len(seqs) * batch.export_capacity()


def _check_frames(tag, e, state, seqs, expect):
    """the frames export against the getters' state; expect[slot] = (run, time stamp or None for an empty slot)"""
    assert len(e.segments) == len(seqs)
    for i, s in enumerate(seqs):
        seg, g = e.segments[i], state[s]
        run, ts = expect[s]
        assert int(seg["seq"]) == s and int(seg["run"]) == run, (tag, s)
        assert int(seg["keyframe_id"]) == -1 and int(seg["_pad"]) == 0, (tag, s)
        if ts is None:                                       # an empty slot: what a fresh ctx reports
            assert int(seg["frame_id"]) == -1 and int(seg["n"]) == 0 and int(seg["is_keyframe"]) == 0, (tag, s)
            assert _bytes(seg["pose"]) == bytes(24) and float(seg["time_stamp"]) == 0.0, (tag, s)
            assert g["frame"][0] == 0 and g["frame"][4] == bytes(24), (tag, s)
        else:
            assert int(seg["frame_id"]) == g["frame_id"] and int(seg["is_keyframe"]) == g["is_keyframe"], (tag, s)
            assert np.float32(seg["time_stamp"]) == np.float32(ts), (tag, s)
        assert _segment_arrays(e, i) == g["frame"], (tag, s)


def _check_keyframes(tag, e, state, seqs):
    for i, s in enumerate(seqs):
        seg, g = e.segments[i], state[s]
        assert int(seg["seq"]) == s and int(seg["keyframe_id"]) == g["n_keyframes"] - 1, (tag, s)
        if g["keyframe"] is None:
            assert int(seg["n"]) == 0 and _bytes(seg["pose"]) == bytes(24), (tag, s)
        else:
            assert _segment_arrays(e, i) == g["keyframe"], (tag, s)


def _run_against_getters(config, n_slots, seeds, steps, starts):
    """slot s plays sequence s % len(seeds) from step starts[s] on; after every step both exports equal the getters"""
    cfg, seqs = _sequences(config, seeds, steps)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    slots = list(range(n_slots))
    later_keyframe = False
    for t in range(steps):
        live = {s: (seqs[s % len(seeds)], t - starts[s]) for s in slots if t >= starts[s]}
        L, R, ts = _frame_set(n_slots, live)
        batch.new_images(L, R, ts)
        frames = batch.export_frames()
        keyframes = batch.export_last_keyframes()
        state = _getter_state(batch)
        expect = {s: (0, ts[s] if s in live else None) for s in slots}
        _check_frames(f"step {t}", frames, state, slots, expect)
        _check_keyframes(f"step {t}", keyframes, state, slots)
        _check_placement(frames, batch, slots)
        _check_placement(keyframes, batch, slots)
        later_keyframe = later_keyframe or any(state[s]["is_keyframe"] and state[s]["frame_id"] > 0 for s in live)
    groups = batch.groups()
    batch.close()
    return groups, later_keyframe


def test_against_the_getters_one_group(monkeypatch):
    """tiny, 5 slots in one group, 24 frames of fast motion: first frames (a keyframe each), tracked frames and
    keyframes made later on"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    groups, later_keyframe = _run_against_getters("tiny", 5, (1, 11, 12, 13, 14), 24, [0, 0, 1, 2, 0])
    assert groups == 1
    assert later_keyframe, "some sequence makes a keyframe after its first frame"


def test_against_the_getters_three_groups(monkeypatch):
    """euroc, 66 slots in three groups; slots start at steps 0, 1 and 2, so a step mixes empty slots, first frames
    (keyframes) and tracked frames"""
    monkeypatch.setenv("SVO_GROUPS", "3")
    groups, _ = _run_against_getters("euroc", 66, (3, 4, 5, 6), 4, [s % 3 for s in range(66)])
    assert groups == 3


def test_a_tile_table_smaller_than_the_export(monkeypatch):
    """SVO_EXPORT_TABLE_TILES=2: seven slots need at least seven tiles, so every export goes out as several
    launches with the table refilled in between; the result is the same"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    monkeypatch.setenv("SVO_EXPORT_TABLE_TILES", "2")
    groups, _ = _run_against_getters("tiny", 7, (1, 11, 12), 4, [0, 0, 1, 0, 2, 0, 1])
    assert groups == 1


# ---------------------------------------------------------------------------------- named slots, errors

def _raw_submit(batch, what, seqs, n, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export(batch._ctx, what, arr, n, C.byref(dst), mem)


def test_named_slots_and_rejected_calls(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "3")
    n_slots = 9
    cfg, seqs = _sequences("tiny", (1, 11, 12), 3)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 3
    slots = list(range(n_slots))
    for t in range(2):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 3], t) for s in slots}))
    state = _getter_state(batch)
    expect = {s: (0, seqs[s % 3][2][1]) for s in slots}
    for named in ([7, 0, 4, 8, 1], [5], [8, 7, 6, 5, 4, 3, 2, 1, 0], []):
        e = batch.export_frames(named)
        _check_frames(f"named {named}", e, state, named, expect)
        _check_placement(e, batch, named)
        k = batch.export_last_keyframes(named, fields=("info",))
        assert k.kps2d is None and k.kps3d is None
        _check_placement(k, batch, named)
        for i, s in enumerate(named):
            assert k.frame(i).info.tobytes() == state[s]["keyframe"][3]
    # rejected on the host, nothing queued
    cap = batch.export_capacity()
    good = batch.export_frames([0, 1])
    seg = np.zeros(4, hip_lib.EXPORT_SEGMENT_DTYPE)
    buf = np.zeros((2 * cap, 44), np.uint8)
    dst = hip_lib.ExportDst(seg.ctypes.data, None, None, buf.ctypes.data, 2 * cap)
    assert _raw_submit(batch, 0, [0, 0], 2, dst, hip_lib.MEM_HOST) == -1           # named twice
    assert _raw_submit(batch, 0, [0, n_slots], 2, dst, hip_lib.MEM_HOST) == -1     # out of range
    assert _raw_submit(batch, 0, [-1, 1], 2, dst, hip_lib.MEM_HOST) == -1
    assert _raw_submit(batch, 0, [0, 1], 2, dst, 2) == -1                          # SVO_MEM_DEVICE_BORROW is no export mode
    assert _raw_submit(batch, 0, [0, 1], 2, dst, 7) == -1
    assert _raw_submit(batch, 2, [0, 1], 2, dst, hip_lib.MEM_HOST) == -1           # no such `what`
    dst.capacity = 2 * cap - 1
    assert _raw_submit(batch, 0, [0, 1], 2, dst, hip_lib.MEM_HOST) == -4           # one record below the bound
    assert b"capacity" in hip_lib.lib().svo_last_error()
    dst.capacity = n_slots * cap - 1
    assert _raw_submit(batch, 0, None, 0, dst, hip_lib.MEM_HOST) == -4             # every slot named
    assert not seg.view(np.uint8).any() and not buf.any()
    # at the bound it is accepted, and the ctx has kept working
    dst.capacity = 2 * cap
    assert _raw_submit(batch, 0, [0, 1], 2, dst, hip_lib.MEM_HOST) == 0
    batch.wait()
    assert seg[:2].tobytes() == good.segments.tobytes()
    lo, n = int(seg[1]["first"]), int(seg[1]["n"])
    assert buf[lo:lo + n].tobytes() == state[1]["frame"][3]
    batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 3], 2) for s in slots}))
    _check_frames("after the errors", batch.export_frames(), _getter_state(batch), slots, {s: (0, seqs[s % 3][2][2]) for s in slots})
    batch.close()


# ---------------------------------------------------------------------------------- slot states

def test_slot_states(monkeypatch):
    """slot 0 runs through; slot 1 never starts; slot 2 is restarted and stays empty for a step, then plays a new
    sequence (run 1); slot 3 sits step 2 out"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    cfg, seqs = _sequences("tiny", (1, 11, 12, 13), 5)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 4)
    slots = [0, 1, 2, 3]
    a, b, c, d = seqs

    def step(live, expect, tag):
        L, R, ts = _frame_set(4, live)
        batch.new_images(L, R, ts)
        e, k = batch.export_frames(), batch.export_last_keyframes()
        state = _getter_state(batch)
        _check_frames(tag, e, state, slots, expect)
        _check_keyframes(tag, k, state, slots)
        return e

    step({0: (a, 0), 2: (b, 0), 3: (c, 0)}, {0: (0, a[2][0]), 1: (0, None), 2: (0, b[2][0]), 3: (0, c[2][0])}, "step 0")
    before = step({0: (a, 1), 2: (b, 1), 3: (c, 1)}, {0: (0, a[2][1]), 1: (0, None), 2: (0, b[2][1]), 3: (0, c[2][1])}, "step 1")
    batch.restart([2])
    e = step({0: (a, 2)}, {0: (0, a[2][2]), 1: (0, None), 2: (1, None), 3: (0, c[2][1])}, "step 2")
    assert int(e.segments[2]["run"]) == 1 and int(e.segments[2]["n"]) == 0 and int(e.segments[2]["frame_id"]) == -1
    assert int(e.segments[1]["frame_id"]) == -1 and int(e.segments[1]["n"]) == 0
    # the slot that sat the step out still shows its previous frame
    assert int(e.segments[3]["frame_id"]) == 1 and _segment_arrays(e, 3) == _segment_arrays(before, 3)
    e = step({0: (a, 3), 2: (d, 0), 3: (c, 2)}, {0: (0, a[2][3]), 1: (0, None), 2: (1, d[2][0]), 3: (0, c[2][2])}, "step 3")
    assert int(e.segments[2]["run"]) == 1 and int(e.segments[2]["frame_id"]) == 0 and int(e.segments[2]["n"]) > 0
    assert int(e.segments[3]["frame_id"]) == 2
    batch.close()


# ---------------------------------------------------------------------------------- ordering, device mode

def test_ordering_without_draining(monkeypatch):
    """frame set t, export A, frame set t+1, export B, one wait: A is the state at t, B at t+1 (a twin ctx stopped
    at each)"""
    monkeypatch.setenv("SVO_GROUPS", "2")
    n_slots, t = 6, 3
    cfg, seqs = _sequences("tiny", (1, 11, 12), t + 2)
    sets = [_frame_set(n_slots, {s: (seqs[s % 3], k) for s in range(n_slots)}) for k in range(t + 2)]
    expect = [{s: (0, seqs[s % 3][2][k]) for s in range(n_slots)} for k in range(t + 2)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 2
    for k in range(t):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
    packed = [batch.pack_images(*sets[k]) for k in (t, t + 1)]
    batch.submit_packed(packed[0])
    a_frames, a_kf = batch.submit_export("frames"), batch.submit_export("last_keyframes")
    batch.submit_packed(packed[1])
    b_frames, b_kf = batch.submit_export("frames"), batch.submit_export("last_keyframes")
    batch.wait()
    slots = list(range(n_slots))
    twin.new_images(*sets[t])
    state = _getter_state(twin)
    _check_frames("A", a_frames, state, slots, expect[t])
    _check_keyframes("A", a_kf, state, slots)
    twin.new_images(*sets[t + 1])
    state = _getter_state(twin)
    _check_frames("B", b_frames, state, slots, expect[t + 1])
    _check_keyframes("B", b_kf, state, slots)
    assert [int(x) for x in a_frames.segments["frame_id"]] == [t] * n_slots
    assert [int(x) for x in b_frames.segments["frame_id"]] == [t + 1] * n_slots
    batch.close()
    twin.close()


def test_device_mode_gives_the_same_bytes(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    n_slots = 6
    cfg, seqs = _sequences("tiny", (1, 11, 12), 3)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    for k in range(3):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 3], k) for s in range(n_slots) if s != 4}))
    for what in ("frames", "last_keyframes"):
        for named in (None, [5, 2, 4, 0]):
            host = batch.submit_export(what, named).wait()
            dev = batch.submit_export(what, named, device=True).wait()
            assert dev.kps2d.is_cuda and dev.info.dtype == torch.uint8 and tuple(dev.info.shape) == (dev.capacity, 44)
            assert host.segments.tobytes() == dev.segments.tobytes()
            for i in range(len(host.segments)):
                assert _segment_arrays(host, i) == _segment_arrays(dev, i), (what, named, i)
            # a device array pre-filled with 0xA5 keeps it outside the segments
            dev.kps2d.view(torch.uint8).fill_(0xA5); dev.kps3d.view(torch.uint8).fill_(0xA5); dev.info.fill_(0xA5)
            dev.submit().wait()
            inside = np.zeros(dev.capacity, bool)
            for seg in dev.segments:
                inside[int(seg["first"]):int(seg["first"]) + int(seg["n"])] = True
            for name in FIELDS:
                raw = getattr(dev, name).cpu().numpy().view(np.uint8).reshape(dev.capacity, -1)
                assert np.all(raw[~inside] == 0xA5), (what, named, name)
            for i in range(len(host.segments)):
                assert _segment_arrays(host, i) == _segment_arrays(dev, i), (what, named, i)
    # host arrays pre-filled with 0xA5: a group delivers its used prefix (first segment to last) and nothing after it
    host = batch.export_frames()
    for name in FIELDS:
        getattr(host, name).view(np.uint8).fill(0xA5)
    host.submit().wait()
    cap = batch.export_capacity()
    touched = np.zeros(host.capacity, bool)
    before = 0
    for lo, count in ER.group_ranges(n_slots, batch.groups()):
        segs = host.segments[lo:lo + count]
        touched[before * cap:int(segs[-1]["first"]) + int(segs[-1]["n"])] = True
        before += count
    assert not touched.all()
    for name in FIELDS:
        raw = getattr(host, name).view(np.uint8).reshape(host.capacity, -1)
        assert np.all(raw[~touched] == 0xA5), name
    state = _getter_state(batch)
    for i in range(n_slots):
        assert _segment_arrays(host, i) == state[i]["frame"], i
    batch.close()


# ---------------------------------------------------------------------------------- no side effects
    batch.close()


# ---------------------------------------------------------------------------------- no side effects

def test_no_side_effects(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    n_slots, steps = 6, 12
    cfg, seqs = _sequences("tiny", (1, 11, 12), steps)
    sets = [_frame_set(n_slots, {s: (seqs[s % 3], k) for s in range(n_slots)}) for k in range(steps)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    fresh = twin.memory().device_bytes
    assert batch.memory().device_bytes == fresh
    batch.submit_export("frames", device=True).wait()          # device mode: no staging block
    assert batch.memory().device_bytes == fresh
    exports = []
    for k in range(steps):
        batch.submit_packed(batch.pack_images(*sets[k]))
        exports.append((batch.submit_export("frames"), batch.submit_export("last_keyframes")))
        twin.new_images(*sets[k])
    batch.wait()
    grown = batch.memory().device_bytes - twin.memory().device_bytes
    assert 0 < grown <= n_slots * batch.export_capacity() * 64, grown
    a, b = _getter_state(batch), _getter_state(twin)
    assert a == b
    for s in range(n_slots):
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes() and len(batch.get_trajectory(s)) == steps
        assert batch.num_keyframes(s) == twin.num_keyframes(s)
    _check_frames("last", exports[-1][0], b, list(range(n_slots)), {s: (0, seqs[s % 3][2][steps - 1]) for s in range(n_slots)})
    _check_keyframes("last", exports[-1][1], b, list(range(n_slots)))
    batch.close()
    twin.close()


def test_many_slots_exporting_every_step_track_like_a_twin(monkeypatch):
    """euroc, 66 slots in three groups, both exports queued behind every frame set (their tile tables reuse the
    groups' argument blocks between the steps): trajectories, keyframes and last frames equal a twin's that never
    exports"""
    monkeypatch.setenv("SVO_GROUPS", "3")
    n_slots, steps = 66, 8
    cfg, seqs = _sequences("euroc", (3, 4, 5, 6), steps)
    sets = [_frame_set(n_slots, {s: (seqs[s % 4], k) for s in range(n_slots)}) for k in range(steps)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 3
    queued = []                                  # (an Export owns the buffers its queued export writes: kept until the wait)
    for k in range(steps):
        batch.submit_packed(batch.pack_images(*sets[k]))
        frames, keyframes = batch.submit_export("frames"), batch.submit_export("last_keyframes", device=True)
        queued.append((frames, keyframes))
        twin.new_images(*sets[k])
    batch.wait()
    a, b = _getter_state(batch), _getter_state(twin)
    assert a == b
    for s in range(n_slots):
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes() and len(twin.get_trajectory(s)) == steps
    slots = list(range(n_slots))
    _check_frames("last", frames, b, slots, {s: (0, seqs[s % 4][2][steps - 1]) for s in slots})
    _check_keyframes("last", keyframes, b, slots)
    batch.close()
    twin.close()
