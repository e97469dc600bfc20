"""The map export (svo_submit_export_map / svo_pack_map_points) on the GPU. The yardsticks are the numpy restatement
(tests/map_ref.py) for the stage entry and, for the ctx, the per-keyframe getters (get_keyframe) with map_ref's
filter applied to their records: every comparison is on bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_ref as MR
from stereo_svo_slam_amd import hip_lib, synth, wire
from stereo_svo_slam_amd.hip_lib import Handle, MapFilter
from stereo_svo_slam_amd.stereo_slam import MapExport, StereoSlamBatch

pytestmark = pytest.mark.gpu

INT_MIN = -2**31
OWN_CURRENT = dict(drop_flags=MR.IGNORE_COMPLETELY, own_only=1, min_inliers=0)
INLIERS_8 = dict(drop_flags=0, own_only=0, min_inliers=8)
COMBINED = dict(drop_flags=MR.IGNORE_COMPLETELY, own_only=1, min_inliers=8)


# ---------------------------------------------------------------------------------- stage entry, crafted

REGION_COUNTS = ((0, 1, 3, 63, 64, 65, 255, 256, 257, 1000),                      # A
                 (),                                                              # B: no sets
                 tuple(int(x) for x in np.random.default_rng(7).integers(0, 6, 300)),   # C: more tiles than a workgroup has lanes
                 (1000,))                                                         # D


def _device_plane(values, offset, keep):
    """the 4-byte values in device memory at a base that is `offset` bytes past an allocation's start"""
    values = np.ascontiguousarray(values)
    raw = np.zeros(offset + values.nbytes + 16, np.uint8)
    raw[offset:offset + values.nbytes] = values.view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw).cuda()
    keep.append(t)
    return t.data_ptr() + offset


class Crafted:
    """the four regions: per set kps3d (any bit pattern, NaNs included) and colour, fixed and in device memory at
    bases 4 and 12 bytes past their allocations; flags, keyframe_id and inlier_count are made per keep pattern"""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.keep, self.sets = [], []                 # sets: (region, n, own_id, kps3d bits, colour, device addresses)
        for r, counts in enumerate(REGION_COUNTS):
            for j, n in enumerate(counts):
                k3 = rng.integers(0, 2**32, (n, 3), dtype=np.uint32)
                if n:
                    k3[0, 0] = 0x7fc00001             # a NaN with a payload
                color = rng.integers(0, 2**32, n, dtype=np.uint32)
                dev = {"kps3d": _device_plane(k3, 12 if j % 2 else 4, self.keep),
                       "color": _device_plane(color, 4 if j % 2 else 12, self.keep)}
                self.sets.append((r, n, (3 * j + r) % 11, k3, color, dev))
        self.bound = [sum(s[1] for s in self.sets if s[0] == r) for r in range(len(REGION_COUNTS))]
        # every region behind the one before it, with records in between that must stay untouched
        self.first, at = [], 8
        for b in self.bound:
            self.first.append(at)
            at += b + 5
        self.records = at + 4

    def pattern(self, name, rng):
        """bool per set: which keypoints are kept"""
        out = []
        for t, (_, n, *_) in enumerate(self.sets):
            i = np.arange(n)
            if name == "all":
                k = np.ones(n, bool)
            elif name == "none":
                k = np.zeros(n, bool)
            elif name == "lanes":
                k = np.isin(i % 256, (0, 63, 64, 255))
            elif name == "waves":
                k = (i // 64) % 2 == 0
            elif name == "tiles":
                k = (i // 256 + t) % 2 == 0
            else:
                k = rng.random(n) < float(name)
            out.append(k)
        return out

    def planes(self, keeps, driver, rng):
        """(filter, per set the three planes) such that exactly `keeps` pass: driven through one filter field, or
        through all three (a dropped point fails a random non-empty choice of them)"""
        filt = dict(drop_flags=0, own_only=0, min_inliers=INT_MIN)
        if driver in ("drop_flags", "combined"):
            filt["drop_flags"] = MR.IGNORE_COMPLETELY | MR.IGNORE_TEMPORARY
        if driver in ("own_only", "combined"):
            filt["own_only"] = 1
        if driver in ("min_inliers", "combined"):
            filt["min_inliers"] = 8
        out = []
        for (_, n, own, *_), keep in zip(self.sets, keeps):
            fail = np.zeros((3, n), bool)
            if driver == "combined":
                fail = rng.random((3, n)) < 0.5
                fail[rng.integers(0, 3, n), np.arange(n)] = True
            else:
                fail[("drop_flags", "own_only", "min_inliers").index(driver)] = True
            fail &= ~keep
            flags = rng.integers(0, 2**32, n, dtype=np.uint32)
            kf_id = rng.integers(-5, 20, n).astype(np.int32)
            inl = rng.integers(-2**31, 2**31, n).astype(np.int32)
            if filt["drop_flags"]:
                bad = np.where(rng.random(n) < 0.5, MR.IGNORE_COMPLETELY, MR.IGNORE_TEMPORARY).astype(np.uint32)
                flags = np.where(fail[0], flags | bad, flags & ~np.uint32(filt["drop_flags"]))
            if filt["own_only"]:
                kf_id = np.where(fail[1], own + 1 + rng.integers(0, 5, n), own).astype(np.int32)
            if filt["min_inliers"] != INT_MIN:
                inl = np.where(fail[2], 7 - rng.integers(0, 100, n), 8 + rng.integers(0, 100, n)).astype(np.int32)
            out.append({"flags": flags, "keyframe_id": kf_id.view(np.uint32), "inlier_count": inl.view(np.uint32)})
        return filt, out

    def call(self, h, filt, planes, reverse=False, with_points=True):
        """one svo_pack_map_points over the four regions (reverse: the regions and the sets inside them in reversed
        order); returns (points bytes or None, counts, the same two from map_ref)"""
        step = -1 if reverse else 1
        regions_of = list(range(len(REGION_COUNTS)))[::step]
        keep = []
        host, dev = [], []
        for r in regions_of:
            hs, ds = [], []
            for t in list(range(len(self.sets)))[::step]:
                reg, n, own, k3, color, d = self.sets[t]
                if reg != r:
                    continue
                p = dict(planes[t], color=color)
                hs.append((n, own, k3, p))
                fields = dict(d)
                for i, name in enumerate(("flags", "keyframe_id", "inlier_count")):
                    fields[name] = _device_plane(p[name], 4 if (i + t) % 2 else 12, keep)
                ds.append((n, own, fields))
            host.append(hs)
            dev.append(ds)
        first = [self.first[r] for r in regions_of]
        want, want_counts = MR.pack(host, first, filt, self.records)
        n_sets = sum(len(r) for r in dev)
        points = torch.full((self.records, 16), 0xA5, dtype=torch.uint8, device="cuda") if with_points else None
        counts = torch.full((n_sets + 3,), -7, dtype=torch.int32, device="cuda")
        h.pack_map_points(dev, first, filt, points, counts)
        got_counts = counts.cpu().numpy()
        assert list(got_counts[n_sets:]) == [-7] * 3
        return (None if points is None else points.cpu().numpy().tobytes()), list(got_counts[:n_sets]), want.tobytes(), want_counts


@pytest.fixture(scope="module")
def crafted():
    return Crafted()


PATTERNS = [("all", "combined"), ("none", "combined"), ("lanes", "drop_flags"), ("waves", "own_only"), ("tiles", "min_inliers")] + \
           [(rate, driver) for rate in ("0.1", "0.5", "0.9") for driver in ("drop_flags", "own_only", "min_inliers", "combined")]


@pytest.mark.parametrize("name,driver", PATTERNS)
def test_pack_map_points_on_crafted_sets(crafted, name, driver):
    """points and counts equal map_ref; every byte outside the kept ranges keeps its 0xA5 (the expected buffer has
    it there)"""
    rng = np.random.default_rng(100 + PATTERNS.index((name, driver)))
    keeps = crafted.pattern(name, rng)
    filt, planes = crafted.planes(keeps, driver, rng)
    h = Handle(0, 1024)
    got, counts, want, want_counts = crafted.call(h, filt, planes)
    assert want_counts == [int(k.sum()) for k in keeps]          # (the planes do drive the pattern)
    assert counts == want_counts, (name, driver)
    assert got == want, (name, driver)
    h.close()


def test_pack_map_points_reversed_null_points_and_chunks(crafted, monkeypatch):
    """the same call in reversed set order; NULL points writes only the counts; a table of 2 tiles gives the same"""
    rng = np.random.default_rng(99)
    keeps = crafted.pattern("0.5", rng)
    filt, planes = crafted.planes(keeps, "combined", rng)
    h = Handle(0, 1024)
    got, counts, want, want_counts = crafted.call(h, filt, planes)
    assert got == want and counts == want_counts
    got_r, counts_r, want_r, want_counts_r = crafted.call(h, filt, planes, reverse=True)
    assert want_counts_r == want_counts[::-1] and want_r != want
    assert got_r == want_r and counts_r == want_counts_r
    none, counts_n, _, _ = crafted.call(h, filt, planes, with_points=False)
    assert none is None and counts_n == want_counts
    monkeypatch.setenv("SVO_MAP_TABLE_TILES", "2")
    got_c, counts_c, _, _ = crafted.call(h, filt, planes)
    assert got_c == want and counts_c == want_counts
    got_c, counts_c, _, _ = crafted.call(h, filt, planes, reverse=True)
    assert got_c == want_r and counts_c == want_counts_r
    h.close()


def test_pack_map_points_rejects_bad_calls():
    h = Handle(0, 1024)
    lib = hip_lib.lib()
    keep = []
    n = 5
    z = np.zeros(n, np.uint32)
    fields = {name: _device_plane(z, 4, keep) for name in ("flags", "keyframe_id", "inlier_count", "color")}
    fields["kps3d"] = _device_plane(np.zeros((n, 3), np.uint32), 4, keep)
    points = torch.full((16, 16), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), -7, dtype=torch.int32, device="cuda")

    def call(n_regions=1, begin=(0, 1), n_kp=n, first=(0,), filt=None, points_at=0, counts_at=0, **replace):
        ks = hip_lib.Keypoints()
        ks.n = n_kp
        for name, v in dict(fields, **replace).items():
            setattr(ks, name, v)
        f = MapFilter(**(filt or {}))
        return lib.svo_pack_map_points(h._h, n_regions, (C.c_int32 * len(begin))(*begin), C.byref(ks), (C.c_int32 * 1)(0),
                                       (C.c_int64 * len(first))(*first), C.byref(f), C.c_void_p(points.data_ptr() + points_at),
                                       C.c_void_p(counts.data_ptr() + counts_at))

    assert call(points_at=4) == -1 and call(points_at=8) == -1              # misaligned points
    assert call(counts_at=2) == -1
    assert call(filt=dict(drop_flags=8)) == -1 and call(filt=dict(drop_flags=0x80000001)) == -1
    assert call(filt=dict(_reserved=1)) == -1
    assert call(n_regions=-1) == -1
    assert call(begin=(1, 1)) == -1 and call(n_regions=2, begin=(0, 1, 0), first=(0, 8)) == -1
    assert call(first=(-1,)) == -1
    assert call(n_kp=-1) == -1
    assert call(flags=None) == -1 and call(kps3d=fields["kps3d"] + 2) == -1
    h.synchronize()
    assert np.all(points.cpu().numpy() == 0xA5) and np.all(counts.cpu().numpy() == -7)
    assert call() == 0                                                       # all-zero planes pass the all-zero filter
    assert counts.cpu().numpy().tolist() == [n, -7, -7, -7] and np.all(points.cpu().numpy()[n:] == 0xA5)
    assert call(filt=dict(drop_flags=7, own_only=1, min_inliers=3)) == 0     # inlier_count 0 < 3
    assert counts.cpu().numpy().tolist() == [0, -7, -7, -7]
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


@pytest.fixture(scope="module")
def tiny():
    """tiny, seeds (1, 11, 12, 13, 14), 24 frames of fast motion: shared, never changed"""
    return _sequences("tiny", (1, 11, 12, 13, 14), 24)


def _frame_set(n, live):
    """live: {slot: (sequence tuple, frame index)} -> lefts, rights, time stamps of new_images / pack_images"""
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for slot, (seq, k) in live.items():
        L[slot], R[slot], ts[slot] = seq[0][k], seq[1][k], seq[2][k]
    return L, R, ts


def _getter_sets(batch, s, from_kf=0):
    """the keyframes of slot s from from_kf on as the getters return them: map_ref sets and (id, n, pose bytes)"""
    sets, meta = [], []
    for k in range(from_kf, batch.num_keyframes(s)):
        f = batch.get_keyframe(k, s)
        info = f.info
        flags = (info["ignore_during_refinement"].astype(np.uint32) * MR.IGNORE_DURING_REFINEMENT |
                 info["ignore_completely"].astype(np.uint32) * MR.IGNORE_COMPLETELY |
                 info["ignore_temporary"].astype(np.uint32) * MR.IGNORE_TEMPORARY)
        col = info["color"].astype(np.uint32).reshape(-1, 3)
        planes = {"flags": flags, "keyframe_id": np.ascontiguousarray(info["keyframe_id"]).view(np.uint32),
                  "inlier_count": np.ascontiguousarray(info["inlier_count"]).view(np.uint32),
                  "color": col[:, 0] | col[:, 1] << 8 | col[:, 2] << 16}
        sets.append((len(info), k, np.ascontiguousarray(f.kps3d), planes))
        meta.append((k, len(info), f.pose.tobytes()))
    return sets, meta


def _check_slot(tag, m, i, s, source, filt, from_kf=0):
    """named slot i of the export (slot s) against the getters of `source`; returns the kept counts per keyframe"""
    seg, r = m.segments[i], m.regions[i]
    sets, meta = _getter_sets(source, s, from_kf)
    assert int(seg["seq"]) == s and int(seg["status"]) == hip_lib.MAP_COMPLETE, (tag, s)
    assert int(seg["n_keyframes"]) == source.num_keyframes(s) and int(seg["from_keyframe"]) == from_kf, (tag, s)
    assert int(seg["n_exported"]) == len(sets) and not np.any(seg["_pad"]), (tag, s)
    bound = sum(n for n, *_ in sets)
    assert int(seg["points_bound"]) == bound, (tag, s)
    want, counts = MR.pack([sets], [0], filt, bound)
    assert int(seg["n_points"]) == sum(counts), (tag, s)
    assert m.points(i).tobytes() == want[:sum(counts)].tobytes(), (tag, s)
    kfs = m.keyframes(i)
    assert len(kfs) == len(sets)
    at = 0
    for j, (k, n_total, pose) in enumerate(meta):
        e = kfs[j]
        assert (int(e["id"]), int(e["n_total"]), int(e["n"]), int(e["_pad"])) == (k, n_total, counts[j], 0), (tag, s, k)
        assert int(e["first"]) == int(r["first_point"]) + at and e["pose"].tobytes() == pose, (tag, s, k)
        assert m.points_of_keyframe(i, j).tobytes() == want[at:at + counts[j]].tobytes(), (tag, s, k)
        at += counts[j]
    return counts, [n for _, n, _ in meta]


def _check_all(tag, batch, slots, source=None, filters=(MR.KEEP_ALL, OWN_CURRENT, INLIERS_8, COMBINED), device=False):
    """every filter's export of the slots against the getters; returns per filter {slot: (kept, totals per keyframe)}"""
    source = source or batch
    out = []
    for filt in filters:
        m = batch.export_map(slots, filter=filt, device=device)
        res = {s: _check_slot(tag, m, i, s, source, filt) for i, s in enumerate(slots)}
        if filt == MR.KEEP_ALL:
            assert all(kept == totals for kept, totals in res.values()), tag
        out.append(res)
    return out


def _run_against_getters(cfg, seqs, n_slots, steps, starts):
    """slot s plays sequence s % len(seqs) from step starts[s] on; after every fourth step and the last one the
    exports equal the getters. Returns what the last check saw."""
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    slots = list(range(n_slots))
    for t in range(steps):
        live = {s: (seqs[s % len(seqs)], t - starts[s]) for s in slots if t >= starts[s]}
        batch.new_images(*_frame_set(n_slots, live))
        if t % 4 == 3 or t == steps - 1:
            res = _check_all(f"step {t}", batch, slots)
            m = batch.export_map(slots)
            for i, s in enumerate(slots):
                assert int(m.segments[i]["frame_id"]) == t - starts[s] == batch.stats(s).frame_id, (t, s)
                assert int(m.segments[i]["run"]) == 0 and np.float32(m.segments[i]["time_stamp"]) == np.float32(live[s][0][2][live[s][1]])
    groups = batch.groups()
    batch.close()
    return groups, res


def _assert_shows_something(res):
    """some slot has two keyframes, and the own-and-current filter drops and keeps points in a later keyframe"""
    unfiltered, own = res[0], res[1]
    assert any(len(totals) >= 2 for _, totals in unfiltered.values()), "a slot with at least 2 keyframes"
    assert any(0 < kept[j] < totals[j] for kept, totals in own.values() for j in range(1, len(totals))), \
        "the filtered export both drops and keeps points in a keyframe after the first"


def test_ctx_against_the_getters_one_group(tiny, monkeypatch):
    """tiny, 5 slots in one group, 24 frames of fast motion, starts [0, 0, 1, 2, 0]"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    cfg, seqs = tiny
    groups, res = _run_against_getters(cfg, seqs, 5, 24, [0, 0, 1, 2, 0])
    assert groups == 1
    _assert_shows_something(res)


def test_wave_boundaries_in_the_ctx(monkeypatch):
    """euroc, 4 slots in 2 groups, seeds (3, 4), 16 frames: keyframes of more than 64 and fewer than 256 points"""
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = _sequences("euroc", (3, 4), 16)
    groups, res = _run_against_getters(cfg, seqs, 4, 16, [0, 0, 0, 0])
    assert groups == 2
    totals = [n for _, t in res[0].values() for n in t]
    assert all(64 < n < 256 for n in totals), totals
    assert any(len(t) >= 2 for _, t in res[0].values()), "a slot with a second keyframe"


def test_a_tile_table_smaller_than_the_export(tiny, monkeypatch):
    """SVO_MAP_TABLE_TILES=2: seven slots need at least seven tiles, so every export goes out as several chunks
    with the table refilled in between; the result is the same"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    monkeypatch.setenv("SVO_MAP_TABLE_TILES", "2")
    cfg, seqs = tiny
    groups, res = _run_against_getters(cfg, seqs[:3], 7, 8, [0, 0, 1, 0, 2, 0, 1])
    assert groups == 1 and len(res[0]) == 7


# ---------------------------------------------------------------------------------- named slots, from_keyframe, states

def test_named_slots_from_keyframe_and_states(tiny, monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "3")
    cfg, seqs = tiny
    n_slots, steps = 7, 24
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 3
    # slot 5 never starts; slot 6 is restarted after step 11 and stays empty; slot 3 is restarted after step 11 and
    # plays another sequence from step 14 on
    for t in range(steps):
        live = {s: (seqs[s % 5], t) for s in (0, 1, 2, 4)}
        if t < 12:
            live[3], live[6] = (seqs[3], t), (seqs[1], t)
        elif t >= 14:
            live[3] = (seqs[2], t - 14)
        batch.new_images(*_frame_set(n_slots, live))
        if t == 11:
            batch.restart([3, 6])
    counts = [batch.num_keyframes(s) for s in range(n_slots)]
    assert counts[5] == 0 and counts[6] == 0 and max(counts) >= 2
    assert batch.map_size(5) == (0, 0) and batch.map_size(0, counts[0]) == (0, 0) and batch.map_size(0, counts[0] + 3) == (0, 0)
    # a subset in shuffled order, regions placed back to front with gaps, every from_keyframe of the list
    named = [4, 6, 0, 3, 5, 2]
    for frm in (0, 1, "count", "beyond"):
        from_kf = [counts[s] if frm == "count" else counts[s] + 2 if frm == "beyond" else frm for s in named]
        sizes = [batch.map_size(s, f) for s, f in zip(named, from_kf)]
        regions = np.zeros(len(named), hip_lib.MAP_REGION_DTYPE)
        at_p, at_k = 3, 1
        for i in reversed(range(len(named))):
            regions[i] = (at_p, sizes[i][1], at_k, sizes[i][0], from_kf[i])
            at_p += sizes[i][1] + 2
            at_k += sizes[i][0] + 1
        for filt in (MR.KEEP_ALL, OWN_CURRENT):
            m = MapExport(batch, named, filter=filt, regions=regions)
            m.points_buffer.fill_(0xA5)
            m._kfs.view(np.uint8)[:] = 0xA5
            m.submit().wait()
            used_p, used_k = np.zeros(m.capacity, bool), np.zeros(len(m._kfs), bool)
            for i, s in enumerate(named):
                seg = m.segments[i]
                if s in (5, 6):
                    assert (int(seg["frame_id"]), int(seg["n_keyframes"]), int(seg["keyframes_retired"]), int(seg["n_exported"]),
                            int(seg["n_points"]), int(seg["points_bound"])) == (-1, 0, 0, 0, 0, 0), (frm, s)
                    assert int(seg["run"]) == (1 if s == 6 else 0) and float(seg["time_stamp"]) == 0.0
                    assert int(seg["status"]) == hip_lib.MAP_COMPLETE and int(seg["from_keyframe"]) == from_kf[i]
                else:
                    _check_slot(f"from {frm}", m, i, s, batch, filt, from_kf[i])
                    assert int(seg["run"]) == (1 if s == 3 else 0)
                    assert int(seg["n_exported"]) == max(0, counts[s] - from_kf[i]) == sizes[i][0]
                    assert int(seg["points_bound"]) == sizes[i][1]
                lo = int(regions[i]["first_point"])
                used_p[lo:lo + int(seg["n_points"])] = True
                lo = int(regions[i]["first_keyframe_entry"])
                used_k[lo:lo + int(seg["n_exported"])] = True
            # of a region exactly the kept records and the exported entries are written
            assert np.all(m.points_buffer.numpy()[:m.capacity][~used_p] == 0xA5), frm
            assert np.all(m._kfs.view(np.uint8).reshape(len(m._kfs), -1)[~used_k] == 0xA5), frm
            assert int(m.segments["n_points"].sum()) == int(used_p.sum())
    # the restarted slot's map is its new run's
    assert int(batch.export_map([3]).segments[0]["frame_id"]) == steps - 1 - 14
    batch.close()


def _raw_submit(batch, seqs, n, regions, filt, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_map(batch._ctx, arr, n, regions.ctypes.data_as(C.c_void_p),
                                               None if filt is None else C.byref(filt), C.byref(dst), mem)


def test_rejected_calls(tiny, monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = tiny
    n_slots = 4
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    for t in range(2):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s], t) for s in range(n_slots)}))
    cap = batch.export_capacity()
    seg = np.zeros(n_slots, hip_lib.MAP_SEGMENT_DTYPE)
    kfs = np.zeros(2 * n_slots, hip_lib.MAP_KEYFRAME_DTYPE)
    pts = np.zeros((n_slots * 2 * cap + 1, 16), np.uint8)
    base = pts.ctypes.data + (-pts.ctypes.data) % 16
    good = np.zeros(n_slots, hip_lib.MAP_REGION_DTYPE)
    for i in range(n_slots):
        good[i] = (i * 2 * cap, 2 * cap, 2 * i, 2, 0)
    dst = hip_lib.MapDst(seg.ctypes.data, kfs.ctypes.data, base)
    H = hip_lib.MEM_HOST

    def changed(i, **kw):
        r = good.copy()
        for k, v in kw.items():
            r[i][k] = v
        return r

    assert _raw_submit(batch, [0, 0], 2, good, None, dst, H) == -1                 # named twice
    assert _raw_submit(batch, [0, n_slots], 2, good, None, dst, H) == -1           # out of range
    assert _raw_submit(batch, [-1, 1], 2, good, None, dst, H) == -1
    assert _raw_submit(batch, [0, 1], 2, good, None, dst, 2) == -1                 # SVO_MEM_DEVICE_BORROW is no export mode
    assert _raw_submit(batch, [0, 1], 2, good, None, dst, 7) == -1
    assert _raw_submit(batch, [0, 1], 2, good, None, hip_lib.MapDst(None, kfs.ctypes.data, base), H) == -1
    assert _raw_submit(batch, [0, 1], 2, good, None, hip_lib.MapDst(seg.ctypes.data, None, base), H) == -1
    assert _raw_submit(batch, [0, 1], 2, good, None, hip_lib.MapDst(seg.ctypes.data, kfs.ctypes.data, None), H) == -1
    for field in ("first_point", "point_capacity", "first_keyframe_entry", "keyframe_capacity", "from_keyframe"):
        assert _raw_submit(batch, [0, 1], 2, changed(1, **{field: -1}), None, dst, H) == -1, field
    for off in (4, 8, 12):
        assert _raw_submit(batch, [0, 1], 2, good, None, hip_lib.MapDst(seg.ctypes.data, kfs.ctypes.data, base + off), H) == -1
    assert _raw_submit(batch, [0, 1], 2, good, MapFilter(drop_flags=8), dst, H) == -1
    assert _raw_submit(batch, [0, 1], 2, good, MapFilter(_reserved=1), dst, H) == -1
    with pytest.raises(hip_lib.SvoError):
        batch.map_size(0, -1)
    with pytest.raises(hip_lib.SvoError):
        batch.map_size(n_slots)
    assert not seg.view(np.uint8).any() and not kfs.view(np.uint8).any() and not pts.any()
    # NULL arrays are fine while every capacity of theirs is 0: the slots come back TOO_SMALL with the counts needed
    none = changed(0, point_capacity=0, keyframe_capacity=0)
    none[1]["point_capacity"] = none[1]["keyframe_capacity"] = 0
    assert _raw_submit(batch, [0, 1], 2, none, None, hip_lib.MapDst(seg.ctypes.data, None, None), H) == 0
    batch.wait()
    assert [int(x) for x in seg["status"][:2]] == [hip_lib.MAP_TOO_SMALL] * 2
    assert [(int(e["n_exported"]), int(e["points_bound"])) for e in seg[:2]] == [batch.map_size(0), batch.map_size(1)]
    # the good call is accepted (every slot: seqs NULL, n ignored), and the ctx has kept working
    assert _raw_submit(batch, None, 0, good, MapFilter(), dst, H) == 0
    batch.wait()
    m = batch.export_map()
    assert seg.tobytes() == m.segments.tobytes()
    for i in range(n_slots):
        n = int(seg[i]["n_points"])
        lo = base - pts.ctypes.data + 16 * int(good[i]["first_point"])
        assert n > 0 and pts.reshape(-1)[lo:lo + 16 * n].tobytes() == m.points(i).tobytes()
    batch.new_images(*_frame_set(n_slots, {s: (seqs[s], 2) for s in range(n_slots)}))
    _check_all("after the errors", batch, list(range(n_slots)), filters=(MR.KEEP_ALL,))
    batch.close()


def test_retired_prefix_is_final(monkeypatch):
    """tiny, seed 12, motion_scale 8 (the sequence of the snapshot tests: keyframes 0 and 1 are both retired from
    frame 44 on): keyframes_retired is what svo_snapshot_size's twin, a saved header, reports; the points of the
    keyframes below it are byte-equal across two later polls, and a poll from there on is the tail of a full one"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n = 50
    cfg, L, R, _, ts = synth.make_sequence("tiny", n, 12, device="cpu", motion_scale=8.0)
    L, R = [x.numpy() for x in L], [x.numpy() for x in R]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1)
    polls = {}
    for k in range(n):
        batch.new_images([L[k]], [R[k]], [float(ts[k])])
        if k in (45, 47, 49):
            m = batch.export_map()
            retired = int(m.segments[0]["keyframes_retired"])
            assert retired == batch.save([0])[0].info.keyframes_retired, k
            _check_slot(f"frame {k}", m, 0, 0, batch, MR.KEEP_ALL)
            polls[k] = (retired, m)
    r0, first = polls[45]
    assert r0 >= 1, "a retired prefix"
    prefix = b"".join(first.points_of_keyframe(0, j).tobytes() for j in range(r0))
    assert len(prefix) > 0
    for k in (47, 49):
        retired, m = polls[k]
        assert retired >= r0
        assert b"".join(m.points_of_keyframe(0, j).tobytes() for j in range(r0)) == prefix, k
        assert m.keyframes(0)[:r0].tobytes() == first.keyframes(0)[:r0].tobytes()
        tail = batch.export_map([0], from_keyframe=r0) if k == 49 else None
        if tail is not None:
            assert int(tail.segments[0]["from_keyframe"]) == r0
            assert tail.points(0).tobytes() == m.points(0).tobytes()[len(prefix):]
            assert [int(x) for x in tail.keyframes(0)["id"]] == list(range(r0, int(m.segments[0]["n_keyframes"])))
    batch.close()


# ---------------------------------------------------------------------------------- TOO_SMALL

def test_too_small(tiny, monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "1")
    cfg, seqs = tiny
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 3)
    for t in range(3):
        batch.new_images(*_frame_set(3, {s: (seqs[s], t) for s in range(3)}))
    sizes = [batch.map_size(s) for s in range(3)]
    assert all(k >= 1 and p >= 1 for k, p in sizes)
    # slot 0: one point short of its bound; slot 1: one keyframe entry short; slot 2 fits
    m = MapExport(batch, [0, 1, 2], point_capacity=[sizes[0][1] - 1, sizes[1][1], sizes[2][1]],
                  keyframe_capacity=[sizes[0][0], sizes[1][0] - 1, sizes[2][0]])
    m.points_buffer.fill_(0xA5)
    m._kfs.view(np.uint8)[:] = 0xA5
    m.submit().wait()                                             # (svo_wait returns SVO_OK: no SvoError)
    for i in (0, 1):
        seg = m.segments[i]
        assert int(seg["status"]) == hip_lib.MAP_TOO_SMALL and int(seg["n_points"]) == 0
        assert (int(seg["n_exported"]), int(seg["points_bound"])) == sizes[i]
        assert int(seg["frame_id"]) == 2 and int(seg["n_keyframes"]) == sizes[i][0]
        assert len(m.keyframes(i)) == 0
    _check_slot("the slot that fits", m, 2, 2, batch, MR.KEEP_ALL)
    lo = int(m.regions[2]["first_point"])
    assert lo == sizes[0][1] - 1 + sizes[1][1]
    assert np.all(m.points_buffer.numpy()[:lo] == 0xA5)
    k_lo = int(m.regions[2]["first_keyframe_entry"])
    assert np.all(m._kfs.view(np.uint8).reshape(len(m._kfs), -1)[:k_lo] == 0xA5)
    # the ctx has not failed: the next frame tracks
    batch.new_images(*_frame_set(3, {s: (seqs[s], 3) for s in range(3)}))
    assert [batch.stats(s).frame_id for s in range(3)] == [3, 3, 3]
    # regrown from the segments' counts, the same export is complete
    assert m.grow()
    m.submit().wait()
    assert not m.grow()
    for i in range(3):
        _check_slot("regrown", m, i, i, batch, MR.KEEP_ALL)
    # the wrapper recovers by itself when the sizes it asked for turn out too small
    real = batch.map_size
    monkeypatch.setattr(batch, "map_size", lambda s, f=0: tuple(max(0, x - 1) for x in real(s, f)))
    again = batch.export_map()
    monkeypatch.undo()
    for i in range(3):
        _check_slot("export_map", again, i, i, batch, MR.KEEP_ALL)
    batch.close()


# ---------------------------------------------------------------------------------- ordering, device mode, side effects

def test_ordering_without_draining(tiny, monkeypatch):
    """frame set t, map A, frame set t+1, map B, one wait: A is the map at t, B at t+1 (a twin ctx stopped at each)"""
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = tiny
    n_slots, t = 6, 7
    sets = [_frame_set(n_slots, {s: (seqs[s % 5], k) for s in range(n_slots)}) for k in range(t + 2)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 2
    for k in range(t):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
    room = dict(point_capacity=(t + 2) * batch.export_capacity(), keyframe_capacity=t + 2)   # (what t + 2 frames can make at most)
    packed = [batch.pack_images(*sets[k]) for k in (t, t + 1)]
    batch.submit_packed(packed[0])
    a = [batch.submit_map(filter=f, **room) for f in (MR.KEEP_ALL, OWN_CURRENT)]
    batch.submit_packed(packed[1])
    b = [batch.submit_map(filter=f, **room) for f in (MR.KEEP_ALL, OWN_CURRENT)]
    batch.wait()
    for maps, k in ((a, t), (b, t + 1)):
        twin.new_images(*sets[k])
        for m, f in zip(maps, (MR.KEEP_ALL, OWN_CURRENT)):
            assert [int(x) for x in m.segments["frame_id"]] == [k] * n_slots
            for s in range(n_slots):
                _check_slot(f"frame {k}", m, s, s, twin, f)
    batch.close()
    twin.close()


def test_device_mode_gives_the_same_bytes(tiny, monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = tiny
    n_slots = 6
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    for k in range(12):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 5], k) for s in range(n_slots) if s != 4}))
    for named in (None, [5, 2, 4, 0]):
        for filt in (MR.KEEP_ALL, COMBINED):
            host = batch.export_map(named, filter=filt)
            dev = batch.export_map(named, filter=filt, device=True)
            assert dev.points_buffer.is_cuda and dev.points_buffer.dtype == torch.uint8 and dev.points_buffer.shape[1] == 16
            assert host.segments.tobytes() == dev.segments.tobytes()
            dev.points_buffer.fill_(0xA5)
            dev.submit().wait()
            inside = np.zeros(max(dev.capacity, 1), bool)
            for i in range(len(host.segments)):
                assert host.keyframes(i).tobytes() == dev.keyframes(i).tobytes(), (named, i)
                assert host.points(i).tobytes() == dev.points(i).tobytes(), (named, i)
                lo = int(dev.regions[i]["first_point"])
                inside[lo:lo + int(dev.segments[i]["n_points"])] = True
            assert np.all(dev.points_buffer.cpu().numpy()[~inside] == 0xA5), (named, filt)
    batch.close()


def test_no_side_effects(tiny, monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = tiny
    n_slots, steps = 6, 12
    sets = [_frame_set(n_slots, {s: (seqs[s % 5], k) for s in range(n_slots)}) for k in range(steps)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)      # exports its map after every step
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)       # never does
    maps = []
    for k in range(steps):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
        if k == 0:
            assert batch.memory().device_bytes == twin.memory().device_bytes
        maps.append((batch.export_map(filter=OWN_CURRENT), batch.export_map(device=True)))
    grown = batch.memory().device_bytes - twin.memory().device_bytes
    bound = sum(batch.map_size(s)[1] for s in range(n_slots))
    assert 0 < grown <= 16 * bound + 2 * 4096, grown      # the staging points and two groups' counts blocks (1024 ints)
    for s in range(n_slots):
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes() and len(twin.get_trajectory(s)) == steps
        assert batch.num_keyframes(s) == twin.num_keyframes(s)
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        _check_slot("last", maps[-1][0], s, s, twin, OWN_CURRENT)
        _check_slot("last", maps[-1][1], s, s, twin, MR.KEEP_ALL)
    batch.close()
    twin.close()


def test_wire_keyframes_messages(tiny, monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    cfg, seqs = tiny
    n_slots = 5
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    for k in range(16):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s], k) for s in range(n_slots) if s != 3}))
    assert max(batch.num_keyframes(s) for s in range(n_slots)) >= 2
    for named in (None, [4, 3, 0]):
        texts = wire.keyframes_messages(batch, named)
        assert texts == [wire.keyframes_message(batch, s) for s in (range(n_slots) if named is None else named)]
    assert wire.keyframes_messages(batch, [3]) == ["[]"]
    batch.close()
