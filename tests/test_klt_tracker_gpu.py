"""klt_track_kernel in the form the tracker launches it (fused projection, reference gathered through kp_index,
the keyframe's template cache), through the diagnostic entry svo_klt_track_batch, against the CPU oracle on the
cases of tests/klt_tracker_cases.py. Every comparison is bit for bit (a NaN equals a NaN); a test collects every
case that differs and names them all. tests/test_klt_tracker_cpu.py asserts what the cases reach.

The cache memory is the test's: one allocation per launch, filled with pseudo-random bytes, out of which every
keyframe's record block and flag block are carved with guard zones between them. So a test can say which bytes a
call may have written and look at all the others.

  ring off            every case without a cache, through proj_pose and through proj_mats: projection and gather alone
  miss, hit, hit      call 1 stores, call 2 loads for the same frame, call 3 loads for another frame and pose whose
  elsewhere           starts lie near, far from or out of range of where call 1 looked; in five image layouts
  record discipline   which flags and bytes a miss writes, headers against the numpy statement, hits on records of
                      flat / outside levels whose bodies hold garbage
  ignored caches      a cache of another window, no cache beside cached keyframes, kp_index >= tmpl_cap
  several keyframes   three keyframes of 3, 2 and 1 levels in one launch; kf_id null against all zero
  batch               five sequences of 0, 1, 63, 65 and n_bound points in one launch against five lone launches
The ctx's own ring (SVO_KLT_CACHE_KF, three slots wrapping at different steps, both kernel shapes) is
tests/test_tracker_gpu.py::test_klt_ring_of_three_slots_changes_nothing.

RUN TIME on an MI355X: 7.0 s for the whole file (its 17 comparison tests; the slowest, test_ring_off[proj_pose], 1.5 s with the
first launch of the process; every other test below 0.8 s).

SEEDED ERRORS. Scratch builds of the library with one line changed each, run once on an MI355X against this file
plus the ring test (19 tests, "new") and against the KLT tests there were before (41 tests: test_window_gpu.py's KLT
and tracker tests, test_parity_gpu.py's KLT tests, test_tracker_gpu.py's sequence, keyframe and cache tests,
test_restart_gpu.py's stale-cache test, "earlier"):
  record addressed with kp instead of kp_index        new: 15 red (82 of 246 calls per layout: every hit)   earlier: 12 red
  vflag without `+ level`                              new: 17 red (all three calls of nearly every case)    earlier: 20 red
  the `tmpl_win == a.win` test dropped                 new: 2 red (test_ignored_caches, all 3 calls)         earlier: none
  hq1 halves of cI1 swapped                            new: 15 red (140 of 246 calls per layout; headers)    earlier: 12 red
  a cached KLT_FLAT treated as KLT_TRACK on a hit      new: 13 red (98 of 246 calls per layout)              earlier: none
  evict_id off by one (id - tmpl_kf - 1)               new: 2 red (the ring test, both windows)              earlier: 1 red
  tile_regs kept for iteration 0 whatever the window   new: none                                             earlier: none
    No value-based test can see this one: the tile that a cached level requests ahead is computed from the very
    position that iteration 0 looks at (nextx - halfWin of the level's start, before and after), and the tile spans
    the window with KLT_MARGIN to spare on every side, so iteration 0's test of the requested tile never fails; the
    later iterations keep their test. (A later call's start outside an EARLIER call's tile is a different matter and
    is what "hit elsewhere" runs: nothing of a tile survives a call.)
  `kpi <= tmpl_cap`, and the flag set for kp_index >= tmpl_cap: NOT run, judged from the code: both write past the
    caller's blocks (a whole record, or flag bytes up to three times the keyframe's surplus of keypoints past the
    flag block). The cases hold the inputs that would show either: in every fifth case and in test_ignored_caches
    one point has kp_index == tmpl_cap exactly and others lie beyond it (test_klt_tracker_cpu.py asserts both), the
    flags are compared with expected_flags and every byte outside the blocks with what it held before.
"""
import numpy as np
import pytest
import torch

import klt_tracker_cases as KC
import window_cases as WC
from geometry_cases import same_bits
from stereo_svo_slam_amd import hip_lib
from test_window_gpu import LAYOUTS, guard_value, place  # noqa: F401 (guard_value: what `place` surrounds a view with)

pytestmark = pytest.mark.gpu

FILL = 0x5A                      # output arrays before a call
GUARD = 512                      # bytes between two carved blocks
OUT_BYTES = dict(tracked=8, status=1, err=4, proj=8, ref=8)
OUT_TYPES = dict(tracked=np.float32, status=np.uint8, err=np.float32, proj=np.float32, ref=np.float32)


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=4096)
    yield h
    h.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _round(n, to=256):
    return (n + to - 1) // to * to


def other_window(win):
    """a window of the other kernel shape (its records have another size)"""
    return 35 if win <= 31 else 31


class Launch:
    """a launch of klt_tracker_cases on the device: images as views in a layout, the caches carved out of one block"""

    def __init__(self, H, seqs, cur_layout="dense", kf_layout="dense", n_bound=None, seed=1):
        self.H, self.seqs, self.win = H, seqs, seqs[0]["win"]
        self.n_bound = max(s["n"] for s in seqs) if n_bound is None else n_bound
        self.rec, self.hdr_off, self.hdr_bytes, self.levels = hip_lib.klt_cache_layout(self.win)
        assert self.levels == KC.LK_LEVELS
        off, self.blocks = GUARD, {}
        for b, s in enumerate(seqs):
            for k, kf in enumerate(s["kfs"]):
                if kf["cache"] is None:
                    continue
                own = kf["cache"] == "own"
                twin = self.win if own else other_window(self.win)
                # (a cache of another window is sized for either record size: nothing may touch it, and nothing that did
                # by mistake would leave the allocation)
                r = self.rec if own else max(self.rec, hip_lib.klt_cache_layout(twin)[0])
                blk = dict(cap=kf["tmpl_cap"], twin=twin, own=own, r=r, rec_off=off, rec_len=kf["tmpl_cap"] * self.levels * r)
                off += _round(blk["rec_len"]) + GUARD
                blk["flag_off"], blk["flag_len"] = off, kf["tmpl_cap"] * self.levels
                off += _round(blk["flag_len"]) + GUARD
                self.blocks[b, k] = blk
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.mem = torch.randint(0, 256, (off,), dtype=torch.uint8, device="cuda", generator=gen)
        assert self.mem.data_ptr() % 256 == 0
        for blk in self.blocks.values():
            self.mem[blk["flag_off"]:blk["flag_off"] + blk["flag_len"]] = 0 if blk["own"] else 1
        nb = max(self.n_bound, 1)
        self.out = [{k: torch.empty(nb * sz, dtype=torch.uint8, device="cuda") for k, sz in OUT_BYTES.items()} for _ in seqs]
        self.dev = []
        for b, s in enumerate(seqs):
            kfs = []
            for k, kf in enumerate(s["kfs"]):
                blk = self.blocks.get((b, k))
                kfs.append(dict(lk=[place(x, kf_layout) for x in kf["levels"]], kps2d=dev(kf["kps2d"]),
                                tmpl=self.mem[blk["rec_off"]:blk["rec_off"] + blk["rec_len"]] if blk else None,
                                valid=self.mem[blk["flag_off"]:blk["flag_off"] + blk["flag_len"]] if blk else None,
                                tmpl_cap=kf["tmpl_cap"], tmpl_win=blk["twin"] if blk else 0))
            o = self.out[b]
            d = dict(kfs=kfs, n=dev(np.array([s["n"]], np.int32)), tracked=o["tracked"], status=o["status"], err=o["err"],
                     proj_out=o["proj"], ref_out=o["ref"])
            self.dev.append(d)
            self.set_frame(b, s, cur_layout)

    def _pad(self, a, fill):
        out = np.full((max(self.n_bound, 1),) + a.shape[1:], fill, a.dtype)
        out[:len(a)] = a
        return dev(out)

    def set_frame(self, b, s, cur_layout="dense"):
        """the current image, pose, points and camera of sequence b from s (the caches and keyframes stay)"""
        d = self.dev[b]
        d["cur"] = [place(x, cur_layout) for x in s["cur"]]
        d["kf_id"] = None if s["kf_id"] is None else self._pad(s["kf_id"], 0)
        d["kp_index"] = self._pad(s["kp_index"], 0)
        d["kps3d"] = self._pad(s["kps3d"], 7e7)
        d["pose"] = dev(np.asarray(s["pose"], np.float32))
        d["cam"] = hip_lib.CameraSettings.from_dict(s["cam"])
        d["n"] = dev(np.array([s["n"]], np.int32))

    def run(self, use_mats):
        """one call; per sequence dict(tracked, status, err, proj, ref) of n_bound entries (numpy)"""
        for o in self.out:
            for t in o.values():
                t.fill_(FILL)
        self.H.klt_track_batch(self.dev, self.n_bound, self.win, use_mats)
        res = []
        for o in self.out:
            r = {k: o[k].cpu().numpy().view(OUT_TYPES[k]) for k in o}
            res.append({k: (v.reshape(-1, 2) if OUT_BYTES[k] == 8 else v) for k, v in r.items()})
        return res

    def flags(self, mem, b, k):
        blk = self.blocks[b, k]
        return mem[blk["flag_off"]:blk["flag_off"] + blk["flag_len"]].reshape(blk["cap"], self.levels)

    def records(self, mem, b, k):
        blk = self.blocks[b, k]
        return mem[blk["rec_off"]:blk["rec_off"] + blk["rec_len"]].reshape(blk["cap"], self.levels, blk["r"])

    def outside_blocks(self, mem):
        """the bytes of the allocation that belong to no block: guard zones and alignment gaps"""
        keep = np.ones(len(mem), bool)
        for blk in self.blocks.values():
            keep[blk["rec_off"]:blk["rec_off"] + blk["rec_len"]] = False
            keep[blk["flag_off"]:blk["flag_off"] + blk["flag_len"]] = False
        return mem[keep]


_EXPECTED = {}


def expected(seqs, key):
    """the oracle's answers for a launch, computed once per key"""
    if key not in _EXPECTED:
        _EXPECTED[key] = [KC.expected_sequence(s) for s in seqs]
    return _EXPECTED[key]


def differs(got, exp, n):
    """'' or what differs between one sequence's outputs and the oracle's answer; entries [n, n_bound) keep FILL"""
    for k in ("proj", "ref", "status", "tracked", "err"):
        g, e = got[k][:n], exp[k]
        eq = same_bits(g, e)
        bad = np.nonzero(~(eq if eq.ndim == 1 else eq.all(axis=1)))[0]
        if bad.size:
            return f"{k} of {bad.size} points, first {bad[:4].tolist()}: {g[bad[:2]].tolist()} for {e[bad[:2]].tolist()}"
        if not (got[k][n:].view(np.uint8) == FILL).all():
            return f"{k} written past the {n} points"
    return ""


def check_launch(failed, name, L, exp, use_mats):
    for b, (got, e) in enumerate(zip(L.run(use_mats), exp)):
        msg = differs(got, e, L.seqs[b]["n"])
        if msg:
            failed.append((f"{name} sequence {b}" if len(exp) > 1 else name, msg))


def _report(failed, total):
    assert not failed, f"{len(failed)} of {total} differ from the oracle:\n" + "\n".join(f"  {n}: {m}" for n, m in failed)


# ------------------------------------------------------------------ ring off
@pytest.mark.parametrize("use_mats", [0, 1], ids=["proj_pose", "proj_mats"])
def test_ring_off(H, use_mats):
    """no cache: the projection (both ways), the gather through kp_index and the build path, for both frames"""
    failed = []
    for c in KC.cases():
        for call in (1, 3):
            seqs = KC.single(c, call, cache=None)
            L = Launch(H, seqs)
            check_launch(failed, f"{c['name']} call {call}", L, expected(seqs, (c["name"], call)), use_mats)
    _report(failed, 2 * len(KC.cases()))


# ------------------------------------------------------------------ miss, hit, hit elsewhere
@pytest.mark.parametrize("layout", ["dense", "strided", "off1", "off3", "oddstride"])
def test_miss_hit_hit_elsewhere(H, layout):
    """call 1 on cleared flags builds and stores, call 2 loads for the same frame, call 3 for another image and pose.
    The keyframe's and the current frame's levels lie in `layout` (an unaligned current level drops the prefetch and
    stages its tiles byte by byte; the other tests of this file mix two layouts). A hit writes nothing: the cache
    after call 3 is the cache after call 1."""
    cur_layout = layout
    failed = []
    for k, c in enumerate(KC.cases()):
        seqs1, seqs3 = KC.single(c, 1), KC.single(c, 3)
        L = Launch(H, seqs1, cur_layout, layout, seed=k)
        check_launch(failed, f"{c['name']} call 1 (miss)", L, expected(seqs1, (c["name"], 1)), k & 1)
        after1 = L.mem.clone()
        flags = L.flags(after1, 0, 0).cpu().numpy()
        if not np.array_equal(flags, KC.expected_flags(seqs1[0])[0]):
            failed.append((c["name"], "flags after call 1"))
        check_launch(failed, f"{c['name']} call 2 (hit)", L, expected(seqs1, (c["name"], 1)), k & 1)
        L.set_frame(0, seqs3[0], cur_layout)
        check_launch(failed, f"{c['name']} call 3 (hit elsewhere)", L, expected(seqs3, (c["name"], 3)), (k >> 1) & 1)
        if not torch.equal(after1, L.mem):
            failed.append((c["name"], "a hit wrote to the cache"))
    _report(failed, 3 * len(KC.cases()))


# ------------------------------------------------------------------ record discipline
_STATEMENT = {}


def statement(c):
    """window_cases.klt_ref on the case's first frame (the small cases: the statement is slow)"""
    if c["name"] not in _STATEMENT:
        pl, cl, _ = KC.levels(c)
        _STATEMENT[c["name"]] = WC.klt_ref(pl, cl, c["table"][c["kp_index"]], KC.starts(c, 1), c["win"])[3]
    return _STATEMENT[c["name"]]


@pytest.mark.parametrize("shape", ["32 columns", "36 columns"])
def test_record_discipline(H, shape):
    failed = []
    n_headers = n_garbage_hits = 0
    for k, c in enumerate(KC.cases()):
        if (c["win"] <= 31) != (shape == "32 columns"):
            continue
        seqs = KC.single(c, 1)
        exp = expected(seqs, (c["name"], 1))
        L = Launch(H, seqs, seed=1000 + k)
        before = L.mem.cpu().numpy()
        # a miss reads nothing of a record: the answer is the oracle's whatever the records held
        check_launch(failed, f"{c['name']} call 1 on garbage records", L, exp, 1)
        after = L.mem.cpu().numpy()
        flags, want = L.flags(after, 0, 0), KC.expected_flags(seqs[0])[0]
        if not np.array_equal(flags, want):
            failed.append((c["name"], f"flags: {int((flags != want).sum())} differ"))
            continue
        if not np.array_equal(L.outside_blocks(before), L.outside_blocks(after)):
            failed.append((c["name"], "a guard byte changed"))
        rb, ra = L.records(before, 0, 0), L.records(after, 0, 0)
        stored = want.astype(bool)
        if not np.array_equal(rb[~stored], ra[~stored]):
            failed.append((c["name"], "a record without a flag changed"))
        hdr = ra[..., L.hdr_off:L.hdr_off + L.hdr_bytes]
        state = np.ascontiguousarray(hdr[..., :4]).view(np.int32)[..., 0]
        if not np.isin(state[stored], (KC.KLT_OUTSIDE, KC.KLT_FLAT, KC.KLT_TRACK)).all():
            failed.append((c["name"], "a stored header's state"))
            continue
        tail = slice(L.hdr_off + L.hdr_bytes, None)
        if not np.array_equal(rb[..., tail], ra[..., tail]):
            failed.append((c["name"], "bytes behind a header changed"))
        untracked = stored & (state != KC.KLT_TRACK)
        if not np.array_equal(rb[untracked][:, :L.hdr_off], ra[untracked][:, :L.hdr_off]):
            failed.append((c["name"], "the body of a flat / outside record was written"))
        # headers against the statement (the small cases)
        if len(c["pts"]) <= 40 and c["win"] in (5, 31, 35):
            info = statement(c)
            for i, kpi in enumerate(c["kp_index"]):
                if kpi >= c["tmpl_cap"]:
                    continue
                for level, lab in enumerate(info["labels"][i]):
                    st = {"prev_outside": KC.KLT_OUTSIDE, "flat": KC.KLT_FLAT}.get(lab, KC.KLT_TRACK)
                    h = np.ascontiguousarray(hdr[kpi, level])
                    ok = state[kpi, level] == st
                    if ok and st == KC.KLT_TRACK:
                        a = np.array([info["sums"][i, level, 0], info["a12"][i, level], info["sums"][i, level, 2]], np.float64)
                        a = a.astype(np.float32) * np.float32(1.0 / (1 << 20))
                        ci = info["ci"][i, level].astype(np.float64)
                        ok = same_bits(h[4:16].view(np.float32), a).all() and same_bits(h[16:32].view(np.float64), ci).all()
                        n_headers += 1
                    if not ok:
                        failed.append((c["name"], f"header of point {i} (kp_index {kpi}) level {level}"))
        # hits on flat / outside records whose bodies hold other garbage than before
        if untracked.any():
            blk = L.blocks[0, 0]
            recs = L.mem[blk["rec_off"]:blk["rec_off"] + blk["rec_len"]].view(blk["cap"], L.levels, L.rec)
            mask = torch.from_numpy(untracked).cuda()
            recs[..., :L.hdr_off][mask] = 0xEE
            n_garbage_hits += int(untracked.sum())
        check_launch(failed, f"{c['name']} call 2 (hit, garbage bodies)", L, exp, 0)
    assert n_headers >= 200 and n_garbage_hits >= 200, (n_headers, n_garbage_hits)
    _report(failed, "the cases")


# ------------------------------------------------------------------ caches that must be ignored
@pytest.mark.parametrize("win", [31, 35])
def test_ignored_caches(H, win):
    """a keyframe whose cache was made for another window (all flags 1, garbage records), a keyframe without a cache and
    a keyframe whose cache holds fewer keypoints than it has, in one launch"""
    failed = []
    seqs1, seqs3 = KC.ignored_caches(win, 1), KC.ignored_caches(win, 3)
    L = Launch(H, seqs1, "strided", "off1", seed=win)
    before = L.mem.cpu().numpy()
    check_launch(failed, "call 1", L, expected(seqs1, ("ignored", win, 1)), 1)
    check_launch(failed, "call 2", L, expected(seqs1, ("ignored", win, 1)), 0)
    L.set_frame(0, seqs3[0], "strided")
    check_launch(failed, "call 3", L, expected(seqs3, ("ignored", win, 3)), 1)
    after = L.mem.cpu().numpy()
    assert np.array_equal(L.records(before, 0, 0), L.records(after, 0, 0)), "the cache of another window was written"
    assert (L.flags(after, 0, 0) == 1).all()
    assert np.array_equal(L.outside_blocks(before), L.outside_blocks(after)), "written past tmpl_cap records"
    assert np.array_equal(L.flags(after, 0, 2), KC.expected_flags(seqs1[0])[2])
    _report(failed, 3)


# ------------------------------------------------------------------ several keyframes
@pytest.mark.parametrize("win", [31, 35])
def test_several_keyframes(H, win):
    """points of three keyframes (3, 2 and 1 levels against the current frame's 3) interleaved in one launch"""
    failed = []
    seqs1, seqs3 = KC.several_keyframes(win, 1), KC.several_keyframes(win, 3)
    L = Launch(H, seqs1, "off3", "strided", seed=win)
    before = L.mem.cpu().numpy()
    check_launch(failed, "call 1", L, expected(seqs1, ("several", win, 1)), 0)
    after = L.mem.cpu().numpy()
    for k, want in enumerate(KC.expected_flags(seqs1[0])):
        assert np.array_equal(L.flags(after, 0, k), want), f"flags of keyframe {k}"
        assert want[:, len(seqs1[0]["kfs"][k]["levels"]):].sum() == 0 and want.sum() > 0
    assert np.array_equal(L.outside_blocks(before), L.outside_blocks(after))
    check_launch(failed, "call 2", L, expected(seqs1, ("several", win, 1)), 1)
    L.set_frame(0, seqs3[0], "off3")
    check_launch(failed, "call 3", L, expected(seqs3, ("several", win, 3)), 0)
    assert np.array_equal(after, L.mem.cpu().numpy()), "a hit wrote to the cache"
    _report(failed, 3)


@pytest.mark.parametrize("name", ["noise_roll1-w31", "island-w35"])
def test_kf_id_null_equals_all_zero(H, name):
    c = KC.case(name)
    seqs = KC.single(c, 1)
    zero = [dict(seqs[0], kf_id=np.zeros(seqs[0]["n"], np.int32))]
    failed = []
    mems = []
    for s in (seqs, zero):
        L = Launch(H, s, seed=3)
        check_launch(failed, f"{name} kf_id {'null' if s[0]['kf_id'] is None else 'zeros'}", L, expected(seqs, (name, 1)), 1)
        mems.append(L.mem.cpu().numpy())
    assert np.array_equal(mems[0], mems[1])
    _report(failed, 2)


# ------------------------------------------------------------------ batch
@pytest.mark.parametrize("win", [31, 35])
def test_batch_of_five(H, win):
    """five sequences (0, 1, 63, 65 and n_bound points, images of three sizes) in one launch: the oracle's answers,
    and per sequence the outputs AND the cache bytes of a lone launch of that sequence"""
    failed = []
    per_call = {call: KC.batch_of_five(win, call) for call in (1, 3)}
    L = Launch(H, per_call[1], "off1", "dense", n_bound=KC.N_BOUND, seed=win)
    lone = [Launch(H, [s], "off1", "dense", n_bound=KC.N_BOUND, seed=100 + b) for b, s in enumerate(per_call[1])]
    before = L.mem.cpu().numpy()
    for step, call, mats in (("call 1", 1, 1), ("call 2", 1, 0), ("call 3", 3, 1)):
        if call == 3:
            for b, s in enumerate(per_call[3]):
                L.set_frame(b, s, "off1")
                lone[b].set_frame(0, s, "off1")
        exp = expected(per_call[call], ("batch", win, call))
        got = L.run(mats)
        for b, (g, e) in enumerate(zip(got, exp)):
            msg = differs(g, e, per_call[call][b]["n"])
            if msg:
                failed.append((f"{step} sequence {b}", msg))
            alone = lone[b].run(mats)[0]
            if any(not np.array_equal(g[k].view(np.uint8), alone[k].view(np.uint8)) for k in g):
                failed.append((f"{step} sequence {b}", "differs from the lone launch"))
        after = L.mem.cpu().numpy()
        assert np.array_equal(L.outside_blocks(before), L.outside_blocks(after)), step
        for b, s in enumerate(per_call[1]):
            assert np.array_equal(L.flags(after, b, 0), KC.expected_flags(s)[0]), (step, b)
            alone = lone[b].mem.cpu().numpy()
            stored = L.flags(after, b, 0).astype(bool)
            # stored records: header and, where trackable, body equal the lone launch's; the others keep their bytes
            ra, rl = L.records(after, b, 0), lone[b].records(alone, 0, 0)
            hdr = slice(L.hdr_off, L.hdr_off + L.hdr_bytes)
            assert np.array_equal(ra[stored][:, hdr], rl[stored][:, hdr]), (step, b)
            track = stored & (np.ascontiguousarray(ra[..., L.hdr_off:L.hdr_off + 4]).view(np.int32)[..., 0] == KC.KLT_TRACK)
            assert np.array_equal(ra[track][:, :L.hdr_off], rl[track][:, :L.hdr_off]), (step, b)
            assert np.array_equal(ra[~stored], L.records(before, b, 0)[~stored]), (step, b)
    _report(failed, 15)


# ------------------------------------------------------------------ what the entry refuses
def test_entry_refuses_what_would_leave_the_callers_arrays(H):
    """the counts and both index arrays are checked before the launch, and a cache that the launch would use must hold
    tmpl_cap records: a refused call launches nothing and writes nothing"""
    c = KC.case("small20x20-w31")
    seqs = KC.single(c, 1)
    L = Launch(H, seqs)
    before = L.mem.clone()
    d = L.dev[0]
    good = dict(d)

    def refused(match, **change):
        d.update(change)
        with pytest.raises(hip_lib.SvoError, match=match):
            L.run(0)
        d.update(good)

    idx = good["kp_index"].clone()
    idx[3] = len(c["table"])
    refused("index", kp_index=idx)
    idx = good["kp_index"].clone()
    idx[0] = -1
    refused("index", kp_index=idx)
    refused("keyframe 1", kf_id=torch.ones(L.n_bound, dtype=torch.int32, device="cuda"))
    refused("outside 0..n_bound", n=dev(np.array([L.n_bound + 1], np.int32)))
    refused("outside 0..n_bound", n=dev(np.array([-1], np.int32)))
    kf = dict(good["kfs"][0], tmpl_cap=good["kfs"][0]["tmpl_cap"] + 1)
    refused("the cache needs", kfs=[kf])
    kf = dict(good["kfs"][0], valid=None)
    refused("the cache needs", kfs=[kf])
    with pytest.raises(hip_lib.SvoError, match="window"):
        H.klt_track_batch(L.dev, L.n_bound, 37, 0)
    assert torch.equal(before, L.mem)
    failed = []
    check_launch(failed, c["name"], L, expected(seqs, (c["name"], 1)), 0)
    _report(failed, 1)
