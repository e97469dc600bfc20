"""compact_kernel, kf_select_merge_kernel, kf_init_kernel and the tracker's form of the ssd_disparity_kernel launch on
the crafted cases of tests/bookkeeping_cases.py, through the four diagnostic entries that fill the argument blocks and
launch the way the tracker's step does (svo_compact_batch, svo_keyframe_merge_batch, svo_keyframe_init_batch,
svo_ssd_disparity_batch), against the numpy statements and against the CPU oracle's accessors (which
tests/test_bookkeeping_cpu.py ties to each other), word for word.

Every sequence of a launch lives in one device buffer laid out by bookkeeping_cases.Arena: each array is followed by
guard words, outputs are pre-filled with patterns, and the whole buffer is compared with the expected one: what a
kernel must write, what it must leave (entries past the count, the other planes, the source set, the guards).

No comparison has a tolerance. A test collects every sequence that differs and names the first word.

Errors that were seeded into scratch builds of the kernels and run once on an MI355X, with the tests of this file
and the tests of test_keyframe_gpu, test_parity_gpu, test_window_gpu, test_tracker_gpu and test_trim_gpu that they
turn red (719 earlier tests ran):
  `per` rounded down in compact_kernel                 6 here, 53 earlier
  one plane (kfP) missing from copy_kp                 6 here, 27 earlier
  the liveness mask taken before the flag test         5 here, none earlier
  `cq <= cj` in the merge rank                         4 here, 210 earlier
  `>=` in the occupancy test                           1 here, none earlier
  `n / 4` as `(n + 3) / 4` in the backup rule          3 here, none earlier
  `q < i` in the colour loop                           5 here, 201 earlier
  the record's flags copied after the clear            4 here, 185 earlier
  `first_ptr` ignored by ssd_disparity_kernel          7 here, none earlier
Judged from the code and not run, because they write outside an array: the scan made inclusive (`pos` runs up to
`per` entries past `total`, past `cap` when everything is kept); `j <= 64` in the mask (`s_live[2]`, a word of LDS
behind the array: the case {5, 69} reports [5, 1, 0] only while that word is not the mask's own); `xi * ncx + yi`
(up to (ncx - 1) * ncx + ncy - 1 >= ncx * ncy whenever ncx > ncy, as on every grid here); the unswapped grid (its
cell count exceeds the swapped one's that `occupied` is sized for, 104 against 102 on the 13 x 6 grid); `kp > n`
(keypoint n is read and disparity[n] written: the cases keep four entries behind n, whose pattern would change,
but the stage entry's arrays of the earlier tests end at n)."""
import numpy as np
import pytest
import torch

import bookkeeping_cases as BC
import window_cases as WC
from stereo_svo_slam_amd import hip_lib, synth
from test_bookkeeping_cpu import oracle_init, oracle_kept, oracle_picked, oracle_select
from test_window_gpu import place, ssd_expected

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=4096)
    yield h
    h.close()


class Buffers:
    """the arenas of a batch in one device tensor: sequence b's words start at base[b]"""

    def __init__(self, arenas, images):
        self.arenas = arenas
        self.base = np.concatenate([[0], np.cumsum([(a.size + 63) // 64 * 64 for a in arenas])]).astype(np.int64)
        host = np.full(int(self.base[-1]) + 64, BC.GUARD, U)
        for b, im in enumerate(images):
            host[self.base[b]:self.base[b] + im.size] = im
        self.before = host
        self.dev = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, b, name, index=0):
        return self.dev.data_ptr() + 4 * (int(self.base[b]) + self.arenas[b].off[name][0] + index)

    def planes(self, b, prefix):
        return {name: self.ptr(b, f"{prefix}.{name}") for name in hip_lib.KPS_PLANES}

    def differs(self, expected, skip=()):
        """[(sequence, message)] for the sequences whose words differ from `expected` (images per sequence); the words
        between the sequences must be unchanged too"""
        got = self.dev.cpu().numpy().view(U)
        out = []
        covered = np.zeros(got.size, bool)
        for b, (a, want) in enumerate(zip(self.arenas, expected)):
            g = got[self.base[b]:self.base[b] + a.size]
            covered[self.base[b]:self.base[b] + a.size] = True
            bad = np.nonzero((g != want) & a.mask(skip))[0]
            if bad.size:
                i = int(bad[0])
                out.append((b, f"{bad.size} words, first {a.where(i)}: {g[i]:#010x} for {want[i]:#010x} (was "
                               f"{self.before[self.base[b] + i]:#010x})"))
        if np.any(got[~covered] != BC.GUARD):
            out.append((-1, "a word between two sequences changed"))
        return out


def _report(failed, names, what):
    assert not failed, f"{what}: {len(failed)} sequences differ:\n" + "\n".join(
        f"  {names[b] if b >= 0 else '-'}: {m}" for b, m in failed[:12])


def hcam(**kw):
    d = dict(synth.CONFIGS["euroc"])
    d.update(kw)
    return hip_lib.CameraSettings.from_dict(d)


# ------------------------------------------------------------------ compaction
def compact_seq(buf, b, c, min_kf=None):
    return dict(src=buf.planes(b, "src"), dst=buf.planes(b, "dst"), mode=c["mode"], width=c["width"], height=c["height"],
                start=c["start"], enable=None if c["enable"] is None else buf.ptr(b, "enable"),
                zero=buf.ptr(b, "zero") if c["zero_count"] else None, zero_count=c["zero_count"],
                zero_res=buf.ptr(b, "zero_res") if c["zero_res_count"] else None, zero_res_count=c["zero_res_count"],
                min_kf=buf.ptr(b, "min_kf") if (c["min_kf"] if min_kf is None else min_kf) else None)


def run_compact(H, cases, cap):
    arenas = [BC.compact_arena(c) for c in cases]
    buf = Buffers(arenas, [a.image(BC.compact_initial(c)) for a, c in zip(arenas, cases)])
    threads = H.compact_batch([compact_seq(buf, b, c) for b, c in enumerate(cases)], cap)
    return buf, arenas, threads


@pytest.mark.parametrize("cap", [1024, 1100, 2048])
def test_compact_cases(H, cap):
    cases = [c for c in BC.compact_cases() if c["cap"] == cap]
    buf, arenas, threads = run_compact(H, cases, cap)
    assert threads == BC.compact_threads(cap)
    names = [c["name"] for c in cases]
    stated = [a.image(BC.compact_expect(c)[0]) for a, c in zip(arenas, cases)]
    _report(buf.differs(stated), names, "against the statement")
    oracle = [a.image(BC.compact_expect(c, None if c["start"] or c["enable"] == 0 else oracle_kept(c))[0])
              for a, c in zip(arenas, cases)]
    _report(buf.differs(oracle), names, "against the oracle")


@pytest.mark.parametrize("batch", [1, 5, 40])
def test_compact_batches_against_lone_launches(H, batch):
    cases = [c for c in BC.compact_cases() if c["cap"] == 1100 and "rnd" in c["name"]]
    rng = np.random.RandomState(batch)
    pick = [cases[i] for i in rng.permutation(len(cases))[:batch]]
    assert batch == 1 or len({c["src"]["n"] for c in pick}) > 1
    buf = run_compact(H, pick, 1100)[0]
    together = buf.dev.cpu().numpy().view(U)
    for b, c in enumerate(pick):
        lone, arenas, _ = run_compact(H, [c], 1100)
        got = lone.dev.cpu().numpy().view(U)[:arenas[0].size]
        assert np.array_equal(got, together[buf.base[b]:buf.base[b] + arenas[0].size]), c["name"]
        assert np.array_equal(got, arenas[0].image(BC.compact_expect(c)[0])), c["name"]


def test_compact_refuses_the_mask_in_mode_1(H):
    c = next(c for c in BC.compact_cases() if c["mode"] == 1 and not c["start"])
    arena = BC.compact_arena(c)
    buf = Buffers([arena], [arena.image(BC.compact_initial(c))])
    with pytest.raises(hip_lib.SvoError, match="mode 0 only"):
        H.compact_batch([compact_seq(buf, 0, c, min_kf=True)], c["cap"])
    assert not buf.differs([arena.image(BC.compact_initial(c))])
    bad = dict(c, src=dict(c["src"], n=c["cap"] + 1))
    buf = Buffers([arena], [arena.image(BC.compact_initial(bad))])
    with pytest.raises(hip_lib.SvoError, match="outside 0..cap"):
        H.compact_batch([compact_seq(buf, 0, bad)], c["cap"])


# ------------------------------------------------------------------ select + merge
def merge_seq(buf, b, c):
    return dict(cam=hcam(grid_width=c["grid_width"], grid_height=c["grid_height"]), width=c["width"], height=c["height"],
                det=buf.ptr(b, "det"), n_det=buf.ptr(b, "n_det"), kps=buf.planes(b, "kps"), sel=buf.ptr(b, "sel"),
                sel_level=buf.ptr(b, "sel_level"), sel_cell=buf.ptr(b, "sel_cell"), occupied=buf.ptr(b, "occupied"),
                occupied_count=BC.merge_cells(c), old_count=buf.ptr(b, "old_count"), overflow=buf.ptr(b, "overflow"),
                enable=None if c["enable"] is None else buf.ptr(b, "enable"))


def run_merge(H, cases):
    c0 = cases[0]
    arenas = [BC.merge_arena(c) for c in cases]
    buf = Buffers(arenas, [a.image(BC.merge_initial(c)) for a, c in zip(arenas, cases)])
    threads = H.keyframe_merge_batch([merge_seq(buf, b, c) for b, c in enumerate(cases)], c0["n_levels"], c0["max_cells"], c0["cap"])
    assert threads == BC.merge_threads(c0["max_cells"])
    return buf, arenas


def test_merge_cases(H):
    groups = {}
    for c in BC.merge_cases():
        groups.setdefault((c["n_levels"], c["max_cells"], c["cap"]), []).append(c)
    assert {BC.merge_threads(k[1]) for k in groups} == {256, 1024}
    for cases in groups.values():
        buf, arenas = run_merge(H, cases)
        names = [c["name"] for c in cases]
        _report(buf.differs([a.image(BC.merge_expect(c)[0]) for a, c in zip(arenas, cases)], BC.MERGE_SCRATCH), names,
                "against the statements")
        oracle = []
        for a, c in zip(arenas, cases):
            sel = oracle_select(c)
            oracle.append(a.image(BC.merge_expect(c, sel, oracle_picked(c, sel).tolist())[0]))
        _report(buf.differs(oracle, BC.MERGE_SCRATCH), names, "against the oracle")


@pytest.mark.parametrize("batch", [1, 5, 40])
def test_merge_batches_against_lone_launches(H, batch):
    base = next(c for c in BC.merge_cases() if c["name"] == "grid13x6")
    rng = np.random.RandomState(batch)
    cases = []
    for b in range(batch):                      # the same candidates beside 0 .. 40 old keypoints
        n_old = int(rng.randint(0, base["kps"]["n"] + 1)) if b else base["kps"]["n"]
        cases.append(dict(base, name=f"{base['name']}-old{n_old}", kps=dict(base["kps"], n=n_old)))
    buf, arenas = run_merge(H, cases)
    want = [a.image(BC.merge_expect(c)[0]) for a, c in zip(arenas, cases)]
    _report(buf.differs(want, BC.MERGE_SCRATCH), [c["name"] for c in cases], "the batch")
    together = buf.dev.cpu().numpy().view(U)
    for b, c in enumerate(cases):
        lone, la = run_merge(H, [c])
        m = la[0].mask(BC.MERGE_SCRATCH)
        assert np.array_equal(lone.dev.cpu().numpy().view(U)[:la[0].size][m], together[buf.base[b]:buf.base[b] + la[0].size][m]), c["name"]


# ------------------------------------------------------------------ initialisation
TABLE_FILL = 0x77


TMPL_CAP, TMPL_WIN = 77, 21


def init_seq(buf, b, c, table, tmpl):
    return dict(cam=hcam(**{k: c["cam"][k] for k in ("fx", "fy", "cx", "cy", "baseline")}), first_frame=c["first_frame"],
                new_kf_id=c["new_kf_id"], kf_mask=c["kf_mask"], evict_id=c["evict_id"], kps=buf.planes(b, "kps"),
                record=dict(buf.planes(b, "record"), n=None), old_count=buf.ptr(b, "old_count"),
                disparity=buf.ptr(b, "disparity"), frame_pose=buf.ptr(b, "frame_pose"), kfs=table,
                kfs_bytes=table.numel(), color_lcg=buf.ptr(b, "lcg"), n_out=buf.ptr(b, "n_out"),
                enable=None if c["enable"] is None else buf.ptr(b, "enable"), tmpl=tmpl,
                tmpl_valid=buf.ptr(b, "tmpl_valid") if c["tmpl_valid_bytes"] else None,
                tmpl_valid_bytes=c["tmpl_valid_bytes"], tmpl_cap=TMPL_CAP, tmpl_win=TMPL_WIN)


def check_table(c, table, seq, ref):
    """'' or what is wrong with the keyframe table of a sequence after the launch; seq: what init_seq passed"""
    L = hip_lib.keyframe_record_layout()
    t = table.cpu().numpy().reshape(c["kf_mask"] + 1, L["bytes"])
    if c["enable"] == 0:
        return "" if np.all(t == TABLE_FILL) else "the table of a disabled sequence changed"
    new = c["new_kf_id"] & c["kf_mask"]
    ev = c["evict_id"] & c["kf_mask"] if c["evict_id"] >= 0 else -1
    for r in range(c["kf_mask"] + 1):
        row = t[r].copy()
        if r == new:
            continue
        if r == ev:
            if np.any(row[L["tmpl"]:L["tmpl"] + 8]):
                return f"record {r} keeps its tmpl"
            row[L["tmpl"]:L["tmpl"] + 8] = TABLE_FILL
        if np.any(row != TABLE_FILL):
            return f"record {r} changed"
    row = t[new]
    word = lambda off, typ: int(row[off:off + np.dtype(typ).itemsize].view(typ)[0])
    if word(L["n"], np.int32) != ref["record_n"]:
        return f"n of the record: {word(L['n'], np.int32)} for {ref['record_n']}"
    if not np.array_equal(row[L["pose"]:L["pose"] + 24].view(U), ref["record_pose"].view(U)):
        return f"pose of the record: {row[L['pose']:L['pose'] + 24].view(F)} for {ref['record_pose']}"
    # the pointers and sizes that `kfs[slot] = a.record` copies: the addresses init_seq passed, field by field
    want = {L["planes"][name]: seq["record"][name] for name in hip_lib.KPS_PLANES[:12]}
    assert len(want) == 12
    # (a keyframe that evicts its own ring slot ends without a block: bookkeeping_cases, ring-13-evict-5)
    want[L["tmpl"]] = 0 if ev == new else seq["tmpl"].data_ptr()
    want[L["tmpl_valid"]] = seq["tmpl_valid"] or 0
    for off, addr in want.items():
        if word(off, np.uint64) != addr:
            return f"the pointer at byte {off} of the record: {word(off, np.uint64):#x} for {addr:#x}"
    if (word(L["tmpl_cap"], np.int32), word(L["tmpl_win"], np.int32)) != (TMPL_CAP, TMPL_WIN):
        return "tmpl_cap or tmpl_win of the record"
    return ""


def run_init(H, cases, cap):
    REC_BYTES = hip_lib.keyframe_record_layout()["bytes"]
    arenas = [BC.init_arena(c) for c in cases]
    buf = Buffers(arenas, [a.image(BC.init_initial(c)) for a, c in zip(arenas, cases)])
    tables = [torch.full(((c["kf_mask"] + 1) * REC_BYTES,), TABLE_FILL, dtype=torch.uint8, device="cuda") for c in cases]
    tmpls = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in cases]
    seqs = [init_seq(buf, b, c, tables[b], tmpls[b]) for b, c in enumerate(cases)]
    H.keyframe_init_batch(seqs, cap)
    return buf, arenas, tables, seqs


def check_init(buf, arenas, tables, seqs, cases, what):
    names = [c["name"] for c in cases]
    refs = [BC.init_ref(c)[0] for c in cases]
    _report(buf.differs([a.image(BC.init_expect(c, r)) for a, c, r in zip(arenas, cases, refs)]), names, f"{what}: statement")
    _report(buf.differs([a.image(BC.init_expect(c, oracle_init(c))) for a, c in zip(arenas, cases)]), names, f"{what}: oracle")
    bad = [(b, m) for b, (c, t, sq, r) in enumerate(zip(cases, tables, seqs, refs)) for m in [check_table(c, t, sq, r)] if m]
    _report(bad, names, f"{what}: keyframe table")


def test_init_cases_one_by_one(H):
    for c in BC.init_cases():
        check_init(*run_init(H, [c], c["cap"]), [c], c["name"])


def test_init_cases_in_one_batch(H):
    cases = list(BC.init_cases())
    check_init(*run_init(H, cases, max(c["cap"] for c in cases)), cases, "batch")


@pytest.mark.parametrize("batch", [1, 5, 40])
def test_init_batches_of_unequal_counts(H, batch):
    """the cases n<count>-old<count> (24 of them) in launches of 1, 5 and 40 sequences: each is picked in turn, so a
    batch of 40 holds 16 of them twice"""
    by_count = [c for c in BC.init_cases() if c["name"].startswith("n")]
    cases = [by_count[(7 * batch + 5 * b) % len(by_count)] for b in range(batch)]
    assert batch == 1 or len({c["kps"]["n"] for c in cases}) > 2
    check_init(*run_init(H, cases, max(c["cap"] for c in cases)), cases, f"batch of {batch}")


def test_init_refuses_bad_counts(H):
    c = next(c for c in BC.init_cases() if c["name"] == "n8-old7")
    for bad, msg in ((dict(c, old_count=9), "old_count"), (dict(c, tmpl_valid_bytes=6), "multiple of 4"),
                     (dict(c, kf_mask=5), "power")):
        arena = BC.init_arena(dict(bad, tmpl_valid_bytes=8))
        buf = Buffers([arena], [arena.image(BC.init_initial(dict(bad, tmpl_valid_bytes=8)))])
        table = torch.full((8 * hip_lib.keyframe_record_layout()["bytes"],), TABLE_FILL, dtype=torch.uint8, device="cuda")
        with pytest.raises(hip_lib.SvoError, match=msg):
            H.keyframe_init_batch([init_seq(buf, 0, bad, table, table)], c["cap"])


# ------------------------------------------------------------------ the SSD launch as the tracker makes it
def ssd_arena(cap):
    a = BC.Arena()
    for name, words in (("n", 1), ("kps2d", 2 * cap), ("disparity", cap), ("first_ptr", 1), ("enable", 1)):
        a.add(name, words)
    return a


def ssd_sequence(case, first, first_dev, layout, enable=None, n=None, extra=4, idx=None):
    """one sequence of a launch: the first n keypoints of a case (or its keypoints idx, which may repeat) behind an
    offset, capacity n + extra"""
    name, left, right, kps, win, sx, sy, clamp = case
    if idx is None:
        idx = np.arange(len(kps) if n is None else n)
    n = len(idx)
    cap = n + extra
    k = np.zeros((cap, 2), F)
    k[:n] = kps[idx]
    k[n:] = (-5000.0, 7.0e8)                 # (never read)
    return dict(name=f"{name} n={n} first={first}+{first_dev} {layout} enable={enable}", case=case, n=n, cap=cap, kps=k, idx=idx,
                first=first, first_dev=first_dev, layout=layout, enable=enable, win=win, sx=sx, sy=sy, clamp=clamp)


def run_ssd(H, seqs, win, search_y, n_bound=None):
    arenas = [ssd_arena(s["cap"]) for s in seqs]
    images = [a.image(dict(n=np.array([s["n"]], np.int32), kps2d=BC.bits(s["kps"]), disparity=np.full(s["cap"], BC.DISPARITY_FILL, U),
                           first_ptr=np.array([s["first_dev"]], np.int32),
                           enable=np.array([0xFFFFFFFF if s["enable"] is None else s["enable"]], U))) for a, s in zip(arenas, seqs)]
    buf = Buffers(arenas, images)
    if n_bound is None:
        n_bound = max(max(s["n"] - s["first"] - s["first_dev"], 0) for s in seqs) + 5
    views = {}
    args = []
    for b, s in enumerate(seqs):
        key = (s["case"][0], s["layout"])
        if key not in views:
            views[key] = (place(s["case"][1], s["layout"]), place(s["case"][2], s["layout"]))
        args.append(dict(left=views[key][0], right=views[key][1], n=buf.ptr(b, "n"), kps2d=buf.ptr(b, "kps2d"),
                         disparity=buf.ptr(b, "disparity"), win=s["win"], search_x=s["sx"], search_y=s["sy"],
                         clamp_half=s["clamp"], first=s["first"], cap=s["cap"],
                         first_ptr=buf.ptr(b, "first_ptr") if s["first_dev"] or b % 2 else None,
                         enable=None if s["enable"] is None else buf.ptr(b, "enable")))
    assert H.ssd_disparity_batch(args, n_bound, win, search_y) == BC.ssd_pick_max_win(win, search_y)
    want = []
    for a, s, im in zip(arenas, seqs, images):
        v = im.copy()
        if s["enable"] != 0:
            o, w = a.off["disparity"]
            v[o:o + w] = BC.ssd_launch_ref(np.concatenate([ssd_expected(s["case"])[s["idx"]], np.zeros(s["cap"] - s["n"], F)]),
                                           s["first"] + s["first_dev"], s["n"], n_bound, s["cap"])
        want.append(v)
    return buf, want, n_bound


def ssd_plan(cases):
    """every case behind an offset: the offsets of ssd_offsets, the layouts and the predicate go round"""
    layouts = ["dense", "oddstride", "off3", "strided", "off7"]
    seqs = []
    for i, case in enumerate(cases):
        n = min(len(case[3]), 150)
        offs = BC.ssd_offsets(n)
        first, first_dev = offs[1 + i % (len(offs) - 1)]
        seqs.append(ssd_sequence(case, first, first_dev, layouts[i % 5], enable=(None, 0x100, None, 0, None, None, 1)[i % 7], n=n))
    return seqs


def small_shape(case):
    return BC.ssd_pick_max_win(case[4], case[6]) == 31


def test_ssd_cases_behind_offsets_small_shape(H):
    seqs = ssd_plan([c for c in WC.ssd_cases() if small_shape(c)])
    assert {s["win"] for s in seqs} >= {5, 21, 30, 31} and len({s["case"][1].shape for s in seqs}) > 3
    buf, want, _ = run_ssd(H, seqs, 31, 6)
    _report(buf.differs(want), [s["name"] for s in seqs], "launch chosen by 31 / 6")


def test_ssd_cases_behind_offsets_large_shape(H):
    """every case, the small windows and search ranges included, in a launch chosen by window 35 and search_y 8"""
    seqs = ssd_plan(list(WC.ssd_cases()))
    assert any(s["win"] == 21 for s in seqs) and any(s["sy"] == 6 for s in seqs)
    buf, want, _ = run_ssd(H, seqs, 35, 8)
    _report(buf.differs(want), [s["name"] for s in seqs], "launch chosen by 35 / 8")


@pytest.mark.parametrize("name", ["noise-w31-sy6-c1", "noise-w35-sy8-c0", "thin9x40-w7"])
def test_ssd_every_offset(H, name):
    case = next(c for c in WC.ssd_cases() if c[0] == name)
    n = len(case[3])
    seqs = [ssd_sequence(case, a, b, "off1" if i % 2 else "dense", enable=0 if i == 3 else None) for i, (a, b) in enumerate(BC.ssd_offsets(n))]
    seqs += [ssd_sequence(case, a, b, "dense", n=1) for a, b in ((0, 0), (1, 0), (0, 1), (2, 2))]
    seqs += [ssd_sequence(case, 0, 0, "dense", n=0), ssd_sequence(case, 3, 4, "dense", n=0)]
    for win, sy in ((case[4], case[6]), (35, 8)):
        buf, want, n_bound = run_ssd(H, seqs, win, sy)
        assert n_bound > n
        _report(buf.differs(want), [s["name"] for s in seqs], f"launch chosen by {win} / {sy}")
    buf, want, _ = run_ssd(H, seqs, case[4], case[6], n_bound=7)          # a grid shorter than the keypoints left
    _report(buf.differs(want), [s["name"] for s in seqs], "n_bound 7")


@pytest.mark.parametrize("batch", [1, 5, 40])
def test_ssd_batches_against_lone_launches(H, batch):
    cases = {c[0]: c for c in WC.ssd_cases()}
    pool = [cases[k] for k in ("noise-w31-sy6-c1", "noise-w21-sy4-c0", "blocks-w5-sy1", "real-w31", "tiny20x20-w31")]
    bound = 80
    counts = [0, 1, 63, 65, bound]
    rng = np.random.RandomState(batch)
    seqs = []
    for b in range(batch):
        # the count goes round one step faster than the case, so every case meets every count; a case's keypoints
        # are drawn with repetition, since most cases hold fewer than 63
        case = pool[b % len(pool)]
        n = counts[(b + b // len(pool)) % len(counts)] if batch > 1 else 65
        first, first_dev = (int(rng.randint(0, 3)), int(rng.randint(0, 3))) if n else (1, 2)
        seqs.append(ssd_sequence(case, first, first_dev, ("dense", "oddstride", "off2")[b % 3], idx=rng.randint(0, len(case[3]), n)))
    assert batch == 1 or {s["n"] for s in seqs} == set(counts)
    assert batch < 40 or {(s["case"][0], s["n"]) for s in seqs} == {(c[0], n) for c in pool for n in counts}
    buf, want, n_bound = run_ssd(H, seqs, 31, 6, n_bound=bound)
    _report(buf.differs(want), [s["name"] for s in seqs], "the batch")
    together = buf.dev.cpu().numpy().view(U)
    for b, s in enumerate(seqs):
        lone, lw, _ = run_ssd(H, [s], 31, 6, n_bound=bound)
        size = lone.arenas[0].size
        assert np.array_equal(lone.dev.cpu().numpy().view(U)[:size], together[buf.base[b]:buf.base[b] + size]), s["name"]


def test_ssd_refuses_a_window_beyond_the_launch(H):
    case = next(c for c in WC.ssd_cases() if c[0] == "noise-w35-sy8-c1")
    with pytest.raises(hip_lib.SvoError, match="exceed"):
        run_ssd(H, [ssd_sequence(case, 0, 0, "dense")], 31, 6)
