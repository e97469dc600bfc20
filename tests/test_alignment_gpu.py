"""sia_prep_kernel and the nine sia_gn_kernel<WAVES, MODE> shapes on the crafted scenes and keypoints of
tests/alignment_cases.py: against the CPU oracle and against the plain numpy statement (which
tests/test_alignment_cpu.py ties to each other), bit for bit, NaN equal to NaN; through svo_sparse_align (one sequence
per launch: every named case, composites on both sides of every shape switch) and through svo_sparse_align_batch
(32 to 40 sequences of unequal counts per launch, the workspaces pre-filled with a pattern); the fast solver within
the project's own bounds; level images that are views into wider or unaligned buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import alignment_cases as AC
import oracle_py as O
from stereo_svo_slam_amd import hip_lib
from test_alignment_cpu import TRACE_INTS, levels_of, ocam, oracle_align
from test_geometry_cpu import same

pytestmark = pytest.mark.gpu
F = np.float32
GUARD_F, GUARD_B = F(-12345.5), 0xA5
PAD = 19                                    # poisoned keypoint slots behind the n that a launch is told
FILLS = (0x7FC00000, 0x42C80000)            # workspace patterns: NaN and 100.0


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=AC.REC_CAP)
    yield h
    h.set_exact_pinv(True)
    h.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hcam(cam):
    return hip_lib.CameraSettings.from_dict(cam)


@functools.lru_cache(maxsize=None)
def pyramids(scene, prev_view="contiguous", cur_view="contiguous"):
    sc = AC.scenes()[scene]
    return [view(a, prev_view) for a in sc["prev"]], [view(a, cur_view) for a in sc["cur"]]


def view(a, kind):
    """a level image on the device: contiguous; `wide`: the left columns of a wider buffer whose row pitch is a
    multiple of 4 (dword rows with a 1-3 byte tail); `odd`: at an odd byte offset with an odd pitch (byte path)"""
    h, w = a.shape
    if kind == "contiguous":
        return dev(a)
    pitch = ((w + 3) & ~3) + 8 if kind == "wide" else (w + 5) | 1
    off = 0 if kind == "wide" else 1
    buf = torch.full((off + h * pitch + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    v = buf[off:off + h * pitch].view(h, pitch)[:, :w]
    v.copy_(dev(a))
    assert v.data_ptr() % 4 == off and v.stride(0) == pitch
    return v


def poisoned(c, n, slots):
    """the first n keypoints of a set in arrays of `slots` entries; the rest holds 1e30, inf and random flags"""
    rng = np.random.RandomState(n + slots)
    k2, k3 = np.full((slots, 2), 1e30, F), np.full((slots, 3), 1e30, F)
    k2[n:, 1], k3[n:, 2] = np.inf, -np.inf
    fl = rng.randint(0, 8, slots).astype(np.uint32)
    k2[:n], k3[:n], fl[:n] = c["kps2d"][:n], c["kps3d"][:n], c["flags"][:n]
    return k2, k3, fl


def run_lone(H, c, n=None, dbg_level=-1, exact=True, prev_view="contiguous", cur_view="contiguous"):
    """svo_sparse_align on the first n keypoints of a set, outputs pre-filled with guards: dict(pose, cost, trace,
    dbg); asserts that nothing beyond the outputs was written"""
    sc = AC.scenes()[c["scene"]]
    cam = sc["cam"]
    n = len(c["kps2d"]) if n is None else n
    k2, k3, fl = (dev(a) for a in poisoned(c, n, n + PAD))
    prev, cur = pyramids(c["scene"], prev_view, cur_view)
    pose = torch.full((8,), float(GUARD_F), dtype=torch.float32, device="cuda")
    cost = torch.full((2,), float(GUARD_F), dtype=torch.float32, device="cuda")
    trace = torch.full((8 * hip_lib.GN_TRACE_DTYPE.itemsize,), GUARD_B, dtype=torch.uint8, device="cuda")
    dbg = torch.full((52,), float(GUARD_F), dtype=torch.float32, device="cuda")
    H.set_exact_pinv(exact)
    try:
        hip_lib._check(hip_lib.lib().svo_sparse_align(
            H._h, hip_lib._imgs(prev, 8), hip_lib._imgs(cur, 8), hip_lib._ptr(k2), hip_lib._ptr(k3), hip_lib._ptr(fl), n,
            C.byref(hcam(cam)), hip_lib._ptr(dev(c["guess"])), hip_lib._ptr(pose), hip_lib._ptr(cost), hip_lib._ptr(trace),
            hip_lib._ptr(dbg) if dbg_level >= 0 else None, dbg_level))
        H.synchronize()
    finally:
        H.set_exact_pinv(True)
    pose, cost, dbg = pose.cpu().numpy(), cost.cpu().numpy(), dbg.cpu().numpy()
    raw = trace.cpu().numpy().reshape(8, -1)
    used = list(levels_of(cam))
    assert np.all(pose[6:] == GUARD_F) and cost[1] == GUARD_F and np.all(dbg[48:] == GUARD_F), c["name"]
    assert np.all(raw[[l for l in range(8) if l not in used]] == GUARD_B), f"{c['name']}: trace of a level not run"
    if dbg_level < 0:
        assert np.all(dbg == GUARD_F)
    return dict(pose=pose[:6], cost=cost[0], trace=raw.reshape(-1).view(hip_lib.GN_TRACE_DTYPE), dbg=dbg[:48])


def check_exact(got, ref, cam, what):
    """pose, cost and every used level's trace against an oracle_align or align_ref result"""
    same(got["pose"], np.asarray(ref["pose"], F), f"{what}: pose")
    same(got["cost"], F(ref["cost"]), f"{what}: cost")
    for level in levels_of(cam):
        tr, r = got["trace"][level], ref["trace"][level]
        assert int(tr["level"]) == level
        assert tuple(int(tr[k]) for k in TRACE_INTS) == tuple(int(r[k]) for k in TRACE_INTS), (what, level, tr, r)
        same(tr["initial_cost"], F(r["initial_cost"]), f"{what} level {level}: initial cost")
        same(tr["final_cost"], F(r["final_cost"] if "final_cost" in r else r["cost"]), f"{what} level {level}: final cost")
        same(tr["pose"], np.asarray(r["pose"], F), f"{what} level {level}: pose of the trace")


def start_pose(c, ref, cam, level):
    """where the level starts: the guess, or the pose the level above ended at"""
    return c["guess"] if level == cam["max_pyramid_levels"] - 1 else np.asarray(ref["trace"][level + 1]["pose"], F)


def oracle_gradient(c, n, cam, level, pose):
    sc = AC.scenes()[c["scene"]]
    return O.sia_gradient(sc["prev"][level], sc["cur"][level], level, c["kps2d"][:n], c["kps3d"][:n], c["flags"][:n],
                          ocam(cam), pose)


def check_dbg(dbg, ref, what):
    for got, want, name in zip((dbg[:36].reshape(6, 6), dbg[36:42], dbg[42:48]), ref, ("H", "b", "step")):
        same(got, want, f"{what}: {name} of the first gradient")


def check_fast(dbg, ref, what):
    """the bounds of test_sia_first_gradient_matches (tests/test_parity_gpu.py)"""
    Hg, bg, sg = dbg[:36].reshape(6, 6), dbg[36:42], dbg[42:48]
    Href, bref, sref = ref
    scale = np.sqrt(np.outer(np.diag(Href), np.diag(Href))) + 1e-20
    assert np.max(np.abs(Hg - Href) / scale) < 2e-5, what
    assert np.max(np.abs(bg - bref)) < 2e-5 * np.max(np.abs(bref)) + 1e-3, what
    assert np.max(np.abs(sg - sref)) < 5e-3 * np.max(np.abs(sref)) + 1e-6, what


# ------------------------------------------------------------------ a. every case, one sequence per launch
def test_every_case_through_the_stage_entry(H):
    stated = AC.results()
    launches = 0
    for c in AC.cases():
        cam = AC.scenes()[c["scene"]]["cam"]
        ref, st = oracle_align(c), stated[c["name"]]
        for level in levels_of(cam):
            got = run_lone(H, c, dbg_level=level)
            check_exact(got, ref, cam, f"{c['name']} against the oracle")
            check_exact(got, st, cam, f"{c['name']} against the statement")
            check_dbg(got["dbg"], oracle_gradient(c, len(c["kps2d"]), cam, level, start_pose(c, ref, cam, level)),
                      f"{c['name']} level {level}")
            first = st["trace"][level]["first"]
            check_dbg(got["dbg"], (first["H"], first["b"], first["step"]), f"{c['name']} level {level}, statement")
            launches += 1
    print(f"{len(AC.cases())} cases, {launches} launches compared with oracle and statement")
    assert launches >= 3 * 40


# ------------------------------------------------------------------ b. the fast solver
def test_fast_solver_on_every_case(H):
    stated = AC.results()
    held = {c["name"] for c in AC.fast_gradient_cases()}
    smooth = {c["name"] for c in AC.fast_pose_cases()}
    checked_gradients = checked_poses = 0
    for c in AC.cases():
        cam = AC.scenes()[c["scene"]]["cam"]
        ref = oracle_align(c)
        top = cam["max_pyramid_levels"] - 1
        got = run_lone(H, c, dbg_level=top, exact=False)
        # the cost is summed in the reference's order in both modes
        same(got["trace"][top]["initial_cost"], F(ref["trace"][top]["initial_cost"]), f"{c['name']}: first cost")
        if c["name"] in held:
            check_fast(got["dbg"], oracle_gradient(c, len(c["kps2d"]), cam, top, c["guess"]), c["name"])
            checked_gradients += 1
        if c["name"] in smooth:
            assert np.max(np.abs(got["pose"] - ref["pose"])) < 1e-4, (c["name"], got["pose"], ref["pose"])
            checked_poses += 1
    print(f"fast solver: {len(AC.cases())} first costs, {checked_gradients} gradients, {checked_poses} poses checked")
    assert checked_poses >= 10 and checked_gradients >= 20


# ------------------------------------------------------------------ c. lone shapes
def test_lone_shapes_on_both_sides_of_every_switch(H):
    for scene, n in AC.lone_plan():
        c = AC.composite(scene, n)
        cam = AC.scenes()[scene]["cam"]
        check_exact(run_lone(H, c), oracle_align(c), cam, f"{c['name']} {AC.host_pick(scene, 1, n)}")
    print("lone launches:", [(scene, n, AC.host_pick(scene, 1, n)[:2]) for scene, n in AC.lone_plan()])


def test_a_small_set_after_a_large_one(H):
    """the handle's workspaces hold the rows of the large set behind the small one's"""
    _, m2 = AC.mode_switches()
    for big, small in ((AC.composite("smooth", m2), AC.case("smooth/flag_holes")),
                       (AC.composite("smooth", 300), AC.case("smooth/one_keypoint")),
                       (AC.composite("large", 129), AC.composite("large", 33)),
                       (AC.composite("smooth", 256), AC.composite("smooth", 3))):
        for c in (big, small):
            check_exact(run_lone(H, c), oracle_align(c), AC.scenes()[c["scene"]]["cam"], c["name"])


# ------------------------------------------------------------------ d. batches
@functools.lru_cache(maxsize=None)
def cached_oracle(name, n):
    c = AC.case(name) if "composite" not in name else AC.composite(name.split("/")[0], int(name.split("composite")[1]))
    return oracle_align(c, n)


MATS_FILL = 0x5A


def check_mats(got, what):
    """the block of rotation matrices the alignment kernel leaves for the tracker's KLT launch to project with
    (SiaArgs::mats_out) is that of the pose it returns, byte for byte: Rd = cv::Rodrigues(r) in double, R = Rd
    rounded to float, Ri = cv::Rodrigues(-r) rounded to float, t the translation. Padding is whatever the layout
    entry leaves out."""
    L = hip_lib.pose_mats_layout()
    pose = np.asarray(got["pose"], F)
    want = dict(Rd=O.rodrigues(pose[3:6]).reshape(9), R=O.rodrigues(pose[3:6]).astype(F).reshape(9),
                Ri=O.rodrigues(-pose[3:6]).astype(F).reshape(9), t=pose[:3])
    covered = 0
    for name in ("Rd", "R", "Ri", "t"):
        off, dtype, count = L[name]
        w = np.ascontiguousarray(want[name], dtype)
        assert w.size == count
        block = got["mats"][off:off + w.nbytes]
        assert block.tobytes() == w.tobytes(), f"{what}: {name} of mats_out: {block.view(dtype)} against {w}"
        covered += w.nbytes
    assert covered <= L["bytes"] < covered + 8 and len(got["mats"]) == L["bytes"]


def run_batch(H, plan, n_bound, ws_fill, dbg_level=-1, exact=True, views=None):
    """svo_sparse_align_batch on a plan [(set, n)]: per sequence dict(pose, cost, trace, dbg, mats), and the shape"""
    batch, stride = len(plan), n_bound + PAD
    mats_bytes = hip_lib.pose_mats_layout()["bytes"]
    mats = torch.full((batch + 1, mats_bytes), MATS_FILL, dtype=torch.uint8, device="cuda")
    cam = AC.scenes()[plan[0][0]["scene"]]["cam"]
    arrays = [poisoned(c, n, stride) for c, n in plan]
    k2, k3, fl = (dev(np.stack([a[k] for a in arrays])) for k in range(3))
    pyr = [pyramids(c["scene"], *(views[b] if views else ())) for b, (c, _) in enumerate(plan)]
    guard = lambda *shape: torch.full(shape, float(GUARD_F), dtype=torch.float32, device="cuda")
    pose, cost, dbg = guard(batch + 1, 6), guard(batch + 1), guard(batch + 1, 48)
    trace = torch.full((batch + 1, 8 * hip_lib.GN_TRACE_DTYPE.itemsize), GUARD_B, dtype=torch.uint8, device="cuda")
    H.set_exact_pinv(exact)
    try:
        *_, shape = H.sparse_align_batch(
            dev(np.array([n for _, n in plan], np.int32)), n_bound, k2, k3, fl, [p[0] for p in pyr], [p[1] for p in pyr],
            hcam(cam), dev(np.stack([c["guess"] for c, _ in plan])), dbg_level, ws_fill,
            outputs=(pose[:batch], cost[:batch], trace[:batch], dbg[:batch] if dbg_level >= 0 else None), mats_out=mats)
    finally:
        H.set_exact_pinv(True)
    pose, cost, dbg, trace = pose.cpu().numpy(), cost.cpu().numpy(), dbg.cpu().numpy(), trace.cpu().numpy()
    mats = mats.cpu().numpy()
    assert np.all(mats[batch] == MATS_FILL), "mats_out behind the last sequence"
    assert np.all(pose[batch] == GUARD_F) and cost[batch] == GUARD_F and np.all(dbg[batch] == GUARD_F)
    assert np.all(trace[batch] == GUARD_B)
    used = list(levels_of(cam))
    assert np.all(trace.reshape(batch + 1, 8, -1)[:, [l for l in range(8) if l not in used]] == GUARD_B)
    if dbg_level < 0:
        assert np.all(dbg == GUARD_F)
    return [dict(pose=pose[b], cost=cost[b], trace=trace[b].view(hip_lib.GN_TRACE_DTYPE), dbg=dbg[b], mats=mats[b])
            for b in range(batch)], shape


def test_mats_out_of_every_case_alone(H):
    """a batch of one takes the lone shapes: every named case (those without a keypoint, without an active keypoint
    and without a valid patch included), the composites on both sides of every lone shape switch, both solvers"""
    stated = AC.results()
    quiet = set()
    for exact in (True, False):
        for c in AC.cases() + ([AC.composite(scene, n) for scene, n in AC.lone_plan()] if exact else []):
            n = len(c["kps2d"])
            (got,), _ = run_batch(H, [(c, n)], max(n, 1), FILLS[0], exact=exact)
            check_mats(got, f"{c['name']} exact {exact}")
            if exact:
                same(got["pose"], np.asarray(oracle_align(c)["pose"], F), f"{c['name']}: pose of the batch of one")
                if c["name"] in stated:
                    quiet |= stated[c["name"]]["labels"] & {"n_zero", "no_active_keypoint", "rank_deficient", "zero_step"}
    assert {"n_zero", "no_active_keypoint"} <= quiet, quiet


@pytest.mark.parametrize("n_bound", AC.BATCH_BOUNDS)
def test_batched_shapes(H, n_bound):
    plan = AC.batch_plan(n_bound)
    cam = AC.scenes()["smooth"]["cam"]
    top = cam["max_pyramid_levels"] - 1
    runs = []
    for fill in FILLS:
        got, shape = run_batch(H, plan, n_bound, fill, dbg_level=top)
        assert shape == AC.host_pick("smooth", len(plan), n_bound)
        runs.append(got)
    for b, (c, n) in enumerate(plan):
        what = f"n_bound {n_bound} sequence {b}: {c['name']}[:{n}]"
        ref = cached_oracle(c["name"], n)
        check_exact(runs[0][b], ref, cam, what)
        check_dbg(runs[0][b]["dbg"], oracle_gradient(c, n, cam, top, c["guess"]), what)
        for run in runs:
            check_mats(run[b], what)
        for key in ("pose", "cost", "dbg"):
            same(runs[1][b][key], runs[0][b][key], f"{what}: {key} with the other workspace pattern")
        assert runs[1][b]["trace"].tobytes() == runs[0][b]["trace"].tobytes(), what
    print(f"n_bound {n_bound}: {len(plan)} sequences, shape {shape}, counts {sorted(n for _, n in plan)}")


def test_batched_fast_solver(H):
    n_bound = 193
    plan = AC.batch_plan(n_bound)
    cam = AC.scenes()["smooth"]["cam"]
    top = cam["max_pyramid_levels"] - 1
    held = {c["name"] for c in AC.fast_gradient_cases()}
    smooth = {c["name"] for c in AC.fast_pose_cases()}
    got, _ = run_batch(H, plan, n_bound, FILLS[0], dbg_level=top, exact=False)
    checked = 0
    for b, (c, n) in enumerate(plan):
        ref = cached_oracle(c["name"], n)
        same(got[b]["trace"][top]["initial_cost"], F(ref["trace"][top]["initial_cost"]), f"{c['name']}[:{n}]: first cost")
        check_mats(got[b], f"{c['name']}[:{n}] with the fast solver")
        whole = n == len(c["kps2d"])
        if whole and c["name"] in held:
            check_fast(got[b]["dbg"], oracle_gradient(c, n, cam, top, c["guess"]), c["name"])
            checked += 1
        if whole and c["name"] in smooth:
            assert np.max(np.abs(got[b]["pose"] - ref["pose"])) < 1e-4, (c["name"], got[b]["pose"], ref["pose"])
    assert checked >= 5


# ------------------------------------------------------------------ e. views
VIEW_SETS = ("smooth/ring_x_level0", "smooth/float_edges", "blocks/interior40_seed5")
VIEW_KINDS = [(p, c) for kind in ("wide", "odd") for p, c in ((kind, "contiguous"), ("contiguous", kind), (kind, kind))]


def test_views_lone(H):
    for c in [AC.case(n) for n in VIEW_SETS] + [AC.composite("smooth", 300)]:
        cam = AC.scenes()[c["scene"]]["cam"]
        base = run_lone(H, c, dbg_level=0)
        check_exact(base, oracle_align(c), cam, c["name"])
        for pv, cv in VIEW_KINDS:
            got = run_lone(H, c, dbg_level=0, prev_view=pv, cur_view=cv)
            for key in ("pose", "cost", "dbg"):
                same(got[key], base[key], f"{c['name']} prev {pv} cur {cv}: {key}")
            assert got["trace"].tobytes() == base["trace"].tobytes(), (c["name"], pv, cv)


def test_views_batched(H):
    sets = [(AC.case(n), len(AC.case(n)["kps2d"])) for n in VIEW_SETS] + [(AC.composite("smooth", 128), 128)]
    n_bound = 128
    plan, views = [], []
    for kinds in [("contiguous", "contiguous")] + VIEW_KINDS + [("wide", "odd")]:
        plan += sets
        views += [kinds] * len(sets)
    assert 32 <= len(plan) <= 40
    cam = AC.scenes()["smooth"]["cam"]
    got, _ = run_batch(H, plan, n_bound, FILLS[0], dbg_level=0, views=views)
    for b, (c, n) in enumerate(plan):
        base = got[b % len(sets)]
        if b < len(sets):
            check_exact(base, cached_oracle(c["name"], n), cam, c["name"])
        for key in ("pose", "cost", "dbg"):
            same(got[b][key], base[key], f"{c['name']} prev {views[b][0]} cur {views[b][1]}: {key}")
        assert got[b]["trace"].tobytes() == base["trace"].tobytes(), (c["name"], views[b])
