"""The CPU oracle's sparse image alignment against the plain numpy statements of tests/alignment_cases.py, bit for
bit (NaN equal to NaN), on every case that tests/test_alignment_gpu.py runs on the GPU; the case list reaches what
it is there for, asserted from the statements' own labels; the float32 statement stays close to its float64 twin;
and the launch plans of the GPU test reach every kernel shape and every keypoint count they are there for (a host
decision: svo_pick_launch_shapes needs no GPU).

`beyond_int_range`: where the statement says "outside" because floor() of a coordinate is not finite or not an int32,
the oracle's (int)floor(x) is undefined C. On x86-64 the conversion instruction returns INT_MIN for every such
value, the window test `ip >= 0` fails, and the oracle says "outside" as well: the comparisons below hold on those
cases too, and it is the statement's rule that the kernels are held to."""
import numpy as np
import pytest

import alignment_cases as AC
import oracle_py as O
from test_geometry_cpu import same

F, D = np.float32, np.float64
TRACE_INTS = ("n_gradient", "n_cost", "n_accepted", "exit_small")


def ocam(cam):
    return O.make_camera(**{k: v for k, v in cam.items() if k not in ("width", "height")})


def ocam_level(cam, level):
    return ocam(AC.level_cam(cam, level))


@pytest.fixture(scope="module")
def stated():
    return AC.results()


def levels_of(cam):
    return range(cam["max_pyramid_levels"] - 1, cam["min_pyramid_level_pose_estimation"] - 1, -1)


def oracle_align(c, n=None):
    """the first n keypoints of a case (or composite) through the oracle"""
    sc = AC.scenes()[c["scene"]]
    n = len(c["kps2d"]) if n is None else n
    pose, cost, tr = O.sparse_align(sc["prev"], sc["cur"], c["kps2d"][:n], c["kps3d"][:n], c["flags"][:n], ocam(sc["cam"]),
                                    c["guess"])
    return dict(pose=pose, cost=F(cost), trace=tr)


# ------------------------------------------------------------------ oracle against statement
def test_cost_oracle_equals_the_statement(stated):
    """O.total_intensity_diff at the start pose of every level"""
    for c in AC.cases():
        sc = AC.scenes()[c["scene"]]
        act = (c["flags"] & AC.IGNORE_TEMPORARY) == 0
        for level in levels_of(sc["cam"]):
            t = stated[c["name"]]["trace"][level]
            lk = AC.level_keypoints(c["kps2d"][act], level)
            proj = O.project_keypoints(t["guess"], c["kps3d"][act], ocam_level(sc["cam"], level))
            got = O.total_intensity_diff(sc["prev"][level], sc["cur"][level], lk, proj) if act.any() else 0.0
            same(F(got), t["initial_cost"], f"{c['name']} level {level}: cost at the level's start")


def test_gradient_oracle_equals_the_statement(stated):
    """O.sia_gradient at the start pose of every level: H, b and the step"""
    for c in AC.cases():
        sc = AC.scenes()[c["scene"]]
        for level in levels_of(sc["cam"]):
            t = stated[c["name"]]["trace"][level]
            H, b, step = O.sia_gradient(sc["prev"][level], sc["cur"][level], level, c["kps2d"], c["kps3d"], c["flags"],
                                        ocam(sc["cam"]), t["guess"])
            same(H, t["first"]["H"], f"{c['name']} level {level}: H")
            same(b, t["first"]["b"], f"{c['name']} level {level}: b")
            same(step, t["first"]["step"], f"{c['name']} level {level}: step")


def test_alignment_oracle_equals_the_statement(stated):
    for c in AC.cases():
        sc = AC.scenes()[c["scene"]]
        ref, st = oracle_align(c), stated[c["name"]]
        same(ref["pose"], st["pose"], f"{c['name']}: pose")
        same(ref["cost"], st["cost"], f"{c['name']}: cost")
        for level in levels_of(sc["cam"]):
            tr, t = ref["trace"][level], st["trace"][level]
            assert tuple(tr[k] for k in TRACE_INTS) == tuple(t[k] for k in TRACE_INTS), (c["name"], level, tr, t)
            same(F(tr["initial_cost"]), t["initial_cost"], f"{c['name']} level {level}: initial cost")
            same(F(tr["final_cost"]), t["cost"], f"{c['name']} level {level}: final cost")
            same(np.asarray(tr["pose"], F), t["pose"], f"{c['name']} level {level}: pose of the trace")


# ------------------------------------------------------------------ what the case list reaches
def test_every_label_is_reached(stated):
    seen = set()
    for r in stated.values():
        seen |= r["labels"]
    assert len(AC.ALLOWED_MISSING) <= 2
    missing = set(AC.LABELS) - seen - set(AC.ALLOWED_MISSING)
    assert not missing, sorted(missing)


def test_enough_cases_for_the_fast_solver():
    assert len(AC.fast_pose_cases()) >= 10


def test_float_statement_is_close_to_its_twin():
    cases = AC.twin_cases()
    assert len(cases) >= 20
    worst_h = worst_b = 0.0
    for c in cases:
        h, b = AC.twin_deviation(c)
        print(f"{c['name']}: H {h:.3g} b {b:.3g}")
        worst_h, worst_b = max(worst_h, h), max(worst_b, b)
    print(f"largest deviation: H {worst_h:.3g} (bound {AC.TWIN_BOUND_H:.3g}), b {worst_b:.3g} (bound {AC.TWIN_BOUND_B:.3g})")
    assert worst_h < AC.TWIN_BOUND_H and worst_b < AC.TWIN_BOUND_B


BORDER = {"partial_patch", "in_cost_not_in_H", "in_H_not_in_cost", "gradient_zero_residual_taken"}


def test_border_patches_reach_the_twin_and_the_fast_solver():
    """both lists hold sets whose coarsest level has partial patches, pixels in H and not in the cost and the other
    way round; the fast solver's list also holds every quarter-pixel ring, where coordinates sit on the limits"""
    for cases, least in ((AC.twin_cases(), 4), (AC.fast_gradient_cases(), 15)):
        with_border = [c for c in cases if BORDER <= AC.border_labels(c)]
        assert len(with_border) >= least, [c["name"] for c in with_border]
    fast = {c["name"] for c in AC.fast_gradient_cases()}
    rings = [c["name"] for c in AC.cases() if "ring" in c["name"] or c["name"] in ("smooth/corners", "smooth/float_edges")]
    missing = [n for n in rings if n not in fast and "constant" not in n]
    assert not missing, missing
    assert any("gradient_taken_residual_zero" in AC.border_labels(c) for c in AC.fast_gradient_cases())


# ------------------------------------------------------------------ the launch plans (host only)
ALL_SHAPES = {(w, m) for w in (1, 2, 4) for m in (0, 1, 2)}


def test_plans_reach_every_shape_the_host_can_choose():
    """Every (waves, mode) that sia_pick_shape chooses for any keypoint bound on these scenes, lone or batched, is
    run by a planned launch. <4, 1> is chosen for the 100 x 76 scenes between the two mode switches; <1, 1> and
    <2, 1> need a level image that fills LDS with few keypoints: scene `large`."""
    possible = set()
    for scene in ("smooth", "mult4", "large"):
        for batch in (1, 32, 40):
            for n in list(range(0, 520)) + list(range(520, AC.REC_CAP + 1, 37)) + [AC.REC_CAP]:
                shape = AC.host_pick(scene, batch, n)
                if shape is not None:
                    possible.add(shape[:2])
    planned = {AC.host_pick(scene, 1, n)[:2] for scene, n in AC.lone_plan()}
    planned |= {AC.host_pick("smooth", len(AC.batch_plan(nb)), nb)[:2] for nb in AC.BATCH_BOUNDS}
    never = ALL_SHAPES - possible
    assert not never, f"no bound makes the host choose {sorted(never)}"
    assert planned == possible, (sorted(possible - planned), sorted(planned))
    m1, m2 = AC.mode_switches()
    assert AC.host_pick("smooth", 1, m1 - 1)[1] == 0 and AC.host_pick("smooth", 1, m1)[1] == 1
    assert AC.host_pick("smooth", 1, m2 - 1)[1] == 1 and AC.host_pick("smooth", 1, m2) [:2] == (4, 2)
    # the fast solver has no staging area: its switches lie elsewhere, the plans' shapes must fit there too
    for scene, n in AC.lone_plan():
        assert AC.host_pick(scene, 1, n, exact=False) is not None


@pytest.mark.parametrize("n_bound", AC.BATCH_BOUNDS)
def test_batch_plans_hold_the_counts(n_bound):
    plan = AC.batch_plan(n_bound)
    batch = len(plan)
    assert 32 <= batch <= 40
    counts = [n for _, n in plan]
    for n in (0, 1, 31, 32, 33, 63, 64, 65, n_bound - 1, n_bound):
        assert n > n_bound or n in counts, n
    waves, mode, cap = AC.host_pick("smooth", batch, n_bound)
    assert mode == 2 and waves == (1 if n_bound <= 192 else 2 if n_bound <= 384 else 4)
    assert cap >= n_bound and cap % (64 * waves) == 0
    if n_bound > 64:                                         # a sequence with keypoints, a whole pass or more below the cap
        assert min(n for n in counts if n > 0) + 64 <= cap and sum(0 < n <= cap - 64 for n in counts) >= 3
    chunk = 32 if waves == 1 else 64                         # keypoints whose rows are staged at a time
    assert len({-(-n // chunk) for n in counts}) >= min(3, -(-n_bound // chunk) + 1)     # different chunk counts
    assert all(c["scene"] in AC.MAIN_SCENES and len(c["kps2d"]) >= n for c, n in plan)
    assert len({c["scene"] for c, _ in plan}) >= 4
    assert sum("composite" not in c["name"] for c, _ in plan) >= 8


def test_planned_sets_stay_finite():
    """no planned composite or cut drives the reference to a NaN pose (from where it would index memory with NaN):
    the oracle's pose and cost of every planned launch are finite"""
    todo = [(AC.composite(scene, n), n) for scene, n in AC.lone_plan()]
    for nb in AC.BATCH_BOUNDS:
        todo += AC.batch_plan(nb)
    seen = set()
    for c, n in todo:
        if (c["name"], n) in seen:
            continue
        seen.add((c["name"], n))
        r = oracle_align(c, n)
        assert np.all(np.isfinite(r["pose"])) and np.isfinite(r["cost"]), (c["name"], n)
