"""The CPU oracle's reprojection refinement and depth filter against the plain numpy statements of
tests/geometry_cases.py, bit for bit (NaN equal to NaN), on every case that tests/test_geometry_gpu.py runs on the
GPU; the case lists reach what they are there for, asserted from the statements' own labels; and the float32
statements stay close to their float64 twins where no threshold, NaN or rank deficiency is in play, which is what
catches a formula that is float-consistent but wrong."""
import numpy as np
import pytest

import geometry_cases as GC
import oracle_py as O

F, D = np.float32, np.float64


def ocam(cam):
    return O.make_camera(**{k: cam[k] for k in ("baseline", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")})


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if a.size == 0:
        return
    bad = np.nonzero(~GC.same_bits(a, b).reshape(len(a), -1).all(axis=1))[0] if a.ndim else \
        np.nonzero(~np.atleast_1d(GC.same_bits(a, b)))[0]
    assert bad.size == 0, f"{what}: entries {bad[:8]}: {a[bad[:4]] if a.ndim else a} against {b[bad[:4]] if b.ndim else b}"


@pytest.fixture(scope="module")
def reproj():
    return GC.reproj_results()


@pytest.fixture(scope="module")
def filt():
    return GC.filter_results()


# ------------------------------------------------------------------ oracle against statement
def test_projection_statement_equals_the_oracle():
    rng = np.random.RandomState(3)
    pts = np.concatenate([rng.uniform(-3, 3, (60, 3)), [[0, 0, 0], [1, 2, 0], [0.1, 0.2, -3]]]).astype(F)
    for cam in GC.CAMERAS.values():
        for pose in ((0, 0, 0, 0, 0, 0), (0.1, -0.05, 0.2, 0.02, -0.03, 0.01), (1, 2, 0.5, 0.9, -0.4, 1.3)):
            same(O.project_keypoints(pose, pts, ocam(cam)), GC.project_ref(np.asarray(pose, F), pts, cam), "projection")


def test_merge_oracle_equals_the_statement(reproj):
    for c in GC.reproj_cases():
        k2, fl = O.refine_merge(c["kps2d"], c["flags"], c["tracked"], c["err"])
        same(k2, reproj[c["name"]]["kps2d"], f"{c['name']}: merged positions")
        same(fl, reproj[c["name"]]["flags"], f"{c['name']}: flags")


def test_reproj_oracle_equals_the_statement(reproj):
    for c in GC.reproj_cases():
        r = reproj[c["name"]]
        cam = ocam(c["cam"])
        H, e = O.reproj_normal(r["kps2d"], c["kps3d"], r["flags"], cam, c["start"])
        same(H, r["H"], f"{c['name']}: the 36 sums of J^T J at the start pose")
        same(e, r["e"], f"{c['name']}: the 6 sums of J^T diff at the start pose")
        pose, cost, tr = O.reproj_gn(r["kps2d"], c["kps3d"], r["flags"], cam, c["start"])
        gn = r["gn"]
        same(F(tr["initial_cost"]), gn["initial_cost"], f"{c['name']}: initial cost")
        assert (tr["n_gradient"], tr["n_cost"], tr["n_accepted"], tr["exit_small"]) == \
            (gn["n_gradient"], gn["n_cost"], gn["n_accepted"], gn["exit_small"]), (c["name"], tr, gn)
        same(pose, gn["pose"], f"{c['name']}: pose")
        same(F(cost), gn["cost"], f"{c['name']}: final cost")
        same(F(tr["final_cost"]), gn["cost"], f"{c['name']}: final cost of the trace")
        same(np.asarray(tr["pose"], F), gn["pose"], f"{c['name']}: pose of the trace")


def oracle_filter(c, do_outlier_check, do_update):
    """the oracle's stages in the kernel's order, then its write-back and counter"""
    cam = ocam(c["cam"])
    outl, inl, k3, kx, kP = c["outlier"], c["inlier"], c["kps3d"], c["kf_inv_depth"], c["kf_variance"]
    if do_outlier_check:
        outl, inl = O.outlier_check(c["kps2d"], c["disparity"], cam, c["frame_pose"], c["ref3d"], c["kf_pose"], outl, inl)
    if do_update:
        k3, outl, kx, kP = O.update_kps3d(c["kps2d"], k3, c["flags"], cam, c["frame_pose"], c["ref2d"], c["kf_pose"],
                                          outl, kx, kP)
    fl = O.filter_flags(c["flags"], outl, inl)
    k2 = O.project_keypoints(c["frame_pose"], k3, cam)
    return dict(outlier=outl, inlier=inl, kps3d=k3, kf_inv_depth=kx, kf_variance=kP, flags=fl, kps2d=k2,
                inside=O.inside_count(k2, fl, c["width"], c["height"]))


def test_filter_oracle_equals_the_statement(filt):
    for c in GC.filter_cases():
        for sw, ref in filt[c["name"]].items():
            got = oracle_filter(c, *sw)
            for key in ("outlier", "inlier", "kf_inv_depth", "kf_variance", "kps3d", "flags", "kps2d"):
                same(got[key], ref[key], f"{c['name']} {sw}: {key}")
            assert got["inside"] == ref["inside"], (c["name"], sw)


# ------------------------------------------------------------------ the cases reach what they are there for
def test_every_label_is_reached(reproj, filt):
    got = set().union(*[r["labels"] for r in reproj.values()])
    assert set(GC.REPROJ_LABELS) <= got, set(GC.REPROJ_LABELS) - got
    got = set().union(*[r["labels"] for sw in filt.values() for r in sw.values()])
    missing = set(GC.FILTER_LABELS) - got
    assert missing <= set(GC.ALLOWED_MISSING), missing
    assert not missing                                              # (today both allowed misses are reached too)


def test_the_edges_fall_on_the_sides_the_reference_puts_them(reproj, filt):
    r = reproj["offsets81"]                                          # 81 merges, the next float does not
    assert [sorted(l - {"at_threshold"}) for l in r["merge_labels"][:8]] == \
        [["merged"]] * 5 + [["moved_over_9px"]] * 2 + [["moved_over_9px"]]
    assert list(r["flags"][:8] & 1) == [0, 0, 0, 0, 0, 1, 1, 1]
    r = reproj["err_edges"]                                          # 20, next(20), inf, NaN, -inf, prev(20)
    assert list((r["flags"][:6] & 2) >> 1) == [0, 1, 1, 0, 0, 0]
    assert "err_inf" in r["merge_labels"][2] and "occluded" in r["merge_labels"][1]
    kl = reproj["residual3"]["gn"]["kp_labels"]                    # 3.0 takes part, the next float does not
    want = ["took_part", "residual_over_3px_x"] * 2 + ["took_part", "residual_over_3px_y"] * 2
    assert [sorted(l - {"at_threshold"}) for l in kl[:8]] == [[w] for w in want]
    gn = reproj["camera_centre"]["gn"]
    assert (gn["n_gradient"], gn["n_cost"], gn["n_accepted"], gn["exit_small"]) == (1, 51, 0, 0)
    assert np.array_equal(gn["pose"], [c for c in GC.reproj_cases() if c["name"] == "camera_centre"][0]["start"])
    gn = reproj["all_ignored"]["gn"]
    assert (gn["n_cost"], gn["exit_small"], float(gn["cost"])) == (2, 1, 0.0)
    assert "accepted_after_halving" in reproj["start_0.3rad"]["gn"]["labels"]
    lo = filt["disparities"][(1, 1)]["kp_labels"][0]                 # -1, 0, 0.5, next, prev, 64, inf, NaN, -inf
    assert ["disparity_clamped" in l for l in lo[:9]] == [True, True, False, False, True, False, False, False, True]
    assert "disparity_nan" in lo[7] and "inlier" in lo[7]           # std::max keeps the NaN, and NaN > 2.5 is false
    c = [c for c in GC.filter_cases() if c["name"] == "straddle2.5"][0]
    lo = filt["straddle2.5"][(1, 0)]["kp_labels"][0]
    for k in range(c["straddle_pairs"]):
        assert "inlier" in lo[2 * k] and "outlier" in lo[2 * k + 1]
        assert abs(int(c["disparity"][2 * k:2 * k + 2].view(np.int32)[0]) - int(c["disparity"][2 * k:2 * k + 2].view(np.int32)[1])) == 1
    lu = filt["offsets0.1"][(0, 1)]["kp_labels"][1]                  # float32(0.1) is not below 0.1, its neighbour is
    want = [["near_y_only"], ["near_skipped"], ["near_x_only"], ["near_skipped"], [], ["near_skipped"], ["near_y_only"],
            ["near_x_only"], ["near_y_only"], ["near_skipped"]]
    assert [sorted(l & {"near_skipped", "near_x_only", "near_y_only"}) for l in lu[:10]] == want
    lw = filt["border"][(0, 0)]["kp_labels"][2]                      # on 0 / width / height: outside; one float in: inside
    names = ["outside_left", "inside", "outside_right", "inside", "outside_top", "inside", "outside_bottom", "inside",
             "inside", "projection_nan", "inside", "projection_nan"]
    assert [n in l for n, l in zip(names, lw)] == [True] * len(names)
    assert filt["border"][(0, 0)]["inside"] == sum("inside" in l for l in lw)


# ------------------------------------------------------------------ float32 statement against its float64 twin
def _rel(a, b):
    a, b = np.asarray(a, D), np.asarray(b, D)
    scale = np.max(np.abs(b)) if b.size else 0.0
    return float(np.max(np.abs(a - b)) / scale) if scale > 0 else float(np.max(np.abs(a - b), initial=0.0))


def twin_deviations():
    """largest relative deviation (max |f32 - f64| over max |f64|, per array) of every float result over the cases
    whose labels hold no threshold, NaN or rank-deficient label; integer results must agree there"""
    dev = {}

    def note(key, a, b):
        dev[key] = max(dev.get(key, 0.0), _rel(a, b))

    r32, r64 = GC.reproj_results(F), GC.reproj_results(D)
    n_cases = 0
    for name in r32:
        a, b = r32[name], r64[name]
        if (a["labels"] | b["labels"]) & set(GC.NO_TWIN_LABELS):
            continue
        n_cases += 1
        assert np.array_equal(a["flags"], b["flags"]), name
        note("merged kps2d", a["kps2d"], b["kps2d"])
        note("initial cost", a["gn"]["initial_cost"], b["gn"]["initial_cost"])
        note("J^T J", a["H"], b["H"])
        note("J^T diff", a["e"], b["e"])
        note("pose", a["gn"]["pose"], b["gn"]["pose"])
        note("final cost", a["gn"]["cost"], b["gn"]["cost"])
    assert n_cases >= 12, n_cases
    f32, f64 = GC.filter_results(F), GC.filter_results(D)
    n_cases = 0
    for name in f32:
        a, b = f32[name][(1, 1)], f64[name][(1, 1)]
        if (a["labels"] | b["labels"]) & set(GC.NO_TWIN_LABELS):
            continue
        n_cases += 1
        for key in ("outlier", "inlier", "flags"):
            assert np.array_equal(a[key], b[key]), (name, key)
        assert a["inside"] == b["inside"], name
        for key in ("kf_inv_depth", "kf_variance", "kps3d", "kps2d"):
            note(key, a[key], b[key])
    assert n_cases >= 6, n_cases
    return dev


# measured (this file, the cases of geometry_cases.py) and the bound: 4 x measured, rounded up to two digits
TWIN_BOUNDS = {
    "merged kps2d": 0.0,    # measured 0
    "initial cost": 2.7e-06,    # measured 6.63e-07
    "J^T J": 1.2e-06,           # measured 2.79e-07
    "J^T diff": 0.0025,        # measured 0.000618
    "pose": 0.00053,            # measured 0.000132
    "final cost": 0.00011,      # measured 2.54e-05
    "kf_inv_depth": 1.1e-06,    # measured 2.67e-07
    "kf_variance": 0.027,     # measured 0.00656
    "kps3d": 9.1e-07,           # measured 2.27e-07
    "kps2d": 5e-06,           # measured 1.24e-06
}


def test_float32_statements_stay_close_to_their_float64_twins():
    dev = twin_deviations()
    print({k: float(f"{v:.3g}") for k, v in dev.items()})
    assert set(dev) == set(TWIN_BOUNDS)
    for key, v in dev.items():
        assert v <= TWIN_BOUNDS[key], (key, v, TWIN_BOUNDS[key])
