"""The statements of tests/bookkeeping_cases.py against the CPU oracle's accessors (oracle/tracker.c, which calls
them itself on every frame), bit for bit, on every crafted case; what the cases reach, from the statements' labels;
the float statement of the initialisation against its float64 twin; and, on the host, the launch shapes and the size
of a keyframe's "stored" flags. No GPU."""
import numpy as np
import pytest

import bookkeeping_cases as BC
import oracle_py as O
from stereo_svo_slam_amd import hip_lib

F, D, U = np.float32, np.float64, np.uint32


def ocam(cam):
    return O.make_camera(**{k: float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline")})


def oracle_kept(c):
    n = c["src"]["n"]
    fl = c["src"]["flags"][:n, 0]
    if c["mode"] == 0:
        return O.remove_outliers(fl)
    return O.find_bad_keypoints(BC.f32(c["src"]["kps2d"][:n]), fl, c["width"], c["height"])


def oracle_select(c):
    sel, sc, ty, lv = O.select_best_keypoints([(np.stack([l["x"], l["y"]], 1), l["score"], l["type"]) for l in c["levels"]])
    return dict(x=sel[:, 0].copy(), y=sel[:, 1].copy(), score=sc, type=ty, level=lv)


def oracle_picked(c, sel):
    n_old = c["kps"]["n"]
    return O.merge_keypoints(BC.f32(c["kps"]["kps2d"][:n_old]).reshape(-1, 2), np.stack([sel["x"], sel["y"]], 1),
                             c["width"], c["height"], c["grid_width"], c["grid_height"])


def oracle_init(c):
    """the oracle's depth_init and backup_rule in the form of init_ref's result"""
    kps = BC.copy_set(c["kps"])
    n, old = kps["n"], c["old_count"]
    pose = np.zeros(6, F) if c["first_frame"] else c["frame_pose"]
    k3, info, st = O.depth_init(ocam(c["cam"]), pose, BC.f32(kps["kps2d"][:n]), BC.f32(c["disparity"][:n]), old,
                                c["new_kf_id"], BC.LCG_SEED if c["first_frame"] else c["lcg"])
    s = slice(old, n)
    kps["kps3d"][s] = BC.bits(k3[s]).reshape(-1, 3)
    kps["color"][s, 0] = (info["color"][s, 0].astype(U) | (info["color"][s, 1].astype(U) << U(8)) |
                          (info["color"][s, 2].astype(U) << U(16)))
    kps["kf_id"][s, 0] = info["keyframe_id"][s].view(U)
    kps["kp_index"][s, 0] = info["keypoint_index"][s].view(U)
    kps["flags"][s, 0] = (info["ignore_during_refinement"][s] * U(1) + info["ignore_completely"][s] * U(2) +
                          info["ignore_temporary"][s] * U(4)).astype(U)
    kps["inlier_count"][s, 0] = info["inlier_count"][s].view(U)
    kps["outlier_count"][s, 0] = info["outlier_count"][s].view(U)
    kps["kf_variance"][s, 0] = BC.bits(info["kf_variance"][s])
    kps["kf_inv_depth"][s, 0] = BC.bits(info["kf_inv_depth"][s])
    record = {name: kps[name][:n].copy() for name in BC.PLANE_NAMES}
    if c["first_frame"]:
        kps["flags"][:n] &= ~U(BC.IGNORE_TEMPORARY)
    else:
        kps["flags"][:n, 0] = O.backup_rule(kps["flags"][:n, 0])[0]           # (the words with their foreign bits)
    return dict(kps=kps, record=record, record_n=n, record_pose=np.asarray(pose, F), lcg=st, n_out=n)


def assert_same_values(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.ascontiguousarray(a[k]).reshape(-1), np.ascontiguousarray(b[k]).reshape(-1)
        assert x.view(U).tolist() == y.view(U).tolist() if x.size < 64 else np.array_equal(x.view(U), y.view(U)), (what, k)


# ------------------------------------------------------------------ oracle == statement
def test_compaction_oracle_equals_statement():
    seen = set()
    for c in BC.compact_cases():
        stated, labels = BC.compact_expect(c)
        seen.update(labels)
        if c["start"] or c["enable"] == 0:
            continue
        kept_s, _ = BC.compact_ref(c["src"], c["mode"], c["width"], c["height"])
        kept_o = oracle_kept(c)
        assert kept_o.tolist() == kept_s, c["name"]
        assert_same_values(BC.compact_expect(c, kept_o)[0], stated, c["name"])
    missing = set(BC.COMPACT_LABELS + BC.LIVE_LABELS) - seen
    assert not missing, f"labels no compaction case reaches: {sorted(missing)}"


def test_compaction_cases_hold_what_the_issue_lists():
    cs = BC.compact_cases()
    for cap in (1024, 1100, 2048):
        ns = {c["src"]["n"] for c in cs if c["cap"] == cap and not c["start"]}
        assert {0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, cap} <= ns
    assert {c["src"]["n"] for c in cs if c["cap"] >= 1100} >= {1025}
    assert {(c["cap"], c["src"]["n"]) for c in cs if c["start"]} >= {(1024, 777), (1024, 1029), (2048, 2053)}
    assert {c["zero_count"] for c in cs} >= {0, 1, 5, 257, 1025}
    assert {c["zero_res_count"] for c in cs} >= {0, 1, 5, 257, 1025}
    assert {c["enable"] for c in cs} >= {None, 0, 0x100}
    # the mask's two ends, from the statement itself
    by = {c["name"]: BC.compact_expect(c)[0]["min_kf"].view(U).tolist() for c in cs if c["name"].startswith("live-")}
    assert by["live-5-68"] == [5, 1, 0x80000000] and by["live-5-69"] == [5, 1, 0] and by["live-5-68-69"] == [5, 1, 0x80000000]
    assert by["live-31-32"] == [5, 0x80000001, 1] and by["live-only-31"] == [5, 0x80000001, 0] and by["live-only-32"] == [5, 1, 1]
    assert by["live-none-kept"] == [BC.INT_MAX, 0, 0] and by["live-min-dropped"][0] == 9 and by["live-min-dropped-last"][0] == 9
    assert by["live-id0"] == [0, 3, 0x80000000] and by["live-every-bit"] == [100, 0xFFFFFFFF, 0xFFFFFFFF]
    assert by["live-5000-spread"] == [5000, 0x80000001, 0x80000001]


def test_select_and_merge_oracle_equals_statement():
    seen = set()
    for c in BC.merge_cases():
        stated, labels = BC.merge_expect(c)
        seen.update(labels)
        sel_s, _ = BC.select_ref(c["levels"])
        sel_o = oracle_select(c)
        for k in sel_s:
            assert np.all(BC.same_bits(sel_s[k], sel_o[k])), (c["name"], k)
        cand = np.stack([sel_s["x"], sel_s["y"]], 1) if len(sel_s["x"]) else np.zeros((0, 2), F)
        n_old = c["kps"]["n"]
        picked_s = BC.merge_ref(BC.f32(c["kps"]["kps2d"][:n_old]).reshape(-1, 2), cand, c["width"], c["height"],
                                c["grid_width"], c["grid_height"])
        picked_o = oracle_picked(c, sel_o)
        assert picked_o.tolist() == picked_s, c["name"]
        assert_same_values(BC.merge_expect(c, sel_o, picked_o.tolist())[0], stated, c["name"])
    missing = set(BC.SELECT_LABELS + BC.MERGE_LABELS) - seen
    assert not missing, f"labels no merge case reaches: {sorted(missing)}"


def test_merge_capacity_cases_are_what_they_say():
    got = {}
    for c in BC.merge_cases():
        if c["name"].startswith("cap-"):
            v, _ = BC.merge_expect(c)
            got[c["name"]] = (int(v["kps.n"][0]), int(v["old_count"][0]), int(v["overflow"].view(U)[0]))
    same = BC.OVERFLOW_FILL                        # no overflow: the word is not written
    assert got["cap-old0"] == (30, 0, same) and got["cap-old-cap-1"] == (64, 63, 1) and got["cap-old-cap"] == (64, 64, 1)
    assert got["cap-exact"] == (64, 34, same) and got["cap-plus-1"] == (64, 35, 1)
    assert got["cap-exact-1024"] == (1024, 724, same) and got["cap-plus-1-1024"] == (1024, 725, 1)
    assert got["cap-plus-many-2048"] == (2048, 2000, 1)


def test_init_oracle_equals_statement():
    seen = set()
    for c in BC.init_cases():
        ref, labels = BC.init_ref(c)
        seen.update(labels)
        orc = oracle_init(c)
        assert_same_values(BC.init_expect(c, orc), BC.init_expect(c, ref), c["name"])
        assert orc["lcg"] == ref["lcg"] and orc["record_n"] == ref["record_n"], c["name"]
        assert np.array_equal(orc["record_pose"].view(U), ref["record_pose"].view(U)), c["name"]
    missing = set(BC.INIT_LABELS) - seen
    assert not missing, f"labels no initialisation case reaches: {sorted(missing)}"


def test_backup_rule_boundaries():
    for c in BC.init_cases():
        if c["name"].startswith("backup-"):
            n, nt = (int(v) for v in c["name"].split("-")[1:])
            ref, labels = BC.init_ref(c)
            cleared = not np.any(ref["kps"]["flags"][:n, 0] & U(BC.IGNORE_TEMPORARY))
            assert cleared == (nt < n // 4) == ("backup_cleared" in labels), c["name"]
            # the keyframe's copy keeps its temporaries
            assert np.all(ref["record"]["flags"][c["old_count"]:n, 0] == U(BC.IGNORE_TEMPORARY)), c["name"]
    want = {(8, 1): True, (8, 2): False, (7, 0): True, (7, 1): False, (3, 0): False}
    for (n, nt), clears in want.items():
        assert (nt < n // 4) == clears


def test_float_init_stays_within_the_derived_bound_of_its_twin():
    """The float statement rounds where the twin does not. With e = 2^-24 and every input a float in both:
    _z = b / m: 1 rounding; _x = (x - cx) / fx * _z: 3 more, so a component of the local point carries at most 4; an
    element of R is rounded to float once; a product once; the three-term sum (0 + p0 exact) twice: each term of a row
    carries at most 9 roundings, the translation's addition one more on the whole result. The float statement rounds
    the oracle's double R, the twin uses numpy's: their difference dR (a few 1e-16, computed here, not assumed zero)
    enters as it is. So |float - twin| <= ((1 + e)^9 - 1) sum_k |R_ik loc_k| + (1 + e)^8 sum_k |dR_ik loc_k|
    + e |result|; 1 / _z carries 2, deviation^2 carries 2 * 2 + 1 = 5 (b / fx, the cast of the double quotient, the
    square)."""
    e = D(2.0) ** -24
    checked = 0
    for c in BC.init_cases():
        f, _ = BC.init_ref(c, F)
        t, _ = BC.init_ref(c, D)
        cam = {k: D(F(c["cam"][k])) for k in ("fx", "fy", "cx", "cy", "baseline")}
        pose = np.zeros(6, D) if c["first_frame"] else c["frame_pose"].astype(D)
        R = np.abs(BC.GC.pose_mats(pose, D)[0])
        dR = np.abs(O.rodrigues(pose[3:6].astype(F)) - BC.GC.pose_mats(pose, D)[0])
        assert np.max(dR) < 1e-14, (c["name"], dR)
        for i in range(c["old_count"], c["kps"]["n"]):
            d = D(BC.f32(c["disparity"][i:i + 1])[0])
            z = cam["baseline"] / (d if 0.5 < d else 0.5)
            if not np.isfinite(z) or z == 0:
                continue
            x, y = (D(v) for v in BC.f32(c["kps"]["kps2d"][i]))
            loc = np.abs([(x - cam["cx"]) / cam["fx"] * z, (y - cam["cy"]) / cam["fy"] * z, z])
            got = BC.f32(f["kps"]["kps3d"][i]).astype(D)
            bound = ((1 + e) ** 9 - 1) * (R @ loc) + (1 + e) ** 8 * (dR @ loc) + e * np.abs(t["twin"]["kps3d"][i])
            assert np.all(np.abs(got - t["twin"]["kps3d"][i]) <= bound), (c["name"], i, got, t["twin"]["kps3d"][i], bound)
            kfx, kfP = (D(BC.f32(f["kps"][k][i])[0]) for k in ("kf_inv_depth", "kf_variance"))
            assert abs(kfx - t["twin"]["kfx"][i]) <= ((1 + e) ** 2 - 1) * abs(t["twin"]["kfx"][i]), (c["name"], i)
            assert abs(kfP - t["twin"]["kfP"][i]) <= ((1 + e) ** 5 - 1) * abs(t["twin"]["kfP"][i]), (c["name"], i)
            checked += 1
    assert checked > 2000


def test_nan_disparity_becomes_half_a_pixel():
    """std::max<float>(0.5, d) is (0.5 < d) ? d : 0.5: a NaN disparity is 0.5 in the reference, the statement and
    the oracle alike"""
    c = next(c for c in BC.init_cases() if c["name"] == "pow2-zero")
    i = c["old_count"] + 7
    assert np.isnan(BC.f32(c["disparity"][i:i + 1])[0])
    z = BC.f32(oracle_init(c)["kps"]["kps3d"][i])[2]
    assert z == F(c["cam"]["baseline"]) / F(0.5)


# ------------------------------------------------------------------ the launch shapes, on the host
@pytest.mark.parametrize("cap", [1, 255, 1023, 1024, 1025, 1100, 2048, 4096])
def test_compact_thread_shape(cap):
    assert hip_lib.keyframe_launch_info(cap, 1, 0)[0] == BC.compact_threads(cap) == (256 if cap <= 1024 else 1024)


@pytest.mark.parametrize("max_cells", [1, 255, 511, 512, 513, 1025, 2000])
def test_merge_thread_shape(max_cells):
    assert hip_lib.keyframe_launch_info(1, max_cells, 0)[1] == BC.merge_threads(max_cells) == (256 if max_cells <= 512 else 1024)


def test_tmpl_valid_bytes_is_a_multiple_of_4():
    """kf_init_kernel clears the flags as dwords: a size that is no multiple of 4 would leave the last ones set"""
    for tmpl_cap in list(range(0, 700)) + [1023, 1024, 1025, 4095, 4096, 4097, 65535]:
        b = hip_lib.keyframe_launch_info(1, 1, tmpl_cap)[2]
        assert b % 4 == 0 and b >= 3 * tmpl_cap, (tmpl_cap, b)


def test_ssd_shape_rule():
    assert [BC.ssd_pick_max_win(w, sy) for w, sy in ((31, 6), (32, 6), (31, 7), (35, 8), (5, 0))] == [31, 35, 35, 35, 31]
