"""What the tracker-form KLT cases of tests/klt_tracker_cases.py reach, asserted without a GPU from the numpy statement
(window_cases.klt_ref) run on the starts that the oracle's projection gives: every way a level can end that the stage
cases reach, in both kernel shapes, and each situation of the keyframe's template cache that
tests/test_klt_tracker_gpu.py is there for, as a predicate on the cases. And the host-only layout getter."""
import collections

import numpy as np
import pytest

import klt_tracker_cases as KC
import oracle_py as O
import window_cases as WC
from geometry_cases import same_bits
from test_window_cpu import klt_margin

SHAPES = {"32 columns": lambda win: win <= 31, "36 columns": lambda win: win > 31}


@pytest.fixture(scope="module")
def runs():
    """name -> {call: (starts, (pts, status, err, info))} for the first frame (1) and the later one (3)"""
    out = {}
    for c in KC.cases():
        pl, cl, cl2 = KC.levels(c)
        ref = c["table"][c["kp_index"]]
        out[c["name"]] = {call: (st, WC.klt_ref(pl, cur, ref, st, c["win"]))
                          for call, cur, st in ((1, cl, KC.starts(c, 1)), (3, cl2, KC.starts(c, 3)))}
    return out


def test_cache_layout_getter():
    """svo_klt_cache_layout against klt_template_bytes, restated from the kernel's shapes: a thread of the 32-column
    shape owns 16 rows, one of the 36-column shape 36, as int16 pairs of I, Ix, Iy in 16-byte quarters of 64 lanes"""
    from stereo_svo_slam_amd import hip_lib
    for win, rows_per_thread in ((31, 16), (35, 36), (3, 16), (33, 36)):
        quarters = (3 * (rows_per_thread // 2) + 3) // 4
        rec, off, hdr, lv = hip_lib.klt_cache_layout(win)
        assert (rec, off, hdr, lv) == (quarters * 64 * 16 + 64, quarters * 64 * 16, 32, KC.LK_LEVELS), win
        assert off % 16 == 0 and rec % 16 == 0 and off + hdr <= rec
    assert hip_lib.klt_cache_layout(31)[0] == 6208 and hip_lib.klt_cache_layout(35)[0] == 14400
    for win in (2, 36):
        with pytest.raises(hip_lib.SvoError):
            hip_lib.klt_cache_layout(win)


def test_keyframe_tables():
    for c in KC.cases():
        n, m = len(c["pts"]), len(c["table"])
        assert m >= n + 8 and len(set(c["kp_index"].tolist())) == n and c["kp_index"].max() < m
        assert np.array_equal(c["table"][c["kp_index"]], c["pts"])
        unused = np.setdiff1d(np.arange(m), c["kp_index"])
        used = {tuple(p) for p in c["pts"].tolist()}
        assert not any(tuple(p) in used for p in c["table"][unused].tolist()), c["name"]
        h, w = c["prev"].shape
        assert (c["table"][unused] >= 0).all() and (c["table"][unused][:, 0] < w + 1).all()
    assert {tuple(c["pose"]) for c in KC.cases()} == {tuple(p) for p in KC.POSES}
    assert any(c["cam"]["k1"] != 0 for c in KC.cases()) and any(c["cam"]["k1"] == 0 for c in KC.cases())
    depth = np.concatenate([np.linalg.norm(c["kps3d"][c["absurd"] < 0] - c["pose"][:3], axis=1) for c in KC.cases()])
    assert depth.min() < 0.1 and depth.max() > 300


def test_projection_lands_near_the_desired_start(runs):
    """pinhole: within 0.01 px (float32 points at depths down to 0.05 and a float result); with the distortion terms
    the fixed-point inverse is good to a pixel inside the image"""
    for c in KC.cases():
        ok = c["absurd"] < 0
        d = np.abs(runs[c["name"]][1][0][ok] - c["init"][ok]).max(axis=1)
        d2 = np.abs(runs[c["name"]][3][0][ok] - c["init2"][ok]).max(axis=1)
        h, w = c["prev"].shape
        inside = (np.abs(c["init"][ok] - [w / 2, h / 2]) < [w / 2, h / 2]).all(axis=1)
        if c["cam"]["k1"] == 0:
            assert d.max() < 0.01 and d2.max() < 0.01, (c["name"], d.max(), d2.max())
        else:
            assert d[inside].max() < 1.0, (c["name"], d[inside].max())


def test_oracle_equals_the_statement_on_projected_starts(runs):
    for c in KC.cases():
        pl, cl, cl2 = KC.levels(c)
        ref = c["table"][c["kp_index"]]
        for call, cur in ((1, cl), (3, cl2)):
            st, (rp, rs, re_, _) = runs[c["name"]][call]
            op, os_, oe = O.klt_track(pl, cur, ref, st, c["win"])
            assert np.array_equal(os_, rs), (c["name"], call)
            assert same_bits(op, rp).all() and same_bits(oe, re_).all(), (c["name"], call)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tracker_cases_reach_what_the_stage_cases_reach(runs, shape):
    """every label of WC.LABELS (the stage cases reach them all, test_window_cpu.py) on the projected starts"""
    seen = collections.Counter()
    for c in KC.cases():
        if SHAPES[shape](c["win"]):
            for labs in runs[c["name"]][1][1][3]["labels"]:
                seen.update(l for l in labs if l is not None)
    print(shape, dict(seen))
    for lab in WC.LABELS:
        assert seen[lab] > 0, f"no level ended as {lab}"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cases_hold_every_cache_situation(runs, shape):
    margin = klt_margin()
    count = collections.Counter()
    for c in KC.cases():
        if not SHAPES[shape](c["win"]):
            continue
        win, top = c["win"], KC.top_level(c)
        pl, cl, cl2 = KC.levels(c)
        lh, lw = cl[top].shape
        scale = 1.0 / (1 << top)
        st1, (_, _, _, info1) = runs[c["name"]][1]
        st3, (_, _, _, info3) = runs[c["name"]][3]
        cached = c["kp_index"] < c["tmpl_cap"]
        count["kp_index >= tmpl_cap"] += int((~cached).sum())
        count["tmpl_cap below the largest kp_index"] += c["tmpl_cap"] <= c["kp_index"].max()
        count["kp_index == tmpl_cap"] += int((c["kp_index"] == c["tmpl_cap"]).sum())
        count["kp_index == tmpl_cap - 1"] += int((c["kp_index"] == c["tmpl_cap"] - 1).sum())
        for i in range(len(c["pts"])):
            labs = info1["labels"][i]
            if not cached[i]:
                continue
            # the states that the first frame leaves in the records of this point, one per level
            count["cached KLT_FLAT level"] += "flat" in labs
            count["cached KLT_OUTSIDE level"] += "prev_outside" in labs
            if labs[top] in ("flat", "prev_outside"):
                continue
            # a trackable template at the coarsest level: what the later frame's hit does there
            with np.errstate(all="ignore"):
                r1 = KC.prefetch_rect(st1[i, 0] * np.float32(scale), st1[i, 1] * np.float32(scale), lw, lh, win, margin)
                r3 = KC.prefetch_rect(st3[i, 0] * np.float32(scale), st3[i, 1] * np.float32(scale), lw, lh, win, margin)
            if r3 is None:
                # floor(x - halfWin) outside [-win, w) or floor(y - halfWin) outside [-win, h): `look` is false
                count["hit where look is false"] += 1
                assert info3["labels"][i][top] == "left_range_in_iteration"
            elif r1 is not None:
                # the window corner of the later call's start lies outside the first call's prefetched tile rectangle
                x3 = np.floor(np.float32(st3[i, 0] * np.float32(scale)) - np.float32(win - 1) * np.float32(0.5))
                y3 = np.floor(np.float32(st3[i, 1] * np.float32(scale)) - np.float32(win - 1) * np.float32(0.5))
                if x3 < r1[0] or y3 < r1[1] or x3 + win + 1 > r1[2] or y3 + win + 1 > r1[3]:
                    count["hit far from where the first call looked"] += 1
                else:
                    count["hit where the first call looked"] += 1
        bad = c["absurd"] >= 0
        for kind in set(c["absurd"][bad].tolist()):
            count["absurd " + KC.ABSURD_KINDS[kind]] += 1
        for call in (1, 3):
            s = runs[c["name"]][call][0][bad]
            count["NaN start"] += int(np.isnan(s).any(axis=1).sum())
            count["infinite start"] += int(np.isinf(s).any(axis=1).sum())
            with np.errstate(all="ignore"):
                count["finite start beyond int32"] += int((np.isfinite(s) & (np.abs(s) > 2.0 ** 31)).any(axis=1).sum())
    print(shape, dict(count))
    for what in ("kp_index >= tmpl_cap", "tmpl_cap below the largest kp_index", "kp_index == tmpl_cap", "kp_index == tmpl_cap - 1", "cached KLT_FLAT level", "cached KLT_OUTSIDE level",
                 "hit where look is false", "hit far from where the first call looked", "hit where the first call looked",
                 "NaN start", "infinite start", "finite start beyond int32") + tuple("absurd " + k for k in KC.ABSURD_KINDS):
        assert count[what] > 0, what
    assert count["hit far from where the first call looked"] >= 50 and count["hit where look is false"] >= 50


@pytest.mark.parametrize("win", [31, 35])
def test_composed_launches_are_what_they_say(win):
    (s,) = KC.several_keyframes(win)
    assert len(s["kfs"]) == 3 and set(s["kf_id"].tolist()) == {0, 1, 2}
    assert [len(k["levels"]) for k in s["kfs"]] == [3, 2, 1] and len(s["cur"]) == 3        # n_lk < n_cur for two of them
    assert len({k["levels"][0].tobytes() for k in s["kfs"]}) == 3
    assert (np.diff(s["kf_id"]) != 0).sum() > len(s["kf_id"]) // 3                          # interleaved, not in blocks
    (s,) = KC.ignored_caches(win)
    assert [k["cache"] for k in s["kfs"]] == ["wrong_win", None, "own"]
    own = s["kp_index"][s["kf_id"] == 2]
    assert own.max() > s["kfs"][2]["tmpl_cap"] > own.min() and (own == s["kfs"][2]["tmpl_cap"]).any()   # both sides, and on it
    flags = KC.expected_flags(s)
    assert flags[0] is None and flags[1] is None and 0 < flags[2].sum() < flags[2].size
    seqs = KC.batch_of_five(win)
    assert tuple(q["n"] for q in seqs) == KC.BATCH_COUNTS == (0, 1, 63, 65, KC.N_BOUND)
    assert len({q["cur"][0].shape for q in seqs}) >= 3                                      # images of several sizes
    assert all(q["kfs"][0]["cache"] == "own" for q in seqs)                                 # spare workgroups beside cached ones
    for q in seqs:
        assert len(set(q["kp_index"].tolist())) == q["n"]
        e = KC.expected_sequence(q)
        assert e["tracked"].shape == (q["n"], 2)
