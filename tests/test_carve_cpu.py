"""The carve without a GPU: the two formulations of tests/carve_ref.py agree on every crafted case of
tests/carve_cases.py, every case reaches what it was made for (asserted from the labels the reference returns, and from
a plain sequential placement for the probe chain), the carve does what it is for on a wall and a box with occluders
made by hand, the C ABI of the new structs and the prototype, and the host arithmetic of the stage entry
(csrc/svo_voxel_plan.hpp) in a stand-alone program, plain and under the address and undefined-behaviour sanitizers.

The stage entry checks its handle first, and a handle needs a GPU: its rejections are in tests/test_carve_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import carve_cases as CC
import carve_ref as CR
import voxel_prune_ref as PR
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _judged(name):
    """(case, map before, verdict of every mark by name, result, labels of all entries)"""
    case = CC.case(name)
    m = VR.run(case)[0]
    each = CR.judge_each(m, case["cam"], *case["size"], case["lattice"], case["rule"])
    index = {int(k): i for i, k in enumerate(m.keys)}
    assert set(index) >= set(case["marks"].values()) and len(index) == len(case["marks"])
    after, res, label = CR.carved(m, case["cam"], *case["size"], case["lattice"], case["rule"], case["keep"])
    return case, m, {n: each[index[k]] for n, k in case["marks"].items()}, res, after, each


def _labels(marks):
    return {n: CR.LABELS[int(v["label"])] for n, v in marks.items()}


@pytest.mark.parametrize("name", CC.NAMES)
def test_two_formulations_agree(name):
    case = CC.case(name)
    m = VR.run(case)[0]
    scalar = VR.run(case, VR.ScalarMap)[0]
    assert sorted(scalar.entries) == [int(k) for k in m.keys]
    each = CR.judge_each(m, case["cam"], *case["size"], case["lattice"], case["rule"])
    every = CR.judge_all(m, case["cam"], *case["size"], case["lattice"], case["rule"])
    assert np.array_equal(each["label"], every)
    # the point of step 1, written twice: per entry here, by voxel_ref's extraction there
    pts = m.extract()
    for i, (k, a) in enumerate(zip(m.keys, m.acc)):
        w = CR.point_of(k, a, m.voxel)
        assert (w[0], w[1], w[2]) == (pts["x"][i], pts["y"][i], pts["z"][i])
    after, res, _ = CR.carved(m, case["cam"], *case["size"], case["lattice"], case["rule"], case["keep"])
    assert res["n_before"] == m.n_voxels and res["n_kept"] == after.n_voxels
    assert (after.n_fused, after.n_outside) == (m.n_fused, m.n_outside)               # the cumulative counters stay
    keep = set(int(k) for k in after.keys)
    for i, k in enumerate(m.keys):
        if int(k) in keep:
            assert np.array_equal(after.acc[list(after.keys).index(k)], m.acc[i])      # the accumulators are unchanged


def test_bounds():
    for name, on_lattice in (("bounds", False), ("bounds_step5", True)):
        case, m, v, res, after, _ = _judged(name)
        lab = _labels(v)
        assert lab["late"] == "late" and lab["last_eq"] == "carved"                    # last > max_last | last == max_last
        assert (v["near_lt"]["c2"], lab["near_lt"]) == (F(0.25), "near") and (v["near_eq"]["c2"], lab["near_eq"]) == (case["rule"]["near"], "carved")
        assert (v["u_0"]["u"], lab["u_0"]) == (F(0), "carved") and (v["v_0"]["v"], lab["v_0"]) == (F(0), "carved")
        assert v["u_neg"]["u"] < 0 and lab["u_neg"] == "outside_image" and v["v_neg"]["v"] < 0 and lab["v_neg"] == "outside_image"
        assert (v["u_w"]["u"], lab["u_w"]) == (F(CC.W), "outside_image") and (v["v_h"]["v"], lab["v_h"]) == (F(CC.H), "outside_image")
        assert CC.W - 1 < v["u_lt_w"]["u"] < CC.W and CC.H - 1 < v["v_lt_h"]["v"] < CC.H
        beyond = "carved" if on_lattice else "outside_lattice"
        assert [lab[n] for n in ("u_lt_w", "v_lt_h", "beyond_cols", "beyond_rows")] == [beyond] * 4
        assert (lab["last_col"], lab["last_row"]) == ("carved", "carved")
        assert int(v["beyond_cols"]["u"]) // 4 == 12 and int(v["beyond_rows"]["v"]) // 4 == 7 and int(v["last_col"]["u"]) // 4 == 11
        cols, rows, step = case["lattice"][1:]
        assert (cols * step < CC.W and rows * step < CC.H) != on_lattice


def test_not_finite():
    case, m, v, res, after, _ = _judged("not_finite")
    assert _labels(v) == {"inf": "not_finite", "finite": "outside_image"}
    w = CR.point_of(case["marks"]["inf"], m.acc[list(m.keys).index(case["marks"]["inf"])], m.voxel)
    with np.errstate(over="ignore"):
        assert np.isinf(case["cam"][0] * w[0]) and np.isfinite(case["cam"]).all()       # a finite camera, an infinite c_0
    assert res["n_tested"] == 0 and after.n_voxels == 2


def test_compare():
    case, m, v, res, after, _ = _judged("compare")
    assert _labels(v) == {"tie": "behind", "next": "carved"}
    margin = case["rule"]["margin"]
    assert F(v["tie"]["c2"] + margin) == v["tie"]["zmin"]
    assert F(v["next"]["c2"] + margin) == np.nextafter(v["next"]["zmin"], F(0)) and v["next"]["zmin"] > v["tie"]["zmin"]


def test_clipped_rings():
    for ring, want in ((0, [1] * 9), (1, [4, 4, 4, 4, 6, 6, 6, 6, 9])):
        case, m, v, res, after, _ = _judged("clip_ring%d" % ring)
        assert [int(v[n]["cells"]) for n in ("nw", "ne", "sw", "se", "n", "s", "w", "e", "mid")] == want
        assert set(_labels(v).values()) == {"carved"} and after.n_voxels == 0


def test_cells_without_a_depth():
    for ring in (0, 1):
        case, m, v, res, after, _ = _judged("bad_ring%d" % ring)
        lab = _labels(v)
        rec, cols = case["lattice"][0], case["lattice"][1]
        for name, (ix, iy) in CC.BAD.items():
            assert lab[name] == "incomplete"                                            # the cell itself, under both rings
            assert lab[name + "_beside"] == ("incomplete" if ring else "carved")        # a neighbour, under the ring only
            assert not CR.has_depth(rec[iy * cols + ix], case["rule"]["drop_flags"])[0]
            assert CR.has_depth(rec[(iy + 1) * cols + ix + 1], case["rule"]["drop_flags"])[0]
        assert lab["other_flag"] == "carved" and rec["flags"][5 * cols + 10] != 0       # a flag that drop_flags does not name
        assert sorted(int(rec["flags"][iy * cols + ix]) for ix, iy in CC.BAD.values()) == [0, 0, 0, 0, VR.IGNORE_TEMPORARY, VR.DROPPED]
        z = [float(rec["z"][iy * cols + ix]) for ix, iy in (CC.BAD[n] for n in ("nan", "inf", "zero", "negative"))]
        assert np.isnan(z[0]) and np.isinf(z[1]) and z[2] == 0 and z[3] < 0


def test_the_foreground_rim():
    lab0, lab1 = _labels(_judged("rim_ring0")[2]), _labels(_judged("rim_ring1")[2])
    assert lab0 == {"rim": "carved", "inside": "behind", "far": "carved"}
    assert lab1 == {"rim": "behind", "inside": "behind", "far": "carved"}


def test_chain():
    """the carved entry lies in the middle of a probe chain: blanking it would cut off the entries behind it"""
    case, m, v, res, after, _ = _judged("chain")
    keys = [case["marks"]["chain%d" % i] for i in range(CC.CHAIN_KEYS)]
    log2 = case["maps"][0][1]
    table = PR.place(keys, log2)
    assert [table.index(k) for k in keys] == [59, 60, 61, 62] and all(VR.home(k, log2) == 59 for k in keys)
    assert _labels(v) == {"chain0": "late", "chain1": "carved", "chain2": "late", "chain3": "late"}
    table[60] = VR.EMPTY
    assert PR.lookup(table, keys[2], log2) is None and PR.lookup(table, keys[3], log2) is None
    rebuilt = PR.place([int(k) for k in after.keys], log2)
    assert all(PR.lookup(rebuilt, k, log2) is not None for k in (keys[0], keys[2], keys[3]))
    assert [int(k) for k in after.keys] == sorted(k for i, k in enumerate(keys) if i != CC.CHAIN_CARVED)


def test_both_reject_and_the_degenerate_ones():
    case, m, v, res, after, _ = _judged("both_reject")
    assert _labels(v) == {"both": "carved", "keep_only": "behind", "carve_only": "carved", "stays": "behind"}
    kept = PR.kept_mask(m, **case["keep"])
    by = {n: bool(kept[list(m.keys).index(k)]) for n, k in case["marks"].items()}
    assert by == {"both": False, "keep_only": False, "carve_only": True, "stays": True}
    assert res == {"n_before": 4, "n_kept": 1, "n_tested": 4, "n_carved": 2} and [int(k) for k in after.keys] == [case["marks"]["stays"]]
    assert _judged("none_carved")[3] == {"n_before": 84, "n_kept": 84, "n_tested": 84, "n_carved": 0}
    assert _judged("all_carved")[3] == {"n_before": 84, "n_kept": 0, "n_tested": 84, "n_carved": 84}
    assert _judged("empty")[3] == {"n_before": 0, "n_kept": 0, "n_tested": 0, "n_carved": 0}
    case, m, v, res, after, _ = _judged("null_occluder")
    assert case["lattice"] is None and set(_labels(v).values()) == {"no_occluder"}
    pruned = PR.pruned(m, **case["keep"])
    assert 0 < pruned.n_voxels < m.n_voxels and np.array_equal(pruned.keys, after.keys) and res["n_tested"] == res["n_carved"] == 0


# ------------------------------------------------------------------------------------------------ what it is for

def _plane(us, vs, c2):
    """records on the plane c_2 = const that the camera of the cases sees at the pixels (us x vs)"""
    uu, vv = np.meshgrid(np.asarray(us, np.float64), np.asarray(vs, np.float64))
    xyz = np.stack([(uu - CC.CX) * c2 / CC.FX, (vv - CC.CY) * c2 / CC.FY, np.full(uu.shape, c2 + CC.EYE_Z)], axis=-1)
    return VR.records(xyz.reshape(-1, 3))


def _room():
    """a wall at c_2 = 4 that is wider than the view, a box at c_2 = 2 over the pixels 15 .. 34 x 10 .. 24 and points
    behind the wall at c_2 = 6, fused into one map; of every entry: (c_2, u, v) by the reference and what it is part of"""
    wall = _plane(np.arange(-19.5, 70, 1.0), np.arange(-9.5, 40, 1.0), 4.0)
    box = _plane(np.arange(15.25, 35, 0.5), np.arange(10.25, 25, 0.5), 2.0)
    behind = _plane(np.arange(0.5, 50, 1.0), np.arange(0.5, 30, 1.0), 6.0)
    m = VR.Map(CC.VOXEL, 14)
    for rec in (wall, box, behind):
        assert m.admits(len(rec))
        m.fuse(rec, 1)
    pts = m.extract()
    c2 = (pts["z"] - F(CC.EYE_Z)).astype(F)
    part = np.where(c2 < 3, 0, np.where(c2 < 5, 1, 2))                                  # box, wall, behind
    assert {int((part == p).sum()) > 50 for p in range(3)} == {True}
    return m, part


def test_what_the_carve_is_for():
    m, part = _room()
    cam, rule = CC.camera(), CR.carve_rule(CC.VOXEL, near=0.5, ring=1)
    wall_only = CC.lattice(10, 6, 5, z=4.0)
    each = CR.judge_each(m, cam, CC.W, CC.H, tuple(wall_only), rule)
    carved = each["label"] == CR.CARVED
    in_view = (each["u"] >= 0) & (each["u"] < CC.W) & (each["v"] >= 0) & (each["v"] < CC.H)    # (NaN where the rule left earlier)
    assert in_view[part == 0].all() and carved[part == 0].all()                         # every box entry inside the view is carved
    assert not carved[part != 0].any()                                                  # no wall entry, none behind the wall
    assert (part == 1)[~in_view].any() and not carved[~in_view].any()                   # and none outside the view
    # the box still stands in the occluder: nothing is carved, the rim included
    with_box = CC.lattice(10, 6, 5, z=4.0)
    z = with_box[0]["z"].reshape(6, 10)
    z[2:5, 3:7] = F(2.0)                                                                # the cells of the pixels 15 .. 34 x 10 .. 24
    again = CR.judge_each(m, cam, CC.W, CC.H, tuple(with_box), rule)
    assert not (again["label"] == CR.CARVED).any()
    rim = (part == 1) & (again["label"] == CR.BEHIND) & (again["zmin"] == F(2.0))
    assert rim.any()                                                                    # wall entries whose ring meets the box
    assert np.array_equal(CR.judge_all(m, cam, CC.W, CC.H, tuple(with_box), rule), again["label"])
    assert np.array_equal(CR.judge_all(m, cam, CC.W, CC.H, tuple(wall_only), rule), each["label"])


# ------------------------------------------------------------------------------------------------ the C ABI and the host arithmetic

def test_struct_layouts_symbol_and_prototype(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header"
    ctypes_of = {"svo_voxel_carve_rule": hip_lib.VoxelCarve, "svo_voxel_carve_result": hip_lib.VoxelCarveResult}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n')
    inc = "-I" + os.path.join(ROOT, "include")
    protos = tmp_path / "protos.c"
    protos.write_text('#include "svo_hip.h"\n'
                      "int (*entry)(svo_handle *, const svo_voxel_map *, const svo_ar_camera *, int, int, const svo_ar_occluder *,\n"
                      "             const svo_voxel_carve_rule *, const svo_voxel_keep *, svo_voxel_carve_result *) = svo_voxel_carve;\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", inc, "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", inc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}
    for name, cls in ctypes_of.items():
        assert c[name] == C.sizeof(cls) == 32, name
        for f, _ in cls._fields_:
            assert c[f"{name}.{f}"] == getattr(cls, f).offset, (name, f)
    assert "svo_voxel_carve" in hip_lib.SYMBOLS
    getattr(hip_lib.lib(), "svo_voxel_carve")
    r = hip_lib.voxel_carve(0.5, near=0.25, ring=0, max_last=7, drop_flags=4)
    assert (r.margin, r.near, r.ring, r.max_last, r.drop_flags, list(r._reserved)) == (0.5, 0.25, 0, 7, 4, [0, 0, 0])
    d = hip_lib.voxel_carve(0.1)
    assert (d.ring, d.max_last, d.drop_flags) == (1, 0xFFFFFFFF, 0) and d.near > 0


def test_the_job_s_record_entries_and_python_surface(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc
    dt = hip_lib.CARVE_INFO_DTYPE
    lines = ['  printf("size %zu\\n", sizeof(svo_carve_info));\n'] + [f'  printf("{f} %zu\\n", offsetof(svo_carve_info, {f}));\n' for f in dt.names]
    lines.append('  printf("enums %d %d %d %d %d\\n", SVO_CARVE_OK, SVO_CARVE_NO_MAP, SVO_CARVE_NO_POSE, SVO_CARVE_TOO_LARGE, SVO_CARVE_NONE);\n')
    src = tmp_path / "info.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svo_hip.h"\n'
                   "int (*submit)(svo_ctx *, const int *, int, const svo_cloud_style *, const svo_sgm_params *, const svo_stereo_check *,\n"
                   "              const svo_voxel_carve_rule *, const svo_voxel_keep *, int, const float *, svo_carve_info *);\n"
                   "int main(void) {\n  submit = svo_submit_carve_voxel_maps; submit = svo_carve_voxel_maps;\n" + "".join(lines) + "  return 0;\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "info.o")])
    exe = tmp_path / "info"
    stub = tmp_path / "stub.c"
    stub.write_text("int svo_submit_carve_voxel_maps(void) { return 0; }\nint svo_carve_voxel_maps(void) { return 0; }\n")
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), str(stub), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    assert c["size"] == [dt.itemsize] == [64]
    for f in dt.names:
        assert c[f] == [dt.fields[f][1]], f
    assert c["enums"] == [hip_lib.CARVE_OK, hip_lib.CARVE_NO_MAP, hip_lib.CARVE_NO_POSE, hip_lib.CARVE_TOO_LARGE, hip_lib.CARVE_NONE] == [0, 1, 2, 3, 4]
    assert (hip_lib.CARVE_OK, hip_lib.CARVE_NO_MAP, hip_lib.CARVE_NO_POSE, hip_lib.CARVE_TOO_LARGE) == \
        (hip_lib.PRUNE_OK, hip_lib.PRUNE_NO_MAP, hip_lib.PRUNE_NO_POSE, hip_lib.PRUNE_TOO_LARGE)
    lib = hip_lib.lib()
    for sym in ("svo_submit_carve_voxel_maps", "svo_carve_voxel_maps"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)
    from stereo_svo_slam_amd import jobs, stereo_slam
    assert issubclass(jobs.Carve, jobs.Prune) and issubclass(jobs.Prune, jobs.Job)
    for name in ("submit_carve", "carve_voxel_maps"):
        assert callable(getattr(stereo_slam.StereoSlamBatch, name))
    assert callable(stereo_slam.StereoSlam.carve_voxel_map)
    import inspect
    assert "carve" in inspect.signature(stereo_slam.StereoSlamBatch.fuse_new_keyframes).parameters


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """the carve's host arithmetic as a program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("voxel_carve_plan")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "voxel_carve_plan_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", src]
    out = {"plain": str(d / "voxel_carve_plan_check"), "sanitized": str(d / "voxel_carve_plan_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_planner(planner, which):
    asks = [((0.0, 0.01, 0, 1, 1), True), ((0.25, 0.5, 1, 32768, 32768), True), ((3e38, 3e38, 1, 752, 480), True),
            ((-0.0, 1e-30, 0, 50, 30), True), ((-1e-30, 0.5, 1, 50, 30), False), (("nan", 0.5, 1, 50, 30), False),
            (("inf", 0.5, 1, 50, 30), False), ((0.25, 0.0, 1, 50, 30), False), ((0.25, -1.0, 1, 50, 30), False),
            ((0.25, "nan", 1, 50, 30), False), ((0.25, "inf", 1, 50, 30), False), ((0.25, 0.5, 2, 50, 30), False),
            ((0.25, 0.5, -1, 50, 30), False), ((0.25, 0.5, 1, 0, 30), False), ((0.25, 0.5, 1, 50, 0), False),
            ((0.25, 0.5, 1, 32769, 30), False), ((0.25, 0.5, 1, 50, 32769), False), ((0.25, 0.5, 1, -5, 30), False)]
    args = [str(x) for a, _ in asks for x in a]
    r = subprocess.run([planner[which]] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[:len(asks)] == ["ok" if ok else "bad" for _, ok in asks]
    plans = [[int(x) for x in line.split()[1:]] for line in lines[len(asks):] if line.startswith("plan")]
    assert [p[0] for p in plans] == list(range(6, 27))
    for log2, ballots, counters, total in plans:
        waves = max(1, (1 << log2) // 256) * 4
        assert (ballots, counters, total) == (0, (8 * waves + 255) // 256 * 256, (8 * waves + 255) // 256 * 256 + 256)
