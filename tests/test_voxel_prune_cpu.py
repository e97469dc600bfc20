"""The prune without a GPU: every crafted case of tests/voxel_prune_cases.py reaches what it is there for (asserted
from the statement, tests/voxel_prune_ref.py, and from a plain sequential placement), the properties the header
states hold for the statement itself, the C ABI of the new structs, and the host arithmetic of the prune
(csrc/svo_voxel_plan.hpp) in a stand-alone program, plain and under the address and undefined-behaviour sanitizers."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import voxel_cases as VC
import voxel_prune_cases as PC
import voxel_prune_ref as PR
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = (dict(), dict(min_count=2), dict(min_stamp=2), dict(min_count=3, min_stamp=2))


def _run(name):
    case = PC.case(name)
    m, = VR.run(case)
    return case, m


def _keys_in_order(case):
    keys = []
    for call in case["calls"]:
        (rec, _, _), = call
        _, inside, key, _ = VR.classify(rec, case["maps"][0][0], 0)
        assert len(rec) == 1 and inside.all()
        keys.append(int(key[0]))
    return keys


@pytest.mark.parametrize("name,leaves", [("chain_mid", (PC.CHAIN_MID_LEAVES,)), ("chain_wrap", PC.CHAIN_WRAP_LEAVES)])
def test_chain_cases_cut_a_chain(name, leaves):
    case, m = _run(name)
    log2 = VC.CHAIN_LOG2
    keys = _keys_in_order(case)
    assert keys == [int(k) for k in VC.chain_keys()[:len(keys)]] and {VR.home(k, log2) for k in keys} == {VC.CHAIN_HOME}
    table = PR.place(keys, log2)
    at = [table.index(k) for k in keys]
    assert at == [(VC.CHAIN_HOME + i) % 64 for i in range(len(keys))]            # one after the other from the home on
    mask = PR.kept_mask(m, **case["keep"])
    gone = sorted(int(k) for k in m.keys[~mask])
    assert gone == sorted(keys[i] for i in leaves) and 0 < len(gone) < len(keys)
    # blanking the keys that leave cuts the chain: entries behind the hole, whose home lies before it, are lost
    blanked = [VR.EMPTY if k in gone else k for k in table]
    behind = [k for i, k in enumerate(keys) if i > max(leaves)]
    assert behind and all(int(k) in m.keys[mask].tolist() for k in behind)
    assert all(PR.lookup(table, k, log2) is not None for k in behind) and all(PR.lookup(blanked, k, log2) is None for k in behind)
    if name == "chain_wrap":                                                        # the chain runs over the table's end
        assert at[4] == 63 and at[5] == 0 and {at[i] for i in leaves} == {63, 0} and at[-1] == 2
    else:
        assert max(at) < 63 and at[leaves[0]] not in (at[0], at[-1])                # the middle of a chain that does not wrap
    # a rebuilt table finds them all
    rebuilt = PR.place(sorted(int(k) for k in m.keys[mask]), log2)
    assert all(PR.lookup(rebuilt, k, log2) is not None for k in m.keys[mask])


@pytest.mark.parametrize("name", ["box", "box_negative", "box_face", "box_r0"])
def test_box_cases_sit_on_the_edges(name):
    case, m = _run(name)
    keep = case["keep"]
    voxel = case["maps"][0][0]
    c = np.array(PR.center_voxel(keep["center"], voxel)) - VR.BIAS
    cells = PC.box_cells(c, keep["radius"])
    assert m.n_voxels == len(cells) and m.n_outside == 0                            # every crafted cell became a voxel of its own
    labels = {tuple(int(x) + VR.BIAS for x in cell): lab for cell, lab in cells}
    mask = PR.kept_mask(m, **keep)
    for k, kept in zip(m.keys, mask):
        assert labels[VR.key_parts(k)] == bool(kept), (VR.key_parts(k), kept)
    r = keep["radius"]
    dist = [max(abs(np.array(VR.key_parts(k)) - VR.BIAS - c)) for k in m.keys]
    assert {d for d, kept in zip(dist, mask) if kept} >= {0, r} and r + 1 in {d for d, kept in zip(dist, mask) if not kept}
    for a in range(3):                                                              # each axis, each side, r and r + 1
        for side in (-1, 1):
            for d, want in ((r, True), (r + 1, False)):
                cell = c.copy()
                cell[a] += side * d
                assert labels[tuple(int(x) + VR.BIAS for x in cell)] == want
    if name == "box_negative":
        assert all(x < 0 for x in keep["center"]) and (c < 0).all()
    if name == "box_face":
        assert [float(x) for x in keep["center"]] == [2.0, -3.0, 0.0] and c.tolist() == [2, -3, 0]
    if name == "box_r0":
        assert r == 0 and mask.sum() == 1


def test_count_and_stamp_cases():
    case, m = _run("count_stamp")
    assert sorted(zip(m.acc[:, 0].tolist(), m.acc[:, 7].tolist())) == [(2, 5), (3, 4), (3, 5), (4, 6)]
    keep = case["keep"]
    assert (keep["min_count"], keep["min_stamp"]) == (3, 5)
    mask = PR.kept_mask(m, **keep)
    assert sorted(zip(m.acc[mask, 0].tolist(), m.acc[mask, 7].tolist())) == [(3, 5), (4, 6)]
    case, m = _run("min_count_0")
    assert case["keep"]["min_count"] == 0
    mask = PR.kept_mask(m, **case["keep"])
    assert sorted(zip(m.acc[mask, 0].tolist(), m.acc[mask, 7].tolist())) == [(2, 5), (3, 5), (4, 6)]


def test_extremes_and_the_full_map():
    case, m = _run("keep_all")
    assert m.n_voxels > 500 and PR.kept_mask(m, **case["keep"]).all() and case["keep"]["radius"] >= 0
    case, m = _run("keep_none")
    assert m.n_voxels > 500 and not PR.kept_mask(m, **case["keep"]).any()
    case, m = _run("empty")
    assert m.n_voxels == 0 and PR.prune(m, **case["keep"]) == (0, 0)
    case, m = _run("full")
    assert m.n_voxels == VR.load_limit(6) == 48 and not m.admits(1)
    assert PR.prune(m, **case["keep"]) == (48, 24) and m.admits(24) and not m.admits(25)
    assert len(set(PC.full_cells())) == 96
    case, m = _run("mixed")
    mask = PR.kept_mask(m, **case["keep"])
    by_test = [PR.kept_mask(m, min_count=2), PR.kept_mask(m, min_stamp=2), PR.kept_mask(m, center=case["keep"]["center"], radius=3)]
    assert all(0 < t.sum() < len(t) for t in by_test) and np.array_equal(mask, by_test[0] & by_test[1] & by_test[2])
    assert all((t & ~mask).any() for t in by_test)                                   # each test alone keeps more: all three decide


def test_no_case_fills_a_table():
    for name in PC.NAMES:
        case, m = _run(name)
        assert m.n_voxels <= VR.load_limit(m.log2_capacity), name
        for call in case["calls"]:
            assert len(call) == 1 and call[0][1] == 0


def test_properties_of_the_statement_on_mixed():
    rec, params = VC.mixed()
    m = VR.Map(*params)
    m.fuse(rec[:1500], 1)
    m.fuse(rec[1500:], 2)
    keep = PC.case("mixed")["keep"]
    before = copy.deepcopy(m)
    n_before, n_kept = PR.prune(m, **keep)
    assert (n_before, n_kept) == (before.n_voxels, m.n_voxels) and 0 < n_kept < n_before
    assert (m.n_fused, m.n_outside) == (before.n_fused, before.n_outside)            # cumulative
    # extraction after prune(K) with F == extraction before with "F and K", written out without the prune
    mask = PR.kept_mask(before, **keep)
    for f in FILTERS:
        both = mask & (before.acc[:, 0] >= max(1, f.get("min_count", 0))) & (before.acc[:, 7] >= f.get("min_stamp", 0))
        sub = copy.deepcopy(before)
        sub.keys, sub.acc = before.keys[both], before.acc[both]
        assert m.extract(**f).tobytes() == sub.extract().tobytes() == PR.extract_both(before, keep, **f).tobytes()
    once = copy.deepcopy(m)
    assert PR.prune(m, **keep) == (n_kept, n_kept)                                   # idempotent
    assert np.array_equal(m.keys, once.keys) and np.array_equal(m.acc, once.acc)
    # fusing on: the statement from the pruned content
    more = VC.mixed(400, seed=22)[0]
    m.fuse(more, 3)
    assert m.n_fused == before.n_fused + int(((more["flags"] & VR.DROPPED) == 0).sum())
    assert set(once.keys.tolist()) <= set(m.keys.tolist())


def test_center_voxel_follows_the_key_rule():
    assert PR.center_voxel((0.0, -0.0, 1e-10), 1.0) == (VR.BIAS, VR.BIAS, VR.BIAS)
    assert PR.center_voxel((-1e-10, 2.0, -3.0), 1.0) == (VR.BIAS - 1, VR.BIAS + 2, VR.BIAS - 3)
    for bad in (np.nan, np.inf, -np.inf, 3e38, float(2**20), -float(2**20) - 1):
        assert PR.center_voxel((0.0, bad, 0.0), 1.0) is None
    assert PR.center_voxel((0.0, float(2**20 - 1), -float(2**20 - 1)), 1.0) == (VR.BIAS, 2 * VR.BIAS - 1, 1)


# ---------------------------------------------------------------------------------- the ABI and the host arithmetic

def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_voxel_keep": hip_lib.VoxelKeep, "svo_voxel_prune_result": hip_lib.VoxelPruneResult}
    dtypes = {"svo_prune_info": hip_lib.PRUNE_INFO_DTYPE}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_]
    for name, dt in dtypes.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in dt.names]
    lines.append('  printf("enums %d %d %d %d %d %d\\n", SVO_PRUNE_OK, SVO_PRUNE_NO_MAP, SVO_PRUNE_NO_POSE, SVO_PRUNE_TOO_LARGE, '
                 'SVO_PRUNE_CENTER_GIVEN, SVO_PRUNE_CENTER_POSE);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_voxel_keep": 32, "svo_voxel_prune_result": 32, "svo_prune_info": 64}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f, _ in cls._fields_:
            assert c[f"{name}.{f}"] == [getattr(cls, f).offset], (name, f)
    for name, dt in dtypes.items():
        assert c[name] == [dt.itemsize] == [want[name]], name
        for f in dt.names:
            assert c[f"{name}.{f}"] == [dt.fields[f][1]], (name, f)
    assert c["enums"] == [hip_lib.PRUNE_OK, hip_lib.PRUNE_NO_MAP, hip_lib.PRUNE_NO_POSE, hip_lib.PRUNE_TOO_LARGE, hip_lib.PRUNE_CENTER_GIVEN,
                          hip_lib.PRUNE_CENTER_POSE] == [0, 1, 2, 3, 0, 1]
    lib = hip_lib.lib()
    for sym in ("svo_voxel_prune", "svo_submit_prune_voxel_maps", "svo_prune_voxel_maps"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)
    k = hip_lib.voxel_keep(3, 4, (1.5, -2.5, 0.25), 7)
    assert (k.min_count, k.min_stamp, list(k.center), k.radius, list(k._reserved)) == (3, 4, [1.5, -2.5, 0.25], 7, [0, 0])
    assert hip_lib.voxel_keep().radius < 0


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """the prune's host arithmetic as a program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("voxel_prune_plan")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "voxel_prune_plan_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", src]
    out = {"plain": str(d / "voxel_prune_plan_check"), "sanitized": str(d / "voxel_prune_plan_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_planner(planner, which):
    # centres given to the program (coordinate, voxel): the index it prints is the statement's, -1 for outside
    asks = [(0.0, 1.0), (-1e-10, 1.0), (2.0, 1.0), (-3.0, 1.0), (-7.3, 0.3), (0.51, 0.05), (1048575.5, 1.0), (1048576.0, 1.0),
            (-1048576.0, 1.0), (-1048577.0, 1.0), (3e38, 0.3), (float("nan"), 1.0), (float("inf"), 1.0), (52428.7, 0.05)]
    args = [x for c, v in asks for x in (repr(float(np.float32(c))), repr(float(np.float32(v))))]
    r = subprocess.run([planner[which]] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "voxel prune plan ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = [int(x) for x in r.stdout.split("centres:")[1].split("\n")[0].split()]
    want = []
    for c, v in asks:
        cv = PR.center_voxel((c, 0.0, 0.0), v)
        want.append(-1 if cv is None else cv[0])
    assert got == want and -1 in want and any(w > 0 for w in want)
