"""The voxel entries without a GPU: the algebra that gives pack, merge and rehash their meaning, asserted on the
statements of tests/voxel_entries_ref.py (vectorised and scalar, which must agree on every case); that the crafted cases
of tests/voxel_entries_cases.py reach what they claim to reach; the C ABI of the new structs; and the host arithmetic of
the entries (csrc/svo_voxel_plan.hpp) in a stand-alone program, plain and under the address and undefined-behaviour
sanitizers."""
import copy
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import voxel_cases as VC
import voxel_entries_cases as EC
import voxel_entries_ref as ER
import voxel_prune_ref as PR
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _map(case):
    m, = VR.run(case)
    return m


def _equal(a, b):
    return np.array_equal(a.keys, b.keys) and np.array_equal(a.acc, b.acc) and a.n_voxels == b.n_voxels


def _both(m, ent, voxel=None):
    """merge into the Map and into its scalar twin; they agree; returns the result"""
    s = ER.scalar_of(m)
    res = ER.merge(m, ent, m.voxel if voxel is None else voxel)
    assert ER.merge_scalar(s, ent, m.voxel if voxel is None else voxel) == res and ER.same(m, s)
    return res


MAPS = [("small_0", lambda: EC.small(0)), ("small_1", lambda: EC.small(1)), ("small_48", lambda: EC.small(48)), ("tiles", EC.tiles),
        ("chain", lambda: VC.case("chain")), ("runs", lambda: VC.case("runs"))]


@pytest.mark.parametrize("name,make", MAPS)
def test_merge_of_a_pack_into_an_empty_map_is_the_map(name, make):
    a = _map(make())
    packed = ER.pack(a)
    assert packed.tobytes() == ER.pack_scalar(ER.scalar_of(a)).tobytes() and len(packed) == a.n_voxels
    assert np.all(np.diff(packed["key"].astype(object)) > 0) if len(packed) > 1 else True
    for log2 in range(6, 13):
        empty = VR.Map(a.voxel, log2)
        if not ER.load_ok(empty, len(packed)):
            assert a.n_voxels > VR.load_limit(log2)
            continue
        res = _both(empty, packed)
        assert _equal(empty, a) and empty.n_fused == a.n_fused == int(a.acc[:, 0].sum())
        assert res == {"n_offered": a.n_voxels, "n_merged": a.n_voxels, "n_skipped": 0, "n_claimed": a.n_voxels}
        assert empty.extract().tobytes() == a.extract().tobytes() == ER.extract_of(packed, a.voxel).tobytes()


def test_fusing_the_union_is_merging_the_maps():
    r1, r2, params = EC.union()
    whole = VR.Map(*params)
    whole.fuse(np.concatenate([r1, r2]), 3)
    m1, m2 = VR.Map(*params), VR.Map(*params)
    m1.fuse(r1, 3)
    m2.fuse(r2, 3)
    assert set(m1.keys.tolist()) & set(m2.keys.tolist()) and set(m1.keys.tolist()) ^ set(m2.keys.tolist())   # overlapping, not identical
    assert ER.load_ok(m2, m1.n_voxels)
    n2 = m2.n_voxels
    res = _both(m2, ER.pack(m1))
    assert _equal(m2, whole) and m2.n_fused == whole.n_fused
    assert res == {"n_offered": m1.n_voxels, "n_merged": m1.n_voxels, "n_skipped": 0, "n_claimed": whole.n_voxels - n2} and 0 < res["n_claimed"] < m1.n_voxels
    assert ER.pack(m2).tobytes() == ER.pack(whole).tobytes() and m2.extract().tobytes() == whole.extract().tobytes()
    # different stamps: last is the max of both sides
    a, b = VR.Map(*params), VR.Map(*params)
    a.fuse(r1, 9)
    b.fuse(r2, 2)
    both = VR.Map(*params)
    both.fuse(r1, 9)
    both.fuse(r2, 2)
    _both(b, ER.pack(a))
    assert _equal(b, both)


def test_sums_and_a_count_that_wrap():
    have, span = EC.wrap_pair()
    m = ER.map_of(have, 0.3, 6)
    res = _both(m, span)
    assert res == {"n_offered": 4, "n_merged": 4, "n_skipped": 0, "n_claimed": 1} and m.n_voxels == 4
    got = {int(k): a.tolist() for k, a in zip(m.keys, m.acc)}
    k = [int(x) for x in span["key"]]
    top = 0xFFFFFFFF
    assert got[k[0]] == [1, 0x10, 0, 1, 0, top - 1, 0, 4]                     # every accumulator wrapped 2^32 (written down, not computed)
    assert got[k[1]] == [3, 11, 22, 33, 44, 55, 66, 5] and got[k[2]] == [3, 11, 22, 33, 44, 55, 66, 5]    # last: a max, both orders
    assert got[k[3]] == [3, 300, 200, 100, 9, 8, 7, 0]
    assert m.n_fused == 2 + 1 + 1 + 3
    # the packed bytes carry the wrapped values verbatim
    assert ER.pack(m)[np.searchsorted(m.keys, np.uint64(k[0]))]["acc"].tolist() == got[k[0]]


def test_merge_commutes_and_associates():
    r1, r2, params = EC.union()
    rec3 = VC.mixed(900, seed=23)[0]
    parts = []
    for rec, stamp in ((r1, 4), (r2, 2), (rec3, 7)):
        m = VR.Map(*params)
        m.fuse(rec, stamp)
        parts.append(m)
    results = []
    for order in itertools.permutations(range(3)):
        acc = VR.Map(*params)
        for i in order:
            assert ER.load_ok(acc, parts[i].n_voxels)
            _both(acc, ER.pack(parts[i]))
        results.append(acc)
    # (a + b) + c against a + (b + c)
    bc = copy.deepcopy(parts[1])
    ER.merge(bc, ER.pack(parts[2]), params[0])
    a_bc = copy.deepcopy(parts[0])
    ER.merge(a_bc, ER.pack(bc), params[0])
    results.append(a_bc)
    for r in results[1:]:
        assert _equal(r, results[0]) and r.n_fused == results[0].n_fused == sum(p.n_fused for p in parts)
    direct = VR.Map(*params)
    for rec, stamp in ((r1, 4), (r2, 2), (rec3, 7)):
        direct.fuse(rec, stamp)
    assert _equal(direct, results[0])


def test_skipped_records_change_nothing_but_n_skipped():
    ent, which = EC.skipped_span()
    sk = ER.skipped(ent)
    assert np.flatnonzero(sk).tolist() == list(which)
    assert int(ent[1]["key"]) >> 63 == 1 and int(ent[1]["key"]) != VR.EMPTY and int(ent[4]["key"]) == VR.EMPTY and ent[6]["acc"][0] == 0
    assert all(ent[i]["acc"][0] > 0 for i in (1, 4)) and int(ent[6]["key"]) >> 63 == 0           # one reason each
    base = _map(EC.tiles())
    only = copy.deepcopy(base)
    res = _both(only, ent[sk])
    assert res == {"n_offered": 3, "n_merged": 0, "n_skipped": 3, "n_claimed": 0}
    assert _equal(only, base) and (only.n_fused, only.n_outside) == (base.n_fused, base.n_outside)
    with_, without = copy.deepcopy(base), copy.deepcopy(base)
    r1, r2 = _both(with_, ent), _both(without, ent[~sk])
    assert _equal(with_, without) and with_.n_fused == without.n_fused == base.n_fused + int(ent["acc"][~sk, 0].sum())
    assert (r1["n_merged"], r1["n_skipped"], r1["n_claimed"]) == (5, 3, 5) and r2["n_skipped"] == 0


def test_n_fused_grows_by_the_merged_counts_and_the_edge_must_match():
    m = _map(EC.tiles())
    before = m.n_fused
    ent = EC.lattice_entries(100)
    assert ER.load_ok(m, 100)
    _both(m, ent)
    assert m.n_fused == before + int(ent["acc"][:, 0].sum()) and m.n_outside == 0
    other = np.nextafter(np.float32(m.voxel), np.float32(1.0))
    assert other != m.voxel and not ER.same_edge(other, m.voxel)
    snapshot = copy.deepcopy(m)
    for fn, target in ((ER.merge, m), (ER.merge_scalar, ER.scalar_of(m))):
        with pytest.raises(ValueError):
            fn(target, ent, other)
    assert _equal(m, snapshot)


def test_the_filters_two_edges():
    m = _map(EC.tiles())
    counts, lasts = set(m.acc[:, 0].tolist()), set(m.acc[:, 7].tolist())
    assert {1, 2, 3} <= counts and lasts == {1, 2, 3}
    for kw in (dict(min_count=2), dict(min_stamp=2), dict(min_count=3, min_stamp=3), dict(min_count=0), dict(min_count=1)):
        p = ER.pack(m, **kw)
        assert p.tobytes() == ER.pack_scalar(ER.scalar_of(m), **kw).tobytes()
        mc, ms = max(1, kw.get("min_count", 0)), kw.get("min_stamp", 0)
        assert (p["acc"][:, 0] >= mc).all() and (p["acc"][:, 7] >= ms).all()
        assert len(p) == int(((m.acc[:, 0] >= mc) & (m.acc[:, 7] >= ms)).sum())
        assert ER.extract_of(p, m.voxel).tobytes() == m.extract(**kw).tobytes()
    p2 = ER.pack(m, min_count=2)
    assert (p2["acc"][:, 0] == 2).any() and not (p2["acc"][:, 0] == 1).any() and (m.acc[:, 0] == 1).any()        # count == min_count, min_count - 1
    s2 = ER.pack(m, min_stamp=2)
    assert (s2["acc"][:, 7] == 2).any() and not (s2["acc"][:, 7] == 1).any() and (m.acc[:, 7] == 1).any()        # last == min_stamp, min_stamp - 1
    assert len(ER.pack(m, min_count=0)) == len(ER.pack(m, min_count=1)) == m.n_voxels


def test_rehash_keeps_entries_and_counters():
    for name, make in MAPS:
        m = _map(make())
        for log2 in (6, 7, 10, 12):
            out, outs = ER.rehash(m, log2), ER.rehash_scalar(ER.scalar_of(m), log2)
            if m.n_voxels > VR.load_limit(log2):
                assert out is None and outs is None
                continue
            assert out.log2_capacity == log2 and _equal(out, m) and (out.n_fused, out.n_outside) == (m.n_fused, m.n_outside)
            assert ER.same(out, outs) and ER.pack(out).tobytes() == ER.pack(m).tobytes()
    m = _map(EC.small(48))
    assert ER.rehash(m, 6) is not None and m.n_voxels == VR.load_limit(6)
    ER.merge(m, EC.lattice_entries(1, first=9000), 1.0)
    assert m.n_voxels == 49 and ER.rehash(m, 6) is None and ER.rehash(m, 7) is not None


def test_the_cases_reach_what_they_claim():
    log2 = EC.SMALL_LOG2
    keys = EC.small_keys()
    assert len(set(keys)) == 48 == EC.SMALL_LIMIT == VR.load_limit(log2)
    chain = keys[:VC.CHAIN_KEYS]
    assert {VR.home(k, log2) for k in chain} == {VC.CHAIN_HOME}
    table = PR.place(chain, log2)                                                    # one after the other from the home on
    at = [table.index(k) for k in chain]
    assert at == [(VC.CHAIN_HOME + i) % 64 for i in range(len(chain))] and 63 in at and 0 in at and at.index(0) == at.index(63) + 1
    # the same keys in another order of arrival, as a merge or rehash may place them: the chain still wraps, the entries differ
    other = PR.place(chain[::-1], log2)
    assert all(PR.lookup(other, k, log2) is not None for k in chain) and other[63] != VR.EMPTY and other[0] != VR.EMPTY
    assert other != table                                                            # so only the sorted pack can be compared
    # under 1024 entries the chain falls apart: the rehash finds new homes
    assert len({VR.home(k, 10) for k in chain}) > 1
    for n in (0, 1, 48):
        m = _map(EC.small(n))
        assert m.n_voxels == n and m.n_outside == 0
        for call in EC.small(n)["calls"]:
            assert len(call) == 1
    m = _map(EC.tiles())
    homes = [VR.home(k, EC.TILES_LOG2) for k in m.keys]
    assert any(h < 256 for h in homes) and any(h >= 256 for h in homes) and m.n_voxels > 128 and m.n_voxels <= VR.load_limit(EC.TILES_LOG2)
    assert m.n_voxels <= VR.load_limit(10) and m.n_voxels > VR.load_limit(6)
    # the repeated key: twice in one wavefront, once in the next, once in a second workgroup
    ent = EC.dup_span()
    same = np.flatnonzero(ent["key"] == ent[0]["key"]).tolist()
    assert same == list(EC.DUP_AT) and len(ent) == 257 and len(np.unique(ent["key"])) == 254
    waves = [(i // 256, i % 256 // 64) for i in same]
    assert waves == [(0, 0), (0, 0), (0, 1), (1, 0)]
    assert not ER.skipped(ent).any() and not ER.skipped(EC.lattice_entries(300)).any()
    assert len(np.unique(EC.lattice_entries(300)["key"])) == 300
    for n in EC.SPAN_SIZES:
        assert len(EC.lattice_entries(n)) == n
    assert set(EC.SPAN_SIZES) >= {0, 1, 255, 256, 257}


def test_repeated_keys_inside_a_span_and_across_spans():
    ent = EC.dup_span()
    m = VR.Map(0.3, 10)
    res = _both(m, ent)
    assert res == {"n_offered": 257, "n_merged": 257, "n_skipped": 0, "n_claimed": 254} and m.n_voxels == 254
    i = np.searchsorted(m.keys, ent[0]["key"])
    want = ent["acc"][list(EC.DUP_AT)].astype(np.uint64)
    assert m.acc[i, :7].tolist() == (want[:, :7].sum(axis=0) & VR.MASK32).tolist() and m.acc[i, 7] == want[:, 7].max()
    # the same records one by one, and in two spans
    one, two = VR.Map(0.3, 10), VR.Map(0.3, 10)
    for j in range(len(ent)):
        ER.merge(one, ent[j:j + 1], 0.3)
    ER.merge(two, ent[100:], 0.3)
    ER.merge(two, ent[:100], 0.3)
    assert _equal(one, m) and _equal(two, m)


# ---------------------------------------------------------------------------------- the ABI and the host arithmetic

def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_voxel_entry_span": hip_lib.VoxelEntrySpan, "svo_voxel_merge_result": hip_lib.VoxelMergeResult,
                 "svo_voxel_entry_dst": hip_lib.VoxelEntryDst}
    dtypes = {"svo_voxel_entry": hip_lib.VOXEL_ENTRY_DTYPE, "svo_voxel_load_info": hip_lib.VOXEL_LOAD_INFO_DTYPE}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_]
    for name, dt in dtypes.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in dt.names]
    lines.append('  printf("align %zu\\n", _Alignof(svo_voxel_entry));\n')
    lines.append('  printf("enums %d %d %d %d %d\\n", SVO_VOXEL_LOAD_REPLACE, SVO_VOXEL_LOAD_MERGE, SVO_VOXEL_LOADED, SVO_VOXEL_LOAD_NO_MAP, '
                 'SVO_VOXEL_LOAD_FULL);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_voxel_entry_span": 24, "svo_voxel_merge_result": 32, "svo_voxel_entry": 40, "svo_voxel_entry_dst": 16, "svo_voxel_load_info": 64}
    assert c["enums"] == [hip_lib.VOXEL_LOAD_REPLACE, hip_lib.VOXEL_LOAD_MERGE, hip_lib.VOXEL_LOADED, hip_lib.VOXEL_LOAD_NO_MAP,
                          hip_lib.VOXEL_LOAD_FULL] == [0, 1, 0, 1, 2]
    span = hip_lib.VOXEL_ENTRY_SPAN_DTYPE                                            # the spans of a load job travel as a numpy array
    assert span.itemsize == 24 and [span.fields[f][1] for f, _ in hip_lib.VoxelEntrySpan._fields_] == [getattr(hip_lib.VoxelEntrySpan, f).offset
                                                                                                       for f, _ in hip_lib.VoxelEntrySpan._fields_]
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f, _ in cls._fields_:
            assert c[f"{name}.{f}"] == [getattr(cls, f).offset], (name, f)
    for name, dt in dtypes.items():
        assert c[name] == [dt.itemsize] == [want[name]], name
        for f in dt.names:
            assert c[f"{name}.{f}"] == [dt.fields[f][1]], (name, f)
    assert c["align"] == [8] and hip_lib.VOXEL_ENTRY_DTYPE == ER.ENTRY
    lib = hip_lib.lib()
    for sym in ("svo_voxel_pack", "svo_voxel_merge", "svo_voxel_rehash", "svo_submit_save_voxel_maps", "svo_save_voxel_maps",
                "svo_submit_load_voxel_maps", "svo_load_voxel_maps", "svo_ctx_resize_voxel_maps"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """the entries' host arithmetic as a program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("voxel_entries_plan")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "voxel_entries_plan_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", src]
    out = {"plain": str(d / "voxel_entries_plan_check"), "sanitized": str(d / "voxel_entries_plan_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_planner(planner, which):
    r = subprocess.run([planner[which]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "voxel entries plan ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
