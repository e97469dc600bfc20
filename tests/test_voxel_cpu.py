"""Voxel maps without a GPU: the two statements of tests/voxel_ref.py agree on every crafted case and do not depend
on the order of the records, every case of tests/voxel_cases.py reaches what it is there for, the C ABI of the
structs and svo_voxel_map_bytes, and the host arithmetic (csrc/svo_voxel_plan.hpp) in a stand-alone program, plain
and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import voxel_cases as VC
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _same(a, b):
    assert (a.n_voxels, a.n_fused, a.n_outside) == (b.n_voxels, b.n_fused, b.n_outside)
    for kw in (dict(), dict(min_count=2), dict(min_stamp=3), dict(min_count=3, min_stamp=2)):
        assert a.extract(**kw).tobytes() == b.extract(**kw).tobytes(), kw


@pytest.mark.parametrize("name", VC.NAMES)
def test_the_two_statements_agree(name):
    case = VC.case(name)
    if name == "pile":                                       # the scalar statement on 70 000 records: a tenth, thrice over
        case = dict(case, calls=[[(r[:7000], m, s) for r, m, s in call] for call in case["calls"]] * 3)
    vec, sca = VR.run(case), VR.run(case, VR.ScalarMap)
    assert len(vec) == len(case["maps"])
    for a, b in zip(vec, sca):
        _same(a, b)
        assert sorted(b.entries) == a.keys.tolist()
        assert np.array_equal(np.array([b.entries[k] for k in sorted(b.entries)], np.uint64).reshape(-1, 8), a.acc)


def test_the_statement_does_not_depend_on_the_order():
    rec, params = VC.mixed()
    rng = np.random.default_rng(3)
    want = VR.Map(*params)
    want.fuse(rec, 4)
    assert want.n_voxels < len(rec) / 3 and int(want.acc[:, 0].max()) >= 5          # many records per voxel
    for order in (np.arange(len(rec))[::-1], rng.permutation(len(rec))):
        m = VR.Map(*params)
        m.fuse(rec[order], 4)
        _same(want, m)
    m = VR.Map(*params)
    for part in np.array_split(rec, 3):
        m.fuse(part, 4)
    _same(want, m)


# ---------------------------------------------------------------------------------- the cases reach what they are there for

def test_case_one_and_pile():
    m, = VR.run(VC.case("one"))
    assert (m.n_voxels, m.n_fused, m.n_outside) == (1, 1, 0)
    out = m.extract()
    assert out["color"].tolist() == [[10, 200, 31]] and out["flags"].tolist() == [0]
    assert abs(out["x"][0] - 0.51) < 0.05 / 256 and abs(out["y"][0] + 0.27) < 0.05 / 256 and abs(out["z"][0] - 2.0) <= 0.05 / 256
    m, = VR.run(VC.case("pile"))
    assert (m.n_voxels, m.n_fused) == (1, 70000) and m.acc[0].tolist() == [70000, 70000 * 255, 70000 * 255, 70000 * 255,
                                                                            70000 * 255, 0, 70000 * 128, 9]
    assert m.extract()["color"].tolist() == [[255, 0, 128]]
    assert 70000 > VR.load_limit(16) and 70000 <= VR.load_limit(17)                   # the smallest table that admits it


def test_case_runs():
    case = VC.case("runs")
    rec, = [r for r, _, _ in case["calls"][0]]
    _, inside, key, _ = VR.classify(rec, 1.0, 0)
    assert inside.all()
    lengths, start = [], 0
    for i in range(1, len(key) + 1):
        if i == len(key) or key[i] != key[start]:
            lengths.append((start, i - start))
            start = i
    assert tuple(n for _, n in lengths[:6]) == VC.RUN_LENGTHS and sum(VC.RUN_LENGTHS) + 2 == 200
    for s, n in lengths[3:6]:                                 # the three long runs cross a wavefront boundary
        assert s // 64 != (s + n - 1) // 64
    assert [n for _, n in lengths[6:8]] == [1, 1]
    tail = key[200:]
    assert len(tail) == 16 and 200 // 64 == 215 // 64          # one wavefront
    assert len(set(tail.tolist())) == 2 and all(tail[i] != tail[i + 1] for i in range(15)) and (tail[::2] == tail[0]).all()
    m, = VR.run(case)
    assert sorted(m.acc[:, 0].tolist()) == sorted(list(VC.RUN_LENGTHS) + [1, 1, 8, 8])


def test_case_chain():
    keys = VC.chain_keys()
    assert len(set(keys.tolist())) == VC.CHAIN_KEYS == 40
    assert {VR.home(k, VC.CHAIN_LOG2) for k in keys} == {VC.CHAIN_HOME} == {59}
    assert VC.CHAIN_HOME + VC.CHAIN_KEYS > 64                                         # the chain wraps past the table's end
    case = VC.case("chain")
    m, = VR.run(case)
    assert sorted(m.keys.tolist()) == sorted(keys.tolist()) and m.n_fused == 48 == VR.load_limit(VC.CHAIN_LOG2)
    assert sorted(m.acc[:, 0].tolist()) == [1] * 32 + [2] * 8 and sorted(m.acc[:, 7].tolist()) == [1] * 32 + [2] * 8


@pytest.mark.parametrize("voxel", [1.0, 0.05, 0.3])
def test_case_edges(voxel):
    vals = VC.edge_values(voxel)
    assert {lab for _, lab in vals} == {True, False}
    for v, label in vals:
        got = VR.scalar_key(v, F(0.25) * F(voxel), F(0.25) * F(voxel), voxel)
        assert (got is not None) == label, (v, label)
    if voxel == 1.0:
        top = 2**20 - 1
        assert VR.key_parts(VR.scalar_key(F(top), 0, 0, 1.0)[0])[0] == 2**21 - 1
        assert VR.key_parts(VR.scalar_key(F(-top), 0, 0, 1.0)[0])[0] == 1
    key, offs = VR.scalar_key(F(-1e-10), F(-0.0), F(0.0), voxel)
    assert VR.key_parts(key) == (VR.BIAS - 1, VR.BIAS, VR.BIAS) and offs == (255, 0, 0)    # the offset clamp; -0.0 is voxel 0
    case = VC.case(f"edges_{voxel}")
    m, = VR.run(case)
    n_out = sum(not lab for _, lab in vals)
    assert m.n_outside == 3 * n_out and m.n_fused == 3 * (len(vals) - n_out)


def test_case_flags_and_spans():
    case = VC.case("flags")
    rec = case["calls"][0][0][0]
    fused = [m.n_fused for m in VR.run(case)]
    assert fused == [int(((rec["flags"] & (VR.DROPPED | d)) == 0).sum()) for d in (0, 1, 2, 4)]
    assert len(set(fused)) >= 3 and all(0 < f < len(rec) for f in fused) and all(m.n_outside == 0 for m in VR.run(case))
    case = VC.case("spans")
    call, = case["calls"]
    assert len(call) == 5 and sorted({m for _, m, _ in call}) == [0, 1, 2] and [len(r) for r, _, _ in call].count(0) == 1
    assert len({s for _, _, s in call}) == 5 and [m[1] for m in case["maps"]] == [6, 10, 12]
    maps = VR.run(case)
    assert all(m.n_voxels > 0 for m in maps) and set(maps[0].acc[:, 7].tolist()) == {2, 4}
    assert 100 not in maps[2].acc[:, 7].tolist()


# ---------------------------------------------------------------------------------- the ABI and the host arithmetic

def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_voxel_params": hip_lib.VoxelParams, "svo_voxel_map": hip_lib.VoxelMap, "svo_voxel_span": hip_lib.VoxelSpan,
                 "svo_voxel_map_info": hip_lib.VoxelMapInfo, "svo_voxel_filter": hip_lib.VoxelFilter}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in cls._fields_]
    lines.append('  printf("enums %d %d\\n", SVO_CLOUD_DROPPED, (int)(SVO_IGNORE_DURING_REFINEMENT | SVO_IGNORE_COMPLETELY | SVO_IGNORE_TEMPORARY));\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_voxel_params": 16, "svo_voxel_map": 24, "svo_voxel_span": 24, "svo_voxel_map_info": 48, "svo_voxel_filter": 16}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f in cls._fields_:
            assert c[f"{name}.{f[0]}"] == [getattr(cls, f[0]).offset], (name, f[0])
    assert c["enums"] == [VR.DROPPED, VR.IGNORE_DURING_REFINEMENT | VR.IGNORE_COMPLETELY | VR.IGNORE_TEMPORARY]
    assert VR.POINT == hip_lib.MAP_POINT_DTYPE
    lib = hip_lib.lib()
    for sym in ("svo_voxel_map_bytes", "svo_voxel_clear", "svo_voxel_fuse", "svo_voxel_info", "svo_voxel_extract"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def test_ctx_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    dtypes = {"svo_fuse_info": hip_lib.FUSE_INFO_DTYPE, "svo_voxel_region": hip_lib.VOXEL_REGION_DTYPE,
              "svo_voxel_segment": hip_lib.VOXEL_SEGMENT_DTYPE}
    lines = ['  printf("svo_voxel_dst %zu %zu %zu\\n", sizeof(svo_voxel_dst), offsetof(svo_voxel_dst, segments), offsetof(svo_voxel_dst, points));\n',
             '  printf("enums %d %d %d %d %d %d %d\\n", SVO_FUSE_OK, SVO_FUSE_NONE, SVO_FUSE_NO_MAP, SVO_FUSE_FULL, SVO_VOXEL_OK, SVO_VOXEL_NO_MAP, '
             'SVO_VOXEL_TOO_SMALL);\n']
    for name, dt in dtypes.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_fuse_info": 64, "svo_voxel_region": 32, "svo_voxel_segment": 64}
    for name, dt in dtypes.items():
        assert c[name] == [dt.itemsize] == [want[name]], name
        for f in dt.names:
            assert c[f"{name}.{f}"] == [dt.fields[f][1]], (name, f)
    assert c["svo_voxel_dst"] == [C.sizeof(hip_lib.VoxelDst), hip_lib.VoxelDst.segments.offset, hip_lib.VoxelDst.points.offset] == [16, 0, 8]
    assert c["enums"] == [hip_lib.FUSE_OK, hip_lib.FUSE_NONE, hip_lib.FUSE_NO_MAP, hip_lib.FUSE_FULL, hip_lib.VOXEL_OK, hip_lib.VOXEL_NO_MAP,
                          hip_lib.VOXEL_TOO_SMALL] == [0, 1, 2, 3, 0, 1, 2]
    lib = hip_lib.lib()
    for sym in ("svo_ctx_set_voxel_maps", "svo_get_voxel_map_info", "svo_submit_fuse_clouds", "svo_fuse_clouds", "svo_submit_export_voxel_maps",
                "svo_export_voxel_maps", "svo_submit_clear_voxel_maps"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def test_map_bytes_through_the_abi():
    for log2 in range(6, 27):
        assert hip_lib.voxel_map_bytes(log2) == VR.map_bytes(log2) == 256 + 40 * 2**log2
    lib = hip_lib.lib()
    for bad in (-1, 0, 5, 27, 64):
        assert lib.svo_voxel_map_bytes(bad) == 0
        with pytest.raises(hip_lib.SvoError):
            hip_lib.voxel_map_bytes(bad)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """the host arithmetic's program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("voxel_plan")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "voxel_plan_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", src]
    out = {"plain": str(d / "voxel_plan_check"), "sanitized": str(d / "voxel_plan_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_planner(planner, which):
    keys = [1, 2**42, VR.EMPTY - 1] + [int(k) for k in VC.chain_keys()[:4]]
    r = subprocess.run([planner[which]] + [str(k) for k in keys], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "voxel plan ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    # the homes of the keys given to it (in a table of 64 and one of 2^26 entries), as the header computes them
    homes = [int(x) for x in r.stdout.split("homes:")[1].split("\n")[0].split()]
    assert homes == [VR.home(k, log2) for k in keys for log2 in (6, 26)]
