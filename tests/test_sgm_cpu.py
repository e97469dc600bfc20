"""Semi-global aggregation without a GPU: the numpy statement (tests/sgm_ref.py) is tied to dense_ref's point rule and
to a second, vectorised formulation; the ABI's layouts and symbols; and every crafted case of tests/sgm_cases.py
asserts that it reaches what it is for. No comparison has a tolerance."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dense_ref as DR
import sgm_cases as SC
import sgm_ref as SR
from stereo_svo_slam_amd import hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _points(name):
    """the lattice points of a pair that the loop statement visits (every point; of the wide pair a sample that holds
    both edges and the tile boundary)"""
    left, right, win, sx, sy, step = SC.pairs()[name][:6]
    cols, rows, xs, ys = DR.lattice(left.shape[1], left.shape[0], step)
    if name not in SC.SLOW:
        return [(ix, iy) for iy in range(rows) for ix in range(cols)]
    pick = sorted(set(range(0, cols, 17)) | set(range(240, 262)) | set(range(cols - 12, cols)))
    return [(ix, iy) for iy in (0, rows // 2, rows - 1) for ix in pick]


@pytest.mark.parametrize("name", sorted(SC.pairs()))
def test_raw_minimum_is_dense_refs_best_and_volume_follows(name):
    """float32(min over j of the raw minimum) is dense_ref.point's best; the volume's entries are the raw minima divided
    and capped; both formulations give the same volume"""
    left, right, win, sx, sy, step, p1, p2, cap = SC.pairs()[name]
    cols, rows, xs, ys = DR.lattice(left.shape[1], left.shape[0], step)
    C_, count = SC.pair_volume(name)
    for ix, iy in _points(name):
        raw, area = SR.raw_minimum(left, right, int(xs[ix]), int(ys[iy]), win, sx, sy)
        d, best = DR.point(left, right, int(xs[ix]), int(ys[iy]), win, sx, sy)
        if raw is None:
            assert (d, best) == (-1.0, -1.0) and count[iy, ix] == 0 and not C_[iy, ix].any()
            continue
        assert F(int(raw.min())) == F(best) and count[iy, ix] == len(raw) <= sx + 1
        assert np.array_equal(C_[iy, ix, :len(raw)], np.minimum(cap, raw // area)) and (C_[iy, ix, len(raw):] == cap).all()
    fast = SR.cost_volume_fast(left, right, win, sx, sy, step, cap)
    assert np.array_equal(fast[0], C_) and np.array_equal(fast[1], count)


@pytest.mark.parametrize("name", sorted(SC.pairs()))
def test_pair_paths_in_two_formulations(name):
    left, right, win, sx, sy, step, p1, p2, cap = SC.pairs()[name]
    C_ = SC.pair_volume(name)[0].astype(np.int64)
    S = SC.pair_sums(name)
    if name in SC.SLOW:                                     # the loop statement on a part: the first and last 70 columns
        for part in (C_[:, :70], C_[:, -70:]):
            assert np.array_equal(SR.sums(part, p1, p2), SR.sums_fast(part, p1, p2))
    else:
        assert np.array_equal(S, SR.sums_fast(C_, p1, p2))
    assert S.max() <= 4 * (cap + p2) <= 65535 and S.min() >= 0


@pytest.mark.parametrize("name", sorted(SC.volumes()))
def test_volume_paths_in_two_formulations(name):
    C_, count, p1, p2, cap = SC.volumes()[name]
    assert np.array_equal(SC.volume_sums(name), SR.sums_fast(np.minimum(C_.astype(np.int64), cap), p1, p2))
    for r in SR.DIRECTIONS:
        assert SR.path(C_.astype(np.int64), r, p1, p2).max() <= cap + p2


def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_sgm_params": hip_lib.SgmParams, "svo_sgm_shape": hip_lib.SgmShape}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_sgm_params": 32, "svo_sgm_shape": 16}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name]], name
        for f in cls._fields_:
            assert c[f"{name}.{f[0]}"] == [getattr(cls, f[0]).offset], (name, f[0])
    p = hip_lib.sgm_params(**hip_lib.SGM_DEFAULTS)
    with open(os.path.join(ROOT, "profiles", "sgm_defaults.json")) as f:
        choice = json.load(f)["choice"]                     # (tools/sgm_sweep.py's)
    assert hip_lib.SGM_DEFAULTS == choice
    assert (p.paths, p.p1, p.p2, p.cost_cap, p.subpixel, list(p._reserved)) == (4, choice["p1"], choice["p2"], choice["cost_cap"], 1, [0, 0, 0])
    assert 4 * (p.cost_cap + p.p2) <= 65535
    lib = hip_lib.lib()
    for sym in ("svo_dense_cost_volume", "svo_sgm_aggregate", "svo_dense_disparity_sgm"):
        assert sym in hip_lib.SYMBOLS
        getattr(lib, sym)


def _winners(S, count, D):
    n = np.minimum(count.astype(np.int64), D)
    j0 = np.array([[int(np.argmin(S[iy, ix, :max(n[iy, ix], 1)])) for ix in range(S.shape[1])] for iy in range(S.shape[0])])
    return n, j0


def test_pairs_reach_what_they_are_for():
    P = SC.pairs()
    seen = {k: False for k in ("count<D", "count=1", "invalid inside a path", "j0=0", "j0=count-1", "clamped", "at cap", "parabola")}
    for name in P:
        left, right, win, sx, sy, step, p1, p2, cap = P[name]
        D = sx + 1
        C_, count = SC.pair_volume(name)
        S = SC.pair_sums(name)
        n, j0 = _winners(S, count, D)
        ref = SC.pair_reference(name)
        valid = n > 0
        assert np.array_equal(ref[0] < 0, ~valid) and np.array_equal(ref[1] < 0, ~valid)
        seen["count<D"] |= bool(((n > 0) & (n < D)).any())
        seen["count=1"] |= bool((n[:, -1] == 1).any())
        inner = ~valid[1:-1, :] if valid.shape[0] > 2 else np.zeros((0, 1), bool)
        seen["invalid inside a path"] |= bool(inner.any() and valid[0].any() and valid[-1].any())
        seen["j0=0"] |= bool((valid & (j0 == 0)).any())
        seen["j0=count-1"] |= bool((valid & (n > 1) & (j0 == n - 1)).any())
        seen["clamped"] |= bool((ref[0][valid] == F(0.5)).any())
        seen["at cap"] |= bool((C_[valid] == cap).any())
        seen["parabola"] |= bool((ref[0][valid] != np.floor(ref[0][valid])).any())
    assert all(seen.values()), seen
    # what single cases are for
    assert (SC.pair_volume("f")[1][4:16] == 0).all() and (SC.pair_volume("f")[1][16:] > 0).all()      # invalid rows inside the columns
    assert (SC.pair_volume("e")[0] == 16000).all()                                                   # the cap bites everywhere
    for name in ("e", "e2"):                       # raw sums beyond float's 24 bits; in e2 also where the cap does not bite
        left, right, win, sx, sy, step, p1, p2, cap = P[name]
        cols, rows, xs, ys = DR.lattice(left.shape[1], left.shape[0], step)
        C_ = SC.pair_volume(name)[0]
        exact, top = 0, 0
        for iy in range(rows):
            for ix in range(cols):
                raw, area = SR.raw_minimum(left, right, int(xs[ix]), int(ys[iy]), win, sx, sy)
                odd = (raw > 1 << 24) & (raw % 2 == 1) & (raw // area < cap)   # (an odd integer above 2^24 is no float)
                exact += int(odd.sum())
                top = max(top, int(raw.max()))
                assert np.array_equal(C_[iy, ix, :len(raw)][odd], (raw // area)[odd])
        assert cap + p2 == 16383 and top > 1 << 24 and (name == "e" or exact > 0)
    assert SC.pair_volume("wide")[0].shape == (24, 300, 64) and SC.pair_sums("e2").max() > 60000


def test_flat_band_carries_the_purpose():
    left, right, win, sx, sy, step, p1, p2, cap = SC.pairs()["band"]
    assert (win, sx, sy, p1, p2, cap) == (7, 15, 1, 32, 256, 4095)
    wta = SC.band_score(DR.planes(left, right, win, sx, sy, step)[0])
    sgm = SC.band_score(SC.pair_reference("band")[0])
    print("flat band: winner takes all", wta, "sgm", sgm)
    assert wta <= 0.5
    assert sgm >= 0.95


def test_volumes_reach_what_they_are_for():
    V = SC.volumes()
    # ties of S go to the lower j, and a parabola offset of exactly + 0.5
    C_, count, p1, p2, cap = V["tie"]
    S = SC.volume_sums("tie")[0, 0]
    assert list(S) == [20, 12, 12, 28]
    ref = SC.volume_reference("tie")
    assert ref[0, 0, 0] == F(1.5) and ref[1, 0, 0] == F(12) and SC.volume_reference("tie", False)[0, 0, 0] == F(1.0)
    S5 = SC.volume_sums("5x7x3")
    n, j0 = _winners(S5, V["5x7x3"][1], 3)
    ties = [(iy, ix) for iy in range(7) for ix in range(5) if n[iy, ix] > 1 and (S5[iy, ix, :n[iy, ix]] == S5[iy, ix, j0[iy, ix]]).sum() > 1]
    assert ties and all(j0[t] == np.flatnonzero(S5[t][:n[t]] == S5[t][:n[t]].min())[0] for t in ties)
    assert SC.volume_reference("1x1x1")[0, 0, 0] == F(0.5)                  # j0 = 0: clamped
    # the random volumes: every argument of the inner min wins somewhere, S above 60 000
    for name in ("3x70x64", "70x3x64"):
        C_, count, p1, p2, cap = V[name]
        assert cap + p2 == 16383 and SC.volume_sums(name).max() > 60000
        assert (count == 0).any() and (count == 1).any() and (count == 64).any()
    won = np.zeros(4, bool)
    for name in ("3x70x64", "70x3x64", "9x9x33"):
        C_, count, p1, p2, cap = V[name]
        Ci = C_.astype(np.int64)
        rows, cols, D = Ci.shape
        for dx, dy in SR.DIRECTIONS:
            L = SR.path(Ci, (dx, dy), p1, p2)
            for iy in range(rows):
                for ix in range(cols):
                    py, px = iy - dy, ix - dx
                    if not (0 <= py < rows and 0 <= px < cols):
                        continue
                    Pv = L[py, px]
                    big = np.int64(1) << 40
                    args = np.stack([Pv, np.concatenate([[big], Pv[:-1]]) + p1, np.concatenate([Pv[1:], [big]]) + p1, np.full(D, Pv.min() + p2)])
                    least = args.min(0)
                    for a in range(4):
                        won[a] |= bool(((args[a] == least) & ((args == least).sum(0) == 1)).any())
    assert won.all(), won
    assert SC.volume_reference("9x9x33", counts=False).min() >= 0              # without a count plane every point is valid
