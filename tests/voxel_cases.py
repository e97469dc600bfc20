"""Crafted inputs of the voxel maps (include/svo_hip.h, "voxel maps"). A case is
    {"maps": [(voxel, log2_capacity, drop_flags)], "calls": [[(records, map index, stamp), ...], ...]}
with records of voxel_ref.POINT: every call is one svo_voxel_fuse. Each case is there for one thing the fuse kernel or
the rule can get wrong; tests/test_voxel_cpu.py checks that it does reach it."""
import numpy as np

import voxel_ref as VR

F = np.float32
NAMES = ("one", "runs", "chain", "edges_1.0", "edges_0.05", "edges_0.3", "flags", "pile", "spans")
RUN_LENGTHS = (1, 2, 3, 63, 64, 65)
CHAIN_HOME, CHAIN_KEYS, CHAIN_LOG2 = 64 - 5, 40, 6


def _in_cell(cells, voxel, rng, n=None):
    """points strictly inside the voxels with integer indices `cells` [n, 3] (offsets 0.1 .. 0.9 of the edge)"""
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    u = rng.uniform(0.1, 0.9, cells.shape)
    return ((cells + u) * float(F(voxel))).astype(F)


def one():
    return {"maps": [(0.05, 6, 0)], "calls": [[(VR.records([[0.51, -0.27, 2.0]], (10, 200, 31)), 0, 7)]]}


def runs():
    """equal-key runs of 1, 2, 3, 63, 64 and 65 records back to back (the long ones straddle lanes 63 | 64 of the
    record order), two single records, then sixteen records that alternate between two keys inside one wavefront"""
    rng = np.random.default_rng(11)
    cells = []
    for i, n in enumerate(RUN_LENGTHS):
        cells += [(i, -i, 2 * i)] * n
    cells += [(20, 0, 0), (21, 0, 0)]
    cells += [(30, 1, 1), (31, 1, 1)] * 8
    rec = VR.records(_in_cell(cells, 1.0, rng))
    rec["color"] = rng.integers(0, 256, (len(rec), 3))
    return {"maps": [(1.0, 10, 0)], "calls": [[(rec, 0, 3)]]}


def chain_keys():
    """CHAIN_KEYS keys (ix varies, iy = iz = 2^20) whose home in a 64-entry table is CHAIN_HOME, by brute force"""
    ix = np.arange(VR.BIAS - 4000, VR.BIAS + 4000, dtype=np.uint64)
    key = ix << np.uint64(42) | np.uint64(VR.BIAS) << np.uint64(21) | np.uint64(VR.BIAS)
    with np.errstate(over="ignore"):
        h = (key * np.uint64(VR.HASH)) >> np.uint64(64 - CHAIN_LOG2)
    found = key[h == CHAIN_HOME][:CHAIN_KEYS]
    assert len(found) == CHAIN_KEYS
    return found


def chain():
    """40 keys with one home 5 entries before the end of a 64-entry table: the probe chain wraps. A second call
    reaches the deepest entries again (40 + 8 = 48 records: exactly the load bound)."""
    rng = np.random.default_rng(12)
    cells = [(VR.key_parts(k)[0] - VR.BIAS, 0, 0) for k in chain_keys()]
    first = VR.records(_in_cell(cells, 1.0, rng), (9, 8, 7))
    again = VR.records(_in_cell(cells[::-1][:8], 1.0, rng), (100, 50, 25))
    return {"maps": [(1.0, CHAIN_LOG2, 0)], "calls": [[(first, 0, 1)], [(again, 0, 2)]]}


def edge_values(voxel):
    """[(value, label)] of one coordinate: label True = inside. The labels are written down here, not computed by the
    rule: with voxel 1.0 the values are exact; the others keep half a voxel from the border, four float32 steps at 2^20."""
    v = float(F(voxel))
    top = 2**20 - 1
    vals = [(F(k) * F(voxel), True) for k in range(-3, 4)]                         # on voxel faces
    vals += [(F(-0.0), True), (F(-1e-10), True), (F(1e-10), True), (F(-0.4 * v), True), (F(-2.6 * v), True)]
    vals += [(F((top + 0.5) * v), True), (F((top + 1.5) * v), False), (F((-top + 0.5) * v), True), (F((-top - 0.5) * v), False)]
    if voxel == 1.0:
        vals += [(F(top), True), (F(top + 1), False), (np.nextafter(F(top + 1), F(0)), True),
                 (F(-top), True), (np.nextafter(F(-top), F(-np.inf)), False), (F(-top - 1), False)]
    vals += [(F(np.nan), False), (F(np.inf), False), (F(-np.inf), False), (F(3e38), False), (F(-3e38), False)]
    return vals


def edges(voxel):
    """every edge value in each coordinate in turn, the other two at a quarter voxel; one record per value and axis"""
    vals = edge_values(voxel)
    quarter = F(0.25) * F(voxel)
    xyz = np.full((3 * len(vals), 3), quarter, F)
    for a in range(3):
        for i, (v, _) in enumerate(vals):
            xyz[a * len(vals) + i, a] = v
    rec = VR.records(xyz)
    rec["color"] = (np.arange(len(rec))[:, None] * (3, 5, 7) % 256)
    return {"maps": [(voxel, 10, 0)], "calls": [[(rec, 0, 1)]]}


def flags():
    """records that carry SVO_CLOUD_DROPPED, each SVO_IGNORE_* bit, combinations and none, into four maps: one that
    drops no flag and one per drop_flags bit"""
    rng = np.random.default_rng(13)
    fl = np.array([0, VR.DROPPED, 1, 2, 4, 3, 6, 7, VR.DROPPED | 1, 0], np.uint8)
    rec = VR.records(_in_cell(rng.integers(-2, 3, (len(fl) * 6, 3)), 0.3, rng))
    rec["flags"] = np.tile(fl, 6)
    rec["color"] = rng.integers(0, 256, (len(rec), 3))
    return {"maps": [(0.3, 8, d) for d in (0, 1, 2, 4)], "calls": [[(rec, m, 5) for m in range(4)]]}


def pile():
    """70 000 records in one voxel, each with the largest offsets; the colours 255, 0 and 128"""
    n = 70000
    xyz = np.tile(np.array([[F(2.999), F(-0.001), F(0.999)]], F), (n, 1))
    return {"maps": [(1.0, 17, 0)], "calls": [[(VR.records(xyz, (255, 0, 128)), 0, 9)]]}


def spans():
    """five spans into three maps (log2_capacity 6, 10, 12) in one call, one of them empty, five stamps; spans 0 and
    3 share map 0 and some of its voxels"""
    rng = np.random.default_rng(14)
    def cloud(n, lo, hi, voxel):
        r = VR.records(_in_cell(rng.integers(lo, hi, (n, 3)), voxel, rng))
        r["color"] = rng.integers(0, 256, (n, 3))
        return r
    return {"maps": [(0.05, 6, 0), (0.3, 10, 0), (1.0, 12, 0)],
            "calls": [[(cloud(20, -1, 1, 0.05), 0, 4), (cloud(300, -3, 3, 0.3), 1, 9), (cloud(0, 0, 1, 1.0), 2, 100),
                       (cloud(25, -2, 2, 0.05), 0, 2), (cloud(700, -6, 6, 1.0), 2, 1)]]}


def case(name):
    if name.startswith("edges_"):
        return edges(float(name.split("_")[1]))
    return globals()[name]()


def mixed(n=3000, seed=21):
    """a cloud with many records per voxel (for the order tests): records, params"""
    rng = np.random.default_rng(seed)
    rec = VR.records(rng.uniform(-1.5, 1.5, (n, 3)).astype(F))
    rec["color"] = rng.integers(0, 256, (n, 3))
    rec["flags"][rng.random(n) < 0.05] = VR.DROPPED
    return rec, (0.3, 12, 0)
