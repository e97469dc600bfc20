"""Crafted inputs of the prune (include/svo_hip.h, "voxel prune"). A case is a case of tests/voxel_cases.py with one map,
    {"maps": [(voxel, log2_capacity, drop_flags)], "calls": [[(records, 0, stamp)], ...], "keep": {...}}
and the keep rule (the keywords of voxel_prune_ref.keeps) that is applied after its calls. Every call holds one span,
and the chain cases fuse one record per call, so where their entries lie is the same in every run. Each case is there
for one thing a prune can get wrong; tests/test_voxel_prune_cpu.py checks that it does reach it. No case lets a probe
visit every entry: `overflow` stays 0."""
import numpy as np

import voxel_cases as VC
import voxel_ref as VR
import voxel_prune_ref as PR

F = np.float32
NAMES = ("chain_mid", "chain_wrap", "box", "box_negative", "box_face", "box_r0", "count_stamp", "min_count_0", "keep_all", "keep_none",
         "empty", "full", "mixed")
CHAIN_MID_KEYS, CHAIN_MID_LEAVES = 4, 1                  # entries 59 .. 62; the one at 60 leaves
CHAIN_WRAP_KEYS, CHAIN_WRAP_LEAVES = 8, (4, 5)           # entries 59 .. 63, 0, 1, 2; those at 63 and 0 leave
BOX_RADIUS = 2


def _one_per_call(cells, voxel, stamps, seed):
    rng = np.random.default_rng(seed)
    pts = VC._in_cell(cells, voxel, rng)
    return [[(VR.records(pts[i:i + 1], (i + 1, 2 * i + 1, 255 - i)), 0, int(s))] for i, s in enumerate(stamps)]


def _chain(n, leaves):
    """the first n keys of voxel_cases.chain_keys (one home, 59 of 64), one record and one call each, in this order;
    the entries named by `leaves` get stamp 1, the others stamp 5, and the rule keeps last >= 2"""
    keys = VC.chain_keys()[:n]
    cells = [(VR.key_parts(k)[0] - VR.BIAS, 0, 0) for k in keys]
    stamps = [1 if i in leaves else 5 for i in range(n)]
    return {"maps": [(1.0, VC.CHAIN_LOG2, 0)], "calls": _one_per_call(cells, 1.0, stamps, 31), "keep": dict(min_stamp=2)}


def chain_mid():
    return _chain(CHAIN_MID_KEYS, (CHAIN_MID_LEAVES,))


def chain_wrap():
    return _chain(CHAIN_WRAP_KEYS, CHAIN_WRAP_LEAVES)


def box_cells(c, r):
    """[(cell, inside)]: the centre cell, on each axis and side the cells r and r + 1 away, the corner (r, r, r) and
    its neighbours one step further out on each axis. The labels are written down here, not computed by the rule."""
    c = np.asarray(c, np.int64)
    out = [(tuple(c), True)]
    for a in range(3):
        e = np.eye(3, dtype=np.int64)[a]
        for side in (-1, 1):
            out.append((tuple(c + side * r * e), True))
            out.append((tuple(c + side * (r + 1) * e), False))
        out.append((tuple(c + r + e), False))               # past the corner on this axis
    out.append((tuple(c + r), True))
    out.append((tuple(c - r), True))
    seen, uniq = set(), []
    for cell, lab in out:                                    # (r = 0: the centre comes again as its own edge)
        if cell not in seen:
            seen.add(cell)
            uniq.append((cell, lab))
    return uniq


def _box(voxel, center, radius, seed, log2=8):
    c = np.array(PR.center_voxel(center, voxel), np.int64) - VR.BIAS
    cells = [cell for cell, _ in box_cells(c, radius)]
    rng = np.random.default_rng(seed)
    rec = VR.records(VC._in_cell(cells, voxel, rng))
    rec["color"] = rng.integers(0, 256, (len(rec), 3))
    return {"maps": [(voxel, log2, 0)], "calls": [[(rec, 0, 3)]], "keep": dict(center=tuple(float(F(x)) for x in center), radius=radius)}


def box():
    return _box(1.0, (3.5, 4.25, 5.75), BOX_RADIUS, 41)


def box_negative():
    return _box(0.3, (-7.3, -0.2, -100.9), BOX_RADIUS, 42)


def box_face():
    """a centre exactly on voxel faces: floorf puts it into the voxel above the face, on both sides of 0"""
    return _box(1.0, (2.0, -3.0, 0.0), BOX_RADIUS, 43)


def box_r0():
    return _box(0.05, (0.51, -0.27, 2.0), 0, 44)


def _count_stamp():
    """four voxels: (count, last) = (3, 5), (2, 5), (3, 4), (4, 6)"""
    rng = np.random.default_rng(45)
    def rec(cell, n):
        return VR.records(VC._in_cell([cell] * n, 0.3, rng), (20, 40, 60))
    a, b, c, d = (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)
    return [[(np.concatenate([rec(a, 2), rec(b, 1), rec(c, 3), rec(d, 3)]), 0, 4)], [(np.concatenate([rec(a, 1), rec(b, 1)]), 0, 5)],
            [(rec(d, 1), 0, 6)]]


def count_stamp():
    """count == min_count and min_count - 1, last == min_stamp and min_stamp - 1"""
    return {"maps": [(0.3, 6, 0)], "calls": _count_stamp(), "keep": dict(min_count=3, min_stamp=5)}


def min_count_0():
    return {"maps": [(0.3, 6, 0)], "calls": _count_stamp(), "keep": dict(min_count=0, min_stamp=5)}


def _mixed_calls():
    rec, params = VC.mixed()
    half = len(rec) // 2
    return params, [[(rec[:half], 0, 1)], [(rec[half:], 0, 2)]]


def keep_all():
    params, calls = _mixed_calls()
    return {"maps": [params], "calls": calls, "keep": dict(min_count=1, min_stamp=1, center=(0.0, 0.0, 0.0), radius=6)}


def keep_none():
    params, calls = _mixed_calls()
    return {"maps": [params], "calls": calls, "keep": dict(min_stamp=3)}


def empty():
    return {"maps": [(0.3, 10, 0)], "calls": [], "keep": dict(min_count=2, center=(1.0, 1.0, 1.0), radius=1)}


def full_cells():
    """96 distinct cells: the first 48 fill a map of 64 entries to its load limit, the others refill it"""
    return [(i % 8 - 4, i // 8 % 4, i // 32 - 1) for i in range(96)]


def full():
    """48 entries in 64, the load limit, fused as 24 with stamp 1 and 24 with stamp 2; half of them leave"""
    rng = np.random.default_rng(46)
    pts = VC._in_cell(full_cells()[:48], 0.3, rng)
    return {"maps": [(0.3, 6, 0)], "calls": [[(VR.records(pts[:24], (1, 2, 3)), 0, 1)], [(VR.records(pts[24:], (4, 5, 6)), 0, 2)]],
            "keep": dict(min_stamp=2)}


def mixed():
    """all three tests at once on a cloud with many records per voxel"""
    params, calls = _mixed_calls()
    return {"maps": [params], "calls": calls, "keep": dict(min_count=2, min_stamp=2, center=(0.1, 0.2, -0.3), radius=3)}


def case(name):
    return globals()[name]()


def records_of_keys(keys, voxel, color=(7, 7, 7)):
    """one record in the middle of the voxel of each key (the reachability fuse)"""
    cells = np.array([[p - VR.BIAS for p in VR.key_parts(k)] for k in keys], np.float64).reshape(-1, 3)
    rec = VR.records(((cells + 0.5) * float(F(voxel))).astype(F), color)
    _, inside, key, _ = VR.classify(rec, voxel, 0)
    assert inside.all() and np.array_equal(key, np.asarray(keys, np.uint64)), "a record left its voxel"
    return rec
