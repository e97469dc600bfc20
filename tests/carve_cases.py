"""Crafted inputs of the carve (include/svo_hip.h, "voxel carve"). A case is a case of tests/voxel_cases.py with one map
and what a carve takes besides it:
    {"maps": [(voxel, log2_capacity, drop_flags)], "calls": [[(records, 0, stamp)], ...], "cam": float32 [16],
     "size": (W, H), "lattice": None | (records, cols, rows, step), "rule": carve_ref.carve_rule(...), "keep": None | {...},
     "marks": {name: key}}
`marks` names the entries a case was built for, so that tests/test_carve_cpu.py can ask the reference where each of them
left the rule. Every number is dyadic: the voxel edge is 0.25, an entry is fused from two records whose sub-voxel
offsets add up to what puts its extracted coordinate on a multiple of 2^-11, the camera looks down +z from z = 0.125
with fx = fy = 16 and the principal point in the middle of a 50 x 30 image, and the entries sit at c_2 = 0.25, 0.5, 2 or
4, so every u, v and every tie below is exact in float32. The lattice is 12 x 7 at step 4 (the step does not divide
the size: columns 48, 49 and rows 28, 29 have no cell) or 10 x 6 at step 5 (it does)."""
import numpy as np

import carve_ref as CR
import voxel_cases as VC
import voxel_ref as VR

F = np.float32
VOXEL = 0.25
W, H = 50, 30
FX = FY = 16.0
CX, CY = 25.0, 15.0
EYE_Z = 0.125                                              # c_2 = w_2 - EYE_Z
NAMES = ("bounds", "bounds_step5", "not_finite", "compare", "clip_ring0", "clip_ring1", "bad_ring0", "bad_ring1", "rim_ring0", "rim_ring1",
         "chain", "both_reject", "none_carved", "all_carved", "empty", "null_occluder")


def camera():
    """identity rotation, the eye at (0, 0, EYE_Z)"""
    view = np.zeros(12, F)
    view[0] = view[5] = view[10] = 1
    view[11] = -EYE_Z
    return np.concatenate([view, np.asarray([FX, FY, CX, CY], F)])


def _split(coord):
    """(cell, n): coord = (cell + n / 512) * VOXEL with n in 1 .. 511"""
    val = coord / VOXEL
    cell = int(np.floor(val))
    n = (val - cell) * 512
    assert n == int(n) and 1 <= n <= 511, coord
    return cell, int(n)


def entry(x, y, z, color=(10, 20, 30)):
    """two records of one voxel whose entry extracts to exactly (x, y, z): per axis the two sub-voxel offsets add up
    to n - 1, so that (mean + 0.5) / 256 = n / 512"""
    rec = np.zeros((2, 3))
    key = 0
    for j, c in enumerate((x, y, z)):
        cell, n = _split(c)
        o = ((n - 1) // 2, n - 1 - (n - 1) // 2)
        for i in range(2):
            rec[i, j] = (cell + (o[i] + 0.25) / 256) * VOXEL
        key = key << 21 | (cell + VR.BIAS)
    return VR.records(rec, color), key


def at_pixel(u, v, c2=2.0, **kw):
    """the entry that the camera sees at exactly (u, v), c_2 away"""
    return entry((u - CX) * c2 / FX, (v - CY) * c2 / FY, c2 + EYE_Z, **kw)


def lattice(cols=12, rows=7, step=4, z=4.0):
    rec = VR.records(np.zeros((cols * rows, 3)))
    rec["z"] = F(z)
    return [rec, cols, rows, step]


def cell_centre(ix, iy, step=4):
    return ix * step + step / 2 + 0.5, iy * step + step / 2 + 0.5     # a pixel centre inside the cell (step 4: the third pixel)


def _case(entries, lat, rule, keep=None, cam=None, log2=8):
    """entries: [(name, (records, key), stamp)]; one call per stamp, in the order given"""
    calls, marks = [], {}
    for name, (rec, key), stamp in entries:
        calls.append([(rec, 0, stamp)])
        assert key not in marks.values(), name
        marks[name] = key
    return {"maps": [(VOXEL, log2, 0)], "calls": calls, "cam": camera() if cam is None else cam, "size": (W, H),
            "lattice": None if lat is None else tuple(lat), "rule": rule, "keep": keep, "marks": marks}


def _bounds_entries():
    """(the entries' coordinates are multiples of 2^-11, so at c_2 = 2 the u and v nearest a border are 2^-8 from it)"""
    return [("late", at_pixel(20.5, 10.5), 5),                           # last > max_last, in front of the wall
            ("last_eq", at_pixel(24.5, 10.5), 3),                        # last == max_last: a candidate
            ("near_lt", at_pixel(33.0, 23.0, 0.25), 1), ("near_eq", at_pixel(29.0, 19.0, 0.5), 1),
            ("u_0", at_pixel(0.0, 12.5), 1), ("u_neg", at_pixel(-2.0 ** -8, 13.5), 1),
            ("u_lt_w", at_pixel(W - 2.0 ** -8, 14.5), 1), ("u_w", at_pixel(float(W), 16.5), 1),
            ("v_0", at_pixel(10.5, 0.0), 1), ("v_neg", at_pixel(11.5, -2.0 ** -8), 1),
            ("v_lt_h", at_pixel(12.5, H - 2.0 ** -8), 1), ("v_h", at_pixel(13.5, float(H)), 1),
            ("beyond_cols", at_pixel(48.5, 6.5), 1), ("beyond_rows", at_pixel(6.5, 28.5), 1),
            ("last_col", at_pixel(47.5, 8.5), 1), ("last_row", at_pixel(8.5, 27.5), 1)]


def bounds():
    """the candidate test, the near plane, the image's four borders and the lattice's far edges, at step 4"""
    return _case(_bounds_entries(), lattice(), CR.carve_rule(0.25, near=0.5, ring=1, max_last=3))


def bounds_step5():
    """the same entries under a lattice that covers the image: the last pixel column and row have a cell"""
    return _case(_bounds_entries(), lattice(10, 6, 5), CR.carve_rule(0.25, near=0.5, ring=1, max_last=3))


def not_finite():
    """a view entry of 3e38: c_0 overflows for the entry at x = 8 and stays finite for the one at x = 2^-9"""
    cam = camera()
    cam[0] = F(3e38)
    return _case([("inf", entry(8.125, 0.125, 2.125), 1), ("finite", entry(2.0 ** -9, 0.125, 2.125), 1)], lattice(),
                 CR.carve_rule(0.25, near=0.5), cam=cam)


def compare():
    """c_2 + margin == zmin is kept; one float more on the occluder's side carves"""
    lat = lattice(z=2.25)
    lat[0]["z"][3 * 12 + 8] = np.nextafter(F(2.25), F(3))
    u0, v0 = cell_centre(2, 3)
    u1, v1 = cell_centre(8, 3)
    return _case([("tie", at_pixel(u0, v0), 1), ("next", at_pixel(u1, v1), 1)], lat, CR.carve_rule(0.25, near=0.5, ring=0))


def _clip(ring):
    """an entry in every corner cell, in the middle of every border and inside: 4, 6 and 9 cells of a ring"""
    cells = {"nw": (0, 0), "ne": (11, 0), "sw": (0, 6), "se": (11, 6), "n": (5, 0), "s": (5, 6), "w": (0, 3), "e": (11, 3), "mid": (5, 3)}
    return _case([(name, at_pixel(*cell_centre(*c)), 1) for name, c in cells.items()], lattice(), CR.carve_rule(0.25, near=0.5, ring=ring))


def clip_ring0():
    return _clip(0)


def clip_ring1():
    return _clip(1)


BAD = {"dropped": (1, 1), "flag": (4, 1), "nan": (7, 1), "inf": (10, 1), "zero": (1, 4), "negative": (4, 4)}


def _bad(ring):
    """six cells without an occluder depth, each for another reason; an entry on each of them, and one in the cell
    diagonally below it, whose ring meets the bad cell"""
    lat = lattice()
    z, flags = lat[0]["z"], lat[0]["flags"]
    flags[BAD["dropped"][1] * 12 + BAD["dropped"][0]] = VR.DROPPED
    flags[BAD["flag"][1] * 12 + BAD["flag"][0]] = VR.IGNORE_TEMPORARY
    for name, value in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0), ("negative", -4.0)):
        z[BAD[name][1] * 12 + BAD[name][0]] = F(value)
    entries = []
    for name, (ix, iy) in BAD.items():
        entries.append((name, at_pixel(*cell_centre(ix, iy)), 1))
        entries.append((name + "_beside", at_pixel(*cell_centre(ix + 1, iy + 1)), 1))
    entries.append(("other_flag", at_pixel(*cell_centre(10, 5)), 1))
    flags[5 * 12 + 10] = VR.IGNORE_COMPLETELY               # not in drop_flags: the cell has a depth
    return _case(entries, lat, CR.carve_rule(0.25, near=0.5, ring=ring, drop_flags=VR.IGNORE_TEMPORARY))


def bad_ring0():
    return _bad(0)


def bad_ring1():
    return _bad(1)


def _rim(ring):
    """a foreground object at c_2 = 2 fills the cells 4 .. 6 x 2 .. 4 of the occluder; the wall at 4 elsewhere. An entry of the
    object projects one cell beside it (the lattice samples every fourth pixel): its own cell shows the wall"""
    lat = lattice()
    for iy in range(2, 5):
        for ix in range(4, 7):
            lat[0]["z"][iy * 12 + ix] = F(2.0)
    return _case([("rim", at_pixel(*cell_centre(7, 3)), 1), ("inside", at_pixel(*cell_centre(5, 3)), 1), ("far", at_pixel(*cell_centre(10, 3)), 1)],
                 lat, CR.carve_rule(0.25, near=0.5, ring=ring))


def rim_ring0():
    return _rim(0)


def rim_ring1():
    return _rim(1)


CHAIN_KEYS, CHAIN_CARVED = 4, 1                            # entries 59 .. 62 of 64; the one at 60 is carved


def chain():
    """the first four keys of voxel_cases.chain_keys (one home, 59 of 64), one record and one call each, so their
    entries lie at 59, 60, 61, 62. The camera maps every point onto its axis at c_2 = 2 (a view of zeros but for the
    depth), the occluder shows 4 everywhere, and only the second entry is a candidate (stamp 1 <= max_last = 2)"""
    keys = VC.chain_keys()[:CHAIN_KEYS]
    cam = camera()
    cam[:12] = 0
    cam[11] = F(2.0)
    rng = np.random.default_rng(51)
    entries = []
    for i, k in enumerate(keys):
        cell = (VR.key_parts(k)[0] - VR.BIAS, 0, 0)
        entries.append(("chain%d" % i, (VR.records(VC._in_cell([cell], VOXEL, rng), (i + 1, 2, 3)), int(k)), 1 if i == CHAIN_CARVED else 5))
    return _case(entries, lattice(), CR.carve_rule(0.25, near=0.5, max_last=2), cam=cam, log2=VC.CHAIN_LOG2)


def both_reject():
    """the keep rule (last >= 2) and the carve reject `both`; each rejects one more entry alone"""
    return _case([("both", at_pixel(*cell_centre(3, 3)), 1), ("keep_only", at_pixel(*cell_centre(5, 3), c2=4.0), 1),
                  ("carve_only", at_pixel(*cell_centre(7, 3)), 3), ("stays", at_pixel(*cell_centre(9, 3), c2=4.0), 3)],
                 lattice(), CR.carve_rule(0.25, near=0.5), keep=dict(min_stamp=2))


def _grid(c2, stamp=1):
    return [("g%d_%d" % (ix, iy), at_pixel(*cell_centre(ix, iy), c2=c2), stamp) for iy in range(7) for ix in range(12)]


def none_carved():
    """an entry in every cell, all on the wall the occluder shows: all tested, none carved"""
    return _case(_grid(4.0), lattice(), CR.carve_rule(0.25, near=0.5))


def all_carved():
    """an entry in every cell, all in front of the wall"""
    return _case(_grid(2.0), lattice(), CR.carve_rule(0.25, near=0.5))


def empty():
    return _case([], lattice(), CR.carve_rule(0.25, near=0.5), log2=6)


def null_occluder():
    """records == NULL: no evidence anywhere, so the call is the prune by its keep rule"""
    return _case(_grid(2.0)[:20] + [("old", at_pixel(20.5, 20.5, c2=4.0), 1)], None, CR.carve_rule(0.25, near=0.5),
                 keep=dict(min_stamp=1, center=(0.0, 0.0, 2.125), radius=8))


def case(name):
    return globals()[name]()
