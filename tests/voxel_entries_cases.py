"""Crafted inputs of the voxel entries (include/svo_hip.h, "voxel entries"): maps given as the fuse calls that make them
(cases of tests/voxel_cases.py, one map each) and spans of entry records written directly. Each is there for one thing
the pack, merge or rehash kernels can get wrong; tests/test_voxel_entries_cpu.py checks that it does reach it."""
import numpy as np

import voxel_cases as VC
import voxel_entries_ref as ER
import voxel_prune_cases as PC
import voxel_ref as VR

F = np.float32
SMALL_LOG2, SMALL_LIMIT = VC.CHAIN_LOG2, 48                  # 64 entries
TILES_LOG2 = 9                                               # 512 entries: two tiles of 256
DUP_AT = (0, 63, 64, 256)                                    # where the repeated key sits in dup_span()
SPAN_SIZES = (0, 1, 255, 256, 257)


def small_keys():
    """48 keys for a table of 64: the 40 of voxel_cases.chain_keys (one home, 59: the chain wraps from entry 63 to 0)
    and 8 more in a row of voxels elsewhere"""
    more = [(VR.BIAS + i) << 42 | (VR.BIAS + 1) << 21 | (VR.BIAS + 1) for i in range(8)]
    return [int(k) for k in VC.chain_keys()] + more


def small(n):
    """the first n of small_keys as a one-map case: halves fused with stamps 1 and 2 (n = 48: 24 + 24 records, each call
    exactly admitted), colours by index"""
    keys = small_keys()[:n]
    calls = []
    for stamp, part in ((1, keys[:n // 2]), (2, keys[n // 2:])):
        if part:
            rec = PC.records_of_keys(part, 1.0)
            rec["color"] = (np.arange(len(rec))[:, None] * (3, 5, 7) + stamp) % 256
            calls.append([(rec, 0, stamp)])
    return {"maps": [(1.0, SMALL_LOG2, 0)], "calls": calls}


def tiles():
    """a map of 512 entries filled from a lattice of 6 x 6 x 6 voxels in three calls with stamps 1, 2, 3: counts from 1
    to several, entries in both tiles of 256, every call admitted"""
    rng = np.random.default_rng(51)
    calls = []
    for stamp, n in ((1, 200), (2, 100), (3, 80)):
        rec = VR.records(VC._in_cell(rng.integers(-3, 3, (n, 3)), 0.3, rng))
        rec["color"] = rng.integers(0, 256, (n, 3))
        calls.append([(rec, 0, stamp)])
    return {"maps": [(0.3, TILES_LOG2, 0)], "calls": calls}


def union():
    """R1 and R2 of one world (voxel_cases.mixed halved) and the params of their maps"""
    rec, params = VC.mixed()
    return rec[:1500], rec[1500:], params


def lattice_entries(n, first=0, seed=52, voxel_cells=40):
    """n entry records with distinct keys first .. first + n - 1 of a row-major lattice, accumulators that a fuse could
    have produced (count 1 .. 5, sums below 256 * count, last 1 .. 9)"""
    rng = np.random.default_rng(seed + first)
    idx = np.arange(first, first + n)
    cells = np.stack([idx % voxel_cells, idx // voxel_cells % voxel_cells, idx // (voxel_cells * voxel_cells)], axis=1) - 7
    ent = np.zeros(n, ER.ENTRY)
    ent["key"] = ((cells[:, 0] + VR.BIAS).astype(np.uint64) << np.uint64(42) | (cells[:, 1] + VR.BIAS).astype(np.uint64) << np.uint64(21) |
                  (cells[:, 2] + VR.BIAS).astype(np.uint64))
    count = rng.integers(1, 6, n)
    ent["acc"][:, 0] = count
    ent["acc"][:, 1:7] = rng.integers(0, 256, (n, 6)) * count[:, None]
    ent["acc"][:, 7] = rng.integers(1, 10, n)
    return ent


def dup_span():
    """257 records, the same key at records 0, 63, 64 and 256: twice in one wavefront, once in the second wavefront of
    the first workgroup, once in a second workgroup; every other key once"""
    ent = lattice_entries(257)
    for i in DUP_AT[1:]:
        ent[i]["key"] = ent[0]["key"]
    return ent


def wrap_pair():
    """(a map's entries written directly, a span): the count and every sum wrap 2^32 in the first key; `last` is a max
    in both orders in the second and third; the fourth key is new"""
    k = lattice_entries(4, first=5000)["key"]
    top = 0xFFFFFFFF
    have = ER.entries([(k[0], (top, top - 15, top, top - 1, 0x80000000, top, 7, 4)),
                       (k[1], (2, 10, 20, 30, 40, 50, 60, 5)),
                       (k[2], (2, 10, 20, 30, 40, 50, 60, 3))])
    span = ER.entries([(k[0], (2, 0x20, 1, 3, 0x80000000, top, top - 6, 4)),
                       (k[1], (1, 1, 2, 3, 4, 5, 6, 3)),
                       (k[2], (1, 1, 2, 3, 4, 5, 6, 5)),
                       (k[3], (3, 300, 200, 100, 9, 8, 7, 0))])
    return have, span


def skipped_span():
    """eight records, three of them skipped, one of each kind: bit 63 of the key set (not ~0), the key ~0, count 0"""
    ent = lattice_entries(8, first=6000)
    ent[1]["key"] = int(ent[1]["key"]) | ER.BIT63
    ent[4]["key"] = VR.EMPTY
    ent[6]["acc"][0] = 0
    return ent, (1, 4, 6)


def case(name):
    return globals()[name]()
