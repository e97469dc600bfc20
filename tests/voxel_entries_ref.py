"""The voxel entries of include/svo_hip.h ("voxel entries") as plain numpy on the maps of tests/voxel_ref.py, written
from that section alone: pack (the kept entries in key order, accumulators verbatim), merge (a span of entry records
into a map: adds modulo 2^32, a max, the skipped records) and rehash (the same entries and counters under another
capacity). Two statements, as in voxel_ref: a vectorised one on voxel_ref.Map whose result cannot depend on the order
of its input, and a scalar twin on voxel_ref.ScalarMap that visits record after record. Where an entry lies in a
table is no part of either."""
import copy

import numpy as np

import voxel_ref as VR

ENTRY = np.dtype([("key", "<u8"), ("acc", "<u4", (8,))])       # svo_voxel_entry: count, sx, sy, sz, sr, sg, sb, last
assert ENTRY.itemsize == 40
BIT63 = 1 << 63


def entries(rows):
    """ENTRY records of [(key, (count, sx, sy, sz, sr, sg, sb, last))]"""
    out = np.zeros(len(rows), ENTRY)
    for i, (key, acc) in enumerate(rows):
        out[i]["key"] = key
        out[i]["acc"] = acc
    return out


def same_edge(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def skipped(ent):
    """of every record: is it skipped (bit 63 of the key, the empty key among them, or count 0)"""
    return ((ent["key"] >> np.uint64(63)) != 0) | (ent["acc"][:, 0] == 0)


def load_ok(m, n_records):
    """the merge's load bound: the fuse's, every record of the call counts"""
    return m.n_voxels + n_records <= VR.load_limit(m.log2_capacity)


# ------------------------------------------------------------------------------------------------ vectorised (VR.Map)

def pack(m, min_count=0, min_stamp=0):
    keep = (m.acc[:, 0] >= max(1, min_count)) & (m.acc[:, 7] >= min_stamp)
    out = np.zeros(int(keep.sum()), ENTRY)
    out["key"] = m.keys[keep]                                    # (Map.keys is sorted)
    out["acc"] = m.acc[keep].astype(np.uint32)
    return out


def merge(m, ent, voxel):
    """the span `ent` offered to m (changed in place); the counts of svo_voxel_merge_result"""
    if not same_edge(voxel, m.voxel):
        raise ValueError("the span's voxel edge is not the map's")
    skip = skipped(ent)
    k = ent["key"][~skip]
    rows = ent["acc"][~skip].astype(np.uint64)
    all_keys = np.concatenate([m.keys, k])
    uniq, inv = np.unique(all_keys, return_inverse=True)
    sums = np.zeros((len(uniq), 7), np.uint64)
    np.add.at(sums, inv, np.concatenate([m.acc[:, :7], rows[:, :7]]))
    last = np.zeros(len(uniq), np.uint64)
    np.maximum.at(last, inv, np.concatenate([m.acc[:, 7], rows[:, 7]]))
    claimed = len(uniq) - len(m.keys)
    m.keys, m.acc = uniq, np.concatenate([sums & VR.MASK32, last[:, None]], axis=1)
    m.n_fused += int(rows[:, 0].sum())
    return {"n_offered": len(ent), "n_merged": len(k), "n_skipped": int(skip.sum()), "n_claimed": claimed}


def rehash(m, log2_capacity):
    """a new Map of the other capacity with m's entries and counters, or None: not admitted"""
    if m.n_voxels > VR.load_limit(log2_capacity):
        return None
    out = copy.deepcopy(m)
    out.log2_capacity = int(log2_capacity)
    return out


def map_of(ent, voxel, log2_capacity, drop_flags=0):
    """a Map that holds exactly these entries (unique keys, none skipped), as if written directly; n_fused = 0"""
    m = VR.Map(voxel, log2_capacity, drop_flags)
    order = np.argsort(ent["key"], kind="stable")
    assert len(np.unique(ent["key"])) == len(ent) and not skipped(ent).any()
    m.keys, m.acc = ent["key"][order].astype(np.uint64), ent["acc"][order].astype(np.uint64)
    return m


# ------------------------------------------------------------------------------------------------ scalar (VR.ScalarMap)

def pack_scalar(m, min_count=0, min_stamp=0):
    rows = [(key, m.entries[key]) for key in sorted(m.entries) if m.entries[key][0] >= max(1, min_count) and m.entries[key][7] >= min_stamp]
    return entries(rows)


def merge_scalar(m, ent, voxel):
    if not same_edge(voxel, m.voxel):
        raise ValueError("the span's voxel edge is not the map's")
    res = {"n_offered": 0, "n_merged": 0, "n_skipped": 0, "n_claimed": 0}
    for r in ent:
        res["n_offered"] += 1
        key, acc = int(r["key"]), [int(x) for x in r["acc"]]
        if key & BIT63 or key == VR.EMPTY or acc[0] == 0:
            res["n_skipped"] += 1
            continue
        if key not in m.entries:
            m.entries[key] = [0] * 8
            res["n_claimed"] += 1
        e = m.entries[key]
        for j in range(7):
            e[j] = (e[j] + acc[j]) & 0xFFFFFFFF
        e[7] = max(e[7], acc[7])
        m.n_fused += acc[0]
        res["n_merged"] += 1
    return res


def rehash_scalar(m, log2_capacity):
    if m.n_voxels > VR.load_limit(log2_capacity):
        return None
    out = copy.deepcopy(m)
    out.log2_capacity = int(log2_capacity)
    return out


def scalar_of(m):
    """the ScalarMap with the content of a Map"""
    s = VR.ScalarMap(m.voxel, m.log2_capacity, m.drop_flags)
    s.entries = {int(k): [int(x) for x in a] for k, a in zip(m.keys, m.acc)}
    s.n_fused, s.n_outside = m.n_fused, m.n_outside
    return s


def same(m, s):
    """a Map and a ScalarMap hold the same entries and counters"""
    return (m.n_voxels == s.n_voxels and (m.n_fused, m.n_outside) == (s.n_fused, s.n_outside) and
            pack(m).tobytes() == pack_scalar(s).tobytes())


def extract_of(ent, voxel, min_count=0, min_stamp=0):
    """the extraction formula of "voxel maps" applied to packed entries: voxel_ref.POINT records"""
    m = VR.Map(voxel, 26)
    m.keys, m.acc = ent["key"].astype(np.uint64), ent["acc"].astype(np.uint64)
    return m.extract(min_count, min_stamp)
