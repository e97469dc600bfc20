"""The prune of include/svo_hip.h ("voxel prune") as plain numpy over voxel_ref.Map, written from that section alone:
the keep rule of one entry, spelled out for the eye, and the map after a prune. A Map is its sorted keys and their
accumulators, so "the map holds exactly the kept entries, each with its accumulators unchanged" is all there is to
say; the three cumulative counters stay. place() and lookup() are the diagnostic side: where sequential inserts put
keys in a table, and what a probe finds there, so that the cases can show that they cut a chain."""
import copy

import numpy as np

import voxel_ref as VR


def center_voxel(center, voxel):
    """(cix, ciy, ciz): the indices the key rule gives the centre, or None: outside (a NaN and an infinity too)"""
    kp = VR.scalar_key(center[0], center[1], center[2], voxel)
    return None if kp is None else VR.key_parts(kp[0])


def keeps(key, acc, voxel, min_count=0, min_stamp=0, center=(0.0, 0.0, 0.0), radius=-1):
    """is the entry (key, its eight accumulators) kept?"""
    count, last = int(acc[0]), int(acc[7])
    if count < max(1, min_count):
        return False
    if last < min_stamp:
        return False
    if radius < 0:
        return True                                           # no box: the centre is not read
    c = center_voxel(center, voxel)
    assert c is not None, "a centre outside the key range is rejected, not applied"
    ix, iy, iz = VR.key_parts(key)
    return abs(ix - c[0]) <= radius and abs(iy - c[1]) <= radius and abs(iz - c[2]) <= radius


def kept_mask(m, **keep):
    return np.array([keeps(k, a, m.voxel, **keep) for k, a in zip(m.keys, m.acc)], bool).reshape(len(m.keys))


def prune(m, **keep):
    """the map after the prune, in place; returns (n_before, n_kept)"""
    mask = kept_mask(m, **keep)
    n_before = m.n_voxels
    m.keys, m.acc = m.keys[mask], m.acc[mask]
    return n_before, m.n_voxels


def pruned(m, **keep):
    out = copy.deepcopy(m)
    prune(out, **keep)
    return out


def extract_both(m, keep, **filt):
    """the extraction of m with "filt and keep", m unchanged"""
    return pruned(m, **keep).extract(**filt)


# ------------------------------------------------------------------------------------------------ placement

def place(keys, log2_capacity):
    """the table after inserting `keys` one after the other: home, then step +1 modulo the capacity"""
    cap = 1 << log2_capacity
    table = [VR.EMPTY] * cap
    for k in keys:
        s = VR.home(k, log2_capacity)
        while table[s] != VR.EMPTY:
            assert table[s] != int(k)
            s = (s + 1) % cap
        table[s] = int(k)
    return table


def lookup(table, key, log2_capacity):
    """the entry a probe for `key` ends at, or None when it meets an empty entry first"""
    s = VR.home(key, log2_capacity)
    for _ in range(len(table)):
        if table[s] == int(key):
            return s
        if table[s] == VR.EMPTY:
            return None
        s = (s + 1) % len(table)
    return None
