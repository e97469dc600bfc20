"""The carve of include/svo_hip.h ("voxel carve") as plain numpy, written from that section alone and built on the
references it names: the point an entry extracts to (voxel_ref), the camera mapping (ar_ref.transform), the "has an
occluder depth" rule (ar_occlusion_ref.occludes) and the keep rule of the prune (voxel_prune_ref.kept_mask). Two
statements: judge() visits one entry at a time and spells every step out for the eye; judge_all() is the same rule
over arrays. Both return, per entry of the map in key order, a label that names where the entry left the rule, so
that the cases can show that they reach what they were crafted for."""
import copy

import numpy as np

import ar_occlusion_ref as AO
import ar_ref as AR
import voxel_prune_ref as PR
import voxel_ref as VR

F = np.float32
# where an entry leaves the rule; only CARVED removes it
LATE, NOT_FINITE, NEAR, OUTSIDE_IMAGE, OUTSIDE_LATTICE, NO_OCCLUDER, INCOMPLETE, BEHIND, CARVED = range(9)
LABELS = ("late", "not_finite", "near", "outside_image", "outside_lattice", "no_occluder", "incomplete", "behind", "carved")
VERDICT = np.dtype([("label", "i4"), ("u", "<f4"), ("v", "<f4"), ("c2", "<f4"), ("cells", "i4"), ("zmin", "<f4")])


def carve_rule(margin, near=0.01, ring=1, max_last=0xFFFFFFFF, drop_flags=0):
    return dict(margin=F(margin), near=F(near), ring=int(ring), max_last=int(max_last), drop_flags=int(drop_flags))


# ------------------------------------------------------------------------------------------------ one entry at a time

def point_of(key, acc, voxel):
    """step 1: the point the entry extracts to, per coordinate in double, rounded once to float"""
    count = int(acc[0])
    return np.array([F((float(cell - VR.BIAS) + (int(acc[1 + j]) / count + 0.5) / 256.0) * float(F(voxel)))
                     for j, cell in enumerate(VR.key_parts(key))], F)


def has_depth(rec, drop_flags):
    """the rule of "ar occlusion": (True, zo) or (False, None)"""
    zo = F(rec["z"])
    if int(rec["flags"]) & (AO.DROPPED | drop_flags):
        return False, None
    if not np.isfinite(zo) or not zo > 0:
        return False, None
    return True, zo


def judge(key, acc, voxel, cam, width, height, lattice, rule):
    """the verdict of one entry: a VERDICT record"""
    out = np.zeros((), VERDICT)
    out["u"] = out["v"] = out["c2"] = out["zmin"] = F(np.nan)
    cam = np.asarray(cam, F)
    view, fx, fy, cx, cy = cam[:12], cam[12], cam[13], cam[14], cam[15]
    if int(acc[7]) > rule["max_last"]:
        out["label"] = LATE
        return out
    w = point_of(key, acc, voxel)
    with np.errstate(all="ignore"):
        c = AR.transform(view, w)
        out["c2"] = c[2]
        if not np.isfinite(c).all():
            out["label"] = NOT_FINITE
            return out
        if c[2] < rule["near"]:
            out["label"] = NEAR
            return out
        u = F(F(fx * c[0]) / c[2]) + cx
        v = F(F(fy * c[1]) / c[2]) + cy
    out["u"], out["v"] = u, v
    if not (u >= F(0) and u < F(width) and v >= F(0) and v < F(height)):
        out["label"] = OUTSIDE_IMAGE
        return out
    if lattice is None:
        out["label"] = NO_OCCLUDER
        return out
    records, cols, rows, step = lattice
    ix, iy = int(u) // step, int(v) // step
    if ix >= cols or iy >= rows:
        out["label"] = OUTSIDE_LATTICE
        return out
    zmin, cells = None, 0
    for dy in range(-rule["ring"], rule["ring"] + 1):
        for dx in range(-rule["ring"], rule["ring"] + 1):
            x, y = ix + dx, iy + dy
            if x < 0 or y < 0 or x >= cols or y >= rows:
                continue
            cells += 1
            ok, zo = has_depth(records[y * cols + x], rule["drop_flags"])
            if not ok:
                out["label"], out["cells"] = INCOMPLETE, cells
                return out
            zmin = zo if zmin is None else min(zmin, zo)
    out["cells"], out["zmin"] = cells, zmin
    with np.errstate(over="ignore"):
        out["label"] = CARVED if F(c[2] + rule["margin"]) < zmin else BEHIND
    return out


def judge_each(m, cam, width, height, lattice, rule):
    out = np.zeros(len(m.keys), VERDICT)
    for i, (k, a) in enumerate(zip(m.keys, m.acc)):
        out[i] = judge(k, a, m.voxel, cam, width, height, lattice, rule)
    return out


# ------------------------------------------------------------------------------------------------ over arrays

def judge_all(m, cam, width, height, lattice, rule):
    """the labels of every entry (int32 [n]) and the c_2, u, v they were judged by, in one sweep"""
    n = len(m.keys)
    label = np.full(n, -1, np.int32)
    if n == 0:
        return label
    cam = np.asarray(cam, F)
    V, fx, fy, cx, cy = cam[:12], cam[12], cam[13], cam[14], cam[15]
    pts = m.extract()                                      # every entry: count >= 1, in key order
    assert len(pts) == n
    w = [pts["x"].astype(F), pts["y"].astype(F), pts["z"].astype(F)]

    def settle(mask, value):
        label[(label < 0) & mask] = value

    settle(m.acc[:, 7] > np.uint64(rule["max_last"]), LATE)
    with np.errstate(all="ignore"):
        c = [((V[4 * k] * w[0] + V[4 * k + 1] * w[1]) + V[4 * k + 2] * w[2]) + V[4 * k + 3] for k in range(3)]
        assert all(x.dtype == F for x in c)
        settle(~(np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])), NOT_FINITE)
        settle(c[2] < rule["near"], NEAR)
        u = (fx * c[0]) / c[2] + cx
        v = (fy * c[1]) / c[2] + cy
        inside = (u >= F(0)) & (u < F(width)) & (v >= F(0)) & (v < F(height))
    settle(~inside, OUTSIDE_IMAGE)
    if lattice is None:
        settle(np.ones(n, bool), NO_OCCLUDER)
        return label
    records, cols, rows, step = lattice
    rec = np.asarray(records).reshape(rows, cols)
    has = AO.occludes(rec, rule["drop_flags"])
    depth = np.where(has, rec["z"], F(np.inf)).astype(F)
    open_ = label < 0
    ix = np.where(open_, u, F(0)).astype(np.int64) // step
    iy = np.where(open_, v, F(0)).astype(np.int64) // step
    settle((ix >= cols) | (iy >= rows), OUTSIDE_LATTICE)
    open_ = label < 0
    ix, iy = np.where(open_, ix, 0), np.where(open_, iy, 0)
    missing = np.zeros(n, bool)
    zmin = np.full(n, np.inf, F)
    r = rule["ring"]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = ix + dx, iy + dy
            inl = (x >= 0) & (y >= 0) & (x < cols) & (y < rows)
            xs, ys = np.clip(x, 0, cols - 1), np.clip(y, 0, rows - 1)
            missing |= inl & ~has[ys, xs]
            zmin = np.minimum(zmin, np.where(inl, depth[ys, xs], F(np.inf))).astype(F)
    settle(missing, INCOMPLETE)
    with np.errstate(all="ignore"):
        front = (c[2] + rule["margin"]).astype(F) < zmin
    settle(front, CARVED)
    settle(np.ones(n, bool), BEHIND)
    return label


# ------------------------------------------------------------------------------------------------ the map afterwards

def carve(m, cam, width, height, lattice, rule, keep=None):
    """the map after the call, in place; returns (result dict of the four counts, labels)"""
    label = judge_all(m, cam, width, height, lattice, rule)
    carved = label == CARVED
    kept = PR.kept_mask(m, **keep) if keep is not None else np.ones(len(m.keys), bool)
    stays = kept & ~carved
    res = {"n_before": m.n_voxels, "n_kept": int(stays.sum()), "n_tested": int(((label == CARVED) | (label == BEHIND)).sum()),
           "n_carved": int(carved.sum())}
    m.keys, m.acc = m.keys[stays], m.acc[stays]
    return res, label


def carved(m, cam, width, height, lattice, rule, keep=None):
    out = copy.deepcopy(m)
    res, label = carve(out, cam, width, height, lattice, rule, keep)
    return out, res, label
