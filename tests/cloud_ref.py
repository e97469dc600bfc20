"""The dense coloured point cloud of include/svo_hip.h ("clouds") as plain numpy float32: the triangulation of a
lattice point from its disparity, the rotation into the world frame, the filter, the record and the two layouts, on top
of the two planes of tests/dense_ref.py. Every operation is one float32 operation, in the header's order; the
compaction is an explicit row-major walk."""
import numpy as np

import dense_ref as DR
import oracle_py as O

F = np.float32
WORLD, CAMERA = 0, 1
COMPACT, ORGANIZED = 0, 1
DROPPED = 0x80
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("color", "u1", (3,)), ("flags", "u1")])
RIG_KEYS = ("fx", "fy", "cx", "cy", "baseline")


def rotation(pose):
    """PoseManager's float rotation matrix of a pose: Rodrigues in double, rounded to float once"""
    return O.rodrigues(np.asarray(pose, F)[3:6]).astype(F)


def _matvec(M, v):
    """Matx33f * Vec3f: s = 0; s += M[i][k] * v[k], k = 0, 1, 2"""
    out = []
    for i in range(3):
        s = np.zeros_like(v[0])
        for k in range(3):
            s = s + M[i, k] * v[k]
        out.append(s)
    return out


def local_points(planes, w, h, step, rig):
    """(_x, _y, _z) float32 [rows, cols] of every lattice point from its disparity (an invalid point: from 0.5)"""
    cols, rows, xs, ys = DR.lattice(w, h, step)
    fx, fy, cx, cy, baseline = (F(rig[k]) for k in RIG_KEYS)
    X = np.broadcast_to(xs.astype(F)[None, :], (rows, cols))
    Y = np.broadcast_to(ys.astype(F)[:, None], (rows, cols))
    _z = baseline / np.maximum(F(0.5), planes[0].astype(F))
    _x = (X - cx) / fx * _z
    _y = (Y - cy) / fy * _z
    assert _x.dtype == _y.dtype == _z.dtype == F
    return _x, _y, _z


def world_points(local, pose):
    pose = np.asarray(pose, F)
    p = _matvec(rotation(pose), list(local))
    return [p[k] + pose[k] for k in range(3)]


def kept_mask(planes, w, h, win, step, local_z, min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0):
    """bool [rows, cols]: valid and not dropped by the filter"""
    cols, rows, xs, ys = DR.lattice(w, h, step)
    disp, best = planes[0].astype(F), planes[1].astype(F)
    keep = disp >= 0
    if F(min_disparity) != 0:
        keep &= ~(disp < F(min_disparity))
    if F(max_depth) != 0:
        keep &= ~(local_z > F(max_depth))
    if F(max_mean_cost) != 0:
        wb, wa = win // 2, (win + 1) // 2
        tw = np.minimum(w - 1, xs + wa) - np.maximum(0, xs - wb)
        th = np.minimum(h, ys + wa) - np.maximum(0, ys - wb)
        area = (th[:, None] * tw[None, :]).astype(F)
        keep &= ~(best > F(max_mean_cost) * area)
    return keep


def cloud(left, planes, win, step, rig, pose, frame=WORLD, layout=COMPACT, min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0):
    """(records, n_points): records of POINT, n_points of them (compact) or rows * cols (organized). left: uint8
    [H, W]; planes: float32 [2, rows, cols], the disparity and cost planes of dense_ref.planes"""
    h, w = left.shape
    cols, rows, xs, ys = DR.lattice(w, h, step)
    local = local_points(planes, w, h, step, rig)
    keep = kept_mask(planes, w, h, win, step, local[2], min_disparity, max_depth, max_mean_cost)
    p = world_points(local, pose) if frame == WORLD else list(local)
    out = []
    for iy in range(rows):                                   # the compaction: row-major, iy outer, ix inner
        for ix in range(cols):
            gray = left[ys[iy], xs[ix]]
            if keep[iy, ix]:
                out.append((p[0][iy, ix], p[1][iy, ix], p[2][iy, ix], (gray, gray, gray), 0))
            elif layout == ORGANIZED:
                out.append((F(0), F(0), F(0), (gray, gray, gray), DROPPED))
    return np.array(out, POINT).reshape(-1), int(keep.sum())
