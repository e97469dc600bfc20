"""The left-right cross-check of include/svo_hip.h ("cross-check") as plain numpy, over the point rule of
tests/dense_ref.py: the mirrored, swapped planes, the lr plane, which points fail at a tolerance, and the planes of a
checked disparity job. Written for the eye, not for speed."""
import numpy as np

import dense_ref as DR

INVALID, NO_WAY_BACK = -1.0, -2.0


def mirrored(left, right):
    """(Lm, Rm): Lm[y][u] = R[y][W - 1 - u], Rm[y][u] = L[y][W - 1 - u]"""
    return np.ascontiguousarray(right[:, ::-1]), np.ascontiguousarray(left[:, ::-1])


def matched_column(x, disp):
    """xr = x + (int)(disp + 0.5f): a float add rounded once, then truncation"""
    return int(x) + int(np.float32(disp) + np.float32(0.5))


def lr_plane(left, right, win, search_x, search_y, step, disp):
    """float32 [rows, cols] of the forward disparity plane `disp` (dense_ref.planes, value = DISPARITY): -1 where the
    forward point is invalid, -2 where the matched column lies outside or the reverse search is invalid, else
    |disp - rd|"""
    h, w = left.shape
    cols, rows, xs, ys = DR.lattice(w, h, step)
    lm, rm = mirrored(left, right)
    out = np.empty((rows, cols), np.float32)
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            d = np.float32(disp[iy, ix])
            if d < 0:
                out[iy, ix] = INVALID
                continue
            xr = matched_column(x, d)
            if xr > w - 1:
                out[iy, ix] = NO_WAY_BACK
                continue
            rd, _ = DR.point(lm, rm, w - 1 - xr, int(y), win, search_x, search_y)
            out[iy, ix] = NO_WAY_BACK if rd < 0 else np.abs(d - np.float32(rd))
    return out


def fails(lr, max_lr_diff):
    """which points fail at the tolerance max_lr_diff > 0: one float32 comparison each"""
    lr = np.asarray(lr, np.float32)
    return (lr < np.float32(0.0)) | (lr > np.float32(max_lr_diff))


def checked_planes(forward, lr, value=DR.DISPARITY, cost=True, baseline=1.0, max_lr_diff=0.0):
    """the planes of a checked disparity job, float32 [1 + cost + 1, rows, cols]: value, [cost], lr. forward: the
    [2, rows, cols] disparity and cost planes of the unchecked search; lr: lr_plane of it. max_lr_diff 0 only reports."""
    disp = forward[0].copy()
    if max_lr_diff > 0:
        disp[fails(lr, max_lr_diff)] = -1.0
    val = disp
    if value == DR.DEPTH:
        val = np.zeros_like(disp)
        val[disp >= 0] = np.float32(baseline) / disp[disp >= 0]   # float / float, one rounding
    return np.stack([val] + ([forward[1]] if cost else []) + [lr]).astype(np.float32)
