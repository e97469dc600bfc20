"""The cross-check of an SGM map (include/svo_hip.h, "sgm cross-check") as plain numpy over tests/sgm_ref.py: the SGM
disparity plane of the pair, that of the mirrored, swapped pair over its own lattice, the lr plane that the lookup into
the mirrored lattice gives, the planes of a checked SGM job, and the max_mean_cost rule of a cloud of SGM planes. Two
formulations: lr_plane walks the lattice point by point, lr_plane_fast is the same numbers as array arithmetic; the
tests tie the second to the first and use it where the first is slow."""
import numpy as np

import cloud_ref as CR
import dense_ref as DR
import lr_ref as LR
import sgm_ref as SR

F = np.float32
INVALID, NO_WAY_BACK = LR.INVALID, LR.NO_WAY_BACK
PATHS = 4


def disparity(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel=True, fast=False):
    """float32 [2, rows, cols]: the SGM disparity and cost planes of a pair (always the disparity)"""
    if fast:
        return SR.planes_fast(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel, SR.DISPARITY, True)
    return SR.planes(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel, SR.DISPARITY, True)


def reverse(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel=True, fast=False):
    """float32 [rows, cols]: the SGM disparity plane of (Lm, Rm) over the lattice "dense" gives the mirrored planes"""
    lm, rm = LR.mirrored(left, right)
    return disparity(lm, rm, win, search_x, search_y, step, p1, p2, cost_cap, subpixel, fast)[0]


def mirrored_cell(w, step, cols, xr):
    """ixm: the lattice cell of the mirrored pair that holds column w - 1 - xr, clamped to the last one"""
    return min((w - 1 - xr) // step, cols - 1)


# ------------------------------------------------------------------ the statement
def lr_plane(fwd, rev, w, step):
    """float32 [rows, cols] from the forward and reverse disparity planes of a pair of width w"""
    rows, cols = fwd.shape
    out = np.empty((rows, cols), F)
    for iy in range(rows):
        for ix in range(cols):
            d = F(fwd[iy, ix])
            if d < 0:
                out[iy, ix] = INVALID
                continue
            xr = LR.matched_column(ix * step + step // 2, d)
            if xr > w - 1:
                out[iy, ix] = NO_WAY_BACK
                continue
            rd = F(rev[iy, mirrored_cell(w, step, cols, xr)])
            out[iy, ix] = NO_WAY_BACK if rd < 0 else np.abs(d - rd)
    return out


# ------------------------------------------------------------------ the second formulation
def lr_plane_fast(fwd, rev, w, step):
    rows, cols = fwd.shape
    d = fwd.astype(F)
    valid = d >= 0
    x = (np.arange(cols) * step + step // 2)[None, :]
    xr = x + (np.where(valid, d, F(0)) + F(0.5)).astype(np.int32)      # float32 add, then truncation
    inside = xr <= w - 1
    ixm = np.minimum((w - 1 - np.where(inside, xr, 0)) // step, cols - 1)
    rd = np.take_along_axis(rev.astype(F), ixm, axis=1)
    out = np.where(rd < 0, F(NO_WAY_BACK), np.abs(d - rd))
    out = np.where(inside, out, F(NO_WAY_BACK))
    return np.where(valid, out, F(INVALID)).astype(F)


def checked_planes(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel=True, value=SR.DISPARITY, cost=True,
                   baseline=1.0, max_lr_diff=0.0, fast=False):
    """svo_dense_disparity_sgm_checked: float32 [1 + cost + 1, rows, cols]: value, [cost], lr"""
    fwd = disparity(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel, fast)
    rev = reverse(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel, fast)
    lr = (lr_plane_fast if fast else lr_plane)(fwd[0], rev, left.shape[1], step)
    return LR.checked_planes(fwd, lr, value, cost, baseline, max_lr_diff)


# ------------------------------------------------------------------ clouds of SGM planes
def kept_mask(planes, local_z, min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0):
    """bool [rows, cols]: cloud_ref.kept_mask with the SGM form of max_mean_cost: best is the sum over four paths of a
    cost per pixel, so a point is dropped iff best > max_mean_cost * 4.0f"""
    disp, best = planes[0].astype(F), planes[1].astype(F)
    keep = disp >= 0
    if F(min_disparity) != 0:
        keep &= ~(disp < F(min_disparity))
    if F(max_depth) != 0:
        keep &= ~(local_z > F(max_depth))
    if F(max_mean_cost) != 0:
        keep &= ~(best > F(max_mean_cost) * F(PATHS))
    return keep


def cloud(left, planes, step, rig, pose, frame=CR.WORLD, layout=CR.COMPACT, min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0):
    """(records, n_points) as cloud_ref.cloud, from the SGM disparity and cost planes (the disparity plane masked by the
    check, where there is one)"""
    h, w = left.shape
    cols, rows, xs, ys = DR.lattice(w, h, step)
    local = CR.local_points(planes, w, h, step, rig)
    keep = kept_mask(planes, local[2], min_disparity, max_depth, max_mean_cost)
    p = CR.world_points(local, pose) if frame == CR.WORLD else list(local)
    out = []
    for iy in range(rows):
        for ix in range(cols):
            gray = left[ys[iy], xs[ix]]
            if keep[iy, ix]:
                out.append((p[0][iy, ix], p[1][iy, ix], p[2][iy, ix], (gray, gray, gray), 0))
            elif layout == CR.ORGANIZED:
                out.append((F(0), F(0), F(0), (gray, gray, gray), CR.DROPPED))
    return np.array(out, CR.POINT).reshape(-1), int(keep.sum())


def masked(fwd, lr, max_lr_diff):
    """the staged planes of a checked cloud: the disparity of a failing point is -1, the cost plane is untouched"""
    out = fwd.copy()
    out[0][LR.fails(lr, max_lr_diff)] = -1.0
    return out
