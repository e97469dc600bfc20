"""The dense disparity / depth map of include/svo_hip.h ("dense") as plain numpy: the lattice, the point rule with the
reference's clipped boxes, the one-pass argmin and tie rule, the depth and cost planes. Written for the eye, not for
speed: every lattice point walks its own candidates."""
import numpy as np

DISPARITY, DEPTH = 0, 1


def lattice(w, h, step):
    """(cols, rows, xs, ys): the pixel columns and rows of the lattice points"""
    cols, rows = w // step, h // step
    return cols, rows, np.arange(cols) * step + step // 2, np.arange(rows) * step + step // 2


def point(left, right, x, y, win, search_x, search_y):
    """(disparity, best) of the pixel (x, y); (-1, -1) for an invalid point. left, right: uint8 [H, W]"""
    h, w = left.shape
    wb, wa = win // 2, (win + 1) // 2
    x11, x12, y11, y12 = max(0, x - wb), min(w - 1, x + wa), max(0, y - wb), min(h, y + wa)
    x21, x22 = x11, min(w - 1, x + wa + search_x)
    y21, y22 = max(0, y - wb - search_y), min(h - 1, y + wa + search_y)
    if x12 <= 0 or y12 <= 0 or x11 >= w - 1 or y11 >= h - 1:
        return -1.0, -1.0
    if x22 <= 0 or y22 <= 0 or x21 >= w - 1 or y21 >= h - 1:
        return -1.0, -1.0
    tw, th = x12 - x11, y12 - y11
    mw, mh = (x22 - x21) - tw + 1, (y22 - y21) - th + 1
    if tw <= 0 or th <= 0 or mw <= 0 or mh <= 0:
        return -1.0, -1.0
    t = left[y11:y12, x11:x12].astype(np.int64)
    best, minx, total, count = None, 0, 0, 0
    for k in range(mh):
        for j in range(mw):
            d = right[y21 + k:y21 + k + th, x21 + j:x21 + j + tw].astype(np.int64) - t
            v = np.float32(int((d * d).sum()))                  # the exact integer, rounded once
            if best is None or v < best:
                best, minx, total, count = v, j, j, 1
            elif v == best and j >= minx:
                total += j
                count += 1
    d = np.float32(total) / np.float32(count)
    return float(np.float32(0.5) if d < np.float32(0.5) else d), float(best)


def planes(left, right, win, search_x, search_y, step=1, value=DISPARITY, cost=True, baseline=1.0):
    """float32 [1 + cost, rows, cols]: the value plane and, with cost, the cost plane"""
    h, w = left.shape
    cols, rows, xs, ys = lattice(w, h, step)
    out = np.empty((2, rows, cols), np.float32)
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            d, b = point(left, right, int(x), int(y), win, search_x, search_y)
            out[0, iy, ix], out[1, iy, ix] = d, b
    if value == DEPTH:
        valid = out[0] >= 0
        z = np.zeros_like(out[0])
        z[valid] = np.float32(baseline) / out[0][valid]          # float / float, one rounding
        out[0] = z
    return out if cost else out[:1]


def lattice_keypoints(w, h, step):
    """the lattice points as keypoints [rows * cols, 2] float32 (row-major), for a per-keypoint disparity function"""
    cols, rows, xs, ys = lattice(w, h, step)
    return np.stack([np.tile(xs, rows), np.repeat(ys, cols)], 1).astype(np.float32)
