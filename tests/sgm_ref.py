"""Semi-global aggregation over the dense search of include/svo_hip.h ("sgm") as plain numpy: the cost volume, the four
paths, their sum and the value rule. The functions of the first half are the statement, written for the eye: every
point walks its own candidates and every path its own points. The second half (the *_fast functions) is a second
formulation of the same numbers, box sums by cumulative sums and paths a row at a time, which the tests tie to the
first and use where the first is too slow."""
import numpy as np

import dense_ref as DR

DISPARITY, DEPTH = DR.DISPARITY, DR.DEPTH
F = np.float32
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1))            # r = (dx, dy) over the lattice


# ------------------------------------------------------------------ the statement
def boxes(w, h, x, y, win, search_x, search_y):
    """the template and region of "dense" at pixel (x, y): (x11, y11, tw, th, y21, mw, mh), or None at an invalid point"""
    wb, wa = win // 2, (win + 1) // 2
    x11, x12, y11, y12 = max(0, x - wb), min(w - 1, x + wa), max(0, y - wb), min(h, y + wa)
    x21, x22 = x11, min(w - 1, x + wa + search_x)
    y21, y22 = max(0, y - wb - search_y), min(h - 1, y + wa + search_y)
    if x12 <= 0 or y12 <= 0 or x11 >= w - 1 or y11 >= h - 1:
        return None
    if x22 <= 0 or y22 <= 0 or x21 >= w - 1 or y21 >= h - 1:
        return None
    tw, th = x12 - x11, y12 - y11
    mw, mh = (x22 - x21) - tw + 1, (y22 - y21) - th + 1
    if tw <= 0 or th <= 0 or mw <= 0 or mh <= 0:
        return None
    return x11, y11, tw, th, y21, mw, mh


def raw_minimum(left, right, x, y, win, search_x, search_y):
    """(raw [count] int64, area): min over k < mh of the exact SSD(k, j) for j < count = mw; (None, 0): invalid point"""
    h, w = left.shape
    b = boxes(w, h, x, y, win, search_x, search_y)
    if b is None:
        return None, 0
    x11, y11, tw, th, y21, mw, mh = b
    t = left[y11:y11 + th, x11:x11 + tw].astype(np.int64)
    raw = np.empty(mw, np.int64)
    for j in range(mw):
        ssd = []
        for k in range(mh):
            d = right[y21 + k:y21 + k + th, x11 + j:x11 + j + tw].astype(np.int64) - t
            ssd.append(int((d * d).sum()))
        raw[j] = min(ssd)
    return raw, tw * th


def cost_volume(left, right, win, search_x, search_y, step, cost_cap):
    """(C uint16 [rows, cols, D], count uint16 [rows, cols])"""
    h, w = left.shape
    cols, rows, xs, ys = DR.lattice(w, h, step)
    D = search_x + 1
    C = np.zeros((rows, cols, D), np.uint16)
    count = np.zeros((rows, cols), np.uint16)
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            raw, area = raw_minimum(left, right, int(x), int(y), win, search_x, search_y)
            if raw is None:
                continue                                   # count = 0 and C = 0 for every j
            count[iy, ix] = len(raw)
            C[iy, ix, :] = cost_cap
            C[iy, ix, :len(raw)] = np.minimum(cost_cap, raw // area)
    return C, count


def path(C, r, p1, p2):
    """L_r int64 [rows, cols, D] of the direction r = (dx, dy)"""
    rows, cols, D = C.shape
    dx, dy = r
    L = np.zeros((rows, cols, D), np.int64)
    ys = range(rows) if dy >= 0 else range(rows - 1, -1, -1)
    xs = range(cols) if dx >= 0 else range(cols - 1, -1, -1)
    for iy in ys:
        for ix in xs:
            py, px = iy - dy, ix - dx
            if not (0 <= py < rows and 0 <= px < cols):
                L[iy, ix] = C[iy, ix]
                continue
            P = L[py, px]
            m = int(P.min())
            for j in range(D):
                best = min(int(P[j]), m + p2)
                if j > 0:
                    best = min(best, int(P[j - 1]) + p1)
                if j < D - 1:
                    best = min(best, int(P[j + 1]) + p1)
                L[iy, ix, j] = int(C[iy, ix, j]) + best - m
    return L


def sums(C, p1, p2):
    """S int64 [rows, cols, D]: the sum of the four paths"""
    return sum(path(C, r, p1, p2) for r in DIRECTIONS)


def value_planes(S, count, subpixel, value=DISPARITY, cost=True, baseline=1.0):
    """float32 [1 + cost, rows, cols] from S and the count plane (None: every point has D candidates)"""
    rows, cols, D = S.shape
    out = np.empty((2, rows, cols), F)
    for iy in range(rows):
        for ix in range(cols):
            n = D if count is None else min(int(count[iy, ix]), D)
            if n == 0:
                out[0, iy, ix], out[1, iy, ix] = (0.0 if value == DEPTH else -1.0), -1.0
                continue
            s = S[iy, ix]
            j0 = int(np.argmin(s[:n]))                     # the first of the least
            d = F(j0)
            if subpixel and 0 < j0 < n - 1:
                a, b, c = int(s[j0 - 1]), int(s[j0]), int(s[j0 + 1])
                d = F(F(j0) + F(F(a - c) / F(2 * (a - 2 * b + c))))
            disp = F(0.5) if d < F(0.5) else d
            out[0, iy, ix] = F(baseline) / disp if value == DEPTH else disp
            out[1, iy, ix] = F(int(s[j0]))
    return out if cost else out[:1]


def aggregate(C, count, p1, p2, cost_cap, subpixel, value=DISPARITY, cost=True, baseline=1.0):
    """svo_sgm_aggregate: entries of C above cost_cap are read as cost_cap"""
    return value_planes(sums(np.minimum(C.astype(np.int64), cost_cap), p1, p2), count, subpixel, value, cost, baseline)


def planes(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel=True, value=DISPARITY, cost=True, baseline=1.0):
    """svo_dense_disparity_sgm: float32 [1 + cost, rows, cols]"""
    C, count = cost_volume(left, right, win, search_x, search_y, step, cost_cap)
    return aggregate(C, count, p1, p2, cost_cap, subpixel, value, cost, baseline)


# ------------------------------------------------------------------ the second formulation
def cost_volume_fast(left, right, win, search_x, search_y, step, cost_cap):
    """cost_volume with the SSD of every point as a box sum over E[yy][xx] = (R[yy + dy][xx + j] - L[yy][xx])^2, taken
    from a table of cumulative sums; candidate k of a point is the vertical offset dy = (y21 - y11) + k"""
    h, w = left.shape
    cols, rows, xs, ys = DR.lattice(w, h, step)
    D = search_x + 1
    big = np.iinfo(np.int64).max
    raw = np.full((rows, cols, D), big, np.int64)
    geo = np.zeros((7, rows, cols), np.int64)              # x11, y11, tw, th, y21, mw, mh; mw = 0 at an invalid point
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            b = boxes(w, h, int(x), int(y), win, search_x, search_y)
            if b is not None:
                geo[:, iy, ix] = b
    x11, y11, tw, th, y21, mw, mh = geo
    Lp = left.astype(np.int64)
    for dy in range(-search_y, search_y + 1):
        k = dy - (y21 - y11)
        for j in range(D):
            Rp = np.zeros((h, w), np.int64)                # R[yy + dy][xx + j], 0 outside (never inside a valid box)
            y0, y1, x1 = max(0, -dy), min(h, h - dy), max(0, w - j)
            if y1 > y0 and x1 > 0:
                Rp[y0:y1, :x1] = right[y0 + dy:y1 + dy, j:j + x1]
            T = np.zeros((h + 1, w + 1), np.int64)
            T[1:, 1:] = np.cumsum(np.cumsum((Rp - Lp) ** 2, 0), 1)
            s = T[y11 + th, x11 + tw] - T[y11, x11 + tw] - T[y11 + th, x11] + T[y11, x11]
            use = (j < mw) & (k >= 0) & (k < mh)
            raw[:, :, j] = np.where(use, np.minimum(raw[:, :, j], s), raw[:, :, j])
    valid = mw > 0
    js = np.arange(D)[None, None, :]
    C = np.where(js < mw[:, :, None], np.minimum(cost_cap, raw // np.maximum(tw * th, 1)[:, :, None]), cost_cap)
    C = np.where(valid[:, :, None], C, 0).astype(np.uint16)
    return C, mw.astype(np.uint16)


def sums_fast(C, p1, p2):
    """sums with every path walked a whole row or column of points at a time"""
    C = C.astype(np.int64)
    rows, cols, D = C.shape
    big = np.int64(1) << 40

    def walk(V):                                           # V [n, lines, D]: the path along axis 0, forwards
        L = np.empty_like(V)
        L[0] = V[0]
        for i in range(1, V.shape[0]):
            P = L[i - 1]
            m = P.min(axis=1, keepdims=True)
            lo = np.concatenate([np.full((P.shape[0], 1), big), P[:, :-1]], 1) + p1
            hi = np.concatenate([P[:, 1:], np.full((P.shape[0], 1), big)], 1) + p1
            L[i] = V[i] + np.minimum(np.minimum(P, m + p2), np.minimum(lo, hi)) - m
        return L

    H = C.transpose(1, 0, 2)                               # [cols, rows, D]: along x
    S = walk(H).transpose(1, 0, 2) + walk(H[::-1])[::-1].transpose(1, 0, 2)
    return S + walk(C) + walk(C[::-1])[::-1]


def planes_fast(left, right, win, search_x, search_y, step, p1, p2, cost_cap, subpixel=True, value=DISPARITY, cost=True, baseline=1.0):
    C, count = cost_volume_fast(left, right, win, search_x, search_y, step, cost_cap)
    return value_planes(sums_fast(np.minimum(C.astype(np.int64), cost_cap), p1, p2), count, subpixel, value, cost, baseline)
