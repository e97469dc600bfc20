"""Crafted 8-bit images, plain statements of the two window operations (pyramidal Lucas-Kanade tracking and
SSD stereo matching) and the case lists of tests/test_window_cpu.py and tests/test_window_gpu.py.

Nothing here calls the HIP library or the C oracle. numpy and scipy only:

  ssd_ref  DepthFilter::calculate_disparities (src/lib/depth_filter.cpp:259-327): the int64 match map of
           cv::matchTemplate(TM_SQDIFF) by brute force, cv::minMaxLoc on the map ROUNDED TO FLOAT (first
           minimum in row-major order), the tie rectangle from it. Next to the disparity it reports what the
           rule "first minimum of the INTEGER map" would have given: above 2^24 two integers can round to one
           float, and then the two rules start their tie rectangles at different positions.
  klt_ref  cv::calcOpticalFlowPyrLK as oracle/hot_path.c's header comment restates it: levels padded with
           np.pad(mode="reflect"), Scharr from scipy.ndimage.correlate (reflection inside the image, zero
           outside it), the 14-bit weights and the three descales as whole-window array expressions, the five
           window sums as Python integers, every float step one np.float32 operation at a time. It labels how
           every level of every point ended and keeps the largest sums it met.

What was tried for the two labels that the issue allows to be missing is written next to `klt_cases`.
"""
import functools
import math

import numpy as np
from scipy import ndimage

F = np.float32
LABELS = ("prev_outside", "flat", "left_range_in_iteration", "converged", "backed_off", "ran_30",
          "final_window_outside")


# ------------------------------------------------------------------ textures
TEXTURES = ("noise", "const0", "const255", "const77", "stripes4_v", "stripes4_h", "diag4", "checker3",
            "binblocks2", "antidiag_blocks", "ramp", "blur", "lowblur", "real")


GUARD = 0xA5            # no generated image holds this grey level: the layout tests surround their views with it


def without_guard(img):
    """img with the grey level GUARD replaced by its neighbour"""
    return np.where(img == GUARD, GUARD - 1, img).astype(np.uint8)


def _stretch(a):
    return np.round((a - a.min()) / (a.max() - a.min()) * 255)


@functools.lru_cache(maxsize=None)
def _real():
    import util
    return util.real_pair()


def texture(name, h, w, seed=0):
    """uint8 [h, w] image of the named class"""
    rng = np.random.RandomState(seed + 7919 * TEXTURES.index(name))
    y, x = np.mgrid[0:h, 0:w]

    def blocks2():
        return np.kron(rng.randint(0, 2, ((h + 1) // 2, (w + 1) // 2)), np.ones((2, 2), np.int64))[:h, :w] * 255

    if name == "noise":
        img = rng.randint(0, 256, (h, w))
    elif name.startswith("const"):
        img = np.full((h, w), int(name[5:]))
    elif name == "stripes4_v":                       # |Ix| = 4080 in every pixel
        img = (x // 2) % 2 * 255
    elif name == "stripes4_h":
        img = (y // 2) % 2 * 255
    elif name == "diag4":                            # one direction only: the largest sums, and flat
        img = ((x + y) // 2) % 2 * 255
    elif name == "checker3":
        img = (x // 3 + y // 3) % 2 * 255
    elif name == "binblocks2":
        img = blocks2()
    elif name == "antidiag_blocks":                  # A12 strongly negative, and trackable
        img = ((x - y) // 2) % 2 * 255
        cells = rng.randint(0, 4, ((h + 7) // 8, (w + 7) // 8)) == 0
        img = np.where(np.kron(cells, np.ones((8, 8), bool))[:h, :w], blocks2(), img)
    elif name == "ramp":
        img = x * 255 // max(w - 1, 1)
    elif name == "blur":                             # smooth: a wide basin for large motions
        img = _stretch(ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 8))
    elif name == "lowblur":                          # smooth and of low contrast: minEig around the threshold
        img = 120 + _stretch(ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 8)) // 24
    elif name == "real":
        src = _real()[0]
        img = np.tile(src, (-(-h // src.shape[0]), -(-w // src.shape[1])))[:h, :w]
    else:
        raise KeyError(name)
    return without_guard(np.ascontiguousarray(img, dtype=np.uint8))


def parity_pair(h, w, seed=1):
    """the dark / bright stereo pair with striped columns: every SSD of a 31 x 31 window is far above 2^24
    and neighbouring offsets differ by a few units, so different integers round to the same float"""
    rng = np.random.RandomState(seed)
    odd = (np.arange(w) % 2 == 1)[None, :]
    left = np.where(odd, rng.randint(0, 4, (h, w)), 0).astype(np.uint8)
    right = np.where(odd, rng.randint(0, 4, (h, w)), 255).astype(np.uint8)
    return left, right


def subpixel(img, dy, dx):
    """img moved by (dy, dx) pixels, bilinear, rounded"""
    out = ndimage.shift(img.astype(np.float64), (dy, dx), order=1, mode="mirror")
    return without_guard(np.clip(np.round(out), 0, 255).astype(np.uint8))


def island(img, field=77, border=0.3):
    """the texture kept in the middle of a constant field"""
    h, w = img.shape
    out = np.full_like(img, field)
    y0, x0 = int(h * border), int(w * border)
    out[y0:h - y0, x0:w - x0] = img[y0:h - y0, x0:w - x0]
    return out


# ------------------------------------------------------------------ SSD
def ssd_ref(left, right, kps, win, sx, sy, clamp):
    """dict of per-keypoint arrays: disparity (float32, -1 where the reference skips the keypoint), tw, th,
    mw, mh (0 where skipped), min_int (smallest integer SSD), ties (entries of the tie rectangle that count),
    split (the first integer minimum and the first float minimum are different positions), disparity_int
    (what the first INTEGER minimum with the same tie rule gives)."""
    rows, cols = left.shape
    wb, wa = win // 2, (win + 1) // 2
    n = len(kps)
    out = dict(disparity=np.full(n, -1, F), disparity_int=np.full(n, -1, F), min_int=np.zeros(n, np.int64),
               ties=np.zeros(n, np.int64), split=np.zeros(n, bool),
               **{k: np.zeros(n, np.int64) for k in ("tw", "th", "mw", "mh")})
    L, R = left.astype(np.int64), right.astype(np.int64)
    for i in range(n):
        x, y = int(kps[i][0]), int(kps[i][1])        # (int) of a float: towards zero
        x11, x12 = max(0, x - wb), min(cols - 1, x + wa)
        y11, y12 = max(0, y - wb), min(rows, y + wa)
        if clamp and (x12 <= 0 or y12 <= 0 or x11 >= cols - 1 or y11 >= rows - 1):
            continue
        x21, x22 = x11, min(cols - 1, x + wa + sx)
        y21, y22 = max(0, y - wb - sy), min(rows - 1, y + wa + sy)
        if clamp and (x22 <= 0 or y22 <= 0 or x21 >= cols - 1 or y21 >= rows - 1):
            continue
        tw, th = x12 - x11, y12 - y11
        mw, mh = (x22 - x21) - tw + 1, (y22 - y21) - th + 1
        if tw <= 0 or th <= 0 or mw <= 0 or mh <= 0:
            continue                                  # cv::matchTemplate would throw
        t, roi = L[y11:y12, x11:x12], R[y21:y22, x21:x22]
        views = np.lib.stride_tricks.sliding_window_view(roi, (th, tw))       # [mh, mw, th, tw]
        m = ((views - t) ** 2).sum(axis=(2, 3))                                # int64, exact
        mf = m.astype(F)                                                       # what cv::minMaxLoc sees
        jj = np.arange(mw)[None, :]

        def tie_average(k0, j0, min_val):
            sel = mf[k0:, j0:] <= min_val
            cnt = int(sel.sum())
            pos = F(int((sel * jj[:, j0:]).sum())) / F(cnt)
            return (max(F(0.5), pos) if clamp else pos), cnt

        kf, jf = np.unravel_index(np.argmin(mf), mf.shape)                    # first minimum, rows outer
        ki, ji = np.unravel_index(np.argmin(m), m.shape)
        out["disparity"][i], out["ties"][i] = tie_average(kf, jf, mf[kf, jf])
        out["disparity_int"][i], _ = tie_average(ki, ji, F(int(m[ki, ji])))
        out["split"][i] = (kf, jf) != (ki, ji)
        out["min_int"][i] = m.min()
        out["tw"][i], out["th"][i], out["mw"][i], out["mh"][i] = tw, th, mw, mh
    return out


# ------------------------------------------------------------------ KLT
def scharr_ref(img):
    """int64 [h, w, 2]: (dx, dy) of calcSharrDeriv, BORDER_REFLECT_101 at the image border"""
    a = img.astype(np.int64)
    kx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]])
    return np.stack([ndimage.correlate(a, kx, mode="mirror"), ndimage.correlate(a, kx.T, mode="mirror")], -1)


def _weights(a, b):
    one, s = F(1), F(1 << 14)
    w00 = int(np.rint((one - a) * (one - b) * s))     # rint: to nearest even, like lrintf
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << 14) - w00 - w01 - w10


def _floor(v):
    """(int)floorf(v); None for what does not fit an int (NaN, infinities, beyond 2^31: outside every image)"""
    v = float(v)
    if not math.isfinite(v) or abs(v) >= 2.0 ** 31:
        return None
    return math.floor(v)


def _inside(ix, iy, win, w, h):
    return ix is not None and iy is not None and -win <= ix < w and -win <= iy < h


def _bilinear(pad, ix, iy, win, wts, shift):
    """(win x win) window whose top-left tap is pixel (ix, iy) of the image that `pad` extends by win pixels
    on every side: 4-tap sum with the integer weights, rounded and shifted down"""
    b = pad[iy + win:iy + 2 * win + 1, ix + win:ix + 2 * win + 1]
    s = b[:-1, :-1] * wts[0] + b[:-1, 1:] * wts[1] + b[1:, :-1] * wts[2] + b[1:, 1:] * wts[3]
    return (s + (1 << (shift - 1))) >> shift


def klt_ref(prev_levels, cur_levels, prev_pts, init, win):
    """(pts [n, 2] float32, status [n] uint8, err [n] float32, info). info: labels [n][level] (None for a
    level that was not entered), sums [n, levels, 5] int64 (largest |A11|, |A12|, |A22|, |b1|, |b2| met; A12
    signed in a12 [n, levels]), moved [n, levels, 2] float32 (position after the level minus before it), ci
    [n, levels, 2] int64 (sum I Ix, sum I Iy over the reference window: constants of a level's template)."""
    nl = min(len(prev_levels), len(cur_levels))
    n = len(prev_pts)
    half = F(win - 1) * F(0.5)
    scale20 = F(1.0 / (1 << 20))
    eps = 0.01
    eps *= eps
    P = [np.pad(im.astype(np.int64), win, mode="reflect") for im in prev_levels[:nl]]
    J = [np.pad(im.astype(np.int64), win, mode="reflect") for im in cur_levels[:nl]]
    D = [np.pad(scharr_ref(im), ((win, win), (win, win), (0, 0))) for im in prev_levels[:nl]]
    pts = np.array(init, F).reshape(n, 2).copy()
    status, err = np.ones(n, np.uint8), np.zeros(n, F)
    labels = [[None] * nl for _ in range(n)]
    sums = np.zeros((n, nl, 5), np.int64)
    a12 = np.zeros((n, nl), np.int64)
    ci = np.zeros((n, nl, 2), np.int64)
    moved = np.zeros((n, nl, 2), F)
    for i in range(n):
        for level in range(nl - 1, -1, -1):
            rows, cols = prev_levels[level].shape
            jrows, jcols = cur_levels[level].shape
            lscale = F(1.0 / (1 << level))
            prevx, prevy = F(prev_pts[i][0]) * lscale, F(prev_pts[i][1]) * lscale
            if level == nl - 1:
                nextx, nexty = pts[i, 0] * lscale, pts[i, 1] * lscale
            else:
                nextx, nexty = pts[i, 0] * F(2), pts[i, 1] * F(2)
            pts[i] = nextx, nexty
            start = pts[i].copy()
            prevx, prevy = prevx - half, prevy - half
            ipx, ipy = _floor(prevx), _floor(prevy)
            if not _inside(ipx, ipy, win, cols, rows):
                labels[i][level] = "prev_outside"
                if level == 0:
                    status[i], err[i] = 0, 0
                continue
            wts = _weights(prevx - F(ipx), prevy - F(ipy))
            Iw = _bilinear(P[level], ipx, ipy, win, wts, 14 - 5)
            Ix = _bilinear(D[level][..., 0], ipx, ipy, win, wts, 14)
            Iy = _bilinear(D[level][..., 1], ipx, ipy, win, wts, 14)
            iA11, iA12, iA22 = int((Ix * Ix).sum()), int((Ix * Iy).sum()), int((Iy * Iy).sum())
            sums[i, level, :3] = abs(iA11), abs(iA12), abs(iA22)
            a12[i, level] = iA12
            ci[i, level] = int((Iw * Ix).sum()), int((Iw * Iy).sum())
            A11, A12, A22 = F(iA11) * scale20, F(iA12) * scale20, F(iA22) * scale20
            Dt = A11 * A22 - A12 * A12
            dif = A11 - A22
            min_eig = (A22 + A11 - np.sqrt(dif * dif + F(4) * A12 * A12)) / F(2 * win * win)
            if float(min_eig) < 1e-4 or Dt < np.finfo(F).eps:
                labels[i][level] = "flat"
                if level == 0:
                    status[i] = 0
                continue
            Dt = F(1) / Dt
            nextx, nexty = nextx - half, nexty - half
            pdx = pdy = F(0)
            label = "ran_30"
            for j in range(30):
                inx, iny = _floor(nextx), _floor(nexty)
                if not _inside(inx, iny, win, jcols, jrows):
                    label = "left_range_in_iteration"
                    if level == 0:
                        status[i] = 0
                    break
                wts = _weights(nextx - F(inx), nexty - F(iny))
                diff = _bilinear(J[level], inx, iny, win, wts, 14 - 5) - Iw
                ib1, ib2 = int((diff * Ix).sum()), int((diff * Iy).sum())
                sums[i, level, 3] = max(sums[i, level, 3], abs(ib1))
                sums[i, level, 4] = max(sums[i, level, 4], abs(ib2))
                b1, b2 = F(ib1) * scale20, F(ib2) * scale20
                dx = (A12 * b2 - A22 * b1) * Dt
                dy = (A12 * b1 - A11 * b2) * Dt
                nextx, nexty = nextx + dx, nexty + dy
                pts[i] = nextx + half, nexty + half
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps:
                    label = "converged"
                    break
                if j > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                    pts[i, 0] -= dx * F(0.5)
                    pts[i, 1] -= dy * F(0.5)
                    label = "backed_off"
                    break
                pdx, pdy = dx, dy
            with np.errstate(invalid="ignore"):                 # (an infinite start stays where it is)
                moved[i, level] = pts[i] - start
            if status[i] and level == 0:
                npx, npy = pts[i, 0] - half, pts[i, 1] - half
                inx, iny = _floor(npx), _floor(npy)
                if not _inside(inx, iny, win, jcols, jrows):
                    status[i] = 0
                    label = "final_window_outside"
                else:
                    wts = _weights(npx - F(inx), npy - F(iny))
                    diff = _bilinear(J[level], inx, iny, win, wts, 14 - 5) - Iw
                    err[i] = F(int(np.abs(diff).sum())) * F(1) / F(32 * win * win)   # (< 2^24: the float sum is exact)
            labels[i][level] = label
    err[status == 0] = np.inf
    return pts, status, err, dict(labels=labels, sums=sums, a12=a12, moved=moved, ci=ci)


# ------------------------------------------------------------------ case lists
KLT_H, KLT_W = 150, 203                              # three LK levels up to window 35; the width is odd


def _points(rng, n, h, w, lo=-45.0):
    """n points, most inside the image, some up to -lo pixels outside it"""
    return np.stack([rng.uniform(lo, w - lo, n), rng.uniform(lo, h - lo, n)], 1).astype(F)


def _inner(rng, n, h, w, margin):
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1).astype(F)


@functools.lru_cache(maxsize=None)
def klt_cases():
    """list of (name, prev image, cur image, prev_pts, init, win). Windows 5, 21, 31 run in the 32-column
    kernel shape, 33 and 35 in the 36-column one; every kind of case exists for both."""
    h, w = KLT_H, KLT_W
    cases = []

    def add(name, prev, cur, pts, init, wins):
        for win in wins:
            cases.append((f"{name}-w{win}", prev, cur, pts, np.ascontiguousarray(init, F), win))

    rng = np.random.RandomState(11)
    noise = texture("noise", h, w)
    # ordinary tracking, points inside and outside the image, the start off by up to 3 px
    pts = _points(rng, 70, h, w)
    add("noise_roll1", noise, np.roll(noise, 1, axis=1), pts, pts + rng.uniform(-3, 3, pts.shape), (5, 21, 31, 33, 35))
    # the start far off: windows that leave the image on the coarse levels and on level 0
    pts = _points(rng, 60, h, w, lo=-20.0)
    add("noise_far_start", noise, subpixel(noise, 0.5, -0.25), pts, pts + rng.uniform(-90, 90, pts.shape), (21, 31, 35))
    # flat everywhere (constant; one-directional stripes: the largest sums there are)
    pts = _points(rng, 24, h, w, lo=-10.0)
    for name in ("const0", "const255", "const77", "stripes4_v", "stripes4_h", "diag4", "ramp"):
        img = texture(name, h, w)
        add(name, img, np.roll(img, 1, axis=(0, 1)), pts, pts + F(0.5), (31, 35) if name != "diag4" else (5, 21, 31, 33, 35))
    # 0/255 textures that track: sums above 2^32, A12 below -2^31, b above 2^31
    pts = _inner(rng, 40, h, w, 12)
    for name in ("binblocks2", "checker3", "antidiag_blocks"):
        img = texture(name, h, w)
        add(name + "_sub", img, subpixel(img, 0.4, -0.3), pts, pts + rng.uniform(-1, 1, pts.shape), (21, 31, 35))
        add(name + "_roll1", img, np.roll(img, 1, axis=1), pts, pts, (31, 33, 35))
        add(name + "_inv", img, 255 - img, pts, pts, (31, 35))
    # flat on the coarse levels (the pyramid averages the +-3 grey levels away), tracked on level 0
    low = (128 + np.random.RandomState(12).randint(-3, 4, (h, w))).astype(np.uint8)
    add("lownoise", low, np.roll(low, 1, axis=0), pts, pts, (21, 31, 35))
    lowb = texture("lowblur", h, w)
    add("lowblur", lowb, subpixel(lowb, -0.5, 0.5), pts, pts + F(0.25), (31, 35))
    # a textured island on a constant field: flat, half flat and textured windows
    isl = island(texture("binblocks2", h, w))
    pts = _points(rng, 60, h, w, lo=5.0)
    add("island", isl, subpixel(isl, 0.3, 0.6), pts, pts, (5, 31, 35))
    real = texture("real", h, w)
    add("real_sub", real, subpixel(real, -1.3, 2.2), pts, pts, (21, 35))
    # large motions from a zero initial flow: 40 px are 10 px on level 2, more than the search tile's margin twice over
    hb, wb_ = 240, 320
    blur = texture("blur", hb, wb_)
    pts = _inner(rng, 60, hb, wb_, 30)
    for tag, shift, axis in (("px", 40, 1), ("nx", -40, 1), ("py", 40, 0), ("ny", -40, 0)):
        add("blur_roll40" + tag, blur, np.roll(blur, shift, axis=axis), pts, pts, (31, 35))
    # windows at the edge of the tracked range on a texture of one direction: D is tiny, the steps are tens of
    # pixels, most points run all 30 iterations, and a few take their last step out of the range (the only
    # inputs found for `final_window_outside`: sub-pixel shifts, inverted copies and rolled copies of
    # checker3, antidiag_blocks and binblocks2 with 400 points at the range's edge gave none; a point that
    # converges or backs off does so with a step below 0.01 px, which does not cross the edge)
    diag = texture("diag4", h, w)
    for win in (21, 31, 33, 35):
        add("diag4_edge", diag, np.roll(diag, 1, axis=(0, 1)), *_edge_points(7, 400, h, w, win), (win,))
    # images smaller than the window: one level, most of every window is reflected border
    small = texture("noise", 20, 20, seed=3)
    pts = _points(rng, 30, 20, 20, lo=-12.0)
    add("small20x20", small, subpixel(small, 0.3, -0.4), pts, pts + rng.uniform(-1, 1, pts.shape), (5, 31, 35))
    thin = texture("binblocks2", 9, 40, seed=4)
    pts = _points(rng, 30, 9, 40, lo=-8.0)
    add("thin9x40", thin, np.roll(thin, 1, axis=1), pts, pts, (21, 33))
    return cases


def _edge_points(seed, n, h, w, win):
    """(prev_pts, init): points whose window corner lies within a few pixels of the edge of [-win, w) x [-win, h)"""
    rng = np.random.RandomState(seed)
    side = rng.randint(0, 4, n)
    half = (win - 1) / 2
    x, y = rng.uniform(0, w, n), rng.uniform(0, h, n)
    x = np.where(side == 0, rng.uniform(-8, 6, n), np.where(side == 1, w + half + rng.uniform(-14, -1, n), x))
    y = np.where(side == 2, rng.uniform(-8, 6, n), np.where(side == 3, h + half + rng.uniform(-14, -1, n), y))
    pts = np.stack([x, y], 1).astype(F)
    return pts, pts + F(0.5)


SSD_H, SSD_W = 60, 123


@functools.lru_cache(maxsize=None)
def ssd_cases():
    """list of (name, left, right, kps, win, search_x, search_y, clamp_half)"""
    cases = []
    rng = np.random.RandomState(21)
    h, w = SSD_H, SSD_W
    noise = texture("noise", h, w, seed=1)
    pair = (noise, np.roll(noise, 7, axis=1))
    # keypoints walking through the image and over all four borders: every template and map size
    xs = np.arange(-22, w + 22)
    ys = np.arange(-22, h + 22)
    walk = np.concatenate([np.stack([xs + 0.6, np.full(len(xs), 30.3)], 1), np.stack([np.full(len(ys), 50.2), ys + 0.4], 1),
                           np.stack([xs[::3] + 0.1, xs[::3] * (h / w) + 0.9], 1),
                           np.stack([xs[::3] + 0.5, h - 1 - xs[::3] * (h / w)], 1)]).astype(F)
    for clamp in (1, 0):
        cases.append((f"walk35-c{clamp}", *pair, walk, 35, 64, 8, clamp))
    cases.append(("walk32-c1", *pair, walk[::2], 32, 64, 8, 1))
    cases.append(("walk5-c0", *pair, walk[::2], 5, 64, 8, 0))
    # low images: the map has fewer rows than search_y + 1 only when both ends of the search are cut
    for k in range(1, 9):
        img = texture("noise", 5 + k, 90, seed=30 + k)
        kps = np.stack([np.arange(0, 95, 4) + 0.5, np.full(24, 2.5)], 1).astype(F)
        cases.append((f"low{5 + k}x90", img, np.roll(img, 3, axis=1), kps, 5, 64, 8, 1))
    # windows and the kernel-shape switch (31 / search_y 6 is the small shape, one more of either the large)
    kps = np.stack([rng.uniform(-5, w + 5, 50), rng.uniform(-5, h + 5, 50)], 1).astype(F)
    blocks = texture("binblocks2", h, w, seed=2)
    for win, sx, sy in ((5, 3, 1), (30, 60, 6), (31, 60, 6), (31, 60, 7), (32, 60, 6), (35, 64, 8), (21, 30, 4)):
        for clamp in (1, 0):
            cases.append((f"noise-w{win}-sy{sy}-c{clamp}", *pair, kps, win, sx, sy, clamp))
        cases.append((f"blocks-w{win}-sy{sy}", blocks, subpixel(blocks, 0.0, 4.5), kps, win, sx, sy, 1))
    # every offset ties (0 against 255: the largest SSD there is, 35 x 35 x 255^2)
    c0, c77, c255 = (texture(f"const{v}", h, w) for v in (0, 77, 255))
    for name, a, b in (("const77", c77, c77), ("const0v255", c0, c255), ("const255v0", c255, c0), ("stripes", texture("stripes4_v", h, w), c77)):
        for win, sx, sy in ((35, 64, 8), (31, 60, 6)):
            cases.append((f"{name}-w{win}", a, b, kps, win, sx, sy, 1))
    real_l, real_r = (without_guard(x) for x in _real())
    rk = np.stack([rng.uniform(0, 203, 40), rng.uniform(0, 150, 40)], 1).astype(F)
    cases.append(("real-w31", real_l[100:250, 300:503], real_r[100:250, 300:503], rk, 31, 60, 6, 1))
    cases.append(("real-w35", real_l[100:250, 300:503], real_r[100:250, 300:503], rk, 35, 64, 8, 1))
    # narrower and lower than the window
    tiny = texture("noise", 20, 20, seed=5)
    tk = np.stack([rng.uniform(-3, 23, 30), rng.uniform(-3, 23, 30)], 1).astype(F)
    cases.append(("tiny20x20-w31", tiny, np.roll(tiny, 2, axis=1), tk, 31, 60, 6, 0))
    cases.append(("tiny20x20-w35", tiny, np.roll(tiny, 2, axis=1), tk, 35, 64, 8, 1))
    thin = texture("noise", 9, 40, seed=6)
    tk = np.stack([rng.uniform(-3, 43, 30), rng.uniform(-3, 12, 30)], 1).astype(F)
    cases.append(("thin9x40-w7", thin, np.roll(thin, 5, axis=1), tk, 7, 30, 4, 1))
    cases.append(("thin9x40-w21", thin, np.roll(thin, 5, axis=1), tk, 21, 30, 4, 0))      # (no template fits: all -1)
    # SSDs far above 2^24 a few units apart: integers that round to one float
    pl, pr = parity_pair(120, 200, 1)
    prng = np.random.RandomState(1)
    pk = np.stack([prng.uniform(0, 200, 300), prng.uniform(0, 120, 300)], 1).astype(F)
    for win, sy, n in ((31, 6, 300), (35, 6, 300), (31, 7, 100), (32, 6, 100), (33, 8, 100)):
        cases.append((f"parity-w{win}-sy{sy}", pl, pr, pk[:n], win, 60 if sy < 8 else 64, sy, 1))
    return cases
