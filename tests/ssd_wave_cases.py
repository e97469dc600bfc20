"""The cases and launches of tests/test_ssd_wave_gpu.py (ssd_disparity_kernel, one wavefront per keypoint, against the
four-wave kernel it replaced and against the oracle), and their geometry in plain numpy, from which
tests/test_ssd_wave_cases_cpu.py asserts that the lists hold what they are meant to hold.

Nothing here calls the HIP library or the C oracle. A case is a tuple of window_cases.ssd_cases():
(name, left, right, kps, win, search_x, search_y, clamp_half). A launch is a dict: name, win and search_y (which choose
the kernel shape), n_bound (grid x) and seqs, each dict(case, idx (keypoints of the case, in order), first, first_dev
(*first_ptr, None: no pointer), enable (None: no pointer, else the device word), layout, extra (capacity - n)).
"""
import functools

import numpy as np

import window_cases as WC

F = np.float32
SMALL_H, SMALL_W = WC.SSD_H, WC.SSD_W                  # 60 x 123
BIG_H, BIG_W = 96, 200
COUNTS = (0, 1, 63, 64, 65)
BATCHES = (1, 5, 33)
SHAPES = ((31, 6), (33, 7), (35, 8))                   # window / search_y: the small shape, and the large one with one and two row blocks
FILL = 0x7FC5A5A5                                      # a NaN no kernel computes: what an unwritten disparity word holds


def _odd_stride(w):
    s = w + 13
    while s % 4 == 0 or s % 16 == 0:
        s += 1
    return s


# name -> (first byte's offset from a dword boundary, row stride as a function of the width)
LAYOUTS = {"dense": (0, lambda w: w), "off1": (1, lambda w: (w + 3) // 4 * 4 + 16), "off2": (2, lambda w: (w + 3) // 4 * 4),
           "off3": (3, _odd_stride), "oddstride": (0, _odd_stride)}
LAYOUT_NAMES = tuple(LAYOUTS)


def shape_of(win, search_y):
    """the largest window of the kernel shape launch_ssd picks"""
    return 31 if win <= 31 and 2 * search_y + 1 <= 13 else 35


def geometry(case):
    """per keypoint, as the kernels compute them: tw, th, mw, mh, rw (0 where skipped), skipped, and whether staging
    the template / region needs a 16-byte chunk that crosses the image's right edge (edge16) and within such a
    chunk a dword that does (edge4)"""
    _, left, right, kps, win, sx, sy, clamp = case
    rows, cols = left.shape
    wb, wa = win // 2, (win + 1) // 2
    n = len(kps)
    g = {k: np.zeros(n, np.int64) for k in ("tw", "th", "mw", "mh", "rw")}
    g.update(skipped=np.ones(n, bool), edge16=np.zeros(n, bool), edge4=np.zeros(n, bool))
    for i in range(n):
        x, y = int(kps[i][0]), int(kps[i][1])
        x11, x12 = max(0, x - wb), min(cols - 1, x + wa)
        y11, y12 = max(0, y - wb), min(rows, y + wa)
        x21, x22 = x11, min(cols - 1, x + wa + sx)
        y21, y22 = max(0, y - wb - sy), min(rows - 1, y + wa + sy)
        if clamp and (x12 <= 0 or y12 <= 0 or x11 >= cols - 1 or y11 >= rows - 1):
            continue
        if clamp and (x22 <= 0 or y22 <= 0 or x21 >= cols - 1 or y21 >= rows - 1):
            continue
        tw, th, rw, rh = x12 - x11, y12 - y11, x22 - x21, y22 - y21
        mw, mh = rw - tw + 1, rh - th + 1
        if tw <= 0 or th <= 0 or mw <= 0 or mh <= 0:
            continue
        g["skipped"][i] = False
        g["tw"][i], g["th"][i], g["mw"][i], g["mh"][i], g["rw"][i] = tw, th, mw, mh, rw
        for x0, width in ((x11, tw), (x21, rw)):
            for c in range(0, width, 16):
                if x0 + c + 16 > cols:
                    g["edge16"][i] = True
                    g["edge4"][i] |= any(x0 + c + 4 * k < cols < x0 + c + 4 * k + 4 for k in range(4))
    return g


def _pair(h, w, seed):
    """random bytes, and the same moved 9 columns with a tenth of the pixels drawn again"""
    rng = np.random.RandomState(seed)
    left = rng.randint(0, 256, (h, w)).astype(np.uint8)
    right = np.where(rng.uniform(size=(h, w)) < 0.1, rng.randint(0, 256, (h, w)), np.roll(left, 9, axis=1)).astype(np.uint8)
    return left, right


def border_points(h, w):
    """keypoints 0 .. 4 px from every border and corner, a few inside, and some beyond the image on every side"""
    xs = list(range(5)) + list(range(w - 5, w)) + [40, 61]
    ys = list(range(5)) + list(range(h - 5, h)) + [30]
    grid = [(x + 0.3, y + 0.6) for y in ys for x in xs]
    outside = [(-40.0, 30.0), (w + 40.0, 30.0), (60.0, -40.0), (60.0, h + 40.0), (-16.5, 30.0), (-15.5, 30.0), (w + 14.5, 30.0),
               (w + 13.5, 30.0), (w + 15.5, 30.0), (w + 16.5, 30.0), (60.0, h + 16.5), (60.0, h + 15.5), (60.0, h + 14.5),
               (60.0, h + 13.5), (60.0, -16.5), (60.0, -15.5), (60.0, -17.5), (-17.5, 30.0)]
    return np.array(grid + outside, F)


@functools.lru_cache(maxsize=None)
def extra_cases():
    """what window_cases.ssd_cases() does not single out"""
    cases = []
    small = _pair(SMALL_H, SMALL_W, 41)
    big = _pair(BIG_H, BIG_W, 42)
    bp = border_points(SMALL_H, SMALL_W)
    for win, sy in SHAPES:
        for clamp in (1, 0):
            cases.append((f"border-w{win}-sy{sy}-c{clamp}", *small, bp, win, 60 if win == 31 else 64, sy, clamp))
    # search_x 64: the map is 65 columns wide, five column blocks, in both shapes; 200 x 96 leaves room for it
    rng = np.random.RandomState(43)
    inner = np.stack([rng.uniform(18, 118, 12), rng.uniform(26, BIG_H - 27, 12)], 1).astype(F)
    bpb = border_points(BIG_H, BIG_W)
    for win, sy in SHAPES:
        cases.append((f"big-w{win}-sy{sy}-sx64", *big, np.concatenate([inner, bpb[::5]]), win, 64, sy, 1))
    # one to five column blocks, at both ends of each block count
    for win, sy in SHAPES:
        for sx in (0, 3, 15, 16, 31, 32, 47, 48, 63):
            cases.append((f"blocks-w{win}-sy{sy}-sx{sx}", *big, inner[:8], win, sx, sy, 1))
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    return list(WC.ssd_cases()) + list(extra_cases())


def _seq(case, idx=None, first=0, first_dev=None, enable=None, layout="dense", extra=4):
    idx = np.arange(len(case[3])) if idx is None else np.asarray(idx, np.int64)
    return dict(case=case, idx=idx, first=first, first_dev=first_dev, enable=enable, layout=layout, extra=extra)


def case_by_name(name):
    return next(c for c in all_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def launches():
    out = []
    # every case as a launch of its own, the layouts going round
    for i, case in enumerate(all_cases()):
        out.append(dict(name="case-" + case[0], win=case[4], search_y=case[6], n_bound=len(case[3]),
                        seqs=[_seq(case, layout=LAYOUT_NAMES[i % len(LAYOUT_NAMES)])]))
    # keypoint counts, in both shapes
    for win, sy in ((31, 6), (35, 8)):
        case = case_by_name(f"border-w{win}-sy{sy}-c1")
        for n in COUNTS:
            out.append(dict(name=f"count{n}-w{win}", win=win, search_y=sy, n_bound=max(n, 1),
                            seqs=[_seq(case, idx=np.arange(n) * 2 % len(case[3]), layout="off3")]))
    # the tracker's form: sequences of different settings in one launch of the largest, offsets in the block and on
    # the device, a grid wider and narrower than what is left, predicates 0 and not 0
    rng = np.random.RandomState(44)
    for win, sy in ((31, 6), (35, 8)):
        pool = [c for c in all_cases() if c[4] <= win and c[6] <= sy and len(c[3]) >= 8 and c[1].shape[1] <= BIG_W]
        for batch in BATCHES:
            seqs = []
            for b in range(batch):
                case = pool[(7 * b + batch) % len(pool)]
                n = int(rng.randint(6, min(len(case[3]), 40) + 1))
                idx = rng.randint(0, len(case[3]), n)
                first = (0, 1, 3)[b % 3]
                first_dev = (None, 2, 0, 5)[b % 4]
                enable = (None, 1, 0, 0x100, None)[b % 5] if batch > 1 else None
                seqs.append(_seq(case, idx=idx, first=first, first_dev=first_dev, enable=enable,
                                 layout=LAYOUT_NAMES[b % len(LAYOUT_NAMES)], extra=b % 3))
            wide = max(len(s["idx"]) for s in seqs) + 9
            out.append(dict(name=f"tracker-w{win}-b{batch}-wide", win=win, search_y=sy, n_bound=wide, seqs=seqs))
            out.append(dict(name=f"tracker-w{win}-b{batch}-narrow", win=win, search_y=sy, n_bound=5, seqs=seqs))
    return out


def expected(seq, disparity, n_bound, stride):
    """the [stride] words of a sequence's output array after the launch: `disparity` (float32, of the sequence's
    keypoints idx) where the launch writes, FILL elsewhere"""
    out = np.full(stride, FILL, np.uint32)
    if seq["enable"] == 0:
        return out
    n = len(seq["idx"])
    lo = seq["first"] + (seq["first_dev"] or 0)
    hi = min(n, lo + n_bound)
    if hi > lo:
        out[lo:hi] = np.asarray(disparity, F)[lo:hi].view(np.uint32)
    return out
