"""Crafted 8-bit images, the shapes that reach every path of csrc/pyramid.hip, and plain int64 numpy statements
of the two pyramids, shared by tests/test_pyramid_cpu.py and tests/test_pyramid_gpu.py.

Nothing here calls the HIP library or the C oracle.

  halfSample (stereo_slam.cpp:93-121): the truncating mean of 2 x 2 blocks, sizes halved rounding down;
  pyrDown (cv::buildOpticalFlowPyramid's image part): the 5 x 5 outer product of [1 4 6 4 1] over the image padded
  with np.pad(mode="reflect") (BORDER_REFLECT_101), (v + 128) >> 8, sizes halved rounding up.

Seams of the kernels that the shapes and the impulses are placed on: the tile kernel's 64 x 64 tile (x, y = 63 | 64);
the stream kernel's 8-pixel unit (x = 7 | 8), its column block of 56 units (x = 447 | 448) and its row blocks of 32 and
64 rows (y = 31 | 32, 63 | 64); the last two rows and columns, where BORDER_REFLECT_101 substitutes taps."""
import collections
import functools

import numpy as np

K5 = np.array([1, 4, 6, 4, 1], np.int64)


# ------------------------------------------------------------------ the two operations, plainly
def half_sample_sums(img):
    """int64 [h // 2, w // 2]: a + b + c + d of every 2 x 2 block"""
    h, w = img.shape[0] // 2 * 2, img.shape[1] // 2 * 2
    a = img[:h, :w].astype(np.int64)
    return a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]


def half_sample_chain(img, n_levels):
    """(levels, sums): levels[0] = img, levels[l] = sums[l] // 4 as uint8; sums[0] is None"""
    levels, sums = [np.asarray(img, np.uint8)], [None]
    for _ in range(1, n_levels):
        s = half_sample_sums(levels[-1])
        sums.append(s)
        levels.append((s // 4).astype(np.uint8))
    return levels, sums


def pyr_down_sums(img):
    """int64 [(h + 1) // 2, (w + 1) // 2]: the 25 weighted taps around every even pixel, before + 128 and >> 8"""
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    p = np.pad(img.astype(np.int64), 2, mode="reflect")
    v = np.zeros((oh, ow), np.int64)
    for a in range(5):
        for b in range(5):
            v += K5[a] * K5[b] * p[a:a + 2 * oh:2, b:b + 2 * ow:2]
    return v


def lk_level_count(h, w, win, max_levels=3):
    """cv::buildOpticalFlowPyramid stops when the next level is not larger than the window"""
    for l in range(max_levels):
        h, w = (h + 1) // 2, (w + 1) // 2
        if w <= win or h <= win:
            return l + 1
    return max_levels


def pyr_down_chain(img, win):
    """(levels, sums) of the LK pyramid: levels[0] = img, levels[l] = (sums[l] + 128) >> 8"""
    levels, sums = [np.asarray(img, np.uint8)], [None]
    for _ in range(1, lk_level_count(*img.shape, win)):
        s = pyr_down_sums(levels[-1])
        sums.append(s)
        levels.append(((s + 128) >> 8).astype(np.uint8))
    return levels, sums


# ------------------------------------------------------------------ shapes
# kernel: the value of SVO_PYR_KERNEL ("stream": no effect; "64": 64-row blocks; "tile": the tile kernel).
# runs: the kernel that a dense, 8-byte aligned image of the shape takes.
Case = collections.namedtuple("Case", "h w n_levels kernel runs")

CASES = (
    Case(16, 16, 4, "stream", "stream32"),       # the minimum
    Case(30, 16, 4, "stream", "stream32"),       # shorter than a row block
    Case(34, 456, 6, "stream", "stream32"),      # a row block + 2 rows; h1 = 17, h2 = 9; 57 units: a second column block of one
    Case(32, 448, 6, "stream", "stream32"),      # exactly 56 units, exactly one row block
    Case(62, 464, 6, "stream", "stream32"),      # h1 = 31; two units in the second column block
    Case(66, 904, 6, "stream", "stream32"),      # three row blocks, 113 units: three column blocks
    Case(64, 64, 7, "stream", "stream64"),       # seven levels: 64-row blocks
    Case(96, 128, 7, "stream", "stream64"),      # ... and a partial second block
    Case(16, 16, 4, "64", "stream64"),
    Case(30, 16, 4, "64", "stream64"),
    Case(34, 456, 6, "64", "stream64"),
    Case(32, 448, 6, "64", "stream64"),
    Case(65, 129, 6, "stream", "tile"),          # one pixel into a second tile both ways
    Case(63, 127, 6, "stream", "tile"),
    Case(131, 203, 7, "stream", "tile"),
    Case(17, 19, 4, "stream", "tile"),
    Case(64, 64, 7, "tile", "tile"),
    Case(34, 456, 6, "tile", "tile"),
)


def case_id(c):
    return f"{c.h}x{c.w}-{c.n_levels}-{c.kernel}"


def lk_window(h, w):
    """the LK window (3 or 5) at which the shape has three LK levels"""
    win = 3 if min(h, w) < 24 else 5
    assert lk_level_count(h, w, win) == 3
    return win


# first byte's offset from an 8-byte boundary and row stride of tests/test_keyframe_gpu.py's `place` layouts
def layout_of(name, w):
    up4 = (w + 3) // 4 * 4
    odd = w + 13 if (w + 13) % 4 else w + 14
    return {"dense": (0, w), "strided": (0, up4 + 16), "off3": (3, odd), "oddstride": (0, odd)}[name]


def expected_kernel(h, w, n_levels, kernel, offset=0, stride=None):
    """pyr_stream_rows + launch_pyr_fused for a level 0 (or ingest source) at `offset` bytes past an 8-byte boundary
    with that row stride; every buffer the library allocates itself is aligned"""
    stride = w if stride is None else stride
    if w % 8 or h % 2 or w < 16 or h < 16 or offset % 8 or stride % 8 or kernel == "tile":
        return "tile"
    return "stream64" if n_levels > 6 or kernel == "64" else "stream32"


# ------------------------------------------------------------------ images
ROUNDING_VALUES = np.array([0, 1, 2, 3, 252, 253, 254, 255], np.uint8)

# Seeds of the "edges of rounding" family per shape, found by a greedy seeded search (tests/test_pyramid_cpu.py
# asserts what they reach). One image cannot reach every condition at every shape: a level of fewer than four
# pixels does not hold four residues of the halfSample sum, and a 4 x 4 level seldom holds both pyrDown residues,
# so the family is a few images per shape and the conditions hold over them together.
ROUNDING_SEEDS = {(16, 16): (0, 1, 2, 5, 7, 22), (30, 16): (0, 2, 7, 20), (34, 456): (0,), (32, 448): (0,),
                  (62, 464): (0,), (66, 904): (0,), (64, 64): (0, 1, 3, 4, 6), (96, 128): (0, 1, 5), (65, 129): (0,),
                  (63, 127): (0, 2, 4), (131, 203): (0, 1), (17, 19): (0, 1, 2, 3, 6)}


def rounding_image(h, w, seed):
    return ROUNDING_VALUES[np.random.RandomState(1000 + seed).randint(0, 8, (h, w))]


def _const(v):
    return lambda h, w, seed=0: np.full((h, w), v, np.uint8)


def _pattern(f):
    def make(h, w, seed=0):
        y, x = np.mgrid[0:h, 0:w]
        return np.ascontiguousarray(f(y, x, h, w), dtype=np.uint8)
    return make


FAMILIES = {
    "const0": _const(0), "const255": _const(255), "const77": _const(77),
    "checker1": _pattern(lambda y, x, h, w: ((x + y) % 2) * 255),
    "checker2": _pattern(lambda y, x, h, w: ((x // 2 + y // 2) % 2) * 255),
    "checker4": _pattern(lambda y, x, h, w: ((x // 4 + y // 4) % 2) * 255),
    "rows1": _pattern(lambda y, x, h, w: (y % 2) * 255 + 0 * x),
    "rows2": _pattern(lambda y, x, h, w: (y // 2 % 2) * 255 + 0 * x),
    "cols1": _pattern(lambda y, x, h, w: (x % 2) * 255 + 0 * y),
    "cols2": _pattern(lambda y, x, h, w: (x // 2 % 2) * 255 + 0 * y),
    "ramp_x": _pattern(lambda y, x, h, w: x * 255 // max(w - 1, 1) + 0 * y),
    "ramp_y": _pattern(lambda y, x, h, w: y * 255 // max(h - 1, 1) + 0 * x),
    "noise": lambda h, w, seed=0: np.random.RandomState(77 + seed).randint(0, 256, (h, w)).astype(np.uint8),
}


def impulse_positions(h, w):
    """(y, x) of the impulses: corners, edge middles, both sides of every seam, the last two rows and columns"""
    my, mx = h // 2, w // 2
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, mx), (h - 1, mx), (my, 0), (my, w - 1)]
    pos += [(my, x) for x in (7, 8, 63, 64, 447, 448) if x < w]
    pos += [(y, mx) for y in (31, 32, 63, 64) if y < h]
    pos += [(h - 2, mx), (my, w - 2), (h - 2, w - 2)]
    return list(dict.fromkeys(pos))


def impulse(h, w, y, x, white):
    """a single 255 on black, or a single 0 on white"""
    img = np.full((h, w), 255 if white else 0, np.uint8)
    img[y, x] = 0 if white else 255
    return img


@functools.lru_cache(maxsize=None)
def images(h, w):
    """name -> image: every family at this shape, in a fixed order; the arrays are read-only"""
    out = {name: make(h, w, 0) for name, make in FAMILIES.items()}
    for seed in ROUNDING_SEEDS[(h, w)]:
        out[f"rounding{seed}"] = rounding_image(h, w, seed)
    for y, x in impulse_positions(h, w):
        out[f"black_y{y}x{x}"] = impulse(h, w, y, x, False)
        out[f"white_y{y}x{x}"] = impulse(h, w, y, x, True)
    for a in out.values():
        a.setflags(write=False)
    return out


def rounding_coverage(img, n_levels, win):
    """what one image reaches: {("hs", level, sum % 4)} and {("pd", level, 127 | 128)}"""
    got = set()
    for l, s in enumerate(half_sample_chain(img, n_levels)[1]):
        if s is not None:
            got |= {("hs", l, int(r)) for r in np.unique(s % 4)}
    for l, s in enumerate(pyr_down_chain(img, win)[1]):
        if s is not None:
            got |= {("pd", l, int(r)) for r in np.unique(s & 255) if r in (127, 128)}
    return got


def rounding_goal(n_levels, n_lk=3):
    return ({("hs", l, r) for l in range(1, n_levels) for r in range(4)} |
            {("pd", l, r) for l in range(1, n_lk) for r in (127, 128)})


def find_rounding_seeds(h, w, n_levels, limit=20000):
    """the greedy search that made ROUNDING_SEEDS: a seed is kept if it reaches something new"""
    goal, have, seeds = rounding_goal(n_levels), set(), []
    for seed in range(limit):
        new = rounding_coverage(rounding_image(h, w, seed), n_levels, lk_window(h, w)) & goal
        if not new <= have:
            have |= new
            seeds.append(seed)
        if have == goal:
            return seeds
    raise AssertionError(f"{h} x {w}: {sorted(goal - have)} not reached")
