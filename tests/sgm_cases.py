"""Crafted inputs for semi-global aggregation (tests/test_sgm_cpu.py, tests/test_sgm_gpu.py), seeded and small.
PAIRS: name -> (left, right, win, search_x, search_y, step, p1, p2, cost_cap) for the cost volume and the whole map;
VOLUMES: name -> (C uint16 [rows, cols, D], count uint16 [rows, cols], p1, p2, cost_cap) for the aggregator alone.
What each one is for is said in the comments and asserted in tests/test_sgm_cpu.py. The references are computed once
and shared, read-only."""
import functools

import numpy as np

import dense_cases as DC
import sgm_ref as SR

BAND_COLS, BAND_ROWS, BAND_TRUTH = (44, 60), (4, 36), 6    # the band's points that are judged, and the true disparity
SLOW = ("wide",)                                           # pairs whose yardstick is the second formulation


def flat_band(seed=7, sigma=2.0, w=96, h=40, shift=BAND_TRUTH):
    """noise at true disparity `shift` with a constant band in left columns 40 .. 63, Gaussian noise on both images"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (h, w)).astype(np.float64)
    left[:, 40:64] = 128.0
    right = np.roll(left, shift, axis=1)                   # R[y][x + shift] = L[y][x]
    noisy = lambda a: np.clip(np.rint(a + rng.normal(0.0, sigma, a.shape)), 0, 255).astype(np.uint8) if sigma > 0 else a.astype(np.uint8)
    return noisy(left), noisy(right)


def band_score(disparity):
    """the share of the band's judged points within 1 px of the truth"""
    d = disparity[BAND_ROWS[0]:BAND_ROWS[1], BAND_COLS[0]:BAND_COLS[1]]
    return float((np.abs(d - BAND_TRUTH) <= 1.0).mean())


def _binary(seed, w, h):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def _flipped(seed, w, h, shift, share):
    """0 / 255 noise and its copy rolled by `shift` with `share` of the pixels flipped"""
    rng = np.random.default_rng(seed)
    left = _binary(seed + 1, w, h)
    flip = rng.random((h, w)) < share
    return left, np.where(flip, 255 - np.roll(left, shift, axis=1), np.roll(left, shift, axis=1)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pairs():
    dc = DC.cases()
    wide = np.random.default_rng(11).integers(0, 256, (24, 300), dtype=np.uint8)
    return {
        "band": (*flat_band(), 7, 15, 1, 1, 32, 256, 4095),                     # the purpose: a flat band inside texture
        "b": (*dc["b"][:2], 6, 9, 2, 3, 32, 256, 4095),                          # even window; the step does not divide the size
        "f": (*dc["f"][:2], 31, 60, 6, 1, 16, 128, 4095),                        # 64 x 20: template clipped top and bottom
        "wide": (wide, np.roll(wide, 9, axis=1), 7, 63, 1, 1, 32, 256, 4095),    # D = 64 across a tile boundary of 256 columns
        "e": (_binary(5, 80, 48), _binary(6, 80, 48), 35, 63, 8, 4, 32, 383, 16000),   # raw sums pass 2^24, the cap bites
        "e2": (*_flipped(8, 80, 48, 5, 0.235), 35, 63, 8, 8, 32, 383, 16000),     # raw sums pass 2^24 below the cap
    }


def _volume(seed, cols, rows, D, cap, low, p1, p2, counts=True):
    """a volume of entries near `cap` with a share `low` of entries near 0, and a count plane that holds 0, 1 and D"""
    rng = np.random.default_rng(seed)
    C = np.where(rng.random((rows, cols, D)) < low, rng.integers(0, min(cap, 40) + 1, (rows, cols, D)),
                 rng.integers(max(cap - 300, 0), cap + 1, (rows, cols, D))).astype(np.uint16)
    count = rng.integers(0, D + 1, (rows, cols)).astype(np.uint16)
    count.flat[rng.integers(0, count.size)] = D
    return C, (count if counts else None), p1, p2, cap


@functools.lru_cache(maxsize=None)
def volumes():
    tie = np.array([[[5, 3, 3, 7]]], np.uint16)            # one point, S = 4 C: a tie at j = 1, 2 and an offset of + 0.5
    small = np.random.default_rng(3).integers(0, 4, (7, 5, 3)).astype(np.uint16)
    return {
        "1x1x1": (np.array([[[9]]], np.uint16), np.array([[1]], np.uint16), 1, 1, 100),
        "tie": (tie, np.array([[4]], np.uint16), 1, 2, 100),
        "5x7x3": (small, np.random.default_rng(4).integers(0, 4, (7, 5)).astype(np.uint16), 1, 2, 3),   # small numbers: ties of S
        "3x70x64": _volume(21, 3, 70, 64, 16000, 0.3, 5, 383),                  # cost_cap + p2 = 16383: S above 60 000
        "70x3x64": _volume(22, 70, 3, 64, 16000, 0.3, 200, 383),
        "9x9x33": _volume(23, 9, 9, 33, 4095, 0.5, 32, 256),
    }


@functools.lru_cache(maxsize=None)
def pair_volume(name):
    """(C, count) of a pair by the statement (SLOW pairs: by the second formulation)"""
    left, right, win, sx, sy, step, p1, p2, cap = pairs()[name]
    C, count = (SR.cost_volume_fast if name in SLOW else SR.cost_volume)(left, right, win, sx, sy, step, cap)
    C.setflags(write=False)
    count.setflags(write=False)
    return C, count


@functools.lru_cache(maxsize=None)
def pair_sums(name):
    left, right, win, sx, sy, step, p1, p2, cap = pairs()[name]
    S = (SR.sums_fast if name in SLOW else SR.sums)(pair_volume(name)[0].astype(np.int64), p1, p2)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def pair_reference(name, subpixel=True, value=SR.DISPARITY, baseline=1.0):
    """[2, rows, cols]: the value and cost planes of a pair"""
    out = SR.value_planes(pair_sums(name), pair_volume(name)[1], subpixel, value, True, baseline)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def volume_sums(name):
    C, count, p1, p2, cap = volumes()[name]
    S = SR.sums(np.minimum(C.astype(np.int64), cap), p1, p2)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def volume_reference(name, subpixel=True, value=SR.DISPARITY, baseline=1.0, counts=True):
    C, count, p1, p2, cap = volumes()[name]
    out = SR.value_planes(volume_sums(name), count if counts else None, subpixel, value, True, baseline)
    out.setflags(write=False)
    return out
