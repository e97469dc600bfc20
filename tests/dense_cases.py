"""Crafted stereo pairs for the dense disparity map (tests/test_dense_cpu.py, tests/test_dense_gpu.py), seeded and
small: name -> (left, right, win, search_x, search_y, step). What each one is for is said in CASES' comments and
asserted in tests/test_dense_cpu.py."""
import functools

import numpy as np

import dense_ref as DR


def _random(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _case_a():
    left = _random(1, 97, 53)
    return left, np.roll(left, 5, axis=1)          # right = left rolled by 5: the minimum sits at j = 5 and is 0


def _case_e():
    rng = np.random.default_rng(5)
    return (rng.integers(0, 2, (48, 80)) * 255).astype(np.uint8), (rng.integers(0, 2, (48, 80)) * 255).astype(np.uint8)


def _case_d():
    col = np.array([10, 200, 60, 130], np.uint8)
    img = np.tile(col, (40, 16))
    return img, img.copy()


@functools.lru_cache(maxsize=None)
def cases():
    a = _case_a()
    f = _random(6, 64, 20)
    return {
        "a": (*a, 7, 9, 2, 1),                                              # plain: a shifted random image, odd sizes
        "b": (*a, 6, 9, 2, 3),                                              # even window; the step does not divide the size
        "c": (np.full((40, 64), 77, np.uint8), np.full((40, 64), 77, np.uint8), 7, 9, 2, 1),   # every candidate ties
        "d": (*_case_d(), 7, 12, 2, 1),                                     # period-4 columns: ties at several j
        "e": (*_case_e(), 35, 64, 8, 4),                                    # the entry's limits; minima >= 2^24
        "f": (f, np.roll(f, 3, axis=1), 31, 60, 6, 1),                      # template clipped top and bottom
    }


@functools.lru_cache(maxsize=None)
def reference(name):
    """dense_ref's [2, rows, cols] disparity and cost planes of a case, computed once and shared (read-only)"""
    left, right, win, sx, sy, step = cases()[name]
    out = DR.planes(left, right, win, sx, sy, step, DR.DISPARITY, True)
    out.setflags(write=False)
    return out
