"""Crafted stereo pairs for the left-right cross-check (tests/test_lr_cpu.py, tests/test_lr_gpu.py), seeded and small:
name -> (left, right, win, search_x, search_y, step). The six pairs of tests/dense_cases.py, an occlusion (a
foreground block in front of a shifted background: a half-occluded band lies left of it) and a wide, odd pair whose
width spans two column tiles, so that a seam of the mirrored tiles lies inside. What each one reaches is asserted in
tests/test_lr_cpu.py."""
import functools

import numpy as np

import dense_cases as DC
import dense_ref as DR
import lr_ref as LR


def _occl():
    rng = np.random.default_rng(11)
    bg = rng.integers(0, 256, (40, 128))
    fg = rng.integers(0, 256, (40, 128))
    left = bg[:, :96].astype(np.uint8)
    right = np.roll(bg, 3, axis=1)[:, :96].astype(np.uint8)
    left[8:32, 40:60] = fg[8:32, 40:60]
    right[8:32, 49:69] = fg[8:32, 40:60]
    return left, right


def _wide():
    left = np.random.default_rng(21).integers(0, 256, (21, 301)).astype(np.uint8)
    return left, np.roll(left, 4, axis=1)


@functools.lru_cache(maxsize=None)
def cases():
    occl, wide = _occl(), _wide()
    out = dict(DC.cases())
    out.update({
        "occl1": (*occl, 7, 12, 1, 1),
        "occl3": (*occl, 6, 12, 1, 3),
        "wide1": (*wide, 5, 6, 1, 1),
        "wide2": (*wide, 6, 6, 1, 2),
    })
    return out


# kept share, share of -2 and share above the tolerance at max_lr_diff = 1, computed with the numpy statement
SHARES = {
    "occl1": (0.787, 0.010, 0.203), "occl3": (0.800, 0.0, 0.200), "wide1": (0.880, 0.003, 0.117), "wide2": (0.912, 0.0, 0.088),
    "a": (0.822, 0.010, 0.167), "b": (0.906, 0.0, 0.094), "c": (0.734, 0.016, 0.250), "d": (0.594, 0.016, 0.391),
    "f": (0.112, 0.006, 0.282),
}


@functools.lru_cache(maxsize=None)
def forward(name):
    """dense_ref's [2, rows, cols] disparity and cost planes of a case, computed once and shared (read-only)"""
    if name in DC.cases():
        return DC.reference(name)
    left, right, win, sx, sy, step = cases()[name]
    out = DR.planes(left, right, win, sx, sy, step, DR.DISPARITY, True)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """lr_ref's lr plane [rows, cols] of a case, computed once and shared (read-only)"""
    left, right, win, sx, sy, step = cases()[name]
    out = LR.lr_plane(left, right, win, sx, sy, step, forward(name)[0])
    out.setflags(write=False)
    return out
