"""Crafted pairs for the cross-check of SGM maps (tests/test_sgm_lr_cpu.py, tests/test_sgm_lr_gpu.py), seeded and small:
name -> (left, right, win, search_x, search_y, step, p1, p2, cost_cap). What each one reaches is asserted in
tests/test_sgm_lr_cpu.py. The references are computed once with the second formulation of tests/sgm_ref.py (tied to the
first there) and shared, read-only."""
import functools

import numpy as np

import sgm_cases as SC
import sgm_lr_ref as SLR

SETTINGS = (7, 15, 1)                                      # window, search_x, search_y of the occlusion scene
PENALTIES = (32, 256, 4095)
SEEDS, STEPS = (3, 4, 5), (1, 2, 4)
SCENE = dict(w=96, h=40, dbg=3, dfg=10, a=30, b=54, y0=8, y1=32)


def occlusion_scene(seed, w=96, h=40, dbg=3, dfg=10, a=30, b=54, y0=8, y1=32, sigma=2.0):
    """a textured foreground rectangle at disparity dfg over a textured background at disparity dbg; (left, right, truth)"""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (h, w)).astype(np.float64); fg = rng.integers(0, 256, (h, w)).astype(np.float64)
    left = bg.copy(); left[y0:y1, a:b] = fg[y0:y1, a:b]
    right = np.roll(bg, dbg, axis=1); right[y0:y1, a + dfg:b + dfg] = fg[y0:y1, a:b]
    noisy = lambda v: np.clip(np.rint(v + rng.normal(0, sigma, v.shape)), 0, 255).astype(np.uint8)   # left first, then right
    truth = np.full((h, w), float(dbg)); truth[y0:y1, a:b] = dfg
    return noisy(left), noisy(right), truth


def _clamp_pair():
    """71 x 40 at step 8: 71 % 8 == 7 >= 2 + 8 / 2, so columns 64 .. 70 lie beyond the last cell of the mirrored lattice;
    true disparity 1, so that the point at ix = 0 (x = 4) is matched to xr = 5 and looks up column 65"""
    left = np.random.default_rng(31).integers(0, 256, (40, 71)).astype(np.uint8)
    return left, np.roll(left, 1, axis=1)


def _thin_pair():
    """40 x 12 at window 1: the last column and the last row are invalid points; right = left, so j0 = 0 (disp = 0.5)"""
    rng = np.random.default_rng(32)
    left = rng.integers(0, 256, (12, 40)).astype(np.uint8)
    right = left.copy()
    right[:, 20:] = np.roll(left, 2, axis=1)[:, 20:]
    return left, right


@functools.lru_cache(maxsize=None)
def cases():
    P = SC.pairs()
    out = {f"occl{seed}s{step}": (*occlusion_scene(seed)[:2], *SETTINGS, step, *PENALTIES) for seed in SEEDS for step in STEPS}
    out.update({
        "b": P["b"],                                                             # the step does not divide the size
        "f": P["f"],                                                             # clipped templates
        "wide": P["wide"],                                                       # D = 64 across the 256-column tile boundary
        "clamp": (*_clamp_pair(), 7, 9, 1, 8, *PENALTIES),                       # ixm is clamped to cols - 1
        "thin": (*_thin_pair(), 1, 5, 1, 1, 8, 64, 4095),                        # invalid points, j0 = 0
    })
    return out


GPU_CASES = ("occl3s1", "occl3s4", "b", "f", "wide", "clamp", "thin")           # what the stage entry is run on


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def forward(name, subpixel=True):
    """[2, rows, cols]: the SGM disparity and cost planes of a case"""
    left, right, win, sx, sy, step, p1, p2, cap = cases()[name]
    return _frozen(SLR.disparity(left, right, win, sx, sy, step, p1, p2, cap, subpixel, fast=True))


@functools.lru_cache(maxsize=None)
def reverse(name, subpixel=True):
    """[rows, cols]: the SGM disparity plane of the mirrored pair of a case"""
    left, right, win, sx, sy, step, p1, p2, cap = cases()[name]
    return _frozen(SLR.reverse(left, right, win, sx, sy, step, p1, p2, cap, subpixel, fast=True))


@functools.lru_cache(maxsize=None)
def reference(name, subpixel=True):
    """[rows, cols]: the lr plane of a case"""
    left, step = cases()[name][0], cases()[name][5]
    return _frozen(SLR.lr_plane_fast(forward(name, subpixel)[0], reverse(name, subpixel), left.shape[1], step))
