"""Crafted cases for the dense point cloud (tests/test_cloud_cpu.py, tests/test_cloud_gpu.py) on the pairs of
tests/dense_cases.py: name -> dict(left, right, win, search_x, search_y, step, rig, pose, filter). What each one is for
is said in CASES' comments and asserted in tests/test_cloud_cpu.py."""
import functools

import numpy as np

import cloud_ref as CR
import dense_cases as DC
import dense_ref as DR

# two cameras: a centred one with square pixels, and one with the principal point off centre and fx != fy
RIG_CENTRED = dict(fx=200.0, fy=200.0, cx=48.0, cy=26.0, baseline=20.0)
RIG_SKEWED = dict(fx=212.0, fy=198.5, cx=41.25, cy=30.75, baseline=23.5)
# two poses: zero, and a general one with all six components non-zero
POSE_ZERO = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
POSE_GENERAL = (0.3, -0.2, 1.1, 0.05, -0.12, 0.2)
NO_FILTER = dict(min_disparity=0.0, max_depth=0.0, max_mean_cost=0.0)


def _case(pair, rig, pose, dense=None, **filter):
    left, right, win, sx, sy, step = DC.cases()[pair]
    if dense is not None:
        win, sx, sy, step = dense
    return dict(pair=pair, left=left, right=right, win=win, search_x=sx, search_y=sy, step=step, rig=rig, pose=pose,
                filter=dict(NO_FILTER, **filter))


@functools.lru_cache(maxsize=None)
def cases():
    same = dict(_case("a", RIG_SKEWED, POSE_GENERAL, dense=(7, 9, 2, 3)))
    same["right"] = same["left"].copy()                     # right = left: every disparity is 0 and is clamped to 0.5
    same["pair"] = None
    return {
        # 97 x 53 at step 1: 5141 lattice points = 20 tiles and 21 points; nothing is filtered: keeps all
        "all": _case("a", RIG_CENTRED, POSE_GENERAL),
        # even window, a step that does not divide the size; min_disparity above the search range: keeps none
        "none": _case("b", RIG_SKEWED, POSE_ZERO, min_disparity=100.0),
        # random binary pair with the entry's limits: disparities all over 0 .. 64. min_disparity = 4 is the median and
        # a value many points have exactly: they stay (the comparison is <)
        "disparity": _case("e", RIG_SKEWED, POSE_GENERAL, min_disparity=4.0),
        # ... so depths all over; 5.875 = 23.5 / 4 is the depth of those points: they stay (the comparison is >)
        "depth": _case("e", RIG_SKEWED, POSE_ZERO, max_depth=5.875),
        # ... and minima all over: costs >= 2^24, templates clipped on every side
        "cost": _case("e", RIG_CENTRED, POSE_GENERAL, max_mean_cost=30000.0),
        # all three at once
        "three": _case("e", RIG_SKEWED, POSE_GENERAL, min_disparity=4.0, max_depth=20.0, max_mean_cost=30000.0),
        # period-4 columns, 64 x 40 at step 1: 2560 points, exactly 10 tiles; ties average to fractional disparities
        "ties": _case("d", RIG_CENTRED, POSE_GENERAL, max_depth=4.0),
        # invalid points (template clipped top and bottom), nothing filtered: every valid point stays
        "invalid": _case("f", RIG_SKEWED, POSE_GENERAL),
        "clamped": same,
    }


FILTERED = ("disparity", "depth", "cost", "three", "ties")    # these keep some and drop some of their valid points


@functools.lru_cache(maxsize=None)
def planes(name):
    """dense_ref's [2, rows, cols] disparity and cost planes of a case, computed once and shared (read-only)"""
    c = cases()[name]
    left, right, win, sx, sy, step = DC.cases()[c["pair"]] if c["pair"] else (None,) * 6
    if c["pair"] and (win, sx, sy, step) == (c["win"], c["search_x"], c["search_y"], c["step"]):
        return DC.reference(c["pair"])
    out = DR.planes(c["left"], c["right"], c["win"], c["search_x"], c["search_y"], c["step"], DR.DISPARITY, True)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, frame, layout):
    """(records, n_points) of cloud_ref for a case, computed once and shared (read-only)"""
    c = cases()[name]
    rec, n = CR.cloud(c["left"], planes(name), c["win"], c["step"], c["rig"], c["pose"], frame, layout, **c["filter"])
    rec.setflags(write=False)
    return rec, n
