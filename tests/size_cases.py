"""Tracker contexts at image sizes that nothing divides: named cases (a preset of synth.CONFIGS plus overrides,
a seed, a motion scale and a frame count) and the oracle's run over each. The sizes are chosen so that, inside a
ctx, the two pyramid rounding rules (halfSample: floor, pyrDown: ceil) disagree, no row is a whole number of
dwords, grid cells are partial, and the LK level count falls below SVO_LK_LEVELS. test_sizes_cpu.py asserts what
each case reaches from the oracle alone; test_sizes_gpu.py plays the same sequences through the HIP ctx."""
import functools

import numpy as np

import oracle_py as O
from stereo_svo_slam_amd import synth
import util

CASES = {
    # odd both ways: w % 4 == 3, level 1 of the alignment pyramid 161x122 against pyrDown's 162x123
    "odd323": dict(preset="tiny", overrides=dict(width=323, height=245, cx=161.0, cy=122.0),
                   seed=1, motion=4.0, frames=30),
    # even size whose half is odd: w % 4 == 2, level 1 is 161x121
    "half322": dict(preset="tiny", overrides=dict(width=322, height=242, cx=161.0, cy=121.0),
                    seed=1, motion=4.0, frames=30),
    # w % 4 == 1 and a non-square grid that divides neither dimension: partial cells, cells != merge_cells
    "cells321": dict(preset="tiny", overrides=dict(width=321, height=247, cx=160.0, cy=123.0,
                                                   grid_width=37, grid_height=29),
                     seed=1, motion=4.0, frames=30),
    # a dense grid: more than 128 keypoints, some of them tracked outside the image
    "dense327": dict(preset="tiny", overrides=dict(width=327, height=241, cx=163.0, cy=120.0,
                                                   grid_width=24, grid_height=20),
                     seed=3, motion=4.0, frames=30),
    # small against the KLT window: two LK levels
    "lk2_167": dict(preset="tiny", overrides=dict(width=167, height=123, fx=110.0, fy=110.0, cx=83.0, cy=61.0,
                                                  grid_width=16, grid_height=16, window_size_opt_flow=31),
                    seed=1, motion=4.0, frames=30),
    # one LK level, two alignment levels
    "lk1_61": dict(preset="tiny", overrides=dict(width=61, height=47, fx=40.0, fy=40.0, cx=30.0, cy=23.0,
                                                 grid_width=8, grid_height=6, window_size_opt_flow=31,
                                                 window_size_depth_calculator=9, search_x=10,
                                                 max_pyramid_levels=2, min_pyramid_level_pose_estimation=0),
                   seed=1, motion=2.0, frames=20),
    # the C2 preset three pixels short each way: six levels, floor and ceil differ from level 1 on
    "euroc749": dict(preset="euroc", overrides=dict(width=749, height=477),
                     seed=5, motion=3.0, frames=8),
}


def config(name, **more):
    c = CASES[name]
    return dict(synth.CONFIGS[c["preset"]], **c["overrides"], **more)


def floor_dims(cfg):
    """(w, h) of every alignment pyramid level (halfSample: floor)"""
    return [(cfg["width"] >> l, cfg["height"] >> l) for l in range(cfg["max_pyramid_levels"])]


def ceil_dims(cfg, levels):
    """(w, h) of `levels` levels of pyrDown ((n + 1) / 2)"""
    w, h, out = cfg["width"], cfg["height"], []
    for _ in range(levels):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def grid_cells(cfg):
    """(cells of the detector's grid, cells of the merge's occupancy grid, which follows the reference's swapped
    grid_height / grid_width: depth_calculator.cpp:90,180)"""
    w, h, gw, gh = cfg["width"], cfg["height"], cfg["grid_width"], cfg["grid_height"]
    return (w // gw) * (h // gh), ((w + gh - 1) // gh) * ((h + gw - 1) // gw)


def sequence(name, n_frames=None, seed=None):
    """(cfg, lefts, rights, timestamps) of a case as numpy arrays, rendered on the CPU"""
    c = CASES[name]
    return _sequence(name, c["frames"] if n_frames is None else n_frames, c["seed"] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _sequence(name, n_frames, seed):
    c = CASES[name]
    cfg, L, R, poses, ts = synth.make_sequence(c["preset"], n_frames, seed, device="cpu", motion_scale=c["motion"],
                                               overrides=c["overrides"])
    L, R = np.stack([x.numpy() for x in L]), np.stack([x.numpy() for x in R])
    L.setflags(write=False); R.setflags(write=False)
    return cfg, L, R, ts


def oracle_run(name, n_frames=None, seed=None):
    """The oracle over a case: per frame (keyframe made, kps2d, kps3d, info, pose, stats), and per keyframe
    (kps2d, kps3d, info, pose). Computed once per (case, length, seed); shared, so leave it unchanged."""
    c = CASES[name]
    return _oracle_run(name, c["frames"] if n_frames is None else n_frames, c["seed"] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _oracle_run(name, n_frames, seed):
    cfg, L, R, ts = _sequence(name, n_frames, seed)
    ref = O.Slam(util.oracle_camera(cfg))
    frames = []
    for k in range(n_frames):
        made = ref.new_image(L[k], R[k], float(ts[k]))
        k2, k3, info = ref.keypoints()
        frames.append((made, k2, k3, info, ref.pose().copy(), ref.stats()))
    keyframes = [ref.keyframe(kid) for kid in range(ref.num_keyframes())]
    ref.close()
    return frames, keyframes
