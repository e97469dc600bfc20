"""What the SGM forms of the cloud's consumers are for, on the references alone: a textured plane whose
disparity runs from D0 to D1 over the image's width, searched by the winner-takes-all statement (tests/dense_ref.py) and
by the sub-pixel SGM statement (tests/sgm_ref.py), each cloud fused once into a voxel map (tests/voxel_ref.py), and the
depth of the voxel points judged against the true plane. The scene is not tuned: the generator is the one the issue
states."""
import numpy as np

import cloud_ref as CR
import dense_ref as DR
import sgm_lr_ref as SLR
import sgm_ref as SR
import voxel_ref as VR

W, H, D0, D1, SIGMA = 160, 40, 4.0, 9.0, 1.0
K = (D1 - D0) / W                                          # the truth: d(x) = D0 + K x
WIN, SEARCH_X, SEARCH_Y, STEP = 7, 15, 1, 4
PENALTIES = (64, 256, 4095)
MIN_DISPARITY = 2.0
RIG = dict(fx=100.0, fy=100.0, cx=80.0, cy=20.0, baseline=40.0)
POSE = np.zeros(6, np.float32)
LOG2 = 14
VOXELS = (0.05, 0.1, 0.2)
SEEDS = (3, 4, 5)
INTERIOR = (16, 120, 8, 32)                                # 16 < px < 120 and 8 < py < 32


def plane_pair(seed):
    """(L, R) uint8 [H, W]: T(y, x) interpolates a row of random texture linearly at (x + 16) / 2; L = T(y, x),
    R = T(y, (x - D0) / (1 + K)); Gaussian noise of SIGMA, L first; rounded and clipped"""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H, 98)).astype(np.float64)

    def T(x):
        u = (x + 16.0) / 2.0
        i = np.clip(np.floor(u).astype(np.int64), 0, tex.shape[1] - 2)
        f = u - i
        return tex[:, i] * (1.0 - f)[None, :] + tex[:, i + 1] * f[None, :]

    x = np.arange(W, dtype=np.float64)
    left, right = T(x), T((x - D0) / (1.0 + K))
    left = left + rng.normal(0.0, SIGMA, left.shape)
    right = right + rng.normal(0.0, SIGMA, right.shape)
    as_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return as_u8(left), as_u8(right)


def planes(left, right):
    """(winner-takes-all, SGM) disparity and cost planes, float32 [2, rows, cols] each"""
    wta = DR.planes(left, right, WIN, SEARCH_X, SEARCH_Y, STEP, DR.DISPARITY, True)
    sgm = SR.planes_fast(left, right, WIN, SEARCH_X, SEARCH_Y, STEP, *PENALTIES, True, SR.DISPARITY, True)
    return wta, sgm


def disparity_error(plane):
    """(mean |d - truth|, share of the points within 0.25 px) over the valid lattice points of the interior"""
    cols, rows, xs, ys = DR.lattice(W, H, STEP)
    x0, x1, y0, y1 = INTERIOR
    inside = ((ys > y0) & (ys < y1))[:, None] & ((xs > x0) & (xs < x1))[None, :] & (plane >= 0)
    err = np.abs(plane.astype(np.float64) - (D0 + K * xs.astype(np.float64))[None, :])[inside]
    return float(err.mean()), float((err <= 0.25).mean())


def fused_depth_error(records, voxel):
    """(RMS of z - truth, points judged) of the voxel points of a map of edge `voxel` that `records` were fused into
    once, where they project into the interior"""
    m = VR.Map(voxel, LOG2)
    assert m.admits(len(records))
    m.fuse(records, 1)
    p = m.extract()
    x, y, z = (p[k].astype(np.float64) for k in ("x", "y", "z"))
    px, py = RIG["fx"] * x / z + RIG["cx"], RIG["fy"] * y / z + RIG["cy"]
    x0, x1, y0, y1 = INTERIOR
    inside = (px > x0) & (px < x1) & (py > y0) & (py < y1)
    truth = RIG["baseline"] / (D0 + K * px[inside])
    return float(np.sqrt(np.mean((z[inside] - truth) ** 2))), int(inside.sum())


def clouds(left, wta, sgm):
    """the compact world-frame clouds of the two maps (the pose is zero)"""
    a = CR.cloud(left, wta, WIN, STEP, RIG, POSE, CR.WORLD, CR.COMPACT, MIN_DISPARITY)[0]
    b = SLR.cloud(left, sgm, STEP, RIG, POSE, CR.WORLD, CR.COMPACT, MIN_DISPARITY)[0]
    return a, b
