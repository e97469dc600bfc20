"""Rectification maps from calibrations (cv::initUndistortRectifyMap, src/app/euroc_input.cpp:24-49): the f64
statement of include/svo_hip.h in explicit numpy element operations (every product and sum a separate rounded
operation, in the statement's association; no matmul, no linalg), an independent twin built on np.linalg.inv and @,
and the calibrations the tests use. A calibration here is (K 3x3, D[8] = k1 k2 p1 p2 k3 k4 k5 k6, R 3x3, P 3x3),
float64."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "euroc_calibration.json")


def inverse(cal):
    """ir[9] of the statement"""
    K, D, R, P = (np.asarray(m, np.float64) for m in cal)
    M = [[(P[r][0] * R[0][c] + P[r][1] * R[1][c]) + P[r][2] * R[2][c] for c in range(3)] for r in range(3)]
    (a, b, c), (d, e, f), (g, h, i) = M
    c00 = e * i - f * h
    c01 = f * g - d * i
    c02 = d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    with np.errstate(all="ignore"):
        t = np.float64(1.0) / det
    return np.array([c00 * t, (c * h - b * i) * t, (b * f - c * e) * t,
                     c01 * t, (a * i - c * g) * t, (c * d - a * f) * t,
                     c02 * t, (b * g - a * h) * t, (a * e - b * d) * t], np.float64)


def maps(cal, w, h):
    """(map_x, map_y) float32 [h, w] of the statement"""
    K, D, R, P = (np.asarray(m, np.float64) for m in cal)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in D)
    ir = inverse(cal)
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        X = j * ir[0] + (i * ir[1] + ir[2])
        Y = j * ir[3] + (i * ir[4] + ir[5])
        W = j * ir[6] + (i * ir[7] + ir[8])
        iw = one / W
        x = X * iw
        y = Y * iw
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = (two * x) * y
        kr = (one + ((k3 * r2 + k2) * r2 + k1) * r2) / (one + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * _2xy) + p2 * (r2 + two * x2)
        yd = (y * kr + p1 * (r2 + two * y2)) + p2 * _2xy
        return (K[0][0] * xd + K[0][2]).astype(np.float32), (K[1][1] * yd + K[1][2]).astype(np.float32)


def twin_maps(cal, w, h):
    """the same maps by another route: np.linalg.inv, a matrix product per pixel, the distortion polynomial in
    another association. Not bit-exact to anything: within rounding of the statement."""
    K, D, R, P = (np.asarray(m, np.float64) for m in cal)
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    iR = np.linalg.inv(P @ R)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        pts = np.stack([u, v, np.ones_like(u)], -1) @ iR.T
        x, y = pts[..., 0] / pts[..., 2], pts[..., 1] / pts[..., 2]
        r2 = x * x + y * y
        kr = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return (K[0, 0] * xd + K[0, 2]).astype(np.float32), (K[1, 1] * yd + K[1, 2]).astype(np.float32)


def rotation(a, b, c):
    """the rotation of the quaternion (1, a, b, c) / |.|: + * / only, so the same bits everywhere"""
    n = 1.0 + a * a + b * b + c * c
    w, x, y, z = 1.0, a, b, c
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], np.float64) / n


def _k(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def _d(*v):
    return np.array(list(v) + [0.0] * (8 - len(v)), np.float64)


@functools.lru_cache(maxsize=1)
def euroc():
    """{"LEFT": calibration, "RIGHT": calibration}, (width, height) of the reference's EuRoC.yaml"""
    raw = json.load(open(GOLDEN))
    mat = lambda k: np.array(raw[k]["data"], np.float64).reshape(raw[k]["rows"], raw[k]["cols"])
    out = {side: (mat(f"{side}.K"), _d(*mat(f"{side}.D").ravel()), mat(f"{side}.R"), mat(f"{side}.P")[:, :3])
           for side in ("LEFT", "RIGHT")}
    return out, (raw["width"], raw["height"])


# the horizon case: a camera turned by exactly 90 degrees about y in front of P = [[64, 0, 2], [0, 64, 1.5], [0, 0, 1]].
# Every entry of P R and of its inverse is exact, W = +-(j - 2) / 64: exactly 0 in column 2 (1 / 0, then inf * 0: not
# finite), of one sign left of it and of the other right of it. Column 2 is 1 / width of the image.
HORIZON_COLUMN = 2


@functools.lru_cache(maxsize=1)
def cases():
    """name -> calibration. `identity`, the two EuRoC cameras, `tangential` (p1, p2 only), `rational` (k4..k6 and a
    strong k1), `horizon` (W crosses zero inside the image) and `outside` (P's principal point outside the image)."""
    e = euroc()[0]
    # (identity: powers of two and dyadic centres, so both routes are exact and pixel (0, 0) maps to exactly (0, 0):
    # a map value next to zero by cancellation has no meaningful distance in float32 steps)
    k = _k(256.0, 128.0, 66.25, 31.5)
    return {
        "identity": (k, _d(), np.eye(3), k.copy()),
        "euroc_left": e["LEFT"],
        "euroc_right": e["RIGHT"],
        "tangential": (_k(123.0, 124.5, 64.0, 33.0), _d(0.0, 0.0, 1.5e-3, -2.25e-3),
                       rotation(0.004, -0.003, 0.002), _k(118.0, 118.0, 65.5, 32.25)),
        "rational": (_k(96.0, 95.0, 63.5, 30.75), _d(-0.61, 0.24, 3.0e-4, -2.0e-4, -0.031, 0.18, 0.05, 0.003),
                     rotation(-0.003, 0.005, -0.001), _k(80.0, 80.0, 66.0, 33.0)),
        "horizon": (_k(200.0, 200.0, 160.0, 120.0), _d(-0.05, 0.01),
                    np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), _k(64.0, 64.0, float(HORIZON_COLUMN), 1.5)),
        "outside": (_k(150.0, 150.0, 70.0, 35.0), _d(-0.2, 0.05, 0.0, 0.0, 0.01),
                    rotation(0.002, 0.001, -0.004), _k(140.0, 141.0, -50.0, 500.0)),
    }


def same_bits(a, b):
    """float32 arrays equal as bit patterns, NaN positions comparing as NaN = NaN (any payload)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
