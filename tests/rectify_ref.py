"""numpy restatement of cv::remap(src, dst, map_x, map_y, INTER_LINEAR) with BORDER_CONSTANT 0 on 8-bit
images and CV_32FC1 maps, in OpenCV's fixed-point form (RemapInvoker + remapBilinear, INTER_BITS = 5,
INTER_REMAP_COEF_BITS = 15): the arithmetic contract of svo_remap_linear and of the tracker's
rectification (the reference's EurocInput::read, src/app/euroc_input.cpp:69-70).

Per output pixel, m = (map_x, map_y):
  * m non-finite, or |m * 32| >= 2^31: 0 (on x86 cvRound gives INT_MIN there, outside every image);
  * X = round_half_even(mx * 32), Y likewise (multiplying a float by 32 is exact);
    sx = X >> 5, sy = Y >> 5 (arithmetic shifts: floor), fx = X & 31, fy = Y & 31;
  * taps v00 = src[sy][sx], v01 = src[sy][sx+1], v10 = src[sy+1][sx], v11 = src[sy+1][sx+1], 0 outside the
    image, weights 32(32-fx)(32-fy), 32 fx(32-fy), 32(32-fx)fy, 32 fx fy (they sum to 2^15);
  * out = (sum w v + 16384) >> 15, which equals (sum' + 512) >> 10 over the products without the factor 32.

Integer positions: OpenCV's int16 weight table cannot hold 2^15; it stores 32767 and moves the remainder
(+1) to another tap of the same position. The sum then differs from 2^15 v00 by at most v00 - v_other,
|.| <= 255 < 2^14, and 2^15 v00 + 16384 + d stays in [2^15 v00, 2^15 (v00 + 1)): the result is exactly v00,
the value the formula above gives.

Colour: the reference remaps the BGR image and converts it to grey afterwards; for a grey image stored as
three equal channels cvtColor(BGR2GRAY) returns v again ((v * 16384 + 8192) >> 14 = v with the BT.601
weights summing to 16384), so remapping the 8-bit grey image is the reference's result.
"""
import numpy as np

INTER_BITS = 5
SCALE = 1 << INTER_BITS


def fixed_point(map_x, map_y):
    """(ok, sx, sy, fx, fy) of float32 maps: ok False where the entry gives 0."""
    mx = np.asarray(map_x, np.float32) * np.float32(SCALE)
    my = np.asarray(map_y, np.float32) * np.float32(SCALE)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) < np.float32(2.0 ** 31)) & (np.abs(my) < np.float32(2.0 ** 31))
    X = np.rint(np.where(ok, mx, 0)).astype(np.int64)          # numpy rounds half to even
    Y = np.rint(np.where(ok, my, 0)).astype(np.int64)
    return ok, X >> INTER_BITS, Y >> INTER_BITS, X & (SCALE - 1), Y & (SCALE - 1)


def _taps(src, sx, sy):
    h, w = src.shape
    src = np.asarray(src, np.int64)

    def at(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)

    return at(sy, sx), at(sy, sx + 1), at(sy + 1, sx), at(sy + 1, sx + 1)


def remap_linear(src, map_x, map_y):
    """uint8 [H, W] output of the map's size: (sum' + 512) >> 10."""
    ok, sx, sy, fx, fy = fixed_point(map_x, map_y)
    v00, v01, v10, v11 = _taps(src, sx, sy)
    s = (v00 * (SCALE - fx) * (SCALE - fy) + v01 * fx * (SCALE - fy) + v10 * (SCALE - fx) * fy + v11 * fx * fy)
    return np.where(ok, (s + 512) >> 10, 0).astype(np.uint8)


def remap_linear_coef15(src, map_x, map_y):
    """the same in OpenCV's 15-bit weight form: (sum w v + 16384) >> 15"""
    ok, sx, sy, fx, fy = fixed_point(map_x, map_y)
    v00, v01, v10, v11 = _taps(src, sx, sy)
    w00, w01 = 32 * (SCALE - fx) * (SCALE - fy), 32 * fx * (SCALE - fy)
    w10, w11 = 32 * (SCALE - fx) * fy, 32 * fx * fy
    s = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11
    return np.where(ok, (s + 16384) >> 15, 0).astype(np.uint8)


def euroc_like_maps(w, h, k1=-0.28, k2=0.07, angle=0.01, f_p=435.0, f_k=458.0, shift=(0.0, 0.0)):
    """cv::initUndistortRectifyMap-style maps of EuRoC's magnitude (radial k1, k2, a small rotation R, a P
    focal length of 435 against a K of 458): float32 (map_x, map_y) of w x h, computed in float64."""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    P = np.array([[f_p, 0, w / 2.0], [0, f_p, h / 2.0], [0, 0, 1]])
    K = np.array([[f_k, 0, w / 2.0 + 2.5 + shift[0]], [0, f_k * 0.997, h / 2.0 - 3.5 + shift[1]], [0, 0, 1]])
    iR = np.linalg.inv(P @ R)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    pts = np.stack([u, v, np.ones_like(u)], -1) @ iR.T
    x, y = pts[..., 0] / pts[..., 2], pts[..., 1] / pts[..., 2]
    r2 = x * x + y * y
    kr = 1 + (k2 * r2 + k1) * r2
    return ((K[0, 0] * x * kr + K[0, 2]).astype(np.float32), (K[1, 1] * y * kr + K[1, 2]).astype(np.float32))


def identity_maps(w, h):
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return u, v
