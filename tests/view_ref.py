"""Numpy statement of the views (include/svo_hip.h, "views"): the layout of a job's images and the rendering of one
image, gray expanded to RGB with one marker per keypoint. The rendering is the painter's loop of the reference app's
draw_frame: keypoints in ascending index, a later marker overwrites. Written from the header alone; the tests compare
the library with it byte for byte."""
import math

import numpy as np

PLANE_LEFT, PLANE_RIGHT = 0, 1
GRAY8, RGB8, RGBA8 = 0, 1, 2
BYTES = {GRAY8: 1, RGB8: 3, RGBA8: 4}
KP_FAST = 0
IGNORE_TEMPORARY = 4


def size(width, height, plane, level, pixel):
    """(cols, rows, pitch, image_bytes)"""
    l = level if plane == PLANE_LEFT else 0
    cols, rows = width >> l, height >> l
    pitch = cols * BYTES[pixel]
    return cols, rows, pitch, (rows * pitch + 255) // 256 * 256


def centre(x, y, level):
    """the marker's centre at `level`, or None for a keypoint that draws nothing"""
    s = np.float32(2.0) ** np.float32(-level)
    fx, fy = np.float32(x) * s, np.float32(y) * s
    if not (math.isfinite(fx) and math.isfinite(fy)) or abs(fx) >= 32768 or abs(fy) >= 32768:
        return None
    return math.trunc(float(fx)), math.trunc(float(fy))


def marker_pixels(cx, cy, kp_type, s):
    """the pixels of one marker, unclipped: [(x, y)]"""
    if kp_type == KP_FAST:
        h = s // 2
        return [(x, cy) for x in range(cx - h, cx + h + 1)] + [(cx, y) for y in range(cy - h, cy + h + 1)]
    h = int(s * 0.8) // 2
    out = []
    for x in range(cx - h, cx + h + 1):
        out += [(x, cy - h), (x, cy + h)]
    for y in range(cy - h, cy + h + 1):
        out += [(cx - h, y), (cx + h, y)]
    return out


def drawn(kps2d, flags, types, level, drop_flags, size_plain, size_temporary):
    """per keypoint its marker's unclipped pixels, or None for one that draws nothing (dropped, or no centre)"""
    out = []
    for i in range(len(kps2d)):
        f = int(flags[i])
        c = None if f & drop_flags else centre(kps2d[i][0], kps2d[i][1], level)
        if c is None:
            out.append(None)
            continue
        s = size_temporary if f & IGNORE_TEMPORARY else size_plain
        out.append(marker_pixels(c[0], c[1], int(types[i]), s))
    return out


def expand(gray, pixel):
    """the plane in the pixel format: [rows, cols] or [rows, cols, 3 | 4]"""
    gray = np.asarray(gray, np.uint8)
    if pixel == GRAY8:
        return gray.copy()
    img = np.repeat(gray[:, :, None], BYTES[pixel], axis=2)
    if pixel == RGBA8:
        img[:, :, 3] = 255
    return img


def render(gray, pixel, kps2d=None, flags=None, types=None, colors=None, level=0, drop_flags=0, size_plain=10,
           size_temporary=10):
    """the image: the painter's loop. types: SVO_KP_* per keypoint; colors: [n, 3] bytes r, g, b. kps2d None: the
    plane only."""
    img = expand(gray, pixel)
    if kps2d is None or pixel == GRAY8:
        return img
    rows, cols = img.shape[:2]
    for i, pix in enumerate(drawn(kps2d, flags, types, level, drop_flags, size_plain, size_temporary)):
        for x, y in pix or ():
            if 0 <= x < cols and 0 <= y < rows:
                img[y, x, :3] = colors[i]
    return img


def render_highest_index(gray, pixel, kps2d, flags, types, colors, level=0, drop_flags=0, size_plain=10,
                         size_temporary=10):
    """the same image stated the way the kernel computes it: per pixel the highest index of a keypoint whose marker
    covers it, in whatever order the keypoints are visited (here: descending)"""
    img = expand(gray, pixel)
    rows, cols = img.shape[:2]
    owner = np.zeros((rows, cols), np.int64)
    pix = drawn(kps2d, flags, types, level, drop_flags, size_plain, size_temporary)
    for i in reversed(range(len(pix))):
        for x, y in pix[i] or ():
            if 0 <= x < cols and 0 <= y < rows:
                owner[y, x] = max(owner[y, x], i + 1)
    covered = owner > 0
    img[covered, :3] = np.asarray(colors, np.uint8).reshape(-1, 3)[owner[covered] - 1]
    return img


def place(images, offsets, total, fill=0xA5):
    """the bytes of a destination of `total` bytes pre-filled with `fill` after the images were written at offsets"""
    out = np.full(total, fill, np.uint8)
    for img, off in zip(images, offsets):
        b = np.ascontiguousarray(img).reshape(-1)
        out[off:off + b.size] = b
    return out


def info_arrays(info):
    """(flags word, types, colors) of the getters' svo_kp_info records (KP_INFO_DTYPE)"""
    flags = (info["ignore_during_refinement"].astype(np.uint32) * 1 + info["ignore_completely"].astype(np.uint32) * 2 +
             info["ignore_temporary"].astype(np.uint32) * 4)
    return flags, info["type"].astype(np.int64), info["color"].copy()
