"""Numpy statement of the input formats (include/svo_hip.h, SVO_INPUT_*): the three operations the reference's
ImageInput classes do before StereoSlam::new_image. It shares no code with the product.

 * gray from colour (src/app/video_input.cpp:29-31, cvtColor BGR2GRAY of OpenCV 4.x, RGB2Gray<uchar>):
   Y = (3735 B + 19235 G + 9798 R + 2^14) >> 15;
 * channel extract (src/app/econ_input.cpp:102-103): byte k of an interleaved 3-channel pixel;
 * side by side (src/app/video_input.cpp:33-36): right = columns 0 .. W-1, left = columns W .. 2W-1.
"""
import numpy as np

B15, G15, R15 = 3735, 19235, 9798          # 15-bit table
B14, G14, R14 = 1868, 9617, 4899           # the older 14-bit table (not implemented by the library)

FORMATS = ("gray_pair", "bgr_pair", "rgb_pair", "sbs_gray", "sbs_bgr", "sbs_rgb", "ch3_econ")
ONE_BUFFER = ("sbs_gray", "sbs_bgr", "sbs_rgb", "ch3_econ")


def gray15(b, g, r):
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return ((B15 * b + G15 * g + R15 * r + (1 << 14)) >> 15).astype(np.uint8)


def gray14(b, g, r):
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return ((B14 * b + G14 * g + R14 * r + (1 << 13)) >> 14).astype(np.uint8)


def gray_pil(b, g, r):
    """PIL's convert("L"): ITU-R 601-2 in 16-bit fixed point"""
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return ((19595 * r + 38470 * g + 7471 * b + (1 << 15)) >> 16).astype(np.uint8)


def gray_of(img, order):
    """[H, W, 3] in `order` ('bgr' | 'rgb') -> [H, W]"""
    if order == "bgr":
        return gray15(img[..., 0], img[..., 1], img[..., 2])
    return gray15(img[..., 2], img[..., 1], img[..., 0])


def convert(fmt, a, b=None, width=None):
    """the (left, right) gray images of one sequence's buffers in format `fmt` (a name of FORMATS). a, b: uint8
    arrays; width: of the images (side by side: default half the buffer's columns)."""
    if fmt == "gray_pair":
        return a[:, :width or a.shape[1]].copy(), b[:, :width or b.shape[1]].copy()
    if fmt in ("bgr_pair", "rgb_pair"):
        w = width or a.shape[1]
        return gray_of(a[:, :w], fmt[:3]), gray_of(b[:, :w], fmt[:3])
    if fmt == "sbs_gray":
        w = width or a.shape[1] // 2
        return a[:, w:2 * w].copy(), a[:, :w].copy()
    if fmt in ("sbs_bgr", "sbs_rgb"):
        w = width or a.shape[1] // 2
        return gray_of(a[:, w:2 * w], fmt[4:]), gray_of(a[:, :w], fmt[4:])
    if fmt == "ch3_econ":
        w = width or a.shape[1]
        return a[:, :w, 2].copy(), a[:, :w, 1].copy()
    raise ValueError(fmt)


def colourize(gray, seed):
    """a genuinely coloured [H, W, 3] B, G, R image from a gray one: per-channel gains and offsets, clipped"""
    rng = np.random.default_rng(seed)
    gain = rng.uniform(0.6, 1.4, 3)
    off = rng.uniform(-30, 30, 3)
    out = np.clip(np.rint(gray[..., None].astype(np.float64) * gain + off), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out)


def pack(fmt, left_bgr, right_bgr):
    """the buffers (a, b) of one sequence in format `fmt` whose images are the coloured left_bgr / right_bgr
    ([H, W, 3] B, G, R). The gray formats carry gray15 of them; ch3_econ carries left in channel 2 and right in
    channel 1 (gray15 of each) and noise in channel 0. b is None for the one-buffer formats."""
    gl, gr = gray_of(left_bgr, "bgr"), gray_of(right_bgr, "bgr")
    if fmt == "gray_pair":
        return gl, gr
    if fmt == "bgr_pair":
        return left_bgr.copy(), right_bgr.copy()
    if fmt == "rgb_pair":
        return np.ascontiguousarray(left_bgr[..., ::-1]), np.ascontiguousarray(right_bgr[..., ::-1])
    if fmt == "sbs_gray":
        return np.ascontiguousarray(np.concatenate([gr, gl], 1)), None
    if fmt == "sbs_bgr":
        return np.ascontiguousarray(np.concatenate([right_bgr, left_bgr], 1)), None
    if fmt == "sbs_rgb":
        return np.ascontiguousarray(np.concatenate([right_bgr, left_bgr], 1)[..., ::-1]), None
    if fmt == "ch3_econ":
        noise = np.random.default_rng(gl.size).integers(0, 256, gl.shape, dtype=np.uint8)
        return np.ascontiguousarray(np.stack([noise, gr, gl], -1)), None
    raise ValueError(fmt)
