"""The fixed-point cv::remap restatement (tests/rectify_ref.py) pinned on known answers."""
import numpy as np

import rectify_ref as RR


def _img(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def test_identity_maps_return_the_image():
    img = _img(37, 53)
    mx, my = RR.identity_maps(53, 37)
    assert np.array_equal(RR.remap_linear(img, mx, my), img)


def test_half_pixel_shift_is_the_rounded_mean():
    img = _img(20, 30, 1)
    mx, my = RR.identity_maps(29, 20)
    out = RR.remap_linear(img, mx + np.float32(0.5), my)
    a, b = img[:, :29].astype(int), img[:, 1:30].astype(int)
    assert np.array_equal(out, ((a + b + 1) >> 1).astype(np.uint8))


def test_ties_round_to_even():
    """m * 32 = k + 0.5 goes to the even neighbour: 0.5/32 -> X = 0, 1.5/32 -> X = 2, 2.5/32 -> X = 2"""
    img = np.zeros((2, 4), np.uint8)
    img[0, 1] = 255
    for m, X in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2)):
        ok, sx, sy, fx, fy = RR.fixed_point(np.float32([[m / 32]]), np.float32([[0]]))
        assert ok[0, 0] and sx[0, 0] * 32 + fx[0, 0] == X, (m, sx, fx)
    # X = 2 -> fx = 2: (255 * 2 * 32 + 512) >> 10 = 16
    out = RR.remap_linear(img, np.float32([[1.5 / 32 + 0.0]]), np.float32([[0.0]]))
    assert out[0, 0] == (255 * 2 * 32 + 512) >> 10


def test_border_taps_count_as_zero():
    img = np.full((4, 4), 200, np.uint8)
    # one tap outside (x = 3.5: v01 outside), two (corner row), three (corner), four (far outside)
    cases = {(3.5, 1.0): (200 * 16 * 32 + 512) >> 10,
             (3.5, 3.0): (200 * 16 * 32 + 512) >> 10,
             (3.5, 3.5): (200 * 16 * 16 + 512) >> 10,
             (-0.5, -0.5): (200 * 16 * 16 + 512) >> 10,
             (-0.5, 1.0): (200 * 16 * 32 + 512) >> 10,
             (4.0, 1.0): 0, (-1.0, 1.0): 0, (10.0, 10.0): 0, (-1.5, -1.5): 0}
    for (x, y), exp in cases.items():
        out = RR.remap_linear(img, np.float32([[x]]), np.float32([[y]]))
        assert out[0, 0] == exp, ((x, y), out[0, 0], exp)


def test_non_finite_and_huge_entries_give_zero():
    img = np.full((8, 8), 77, np.uint8)
    bad = [np.nan, np.inf, -np.inf, 1e10, -1e10, 2.0 ** 31 / 32, -(2.0 ** 31) / 32]
    for v in bad:
        for mx, my in ((v, 1.0), (1.0, v)):
            out = RR.remap_linear(img, np.float32([[mx]]), np.float32([[my]]))
            assert out[0, 0] == 0, (mx, my)
    # just below the range limit: a valid entry far outside the image, also 0; inside: the pixel
    assert RR.fixed_point(np.float32([[(2.0 ** 31 - 128) / 32]]), np.float32([[0]]))[0][0, 0]
    assert RR.remap_linear(img, np.float32([[2.0]]), np.float32([[3.0]]))[0, 0] == 77


def test_coefficient_forms_agree_on_random_inputs():
    rng = np.random.default_rng(5)
    img = _img(41, 67, 2)
    mx = rng.uniform(-3, 70, (50, 60)).astype(np.float32)
    my = rng.uniform(-3, 44, (50, 60)).astype(np.float32)
    a = RR.remap_linear(img, mx, my)
    b = RR.remap_linear_coef15(img, mx, my)
    assert np.array_equal(a, b)
    assert a.std() > 10


def test_euroc_like_maps_keep_taps_near_the_pixel():
    """the calibration the GPU tests use: a 64 x 64 output tile reads a source box of at most ~68 x 68"""
    w, h = 752, 480
    mx, my = RR.euroc_like_maps(w, h)
    ok, sx, sy, _, _ = RR.fixed_point(mx, my)
    assert ok.all()
    boxes = []
    for ty in range(0, h, 64):
        for tx in range(0, w, 64):
            bx, by = sx[ty:ty + 64, tx:tx + 64], sy[ty:ty + 64, tx:tx + 64]
            boxes.append((bx.max() - bx.min() + 2, by.max() - by.min() + 2))
    assert max(b[0] for b in boxes) <= 80 and max(b[1] for b in boxes) <= 80, max(boxes)
