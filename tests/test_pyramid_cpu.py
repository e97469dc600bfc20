"""The oracle's two pyramids against plain int64 numpy statements (tests/pyramid_cases.py) on every crafted image
and shape of tests/test_pyramid_gpu.py, and proof that those images reach the edges of the arithmetic that they are
there for. The statements share no code with the oracle: halfSample is (a + b + c + d) // 4, pyrDown the full 5 x 5
outer product of [1 4 6 4 1] over an np.pad(mode="reflect") image."""
import numpy as np
import pytest

import oracle_py as O
import pyramid_cases as P
import snapshot_ref as SR

SHAPES = sorted({(c.h, c.w, c.n_levels) for c in P.CASES})
assert len({(h, w) for h, w, _ in SHAPES}) == len(SHAPES), "one level count per shape"


def _id(s):
    return f"{s[0]}x{s[1]}-{s[2]}"


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_oracle_equals_the_numpy_statements(shape):
    h, w, n_levels = shape
    win = P.lk_window(h, w)
    assert SR.lk_levels(dict(width=w, height=h, window_size_opt_flow=win)) == P.lk_level_count(h, w, win) == 3
    bad = []
    for name, img in P.images(h, w).items():
        hs, _ = P.half_sample_chain(img, n_levels)
        got = O.build_pyramid(img, n_levels)
        bad += [(name, "halfSample", l) for l in range(n_levels)
                if got[l].shape != (h >> l, w >> l) or not np.array_equal(got[l], hs[l])]
        pd, _ = P.pyr_down_chain(img, win)
        got = O.build_lk_pyramid(img, win)
        if len(got) != len(pd):
            bad.append((name, "LK level count", len(got)))
        bad += [(name, "pyrDown", l) for l in range(min(len(pd), len(got))) if not np.array_equal(got[l], pd[l])]
    assert not bad, bad


def test_lk_level_rule():
    """the stop rule of cv::buildOpticalFlowPyramid as the oracle applies it, around the window sizes"""
    for h, w in ((16, 16), (34, 456), (65, 129), (17, 19)):
        img = P.FAMILIES["noise"](h, w)
        for win in (3, 4, 5, 8, 9, 16, 17, 33):
            assert len(O.build_lk_pyramid(img, win)) == P.lk_level_count(h, w, win), (h, w, win)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_constant_255_reaches_the_16_bit_ceiling(shape):
    """256 * 255 + 128 = 65408 before the shift, 128 below what a packed 16-bit lane holds, at both levels"""
    h, w, _ = shape
    levels, sums = P.pyr_down_chain(P.images(h, w)["const255"], P.lk_window(h, w))
    assert len(levels) == 3
    for l in (1, 2):
        assert sums[l].min() == sums[l].max() == 65280 and int(sums[l].max()) + 128 == 65408
        assert np.all(levels[l] == 255)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_rounding_images_reach_every_residue(shape):
    """over the shape's rounding images: pre-shift pyrDown sums with v & 255 == 127 and == 128 at both levels (the
    two sides of (v + 128) >> 8), and halfSample sums of every residue modulo 4 at every level (the truncating / 4)"""
    h, w, n_levels = shape
    imgs = P.images(h, w)
    have = set()
    for seed in P.ROUNDING_SEEDS[(h, w)]:
        img = imgs[f"rounding{seed}"]
        assert set(np.unique(img)) <= set(P.ROUNDING_VALUES.tolist())
        have |= P.rounding_coverage(img, n_levels, P.lk_window(h, w))
    goal = P.rounding_goal(n_levels)
    assert len(goal) == 4 * (n_levels - 1) + 4
    assert goal <= have, sorted(goal - have)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_impulse_shows_on_every_level_it_can_reach(shape):
    """A level that an impulse can reach: pyrDown levels 1 and 2 always (every tap weight is at least 1 of 256 and
    the smallest value left on level 1 is 16); halfSample level l if the pixel's 2^l block lies inside the floor-
    halved image, and for a 255 on black while 255 >> 2l is not 0 (l <= 3); a 0 on white stays visible for ever
    (255 -> 191 -> 239 -> 251 -> 254 -> 254)."""
    h, w, n_levels = shape
    win = P.lk_window(h, w)
    imgs = P.images(h, w)
    base = {white: (P.half_sample_chain(imgs[name], n_levels)[0], P.pyr_down_chain(imgs[name], win)[0])
            for white, name in ((False, "const0"), (True, "const255"))}
    positions = P.impulse_positions(h, w)
    assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h - 2, w // 2), (h // 2, w - 2)} <= set(positions)
    for x in (7, 8, 63, 64, 447, 448):
        assert (x < w) == ((h // 2, x) in positions)
    for y in (31, 32, 63, 64):
        assert (y < h) == ((y, w // 2) in positions)
    unseen = []
    for y, x in positions:
        for white in (False, True):
            name = f"{'white' if white else 'black'}_y{y}x{x}"
            img = imgs[name]
            assert (img != (255 if white else 0)).sum() == 1 and img[y, x] == (0 if white else 255)
            hs, pd = P.half_sample_chain(img, n_levels)[0], P.pyr_down_chain(img, win)[0]
            for l in range(1, n_levels):
                inside = (y >> l) < (h >> l) and (x >> l) < (w >> l)
                if inside and (white or l <= 3) and np.array_equal(hs[l], base[white][0][l]):
                    unseen.append((name, "halfSample", l))
            for l in (1, 2):
                if np.array_equal(pd[l], base[white][1][l]):
                    unseen.append((name, "pyrDown", l))
    assert not unseen, unseen


def test_case_table_reaches_every_kernel_and_path():
    """what the GPU file relies on, from the selection rule as pyramid.hip states it (pyr_stream_rows): the shapes
    take the kernels they are listed for, unaligned views always take the tile kernel, and the table holds second
    column blocks, partial row blocks, odd h1 and odd unit counts at level 4"""
    for c in P.CASES:
        assert P.expected_kernel(c.h, c.w, c.n_levels, c.kernel) == c.runs, c
        for layout in ("off3", "oddstride"):
            off, stride = P.layout_of(layout, c.w)
            assert P.expected_kernel(c.h, c.w, c.n_levels, c.kernel, off, stride) == "tile"
        off, stride = P.layout_of("strided", c.w)
        assert stride > c.w and P.expected_kernel(c.h, c.w, c.n_levels, c.kernel, off, stride) == c.runs
    stream = [c for c in P.CASES if c.runs != "tile"]
    assert {c.runs for c in P.CASES} == {"stream32", "stream64", "tile"}
    assert any(c.w // 8 == 57 for c in stream) and any(c.w // 8 == 56 for c in stream)       # 56 units + 1, exactly 56
    assert any(c.w // 8 > 112 for c in stream)                                                 # a third column block
    assert any(((c.h + 1) // 2) % 2 == 1 for c in stream)                                      # odd h1
    assert any(c.runs == "stream32" and c.h % 32 == 2 for c in stream)                         # a block of two rows
    assert any(c.runs == "stream64" and c.h > 64 and c.h % 64 for c in stream)                 # a partial 64-row block
    assert any(c.runs == "stream64" and c.h < 32 for c in stream)
    tile = [c for c in P.CASES if c.runs == "tile"]
    assert any(c.w % 64 == 1 and c.h % 64 == 1 for c in tile) and any(c.w % 64 == 63 and c.h % 64 == 63 for c in tile)
    assert any(c.w % 8 == 0 and c.h % 2 == 0 for c in tile)                                    # forced, not chosen
