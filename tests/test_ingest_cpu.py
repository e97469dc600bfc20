"""The input formats without a GPU: the arithmetic statement (tests/ingest_ref.py) pinned on known answers, the
replay harness's host conversion and inputs against it, and svo_input_format_info."""
import numpy as np
import pytest

import ingest_ref as IR
from stereo_svo_slam_amd import hip_lib, replay


def test_gray_of_equal_channels_is_the_value():
    v = np.arange(256)
    assert np.array_equal(IR.gray15(v, v, v), v)
    assert IR.B15 + IR.G15 + IR.R15 == 1 << 15


def test_the_accumulator_fits_24_bits():
    assert 255 * (IR.B15 + IR.G15 + IR.R15) + (1 << 14) == 8372224 < 1 << 24
    assert max(IR.B15, IR.G15, IR.R15) < 1 << 24


def test_corner_colours():
    """the eight corners of the colour cube, (B, G, R) -> Y by hand: (sum of the weights of the channels at 255) * 255
    + 2^14, >> 15"""
    exp = {(0, 0, 0): 0, (255, 0, 0): 29, (0, 255, 0): 150, (0, 0, 255): 76, (255, 255, 0): 179,
           (255, 0, 255): 105, (0, 255, 255): 226, (255, 255, 255): 255}
    for (b, g, r), y in exp.items():
        assert int(IR.gray15(b, g, r)) == y, (b, g, r)
        assert y == (3735 * b + 19235 * g + 9798 * r + 16384) // 32768


def _all_colours_sample():
    rng = np.random.default_rng(11)
    c = rng.integers(0, 256, (2_000_000, 3), dtype=np.uint8)
    return c[:, 0], c[:, 1], c[:, 2]


def test_the_three_tables_disagree_somewhere():
    """colours at which the 15-bit form differs from the 14-bit form and from PIL's "L": found by search, they
    exist, by one level, in about the shares the design notes state; known answers at the first of each"""
    b, g, r = _all_colours_sample()
    y15, y14, yp = IR.gray15(b, g, r), IR.gray14(b, g, r), IR.gray_pil(b, g, r)
    d14 = np.flatnonzero(y15 != y14)
    dp = np.flatnonzero(y15 != yp)
    assert len(d14) > 0 and len(dp) > 0
    assert np.abs(y15.astype(int) - y14)[d14].max() == 1 and np.abs(y15.astype(int) - yp)[dp].max() == 1
    assert 0.001 < len(d14) / len(b) < 0.006 and 0.0004 < len(dp) / len(b) < 0.004
    for i in (d14[0], dp[0]):
        bb, gg, rr = int(b[i]), int(g[i]), int(r[i])
        assert int(y15[i]) == (3735 * bb + 19235 * gg + 9798 * rr + 16384) >> 15
    i = d14[0]
    assert int(IR.gray14(b[i], g[i], r[i])) == (1868 * int(b[i]) + 9617 * int(g[i]) + 4899 * int(r[i]) + 8192) >> 14


def test_replay_bgr2gray_is_the_statement():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (61, 83, 3), dtype=np.uint8)
    assert np.array_equal(replay.bgr2gray(img), IR.gray_of(img, "bgr"))
    assert np.array_equal(replay.bgr2gray(img, "rgb"), IR.gray_of(img, "rgb"))
    assert replay.bgr2gray(img).dtype == np.uint8
    # the statement is not PIL's "L"
    from PIL import Image
    pil = np.array(Image.fromarray(np.ascontiguousarray(img[..., ::-1])).convert("L"))
    big = rng.integers(0, 256, (400, 500, 3), dtype=np.uint8)
    pil_big = np.array(Image.fromarray(np.ascontiguousarray(big[..., ::-1])).convert("L"))
    assert np.array_equal(pil, IR.gray_pil(img[..., 0], img[..., 1], img[..., 2]))
    assert not np.array_equal(pil_big, replay.bgr2gray(big))


def test_split_then_convert_equals_convert_then_split():
    rng = np.random.default_rng(6)
    frame = rng.integers(0, 256, (9, 34, 3), dtype=np.uint8)
    left, right = IR.convert("sbs_bgr", frame)
    whole = IR.gray_of(frame, "bgr")
    assert np.array_equal(left, whole[:, 17:]) and np.array_equal(right, whole[:, :17])


def test_pack_and_convert_are_inverse():
    rng = np.random.default_rng(7)
    g = rng.integers(0, 256, (2, 12, 20), dtype=np.uint8)
    lc, rc = IR.colourize(g[0], 1), IR.colourize(g[1], 2)
    assert (lc[..., 0] != lc[..., 1]).any() and (lc[..., 1] != lc[..., 2]).any(), "genuinely coloured"
    want = IR.gray_of(lc, "bgr"), IR.gray_of(rc, "bgr")
    for fmt in IR.FORMATS:
        a, b = IR.pack(fmt, lc, rc)
        assert (b is None) == (fmt in IR.ONE_BUFFER)
        got = IR.convert(fmt, a, b)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), fmt


def test_input_format_info_for_every_format():
    """svo_input_format_info (no GPU): buffers, channels, minimum row, and each side's start column and operation"""
    W = 752
    bgr, rgb = [IR.B15, IR.G15, IR.R15], [IR.R15, IR.G15, IR.B15]
    COPY, GRAY = hip_lib.INGEST_COPY, hip_lib.INGEST_GRAY
    # name: (buffers, channels, min row, left (buffer, start, op, channel / weights), right)
    exp = {
        "gray_pair": (2, 1, W, (0, 0, COPY, 0), (1, 0, COPY, 0)),
        "bgr_pair": (2, 3, W, (0, 0, GRAY, bgr), (1, 0, GRAY, bgr)),
        "rgb_pair": (2, 3, W, (0, 0, GRAY, rgb), (1, 0, GRAY, rgb)),
        "sbs_gray": (1, 1, 2 * W, (0, W, COPY, 0), (0, 0, COPY, 0)),
        "sbs_bgr": (1, 3, 2 * W, (0, W, GRAY, bgr), (0, 0, GRAY, bgr)),
        "sbs_rgb": (1, 3, 2 * W, (0, W, GRAY, rgb), (0, 0, GRAY, rgb)),
        "ch3_econ": (1, 3, W, (0, 0, COPY, 2), (0, 0, COPY, 1)),
    }
    assert hip_lib.INPUT_FORMATS == IR.FORMATS
    assert (hip_lib.INPUT_GRAY_PAIR, hip_lib.INPUT_SBS_GRAY, hip_lib.INPUT_CH3_ECON) == (0, 3, 6)
    for fmt, name in enumerate(hip_lib.INPUT_FORMATS):
        info = hip_lib.input_format_info(fmt, W)
        buffers, channels, row, left, right = exp[name]
        assert (info.buffers, info.channels, info.min_row_pixels) == (buffers, channels, row), name
        for side, e in ((info.left, left), (info.right, right)):
            assert (side.buffer, side.start_column, side.op) == e[:3], name
            if e[2] == COPY:
                assert side.channel == e[3], name
            else:
                assert list(side.weight) == e[3] and sum(side.weight) == 1 << 15, name
    import ctypes as C
    out = hip_lib.InputLayout()
    f = hip_lib.lib().svo_input_format_info
    assert f(7, W, C.byref(out)) == -1 and f(-1, W, C.byref(out)) == -1
    assert f(0, 0, C.byref(out)) == -1 and f(0, W, None) == -1
    with pytest.raises(hip_lib.SvoError):
        hip_lib.input_format_info(99, W)


def _write_pngs(tmp_path, frames):
    from PIL import Image
    for k, f in enumerate(frames):
        im = Image.fromarray(f if f.ndim == 2 else np.ascontiguousarray(f[..., ::-1]))     # (files hold R, G, B)
        im.save(str(tmp_path / f"{k:06d}.png"))
    return str(tmp_path / "%06d.png")


def test_side_by_side_input_colour_and_raw(tmp_path):
    rng = np.random.default_rng(8)
    colour = [rng.integers(0, 256, (10, 24, 3), dtype=np.uint8) for _ in range(2)]
    pattern = _write_pngs(tmp_path, colour)
    split = replay.SideBySideInput(pattern, 2, fps=30.0)
    raw = replay.SideBySideInput(pattern, 2, fps=30.0, raw=True)
    assert raw.input_format() == "sbs_bgr"
    for k in range(2):
        left, right, t = split.read(k)
        frame, none, t_raw = raw.read(k)
        assert none is None and t == t_raw == pytest.approx((k + 1) / 30.0)
        assert np.array_equal(frame, colour[k]), "the raw frame is the decoded B, G, R frame"
        el, er = IR.convert("sbs_bgr", frame)
        assert np.array_equal(left, el) and np.array_equal(right, er)
        assert left.flags["C_CONTIGUOUS"] and left.dtype == np.uint8
    # gray files: unchanged, and raw hands out the gray frame
    (tmp_path / "g").mkdir()
    gray = [rng.integers(0, 256, (10, 24), dtype=np.uint8)]
    gp = _write_pngs(tmp_path / "g", gray)
    left, right, _ = replay.SideBySideInput(gp, 1).read(0)
    assert np.array_equal(left, gray[0][:, 12:]) and np.array_equal(right, gray[0][:, :12])
    rawg = replay.SideBySideInput(gp, 1, raw=True)
    assert rawg.input_format() == "sbs_gray" and np.array_equal(rawg.read(0)[0], gray[0])


def test_interleaved_input(tmp_path):
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (7, 13, 3), dtype=np.uint8) for _ in range(3)]
    pattern = _write_pngs(tmp_path, frames)
    split = replay.InterleavedInput(pattern, 3, fps=20.0)
    raw = replay.InterleavedInput(pattern, 3, fps=20.0, raw=True)
    assert len(split) == 3 and raw.input_format() == "ch3_econ"
    for k in range(3):
        left, right, t = split.read(k)
        frame, none, t_raw = raw.read(k)
        assert none is None and t == t_raw == pytest.approx((k + 1) / 20.0)
        el, er = IR.convert("ch3_econ", frame)
        assert np.array_equal(left, el) and np.array_equal(right, er)
        assert np.array_equal(left, frames[k][..., 2]) and np.array_equal(right, frames[k][..., 1])
