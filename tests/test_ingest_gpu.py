"""The input formats on the GPU (svo_convert_frames, svo_ctx_set_input_format) against the numpy statement
(tests/ingest_ref.py) bit for bit: the stage entry on crafted buffers, and the tracker fed colour / packed frames
against a tracker with the default format fed the statement's gray images, and against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ingest_ref as IR
import rectify_ref as RR
from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.hip_lib import SvoError, lib
from stereo_svo_slam_amd.stereo_slam import StereoSlam, StereoSlamBatch
from test_rectify_gpu import StatsView, _euroc_maps, _final, _oracle, _render, _same_as_oracle, _snapshot

pytestmark = pytest.mark.gpu

W, H = 752, 480
FMT = {name: i for i, name in enumerate(IR.FORMATS)}
CONVERTING = [f for f in IR.FORMATS if f != "gray_pair"]


@pytest.fixture(scope="module")
def handle():
    h = hip_lib.Handle(0, 1024)
    yield h
    h.close()


# ------------------------------------------------------------------------------------------- stage

def _channels(fmt):
    return 1 if fmt in ("gray_pair", "sbs_gray") else 3


def _row_pixels(fmt, w):
    return 2 * w if fmt.startswith("sbs") else w


class Buf:
    """a [h, px(, 3)] uint8 image inside a flat device buffer: `off` bytes before it, rows `stride` bytes apart,
    everything that is not a pixel holds `fill`"""

    def __init__(self, h, px, channels, off, stride, fill, content=None):
        self.h, self.row, self.off, self.stride, self.fill = h, px * channels, off, stride, fill
        assert stride >= self.row
        self.flat = torch.full((off + h * stride + 64,), fill, dtype=torch.uint8, device="cuda")
        shape, strides = ((h, px, 3), (stride, 3, 1)) if channels == 3 else ((h, px), (stride, 1))
        self.view = torch.as_strided(self.flat, shape, strides, off)
        if content is not None:
            self.view.copy_(torch.from_numpy(content).cuda())

    def outside_untouched(self):
        flat = self.flat.cpu().numpy()
        mask = np.ones(flat.shape, bool)
        for y in range(self.h):
            mask[self.off + y * self.stride: self.off + y * self.stride + self.row] = False
        return bool((flat[mask] == self.fill).all())


def _convert(handle, fmt, srcs_a, srcs_b, w, h, src_off=0, src_pad=0, dst_off=0, dst_pad=0, sentinel=0x5a):
    """svo_convert_frames of host arrays through crafted device buffers; returns the (left, right) arrays per
    image after checking the output guards"""
    ch, px = _channels(fmt), _row_pixels(fmt, w)
    n = len(srcs_a)
    sa = [Buf(h, px, ch, src_off, px * ch + src_pad, sentinel, a) for a in srcs_a]
    sb = [Buf(h, px, ch, src_off, px * ch + src_pad, sentinel, b) for b in srcs_b] if srcs_b is not None else None
    dl = [Buf(h, w, 1, dst_off, w + dst_pad, 0xa5) for _ in range(n)]
    dr = [Buf(h, w, 1, dst_off, w + dst_pad, 0xa5) for _ in range(n)]
    handle.convert_frames(FMT[fmt], [b.view for b in sa], [b.view for b in sb] if sb else None, w,
                          [b.view for b in dl], [b.view for b in dr])
    handle.synchronize()
    for b in dl + dr:
        assert b.outside_untouched(), "a store outside the output rows"
    return [(l.view.cpu().numpy(), r.view.cpu().numpy()) for l, r in zip(dl, dr)]


def _check(handle, fmt, srcs_a, srcs_b, w, h, **kw):
    """the outputs equal the statement, whatever the bytes around the source rows hold"""
    for sentinel in (0x00, 0xff):
        got = _convert(handle, fmt, srcs_a, srcs_b, w, h, sentinel=sentinel, **kw)
        for i, (gl, gr) in enumerate(got):
            el, er = IR.convert(fmt, srcs_a[i], srcs_b[i] if srcs_b is not None else None, width=w)
            assert np.array_equal(gl, el), (fmt, i, "left", int(np.sum(gl != el)), kw)
            assert np.array_equal(gr, er), (fmt, i, "right", int(np.sum(gr != er)), kw)


def _random_bufs(fmt, w, h, n, seed):
    rng = np.random.default_rng(seed)
    shape = (h, _row_pixels(fmt, w)) + ((3,) if _channels(fmt) == 3 else ())
    a = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n)]
    b = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n)] if fmt not in IR.ONE_BUFFER else None
    return a, b


@pytest.mark.parametrize("fmt", IR.FORMATS)
def test_convert_random_images_sizes_and_alignments(handle, fmt):
    """every format on random images: the tracker's size and 1920 x 1080 on aligned buffers (the 16-byte path),
    tiny and odd sizes, widths that are no multiple of 16, bases at offset 1, 2, 3 and odd strides (the byte path)"""
    for w, h in ((752, 480), (1920, 1080)):
        a, b = _random_bufs(fmt, w, h, 2, w)
        _check(handle, fmt, a, b, w, h, dst_off=16)
    for k, (w, h) in enumerate(((1, 1), (5, 3), (17, 9), (100, 7), (333, 5), (48, 4))):
        a, b = _random_bufs(fmt, w, h, 3, 10 + k)
        _check(handle, fmt, a, b, w, h, src_off=16, src_pad=(-_row_pixels(fmt, w) * _channels(fmt)) % 4,
               dst_off=32, dst_pad=(-w) % 16)                     # aligned rows: wide path + tails
        for off in (1, 2, 3):
            _check(handle, fmt, a, b, w, h, src_off=off, src_pad=off, dst_off=16, dst_pad=(-w) % 16)
        _check(handle, fmt, a, b, w, h, src_off=4, src_pad=1, dst_off=3, dst_pad=5)      # odd strides, odd output
        _check(handle, fmt, a, b, w, h, src_off=0, src_pad=0, dst_off=0, dst_pad=0)      # dense


@functools.lru_cache(None)
def _boundary_colours():
    """colours whose weighted sum lies exactly on a rounding boundary (low 15 bits 16384: the first value that
    rounds up) or as closely below it as any colour gets (the weights reach only some residues: found by search),
    ordered as a ramp in Y"""
    v = np.arange(256, dtype=np.int32)
    b, g, r = np.meshgrid(v, v, v, indexing="ij")
    acc = (IR.B15 * b + IR.G15 * g + IR.R15 * r).ravel()
    res = acc & 0x7fff
    below = int(res[res < 16384].max())
    assert 16384 - 8 <= below < 16384 and (res == 16384).any(), "the ramp hits the boundary from both sides"
    pick = np.flatnonzero((res == below) | (res == 16384))
    pick = pick[np.argsort(acc[pick], kind="stable")]
    cols = np.stack([b.ravel()[pick], g.ravel()[pick], r.ravel()[pick]], -1).astype(np.uint8)
    y = IR.gray_of(cols, "bgr").astype(np.int64)
    exact = acc[pick] / 32768.0
    assert np.array_equal(y, np.where(res[pick] == 16384, np.ceil(exact), np.floor(exact)).astype(np.int64))
    return cols


@pytest.mark.parametrize("fmt", CONVERTING)
def test_convert_constant_channel_and_boundary_images(handle, fmt):
    """all 0, all 255, each single channel at 255, and a ramp of the colours at the rounding boundary"""
    w, h = 64, 40
    ch, px = _channels(fmt), _row_pixels(fmt, w)
    shape = (h, px, 3) if ch == 3 else (h, px)
    images = [np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]
    if ch == 3:
        for k in range(3):
            im = np.zeros(shape, np.uint8)
            im[..., k] = 255
            images.append(im)
        cols = _boundary_colours()
        ramp = np.resize(cols, (h * px, 3)).reshape(shape)
        assert len(cols) >= 100
        images.append(np.ascontiguousarray(ramp))
        images.append(np.ascontiguousarray(ramp[..., ::-1]))
    b = [im[::-1].copy() for im in images] if fmt not in IR.ONE_BUFFER else None
    _check(handle, fmt, images, b, w, h, dst_off=16)
    _check(handle, fmt, images, b, w, h, src_off=1, src_pad=2, dst_off=1, dst_pad=3)


@pytest.mark.parametrize("n", [1, 7, 300])
def test_convert_counts(handle, n):
    w, h = 80, 24
    for fmt in ("sbs_bgr", "rgb_pair", "ch3_econ", "sbs_gray"):
        a, b = _random_bufs(fmt, w, h, n, 1000 + n)
        _check(handle, fmt, a, b, w, h, dst_off=16)


def test_convert_rejects_bad_calls(handle):
    f = lib().svo_convert_frames
    col = torch.zeros((16, 32, 3), dtype=torch.uint8, device="cuda")
    a = (hip_lib.Image * 1)(hip_lib._raw_img(col, 3))
    out = hip_lib._imgs([torch.zeros((16, 16), dtype=torch.uint8, device="cuda")])
    small = hip_lib._imgs([torch.zeros((8, 8), dtype=torch.uint8, device="cuda")])
    assert f(handle._h, FMT["sbs_bgr"], 0, a, None, out, out) == -1           # n
    assert f(handle._h, 7, 1, a, None, out, out) == -1                        # format
    assert f(handle._h, -1, 1, a, None, out, out) == -1
    assert f(handle._h, FMT["sbs_bgr"], 1, None, None, out, out) == -1        # no source
    assert f(handle._h, FMT["bgr_pair"], 1, a, None, out, out) == -1          # a pair format without src_b
    assert f(handle._h, FMT["sbs_bgr"], 1, a, None, out, None) == -1
    assert f(handle._h, FMT["sbs_bgr"], 1, a, None, out, small) == -1         # outputs of two sizes
    wide = hip_lib._imgs([torch.zeros((16, 17), dtype=torch.uint8, device="cuda")])
    assert f(handle._h, FMT["sbs_bgr"], 1, a, None, wide, wide) == -1         # the buffer has fewer than 2 W pixels
    bad = (hip_lib.Image * 1)(hip_lib.Image(col.data_ptr(), 32, 16, 95))      # stride below the row's bytes
    assert f(handle._h, FMT["sbs_bgr"], 1, bad, None, out, out) == -1
    with pytest.raises(SvoError):
        hip_lib._check(f(handle._h, 99, 1, a, None, out, out))
    # the handle still works
    a_np, _ = _random_bufs("sbs_bgr", 16, 16, 1, 3)
    _check(handle, "sbs_bgr", a_np, None, 16, 16)


# ------------------------------------------------------------------------------------------ tracker

def _colour_frames(rendered, lengths=None):
    """per sequence the coloured frames [F, 2, H, W, 3] (B, G, R; 0 left, 1 right; device) made from the rendered
    gray ones by per-channel gains and offsets with clipping, and the statement's gray images of them
    ([F, H, W] left, right; device)"""
    colour, gray = [], []
    for s, r in enumerate(rendered):
        n = lengths[s] if lengths else len(r[4])
        sides = []
        for side in (1, 2):
            g = r[side][:n].cpu().numpy()
            sides.append(np.stack([IR.colourize(g[k], 1000 * s + 10 * k + side) for k in range(n)]))
        c = np.stack(sides, 1)
        assert (c[..., 0] != c[..., 2]).mean() > 0.5, "genuinely coloured"
        colour.append(torch.from_numpy(c).cuda())
        gray.append((torch.from_numpy(IR.gray_of(c[:, 0], "bgr")).cuda(), torch.from_numpy(IR.gray_of(c[:, 1], "bgr")).cuda()))
    return colour, gray


def _pack_dev(fmt, lc, rc, gl=None, gr=None):
    """IR.pack on device tensors (lc, rc: [H, W, 3] B, G, R): the buffers (a, b) of format fmt. gl, gr: the
    statement's gray images of lc, rc where the caller has them already"""
    if fmt == "bgr_pair":
        return lc, rc
    if fmt == "rgb_pair":
        return lc.flip(-1).contiguous(), rc.flip(-1).contiguous()
    if fmt == "sbs_bgr":
        return torch.cat([rc, lc], 1).contiguous(), None
    if fmt == "sbs_rgb":
        return torch.cat([rc, lc], 1).flip(-1).contiguous(), None
    if gl is None:
        gl, gr = (torch.from_numpy(IR.gray_of(t.cpu().numpy(), "bgr")).cuda() for t in (lc, rc))
    if fmt == "gray_pair":
        return gl, gr
    if fmt == "sbs_gray":
        return torch.cat([gr, gl], 1).contiguous(), None
    if fmt == "ch3_econ":
        return torch.stack([gl ^ 0x55, gr, gl], -1).contiguous(), None
    raise ValueError(fmt)


def test_device_packing_is_the_statements():
    rng = np.random.default_rng(1)
    lc, rc = (rng.integers(0, 256, (6, 8, 3), dtype=np.uint8) for _ in range(2))
    for fmt in IR.FORMATS:
        a, b = _pack_dev(fmt, torch.from_numpy(lc).cuda(), torch.from_numpy(rc).cuda())
        got = IR.convert(fmt, a.cpu().numpy(), None if b is None else b.cpu().numpy())
        want = IR.convert(fmt, *IR.pack(fmt, lc, rc))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), fmt


def _drive(cfg, n_seq, n_steps, feed, fmt="gray_pair", mode="device", maps=None, restarts=None, overwrite=False,
           switch=None, stamp=None):
    """one ctx of n_seq slots through n_steps steps. feed(s, k, fmt) -> (a, b) device tensors (b None for one
    buffer) or None: the slot sits the step out. mode 'host' | 'device' | 'borrow'. restarts: {step: slots ended
    before it}. switch: {step: format set before it}. stamp(s, k): the time stamp of slot s at step k (default k / 20). overwrite: the buffers handed over are copies that are
    filled with noise after each step. Returns per step {slot: snapshot}, the final trajectories / keyframes,
    the groups and the ctx's memory record."""
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_seq)
    if maps is not None:
        slam.set_rectification(*maps)
    slam.set_input_format(fmt)
    frames = []
    for k in range(n_steps):
        if switch and k in switch:
            fmt = switch[k]
            slam.set_input_format(fmt)
        if restarts and k in restarts:
            slam.restart(restarts[k])
        bufs = [feed(s, k, fmt) for s in range(n_seq)]
        act = [s for s in range(n_seq) if bufs[s] is not None]
        if overwrite:
            bufs = [None if b is None else tuple(None if t is None else t.clone() for t in b) for b in bufs]
        A = [None if b is None else b[0] for b in bufs]
        Bs = [None if b is None else b[1] for b in bufs]
        ts = [stamp(s, k) if stamp else k / 20.0 for s in range(n_seq)]
        torch.cuda.synchronize()
        if mode == "host":
            slam.new_images([None if t is None else t.cpu().numpy() for t in A],
                            [None if t is None else t.cpu().numpy() for t in Bs], ts)
        elif mode == "device":
            slam.new_images(A, Bs, ts)
        else:
            slam.submit_packed(slam.pack_images(A, Bs, ts, borrow=True))
            slam.wait()
        if overwrite:
            for t in A + Bs:
                if t is not None:
                    t.random_(0, 255)
            torch.cuda.synchronize()
        frames.append({s: _snapshot(slam, s) for s in act})
    final = [_final(slam, s) for s in range(n_seq)]
    groups, mem = slam.groups(), slam.memory()
    slam.close()
    return frames, final, groups, mem


@pytest.fixture(scope="module")
def c2_colour():
    rendered = _render(16, 32)
    colour, gray = _colour_frames(rendered)
    return rendered[0][0], colour, gray


def _feed_of(colour, gray, lengths=None, first=None):
    """feed for _drive: sequence s plays its frames from step first[s] on"""
    def feed(s, k, fmt):
        k0 = first[s] if first else 0
        n = lengths[s] if lengths else colour[s].shape[0]
        if k < k0 or k - k0 >= n:
            return None
        if fmt == "gray_pair":
            return gray[s][0][k - k0], gray[s][1][k - k0]
        return _pack_dev(fmt, colour[s][k - k0, 0], colour[s][k - k0, 1], gray[s][0][k - k0], gray[s][1][k - k0])
    return feed


def test_colour_frames_equal_the_default_format_on_gray(monkeypatch, c2_colour):
    """C2, 16 sequences in 2 groups, 32 frames with keyframes inside: each of the six other formats, in the three
    memory modes, gives bit for bit what the default format gives on the statement's gray images: per frame pose,
    keypoints, info and frame stats, at the end trajectories and keyframes"""
    cfg, colour, gray = c2_colour
    monkeypatch.setenv("SVO_GROUPS", "2")
    feed = _feed_of(colour, gray)
    ref_frames, ref_final, groups, _ = _drive(cfg, 16, 32, feed)
    assert groups == 2
    assert any(StatsView(snap[4]).is_keyframe for fr in ref_frames[1:] for snap in fr.values()), "a keyframe inside"
    for fmt in CONVERTING:
        for mode in ("host", "device", "borrow"):
            frames, final, _, _ = _drive(cfg, 16, 32, feed, fmt=fmt, mode=mode)
            assert frames == ref_frames, (fmt, mode)
            assert final == ref_final, (fmt, mode)


@pytest.fixture(scope="module")
def gray_unequal():
    """8 sequences of unequal length; slot 4 (6 frames) is restarted and plays sequence 8 from step 7 on"""
    rendered = _render(9, 14, seed0=500)
    lengths = [14, 14, 9, 14, 6, 14, 11, 14, 7]
    host = [(r[1].cpu().numpy(), r[2].cpu().numpy(), n) for r, n in zip(rendered, lengths)]
    return rendered, lengths, host


def _equal_channels(rendered, lengths):
    """R = G = B frames: [F, 2, H, W, 3] per sequence, and the gray ones as the statement has them (the same)"""
    colour, gray = [], []
    for r, n in zip(rendered, lengths):
        c = torch.stack([r[1][:n], r[2][:n]], 1)[..., None].expand(-1, -1, -1, -1, 3).contiguous()
        colour.append(c)
        gray.append((r[1][:n], r[2][:n]))
    return colour, gray


def _slot_plan():
    """slots 0..7 play sequences 0..7 from step 0; slot 4's ends after 6 frames, and after a restart before step 7
    it plays sequence 8. Returns feed-index helpers: which (sequence, frame) slot s has at step k, or None."""
    def at(lengths, s, k):
        if s == 4 and k >= 7:
            return (8, k - 7) if k - 7 < lengths[8] else None
        return (s, k) if k < lengths[s] else None
    return at


def test_equal_channel_frames_equal_the_oracle(monkeypatch, gray_unequal):
    """R = G = B packed frames (every format that converts, device memory; sbs_bgr also from the host) == the oracle
    on the original gray frames, with sequences of unequal length and a restart inside"""
    rendered, lengths, host = gray_unequal
    monkeypatch.setenv("SVO_GROUPS", "2")
    oracle = _oracle(host, rendered[0][0], lambda k: None)
    colour, gray = _equal_channels(rendered, lengths)
    at = _slot_plan()

    def feed(s, k, fmt):
        w = at(lengths, s, k)
        if w is None:
            return None
        q, i = w
        return _pack_dev(fmt, colour[q][i, 0], colour[q][i, 1], gray[q][0][i], gray[q][1][i])

    def stamp(s, k):
        w = at(lengths, s, k)
        return w[1] / 20.0 if w else 0.0

    for fmt, mode in [(f, "device") for f in CONVERTING] + [("sbs_bgr", "host"), ("ch3_econ", "borrow")]:
        frames, final, groups, _ = _drive(rendered[0][0], 8, 14, feed, fmt=fmt, mode=mode, restarts={7: [4]}, stamp=stamp)
        assert groups == 2
        seen = set()
        for k, fr in enumerate(frames):
            for s, snap in fr.items():
                q, i = at(lengths, s, k)
                seen.add(q)
                _same_as_oracle(f"{fmt} {mode} slot {s} step {k}", snap, oracle[q][0][i])
        assert seen == set(range(9))
        for s in range(8):
            q = 8 if s == 4 else s
            assert np.array_equal(np.frombuffer(final[s][0], np.float32).reshape(-1, 6), oracle[q][1]), (fmt, s)
    assert any(o[0] for seq in oracle for o in seq[0][1:]), "a keyframe inside the run"


def test_side_by_side_gray_borrowed_is_used_in_place(monkeypatch, c2_colour):
    """SVO_INPUT_SBS_GRAY with borrowed frames: nothing is converted or copied. Equal to the default format given
    the two half pointers, with no more image sets or device bytes than that run"""
    cfg, colour, gray = c2_colour
    monkeypatch.setenv("SVO_GROUPS", "2")
    n = 12
    sbs = [torch.cat([gray[s][1][:n], gray[s][0][:n]], 2).contiguous() for s in range(4)]     # [n, H, 2W]

    def halves(s, k, fmt):
        return sbs[s][k][:, W:], sbs[s][k][:, :W]                   # views into the frame: left = right half

    ref = _drive(cfg, 4, n, halves, mode="borrow")
    got = _drive(cfg, 4, n, lambda s, k, fmt: (sbs[s][k], None), fmt="sbs_gray", mode="borrow")
    assert got[0] == ref[0] and got[1] == ref[1]
    assert got[3].image_sets <= ref[3].image_sets and got[3].device_bytes <= ref[3].device_bytes
    # and in the copying modes
    for mode in ("device", "host"):
        other = _drive(cfg, 4, n, lambda s, k, fmt: (sbs[s][k], None), fmt="sbs_gray", mode=mode)
        assert other[0] == ref[0] and other[1] == ref[1], mode


def test_borrowed_buffers_of_converting_formats_may_be_reused(monkeypatch, c2_colour):
    """borrowed raw buffers are read once during the step: overwritten with noise after each wait, results unchanged"""
    cfg, colour, gray = c2_colour
    monkeypatch.setenv("SVO_GROUPS", "2")
    n = 12
    short = [c[:n] for c in colour[:6]], [(g[0][:n], g[1][:n]) for g in gray[:6]]
    feed = _feed_of(*short)
    ref = _drive(cfg, 6, n, feed)
    for fmt in ("sbs_bgr", "rgb_pair", "ch3_econ"):
        got = _drive(cfg, 6, n, feed, fmt=fmt, mode="borrow", overwrite=True)
        assert got[0] == ref[0] and got[1] == ref[1], fmt


def test_colour_side_by_side_with_rectification_equals_the_oracle(monkeypatch, gray_unequal):
    """colour side-by-side frames plus EuRoC-like maps == the oracle on remap(statement gray): the order is
    format -> remap -> pyramids. Host, device and borrowed (overwritten) buffers; ch3_econ too."""
    rendered, lengths, _ = gray_unequal
    rendered, lengths = rendered[:4], [10, 7, 10, 5]
    monkeypatch.setenv("SVO_GROUPS", "2")
    maps = _euroc_maps()
    colour, gray = _colour_frames(rendered, lengths)
    host = [(g[0].cpu().numpy(), g[1].cpu().numpy(), n) for g, n in zip(gray, lengths)]
    oracle = _oracle(host, rendered[0][0], lambda k: maps)
    feed = _feed_of(colour, gray, lengths)
    for fmt, mode, ow in (("sbs_bgr", "device", False), ("sbs_rgb", "host", False), ("sbs_bgr", "borrow", True),
                          ("ch3_econ", "device", False), ("sbs_gray", "borrow", True)):
        frames, final, _, mem = _drive(rendered[0][0], 4, 10, feed, fmt=fmt, mode=mode, maps=maps, overwrite=ow)
        for k, fr in enumerate(frames):
            for s, snap in fr.items():
                _same_as_oracle(f"{fmt} {mode} seq {s} frame {k}", snap, oracle[s][0][k])
        for s in range(4):
            assert np.array_equal(np.frombuffer(final[s][0], np.float32).reshape(-1, 6), oracle[s][1]), (fmt, s)
        assert mem.device_bytes > 0


def test_switching_the_format_between_frames(c2_colour):
    """default for steps 0-3, sbs_rgb 4-7, ch3_econ 8-10, bgr_pair 11-12, default again 13-15: every frame follows
    the format in force and the run equals the default format on gray throughout"""
    cfg, colour, gray = c2_colour
    feed = _feed_of([c[:16] for c in colour[:2]], [(g[0][:16], g[1][:16]) for g in gray[:2]])
    ref = _drive(cfg, 2, 16, feed)
    plan = {4: "sbs_rgb", 8: "ch3_econ", 11: "bgr_pair", 13: "gray_pair"}
    for mode in ("device", "host"):
        got = _drive(cfg, 2, 16, feed, mode=mode, switch=plan)
        assert got[0] == ref[0] and got[1] == ref[1], mode
    # a format given before the first frame applies to it (StereoSlam makes its ctx with that frame)
    one = StereoSlam(cfg)
    one.set_input_format("sbs_bgr")
    a, _ = _pack_dev("sbs_bgr", colour[0][0, 0], colour[0][0, 1])
    one.new_image(a.cpu().numpy(), None, 0.0)
    assert (one.width, one.height) == (W, H)
    assert _snapshot(one, 0) == ref[0][0][0]
    one.close()


def test_invalid_format_calls_leave_the_ctx_usable(c2_colour):
    cfg, colour, gray = c2_colour
    slam = StereoSlamBatch(cfg, W, H, 1)
    ref = StereoSlamBatch(cfg, W, H, 1)
    f = lib().svo_ctx_set_input_format
    assert f(slam._ctx, 7) == -1 and f(slam._ctx, -1) == -1 and f(None, 1) == -1
    with pytest.raises(SvoError):
        slam.set_input_format(42)
    L, R = gray[0]
    for k in range(2):
        slam.new_images([L[k]], [R[k]], [k / 20.0])
        ref.new_images([L[k]], [R[k]], [k / 20.0])
        assert _snapshot(slam, 0) == _snapshot(ref, 0)
    assert f(slam._ctx, FMT["sbs_bgr"]) == 0 and f(slam._ctx, 9) == -1          # the bad call keeps sbs_bgr
    ptrs = (C.c_void_p * 1)()
    ts = (C.c_float * 1)(0.1)
    a, _ = _pack_dev("sbs_bgr", colour[0][2, 0], colour[0][2, 1])
    ptrs[0] = a.data_ptr()
    torch.cuda.synchronize()
    assert lib().svo_new_images(slam._ctx, ptrs, None, 2 * W * 3 - 1, ts, 1) == -1     # stride below the row's bytes
    assert lib().svo_new_images(slam._ctx, ptrs, None, 2 * W * 3, ts, 1) == 0      # right array NULL: ignored
    ref.new_images([L[2]], [R[2]], [0.1])
    assert _snapshot(slam, 0) == _snapshot(ref, 0)
    assert f(slam._ctx, 0) == 0
    assert lib().svo_new_images(slam._ctx, ptrs, None, W, ts, 1) == -1                 # the pair formats need both arrays
    slam.new_images([L[3]], [R[3]], [0.15])
    ref.new_images([L[3]], [R[3]], [0.15])
    assert _snapshot(slam, 0) == _snapshot(ref, 0)
    slam.close(); ref.close()


def test_new_image_with_a_one_buffer_format(c2_colour):
    """svo_new_image: right and right_stride are ignored, width and height stay the ctx's"""
    cfg, colour, gray = c2_colour
    ref = StereoSlamBatch(cfg, W, H, 1)
    one = StereoSlamBatch(cfg, W, H, 1)
    one.set_input_format("sbs_bgr")
    for k in range(5):
        a = _pack_dev("sbs_bgr", colour[1][k, 0], colour[1][k, 1])[0].cpu().numpy()
        hip_lib._check(lib().svo_new_image(one._ctx, a.ctypes.data_as(C.c_void_p), a.strides[0], None, 12345, W, H,
                                           C.c_float(k / 20.0)))
        ref.new_images([gray[1][0][k]], [gray[1][1][k]], [k / 20.0])
        assert _snapshot(one, 0) == _snapshot(ref, 0), k
    assert lib().svo_new_image(one._ctx, a.ctypes.data_as(C.c_void_p), a.strides[0], None, 0, 2 * W, H, C.c_float(1.0)) == -1
    assert _final(one, 0) == _final(ref, 0)
    one.close(); ref.close()


# ------------------------------------------------------------------------------------------- replay

def test_replay_gpu_ingest_equals_the_host_split(tmp_path):
    """colour side-by-side PNG frames and 3-channel Econ frames: `replay --gpu-ingest` (raw frames into the
    library) writes the poses of the host-converted run"""
    from PIL import Image
    cfg, L, R, _, _ = synth.make_sequence("tiny", 4, 0, device="cpu")
    keys = "".join(f"{k}: {cfg[f]}\n" for k, f in replay._YAML_KEYS.items())
    y = tmp_path / "cam.yaml"
    y.write_text("%YAML:1.0\n" + keys + f"Camera.width: {cfg['width']}\nCamera.height: {cfg['height']}\n")
    for name in ("sbs", "econ"):
        (tmp_path / name).mkdir()
    for k in range(4):
        lc, rc = IR.colourize(L[k].numpy(), 2 * k), IR.colourize(R[k].numpy(), 2 * k + 1)
        sbs = IR.pack("sbs_bgr", lc, rc)[0]
        econ = IR.pack("ch3_econ", lc, rc)[0]
        Image.fromarray(np.ascontiguousarray(sbs[..., ::-1])).save(str(tmp_path / "sbs" / f"{k:06d}.png"))
        Image.fromarray(np.ascontiguousarray(econ[..., ::-1])).save(str(tmp_path / "econ" / f"{k:06d}.png"))
    for name, flag in (("sbs", "--sbs"), ("econ", "--interleaved")):
        rows = []
        for extra in ([], ["--gpu-ingest"]):
            out = tmp_path / f"{name}{len(extra)}.csv"
            replay.main(["--settings", str(y), flag, str(tmp_path / name / "%06d.png"), "--frames", "4", "-t", str(out)] + extra)
            rows.append(np.loadtxt(str(out), delimiter=","))
        assert rows[0].shape == (4, 7) and np.array_equal(rows[0][:, 1:], rows[1][:, 1:]), name
        assert np.abs(rows[0][1:, 1:4]).max() > 0
