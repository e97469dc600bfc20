"""The views (svo_submit_export_views / svo_render_views) on the GPU. The yardsticks: the numpy restatement
(tests/view_ref.py) for the stage entry on crafted inputs; for the ctx the frames given, numpy's 2x2 mean chain, the
planes of a snapshot (tests/snapshot_ref.py), rectify_ref and ingest_ref for the gray planes, and view_ref rendered
from the getters' state for the marker views. Every comparison is on bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import ingest_ref as IR
import rectify_ref as RR
import snapshot_ref as SR
import view_ref as VR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import Handle
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu

FILL = 0xA5
FRAMES, KEYFRAMES = hip_lib.EXPORT_FRAMES, hip_lib.EXPORT_LAST_KEYFRAMES


def _style(plane=0, level=0, pixel=0, markers=0, drop_flags=0, size=10, size_temporary=10, reserved=0):
    return hip_lib.ViewStyle(plane, level, pixel, markers, drop_flags, size, size_temporary, reserved)


# ---------------------------------------------------------------------------------- stage entry on crafted inputs

def _on_device(raw, offset, keep):
    """the bytes in device memory at a base `offset` bytes past an allocation's start: the address"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    buf = np.full(offset + raw.size + 16, 0x5A, np.uint8)
    buf[offset:offset + raw.size] = raw
    t = torch.from_numpy(buf).cuda()
    keep.append(t)
    return t.data_ptr() + offset


def _plane(rng, w, h, extra, offset, keep):
    """a random gray plane of w x h with `extra` bytes between its rows, `offset` bytes past an allocation:
    (host [h, w], (address, w, h, stride))"""
    rows = rng.integers(0, 256, (h, w + extra), dtype=np.uint8)
    return rows[:, :w].copy(), (_on_device(rows, offset, keep), w, h, w + extra)


def _kps(k2, flags, types, colors, keep, rng):
    """a keypoint set on the device: (n, fields). level_type carries a random level byte and the type, the colour word
    a random top byte, the flags word random bits above the three"""
    n = len(k2)
    k2 = np.asarray(k2, np.float32).reshape(n, 2)
    lt = (np.asarray(types, np.int64) << 8 | rng.integers(0, 8, n)).astype(np.int32)
    col = np.asarray(colors, np.uint32).reshape(n, 3)
    word = (col[:, 0] | col[:, 1] << 8 | col[:, 2] << 16 | rng.integers(0, 256, n).astype(np.uint32) << 24).astype(np.uint32)
    fl = (np.asarray(flags, np.uint32) | (rng.integers(0, 2**20, n).astype(np.uint32) << 3)).astype(np.uint32)
    fields = {"kps2d": _on_device(k2, 4, keep), "flags": _on_device(fl, 12, keep), "level_type": _on_device(lt, 4, keep),
              "color": _on_device(word, 8, keep)}
    return n, fields


def _random_set(rng, n, w, h, level):
    """n keypoints, heavy overlap: most on a few centres in and around the w x h image of `level`"""
    centres = np.stack([rng.integers(-8, w + 8, 9), rng.integers(-8, h + 8, 9)], 1).astype(np.float32)
    k2 = centres[rng.integers(0, 9, n)] + rng.random((n, 2)).astype(np.float32)
    far = rng.random(n) < 0.3
    k2[far] = np.stack([rng.uniform(-40, w + 40, far.sum()), rng.uniform(-40, h + 40, far.sum())], 1)
    return k2 * np.float32(1 << level), rng.integers(0, 8, n), rng.integers(0, 2, n), rng.integers(0, 256, (n, 3))


def _render_and_check(h, images, style, base=4, tag=""):
    """images: [(host gray, device image, host set or None, device set or None)] rendered in one call into a
    destination pre-filled with FILL whose `pixels` is `base` bytes past a 256-byte aligned allocation; every byte of
    the destination equals the restatement's"""
    bpp = VR.BYTES[style.pixel]
    offsets, at = [], 8
    for gray, *_ in images:
        offsets.append(at)
        at += (gray.size * bpp + 3) // 4 * 4 + 4 * (len(offsets) % 3)       # gaps of 0, 4, 8 bytes between the images
    total = at + 12
    want_imgs = []
    for gray, _, hs, _ in images:
        if style.markers and hs is not None:
            want_imgs.append(VR.render(gray, style.pixel, hs[0], hs[1], hs[2], hs[3], style.level, style.drop_flags,
                                       style.size, style.size_temporary))
        else:
            want_imgs.append(VR.expand(gray, style.pixel))
    want = np.full(base + total, FILL, np.uint8)
    want[base:] = VR.place(want_imgs, offsets, total, FILL)
    dst = torch.full((base + total,), FILL, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 256 == 0
    h.render_views([(img, ds) for _, img, _, ds in images], offsets, style, dst.data_ptr() + base)
    got = dst.cpu().numpy()
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at {bad[0] - base} (offsets {offsets})")


WIDTHS = (1, 3, 4, 5, 63, 64, 65, 67, 257)
HEIGHTS = (1, 2, 16, 17)


@pytest.mark.parametrize("pixel", [VR.GRAY8, VR.RGB8, VR.RGBA8])
def test_render_sizes_strides_and_alignments(pixel):
    """every width x height in one call, in two orders; source strides beyond the width, source bases 0 - 3 bytes
    past an allocation, pixels 4-byte but not 16-byte aligned; with markers where the format has them"""
    h = Handle(0, 1024)
    rng = np.random.default_rng(10 + pixel)
    keep, images = [], []
    for i, (w, ht) in enumerate((w, ht) for w in WIDTHS for ht in HEIGHTS):
        gray, img = _plane(rng, w, ht, (0, 1, 7, 64)[i % 4], i % 4, keep)
        hs = _random_set(rng, 12, w, ht, 0)
        images.append((gray, img, hs, _kps(*hs, keep, rng)))
    torch.cuda.synchronize()
    markers = int(pixel != VR.GRAY8)
    for order, base in ((images, 4), (images[::-1], 12), (images[::5], 0)):
        _render_and_check(h, order, _style(0, 0, pixel, markers, 0, 10, 20), base, f"pixel {pixel} base {base}")
        _render_and_check(h, order, _style(0, 0, pixel, 0), base, f"plain pixel {pixel} base {base}")
    h.close()


def _crafted_set(w, h):
    """centres inside, on each border, outside by less than half a marker, far outside, the truncation and the
    non-finite cases, tile seams, and stacks on one centre (a cross over a square and the reverse): (x, y, type)"""
    c = [(20, 20, 0), (100, 30, 1), (40.75, 8.25, 0), (90.5, 22.99, 1)]
    c += [(0, 10, 0), (w - 1, 10, 1), (50, 0, 1), (50, h - 1, 0), (0, 0, 1), (w - 1, h - 1, 0), (0, h - 1, 0), (w - 1, 0, 1)]
    c += [(-3, 12, 0), (-3, 25, 1), (w + 2, 12, 1), (w + 2, 25, 0), (70, -4, 0), (85, -4, 1), (70, h + 3, 1), (85, h + 3, 0)]
    c += [(-500, 10, 0), (5000, 5000, 1), (10, -40, 0), (w + 33, 5, 1), (w + 32, 5, 0)]
    c += [(-0.5, 30, 0), (30, -0.5, 1), (-0.99, -0.99, 0)]
    nan, inf = float("nan"), float("inf")
    c += [(nan, 5, 0), (5, nan, 1), (inf, 5, 0), (5, -inf, 1), (-inf, inf, 0), (1e10, 5, 1), (5, -1e10, 0), (-1e10, 1e10, 1),
          (32768.0, 5, 0), (5, -32768.0, 1)]
    c += [(63, 15, 0), (64, 16, 1), (63, 16, 1), (64, 15, 0), (63.5, 20, 1), (64, 5, 0), (120, 15, 1), (120, 16, 0), (127, 31, 1), (128, 32, 0)]
    c += [(40, 20, t) for t in (1, 0, 0, 1, 1, 0)] + [(110, 10, t) for t in (0, 1, 0)]
    return c


SIZES = ((0, 1), (1, 0), (10, 20), (20, 64), (64, 10))
COUNTS = (0, 1, 255, 256, 257, 1000)


@pytest.mark.parametrize("level", [0, 2])
def test_render_markers(level):
    """sets of every count, crafted centres first and seeded random ones behind them, every drop_flags combination,
    every size as size and as size_temporary, both pixel formats with markers"""
    h = Handle(0, 1024)
    rng = np.random.default_rng(20 + level)
    w, ht = 131, 37
    keep, images = [], []
    crafted = _crafted_set(w, ht)
    for n in COUNTS:
        k2, flags, types, colors = _random_set(rng, n, w, ht, level)
        m = min(n, len(crafted))
        if m:
            k2[:m] = np.float32([[x, y] for x, y, _ in crafted[:m]]) * np.float32(1 << level)
            types[:m] = [t for _, _, t in crafted[:m]]
        if level and m:                                            # (a sub-pixel position of the level: truncated after the scaling)
            k2[:m:3] += np.float32((1 << level) - 1)
        gray, img = _plane(rng, w, ht, 5, len(images) % 4, keep)
        hs = (k2, flags, types, colors)
        images.append((gray, img, hs, _kps(*hs, keep, rng)))
    torch.cuda.synchronize()
    seen = set()
    for drop in range(8):
        size, size_t = SIZES[(drop + 3 * (level // 2)) % 5]
        seen.add((size, size_t))
        for pixel in (VR.RGB8, VR.RGBA8):
            _render_and_check(h, images, _style(0, level, pixel, 1, drop, size, size_t), 4 if drop % 2 else 0,
                              f"level {level} drop {drop} sizes {size}/{size_t} pixel {pixel}")
    assert seen == set(SIZES)
    h.close()


def test_render_through_a_small_tile_table(monkeypatch):
    """SVO_VIEW_TABLE_TILES=2: the same bytes through chunked launches"""
    monkeypatch.setenv("SVO_VIEW_TABLE_TILES", "2")
    h = Handle(0, 1024)
    rng = np.random.default_rng(30)
    keep, images = [], []
    for i, (w, ht) in enumerate(((257, 17), (5, 1), (64, 16), (131, 37), (65, 33))):
        gray, img = _plane(rng, w, ht, 3, i % 4, keep)
        hs = _random_set(rng, 300, w, ht, 0)
        images.append((gray, img, hs, _kps(*hs, keep, rng)))
    torch.cuda.synchronize()
    for pixel in (VR.GRAY8, VR.RGB8, VR.RGBA8):
        _render_and_check(h, images, _style(0, 0, pixel, int(pixel != VR.GRAY8), 2, 20, 10), 4, f"chunked pixel {pixel}")
    h.close()


def test_render_rejects_bad_calls():
    h = Handle(0, 1024)
    keep = []
    rng = np.random.default_rng(31)
    gray, img = _plane(rng, 20, 10, 0, 0, keep)
    hs = _random_set(rng, 5, 20, 10, 0)
    ds = _kps(*hs, keep, rng)
    dst = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    good = _style(0, 0, VR.RGB8, 1)

    def call(src=(img, ds), offset=0, style=good, pixels=None):
        h.render_views([src], [offset], style, dst.data_ptr() if pixels is None else pixels)

    call()
    for kw in (dict(offset=-4), dict(offset=2), dict(pixels=dst.data_ptr() + 2), dict(pixels=0),
               dict(src=((0, 20, 10, 20), ds)), dict(src=((img[0], 20, 10, 19), ds)), dict(src=((img[0], 0, 10, 20), ds)),
               dict(src=(img, (-1, ds[1]))), dict(src=(img, (5, dict(ds[1], color=ds[1]["color"] + 2)))),
               dict(src=(img, (5, dict(ds[1], kps2d=0)))),
               dict(style=_style(0, 8, VR.RGB8, 1)), dict(style=_style(0, 0, 3, 0)), dict(style=_style(0, 0, VR.GRAY8, 1)),
               dict(style=_style(1, 0, VR.RGB8, 1)), dict(style=_style(0, 0, VR.RGB8, 1, 8)),
               dict(style=_style(0, 0, VR.RGB8, 1, 0, 65)), dict(style=_style(0, 0, VR.RGB8, 0, reserved=1))):
        dst.fill_(FILL)
        with pytest.raises(hip_lib.SvoError):
            call(**kw)
        assert bool((dst == FILL).all()), kw
    h.render_views([], [], good, dst.data_ptr())            # nothing to do
    call()                                                    # the handle has kept working
    assert dst[:600].cpu().numpy().tobytes() == VR.render(gray, VR.RGB8, *hs, 0, 0, 10, 10).tobytes()
    h.close()


# ---------------------------------------------------------------------------------- the ctx

def _sequences(config, seeds, n_frames, motion_scale=4.0):
    out = []
    for seed in seeds:
        cfg, L, R, _, ts = synth.make_sequence_gpu(config, n_frames, seed, motion_scale=motion_scale)
        out.append((L, R, [float(t) for t in ts]))
    torch.cuda.synchronize()
    return cfg, out


def _frame_set(n, live):
    """live: {slot: (sequence tuple, frame index)} -> lefts, rights, time stamps of new_images / pack_images"""
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for slot, (seq, k) in live.items():
        L[slot], R[slot], ts[slot] = seq[0][k], seq[1][k], seq[2][k]
    return L, R, ts


def _half(a):
    """halfSample: the truncating mean of 2 x 2 blocks"""
    h, w = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
    a = a[:h, :w].astype(np.uint32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) // 4).astype(np.uint8)


def _chain(a, levels):
    out = [np.asarray(a, np.uint8)]
    for _ in range(1, levels):
        out.append(_half(out[-1]))
    return out


def _snapshot_planes(snap, cfg, which):
    """(left levels, right) of the image set of the current frame (which = "frame") or of the newest keyframe
    ("keyframe"; None when it is retired or missing) in a host-mode Snapshot, through snapshot_ref's parser"""
    ref = SR.parse(snap.host)
    if which == "frame":
        s = 0 if ref["frame_id"] >= 0 else -1
    else:
        s = ref["keyframes"][-1][2] if ref["keyframes"] else -1
    if s < 0:
        return None
    levels, lk = ref["pyramid_levels"], ref["lk_levels"]
    base = 14 + 12 * ref["n_keyframes"] + s * (levels + lk)

    def plane(i):
        off, row_bytes, rows = ref["directory"][i]
        return snap.data[off:off + rows * row_bytes].reshape(rows, row_bytes)

    return [plane(base + l) for l in range(levels)], plane(base + levels)


def _gray_views(batch, what, seqs=None, device=False):
    """the gray views of every level of the left plane, and of the right plane"""
    levels = batch.cam.max_pyramid_levels
    return ([batch.export_views(what, seqs, plane="left", level=l, device=device) for l in range(levels)],
            batch.export_views(what, seqs, plane="right", device=device))


def _np(img):
    return None if img is None else (img.cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img))


def _check_segment(tag, seg, batch, what, s, status=None):
    """a view segment against the getters"""
    st = batch.stats(s)
    empty = batch.get_trajectory(s).shape[0] == 0
    assert int(seg["seq"]) == s and int(seg["_pad"]) == 0, tag
    assert int(seg["frame_id"]) == (-1 if empty else st.frame_id), tag
    if what == FRAMES:
        f = batch.get_frame(s)
        assert int(seg["keyframe_id"]) == -1 and int(seg["n"]) == len(f.kps2d), tag
        assert seg["pose"].tobytes() == batch.pose(s).tobytes(), tag
        want = hip_lib.VIEW_NONE if empty else hip_lib.VIEW_OK
    else:
        nk = batch.num_keyframes(s)
        assert int(seg["keyframe_id"]) == nk - 1, tag
        if nk:
            f = batch.get_keyframe(None, s)
            assert int(seg["n"]) == len(f.kps2d) and seg["pose"].tobytes() == f.pose.tobytes(), tag
        else:
            assert int(seg["n"]) == 0 and seg["pose"].tobytes() == bytes(24), tag
        want = hip_lib.VIEW_OK if nk else hip_lib.VIEW_NONE
    if status is not None:
        want = status
    assert int(seg["status"]) == want, (tag, int(seg["status"]))


def _expected_markers(batch, what, s, style, gray):
    """view_ref rendered from the getters' state over the gray image"""
    f = batch.get_frame(s) if what == FRAMES else batch.get_keyframe(None, s)
    flags, types, colors = VR.info_arrays(f.info)
    return VR.render(gray, style.pixel, f.kps2d, flags, types, colors, style.level, style.drop_flags, style.size,
                     style.size_temporary), flags


def _check_marker_views(tag, batch, what, named, views, gray_views):
    """a marker job against view_ref over the gray job of the same slots and level"""
    assert len(views.segments) == len(named)
    for i, s in enumerate(named):
        _check_segment((tag, s), views.segments[i], batch, what, s)
        assert int(views.segments[i]["offset"]) == i * views.image_bytes
        got, gray = _np(views.image(i)), _np(gray_views.image(i))
        assert (got is None) == (gray is None), (tag, s)
        if got is not None:
            want, _ = _expected_markers(batch, what, s, views.style, gray)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, s)


def test_gray_planes_against_frames_chain_and_snapshot(monkeypatch):
    """tiny, 3 slots, 24 frames of fast motion: LEFT level 0 and RIGHT are the frames given, level l the 2 x 2 mean chain, and all of
    them the planes of a snapshot, for the current frame and the newest keyframe"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    steps = 24
    cfg, seqs = _sequences("tiny", (1, 11, 12), steps)
    n = 3
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n)
    levels = cfg["max_pyramid_levels"]
    kf_frame = [0] * n
    for k in range(steps):
        batch.new_images(*_frame_set(n, {s: (seqs[s], k) for s in range(n)}))
        for s in range(n):
            if batch.stats(s).is_keyframe:
                kf_frame[s] = k
        if k not in (0, 5, steps - 1) and not any(batch.stats(s).is_keyframe for s in range(n)):
            continue
        snaps = batch.save()
        for what, which in ((FRAMES, "frame"), (KEYFRAMES, "keyframe")):
            left, right = _gray_views(batch, what)
            for s in range(n):
                src = k if what == FRAMES else kf_frame[s]
                chain = _chain(seqs[s][0][src].cpu().numpy(), levels)
                planes = _snapshot_planes(snaps[s], cfg, which)
                assert planes is not None
                for l in range(levels):
                    img = left[l].image(s)
                    assert img.shape == (cfg["height"] >> l, cfg["width"] >> l) and img.dtype == np.uint8
                    assert img.tobytes() == chain[l].tobytes(), (k, what, s, l)
                    assert img.tobytes() == planes[0][l].tobytes(), (k, what, s, l)
                    _check_segment((k, what, s, l), left[l].segments[s], batch, what, s)
                assert right.image(s).tobytes() == seqs[s][1][src].cpu().numpy().tobytes(), (k, what, s)
                assert right.image(s).tobytes() == planes[1].tobytes(), (k, what, s)
    assert any(f > 0 for f in kf_frame), "a keyframe was made after the first frame"
    batch.close()


def _feed(one, frames):
    """the frames (one call of `frames[k]` each) into the 1-slot ctx; the index of the frame its newest keyframe shows"""
    kf = 0
    for k, give in enumerate(frames):
        give()
        if one.stats(0).is_keyframe:
            kf = k
    return kf


def test_gray_planes_with_rectification_input_format_and_borrowed_frames():
    cfg, seqs = _sequences("tiny", (5,), 3)
    W, H = cfg["width"], cfg["height"]
    L, R, ts = seqs[0][0].cpu().numpy(), seqs[0][1].cpu().numpy(), seqs[0][2]
    # rectification: the views show remap_linear of the raw frame
    left_maps = RR.euroc_like_maps(W, H, angle=0.012, shift=(1.5, -2.0), f_p=190.0, f_k=200.0)
    right_maps = RR.euroc_like_maps(W, H, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068, f_p=190.0, f_k=200.0)
    one = StereoSlamBatch(cfg, W, H, 1)
    one.set_rectification(left_maps, right_maps)
    kf = _feed(one, [lambda k=k: one.new_images([L[k]], [R[k]], [ts[k]]) for k in range(2)])
    assert one.export_views("frames").image(0).tobytes() == RR.remap_linear(L[1], *left_maps).tobytes()
    assert one.export_views("frames", plane="right").image(0).tobytes() == RR.remap_linear(R[1], *right_maps).tobytes()
    assert one.export_views("frames", level=1).image(0).tobytes() == _half(RR.remap_linear(L[1], *left_maps)).tobytes()
    assert one.export_views("last_keyframes").image(0).tobytes() == RR.remap_linear(L[kf], *left_maps).tobytes()
    one.close()
    # a converting input format: the views show ingest_ref's gray
    lc = [IR.colourize(L[k], 2 * k) for k in range(2)]
    rc = [IR.colourize(R[k], 2 * k + 1) for k in range(2)]
    one = StereoSlamBatch(cfg, W, H, 1)
    one.set_input_format("bgr_pair")
    kf = _feed(one, [lambda k=k: one.new_images([lc[k]], [rc[k]], [ts[k]]) for k in range(2)])
    gl, gr = IR.convert("bgr_pair", lc[1], rc[1])
    assert gl.tobytes() != L[1].tobytes()
    assert one.export_views("frames").image(0).tobytes() == gl.tobytes()
    assert one.export_views("frames", plane="right").image(0).tobytes() == gr.tobytes()
    kl, kr = IR.convert("bgr_pair", lc[kf], rc[kf])
    assert one.export_views("last_keyframes").image(0).tobytes() == kl.tobytes()
    assert one.export_views("last_keyframes", plane="right").image(0).tobytes() == kr.tobytes()
    one.close()
    # borrowed device frames with a row pitch beyond the width: level 0 and the right image are the caller's buffers
    bl = torch.zeros((3, H, W + 24), dtype=torch.uint8, device="cuda")
    br = torch.zeros((3, H, W + 24), dtype=torch.uint8, device="cuda")
    bl[:, :, :W], br[:, :, :W] = seqs[0][0], seqs[0][1]
    torch.cuda.synchronize()
    one = StereoSlamBatch(cfg, W, H, 1)
    kf = _feed(one, [lambda k=k: one.new_images_packed(one.pack_images([bl[k, :, :W]], [br[k, :, :W]], [ts[k]], borrow=True))
                     for k in range(3)])
    for device in (False, True):
        assert _np(one.export_views("frames", device=device).image(0)).tobytes() == L[2].tobytes()
        assert _np(one.export_views("frames", plane="right", device=device).image(0)).tobytes() == R[2].tobytes()
        assert _np(one.export_views("last_keyframes", device=device).image(0)).tobytes() == L[kf].tobytes()
        assert _np(one.export_views("frames", level=2, device=device).image(0)).tobytes() == _chain(L[2], 3)[2].tobytes()
        v = one.export_views("frames", pixel="rgb8", markers=True, device=device)
        want, _ = _expected_markers(one, FRAMES, 0, v.style, L[2])
        assert _np(v.image(0)).tobytes() == want.tobytes()
    one.close()


def test_marker_views_against_the_getters(monkeypatch):
    """tiny, 5 slots, 24 frames of fast motion (keyframes are made later on, keypoints carry flags): at four steps of
    the run RGB and RGBA views of frames and of last keyframes, at levels 0 and 2, equal view_ref over the getters'
    state"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    n, steps, starts = 5, 24, [0, 0, 1, 2, 0]
    cfg, seqs = _sequences("tiny", (1, 11, 12, 13, 14), steps)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n)
    slots = list(range(n))
    later_keyframe, carried = False, 0
    for t in range(steps):
        batch.new_images(*_frame_set(n, {s: (seqs[s], t - starts[s]) for s in slots if t >= starts[s]}))
        later_keyframe = later_keyframe or any(batch.stats(s).is_keyframe and batch.stats(s).frame_id > 0 for s in slots)
        if t % 6 != 5:
            continue
        for what in (FRAMES, KEYFRAMES):
            for s in slots:
                f = batch.get_frame(s) if what == FRAMES else batch.get_keyframe(None, s)
                carried |= int(np.bitwise_or.reduce(VR.info_arrays(f.info)[0])) if len(f.info) else 0
            for level in (0, 2):
                gray = batch.export_views(what, level=level)
                for pixel in ("rgb8", "rgba8"):
                    v = batch.export_views(what, level=level, pixel=pixel, markers=True)
                    assert v.style.size == (20 if what == FRAMES else 10) and v.style.size_temporary == 10
                    assert v.style.drop_flags == (hip_lib.IGNORE_COMPLETELY if what == FRAMES else 0)
                    _check_marker_views((t, what, level, pixel), batch, what, slots, v, gray)
                    assert any(v.image(i)[:, :, :3].tobytes() != np.repeat(gray.image(i)[:, :, None], 3, 2).tobytes() for i in slots)
            # the app's style is not the only one: two flags dropped and one size only, and nothing dropped
            for drop, size, size_t in ((5, 64, 0), (0, 1, 33)):
                v = batch.export_views(what, pixel="rgb8", markers=True, drop_flags=drop, size=size, size_temporary=size_t)
                _check_marker_views((t, what, drop), batch, what, slots, v, batch.export_views(what))
    assert later_keyframe
    print("flags carried by the keypoints shown:", carried)
    assert carried == 7, carried
    batch.close()


def test_slot_states(monkeypatch):
    """slot 0 runs through; slot 1 never starts; slot 2 is restarted and stays empty for a step (NONE, run 1), then
    plays a new sequence; slot 3 sits step 2 out and shows its previous frame"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    cfg, seqs = _sequences("tiny", (1, 11, 12, 13), 5)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 4)
    slots = [0, 1, 2, 3]
    a, b, c, d = seqs

    def step(live):
        batch.new_images(*_frame_set(4, live))
        out = {}
        for what in (FRAMES, KEYFRAMES):
            gray = batch.export_views(what)
            v = batch.export_views(what, pixel="rgba8", markers=True)
            _check_marker_views(("states", what), batch, what, slots, v, gray)
            out[what] = (gray, v)
        return out

    step({0: (a, 0), 2: (b, 0), 3: (c, 0)})
    before = step({0: (a, 1), 2: (b, 1), 3: (c, 1)})
    batch.restart([2])
    now = step({0: (a, 2)})
    for what in (FRAMES, KEYFRAMES):
        seg = now[what][1].segments
        assert [int(x) for x in seg["status"]] == [0, 1, 1, 0]
        assert int(seg[2]["run"]) == 1 and int(seg[2]["frame_id"]) == -1 and int(seg[2]["n"]) == 0 and int(seg[1]["run"]) == 0
        assert now[what][1].image(1) is None and now[what][1].image(2) is None
        assert now[what][1].image(3).tobytes() == before[what][1].image(3).tobytes()
        # a NONE slot writes nothing but its segment: its image bytes keep what the buffer held
        v = now[what][1]
        v.pixels[:] = FILL
        v.submit().wait()
        for i in (1, 2):
            assert (v.pixels[i * v.image_bytes:(i + 1) * v.image_bytes] == FILL).all()
        assert v.image(0).tobytes() != bytes([FILL]) * (v.rows * v.pitch)
    assert now[FRAMES][0].image(0).tobytes() == a[0][2].cpu().numpy().tobytes()
    assert now[FRAMES][0].image(3).tobytes() == c[0][1].cpu().numpy().tobytes()
    after = step({0: (a, 3), 2: (d, 0), 3: (c, 2)})
    seg = after[FRAMES][1].segments
    assert [int(x) for x in seg["status"]] == [0, 1, 0, 0] and int(seg[2]["run"]) == 1 and int(seg[2]["frame_id"]) == 0
    assert after[FRAMES][0].image(2).tobytes() == d[0][0].cpu().numpy().tobytes()
    assert after[KEYFRAMES][0].image(2).tobytes() == d[0][0].cpu().numpy().tobytes()
    batch.close()


def _raw_submit(batch, what, seqs, n, style, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_views(batch._ctx, what, arr, n, C.byref(style) if style is not None else None,
                                                 C.byref(dst) if dst is not None else None, mem)


def test_named_slots_and_rejected_calls(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "3")
    n_slots = 9
    cfg, seqs = _sequences("tiny", (1, 11, 12), 3)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 3
    slots = list(range(n_slots))
    for t in range(2):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 3], t) for s in slots if s != 4}))
    for named in ([7, 0, 4, 8, 1], [5], [8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 4, 5, 0, 1, 2], []):
        for what in (FRAMES, KEYFRAMES):
            gray = batch.export_views(what, named, level=1)
            v = batch.export_views(what, named, level=1, pixel="rgb8", markers=True)
            _check_marker_views(("named", named, what), batch, what, named, v, gray)
            for i, s in enumerate(named):
                if s != 4:
                    src = seqs[s % 3][0][1 if what == FRAMES else 0].cpu().numpy()
                    assert gray.image(i).tobytes() == _half(src).tobytes(), (named, what, s)
                else:
                    assert gray.image(i) is None
    # rejected on the host: nothing queued, segments and pixels untouched
    good_style = hip_lib.view_style(FRAMES, "left", 0, "rgb8", True)
    _, _, _, image_bytes = batch.view_size(good_style)
    good = batch.export_views("frames", [0, 1], style=good_style)
    seg = np.zeros(n_slots, hip_lib.VIEW_SEGMENT_DTYPE)
    buf = np.zeros(n_slots * image_bytes + 8, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 4
    dst = hip_lib.ViewDst(seg.ctypes.data, base, 2 * image_bytes)
    H, D = hip_lib.MEM_HOST, hip_lib.MEM_DEVICE
    levels = cfg["max_pyramid_levels"]
    rejected = [
        (0, [0, 0], 2, good_style, dst, H), (0, [0, n_slots], 2, good_style, dst, H), (0, [-1, 1], 2, good_style, dst, H),
        (2, [0, 1], 2, good_style, dst, H), (-1, [0, 1], 2, good_style, dst, H),
        (0, [0, 1], 2, good_style, dst, 2), (0, [0, 1], 2, good_style, dst, 7),
        (0, [0, 1], 2, _style(plane=2), dst, H), (0, [0, 1], 2, _style(level=levels), dst, H), (0, [0, 1], 2, _style(level=-1), dst, H),
        (0, [0, 1], 2, _style(plane=1, level=1), dst, H), (0, [0, 1], 2, _style(pixel=3), dst, H),
        (0, [0, 1], 2, _style(size=65, pixel=1, markers=1), dst, H), (0, [0, 1], 2, _style(size_temporary=-1, pixel=1, markers=1), dst, H),
        (0, [0, 1], 2, _style(plane=1, pixel=1, markers=1), dst, H), (0, [0, 1], 2, _style(pixel=0, markers=1), dst, H),
        (0, [0, 1], 2, _style(pixel=1, markers=1, drop_flags=8), dst, H), (0, [0, 1], 2, _style(reserved=1), dst, H),
        (0, [0, 1], 2, None, dst, H), (0, [0, 1], 2, good_style, None, H),
        (0, [0, 1], 2, good_style, hip_lib.ViewDst(None, base, 2 * image_bytes), H),
        (0, [0, 1], 2, good_style, hip_lib.ViewDst(seg.ctypes.data, base + 2, 2 * image_bytes), H),
        (0, [0, 1], 2, good_style, hip_lib.ViewDst(seg.ctypes.data, base + 1, 2 * image_bytes), D),
    ]
    for args in rejected:
        assert _raw_submit(batch, *args) == -1, args[:3]
    dst.capacity = 2 * image_bytes - 1
    assert _raw_submit(batch, 0, [0, 1], 2, good_style, dst, H) == -4               # one byte below the bound
    assert b"capacity" in hip_lib.lib().svo_last_error()
    dst.capacity = n_slots * image_bytes - 1
    assert _raw_submit(batch, 0, None, 0, good_style, dst, H) == -4                 # every slot named
    assert not seg.view(np.uint8).any() and not buf.any()
    # at the bound it is accepted, and the ctx has kept working
    dst.capacity = 2 * image_bytes
    assert _raw_submit(batch, 0, [0, 1], 2, good_style, dst, H) == 0
    batch.wait()
    assert seg[:2].tobytes() == good.segments.tobytes()
    off = base - buf.ctypes.data
    assert buf[off:off + 2 * image_bytes].tobytes() == good.pixels[:2 * image_bytes].tobytes()
    assert not buf[off + 2 * image_bytes:].any()
    batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 3], 2) for s in slots}))
    v = batch.export_views("frames", pixel="rgba8", markers=True)
    _check_marker_views("after the errors", batch, FRAMES, slots, v, batch.export_views("frames"))
    batch.close()


def test_ordering_without_draining(monkeypatch):
    """frame set t, views A, frame set t+1, views B, one wait: A shows frame t and B frame t+1 (frame t's image set is
    recycled after t+1), markers as a twin ctx stopped at each shows them"""
    monkeypatch.setenv("SVO_GROUPS", "2")
    n_slots, t = 6, 3
    cfg, seqs = _sequences("tiny", (1, 11, 12), t + 2)
    sets = [_frame_set(n_slots, {s: (seqs[s % 3], k) for s in range(n_slots)}) for k in range(t + 2)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 2
    for k in range(t):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
    packed = [batch.pack_images(*sets[k]) for k in (t, t + 1)]

    def submit_all():
        return (batch.submit_views("frames"), batch.submit_views("frames", pixel="rgb8", markers=True, level=1),
                batch.submit_views("last_keyframes", pixel="rgba8", markers=True), batch.submit_views("frames", plane="right", device=True))

    batch.submit_packed(packed[0])
    a = submit_all()
    batch.submit_packed(packed[1])
    b = submit_all()
    batch.wait()
    for k, got in ((t, a), (t + 1, b)):
        twin.new_images(*sets[k])
        want = (twin.export_views("frames"), twin.export_views("frames", pixel="rgb8", markers=True, level=1),
                twin.export_views("last_keyframes", pixel="rgba8", markers=True), twin.export_views("frames", plane="right"))
        for s in range(n_slots):
            assert got[0].image(s).tobytes() == seqs[s % 3][0][k].cpu().numpy().tobytes(), (k, s)
            assert _np(got[3].image(s)).tobytes() == seqs[s % 3][1][k].cpu().numpy().tobytes(), (k, s)
            for g, w in zip(got[:3], want[:3]):
                assert g.image(s).tobytes() == w.image(s).tobytes(), (k, s)
        for g, w in zip(got, want):
            assert g.segments.tobytes() == w.segments.tobytes()
            assert [int(x) for x in g.segments["frame_id"]] == [k] * n_slots
        _check_marker_views(("twin", k), twin, FRAMES, list(range(n_slots)), want[1], twin.export_views("frames", level=1))
    batch.close()
    twin.close()


def test_device_mode_gives_the_same_bytes(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    n_slots = 6
    cfg, seqs = _sequences("tiny", (1, 11, 12), 3)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    for k in range(3):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s % 3], k) for s in range(n_slots) if s != 4}))
    for what in ("frames", "last_keyframes"):
        for named in (None, [5, 2, 4, 0]):
            for kw in (dict(level=2), dict(level=2, pixel="rgb8", markers=True), dict(pixel="rgba8", markers=True), dict(plane="right")):
                host = batch.submit_views(what, named, **kw)
                dev = batch.submit_views(what, named, device=True, **kw)
                batch.wait()
                host.pixels[:] = FILL
                dev.pixels.fill_(FILL)
                host.submit(), dev.submit()
                batch.wait()
                assert dev.pixels.is_cuda and host.segments.tobytes() == dev.segments.tobytes()
                # host and device mode write the same bytes, and nothing outside the images
                assert host.pixels.tobytes() == dev.pixels.cpu().numpy().tobytes(), (what, named, kw)
                inside = np.zeros(host.capacity, bool)
                for seg in host.segments:
                    if int(seg["status"]) == hip_lib.VIEW_OK:
                        inside[int(seg["offset"]):int(seg["offset"]) + host.rows * host.pitch] = True
                assert inside.any() and (named is None or not inside.all())
                assert (host.pixels[:host.capacity][~inside] == FILL).all(), (what, named, kw)
                assert [int(s["status"]) for s in host.segments] == [int(s != 4) ^ 1 for s in (named or range(n_slots))]
    batch.close()


def test_no_side_effects(monkeypatch):
    monkeypatch.setenv("SVO_GROUPS", "2")
    n_slots, steps = 6, 12
    cfg, seqs = _sequences("tiny", (1, 11, 12), steps)
    sets = [_frame_set(n_slots, {s: (seqs[s % 3], k) for s in range(n_slots)}) for k in range(steps)]
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    twin = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    fresh = twin.memory().device_bytes
    assert batch.memory().device_bytes == fresh
    batch.submit_views("frames", pixel="rgba8", markers=True, device=True).wait()          # device mode: no staging block
    assert batch.memory().device_bytes == fresh
    queued = []
    for k in range(steps):
        batch.submit_packed(batch.pack_images(*sets[k]))
        queued.append((batch.submit_views("frames", pixel="rgba8", markers=True), batch.submit_views("last_keyframes", level=1),
                       batch.submit_views("frames", pixel="rgb8", markers=True, device=True)))
        twin.new_images(*sets[k])
    batch.wait()
    grown = batch.memory().device_bytes - twin.memory().device_bytes
    assert 0 < grown <= n_slots * queued[0][0].image_bytes, grown           # (the largest image of the jobs: RGBA level 0)
    for s in range(n_slots):
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes() and len(batch.get_trajectory(s)) == steps
        assert batch.num_keyframes(s) == twin.num_keyframes(s)
        for f, g in ((batch.get_frame(s), twin.get_frame(s)), (batch.get_keyframe(None, s), twin.get_keyframe(None, s))):
            assert (f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes(), f.pose.tobytes()) == \
                   (g.kps2d.tobytes(), g.kps3d.tobytes(), g.info.tobytes(), g.pose.tobytes())
    slots = list(range(n_slots))
    _check_marker_views("last", twin, FRAMES, slots, queued[-1][0], twin.export_views("frames"))
    assert queued[-1][2].pixels.cpu().numpy().tobytes() == twin.export_views("frames", pixel="rgb8", markers=True).pixels.tobytes()
    batch.close()
    twin.close()


def test_euroc_level_4_rgb_in_three_groups(monkeypatch):
    """euroc, 66 slots in three groups, 4 frames, slots starting at steps 0, 1 and 2: LEFT level 4 RGB with markers,
    rows of 47 pixels (141 bytes: no row but the first is dword aligned)"""
    monkeypatch.setenv("SVO_GROUPS", "3")
    n_slots, steps = 66, 4
    cfg, seqs = _sequences("euroc", (3, 4, 5, 6), steps)
    batch = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    assert batch.groups() == 3
    slots = list(range(n_slots))
    for t in range(steps):
        batch.submit_packed(batch.pack_images(*_frame_set(n_slots, {s: (seqs[s % 4], t - s % 3) for s in slots if t >= s % 3})))
        if t == 0:
            first = batch.submit_views("frames", level=4, pixel="rgb8", markers=True)
    gray = batch.submit_views("frames", level=4)
    v = batch.submit_views("frames", level=4, pixel="rgb8", markers=True)
    kf = batch.submit_views("last_keyframes", level=4, pixel="rgb8", markers=True, device=True)
    batch.wait()
    assert (v.cols, v.rows, v.pitch, v.image_bytes) == (47, 30, 141, 4352)
    assert [int(x) for x in first.segments["status"]] == [int(s % 3 != 0) for s in slots]
    for s in slots:
        src = seqs[s % 4][0][steps - 1 - s % 3].cpu().numpy()
        assert gray.image(s).tobytes() == _chain(src, 5)[4].tobytes(), s
        _check_segment(("euroc", s), v.segments[s], batch, FRAMES, s)
        _check_segment(("euroc kf", s), kf.segments[s], batch, KEYFRAMES, s)
    some = [s for s in slots if s % 5 == 0 or s in (21, 22, 43, 44, 65)]
    for s in some:
        want, _ = _expected_markers(batch, FRAMES, s, v.style, gray.image(s))
        assert v.image(s).tobytes() == want.tobytes(), s
        assert want.tobytes() != VR.expand(gray.image(s), VR.RGB8).tobytes()
    host_kf = batch.export_views("last_keyframes", level=4, pixel="rgb8", markers=True)
    assert host_kf.pixels.tobytes() == kf.pixels.cpu().numpy().tobytes()
    batch.close()
