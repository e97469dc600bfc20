"""The scene on the GPU: the stage entry (svo_render_scene) on crafted points, lines and image shapes, and the ctx job
(svo_submit_export_scenes) against the restatement (tests/scene_ref.py) rendered from the getters. Every comparison
is on bytes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import map_ref as MR
import scene_ref as SR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import Handle
from stereo_svo_slam_amd.stereo_slam import Scenes, StereoSlamBatch

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xA5
INT_MIN = -2**31
PLANES = ("flags", "keyframe_id", "inlier_count", "color")


# ---------------------------------------------------------------------------------- stage entry, crafted

def _device_plane(values, offset, keep):
    """the 4-byte values in device memory at a base that is `offset` bytes past an allocation's start"""
    values = np.ascontiguousarray(values)
    raw = np.zeros(offset + values.nbytes + 16, np.uint8)
    raw[offset:offset + values.nbytes] = values.view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw).cuda()
    keep.append(t)
    return t.data_ptr() + offset


def _cam(c):
    return hip_lib.SceneCamera.from_buffer_copy(np.asarray(c, F).tobytes())


def _set(k3, color=None, flags=None, kf_id=None, inl=None, own_id=0):
    """a map_ref set of the points k3 [n, 3]"""
    k3 = np.asarray(k3, F).reshape(-1, 3)
    n = len(k3)
    z = np.zeros(n, np.uint32)
    planes = {"flags": z if flags is None else np.asarray(flags, np.uint32),
              "keyframe_id": z if kf_id is None else np.asarray(kf_id, np.int32).view(np.uint32),
              "inlier_count": z if inl is None else np.asarray(inl, np.int32).view(np.uint32),
              "color": ((np.arange(n, dtype=np.uint64) * 2654435761 >> 8) & 0xffffffff).astype(np.uint32) if color is None else np.asarray(color, np.uint32)}
    return (n, own_id, k3, planes)


def _call(h, images, style, filt=MR.KEEP_ALL, order=None, gap=36):
    """one svo_render_scene of images [(cols, rows, camera float32 [16], sets, lines)] in the given order, into a
    buffer pre-filled with FILL whose base is 4-byte but not 16-byte aligned, with gaps between the images; the whole
    buffer is compared with the restatement"""
    order = list(range(len(images))) if order is None else order
    bpp = SR.BYTES[style.pixel]
    keep, srcs, cams, offsets = [], [], [], []
    at = 8
    for i in order:
        cols, rows, cam, sets, lines = images[i]
        dev_sets = []
        for j, (n, own_id, k3, planes) in enumerate(sets):
            fields = {"kps3d": _device_plane(np.ascontiguousarray(k3).view(np.uint32), 12 if j % 2 else 4, keep)}
            for t, name in enumerate(PLANES):
                fields[name] = _device_plane(planes[name], 4 if (t + j) % 2 else 12, keep)
            dev_sets.append((n, own_id, fields))
        rec = np.zeros(len(lines), hip_lib.SCENE_LINE_DTYPE)
        for j, (a, b, low) in enumerate(lines):
            rec[j] = (a, b, low, 0)
        dev_lines = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda() if len(lines) else None
        keep.append(dev_lines)
        srcs.append((cols, rows, dev_sets, dev_lines))
        cams.append(_cam(cam))
        offsets.append(at)
        at += (cols * rows * bpp + gap + 3) // 4 * 4
    total = at + 8
    buf = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 4
    assert base % 16 == 4
    h.render_scene(srcs, cams, offsets, style, base)
    got = buf.cpu().numpy()
    want = np.full(total + 16, FILL, np.uint8)
    for i, off in zip(order, offsets):
        cols, rows, cam, sets, lines = images[i]
        img = _reference(images[i], style, filt)
        want[4 + off:4 + off + img.size] = img.reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[:5]} (offsets {offsets})"
    return [want[4 + off:4 + off + images[i][0] * images[i][1] * bpp].reshape(images[i][1], images[i][0], bpp) for i, off in zip(order, offsets)]


_REF = {}


def _reference(image, style, filt):
    """SR.render of an image, computed once per (image, point size, filter, background); RGBA adds the fourth byte"""
    cols, rows, cam, sets, lines = image
    key = (id(image), style.point_size, style.background, tuple(sorted(filt.items())))
    if key not in _REF:
        _REF[key] = (image, SR.render(cols, rows, SR.RGB8, np.asarray(cam, F), sets, lines, filt, style.point_size, style.background))
    rgb = _REF[key][1]
    if style.pixel == SR.RGB8:
        return rgb
    return np.concatenate([rgb, np.full((rows, cols, 1), 255, np.uint8)], axis=2)


def _style(pixel=SR.RGB8, point_size=1, background=0xffffff, filt=MR.KEEP_ALL):
    return hip_lib.scene_style(cols=1, rows=1, pixel=pixel, point_size=point_size, background=background, filter=dict(filt))


@pytest.fixture(scope="module")
def handle():
    h = Handle(0, 1024)
    yield h
    h.close()


WIDTHS, HEIGHTS = (1, 3, 4, 5, 63, 64, 65, 67, 257), (1, 2, 16, 17)


@pytest.fixture(scope="module")
def shapes():
    """an image per width and height: the same cloud and lines through a camera that fits the image"""
    rng = np.random.default_rng(21)
    n = 90
    z = rng.choice(F([1.0, 1.5, 2.0, 3.0]), n)
    k3 = np.stack([rng.uniform(-1.2, 1.2, n).astype(F) * z, rng.uniform(-1.2, 1.2, n).astype(F) * z, z], 1)
    sets = [_set(k3[:40], own_id=0), _set(k3[40:], own_id=1)]
    ends = np.stack([rng.uniform(-1.3, 1.3, (14, 2)), rng.uniform(-1.3, 1.3, (14, 2)), rng.uniform(0.2, 3, (14, 2))], 2).astype(F)
    lines = [(e[0], e[1], int(rng.integers(0, 3)) << 24 | int(rng.integers(0, 2**24))) for e in ends]
    out = []
    for w in WIDTHS:
        for hgt in HEIGHTS:
            cam = SR.camera(np.eye(3, 4), max(w, hgt) / 2, w / 2, hgt / 2, 0.5)
            out.append((w, hgt, cam, sets, lines))
    return out


@pytest.mark.parametrize("pixel", [SR.RGB8, SR.RGBA8])
def test_image_shapes_in_one_call(handle, shapes, pixel, monkeypatch):
    """every width x height in one call, in two orders (the second through a tile table of 3 tiles: chunked launches),
    at a base that is not 16-byte aligned, gaps between the images untouched"""
    st = _style(pixel, point_size=5)
    imgs = _call(handle, shapes, st)
    big = imgs[-1]
    assert (big[:, :, :3] != 255).any() and (big[:, :, :3] == 255).all(axis=2).any()
    monkeypatch.setenv("SVO_SCENE_TABLE_TILES", "3")
    _call(handle, shapes, st, order=list(np.random.default_rng(2).permutation(len(shapes))), gap=4)


def _at(u, v, z, cam):
    """the world point that an identity-view camera projects to (u, v) at depth z (f is a power of two: exact)"""
    f, cx, cy = cam[12], cam[13], cam[14]
    return F([(F(u) - cx) / f * F(z), (F(v) - cy) / f * F(z), z])


@pytest.fixture(scope="module")
def point_image():
    """70 x 20 (two tiles a side): sets of 0, 1, 63, 64, 65 and 300 keypoints, and a set of crafted ones"""
    rng = np.random.default_rng(22)
    cols, rows = 70, 20
    cam = SR.camera(np.eye(3, 4), 8.0, 32.0, 8.0, 0.5)
    sets = []
    for j, n in enumerate((0, 1, 63, 64, 65, 300)):
        z = rng.choice(F([0.5, 1.0, 2.0, 4.0]), n)
        k3 = np.array([_at(rng.uniform(-10, 80), rng.uniform(-10, 30), zz, cam) for zz in z], F).reshape(-1, 3)
        sets.append(_set(k3, color=rng.integers(0, 2**32, n), flags=rng.integers(0, 8, n), kf_id=rng.integers(0, 7, n),
                         inl=rng.integers(-3, 12, n), own_id=j))
    near, below = F(0.5), np.nextafter(F(0.5), F(0))
    big = F(32768) - F(1 / 256)
    crafted = [_at(10, 3, 1.0, cam), _at(11.0, 5.0, 2.0, cam),                     # u, v exactly integers
               _at(20, 10, near, cam), _at(24, 10, below, cam),                    # depth exactly near; just below it
               F([np.nan, 0, 1]), F([0, np.inf, 1]), F([0, 0, -np.inf]), F([1e30, 0, 1]), F([0, 1e30, 1e30]), F([0, 0, 1e30]),
               _at(big, 5, 1.0, cam), _at(-big, 5, 1.0, cam), _at(5, big, 1.0, cam), _at(5, -big, 1.0, cam),   # just below 2^15
               _at(32768, 5, 1.0, cam), _at(-32768, 5, 1.0, cam), _at(5, 32768, 1.0, cam), _at(5, -32768, 1.0, cam),   # at 2^15
               _at(63.5, 15.5, 1.0, cam), _at(64.0, 16.0, 1.5, cam), _at(0, 0, 1.0, cam), _at(69.9, 19.9, 1.0, cam),   # tile and image borders
               _at(-7.5, 8, 1.0, cam), _at(77, 8, 1.0, cam), _at(30, -7.2, 1.0, cam), _at(30, 27, 1.0, cam)]   # outside, reaching in at size 16
    sets.append(_set(crafted, color=rng.integers(0, 2**24, len(crafted)), own_id=6))
    # 300 coincident points of different colours at one depth (the smallest colour word wins), and some nearer and
    # farther ones on the same pixel
    same = np.tile(_at(40.3, 12.6, 2.0, cam), (300, 1))
    colors = rng.permutation(np.arange(5000, 5300)).astype(np.uint32)
    colors = (colors & 0xff) << 16 | (colors & 0xff00) | (colors >> 16)             # (the plane holds b << 16 | g << 8 | r)
    sets.append(_set(same, color=colors, own_id=7))
    sets.append(_set([_at(40.3, 12.6, 4.0, cam), _at(50.5, 3.5, 1.0, cam), _at(50.5, 3.5, np.nextafter(F(1.0), F(0)), cam)],
                     color=[0x000001, 0x0000ff, 0x00ff00], own_id=8))
    return (cols, rows, cam, sets, [])


@pytest.mark.parametrize("size", [1, 4, 5, 16])
def test_points(handle, point_image, size):
    img = _call(handle, [point_image], _style(SR.RGBA8, size, 0x203040))[0]
    cols, rows, cam, sets, _ = point_image
    assert tuple(img[10, 20, :3]) != (0x20, 0x30, 0x40), "the point at depth == near is drawn"
    if size == 1:
        assert tuple(img[10, 24, :3]) == (0x20, 0x30, 0x40), "the point just below near is not"
        assert tuple(img[12, 40, :3]) == ((5000 >> 16) & 0xff, (5000 >> 8) & 0xff, 5000 & 0xff), "the smallest colour word of the 300"
        assert tuple(img[3, 50, :3]) == (0, 0xff, 0), "the nearer of two points on a pixel"


def test_point_filters(handle, point_image):
    for filt in (dict(drop_flags=MR.IGNORE_COMPLETELY | MR.IGNORE_TEMPORARY, own_only=0, min_inliers=INT_MIN),
                 dict(drop_flags=0, own_only=1, min_inliers=INT_MIN), dict(drop_flags=0, own_only=0, min_inliers=8),
                 dict(drop_flags=MR.IGNORE_DURING_REFINEMENT, own_only=1, min_inliers=2)):
        a = _call(handle, [point_image], _style(SR.RGB8, 4, 0xffffff, filt), filt)[0]
        b = _reference(point_image, _style(SR.RGB8, 4), MR.KEEP_ALL)
        assert a.tobytes() != b.tobytes(), filt                                    # the filter drops something visible


@pytest.fixture(scope="module")
def line_image():
    """200 x 40 (4 x 3 tiles)"""
    cols, rows = 200, 40
    cam = SR.camera(np.eye(3, 4), 16.0, 100.0, 20.0, 0.5)
    rgb = iter(range(0x010203, 0xffffff, 0x070b0d))
    P = lambda u, v, z: _at(u + 0.5, v + 0.5, z, cam)
    L = lambda a, b, cls=2: (P(*a), P(*b), cls << 24 | next(rgb))
    lines = [L((5, 3, 1), (40, 3, 1)), L((40, 5, 1), (5, 5, 1)),                   # horizontal, both directions
             L((8, 8, 1), (8, 30, 1)), L((10, 30, 1), (10, 8, 1)),                 # vertical
             L((20, 8, 1), (40, 28, 1)), L((60, 28, 1), (40, 8, 1)), L((20, 28, 1), (40, 8, 1)), L((60, 8, 1), (40, 28, 1)),   # both diagonals
             L((70, 2, 1), (76, 37, 1)), L((82, 37, 1), (78, 2, 1)), L((70, 37, 1), (64, 2, 1)),   # steep
             L((90, 10, 1), (190, 17, 1)), L((190, 25, 1), (90, 21, 1)), L((90, 30, 1), (190, 24, 1)),   # shallow
             L((50, 35, 1), (50, 35, 1)), L((63, 15, 1), (63, 15, 1)), L((64, 16, 1), (64, 16, 1)),   # zero length, at tile corners
             L((-3, -2, 1), (203, 42, 1), 1), L((199, 0, 2), (0, 39, 3), 0),       # corner to corner: a dozen tiles
             L((120, 5, 2), (30000, 900, 2)), L((-30000, -20000, 2), (130, 35, 2)), L((150, -32000, 1), (150, 32000, 1)),   # ends far outside
             L((100, 2, 3), (180, 38, 3), 1), L((100, 38, 2), (180, 2, 2), 1)]     # two crossing at different depths
    A = lambda x, y, z: F([x, y, z])
    lines += [(A(-2, -0.5, -1.0), A(1, 0.5, 2.0), 2 << 24 | 0x00aa00),            # crossing near from the a end
              (A(2, -0.5, 2.0), A(-1, 0.8, -0.25), 2 << 24 | 0x00bb00),           # from the b end
              (A(0, 0, 0.25), A(1, 1, -3.0), 2 << 24 | 0x00cc00),                 # both ends behind
              (A(0, 0, 0.5), A(0.5, 0.25, 0.5), 0 << 24 | 0x00dd00),              # both ends exactly at near
              (A(np.nan, 0, 1), A(1, 1, 1), 2 << 24 | 0x00ee00), (A(0, 0, 1), A(np.inf, 1, 1), 2 << 24 | 0x00ef00),
              (A(1e30, 0, 1), A(0, 0, 1), 2 << 24 | 0x00f000), (A(0, 0, 0.1), A(1e30, 1e30, 1e30), 2 << 24 | 0x00f100)]
    # a line from depth 1 to depth 3 and points of size 3 along it at depth 2: in front of its far half, behind its
    # near half; a line at depth exactly 2 through points at depth exactly 2: the line wins
    lines += [(P(20, 36, 1), P(180, 36, 3), 2 << 24 | 0x808080), (P(20, 33, 2), P(180, 33, 2), 2 << 24 | 0x404040)]
    pts = [P(u, 36, 2) for u in range(25, 180, 10)] + [P(u, 33, 2) for u in range(25, 180, 10)]
    sets = [_set(pts, color=[0x0000ff] * len(pts))]
    return (cols, rows, cam, sets, lines)


@pytest.mark.parametrize("pixel", [SR.RGB8, SR.RGBA8])
def test_lines(handle, line_image, pixel):
    img = _call(handle, [line_image], _style(pixel, 3, 0xffffff))[0]
    assert tuple(img[33, 25, :3]) == (0x40, 0x40, 0x40) and tuple(img[32, 25, :3]) == (0xff, 0, 0), "a line beats a point at equal depth"
    assert tuple(img[36, 35, :3]) == (0x80, 0x80, 0x80) and tuple(img[36, 165, :3]) == (0xff, 0, 0), "a point behind / in front of the line"
    assert tuple(img[3, 20, :3]) != (255, 255, 255) and tuple(img[39, 0, :3]) != (255, 255, 255) and tuple(img[0, 199, :3]) != (255, 255, 255)


def test_cameras_per_image_and_an_empty_image(handle, monkeypatch):
    rng = np.random.default_rng(23)
    n = 200
    k3 = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    sets = [_set(k3[:120], own_id=0), _set(k3[120:], own_id=1)]
    lines = SR.line_records(SR.frustum([0.2, 0.1, -0.3, 0.3, -0.2, 0.1], (0.4, 0.3, 0.5)), 0, 0x00ff00) + \
        SR.line_records(SR.frustum([-0.5, 0.3, 0.2, 3.0, 0.1, -0.4], (0.4, 0.3, 0.5)), 1, 0x0000ff) + \
        SR.line_records([np.concatenate([k3[i], k3[i + 1]]) for i in range(0, 24)], 2, 0xff0000)
    cols, rows = 96, 48
    images = []
    for name in ("front", "top", "side"):
        c = hip_lib.scene_preset(name, cols, rows)
        images.append((cols, rows, np.frombuffer(bytes(c), F).copy(), sets, lines))
    c = hip_lib.scene_look_at((2.5, -1.5, -2.0), (0.1, 0.2, 0.0), (0.1, -1.0, 0.2), 70.0, cols, rows, 0.3)
    images.append((cols, rows, np.frombuffer(bytes(c), F).copy(), sets, lines))
    images.insert(2, (33, 18, images[0][2], [], []))                              # no element at all
    images.append((40, 17, images[1][2], [_set(np.zeros((0, 3)))], lines[:3]))
    out = _call(handle, images, _style(SR.RGB8, 2))
    assert (out[2] == 255).all()
    assert len({o.tobytes() for o in out[:2] + out[3:5]}) == 4                     # four cameras, four pictures
    monkeypatch.setenv("SVO_SCENE_TABLE_TILES", "1")
    _call(handle, images, _style(SR.RGBA8, 2, 0x000000), order=[5, 4, 3, 2, 1, 0])


def test_stage_entry_rejects(handle):
    lib = hip_lib.lib()
    st = _style()
    cam = _cam(SR.camera(np.eye(3, 4), 8.0, 4.0, 4.0, 0.5))
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    lines = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ok = lambda: ([(8, 8, [], lines)], [cam], [0], st, buf)
    handle.render_scene(*ok())
    assert (buf[:192] == 255).all() and (buf[192:] == FILL).all()

    def rejected(srcs=None, cams=None, offsets=None, style=None, pixels=None):
        a = list(ok())
        for i, v in enumerate((srcs, cams, offsets, style, pixels)):
            if v is not None:
                a[i] = v
        with pytest.raises(hip_lib.SvoError):
            handle.render_scene(*a)

    rejected(srcs=[(0, 8, [], None)]); rejected(srcs=[(8, 4097, [], None)]); rejected(offsets=[2]); rejected(offsets=[-4])
    rejected(pixels=buf.data_ptr() + 2); rejected(srcs=[(8, 8, [], lines[4:])])
    rejected(srcs=[(8, 8, [(1, 0, {"kps3d": buf.data_ptr() + 2, "flags": buf, "keyframe_id": buf, "inlier_count": buf, "color": buf})], None)])
    rejected(srcs=[(8, 8, [(-1, 0, {})], None)]); rejected(srcs=[(8, 8, [(1, 0, {})], None)])
    for field, v in (("f", 0.0), ("f", float("nan")), ("near", 0.0), ("near", -1.0), ("cx", float("inf"))):
        bad = _cam(SR.camera(np.eye(3, 4), 8.0, 4.0, 4.0, 0.5))
        setattr(bad, field, v)
        rejected(cams=[bad])
    bad = _cam(SR.camera(np.eye(3, 4), 8.0, 4.0, 4.0, 0.5))
    bad.view[7] = float("nan")
    rejected(cams=[bad])
    rejected(style=hip_lib.scene_style(pixel=0)); rejected(style=hip_lib.scene_style(point_size=17))
    assert lib.svo_render_scene(handle._h, 1, None, None, None, C.byref(st), C.c_void_p(buf.data_ptr())) == -1
    assert lib.svo_render_scene(handle._h, 0, None, None, None, None, C.c_void_p(buf.data_ptr())) == -1
    assert (buf[192:] == FILL).all()
    handle.render_scene(*ok())                                                     # still usable


# ---------------------------------------------------------------------------------- the ctx against its getters

COLS, ROWS = 96, 40


def _sequences(config, seeds, n_frames, motion_scale=4.0):
    """[(lefts [n, H, W], rights, time stamps)] rendered on the GPU, and the config"""
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


@pytest.fixture(scope="module")
def tiny():
    """tiny, seeds (1, 11, 12, 13, 14), 24 frames of fast motion (the recipe of test_map_gpu.py): shared, never changed"""
    return _sequences("tiny", (1, 11, 12, 13, 14), 24)


def _batch(cfg, n_slots, groups):
    old = os.environ.get("SVO_GROUPS")
    os.environ["SVO_GROUPS"] = str(groups)
    try:
        b = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    finally:
        if old is None:
            del os.environ["SVO_GROUPS"]
        else:
            os.environ["SVO_GROUPS"] = old
    assert b.groups() == groups
    return b


@pytest.fixture(scope="module")
def played(tiny):
    """5 slots in 2 groups after 24 frames; the tests only read it"""
    cfg, seqs = tiny
    batch = _batch(cfg, 5, 2)
    for t in range(24):
        batch.new_images(*_frame_set(5, {s: (seqs[s], t) for s in range(5)}))
    yield batch
    batch.close()


def _getter_sets(batch, s, from_kf=0):
    """the keyframes of slot s from from_kf on as the getters return them: map_ref sets and their poses"""
    sets, poses = [], []
    for k in range(from_kf, batch.num_keyframes(s)):
        f = batch.get_keyframe(k, s)
        info = f.info
        flags = (info["ignore_during_refinement"].astype(np.uint32) * MR.IGNORE_DURING_REFINEMENT |
                 info["ignore_completely"].astype(np.uint32) * MR.IGNORE_COMPLETELY |
                 info["ignore_temporary"].astype(np.uint32) * MR.IGNORE_TEMPORARY)
        col = info["color"].astype(np.uint32).reshape(-1, 3)
        planes = {"flags": flags, "keyframe_id": np.ascontiguousarray(info["keyframe_id"]).view(np.uint32),
                  "inlier_count": np.ascontiguousarray(info["inlier_count"]).view(np.uint32),
                  "color": col[:, 0] | col[:, 1] << 8 | col[:, 2] << 16}
        sets.append((len(info), k, np.ascontiguousarray(f.kps3d), planes))
        poses.append(f.pose)
    return sets, poses


def _restate(source, s, style, cam):
    """(image, keypoints considered, poses drawn) of slot s of `source` through the getters and the restatement"""
    sets, poses = _getter_sets(source, s, style.from_keyframe)
    filt = dict(drop_flags=style.filter.drop_flags, own_only=style.filter.own_only, min_inliers=style.filter.min_inliers)
    lines, n_poses = SR.slot_lines(source.get_trajectory(s), poses, source.pose(s), style.show, style.trajectory_rgb, style.keyframe_rgb,
                                   style.pose_rgb, (style.frustum_w, style.frustum_h, style.frustum_d), style.trajectory_tail)
    if not style.show & SR.POINTS:
        sets = []
    img = SR.render(style.cols, style.rows, style.pixel, np.frombuffer(bytes(cam), F), sets, lines, filt, style.point_size, style.background)
    return img, sum(n for n, *_ in sets), n_poses


def _check_slot(tag, sc, i, s, source, cam, run=0):
    """named slot i of the job (slot s) against the getters of `source`"""
    seg = sc.segments[i]
    want, n_kps, n_poses = _restate(source, s, sc.style, cam)
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, run, hip_lib.SCENE_OK), (tag, s)
    assert int(seg["frame_id"]) == source.stats(s).frame_id and int(seg["n_keyframes"]) == source.num_keyframes(s), (tag, s)
    assert (int(seg["from_keyframe"]), int(seg["n_keypoints"]), int(seg["n_poses"])) == (sc.style.from_keyframe, n_kps, n_poses), (tag, s)
    assert int(seg["offset"]) == i * sc.image_bytes and seg["pose"].tobytes() == source.pose(s).tobytes(), (tag, s)
    got = sc.image(i)
    got = got.cpu().numpy() if sc.device_mode else got
    assert got.tobytes() == want.tobytes(), (tag, s, int((got != want).sum()))
    return want


def _has_colour(img, rgb):
    return bool((img[:, :, :3] == np.array([(rgb >> 16) & 0xff, (rgb >> 8) & 0xff, rgb & 0xff], np.uint8)).all(axis=2).any())


def _cams(names):
    return [hip_lib.scene_preset(n, COLS, ROWS) for n in names]


def test_ctx_against_the_getters(played):
    """5 slots in 2 groups, a camera per slot, host and device mode, RGB and RGBA; a picture shows points, every line
    class and background"""
    cams = _cams(("front", "top", "side", "front", "top"))
    assert max(played.num_keyframes(s) for s in range(5)) >= 2
    for pixel, device in ((SR.RGB8, False), (SR.RGBA8, True)):
        sc = played.export_scenes(camera=cams, device=device, cols=COLS, rows=ROWS, pixel=pixel, point_size=3)
        imgs = [_check_slot("all", sc, s, s, played, cams[s]) for s in range(5)]
        assert sc.pixels.shape[0] == 5 * sc.image_bytes and (sc.pitch, sc.image_bytes) == SR.size(COLS, ROWS, pixel)
        # some picture shows background, a line class and points (a colour that is neither)
        lines_rgb = (0xff0000, 0x0000ff, 0x00ff00)
        shows = []
        for img in imgs:
            word = img[:, :, 0].astype(np.uint32) << 16 | img[:, :, 1].astype(np.uint32) << 8 | img[:, :, 2]
            shows.append(_has_colour(img, 0xffffff) and any(_has_colour(img, c) for c in lines_rgb) and
                         bool((~np.isin(word, (0xffffff,) + lines_rgb)).any()))
        assert any(shows), shows
    points_only = played.export_scenes([0], camera=cams[0], cols=COLS, rows=ROWS, show=SR.POINTS, point_size=3)
    img = _check_slot("points", points_only, 0, 0, played, cams[0])
    assert int(points_only.segments[0]["n_poses"]) == 0 and (img != 255).any()


def test_host_and_device_mode_and_a_chunked_table_give_the_same_bytes(played, monkeypatch):
    cams = _cams(("side", "front", "top"))
    named = [4, 0, 2]
    host = played.export_scenes(named, camera=cams, cols=130, rows=33, pixel="rgba8", point_size=4)
    for i, s in enumerate(named):
        _check_slot("host", host, i, s, played, cams[i])
    dev = Scenes(played, named, host.style, cams, True)
    dev.pixels.fill_(FILL)
    dev.submit().wait()
    assert dev.pixels.is_cuda and host.segments.tobytes() == dev.segments.tobytes()
    assert dev.pixels.cpu().numpy()[:host.capacity].reshape(3, -1)[:, :33 * host.pitch].tobytes() == \
        host.pixels[:host.capacity].reshape(3, -1)[:, :33 * host.pitch].tobytes()
    assert (dev.pixels.cpu().numpy()[:host.capacity].reshape(3, -1)[:, 33 * host.pitch:] == FILL).all()   # exactly rows * pitch bytes a slot
    monkeypatch.setenv("SVO_SCENE_TABLE_TILES", "2")                             # 3 x 3 tiles an image: chunks in both groups
    for device in (False, True):
        again = played.export_scenes(named, camera=cams, device=device, style=host.style)
        px = again.pixels.cpu().numpy() if device else again.pixels
        assert px[:host.capacity].tobytes() == host.pixels[:host.capacity].tobytes() and again.segments.tobytes() == host.segments.tobytes()


def test_named_slots_from_keyframe_and_tail(played):
    counts = [played.num_keyframes(s) for s in range(5)]
    front = hip_lib.scene_preset("front", COLS, ROWS)
    for named in ([3], [4, 1, 0], [2, 3]):
        for from_kf, tail in ((0, 0), (1, 5), (max(counts), 1), (max(counts) + 3, 1000), (0, 2)):
            sc = Scenes(played, named, hip_lib.scene_style(cols=COLS, rows=ROWS, point_size=2, from_keyframe=from_kf, trajectory_tail=tail),
                        front, False)
            sc.pixels[:] = FILL
            sc.submit().wait()
            for i, s in enumerate(named):
                _check_slot((named, from_kf, tail), sc, i, s, played, front)
                assert int(sc.segments[i]["n_poses"]) == (min(tail, 24) if tail else 24)
            tailing = sc.pixels[:sc.capacity].reshape(len(named), -1)[:, ROWS * sc.pitch:]
            assert (tailing == FILL).all()
    whole = played.export_scenes([0], camera=front, cols=COLS, rows=ROWS)
    part = played.export_scenes([0], camera=front, cols=COLS, rows=ROWS, from_keyframe=1, trajectory_tail=3)
    assert whole.image(0).tobytes() != part.image(0).tobytes()


def test_an_empty_slot_and_a_restarted_one(tiny):
    cfg, seqs = tiny
    batch = _batch(cfg, 4, 2)
    front = hip_lib.scene_preset("front", COLS, ROWS)
    for t in range(8):                                                               # slot 1 never starts
        batch.new_images(*_frame_set(4, {s: (seqs[s], t) for s in (0, 2, 3)}))
    batch.restart([2, 3])
    for t in range(3):                                                               # slot 3 plays another sequence, slot 2 stays empty
        batch.new_images(*_frame_set(4, {0: (seqs[0], 8 + t), 3: (seqs[4], t)}))
    sc = Scenes(batch, None, hip_lib.scene_style(cols=COLS, rows=ROWS, point_size=2), front, False)
    sc.pixels[:] = FILL
    sc.submit().wait()
    _check_slot("runs on", sc, 0, 0, batch, front)
    _check_slot("restarted", sc, 3, 3, batch, front, run=1)
    assert int(sc.segments[3]["frame_id"]) == 2 and int(sc.segments[3]["n_poses"]) == 3
    for s, run in ((1, 0), (2, 1)):
        seg = sc.segments[s]
        assert (int(seg["seq"]), int(seg["run"]), int(seg["frame_id"]), int(seg["status"])) == (s, run, -1, hip_lib.SCENE_NONE)
        assert (int(seg["n_keyframes"]), int(seg["n_keypoints"]), int(seg["n_poses"]), int(seg["offset"])) == (0, 0, 0, s * sc.image_bytes)
        assert sc.image(s) is None
        assert (sc.pixels[s * sc.image_bytes:(s + 1) * sc.image_bytes] == FILL).all()   # only its segment is written
    batch.close()


def test_ordering_without_draining(tiny):
    """frame set t, scene A, frame set t + 1, scene B, one wait: A shows the state at t, B at t + 1 (a twin ctx stopped
    at each)"""
    cfg, seqs = tiny
    n_slots, t = 5, 9
    sets = [_frame_set(n_slots, {s: (seqs[s], k) for s in range(n_slots)}) for k in range(t + 2)]
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(t):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
    front = hip_lib.scene_preset("front", COLS, ROWS)
    packed = [batch.pack_images(*sets[k]) for k in (t, t + 1)]
    batch.submit_packed(packed[0])
    a = batch.submit_scenes(camera=front, cols=COLS, rows=ROWS, point_size=2)
    batch.submit_packed(packed[1])
    b = batch.submit_scenes(camera=front, cols=COLS, rows=ROWS, point_size=2, device=True)
    batch.wait()
    for sc, k in ((a, t), (b, t + 1)):
        twin.new_images(*sets[k])
        assert [int(x) for x in sc.segments["frame_id"]] == [k] * n_slots
        for s in range(n_slots):
            _check_slot(f"frame {k}", sc, s, s, twin, front)
    assert any(a.image(s).tobytes() != b.image(s).cpu().numpy().tobytes() for s in range(n_slots))
    batch.close()
    twin.close()


def _raw_submit(batch, seqs, n, style, cams, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_scenes(batch._ctx, arr, n, None if style is None else C.byref(style), cams,
                                                  None if dst is None else C.byref(dst), mem)


def test_rejected_calls_queue_nothing(tiny):
    cfg, seqs = tiny
    n_slots = 4
    batch = _batch(cfg, n_slots, 2)
    for t in range(2):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s], t) for s in range(n_slots)}))
    st = hip_lib.scene_style(cols=COLS, rows=ROWS)
    _, image_bytes = hip_lib.scene_size(st)
    seg = np.zeros(n_slots, hip_lib.SCENE_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = FILL
    px = torch.full((n_slots * image_bytes + 16,), FILL, dtype=torch.uint8).pin_memory()
    dpx = torch.full((n_slots * image_bytes + 16,), FILL, dtype=torch.uint8, device="cuda")
    front = hip_lib.scene_preset("front", COLS, ROWS)
    cams = (hip_lib.SceneCamera * n_slots)(*[front] * n_slots)
    dst = lambda p=px.data_ptr(), cap=n_slots * image_bytes, s=seg.ctypes.data: hip_lib.SceneDst(s, p, cap)
    INVALID, CAPACITY = -1, hip_lib.lib().svo_submit_export_scenes(batch._ctx, None, 0, C.byref(st), cams, C.byref(dst(cap=n_slots * image_bytes - 1)), 0)
    assert CAPACITY not in (0, INVALID)
    bad_cam = (hip_lib.SceneCamera * n_slots)(*[front] * n_slots)
    bad_cam[2].near = 0.0
    nan_cam = (hip_lib.SceneCamera * n_slots)(*[front] * n_slots)
    nan_cam[3].view[5] = float("nan")
    gray = hip_lib.scene_style(cols=COLS, rows=ROWS)
    gray.pixel = 0
    reserved = hip_lib.scene_style(cols=COLS, rows=ROWS)
    reserved._reserved = 1
    calls = [([4], 1, st, cams, dst(), 0), ([-1], 1, st, cams, dst(), 0), ([0, 1, 0], 3, st, cams, dst(), 0), ([0], -1, st, cams, dst(), 0),
             (None, 0, st, cams, dst(), 2), (None, 0, st, cams, dst(), -1), (None, 0, None, cams, dst(), 0), (None, 0, st, None, dst(), 0),
             (None, 0, st, cams, None, 0), (None, 0, st, cams, dst(s=None), 0), (None, 0, st, cams, dst(p=None), 0),
             (None, 0, st, cams, dst(p=px.data_ptr() + 2), 0), (None, 0, st, cams, dst(p=dpx.data_ptr() + 1), 1),
             (None, 0, st, bad_cam, dst(), 0), (None, 0, st, nan_cam, dst(), 0), (None, 0, gray, cams, dst(), 0),
             (None, 0, reserved, cams, dst(), 0), (None, 0, hip_lib.scene_style(cols=0), cams, dst(), 0),
             (None, 0, hip_lib.scene_style(cols=COLS, rows=ROWS, show=16), cams, dst(), 0),
             (None, 0, hip_lib.scene_style(cols=COLS, rows=ROWS, filter=dict(drop_flags=8)), cams, dst(), 0)]
    for c in calls:
        assert _raw_submit(batch, *c) == INVALID, c[:2]
        assert hip_lib.lib().svo_last_error()
    assert _raw_submit(batch, [1, 2], 2, st, cams, dst(cap=2 * image_bytes - 1), 0) == CAPACITY
    assert _raw_submit(batch, [0, 2], 2, st, bad_cam, dst(), 0) == 0                # (the bad camera belongs to no named slot)
    batch.wait()
    assert (seg.view(np.uint8).reshape(n_slots, -1)[2:] == FILL).all() and (px.numpy()[2 * image_bytes:] == FILL).all() and (dpx == FILL).all()
    seg.view(np.uint8)[:] = FILL
    # nothing was queued and the ctx goes on: the next frame and a scene of it
    batch.new_images(*_frame_set(n_slots, {s: (seqs[s], 2) for s in range(n_slots)}))
    sc = batch.export_scenes(camera=front, cols=COLS, rows=ROWS)
    assert [int(x) for x in sc.segments["frame_id"]] == [2] * n_slots
    _check_slot("after", sc, 1, 1, batch, front)
    batch.close()


def test_no_side_effects(tiny):
    """getters and the next frames are the same bits with and without scene jobs in between; a ctx that never asks
    allocates nothing more, one that does counts what it allocates"""
    cfg, seqs = tiny
    n_slots, steps = 4, 10
    sets = [_frame_set(n_slots, {s: (seqs[s], k) for s in range(n_slots)}) for k in range(steps)]
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    front = hip_lib.scene_preset("front", COLS, ROWS)
    for k in range(steps):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
        if k == 0:
            assert batch.memory().device_bytes == twin.memory().device_bytes
        jobs = (batch.export_scenes(camera=front, cols=COLS, rows=ROWS), batch.export_scenes([3, 0], camera=front, cols=COLS, rows=ROWS, device=True))
        if k == 0:
            grown = batch.memory().device_bytes - twin.memory().device_bytes
            # per group an input block (one page here) and, for the host-mode job, the images of its slots
            assert 0 < grown <= 2 * 4096 + n_slots * jobs[0].image_bytes, grown
    assert batch.memory().device_bytes - twin.memory().device_bytes <= 2 * 8192 + n_slots * jobs[0].image_bytes
    for s in range(n_slots):
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes() and len(twin.get_trajectory(s)) == steps
        assert batch.num_keyframes(s) == twin.num_keyframes(s)
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        _check_slot("last", jobs[0], s, s, twin, front)
    batch.close()
    twin.close()
