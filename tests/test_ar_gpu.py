"""The AR picture on the GPU (ar.hip through svo_render_ar and svo_submit_export_ar) against the numpy restatement
(tests/ar_ref.py), byte for byte: crafted triangles at the smallest shapes where the kernels can go wrong, then a ctx
of 5 slots in 2 groups against its own getters."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ar_ref as AR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import Handle
from stereo_svo_slam_amd.stereo_slam import ArPictures, StereoSlamBatch

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xA5
SIZES = ((64, 16), (65, 17), (200, 40))                    # one tile; edge tiles of one pixel; 4 x 3 tiles
LIGHT, AMBIENT, NEAR = (0.0, 0.0, 1.0), 0.25, 0.01
I12 = np.eye(3, 4, dtype=F).ravel()
PIX = np.concatenate([I12, np.asarray([1, 1, 0, 0], F)])   # a vertex (u z, v z, z) lands on (u, v) at depth z


def _cam(c):
    return hip_lib.ArCamera.from_buffer_copy(np.asarray(c, F).tobytes())


@pytest.fixture(scope="module")
def handle():
    h = Handle(0, 1024)
    yield h
    h.close()


def tri(p0, p1, p2, z=(1.0, 1.0, 1.0)):
    """three vertices that PIX projects to the pixel coordinates p at depths z"""
    return [(F(p[0]) * F(d), F(p[1]) * F(d), F(d)) for p, d in zip((p0, p1, p2), z)]


def mesh(tris, rgb=None, rgb_all=0xc08040, model=I12):
    """a draw of independent triangles (vertices three by three)"""
    v = np.asarray([p for t in tris for p in t], F).reshape(-1, 3)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return (np.asarray(model, F), v, t, None if rgb is None else np.asarray(rgb, np.uint32), rgb_all)


def run(handle, images, pixel, light=LIGHT, ambient=AMBIENT, near=NEAR):
    """images: [(W, H, camera float32 [16], draws)]. Renders all in one call over random gray planes (stride above
    the width, an odd base) into a filled buffer at offsets that are multiples of 4 but not of 16; checks every image
    against the restatement and every other byte against the fill. Returns the images."""
    rng = np.random.default_rng(len(images) * 7 + pixel)
    bpp = AR.BYTES[pixel]
    srcs, offs, grays, keep = [], [], [], []
    at = 4
    for W, H, cam, draws in images:
        stride = W + 3
        g = rng.integers(0, 256, (H, stride), dtype=np.uint8)
        buf = torch.zeros(H * stride + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(g.ravel()).cuda()
        dd = []
        for model, v, t, rgb, rgb_all in draws:
            tv = torch.from_numpy(np.ascontiguousarray(v, F).reshape(-1, 3) if len(v) else np.zeros((1, 3), F)).cuda()
            tt = torch.from_numpy(np.ascontiguousarray(t, np.int32).reshape(-1, 3)).cuda() if len(t) else torch.zeros((0, 3), dtype=torch.int32, device="cuda")
            tc = None if rgb is None else torch.from_numpy(np.asarray(rgb, np.uint32).view(np.int32)).cuda()
            dd.append((model, tv if len(v) else tv[:0], tt, tc, rgb_all))
        keep.append((buf, dd))
        srcs.append(((buf.data_ptr() + 1, W, H, stride), dd))
        grays.append(g[:, :W])
        offs.append(at)
        at += (H * W * bpp + 3) // 4 * 4 + 4
    out = torch.full((at + 16,), FILL, dtype=torch.uint8, device="cuda")
    style = hip_lib.ar_style(pixel=pixel, light=light, ambient=ambient, near=near)
    handle.render_ar(srcs, [_cam(im[2]) for im in images], offs, style, out)
    got = out.cpu().numpy()
    used = np.zeros(len(got), bool)
    res = []
    for i, (W, H, cam, draws) in enumerate(images):
        want = AR.render(grays[i], cam, draws, light, ambient, near, pixel)
        mine = got[offs[i]:offs[i] + H * W * bpp].reshape(H, W, bpp)
        assert mine.tobytes() == want.tobytes(), (i, W, H, int((mine != want).any(axis=2).sum()))
        used[offs[i]:offs[i] + H * W * bpp] = True
        res.append((mine, grays[i]))
    assert (got[~used] == FILL).all()
    return res


def covered(res):
    """pixels of (image, gray) that show something other than the gray plane"""
    img, g = res
    return int((img[:, :, :3] != g[:, :, None]).any(axis=2).sum())


@pytest.mark.parametrize("pixel", (AR.RGB8, AR.RGBA8))
@pytest.mark.parametrize("size", SIZES)
def test_crafted_triangles(handle, size, pixel):
    W, H = size
    inf, nan = float("inf"), float("nan")
    cases = {
        "inside one tile": [mesh([tri((5.3, 2.1), (30.7, 4.2), (12.5, 13.9))])],
        "across tiles": [mesh([tri((50.2, 10.1), (80.9, 12.4), (60.3, 30.7))])],
        "the whole image": [mesh([tri((-10, -10), (3 * W, -10), (-10, 3 * H))])],
        "a sliver": [mesh([tri((0, 0.4375), (10, 0.4375), (10, 0.5625)), tri((0, 1.0625), (10, 1.0625), (10, 1.1875))])],
        "on centres": [mesh([tri((0.5, 0.5), (4.5, 0.5), (0.5, 4.5)), tri((10.5, 2.5), (20.5, 12.5), (10.5, 12.5))])],
        "a shared edge": [mesh([tri((3.2, 1.7), (40.4, 3.3), (20.6, 14.8)), tri((40.4, 3.3), (20.6, 14.8), (55.1, 15.9))], rgb=[0xff0000, 0x00ff00])],
        "interpenetrating": [mesh([tri((2, 2), (60, 3), (30, 15), (1, 1, 3)), tri((3, 1), (58, 2), (28, 14), (3, 3, 1))], rgb=[0xff0000, 0x0000ff])],
        "coplanar": [mesh([tri((2, 2), (60, 3), (30, 15)), tri((2, 2), (60, 3), (30, 15))], rgb=[0x808080, 0x7f8080]),
                     mesh([tri((2, 2), (60, 3), (30, 15))], rgb_all=0x80807f)],
        "no area": [mesh([tri((1, 1), (10, 10), (20, 20)), tri((4, 4), (4, 4), (30, 9)), tri((5, 5), (5, 5), (5, 5))])],
        "behind near": [mesh([tri((2, 2), (60, 3), (30, 15), (1, 1, 0.001)), tri((2, 2), (60, 3), (30, 15), (1, -1, 1))])],
        "not finite": [mesh([[(inf, 0, 1), (5, 0, 1), (0, 5, 1)], [(0, 0, 1), (nan, 0, 1), (0, 5, 1)], [(0, 0, 1), (5, 0, 1), (0, 3e38, 1)]],
                            model=np.asarray([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 1, 0], F))],
        "beyond 2^15": [mesh([tri((0, 0), (32768, 0), (0, 10)), tri((0, 0), (10, -32768.5), (5, 10)), tri((32767.9, 0), (0, 0), (0, 10))])],
        "outside": [mesh([tri((-50, -50), (-20, -50), (-50, -20)), tri((W + 1, 0), (W + 30, 0), (W + 1, 30)), tri((0, H + 0.6), (30, H + 0.6), (0, H + 9))])],
        "nothing": [],
        "an empty mesh": [mesh([]), mesh([tri((1, 1), (9, 1), (1, 9))])],
    }
    names = list(cases)
    res = run(handle, [(W, H, PIX, cases[k]) for k in names], pixel)
    n = {k: covered(r) for k, r in zip(names, res)}
    assert n["inside one tile"] > 100 and n["the whole image"] >= W * H - 2 and n["on centres"] == 15 + 66
    assert n["a sliver"] == 5 and n["no area"] == 0 and n["behind near"] == 0 and n["not finite"] == 0 and n["outside"] == 0 and n["nothing"] == 0
    assert n["beyond 2^15"] > 0                                            # (the third one is drawn: 32767.9 < 2^15)
    if W == 200:
        assert n["across tiles"] > 200


def test_the_key_decides_per_pixel(handle):
    (img, g), (img2, g2) = run(handle, [(64, 16, PIX, [mesh([tri((2, 2), (60, 3), (30, 15), (1, 1, 3)), tri((3, 1), (58, 2), (28, 14), (3, 3, 1))],
                                                             rgb=[0xff0000, 0x0000ff])]),
                                       (64, 16, PIX, [mesh([tri((2, 2), (60, 3), (30, 15)), tri((2, 2), (60, 3), (30, 15))], rgb=[0x808080, 0x7f8080])])],
                              AR.RGB8, ambient=1.0)
    red, blue = (img == (255, 0, 0)).all(axis=2).sum(), (img == (0, 0, 255)).all(axis=2).sum()
    assert red > 20 and blue > 20                                          # each is nearer somewhere
    won = (img2 == (0x7f, 0x80, 0x80)).all(axis=2)                         # the smaller colour word, everywhere the two cover
    assert won.sum() > 100 and (won | (img2 == g2[:, :, None]).all(axis=2)).all()


def _small_triangles(rng, n, W, H):
    tris, cols = [], []
    for _ in range(n):
        c = np.array([rng.uniform(-2, W + 2), rng.uniform(-2, H + 2)])
        p = c + rng.uniform(-3, 3, (3, 2))
        tris.append(tri(p[0], p[1], p[2], rng.uniform(0.5, 4, 3)))
        cols.append(int(rng.integers(0, 1 << 24)))
    return tris, cols


@pytest.mark.parametrize("size", SIZES)
def test_many_small_triangles_mixed_with_large_ones(handle, size, monkeypatch):
    """257 and 600 small triangles (the walk takes 256 at a time) with two large ones among them: both paths of the
    tile pass in one tile, in every round position; also with a tile table of 1 (chunked launches)"""
    W, H = size
    rng = np.random.default_rng(W)
    images = []
    for n in (257, 600):
        tris, cols = _small_triangles(rng, n, W, H)
        big = [tri((-5, -3), (W + 9, 2), (W / 2, H + 20), (2, 3, 1.5)), tri((W, H), (0, H - 1), (W / 3, -4), (1.2, 2.5, 3))]
        tris[100:100] = big[:1]; cols[100:100] = [0x40c040]
        tris.append(big[1]); cols.append(0xc040c0)
        images.append((W, H, PIX, [mesh(tris[:300], rgb=cols[:300]), mesh(tris[300:], rgb=cols[300:])]))
    res = run(handle, images, AR.RGBA8)
    assert all(covered(r) > W * H // 2 for r in res)
    monkeypatch.setenv("SVO_AR_TABLE_TILES", "1")
    res2 = run(handle, images, AR.RGBA8)
    assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(res, res2))


def test_three_images_with_their_own_cameras_colours_and_models(handle):
    """three images of different sizes, triangle counts and cameras in one call; per-triangle and per-instance colours;
    models that scale, rotate and move; a vertex index out of range; small, large, small on one handle"""
    box_v, box_t = hip_lib.ar_box(1.0)
    rot = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])
    cams = [AR.camera_of_pose([0.1, -0.05, -0.2, 0.02, -0.3, 0.1], 60.0, 55.0, 31.5, 8.0),
            AR.camera_of_pose([0, 0, 0, 0, 0, 0], 80.0, 80.0, 100.0, 20.0),
            AR.camera_of_pose([-0.3, 0.2, 0.1, 0.4, 0.2, -0.1], 40.0, 42.0, 30.0, 9.0)]
    bad_t = box_t.copy(); bad_t[3, 1] = 8; bad_t[5, 0] = -1
    rgb = np.arange(12, dtype=np.uint32) * 0x151515 + 0x101010
    images = [(65, 17, cams[0], [(hip_lib.ar_model((0.1, 0, 1.5), 0.8, rot), box_v, box_t, rgb, 0)]),
              (200, 40, cams[1], [(hip_lib.ar_model((-0.4, 0, 2.0), 0.5), box_v, box_t, None, 0x3060c0),
                                  (hip_lib.ar_model((0.5, 0.1, 2.5), 1.0, rot), box_v, bad_t, rgb, 0),
                                  (hip_lib.ar_model((0, 0, 1.2), 0.2), box_v, box_t, None, 0xffffff)]),
              (64, 16, cams[2], [])]
    for pixel in (AR.RGB8, AR.RGBA8):
        res = run(handle, images, pixel, light=(0.3, -0.5, 0.8), ambient=0.2)
        assert covered(res[0]) > 50 and covered(res[1]) > 500 and covered(res[2]) == 0
    run(handle, images[2:], AR.RGB8)                                       # a smaller call after the larger one
    run(handle, images[:1], AR.RGB8)


def test_lighting(handle):
    box_v, box_t = hip_lib.ar_box(1.0)
    cam = AR.camera_of_pose([0.9, -0.7, -2.0, -0.3, -0.4, 0.0], 40.0, 40.0, 32.0, 8.0)
    draws = [(hip_lib.ar_model((0, 0, 0)), box_v, box_t, None, 0xe0a060)]
    faces = lambda r: len(np.unique(r[0].reshape(-1, r[0].shape[2])[(r[0][:, :, :3] != r[1][:, :, None]).any(axis=2).ravel()], axis=0))
    r0 = run(handle, [(64, 16, cam, draws)], AR.RGB8, light=(0, 0, 1), ambient=0.0)[0]      # parallel to four faces: those are black
    r1 = run(handle, [(64, 16, cam, draws)], AR.RGB8, light=(0, 0, 1), ambient=1.0)[0]      # every face the plain colour
    r2 = run(handle, [(64, 16, cam, draws)], AR.RGB8, light=(0.2, 0.5, 0.9), ambient=0.3)[0]
    assert (r0[0] == (0, 0, 0)).all(axis=2).any() and (r0[0] == (0xe0, 0xa0, 0x60)).all(axis=2).any()
    assert faces(r1) == 1 and faces(r2) == 3 and covered(r1) == covered(r2) > 30


def test_stage_entry_rejects(handle):
    lib = hip_lib.lib()
    W, H = 64, 16
    gray = torch.zeros(H * W, dtype=torch.uint8, device="cuda")
    out = torch.full((H * W * 4 + 64,), FILL, dtype=torch.uint8, device="cuda")
    v = torch.from_numpy(np.asarray(tri((1, 1), (9, 1), (1, 9)), F)).cuda()
    t = torch.from_numpy(np.arange(3, dtype=np.int32).reshape(1, 3)).cuda()
    st = hip_lib.ar_style()

    def call(img=None, draws=None, cams=None, offs=(0,), style=st, pixels=out, n=1):
        img = (gray, W, H, W) if img is None else img
        draws = [(I12, v, t, None, 0x123456)] if draws is None else draws
        packed = handle.pack_ar([(img, draws)], [_cam(PIX)] if cams is None else cams, offs)
        return packed, style, pixels

    def rejected(code=-1, **kw):
        packed, style, pixels = call(**kw)
        p = pixels.data_ptr() if isinstance(pixels, torch.Tensor) else int(pixels)
        assert lib.svo_render_ar(handle._h, packed[0], packed[1], packed[2], packed[3], C.byref(style), C.c_void_p(p)) == code

    rejected(img=(gray, W, H, W - 1)); rejected(img=(gray, 0, H, W)); rejected(img=(0, W, H, W)); rejected(img=(gray, 32769, 1, 32769))
    rejected(offs=(-4,)); rejected(offs=(2,)); rejected(pixels=0); rejected(pixels=out.data_ptr() + 1)
    nan_model = I12.copy(); nan_model[5] = float("nan")
    rejected(draws=[(nan_model, v, t, None, 0)]); rejected(draws=[(I12, v, t, None, 0x1000000)])
    bad = _cam(PIX); bad.fx = 0.0
    rejected(cams=[bad])
    bad = _cam(PIX); bad.view[7] = float("inf")
    rejected(cams=[bad])
    rejected(style=hip_lib.ar_style(pixel=0)); rejected(style=hip_lib.ar_style(ambient=1.5)); rejected(style=hip_lib.ar_style(near=0.0))
    many = torch.zeros((hip_lib.AR_MAX_TRIANGLES // 2 + 1, 3), dtype=torch.int32, device="cuda")
    capacity = lib.svo_render_ar
    packed, style, pixels = call(draws=[(I12, v, many, None, 0), (I12, v, many, None, 0)])
    rc = capacity(handle._h, packed[0], packed[1], packed[2], packed[3], C.byref(style), C.c_void_p(pixels.data_ptr()))
    assert rc not in (0, -1)
    assert lib.svo_render_ar(handle._h, 1, None, None, None, C.byref(st), C.c_void_p(out.data_ptr())) == -1
    assert (out == FILL).all()
    run(handle, [(W, H, PIX, [mesh([tri((1, 1), (9, 1), (1, 9))])])], AR.RGB8)     # still usable


# ---------------------------------------------------------------------------------- the ctx against its getters

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
def tiny():
    """tiny, 4 sequences of 5 frames of fast motion: shared, never changed"""
    out = []
    for seed in (1, 11, 12, 13):
        cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", 5, seed, motion_scale=4.0)
        out.append((L, R, [float(t) for t in ts]))
    torch.cuda.synchronize()
    return cfg, out


def _frames(n, seqs, k, slots):
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for s in slots:
        L[s], R[s], ts[s] = seqs[s][0][k], seqs[s][1][k], seqs[s][2][k]
    return L, R, ts


RIG = dict(fx=212.0, fy=212.0, cx=151.5, cy=127.25, baseline=23.5)
BOX = hip_lib.ar_box(0.2)
MESHES = [BOX, (BOX[0] * F(0.5), BOX[1], np.arange(12, dtype=np.uint32) * 0x0a1408 + 0x202020)]
INSTANCES = [(hip_lib.ar_model(hip_lib.AR_AT), 0, 0xc08040), (hip_lib.ar_model((0.12, -0.05, 0.4)), 1, 0)]


@pytest.fixture(scope="module")
def played(tiny):
    """5 slots in 2 groups: slots 0 .. 3 after 4 frames (slot 3 on a rig of its own), slot 4 empty"""
    cfg, seqs = tiny
    batch = _batch(cfg, 5, 2)
    ids = batch.add_rigs([{k: dict(cfg, **RIG)[k] for k in hip_lib.RIG_FLOATS}])
    batch.assign_rigs([3], ids)
    for k in range(4):
        batch.new_images(*_frames(5, seqs, k, range(4)))
    yield batch
    batch.close()


def _check_slot(tag, job, i, s, batch, instances):
    """named slot i of the job (slot s) against the getters and the restatement"""
    seg = job.segments[i]
    rig, cam = batch.slot_rig(s)
    pose = batch.pose(s)
    view = batch.export_views("frames", [s], plane="left", level=0, pixel="gray8")
    gray = view.image(0)
    draws = [(np.asarray(m, F), MESHES[k][0], MESHES[k][1], MESHES[k][2] if len(MESHES[k]) > 2 else None, rgb) for m, k, rgb in instances]
    st = job.style
    want = AR.render(gray, AR.camera_of_pose(pose, cam.fx, cam.fy, cam.cx, cam.cy), draws, tuple(st.light), st.ambient, st.near, st.pixel)
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, int(view.segments[0]["run"]), hip_lib.AR_OK), (tag, s)
    assert int(seg["frame_id"]) == batch.stats(s).frame_id and int(seg["offset"]) == i * job.image_bytes, (tag, s)
    assert (int(seg["n_instances"]), int(seg["n_triangles"])) == (len(instances), 12 * len(instances)), (tag, s)
    assert seg["pose"].tobytes() == pose.tobytes() and int(seg["_pad"]) == 0 and int(seg["_pad2"]) == 0, (tag, s)
    got = job.image(i)
    got = got.cpu().numpy() if job.device_mode else got
    assert got.tobytes() == want.tobytes(), (tag, s, int((got != want).any(axis=2).sum()))
    shows = int((want[:, :, :3] != np.asarray(gray)[:, :, None]).any(axis=2).sum())
    assert 200 < shows < want.shape[0] * want.shape[1] // 2, (tag, s, shows)      # some pixels show the box and most the image
    return want


@pytest.mark.parametrize("device", (False, True))
def test_ctx_against_the_getters(played, device):
    """5 slots in 2 groups; slot 2 alone shows the second instance (through `first`); slot 3 has its rig's intrinsics;
    slot 4 is empty"""
    first = [0, 1, 2, 4, 5, 6]
    inst = [INSTANCES[0], INSTANCES[0], INSTANCES[0], INSTANCES[1], INSTANCES[0], INSTANCES[0]]
    for pixel in ("rgb8", "rgba8"):
        job = ArPictures(played, None, hip_lib.ar_style(pixel=pixel), MESHES, inst, first, device)
        job._buf.fill_(FILL)
        job.submit().wait()
        imgs = [_check_slot(pixel, job, s, s, played, inst[first[s]:first[s + 1]]) for s in range(4)]
        assert played.slot_rig(3)[0] != 0 and imgs[3].tobytes() != imgs[0].tobytes()
        seg = job.segments[4]
        assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"]), int(seg["n_triangles"])) == (4, hip_lib.AR_NONE, -1, 0)
        assert job.image(4) is None
        px = job.pixels.cpu().numpy() if device else job.pixels
        assert (px[4 * job.image_bytes:] == FILL).all()
        used = job.rows * job.pitch
        assert all((px[s * job.image_bytes + used:(s + 1) * job.image_bytes] == FILL).all() for s in range(4))
    # named slots out of order, one instance for all
    job = played.export_ar(MESHES, INSTANCES[:1], [3, 0, 4, 2], device=device)
    for i, s in ((0, 3), (1, 0), (3, 2)):
        _check_slot("named", job, i, s, played, INSTANCES[:1])
    assert int(job.segments[2]["status"]) == hip_lib.AR_NONE


def _raw_submit(batch, seqs, n, style, meshes, n_meshes, inst, first, n_inst, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    fa = None if first is None else (C.c_int * len(first))(*first)
    return hip_lib.lib().svo_submit_export_ar(batch._ctx, arr, n, None if style is None else C.byref(style), meshes, n_meshes, inst, fa,
                                              n_inst, None if dst is None else C.byref(dst), mem)


def test_rejected_calls_queue_nothing_and_memory(tiny):
    cfg, seqs = tiny
    n_slots = 4
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(2):
        batch.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
        twin.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
    assert batch.memory().device_bytes == twin.memory().device_bytes
    st = hip_lib.ar_style()
    _, image_bytes = hip_lib.ar_size(batch.cam, batch.width, batch.height, st)
    seg = np.zeros(n_slots, hip_lib.AR_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = FILL
    px = torch.full((n_slots * image_bytes + 16,), FILL, dtype=torch.uint8).pin_memory()
    dpx = torch.full((n_slots * image_bytes + 16,), FILL, dtype=torch.uint8, device="cuda")
    v, t = np.ascontiguousarray(BOX[0]), np.ascontiguousarray(BOX[1])
    rgb = np.full(12, 0x808080, np.uint32)

    def meshes(**kw):
        f = dict(vertices=v.ctypes.data, triangles=t.ctypes.data, rgb=None, n_vertices=8, n_triangles=12, _reserved=0)
        f.update(kw)
        return (hip_lib.ArMesh * 1)(hip_lib.ArMesh(*[f[k] for k in ("vertices", "triangles", "rgb", "n_vertices", "n_triangles", "_reserved")]))

    def insts(n=1, **kw):
        arr = (hip_lib.ArInstance * n)(*[hip_lib.ar_instance(hip_lib.ar_model(hip_lib.AR_AT), 0, 0xc08040) for _ in range(n)])
        for k, val in kw.items():
            if k == "model":
                arr[0].model[val[0]] = val[1]
            elif k == "reserved":
                arr[0]._reserved[1] = val
            else:
                setattr(arr[0], k, val)
        return arr

    dst = lambda p=px.data_ptr(), cap=n_slots * image_bytes, s=seg.ctypes.data: hip_lib.ArDst(s, p, cap)
    ok_m, ok_i = meshes(), insts()
    INVALID = -1
    CAPACITY = _raw_submit(batch, None, 0, st, ok_m, 1, ok_i, None, 1, dst(cap=n_slots * image_bytes - 1), 0)
    assert CAPACITY not in (0, INVALID)
    bad_t = t.copy(); bad_t[7, 2] = 8
    neg_t = t.copy(); neg_t[0, 0] = -1
    bad_rgb = rgb.copy(); bad_rgb[11] = 0x01000000
    style = lambda **kw: hip_lib.ar_style(**kw)
    res = style(); res._reserved[0] = 1
    nan, inf = float("nan"), float("inf")
    calls = [([4], 1, st, ok_m, 1, ok_i, None, 1, dst(), 0), ([-1], 1, st, ok_m, 1, ok_i, None, 1, dst(), 0),
             ([0, 1, 0], 3, st, ok_m, 1, ok_i, None, 1, dst(), 0), ([0], -1, st, ok_m, 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, ok_m, 1, ok_i, None, 1, dst(), 2), (None, 0, st, ok_m, 1, ok_i, None, 1, dst(), -1),
             (None, 0, None, ok_m, 1, ok_i, None, 1, dst(), 0), (None, 0, style(pixel=0), ok_m, 1, ok_i, None, 1, dst(), 0),
             (None, 0, style(light=(0, nan, 1)), ok_m, 1, ok_i, None, 1, dst(), 0), (None, 0, style(ambient=-0.1), ok_m, 1, ok_i, None, 1, dst(), 0),
             (None, 0, style(ambient=1.1), ok_m, 1, ok_i, None, 1, dst(), 0), (None, 0, style(ambient=nan), ok_m, 1, ok_i, None, 1, dst(), 0),
             (None, 0, style(near=0.0), ok_m, 1, ok_i, None, 1, dst(), 0), (None, 0, style(near=-1.0), ok_m, 1, ok_i, None, 1, dst(), 0),
             (None, 0, style(near=inf), ok_m, 1, ok_i, None, 1, dst(), 0), (None, 0, res, ok_m, 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, ok_m, 1, insts(model=(6, nan)), None, 1, dst(), 0), (None, 0, st, ok_m, 1, insts(model=(11, inf)), None, 1, dst(), 0),
             (None, 0, st, ok_m, 1, insts(rgb=0x1000000), None, 1, dst(), 0), (None, 0, st, ok_m, 1, insts(mesh=1), None, 1, dst(), 0),
             (None, 0, st, ok_m, 1, insts(mesh=-1), None, 1, dst(), 0), (None, 0, st, ok_m, 1, insts(reserved=1), None, 1, dst(), 0),
             (None, 0, st, meshes(triangles=bad_t.ctypes.data), 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, meshes(triangles=neg_t.ctypes.data), 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, meshes(rgb=bad_rgb.ctypes.data), 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, meshes(_reserved=1), 1, ok_i, None, 1, dst(), 0), (None, 0, st, meshes(n_vertices=-1), 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, meshes(vertices=None), 1, ok_i, None, 1, dst(), 0), (None, 0, st, meshes(triangles=None), 1, ok_i, None, 1, dst(), 0),
             (None, 0, st, None, 1, ok_i, None, 1, dst(), 0), (None, 0, st, ok_m, 1, None, None, 1, dst(), 0),
             (None, 0, st, ok_m, -1, ok_i, None, 1, dst(), 0), (None, 0, st, ok_m, 1, ok_i, None, -1, dst(), 0),
             (None, 0, st, ok_m, 1, insts(2), [0, 1, 1, 0, 2], 2, dst(), 0), (None, 0, st, ok_m, 1, insts(2), [0, 0, 1, 1, 1], 2, dst(), 0),
             (None, 0, st, ok_m, 1, insts(2), [-1, 0, 1, 1, 2], 2, dst(), 0), ([1, 2], 2, st, ok_m, 1, insts(2), [0, 1, 3], 2, dst(), 0),
             (None, 0, st, ok_m, 1, ok_i, None, 1, None, 0), (None, 0, st, ok_m, 1, ok_i, None, 1, dst(s=None), 0),
             (None, 0, st, ok_m, 1, ok_i, None, 1, dst(p=None), 0), (None, 0, st, ok_m, 1, ok_i, None, 1, dst(p=px.data_ptr() + 2), 0),
             (None, 0, st, ok_m, 1, ok_i, None, 1, dst(p=dpx.data_ptr() + 1), 1)]
    for c in calls:
        assert _raw_submit(batch, *c) == INVALID, c[:2]
        assert hip_lib.lib().svo_last_error()
    assert _raw_submit(batch, [1, 2], 2, st, ok_m, 1, ok_i, None, 1, dst(cap=2 * image_bytes - 1), 0) == CAPACITY
    big_t = np.zeros((hip_lib.AR_MAX_TRIANGLES + 1, 3), np.int32)
    assert _raw_submit(batch, None, 0, st, meshes(triangles=big_t.ctypes.data, n_triangles=len(big_t)), 1, ok_i, None, 1, dst(), 0) == CAPACITY
    half = meshes(triangles=big_t.ctypes.data, n_triangles=hip_lib.AR_MAX_TRIANGLES // 2 + 1)
    assert _raw_submit(batch, None, 0, st, half, 1, insts(2), None, 2, dst(), 0) == CAPACITY            # (the bound is per slot)
    batch.wait()
    assert (seg.view(np.uint8) == FILL).all() and (px.numpy() == FILL).all() and (dpx == FILL).all()
    # nothing else was queued and the ctx goes on: the next frame still tracks, and a picture of it
    batch.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    twin.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    for s in range(n_slots):
        assert batch.pose(s).tobytes() == twin.pose(s).tobytes() and batch.stats(s).frame_id == 2
    before = batch.memory().device_bytes
    jobs = [batch.export_ar(MESHES[:1], INSTANCES[:1]), batch.export_ar(MESHES[:1], INSTANCES[:1], [3, 0], device=True)]
    grown = batch.memory().device_bytes - before
    # per group (2 slots each): an input block (one page here), 12 records of 64 bytes a slot and, for the host-mode job,
    # the images of its slots; the device-mode job of one slot a group fits what is there
    assert grown == 2 * (4096 + 2 * 12 * 64) + n_slots * jobs[0].image_bytes, grown
    batch.export_ar(MESHES[:1], INSTANCES[:1])
    batch.export_ar(MESHES[:1], INSTANCES[:1], [3, 0], device=True)
    assert batch.memory().device_bytes - before == grown                          # not again on a second job
    assert twin.memory().device_bytes == before                                  # (a ctx that never asks has nothing more)
    _check_slot_plain(jobs[0], 1, 1, batch)
    _check_slot_plain(jobs[1], 0, 3, batch)
    batch.close(); twin.close()


def _check_slot_plain(job, i, s, batch):
    gray = batch.export_views("frames", [s], plane="left", level=0, pixel="gray8").image(0)
    _, cam = batch.slot_rig(s)
    st = job.style
    draws = [(np.asarray(INSTANCES[0][0], F), BOX[0], BOX[1], None, INSTANCES[0][2])]
    want = AR.render(gray, AR.camera_of_pose(batch.pose(s), cam.fx, cam.fy, cam.cx, cam.cy), draws, tuple(st.light), st.ambient, st.near, st.pixel)
    got = job.image(i)
    got = got.cpu().numpy() if job.device_mode else got
    assert got.tobytes() == want.tobytes()


def test_no_side_effects(tiny):
    """poses and keypoints are the same bits with and without ar jobs between the steps"""
    cfg, seqs = tiny
    batch, twin = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    for k in range(4):
        batch.new_images(*_frames(3, seqs, k, range(3)))
        twin.new_images(*_frames(3, seqs, k, range(3)))
        batch.submit_ar(MESHES, INSTANCES)                                          # not waited for: ordered with the frame sets
    batch.wait()
    for s in range(3):
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes()
    batch.close(); twin.close()
