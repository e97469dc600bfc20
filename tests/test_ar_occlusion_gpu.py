"""The occluded AR picture on the GPU (ar_render_kernel<true> through svo_render_ar_occluded and
svo_submit_export_ar_occluded) against the numpy statement (tests/ar_occlusion_ref.py), byte for byte and count for
count: the crafted cases of tests/ar_occlusion_cases.py, then a ctx of 5 slots in 2 groups against its own view, pose
and cloud jobs, with a box that stands half in the floor of the synthetic room."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ar_occlusion_cases as CASES
import ar_occlusion_ref as OR
import ar_ref as AR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import Handle
from stereo_svo_slam_amd.stereo_slam import ArPictures, StereoSlamBatch

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xA5
ALL = CASES.cases()
_WANT = {}


def _cam(c):
    return hip_lib.ArCamera.from_buffer_copy(np.asarray(c, F).tobytes())


def want(case, pixel, mode, alpha):
    """the statement's (image, covered, hidden) of a case: computed once, shared, never changed"""
    key = (case["name"], pixel, mode, alpha)
    if key not in _WANT:
        _WANT[key] = OR.render(case["gray"], case["cam"], case["draws"], case["light"], case["ambient"], case["near"], pixel,
                               case["lattice"], mode, alpha, case["margin"], case["drop_flags"])
    return _WANT[key]


@pytest.fixture(scope="module")
def handle():
    h = Handle(0, 1024)
    yield h
    h.close()


def upload(cases, pixel):
    """the device arrays of a call that renders `cases` (one style: the first case's light, ambient, near): gray
    planes with a stride above the width at an odd base, draws, lattices, a filled output at offsets that are
    multiples of 4 but not of 16"""
    bpp = AR.BYTES[pixel]
    srcs, offs, occluders, keep = [], [], [], []
    at = 4
    for c in cases:
        W, H = c["W"], c["H"]
        stride = W + 3
        g = np.zeros((H, stride), np.uint8)
        g[:, :W] = c["gray"]
        buf = torch.zeros(H * stride + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(g.ravel()).cuda()
        dd = []
        for model, v, t, rgb, rgb_all in c["draws"]:
            tv = torch.from_numpy(np.ascontiguousarray(v, F).reshape(-1, 3)).cuda()
            tt = torch.from_numpy(np.ascontiguousarray(t, np.int32).reshape(-1, 3)).cuda()
            tc = None if rgb is None else torch.from_numpy(np.asarray(rgb, np.uint32).view(np.int32)).cuda()
            dd.append((model, tv, tt, tc, rgb_all))
        if c["lattice"] is None:
            occluders.append(hip_lib.ar_occluder(None))
        else:
            rec, cols, rows, step = c["lattice"]
            tr = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).cuda()
            keep.append(tr)
            occluders.append(hip_lib.ar_occluder(tr, cols, rows, step))
        keep.append((buf, dd))
        srcs.append(((buf.data_ptr() + 1, W, H, stride), dd))
        offs.append(at)
        at += (H * W * bpp + 3) // 4 * 4 + 4
    out = torch.full((at + 16,), FILL, dtype=torch.uint8, device="cuda")
    return srcs, offs, occluders, out, keep


def run(handle, cases, pixel, mode, alpha=128, occlusion=None, check=True):
    """renders the cases in one call; checks every image and count against the statement and every other byte against
    the fill. Returns [(image, covered, hidden)]."""
    bpp = AR.BYTES[pixel]
    c0 = cases[0]
    assert all((c["light"], c["ambient"], c["near"], c["margin"], c["drop_flags"]) ==
               (c0["light"], c0["ambient"], c0["near"], c0["margin"], c0["drop_flags"]) for c in cases)
    srcs, offs, occluders, out, keep = upload(cases, pixel)
    style = hip_lib.ar_style(pixel=pixel, light=c0["light"], ambient=c0["ambient"], near=c0["near"])
    if occlusion is None:
        occlusion = hip_lib.ar_occlusion(hidden=mode, alpha=alpha, margin=c0["margin"], drop_flags=c0["drop_flags"])
    vis = handle.render_ar(srcs, [_cam(c["cam"]) for c in cases], offs, style, out, occluders, occlusion)
    got = out.cpu().numpy()
    used = np.zeros(len(got), bool)
    res = []
    for i, c in enumerate(cases):
        W, H = c["W"], c["H"]
        mine = got[offs[i]:offs[i] + H * W * bpp].reshape(H, W, bpp)
        used[offs[i]:offs[i] + H * W * bpp] = True
        res.append((mine, int(vis[i]["covered"]), int(vis[i]["hidden"])))
        if check:
            img, covered, hidden = want(c, pixel, mode, alpha)
            print(c["name"], pixel, mode, "covered", res[-1][1], covered, "hidden", res[-1][2], hidden, "pixels off", int((mine != img).any(axis=2).sum()))
            assert (res[-1][1], res[-1][2]) == (covered, hidden), (c["name"], res[-1][1:], covered, hidden)
            assert mine.tobytes() == img.tobytes(), (c["name"], int((mine != img).any(axis=2).sum()))
            assert int(vis[i]["status"]) == (hip_lib.CLOUD_NONE if c["lattice"] is None else hip_lib.CLOUD_OK)
            assert int(vis[i]["occluder_points"]) == 0 and int(vis[i]["_pad"]) == 0
    assert (got[~used] == FILL).all()
    return res


def groups_of(cases):
    """the cases that one call can render together (one style, margin and drop_flags)"""
    out = {}
    for c in cases:
        out.setdefault((c["light"], c["ambient"], c["near"], c["margin"], c["drop_flags"]), []).append(c)
    return list(out.values())


@pytest.mark.parametrize("mode", (OR.DROP, OR.DIM))
@pytest.mark.parametrize("pixel", (AR.RGB8, AR.RGBA8))
def test_every_case(handle, pixel, mode):
    """every case, the ones that share a style in one call: images of different sizes with their own lattices and
    steps, one of them without records"""
    gs = groups_of(ALL)
    assert max(len(g) for g in gs) >= 3 and any(c["lattice"] is None for g in gs if len(g) >= 3 for c in g)
    for g in gs:
        run(handle, g, pixel, mode)


def test_dim_alphas(handle):
    case = next(c for c in ALL if c["name"] == "dim ends")
    imgs = [run(handle, [case], AR.RGB8, OR.DIM, a)[0][0] for a in (0, 1, 128, 255, 256)]
    assert len({i.tobytes() for i in imgs}) == 5


def test_chunked_tile_table(handle, monkeypatch):
    case = next(c for c in ALL if c["name"] == "130x33 step 4 small and large")
    monkeypatch.setenv("SVO_AR_TABLE_TILES", "1")
    run(handle, [case, case], AR.RGBA8, OR.DROP)


def test_without_an_occluder_it_is_render_ar(handle):
    """on = 0, a NULL occlusion's twin (the old entry), records = NULL and an all-dropped lattice: the bytes of
    svo_render_ar"""
    cases = [c for c in ALL if c["margin"] == 0.0 and c["drop_flags"] == 0 and c["ambient"] == CASES.AMBIENT]
    assert len(cases) >= 3
    for pixel in (AR.RGB8, AR.RGBA8):
        srcs, offs, occluders, out, keep = upload(cases, pixel)
        style = hip_lib.ar_style(pixel=pixel, light=CASES.LIGHT, ambient=CASES.AMBIENT, near=CASES.NEAR)
        cams = [_cam(c["cam"]) for c in cases]
        assert handle.render_ar(srcs, cams, offs, style, out) is None
        plain = out.cpu().numpy().copy()
        for i, c in enumerate(cases):
            img = AR.render(c["gray"], c["cam"], c["draws"], c["light"], c["ambient"], c["near"], pixel)
            assert plain[offs[i]:offs[i] + img.size].tobytes() == img.tobytes()
        out.fill_(FILL)
        vis = handle.render_ar(srcs, cams, offs, style, out, occluders, hip_lib.ar_occlusion(on=False))
        assert out.cpu().numpy().tobytes() == plain.tobytes()
        assert (vis["status"] == hip_lib.CLOUD_NONE).all() and (vis["covered"] == 0).all() and (vis["hidden"] == 0).all()
        out.fill_(FILL)
        vis = handle.render_ar(srcs, cams, offs, style, out, [hip_lib.ar_occluder(None)] * len(cases), hip_lib.ar_occlusion())
        assert out.cpu().numpy().tobytes() == plain.tobytes()
        assert (vis["status"] == hip_lib.CLOUD_NONE).all() and (vis["hidden"] == 0).all()
        assert [int(v) for v in vis["covered"]] == [want(c, pixel, OR.DROP, 128)[1] for c in cases]
        res = run(handle, [CASES.all_dropped(c) for c in cases if c["lattice"] is not None], pixel, OR.DROP, check=False)
        for (mine, covered, hidden), c in zip(res, [c for c in cases if c["lattice"] is not None]):
            img = AR.render(c["gray"], c["cam"], c["draws"], c["light"], c["ambient"], c["near"], pixel)
            assert mine.tobytes() == img.tobytes() and hidden == 0 and covered == want(c, pixel, OR.DROP, 128)[1]


def test_stage_entry_rejects(handle):
    lib = hip_lib.lib()
    case = ALL[0]
    srcs, offs, occluders, out, keep = upload([case], AR.RGB8)
    packed = handle.pack_ar(srcs, [_cam(case["cam"])], offs)
    st = hip_lib.ar_style()
    vis = np.zeros(1, hip_lib.AR_VISIBILITY_DTYPE)
    vis.view(np.uint8)[:] = FILL
    rec = occluders[0].records

    def rejected(occluder=None, occlusion=None, occl_array=True):
        arr = (hip_lib.ArOccluder * 1)(occluders[0] if occluder is None else occluder) if occl_array else None
        o = hip_lib.ar_occlusion() if occlusion is None else occlusion
        rc = lib.svo_render_ar_occluded(handle._h, packed[0], packed[1], packed[2], packed[3], C.byref(st), C.byref(o), arr,
                                        C.c_void_p(out.data_ptr()), C.c_void_p(vis.ctypes.data))
        assert rc == -1, (occluder, occlusion)

    for step in (0, -1, 17):
        rejected(hip_lib.ArOccluder(rec, 64, 16, step, 0))
    rejected(hip_lib.ArOccluder(rec, 0, 16, 1, 0)); rejected(hip_lib.ArOccluder(rec, 64, -1, 1, 0))
    rejected(hip_lib.ArOccluder(rec + 8, 32, 16, 1, 0)); rejected(hip_lib.ArOccluder(rec, 64, 16, 1, 1))
    rejected(hip_lib.ArOccluder(None, 0, 0, 0, 1)); rejected(occl_array=False)
    for field, value in (("on", 2), ("hidden", 2), ("alpha", 257), ("alpha", -1), ("margin", -1.0), ("margin", float("nan")), ("_reserved2", 1)):
        o = hip_lib.ar_occlusion()
        setattr(o, field, value)
        rejected(occlusion=o)
    assert (out == FILL).all() and (vis.view(np.uint8) == FILL).all()
    run(handle, [case], AR.RGB8, OR.DROP)                                  # still usable


# ---------------------------------------------------------------------------------- the ctx against its own jobs

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
# The room of synth.py has its floor at y = 1.6 (y is down) and the camera starts at the origin looking along +z. A box
# of edge 0.8 about (0, 1.6, 4) stands half in the floor: the rays to its lower half meet the floor first, its upper
# half stands before the back wall (z = 6.5) and the floor behind it.
BOX = hip_lib.ar_box(0.8)
MESHES = [BOX]
INSTANCES = [(hip_lib.ar_model((0.0, 1.6, 4.0)), 0, 0xc08040)]
OCCLUSION = dict(step=4, margin=0.05, max_depth=20.0, lr_check=1.5)


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


def _statement(batch, s, style, occlusion, hidden, alpha):
    """(image, covered, hidden, kept) of slot s by the statement: ar_occlusion_ref applied to the view job's left
    plane, svo_ar_camera_of_pose of the pose, and the organized camera-frame records of an export_cloud with the same
    style and check"""
    gray = batch.export_views("frames", [s], plane="left", level=0, pixel="gray8").image(0)
    o = dict(ArPictures.OCCLUSION_DEFAULTS, **occlusion)
    cloud = batch.export_cloud("frames", [s], step=o["step"], win=o["win"], search_x=o["search_x"], search_y=o["search_y"], frame="camera",
                               layout="organized", min_disparity=o["min_disparity"], max_depth=o["max_depth"],
                               max_mean_cost=o["max_mean_cost"], lr_check=o["lr_check"] or None)
    rec = cloud.organized(0)
    _, cam = batch.slot_rig(s)
    camera = np.frombuffer(bytes(hip_lib.ar_camera_of_pose(batch.pose(s), cam)), F)
    draws = [(np.asarray(m, F), MESHES[k][0], MESHES[k][1], None, rgb) for m, k, rgb in INSTANCES]
    img, covered, hid = OR.render(np.asarray(gray), camera, draws, tuple(style.light), style.ambient, style.near, style.pixel,
                                  (rec.reshape(-1), cloud.cols, cloud.rows, o["step"]), hidden, alpha, o["margin"], o["drop_flags"])
    return img, covered, hid, int(cloud.segments[0]["n_points"])


def _check_job(tag, job, named, batch, occlusion, hidden=OR.DROP, alpha=128):
    """every named slot of the job against the statement; returns [(covered, hidden)] of the delivered ones"""
    out = []
    for i, s in enumerate(named):
        seg, vis = job.segments[i], job.visibility[i]
        if int(seg["frame_id"]) < 0:
            assert (int(seg["status"]), int(vis["status"]), int(vis["covered"]), int(vis["hidden"]), int(vis["occluder_points"])) == \
                   (hip_lib.AR_NONE, hip_lib.CLOUD_NONE, 0, 0, 0), (tag, s)
            assert job.image(i) is None
            continue
        img, covered, hid, kept = _statement(batch, s, job.style, occlusion, hidden, alpha)
        got = job.image(i)
        got = got.cpu().numpy() if job.device_mode else got
        print(tag, "slot", s, "covered", int(vis["covered"]), covered, "hidden", int(vis["hidden"]), hid, "occluder points",
              int(vis["occluder_points"]), kept, "pixels off", int((got != img).any(axis=2).sum()))
        assert (int(seg["status"]), int(vis["status"])) == (hip_lib.AR_OK, hip_lib.CLOUD_OK), (tag, s)
        assert (int(vis["covered"]), int(vis["hidden"]), int(vis["occluder_points"]), int(vis["_pad"])) == (covered, hid, kept, 0), (tag, s)
        assert got.tobytes() == img.tobytes(), (tag, s, int((got != img).any(axis=2).sum()))
        out.append((covered, hid))
    return out


@pytest.mark.parametrize("device", (False, True))
def test_ctx_against_the_statement(played, device):
    """5 slots in 2 groups, slot 3 with its rig's intrinsics, slot 4 empty; drop and dim, RGB8 and RGBA8"""
    for pixel, hidden, alpha in (("rgb8", "drop", 128), ("rgba8", "dim", 96)):
        occ = dict(OCCLUSION, hidden=hidden, alpha=alpha)
        job = ArPictures(played, None, hip_lib.ar_style(pixel=pixel), MESHES, INSTANCES, None, device, occ)
        job._buf.fill_(FILL)
        job.submit().wait()
        counts = _check_job(pixel, job, range(5), played, OCCLUSION, hip_lib.AR_HIDDEN.index(hidden), alpha)
        # the box straddles the floor: somewhere both a good part of it is hidden and a good part is seen
        assert any(h * 20 > c and (c - h) * 20 > c for c, h in counts), counts
        px = job.pixels.cpu().numpy() if device else job.pixels
        assert (px[4 * job.image_bytes:] == FILL).all()                     # the empty slot wrote only its segment
        used = job.rows * job.pitch
        assert all((px[s * job.image_bytes + used:(s + 1) * job.image_bytes] == FILL).all() for s in range(4))
    # named slots out of order, through the batch's own entry
    job = played.export_ar(MESHES, INSTANCES, [3, 0, 4, 2], device=device, occlusion=OCCLUSION)
    _check_job("named", job, [3, 0, 4, 2], played, OCCLUSION)


def test_lr_check_on_and_off(played):
    plain = dict(OCCLUSION, lr_check=0.0)
    a = played.export_ar(MESHES, INSTANCES, [0, 1], occlusion=OCCLUSION)
    b = played.export_ar(MESHES, INSTANCES, [0, 1], occlusion=plain)
    _check_job("lr on", a, [0, 1], played, OCCLUSION)
    _check_job("lr off", b, [0, 1], played, plain)
    assert all(int(x["occluder_points"]) < int(y["occluder_points"]) for x, y in zip(a.visibility, b.visibility))   # the check drops cells
    for i, s in enumerate((0, 1)):
        recs = [played.export_cloud("frames", [s], step=4, frame="camera", layout="organized", max_depth=20.0, lr_check=lr).organized(0)
                for lr in (1.5, None)]
        differs = (a.image(i) != b.image(i)).any(axis=2)
        cell = (recs[0]["flags"] != recs[1]["flags"]).repeat(4, 0).repeat(4, 1)
        assert not (differs & ~cell[:differs.shape[0], :differs.shape[1]]).any()    # the pictures differ only in cells the check drops


def test_three_slots_in_chunks_of_one(tiny, monkeypatch):
    cfg, seqs = tiny
    batch = _batch(cfg, 3, 1)
    for k in range(3):
        batch.new_images(*_frames(3, seqs, k, (0, 2)))                     # (slot 1 stays empty: a chunk without a picture)
    one = batch.export_ar(MESHES, INSTANCES, occlusion=OCCLUSION)
    monkeypatch.setenv("SVO_AR_CHUNK_SLOTS", "1")
    for device in (False, True):
        job = batch.export_ar(MESHES, INSTANCES, device=device, occlusion=OCCLUSION)
        px = job.pixels.cpu().numpy() if device else job.pixels
        assert px.tobytes() == one.pixels.tobytes() and job.visibility.tobytes() == one.visibility.tobytes()
        assert job.segments.tobytes() == one.segments.tobytes()
    assert [int(s) for s in one.segments["status"]] == [hip_lib.AR_OK, hip_lib.AR_NONE, hip_lib.AR_OK]
    _check_job("chunked", job, range(3), batch, OCCLUSION)
    batch.close()


def _raw_submit(batch, occlusion, dst, seqs=None, mem=0):
    v, t = np.ascontiguousarray(BOX[0]), np.ascontiguousarray(BOX[1])
    meshes = (hip_lib.ArMesh * 1)(hip_lib.ArMesh(v.ctypes.data, t.ctypes.data, None, 8, 12, 0))
    inst = (hip_lib.ArInstance * 1)(hip_lib.ar_instance(*INSTANCES[0]))
    st = hip_lib.ar_style()
    arr = None if seqs is None else (C.c_int * len(seqs))(*seqs)
    return hip_lib.lib().svo_submit_export_ar_occluded(batch._ctx, arr, 0 if seqs is None else len(seqs), C.byref(st),
                                                       None if occlusion is None else C.byref(occlusion), meshes, 1, inst, None, 1,
                                                       C.byref(dst), mem)


def test_memory_rejections_and_no_side_effects(tiny):
    """on = 0 and a NULL occlusion through the new entry are the old entry (bytes and memory); the live layer's block is
    all an occluded job adds to an unoccluded one plus a cloud job; rejected calls queue nothing; later frames are the
    bits of a ctx that never drew, whose memory is the parent's"""
    cfg, seqs = tiny
    n_slots = 4
    old, new, occluded, never = (_batch(cfg, n_slots, 2) for _ in range(4))
    for k in range(2):
        for b in (old, new, occluded, never):
            b.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
    before = never.memory().device_bytes
    assert {b.memory().device_bytes for b in (old, new, occluded)} == {before}
    # on = 0 / NULL through the new entry, and the old entry
    a = old.export_ar(MESHES, INSTANCES)
    off = hip_lib.ar_occlusion(on=False, step=0)                           # (with on == 0 the cloud style is not read)
    st = hip_lib.ar_style()
    _, image_bytes = hip_lib.ar_size(new.cam, new.width, new.height, st)
    for occlusion in (off, None):
        seg = np.zeros(n_slots, hip_lib.AR_SEGMENT_DTYPE)
        px = torch.zeros(n_slots * image_bytes, dtype=torch.uint8).pin_memory()
        assert _raw_submit(new, occlusion, hip_lib.ArDst(seg.ctypes.data, px.data_ptr(), n_slots * image_bytes)) == 0
        new.wait()
        assert px.numpy().tobytes() == a.pixels.tobytes() and seg.tobytes() == a.segments.tobytes()
    assert new.memory().device_bytes == old.memory().device_bytes > before
    # an occluded job against an unoccluded one plus a checked cloud job: the live layer's block, 16 bytes a point
    cloud = old.export_cloud("frames", None, step=4, frame="camera", layout="organized", max_depth=20.0, lr_check=1.5, device=True)
    job = occluded.export_ar(MESHES, INSTANCES, occlusion=OCCLUSION)
    grown = occluded.memory().device_bytes
    assert grown - old.memory().device_bytes == n_slots * 16 * cloud.points_per_slot
    occluded.export_ar(MESHES, INSTANCES, occlusion=OCCLUSION)
    occluded.export_ar(MESHES, INSTANCES, [2, 1], device=True, occlusion=dict(OCCLUSION, hidden="dim"))
    assert occluded.memory().device_bytes == grown                         # not again
    # rejected calls
    seg = np.zeros(n_slots, hip_lib.AR_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = FILL
    vis = np.zeros(n_slots, hip_lib.AR_VISIBILITY_DTYPE)
    vis.view(np.uint8)[:] = FILL
    px = torch.full((n_slots * image_bytes,), FILL, dtype=torch.uint8).pin_memory()
    dst = hip_lib.ArDst(seg.ctypes.data, px.data_ptr(), n_slots * image_bytes)
    nan, inf = float("nan"), float("inf")
    bad = []
    for kw in (dict(alpha=257), dict(alpha=-1), dict(margin=-0.1), dict(margin=inf), dict(margin=nan), dict(hidden=2), dict(hidden=-1),
               dict(step=0), dict(step=17), dict(win=36), dict(search_x=65), dict(min_disparity=-1.0), dict(max_depth=nan), dict(max_mean_cost=inf)):
        bad.append(hip_lib.ar_occlusion(info=vis, **kw))
    for path, value in (("on", 2), ("on", -1), ("_reserved2", 1), ("cloud.frame", hip_lib.CLOUD_WORLD), ("cloud.layout", hip_lib.CLOUD_ORGANIZED),
                        ("cloud._reserved", 1), ("check.lr", 2), ("check.max_lr_diff", -1.0), ("check._reserved", 1), ("_reserved", 1)):
        o = hip_lib.ar_occlusion(info=vis, lr_check=1.5)
        target, names = o, path.split(".")
        for name in names[:-1]:
            target = getattr(target, name)
        if names[-1] == "_reserved":
            target._reserved[len(target._reserved) - 1] = value
        else:
            setattr(target, names[-1], value)
        bad.append(o)
    lr0 = hip_lib.ar_occlusion(info=vis)
    lr0.check.lr = 1                                                       # (a cloud's check needs a tolerance)
    bad.append(lr0)
    for o in bad:
        assert _raw_submit(occluded, o, dst) == -1
        assert hip_lib.lib().svo_last_error()
    assert _raw_submit(occluded, hip_lib.ar_occlusion(info=vis), dst, seqs=[0, 0]) == -1      # (what the old entry rejects)
    assert _raw_submit(occluded, hip_lib.ar_occlusion(info=vis), dst, mem=2) == -1
    occluded.wait()
    assert (seg.view(np.uint8) == FILL).all() and (vis.view(np.uint8) == FILL).all() and (px.numpy() == FILL).all()
    # later frames: the bits of the ctx that never drew; jobs not waited for are ordered with the frame sets
    for k in range(2, 4):
        for b in (occluded, never):
            b.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
        last = occluded.submit_ar(MESHES, INSTANCES, occlusion=OCCLUSION)
    occluded.wait()
    for s in range(n_slots):
        x, y = occluded.get_frame(s), never.get_frame(s)
        assert (x.kps2d.tobytes(), x.kps3d.tobytes(), x.info.tobytes(), x.pose.tobytes()) == \
               (y.kps2d.tobytes(), y.kps3d.tobytes(), y.info.tobytes(), y.pose.tobytes())
        assert occluded.get_trajectory(s).tobytes() == never.get_trajectory(s).tobytes()
    assert never.memory().device_bytes == before
    _check_job("after", last, range(n_slots), occluded, OCCLUSION)
    del job
    for b in (old, new, occluded, never):
        b.close()
