"""Cloud points in the scene on the GPU: the stage entry (svo_render_scene_clouds) on the crafted cases of
tests/scene_cloud_cases.py, and the ctx job (svo_submit_export_scenes_clouds) against the restatement
(tests/scene_cloud_ref.py) fed with the getters' sets and lines and the records of a cloud job submitted next to it.
Every comparison is on bytes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import map_ref as MR
import oracle_py as O
import scene_cloud_cases as CC
import scene_cloud_ref as CR
import scene_ref as SR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import Handle
from stereo_svo_slam_amd.stereo_slam import Scenes, StereoSlamBatch

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xA5
PLANES = ("flags", "keyframe_id", "inlier_count", "color")
INVALID = -1


# ---------------------------------------------------------------------------------- stage entry, crafted

def _dev(values, offset, keep):
    """the bytes of `values` in device memory, `offset` bytes past an allocation's start"""
    values = np.ascontiguousarray(values)
    raw = np.zeros(offset + values.nbytes + 16, np.uint8)
    raw[offset:offset + values.nbytes] = values.view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw).cuda()
    keep.append(t)
    return t.data_ptr() + offset


def _cam(c):
    return hip_lib.SceneCamera.from_buffer_copy(np.asarray(c, F).tobytes())


_REF = {}


def _reference(case, style, cloud_size, filt):
    """CR.render of a case, computed once per (case, sizes, filter, background); RGBA adds the fourth byte"""
    cols, rows, cam, sets, lines, spans = case
    key = (id(case), style.point_size, cloud_size, style.background, tuple(sorted(filt.items())))
    if key not in _REF:
        _REF[key] = (case, CR.render(cols, rows, SR.RGB8, np.asarray(cam, F), sets, lines, spans, filt, style.point_size, cloud_size,
                                     style.background))
    rgb = _REF[key][1]
    return rgb if style.pixel == SR.RGB8 else np.concatenate([rgb, np.full((rows, cols, 1), 255, np.uint8)], axis=2)


def _pack(h, cases, style, order, gap):
    bpp = SR.BYTES[style.pixel]
    keep, srcs, cams, offsets, spans = [], [], [], [], []
    at = 8
    for i in order:
        cols, rows, cam, sets, lines, sp = cases[i]
        dev_sets = []
        for j, (n, own_id, k3, planes) in enumerate(sets):
            fields = {"kps3d": _dev(np.ascontiguousarray(k3).view(np.uint32), 12 if j % 2 else 4, keep)}
            for t, name in enumerate(PLANES):
                fields[name] = _dev(planes[name], 4 if (t + j) % 2 else 12, keep)
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
        # (records at a base that is 16-byte but not 32-byte aligned; an empty span keeps a null address)
        spans.append([(_dev(s.view(np.uint8).reshape(-1), 16 + 32 * (j % 2), keep) if len(s) else 0, len(s)) for j, s in enumerate(sp)])
    return keep, srcs, cams, offsets, spans, at + 8


def _call(h, cases, style, cloud_size, filt=MR.KEEP_ALL, order=None, gap=36):
    """one svo_render_scene_clouds of the cases in the given order, into a buffer pre-filled with FILL whose base is
    4-byte but not 16-byte aligned, with gaps between the images; the whole buffer is compared with the restatement"""
    order = list(range(len(cases))) if order is None else order
    keep, srcs, cams, offsets, spans, total = _pack(h, cases, style, order, gap)
    buf = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 4
    assert base % 16 == 4
    h.render_scene_clouds(srcs, spans, cams, offsets, style, cloud_size, base)
    got = buf.cpu().numpy()
    want = np.full(total + 16, FILL, np.uint8)
    for i, off in zip(order, offsets):
        img = _reference(cases[i], style, cloud_size, filt)
        want[4 + off:4 + off + img.size] = img.reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[:5]} (offsets {offsets})"
    bpp = SR.BYTES[style.pixel]
    return [got[4 + off:4 + off + cases[i][0] * cases[i][1] * bpp].reshape(cases[i][1], cases[i][0], bpp) for i, off in zip(order, offsets)]


def _style(pixel=SR.RGB8, point_size=1, background=0xffffff, filt=MR.KEEP_ALL):
    return hip_lib.scene_style(cols=1, rows=1, pixel=pixel, point_size=point_size, background=background, filter=dict(filt))


@pytest.fixture(scope="module")
def handle():
    h = Handle(0, 1024)
    yield h
    h.close()


@pytest.fixture(scope="module")
def shape_cases():
    """the four shapes, then an image without a span and one whose only span is empty (the 65 x 17 sparse elements)"""
    cases = [CC.shape_case(w, h) for w, h in CC.SHAPES]
    return cases + [cases[2][:5] + ([],), cases[2][:5] + ([cases[2][5][0][:0]],)]


@pytest.mark.parametrize("pixel", [SR.RGB8, SR.RGBA8])
def test_image_shapes_in_one_call(handle, shape_cases, pixel, monkeypatch):
    """1 x 1, 63 x 15, 65 x 17, 130 x 33 with two spans each, and images with and without spans, in one call; then in
    another order through a tile table of 2 tiles and a span table of 1 piece (chunked launches of both kernels)"""
    st = _style(pixel, point_size=2)
    imgs = _call(handle, shape_cases, st, 4)
    assert imgs[4].tobytes() == imgs[5].tobytes() != imgs[2].tobytes()
    monkeypatch.setenv("SVO_SCENE_TABLE_TILES", "2")
    monkeypatch.setenv("SVO_SCENE_TABLE_SPANS", "1")
    _call(handle, shape_cases, st, 4, order=[5, 3, 0, 4, 2, 1], gap=4)


@pytest.fixture(scope="module")
def crafted():
    return CC.records_case(), CC.edge_case(), CC.tie_case()


@pytest.mark.parametrize("size", CC.CLOUD_SIZES)
def test_cloud_sizes_on_crafted_records(handle, crafted, size):
    """DROPPED, drop_flags, NaN and infinities, behind and exactly at near, at and beyond 2^15, squares outside and
    across the image's and the tiles' borders, at every point size; the keypoints keep the style's size"""
    st = _style(SR.RGBA8, 3, 0x203040)
    rec, edge, tie = _call(handle, list(crafted), st, size)
    bg = (0x20, 0x30, 0x40)
    x, y = CC.RECORD_PIXEL["at_near"]
    assert tuple(rec[y, x, :3]) != bg, "the record at depth == near is drawn"
    for k in ("dropped", "dropped_and_more", "below_near", "behind"):
        x, y = CC.RECORD_PIXEL[k]
        if size == 1:
            assert tuple(rec[y, x, :3]) == bg, k
    filt = dict(drop_flags=CC.IGNORE_COMPLETELY, own_only=0, min_inliers=0)
    dropped = _call(handle, [crafted[0]], _style(SR.RGBA8, 3, 0x203040, filt), size, filt)[0]
    x, y = CC.RECORD_PIXEL["ignore_completely"]
    assert tuple(rec[y, x, :3]) != bg and (size > 5 or tuple(dropped[y, x, :3]) == bg)
    assert (edge[0, 0, :3] != bg).any() and (edge[32, 129, :3] != bg).any()


def test_ties(handle, crafted):
    tie = crafted[2]
    img = _call(handle, [tie], _style(SR.RGB8, 1), 1)[0]
    px = lambda name: tuple(int(v) for v in img[CC.TIE[name][1], CC.TIE[name][0]])
    assert px("keypoint") == (0xfe, 0xfe, 0xfe) and px("line") == (0xff, 0, 0) and px("beside_line") == (0, 0xaa, 0)
    assert px("smaller") == (0x10, 0x20, 0x30) and px("larger") == (0x30, 0x20, 0x10) and px("nearer") == (0, 0xff, 0)
    # the two spans the other way round: the same picture
    swapped = tie[:5] + (tie[5][::-1],)
    assert _call(handle, [swapped], _style(SR.RGB8, 1), 1)[0].tobytes() == img.tobytes()


def test_span_lengths(handle, monkeypatch):
    cases = [CC.span_case(n) for n in CC.SPAN_LENGTHS]
    _call(handle, cases, _style(SR.RGB8, 2), 1)
    monkeypatch.setenv("SVO_SCENE_TABLE_SPANS", "1")
    _call(handle, cases[::-1], _style(SR.RGBA8, 2), 5)


def test_pile(handle):
    """4096 records of distinct depths on one pixel: the nearest shows, and two runs give the same bytes"""
    case = CC.pile_case()
    a = _call(handle, [case], _style(SR.RGBA8, 1, 0x000000), 1)[0]
    b = _call(handle, [case], _style(SR.RGBA8, 1, 0x000000), 1)[0]
    x, y = CC.PILE_PIXEL
    assert a.tobytes() == b.tobytes() and tuple(a[y, x]) == (0, 0, 1, 255) and int((a[:, :, :3] != 0).any(axis=2).sum()) == 1


def test_no_span_anywhere_is_render_scene(handle, shape_cases):
    st = _style(SR.RGB8, 3)
    cases = [c[:5] + ([],) for c in shape_cases[:4]]
    keep, srcs, cams, offsets, spans, total = _pack(handle, cases, st, range(4), 36)
    a = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    b = a.clone()
    handle.render_scene(srcs, cams, offsets, st, a.data_ptr() + 4)
    handle.render_scene_clouds(srcs, spans, cams, offsets, st, 7, b.data_ptr() + 4)
    assert torch.equal(a, b) and (a != FILL).any()
    c = a.clone().fill_(FILL)
    handle.render_scene_clouds(srcs, [[(0, 0), (0, 0)] for _ in cases], cams, offsets, st, 7, c.data_ptr() + 4)
    assert torch.equal(a, c)


def test_stage_entry_rejects(handle):
    lib = hip_lib.lib()
    st = _style()
    cam = _cam(SR.camera(np.eye(3, 4), 8.0, 4.0, 4.0, 0.5))
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    rec = torch.from_numpy(CR.records([[0, 0, 1.0]], [0x0a0b0c]).view(np.uint8).copy()).cuda()
    ok = lambda: dict(srcs=[(8, 8, [], None)], spans=[[rec]], cameras=[cam], offsets=[0], style=st, point_size=1, pixels=buf)
    handle.render_scene_clouds(**ok())
    img = buf[:192].cpu().numpy().reshape(8, 8, 3)
    assert tuple(img[4, 4]) == (0x0a, 0x0b, 0x0c) and int((img != 255).any(axis=2).sum()) == 1 and (buf[192:] == FILL).all()
    buf.fill_(FILL)
    for bad in (dict(point_size=0), dict(point_size=17), dict(spans=[[(rec.data_ptr(), -1)]]), dict(spans=[[(0, 1)]]),
                dict(spans=[[rec, (rec.data_ptr() + 8, 1)]]), dict(spans=[[(rec.data_ptr() + 4, 1)]]), dict(offsets=[2]),
                dict(srcs=[(0, 8, [], None)]), dict(pixels=buf.data_ptr() + 2), dict(style=hip_lib.scene_style(pixel=0))):
        with pytest.raises(hip_lib.SvoError):
            handle.render_scene_clouds(**dict(ok(), **bad))
    packed = handle.pack_scene(ok()["srcs"], [cam], [0])
    spans, counts, _ = handle.pack_scene_spans([[rec]])
    bad_counts = (C.c_int32 * 1)(-1)
    for args in ((spans, bad_counts), (None, counts), (spans, None)):
        assert lib.svo_render_scene_clouds(handle._h, 1, packed[1], args[0], args[1], packed[2], packed[3], C.byref(st), C.c_int32(1),
                                           C.c_void_p(buf.data_ptr())) == INVALID
    torch.cuda.synchronize()
    assert (buf == FILL).all()
    handle.render_scene_clouds(**ok())                                               # still usable
    assert tuple(buf[:192].cpu().numpy().reshape(8, 8, 3)[4, 4]) == (0x0a, 0x0b, 0x0c)


# ---------------------------------------------------------------------------------- the ctx against its getters and its cloud job

COLS, ROWS = 96, 40
DENSE = dict(step=8, point_size=2)
MIN_CLOUD_SHARE = 0.01                     # of a delivered picture's pixels are won by a class-4 element (and one by a sparse one)


def _sequences(config, seeds, n_frames, motion_scale=4.0):
    out = []
    for seed in seeds:
        cfg, L, R, _, ts = synth.make_sequence_gpu(config, n_frames, seed, motion_scale=motion_scale)
        out.append((L, R, [float(t) for t in ts]))
    torch.cuda.synchronize()
    return cfg, out


def _frame_set(n, live):
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for slot, (seq, k) in live.items():
        L[slot], R[slot], ts[slot] = seq[0][k], seq[1][k], seq[2][k]
    return L, R, ts


@pytest.fixture(scope="module")
def tiny():
    """tiny, seeds (1, 11, 12, 13, 14), 24 frames of fast motion (the recipe of test_scene_gpu.py): shared, never changed"""
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


def _behind(pose, back=1.0):
    """svo_scene_look_at from `back` behind a pose along its viewing direction, its up the pose's"""
    pose = np.asarray(pose, np.float64)
    R = O.rodrigues(pose[3:6].astype(F)).astype(np.float64)
    return hip_lib.scene_look_at(pose[:3] - back * R[:, 2], pose[:3] + R[:, 2], -R[:, 1], 60.0, COLS, ROWS, 0.05)


def _restate(source, s, style, cam, spans, cloud_size):
    """(image, classes that won each pixel, keypoints considered, poses drawn) of slot s of `source` through the
    getters, the given spans and the restatement"""
    sets, poses = _getter_sets(source, s, style.from_keyframe)
    filt = dict(drop_flags=style.filter.drop_flags, own_only=style.filter.own_only, min_inliers=style.filter.min_inliers)
    lines, n_poses = SR.slot_lines(source.get_trajectory(s), poses, source.pose(s), style.show, style.trajectory_rgb, style.keyframe_rgb,
                                   style.pose_rgb, (style.frustum_w, style.frustum_h, style.frustum_d), style.trajectory_tail)
    els = CR.elements(style.cols, style.rows, np.frombuffer(bytes(cam), F), sets, lines, spans, filt, style.point_size, cloud_size)
    low, covered = CR.depth_buffer(style.cols, style.rows, els)
    return CR.picture(style.cols, style.rows, style.pixel, low, covered, style.background), CR.classes(low, covered), sum(n for n, *_ in sets), n_poses


def _image(sc, i):
    got = sc.image(i)
    return got.cpu().numpy() if sc.device_mode else got


def _check_slot(tag, sc, i, s, source, cam, cloud, extra=None, run=0, vacuous_ok=False):
    """named slot i of the scene job (slot s) against the getters of `source` plus the records of named slot i of the
    cloud job `cloud` (None: no live layer) and the extra records"""
    seg, info = sc.segments[i], sc.cloud_info[i]
    live = None if cloud is None else cloud.organized(i)
    spans = ([] if extra is None else [extra]) + ([] if live is None else [live.reshape(-1)])
    want, cls, n_kps, n_poses = _restate(source, s, sc.style, cam, spans, DENSE["point_size"])
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, run, hip_lib.SCENE_OK), (tag, s)
    assert int(seg["frame_id"]) == source.stats(s).frame_id and int(seg["n_keyframes"]) == source.num_keyframes(s), (tag, s)
    assert (int(seg["from_keyframe"]), int(seg["n_keypoints"]), int(seg["n_poses"])) == (sc.style.from_keyframe, n_kps, n_poses), (tag, s)
    assert int(seg["offset"]) == i * sc.image_bytes and seg["pose"].tobytes() == source.pose(s).tobytes(), (tag, s)
    if live is None:
        assert (int(info["status"]), int(info["keyframe_id"]), int(info["live_points"])) == (hip_lib.CLOUD_NONE, -1, 0), (tag, s)
    else:
        cseg = cloud.segments[i]
        assert (int(info["status"]), int(info["keyframe_id"]), int(info["live_points"])) == \
            (hip_lib.CLOUD_OK, int(cseg["keyframe_id"]), int(cseg["n_points"])), (tag, s)
        assert int(cseg["n_points"]) == int(((live["flags"] & hip_lib.CLOUD_DROPPED) == 0).sum()) > 0, (tag, s)
    assert (int(info["extra_points"]), int(info["_pad"]), int(info["_pad2"])) == (0 if extra is None else len(extra), 0, 0), (tag, s)
    # not vacuous: the restatement alone says that cloud points and sparse elements both win pixels
    share = float((cls == CR.CLASS_CLOUD).mean())
    sparse = int(((cls >= 0) & (cls < CR.CLASS_CLOUD)).sum())
    print(f"{tag} slot {s}: class 4 wins {share:.3f} of the pixels, sparse elements win {sparse}")
    if not vacuous_ok:
        assert share >= MIN_CLOUD_SHARE and sparse >= 1, (tag, s, share, sparse)
    got = _image(sc, i)
    assert got.tobytes() == want.tobytes(), (tag, s, int((got != want).sum()))
    return want


def _style_ctx(pixel="rgb8"):
    return hip_lib.scene_style(cols=COLS, rows=ROWS, pixel=pixel, point_size=3)


@pytest.mark.parametrize("lr_check", (None, 1.0))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_ctx_live_layer(played, what, lr_check, monkeypatch):
    """5 slots in 2 groups, a camera behind each slot's pose; host and device mode; SVO_SCENE_CHUNK_SLOTS=1 gives the
    same bytes"""
    cams = [_behind(played.pose(s)) for s in range(5)]
    dense = dict(DENSE, what=what, lr_check=lr_check or 0.0)
    cloud = played.submit_cloud(what, None, step=DENSE["step"], layout="organized", lr_check=lr_check)
    host = played.submit_scenes(camera=cams, style=_style_ctx(), dense=dense)
    dev = played.submit_scenes(camera=cams, style=_style_ctx("rgba8"), dense=dense, device=True)
    played.wait()
    imgs = [_check_slot((what, lr_check, "host"), host, s, s, played, cams[s], cloud) for s in range(5)]
    for s in range(5):
        assert _image(dev, s)[:, :, :3].tobytes() == imgs[s].tobytes() and (_image(dev, s)[:, :, 3] == 255).all()
    for f in host.segments.dtype.names:                                             # (RGBA: only the images' offsets differ)
        assert f == "offset" or host.segments[f].tobytes() == dev.segments[f].tobytes(), f
    assert [int(o) for o in dev.segments["offset"]] == [s * dev.image_bytes for s in range(5)] and dev.cloud_info.tobytes() == host.cloud_info.tobytes()
    plain = played.export_scenes(camera=cams, style=_style_ctx())
    assert plain.segments.tobytes() == host.segments.tobytes() and plain.cloud_info is None
    assert all(plain.image(s).tobytes() != imgs[s].tobytes() for s in range(5))
    monkeypatch.setenv("SVO_SCENE_CHUNK_SLOTS", "1")
    monkeypatch.setenv("SVO_SCENE_TABLE_SPANS", "1")
    for device in (False, True):
        again = played.export_scenes(camera=cams, style=_style_ctx(), dense=dense, device=device)
        px = again.pixels.cpu().numpy() if device else again.pixels
        assert px[:host.capacity].tobytes() == host.pixels[:host.capacity].tobytes()
        assert again.segments.tobytes() == host.segments.tobytes() and again.cloud_info.tobytes() == host.cloud_info.tobytes()


def test_ctx_extra_span_alone_and_with_the_live_layer(played):
    """named slots [3, 0, 4] of both groups; slot 0 has no extra span; the extra records are a compact device cloud
    of another job"""
    named = [3, 0, 4]
    cams = [_behind(played.pose(s), 1.5) for s in named]
    comp = played.export_cloud("last_keyframes", named, step=8, layout="compact", device=True)
    per, extra_dev, extra = comp.points_per_slot, [], []
    for i in range(3):
        n = int(comp.segments[i]["n_points"]) if i != 1 else 0
        extra_dev.append((comp.points_buffer[i * per:].data_ptr(), n) if n else None)
        extra.append(comp.points(i)[:n] if n else None)
    assert all(e is None or len(e) > 100 for e in extra) and extra[1] is None
    alone = played.export_scenes(named, camera=cams, style=_style_ctx(), dense=dict(live=False, point_size=DENSE["point_size"]), clouds=extra_dev)
    for i, s in enumerate(named):
        _check_slot("extra", alone, i, s, played, cams[i], None, extra[i], vacuous_ok=i == 1)
    assert alone.image(1).tobytes() == played.export_scenes([0], camera=cams[1], style=_style_ctx()).image(0).tobytes()
    cloud = played.submit_cloud("frames", named, step=DENSE["step"], layout="organized")
    both = played.submit_scenes(named, camera=cams, style=_style_ctx(), dense=dict(DENSE, what="frames"), clouds=extra_dev, device=True)
    played.wait()
    for i, s in enumerate(named):
        _check_slot("both", both, i, s, played, cams[i], cloud, extra[i])
    assert both.image(0).cpu().numpy().tobytes() != alone.image(0).tobytes()


def _raw_submit(batch, seqs, n, style, clouds, cams, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_scenes_clouds(batch._ctx, arr, n, C.byref(style), None if clouds is None else C.byref(clouds),
                                                         cams, C.byref(dst), mem)


def test_ctx_without_clouds_is_the_scene_job(played, tiny):
    """clouds == NULL, and live == 0 with extra == NULL: the unchanged job's bytes and segments, and memory() stays; a
    job with clouds books exactly the header's sum"""
    cams = [_behind(played.pose(s)) for s in range(5)]
    plain = played.export_scenes(camera=cams, style=_style_ctx())
    before = played.memory().device_bytes
    info = np.zeros(5, hip_lib.SCENE_CLOUD_INFO_DTYPE)
    info.view(np.uint8)[:] = FILL
    nothing, keep = hip_lib.scene_clouds(live=False, point_size=4, info=info)
    for clouds in (None, nothing):
        sc = Scenes(played, None, plain.style, cams, False)
        sc.pixels[:] = FILL
        assert _raw_submit(played, None, 0, sc.style, clouds, sc._cams, sc._dst, hip_lib.MEM_HOST) == 0
        played.wait()
        for s in range(5):
            assert sc.image(s).tobytes() == plain.image(s).tobytes()
        assert sc.segments.tobytes() == plain.segments.tobytes()
        assert played.memory().device_bytes == before and (info.view(np.uint8) == FILL).all()
    bad, _ = hip_lib.scene_clouds(live=False, point_size=0)                             # (checked even when nothing is drawn)
    assert _raw_submit(played, None, 0, plain.style, bad, plain._cams, plain._dst, hip_lib.MEM_HOST) == INVALID
    # a fresh ctx that has run the cloud job and the plain scene job books, for its first job with clouds, the key
    # planes and the live records of its slots and nothing else
    cfg, seqs = tiny
    fresh = _batch(cfg, 2, 1)
    fresh.new_images(*_frame_set(2, {s: (seqs[s], 0) for s in range(2)}))
    cams = [_behind(fresh.pose(s)) for s in range(2)]
    fresh.export_cloud("frames", None, step=DENSE["step"], layout="organized", device=True, lr_check=1.0)
    fresh.export_scenes(camera=cams, style=_style_ctx(), device=True)
    before = fresh.memory().device_bytes
    sc = fresh.export_scenes(camera=cams, style=_style_ctx(), device=True, dense=dict(DENSE, lr_check=1.0))
    points = (cfg["width"] // DENSE["step"]) * (cfg["height"] // DENSE["step"])
    key_bytes = (8 * COLS * ROWS + 255) // 256 * 256
    assert fresh.memory().device_bytes - before == 2 * (key_bytes + 16 * points)
    assert [int(x) for x in sc.cloud_info["status"]] == [hip_lib.CLOUD_OK] * 2
    fresh.export_scenes([1], camera=cams[1], style=_style_ctx(), device=True, dense=dict(DENSE, lr_check=1.0), clouds=[None])
    assert fresh.memory().device_bytes - before == 2 * (key_bytes + 16 * points)
    fresh.close()


def test_an_empty_slot_and_a_restarted_one(tiny):
    """slots 1 and 2 are empty (SCENE_NONE: only the segment and the info are written); under LAST_KEYFRAMES a started
    slot always has a keyframe (its first frame makes one), so the empty slots are the ones without"""
    cfg, seqs = tiny
    batch = _batch(cfg, 4, 2)
    for t in range(8):                                                               # slot 1 never starts
        batch.new_images(*_frame_set(4, {s: (seqs[s], t) for s in (0, 2, 3)}))
    batch.restart([2, 3])
    for t in range(3):                                                               # slot 3 plays another sequence, slot 2 stays empty
        batch.new_images(*_frame_set(4, {0: (seqs[0], 8 + t), 3: (seqs[4], t)}))
    cams = [_behind(batch.pose(s) if batch.stats(s).frame_id >= 0 else np.zeros(6)) for s in range(4)]
    rec = torch.from_numpy(CR.records([[0, 0, 1.0]] * 3, [1, 2, 3]).view(np.uint8).copy()).cuda()
    for what in ("frames", "last_keyframes"):
        cloud = batch.submit_cloud(what, None, step=DENSE["step"], layout="organized")
        sc = Scenes(batch, None, _style_ctx(), cams, False, dict(DENSE, what=what), [None, rec, None, None])
        assert sc._clouds[0].live == 1 and sc._clouds[0].point_size == DENSE["point_size"]
        sc.pixels[:] = FILL
        sc.submit().wait()
        _check_slot("runs on", sc, 0, 0, batch, cams[0], cloud)
        _check_slot("restarted", sc, 3, 3, batch, cams[3], cloud, run=1)
        for s, run in ((1, 0), (2, 1)):
            seg, info = sc.segments[s], sc.cloud_info[s]
            assert (int(seg["seq"]), int(seg["run"]), int(seg["frame_id"]), int(seg["status"])) == (s, run, -1, hip_lib.SCENE_NONE)
            assert (int(info["status"]), int(info["keyframe_id"]), int(info["live_points"]), int(info["extra_points"])) == \
                (hip_lib.CLOUD_NONE, -1, 0, 3 if s == 1 else 0)
            assert int(cloud.segments[s]["status"]) == hip_lib.CLOUD_NONE and sc.image(s) is None
            assert (sc.pixels[s * sc.image_bytes:(s + 1) * sc.image_bytes] == FILL).all()
    batch.close()


def test_ordering_without_draining_and_no_side_effects(tiny):
    """frame set t, scene A, frame set t + 1, scene B, one wait: A shows the state at t, B at t + 1 (a twin ctx stopped
    at each, which never runs a scene job); afterwards both track the next frames to the same bits"""
    cfg, seqs = tiny
    n_slots, t = 5, 9
    sets = [_frame_set(n_slots, {s: (seqs[s], k) for s in range(n_slots)}) for k in range(t + 4)]
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(t):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
    cams = [_behind(twin.pose(s)) for s in range(n_slots)]
    packed = [batch.pack_images(*sets[k]) for k in (t, t + 1)]
    dense = dict(DENSE, what="frames", lr_check=1.0)
    batch.submit_packed(packed[0])
    a = batch.submit_scenes(camera=cams, style=_style_ctx(), dense=dense)
    batch.submit_packed(packed[1])
    b = batch.submit_scenes(camera=cams, style=_style_ctx(), dense=dense, device=True)
    batch.wait()
    for sc, k in ((a, t), (b, t + 1)):
        twin.new_images(*sets[k])
        cloud = twin.export_cloud("frames", None, step=DENSE["step"], layout="organized", lr_check=1.0)
        assert [int(x) for x in sc.segments["frame_id"]] == [k] * n_slots
        for s in range(n_slots):
            _check_slot(f"frame {k}", sc, s, s, twin, cams[s], cloud)
    assert any(a.image(s).tobytes() != b.image(s).cpu().numpy().tobytes() for s in range(n_slots))
    for k in (t + 2, t + 3):
        batch.new_images(*sets[k])
        twin.new_images(*sets[k])
        batch.export_scenes([4, 1], camera=cams[:2], style=_style_ctx(), dense=dense)
    for s in range(n_slots):
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes() and batch.num_keyframes(s) == twin.num_keyframes(s)
        x, y = batch.get_frame(s), twin.get_frame(s)
        assert (x.kps2d.tobytes(), x.kps3d.tobytes(), x.info.tobytes(), x.pose.tobytes()) == \
               (y.kps2d.tobytes(), y.kps3d.tobytes(), y.info.tobytes(), y.pose.tobytes())
    batch.close()
    twin.close()


def test_rejected_calls_queue_nothing(tiny):
    cfg, seqs = tiny
    n_slots = 4
    batch = _batch(cfg, n_slots, 2)
    for t in range(2):
        batch.new_images(*_frame_set(n_slots, {s: (seqs[s], t) for s in range(n_slots)}))
    st = _style_ctx()
    _, image_bytes = hip_lib.scene_size(st)
    seg = np.zeros(n_slots, hip_lib.SCENE_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = FILL
    info = np.zeros(n_slots, hip_lib.SCENE_CLOUD_INFO_DTYPE)
    info.view(np.uint8)[:] = FILL
    px = torch.full((n_slots * image_bytes + 16,), FILL, dtype=torch.uint8).pin_memory()
    front = hip_lib.scene_preset("front", COLS, ROWS)
    cams = (hip_lib.SceneCamera * n_slots)(*[front] * n_slots)
    dst = hip_lib.SceneDst(seg.ctypes.data, px.data_ptr(), n_slots * image_bytes)
    rec = torch.from_numpy(CR.records([[0, 0, 1.0]] * 4).view(np.uint8).copy()).cuda()
    keeps = []

    def clouds(extra=None, **kw):
        fields = {k: kw.pop(k) for k in list(kw) if k in ("live_raw", "what_raw", "frame", "layout", "reserved", "cloud_reserved", "check")}
        c, keep = hip_lib.scene_clouds(live=kw.pop("live", True), extra=extra, info=info, **dict(dict(step=8, lr_check=1.0), **kw))
        keeps.append(keep)
        if "live_raw" in fields: c.live = fields["live_raw"]
        if "what_raw" in fields: c.what = fields["what_raw"]
        if "frame" in fields: c.cloud.frame = fields["frame"]
        if "layout" in fields: c.cloud.layout = fields["layout"]
        if "reserved" in fields: c._reserved[2] = fields["reserved"]
        if "cloud_reserved" in fields: c.cloud._reserved[0] = fields["cloud_reserved"]
        if "check" in fields: c.check = fields["check"]
        return c

    p = rec.data_ptr()
    bad = [clouds(live_raw=2), clouds(live_raw=-1), clouds(what_raw=2), clouds(what_raw=-1), clouds(point_size=0), clouds(point_size=17),
           clouds(reserved=1), clouds(frame=hip_lib.CLOUD_CAMERA), clouds(layout=hip_lib.CLOUD_ORGANIZED), clouds(step=0), clouds(step=17),
           clouds(max_depth=-1.0), clouds(min_disparity=float("nan")), clouds(cloud_reserved=1),
           clouds(check=hip_lib.stereo_check(True, 0.0)), clouds(check=hip_lib.StereoCheck(2, 1.0)), clouds(check=hip_lib.stereo_check(False, -1.0)),
           clouds(live=False, point_size=0, extra=[rec] * 4), clouds(live=False, reserved=1, extra=[rec] * 4),
           clouds(live=False, extra=[rec, rec, (p, -1), rec]), clouds(live=False, extra=[rec, (0, 2), rec, rec]),
           clouds(live=False, extra=[rec, rec, rec, (p + 8, 1)]), clouds(extra=[(p + 4, 1), None, None, None])]
    for i, c in enumerate(bad):
        assert _raw_submit(batch, None, 0, st, c, cams, dst, hip_lib.MEM_HOST) == INVALID, i
        assert hip_lib.lib().svo_last_error()
    # what the scene job rejects is rejected with clouds too
    good = clouds()
    assert _raw_submit(batch, [0, 0], 2, st, good, cams, dst, hip_lib.MEM_HOST) == INVALID
    assert _raw_submit(batch, None, 0, st, good, cams, dst, 2) == INVALID
    assert _raw_submit(batch, None, 0, hip_lib.scene_style(cols=0), good, cams, dst, hip_lib.MEM_HOST) == INVALID
    small = hip_lib.SceneDst(seg.ctypes.data, px.data_ptr(), n_slots * image_bytes - 1)
    assert _raw_submit(batch, None, 0, st, good, cams, small, hip_lib.MEM_HOST) not in (0, INVALID)
    # (live == 0: cloud and check are not looked at)
    assert _raw_submit(batch, [1], 1, st, clouds(live=False, frame=7, check=hip_lib.StereoCheck(2, -1.0), extra=[rec]), cams, dst, hip_lib.MEM_HOST) == 0
    batch.wait()
    assert (seg.view(np.uint8).reshape(n_slots, -1)[1:] == FILL).all() and (px.numpy()[image_bytes:] == FILL).all()
    assert (info.view(np.uint8).reshape(n_slots, -1)[1:] == FILL).all() and int(info[0]["extra_points"]) == 4
    # nothing else was queued and the ctx goes on: the next frame and a scene of it
    batch.new_images(*_frame_set(n_slots, {s: (seqs[s], 2) for s in range(n_slots)}))
    cams = [_behind(batch.pose(s)) for s in range(n_slots)]
    cloud = batch.submit_cloud("frames", None, step=DENSE["step"], layout="organized")
    sc = batch.export_scenes(camera=cams, style=st, dense=dict(DENSE))
    assert [int(x) for x in sc.segments["frame_id"]] == [2] * n_slots
    _check_slot("after", sc, 1, 1, batch, cams[1], cloud)
    batch.close()
