"""The cross-check of SGM maps and the clouds of SGM maps on the GPU, bit for bit against the numpy statement
(tests/sgm_lr_ref.py over tests/sgm_ref.py, tests/lr_ref.py and tests/cloud_ref.py) on the crafted pairs of
tests/sgm_lr_cases.py, every destination surrounded by guards; and the jobs (svo_submit_export_disparity_sgm_checked,
svo_submit_export_cloud_sgm) against the stage entries run on the planes that a view job exports of the same slots. No
comparison has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cloud_ref as CR
import lr_ref as LR
import sgm_lr_cases as LC
import sgm_lr_ref as SLR
import test_cloud_gpu as CG
from stereo_svo_slam_amd import hip_lib
from test_dense_gpu import GUARD, WIN, _batch, _bits, _frames, _np, _planes_of, _style, _view, played, tiny   # noqa: F401 (played, tiny: fixtures)
from test_sgm_gpu import _collect, _guarded_floats

pytestmark = pytest.mark.gpu

F = np.float32
POINT = hip_lib.MAP_POINT_DTYPE
RIG = dict(fx=90.0, fy=91.0, cx=47.5, cy=20.25, baseline=0.12)
POSE = np.array([0.3, -0.2, 1.5, 0.05, -0.1, 0.02], F)
# value, cost, max_lr_diff: report only and tolerance 1, disparity and depth, with and without the cost plane
FORMS = ((0, 1, 0.0), (0, 1, 1.0), (1, 1, 1.0), (1, 0, 0.0), (0, 0, 1.0), (1, 0, 1.0))


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def _case(name, keep, offset=0, extra=0, baseline=20.0):
    left, right, win, sx, sy, step, p1, p2, cap = LC.cases()[name]
    pair = (_view(left, offset, extra, keep), _view(right, (offset * 2) % 4 if offset else 0, extra, keep), baseline)
    return pair, (step, win, sx, sy), hip_lib.sgm_params(p1, p2, cap)


def _checked(handle, pairs, style, sgm, check, gap=4):
    n_planes = 1 + style.cost + (1 if check is not None and check.lr else 0)
    shapes = [(n_planes, p[0][2] // style.step, p[0][1] // style.step) for p in pairs]
    offsets, dst = _guarded_floats(shapes, gap)
    handle.dense_disparity_sgm(pairs, offsets, style, sgm, dst, check)
    return _collect(dst, shapes, offsets)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", LC.GPU_CASES)
def test_checked_map_against_the_statement(H, name):
    """disparity and depth, with and without the cost plane, report only and tolerance 1; once more through views of
    stride width + 13 at odd bases, which the mirrored staging must read as well"""
    keep = []
    pair, (step, win, sx, sy), sgm = _case(name, keep)
    odd, _, _ = _case(name, keep, 3, 13)
    torch.cuda.synchronize()
    fwd, lr = LC.forward(name), LC.reference(name)
    for value, cost, diff in FORMS:
        got = _checked(H, [pair], hip_lib.DisparityStyle(value, step, win, sx, sy, cost), sgm, hip_lib.stereo_check(True, diff))[0]
        want = LR.checked_planes(fwd, lr, value, bool(cost), 20.0, diff)
        assert _same(got, want), (name, value, cost, diff, int((_bits(got) != _bits(want)).sum()))
    got = _checked(H, [odd], hip_lib.DisparityStyle(0, step, win, sx, sy, 1), sgm, hip_lib.stereo_check(True, 1.0))[0]
    assert _same(got, LR.checked_planes(fwd, lr, 0, True, 20.0, 1.0)), (name, "odd views")
    if name == "occl3s4":                                  # the clamp case aside, the purpose on the GPU's own planes
        assert LR.fails(got[2], 1.0).mean() > 0.05
    sgm.subpixel = 0
    got = _checked(H, [pair], hip_lib.DisparityStyle(0, step, win, sx, sy, 1), sgm, hip_lib.stereo_check(True, 1.0))[0]
    assert _same(got, LR.checked_planes(LC.forward(name, False), LC.reference(name, False), 0, True, 20.0, 1.0)), (name, "whole disparities")


@functools.lru_cache(maxsize=None)
def _two_sizes():
    """the occlusion scene and the images of b (96 x 40 and 97 x 53) under the scene's settings at step 2"""
    left, right = LC.cases()["b"][:2]
    scene = LC.cases()["occl4s2"]
    args = (*LC.SETTINGS, 2, *LC.PENALTIES)
    fwd = SLR.disparity(left, right, *args, fast=True)
    lr = SLR.lr_plane_fast(fwd[0], SLR.reverse(left, right, *args, fast=True), left.shape[1], 2)
    return [(scene[0], scene[1], LC.forward("occl4s2"), LC.reference("occl4s2")), (left, right, fwd, lr)]


def test_two_sizes_in_one_call_and_one_pair_per_chunk(H, monkeypatch):
    keep = []
    cases = _two_sizes()
    pairs = [(_view(c[0], 0, 0, keep), _view(c[1], 0, 0, keep), 20.0 + i) for i, c in enumerate(cases)]
    torch.cuda.synchronize()
    sgm = hip_lib.sgm_params(*LC.PENALTIES)
    for chunk in (None, "1"):
        if chunk:
            monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", chunk)
        for order, (value, cost, diff) in (((0, 1), (0, 1, 1.0)), ((1, 0), (1, 0, 1.0))):
            got = _checked(H, [pairs[i] for i in order], hip_lib.DisparityStyle(value, 2, *LC.SETTINGS, cost), sgm,
                           hip_lib.stereo_check(True, diff), gap=8)
            for g, i in zip(got, order):
                assert _same(g, LR.checked_planes(cases[i][2], cases[i][3], value, bool(cost), 20.0 + i, diff)), (chunk, order, i)


def test_no_check_is_the_unchecked_entry(H):
    """check = NULL and lr = 0 give the bytes of svo_dense_disparity_sgm; a depth point that does not fail has its bits"""
    keep = []
    pair, (step, win, sx, sy), sgm = _case("occl3s4", keep)
    torch.cuda.synchronize()
    for value in (0, 1):
        style = hip_lib.DisparityStyle(value, step, win, sx, sy, 1)
        plain = _checked(H, [pair], style, sgm, None)[0]
        off = hip_lib.stereo_check(False, 1.0)
        shapes = [plain.shape]
        offsets, dst = _guarded_floats(shapes, 4)
        packed = H.pack_dense([pair], offsets)
        lib = hip_lib.lib()
        for check in (None, C.byref(off)):
            dst.fill_(float(GUARD))
            assert lib.svo_dense_disparity_sgm_checked(H._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(sgm), check,
                                                       C.c_void_p(dst.data_ptr())) == 0
            assert _same(_collect(dst, shapes, offsets)[0], plain)
        checked = _checked(H, [pair], style, sgm, hip_lib.stereo_check(True, 1.0))[0]
        kept = ~LR.fails(checked[2], 1.0)
        assert kept.any() and (~kept).any()
        assert np.array_equal(_bits(checked[0][kept]), _bits(plain[0][kept])) and np.array_equal(_bits(checked[1]), _bits(plain[1]))
        assert (checked[0][~kept] == (0.0 if value else -1.0)).all()


def _cloud(handle, srcs, style, sgm, check, with_counts=True, gap=3):
    """CG._run over svo_cloud_points_sgm"""
    first, sizes, at = [], [], gap
    for left, _, _, _ in srcs:
        n = (left[1] // style.step) * (left[2] // style.step)
        first.append(at)
        sizes.append(n)
        at += n + gap
    dst = torch.full((at, 16), CG.GUARD, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(srcs) + 2,), -7, dtype=torch.int32, device="cuda") if with_counts else None
    handle.cloud_points_sgm(srcs, first, style, sgm, dst, None if counts is None else counts[1:], check)
    got = dst.cpu().numpy()
    outside = np.ones(at, bool)
    out = []
    if counts is not None:
        counts = counts.cpu().numpy()
        assert counts[0] == -7 and counts[-1] == -7
    for i, (lo, n) in enumerate(zip(first, sizes)):
        out.append((got[lo:lo + n].copy().view(POINT)[:, 0], None if counts is None else int(counts[1 + i])))
        outside[lo:lo + n] = False
    assert (got[outside] == CG.GUARD).all(), "a guard record changed"
    return out


@pytest.mark.parametrize("checked", (False, True))
@pytest.mark.parametrize("frame", sorted(CG.FRAMES))
@pytest.mark.parametrize("layout", sorted(CG.LAYOUTS))
def test_cloud_of_sgm_planes_against_the_statement(H, layout, frame, checked, monkeypatch):
    """two sizes in one call (and one image per table), the three filters on: cloud_ref's triangulation and layouts fed
    with the SGM planes, masked by the check where there is one, and max_mean_cost as best > max_mean_cost * 4"""
    keep = []
    cases = _two_sizes()
    srcs = [(_view(c[0], 0, 0, keep), _view(c[1], 0, 0, keep), dict(RIG, baseline=0.12 + 0.01 * i), POSE) for i, c in enumerate(cases)]
    torch.cuda.synchronize()
    bound = float(np.median(cases[0][2][1])) / 4.0
    filt = dict(min_disparity=2.0, max_depth=0.05, max_mean_cost=bound)
    style = hip_lib.cloud_style(2, *LC.SETTINGS, CG.FRAMES[frame], CG.LAYOUTS[layout], **filt)
    check = hip_lib.stereo_check(True, 1.0) if checked else None
    wants = []
    for i, (left, right, fwd, lr) in enumerate(cases):
        planes = SLR.masked(fwd, lr, 1.0) if checked else fwd
        wants.append(SLR.cloud(left, planes, 2, dict(RIG, baseline=0.12 + 0.01 * i), POSE, CG.FRAMES[frame], CG.LAYOUTS[layout], **filt))
        valid = int((planes[0] >= 0).sum())
        assert 0 < wants[-1][1] < valid                     # the filters keep some and drop some
        by_cost = SLR.kept_mask(planes, np.zeros_like(planes[0]), max_mean_cost=bound)
        assert 0 < int(by_cost.sum()) < valid               # and so does max_mean_cost alone
    sgm = hip_lib.sgm_params(*LC.PENALTIES)
    for table in (None, "1"):
        if table:
            monkeypatch.setenv("SVO_CLOUD_TABLE_IMAGES", table)
        for got, want, i in zip(_cloud(H, srcs, style, sgm, check, with_counts=table is None), wants, range(2)):
            CG._check(got, want, CG.LAYOUTS[layout], (layout, frame, checked, table, i))
    if checked:                                            # (the check masks points that the search found)
        assert int((SLR.masked(cases[0][2], cases[0][3], 1.0)[0] < 0).sum()) > int((cases[0][2][0] < 0).sum())


def _set(obj, **kw):
    for k, v in kw.items():
        if k == "reserved":
            obj._reserved[v] = 1
        else:
            setattr(obj, k, v)
    return obj


def _bad_params():
    p = lambda **kw: _set(hip_lib.sgm_params(*LC.PENALTIES), **kw)
    return [p(paths=8), p(p1=0), p(p2=1), p(cost_cap=0), p(subpixel=2), p(cost_cap=16128), p(reserved=0), p(reserved=2), None]


def _bad_checks(cloud):
    c = lambda lr=1, diff=1.0, **kw: _set(hip_lib.StereoCheck(lr, diff), **kw)
    bad = [c(lr=2), c(lr=-1), c(diff=-1.0), c(diff=float("nan")), c(diff=float("inf")), c(reserved=0), c(reserved=5), c(lr=0, diff=-1.0), c(lr=0, reserved=3)]
    return bad + ([c(diff=0.0)] if cloud else [])


def test_stage_entries_reject(H):
    """what the SGM entry rejects and what the cross-check rejects of a check, together; nothing is written"""
    keep = []
    pair, (step, win, sx, sy), sgm = _case("occl3s4", keep)
    lib = hip_lib.lib()
    dst = torch.full((4096,), float(GUARD), dtype=torch.float32, device="cuda")
    rec = torch.full((512, 16), CG.GUARD, dtype=torch.uint8, device="cuda")
    style, cstyle = hip_lib.DisparityStyle(0, step, win, sx, sy, 1), hip_lib.cloud_style(step, win, sx, sy)
    good = hip_lib.stereo_check(True, 1.0)
    packed = H.pack_dense([pair], [0])
    cpacked = H.pack_cloud([(pair[0], pair[1], RIG, POSE)], [0])

    def dense(style=style, sgm=sgm, check=good):
        return lib.svo_dense_disparity_sgm_checked(H._h, packed[0], packed[1], packed[2], C.byref(style), None if sgm is None else C.byref(sgm),
                                                   None if check is None else C.byref(check), C.c_void_p(dst.data_ptr()))

    def cloud(style=cstyle, sgm=sgm, check=good):
        return lib.svo_cloud_points_sgm(H._h, cpacked[0], cpacked[1], cpacked[2], C.byref(style), None if sgm is None else C.byref(sgm),
                                        None if check is None else C.byref(check), C.c_void_p(rec.data_ptr()), None)

    for p in _bad_params():
        assert dense(sgm=p) == -1 and b"svo_dense_disparity_sgm_checked" in lib.svo_last_error()
        assert cloud(sgm=p) == -1 and b"svo_cloud_points_sgm" in lib.svo_last_error()
        assert cloud(sgm=p, check=None) == -1
    for c in _bad_checks(False):
        assert dense(check=c) == -1, (c.lr, c.max_lr_diff)
    for c in _bad_checks(True):
        assert cloud(check=c) == -1, (c.lr, c.max_lr_diff)
    assert dense(style=hip_lib.DisparityStyle(0, step, win, 64, sy, 1)) == -1
    assert dense(style=hip_lib.DisparityStyle(2, step, win, sx, sy, 1)) == -1
    assert cloud(style=hip_lib.cloud_style(step, win, 64, sy)) == -1
    assert cloud(style=hip_lib.cloud_style(step, 36, sx, sy)) == -1
    torch.cuda.synchronize()
    assert (_bits(dst) == _bits(np.full(1, GUARD))[0]).all() and (rec.cpu().numpy() == CG.GUARD).all()
    assert dense() == 0 and cloud() == 0 and cloud(check=None) == 0       # the handle carries on
    want = LR.checked_planes(LC.forward("occl3s4"), LC.reference("occl3s4"), 0, True, 20.0, 1.0)
    assert _same(dst.cpu().numpy()[:want.size].reshape(want.shape), want)


# ------------------------------------------------------------------ the jobs
SGM = dict(p1=32, p2=256, cost_cap=4095)


def _stage_planes(handle, left, right, style, sgm, check, baseline):
    keep = []
    pair = (_view(np.ascontiguousarray(left), 0, 0, keep), _view(np.ascontiguousarray(right), 0, 0, keep), float(baseline))
    torch.cuda.synchronize()
    return _checked(handle, [pair], style, sgm, check)[0]


@pytest.mark.parametrize("device", (False, True))
def test_jobs_against_the_stage_entries_on_their_views(H, played, device, monkeypatch):
    """5 slots in 2 groups; slot 3 has its rig's baseline; slot 4 is empty. The checked SGM disparity job (depth, cost,
    tolerance 1; then report only, named out of order, one slot per chunk) and the SGM cloud job (checked and not)"""
    what = "frames"
    views = {s: _planes_of(played, what, s) for s in range(4)}
    job = played.submit_disparity(what, None, value="depth", step=7, cost=True, device=device, sgm=dict(SGM, lr_check=1.0), **WIN)
    job.wait()
    job._buf.fill_(float(GUARD))
    job.submit().wait()
    assert job.n_planes == 3 and (job.cols, job.rows, job.n_planes, job.image_bytes) == played.disparity_size(job.style, job.check)
    for s in range(4):
        left, right, vseg = views[s]
        cam = played.slot_rig(s)[1]
        want = _stage_planes(H, left, right, job.style, job.sgm, job.check, cam.baseline)
        got = _np(job.planes(s))
        assert _same(got, want), (s, int((_bits(got) != _bits(want)).sum()))
        assert np.array_equal(_bits(_np(job.lr(s))), _bits(want[2])) and (want[2] >= 0).any() and LR.fails(want[2], 1.0).any()
        seg = job.segments[s]
        assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"])) == (s, hip_lib.DISPARITY_OK, int(vseg["frame_id"]))
        assert int(seg["offset"]) == s * job.image_bytes and F(seg["baseline"]) == F(cam.baseline)
    assert job.planes(4) is None and job.lr(4) is None and int(job.segments[4]["status"]) == hip_lib.DISPARITY_NONE
    flat, guard = _bits(job._buf), _bits(np.full(1, GUARD))[0]
    used = job.n_planes * job.rows * job.cols
    assert (flat[4 * job.image_bytes // 4:] == guard).all()
    assert all((flat[s * job.image_bytes // 4 + used:(s + 1) * job.image_bytes // 4] == guard).all() for s in range(4))
    monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", "1")
    named = played.export_disparity(what, [3, 0, 4, 2], step=4, device=device, sgm=dict(SGM, subpixel=False, lr_check=True), **WIN)
    assert named.n_planes == 2 and int(named.segments[2]["status"]) == hip_lib.DISPARITY_NONE
    for i, s in ((0, 3), (1, 0), (3, 2)):
        want = _stage_planes(H, views[s][0], views[s][1], named.style, named.sgm, named.check, played.slot_rig(s)[1].baseline)
        assert _same(_np(named.planes(i)), want), ("named", s)
    monkeypatch.delenv("SVO_SGM_CHUNK_SLOTS")
    # clouds: the stage entry on the same planes, with the segment's pose and the slot's rig
    filt = dict(min_disparity=3.5, max_depth=0.0, max_mean_cost=1000.0)   # (a bound on S / 4: the mean over the paths)
    for layout, frame, lr_check, chunk in (("compact", "world", 1.0, None), ("organized", "camera", None, None), ("compact", "world", 1.0, "1")):
        if chunk:
            monkeypatch.setenv("SVO_CLOUD_CHUNK_SLOTS", chunk)
            monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", chunk)
        cjob = played.submit_cloud(what, [2, 3, 4, 0], step=8, frame=frame, layout=layout, device=device, sgm=dict(SGM, lr_check=lr_check), **WIN, **filt)
        cjob.wait()
        cjob.points_buffer.fill_(CG.GUARD)
        cjob.submit().wait()
        for i, s in ((0, 2), (1, 3), (3, 0)):
            keep = []
            cam = played.slot_rig(s)[1]
            seg = cjob.segments[i]
            src = (_view(np.ascontiguousarray(views[s][0]), 0, 0, keep), _view(np.ascontiguousarray(views[s][1]), 0, 0, keep),
                   {k: getattr(cam, k) for k in CR.RIG_KEYS}, seg["pose"])
            torch.cuda.synchronize()
            rec, n = _cloud(H, [src], cjob.style, cjob.sgm, cjob.check)[0]
            per = cjob.points_per_slot
            raw = _np(cjob.points_buffer[i * per:(i + 1) * per]).view(POINT)[:, 0]
            assert (int(seg["status"]), int(seg["n_points"]), int(seg["first_point"])) == (hip_lib.CLOUD_OK, n, i * per), (layout, s)
            assert 0 < n <= per
            m = per if layout == "organized" else n
            assert raw[:m].tobytes() == rec[:m].tobytes(), (layout, frame, s)
            assert (raw[m:].view(np.uint8) == CG.GUARD).all()
        assert int(cjob.segments[2]["status"]) == hip_lib.CLOUD_NONE and int(cjob.segments[2]["n_points"]) == 0
        assert (_np(cjob.points_buffer[2 * cjob.points_per_slot:3 * cjob.points_per_slot]) == CG.GUARD).all()


def _up(v):
    return (v + 255) // 256 * 256


def _sgm_slot(cols, rows, D, checked):
    one = 2 * _up(cols * rows * D * 2) + _up(cols * rows * 2)
    return 2 * one + _up(cols * rows * 4) if checked else one


def test_jobs_reject_memory_and_no_side_effects(tiny):
    """rejected calls return -1 and queue nothing; the memory grows by the stated block and not again; an unchecked SGM
    job, a checked winner-takes-all job and a plain job give the bytes of a twin ctx that ran none of this"""
    cfg, seqs = tiny
    n_slots = 4
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(2):
        batch.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
        twin.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
    lib = hip_lib.lib()
    st = _style(0, 4, 7, 9, 2, 1)
    good = hip_lib.stereo_check(True, 1.0)
    cols, rows, planes, image_bytes = batch.disparity_size(st, good)
    assert planes == 3
    seg = np.zeros(n_slots, hip_lib.DISPARITY_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = 0xA5
    dpx = torch.full((n_slots * image_bytes // 4 + 8,), float(GUARD), dtype=torch.float32, device="cuda")
    dst = hip_lib.DisparityDst(seg.ctypes.data, dpx.data_ptr(), n_slots * image_bytes)
    cst = hip_lib.cloud_style(4, 7, 9, 2)
    per_slot = batch.cloud_size(cst)[2]
    cseg = np.zeros(n_slots, hip_lib.CLOUD_SEGMENT_DTYPE)
    cseg.view(np.uint8)[:] = 0xA5
    rec = torch.full((n_slots * per_slot, 16), CG.GUARD, dtype=torch.uint8, device="cuda")
    cdst = hip_lib.CloudDst(cseg.ctypes.data, rec.data_ptr(), n_slots * per_slot)
    params = hip_lib.sgm_params(32, 256, 4095)

    def disparity(style=st, sgm=params, check=good, dst=dst, what=0, mem=1):
        return lib.svo_submit_export_disparity_sgm_checked(batch._ctx, what, None, 0, C.byref(style), None if sgm is None else C.byref(sgm),
                                                           None if check is None else C.byref(check), C.byref(dst), mem)

    def cloud(style=cst, sgm=params, check=good, dst=cdst, what=0, mem=1):
        return lib.svo_submit_export_cloud_sgm(batch._ctx, what, None, 0, C.byref(style), None if sgm is None else C.byref(sgm),
                                               None if check is None else C.byref(check), C.byref(dst), mem)

    for p in _bad_params():
        assert disparity(sgm=p) == -1 and cloud(sgm=p) == -1 and cloud(sgm=p, check=None) == -1
        assert lib.svo_last_error()
    for c in _bad_checks(False):
        assert disparity(check=c) == -1, (c.lr, c.max_lr_diff)
    for c in _bad_checks(True):
        assert cloud(check=c) == -1, (c.lr, c.max_lr_diff)
    assert disparity(style=_style(0, 4, 7, 64, 2, 1)) == -1 and cloud(style=hip_lib.cloud_style(4, 7, 64, 2)) == -1    # search_x = 64
    assert disparity(style=_style(0, 4, 36, 9, 2, 1)) == -1 and cloud(style=hip_lib.cloud_style(4, 36, 9, 2)) == -1    # what the plain jobs reject
    assert disparity(what=2) == -1 and cloud(what=2) == -1 and disparity(mem=2) == -1 and cloud(mem=2) == -1
    assert cloud(style=hip_lib.cloud_style(4, 7, 9, 2, 2, 0)) == -1
    unchecked_bytes = batch.disparity_size(st)[3]
    assert unchecked_bytes < image_bytes                   # the shape is that of svo_disparity_size_checked
    assert disparity(dst=hip_lib.DisparityDst(seg.ctypes.data, dpx.data_ptr(), n_slots * image_bytes - 1)) == -4
    assert cloud(dst=hip_lib.CloudDst(cseg.ctypes.data, rec.data_ptr(), n_slots * per_slot - 1)) == -4
    for make in (batch.submit_disparity, batch.submit_cloud):
        with pytest.raises(ValueError, match="sgm dict"):
            make("frames", None, step=4, lr_check=1.0, sgm=SGM, **WIN)
    batch.wait()
    assert (seg.view(np.uint8) == 0xA5).all() and (cseg.view(np.uint8) == 0xA5).all()
    assert (_bits(dpx) == _bits(np.full(1, GUARD))[0]).all() and (rec.cpu().numpy() == CG.GUARD).all()
    # the ctx carries on; the jobs that exist already, before
    kw = dict(step=4, cost=True, device=True, **WIN)
    first = [batch.export_disparity("frames", None, **kw), batch.export_disparity("frames", None, lr_check=1.0, **kw),
             batch.export_disparity("frames", None, sgm=SGM, **dict(kw, step=8))]
    first_cloud = batch.export_cloud("frames", None, step=4, device=True, lr_check=1.0, **WIN)
    before = batch.memory().device_bytes
    D = 10
    small = _sgm_slot(cols // 2, rows // 2, D, False)      # the unchecked job at step 8: per group the block of its two slots
    job = batch.export_disparity("frames", None, sgm=dict(SGM, lr_check=1.0), **kw)
    grown = batch.memory().device_bytes - before
    assert grown == n_slots * (_sgm_slot(cols, rows, D, True) - small), (grown, _sgm_slot(cols, rows, D, True), small)
    batch.export_disparity("frames", None, sgm=dict(SGM, lr_check=1.0), **kw)
    batch.export_disparity("frames", [1], sgm=dict(SGM, lr_check=True), **dict(kw, step=8))
    batch.export_disparity("frames", None, sgm=SGM, **kw)
    assert batch.memory().device_bytes - before == grown                         # not again on a second, a smaller or an unchecked job
    cjob = batch.export_cloud("frames", None, step=4, device=True, sgm=dict(SGM, lr_check=1.0), **WIN)
    batch.export_cloud("frames", None, step=4, device=True, sgm=SGM, **WIN)
    assert batch.memory().device_bytes - before == grown                         # a cloud job: the cloud job's block (there already) and this one
    assert all(int(s["n_points"]) > 0 for s in cjob.segments)
    assert LR.fails(_np(job.lr(1)), 1.0).any() and (_np(job.lr(1)) >= 0).any()
    # after, and in a twin that ran none of the new jobs
    again = [batch.export_disparity("frames", None, **kw), batch.export_disparity("frames", None, lr_check=1.0, **kw),
             batch.export_disparity("frames", None, sgm=SGM, **dict(kw, step=8))]
    again_cloud = batch.export_cloud("frames", None, step=4, device=True, lr_check=1.0, **WIN)
    other = [twin.export_disparity("frames", None, **kw), twin.export_disparity("frames", None, lr_check=1.0, **kw),
             twin.export_disparity("frames", None, sgm=SGM, **dict(kw, step=8))]
    other_cloud = twin.export_cloud("frames", None, step=4, device=True, lr_check=1.0, **WIN)
    for a, b, c in zip(first, again, other):
        assert _np(a.values).tobytes() == _np(b.values).tobytes() == _np(c.values).tobytes()
        assert a.segments.tobytes() == b.segments.tobytes() == c.segments.tobytes()
    assert _np(first_cloud.points_buffer).tobytes() == _np(again_cloud.points_buffer).tobytes() == _np(other_cloud.points_buffer).tobytes()
    assert twin.memory().device_bytes == before
    batch.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    twin.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    for s in range(n_slots):
        assert batch.pose(s).tobytes() == twin.pose(s).tobytes() and batch.stats(s).frame_id == 2
    batch.close(); twin.close()
