"""Semi-global aggregation on the GPU, bit for bit against the numpy statement (tests/sgm_ref.py): the stage entries
(svo_sgm_aggregate, svo_dense_cost_volume, svo_dense_disparity_sgm) on the crafted inputs of tests/sgm_cases.py, every
destination surrounded by guards; and the job (svo_submit_export_disparity_sgm) against the statement run on the
planes that a view job exports of the same slots. No comparison has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import sgm_cases as SC
import sgm_ref as SR
from stereo_svo_slam_amd import hip_lib
from test_dense_gpu import GUARD, _bits, _style, _view

pytestmark = pytest.mark.gpu

F = np.float32
GUARD16 = np.uint16(0xABCD)                        # what a volume destination holds where nothing may be written


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _guarded_floats(shapes, gap):
    """offsets (bytes) of planes of `shapes` in a destination of GUARD floats with `gap` guard floats around each"""
    offsets, at = [], gap
    for shape in shapes:
        offsets.append(at * 4)
        at = (at + int(np.prod(shape)) + 3) // 4 * 4 + gap
    return offsets, torch.full((at,), float(GUARD), dtype=torch.float32, device="cuda")


def _collect(dst, shapes, offsets):
    got = dst.cpu().numpy()
    written = np.zeros(got.size, bool)
    out = []
    for shape, off in zip(shapes, offsets):
        n = int(np.prod(shape))
        out.append(got[off // 4:off // 4 + n].reshape(shape).copy())
        written[off // 4:off // 4 + n] = True
    assert (_bits(got[~written]) == _bits(np.full(1, GUARD))[0]).all(), "a guard float changed"
    return out


def _aggregate(handle, names, value, cost, subpixel, counts=True, gap=4, baselines=None, params=None):
    """the volumes `names` in one call; returns [planes [1 + cost, rows, cols]] and checks the guards. params: (p1,
    p2, cost_cap) of the call (None: those of the first volume)"""
    vols = [SC.volumes()[n] for n in names]
    p1, p2, cap = params or vols[0][2:]
    shapes = [(1 + cost, v[0].shape[0], v[0].shape[1]) for v in vols]
    offsets, dst = _guarded_floats(shapes, gap)
    keep = [_dev16(v[0]) for v in vols]
    cnts = [_dev16(v[1]) for v in vols] if counts else None
    base = baselines or [1.0] * len(vols)
    torch.cuda.synchronize()
    handle.sgm_aggregate([(v[0].shape[1], v[0].shape[0], v[0].shape[2], b) for v, b in zip(vols, base)], keep, cnts, value, cost,
                         hip_lib.sgm_params(p1, p2, cap, subpixel), offsets, dst)
    return _collect(dst, shapes, offsets)


@pytest.mark.parametrize("name", sorted(SC.volumes()))
def test_aggregate_random_volumes(H, name):
    """every shape with and without a count plane, both values of subpixel, disparity and depth, cost plane on and off"""
    for counts in (True, False):
        for subpixel in (True, False):
            for value, baseline in ((hip_lib.DENSE_DISPARITY, 1.0), (hip_lib.DENSE_DEPTH, 17.5)):
                want = SC.volume_reference(name, subpixel, value, baseline, counts)
                for cost in (1, 0):
                    got = _aggregate(H, [name], value, cost, subpixel, counts, baselines=[baseline])[0]
                    assert got.shape[0] == 1 + cost
                    assert np.array_equal(_bits(got), _bits(want[:1 + cost])), (name, counts, subpixel, value, cost)


def test_aggregate_several_shapes_in_one_call_and_chunked(H, monkeypatch):
    """the shapes that share 1 / 2 as p1 / p2 go together, and the two of 64 candidates with 9x9x33's params; then the
    same with one and two volumes per chunk"""
    groups = (("tie", "5x7x3", "1x1x1"), ("9x9x33", "3x70x64", "70x3x64"))
    for chunk in (None, "1", "2"):
        if chunk:
            monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", chunk)
        for names in groups:
            _, _, p1, p2, cap = SC.volumes()[names[0]]
            for order in ((0, 1, 2), (2, 0, 1)):
                picked = [names[i] for i in order]
                got = _aggregate(H, picked, hip_lib.DENSE_DISPARITY, 1, True, gap=8, params=(p1, p2, cap))
                for g, n in zip(got, picked):
                    C_, count, _, _, _ = SC.volumes()[n]
                    want = SR.aggregate(C_, count, p1, p2, cap, True) if n != names[0] else SC.volume_reference(n)
                    assert np.array_equal(_bits(g), _bits(want)), (chunk, picked, n)


def _pair_views(name, keep, offset=0, extra=0, baseline=20.0):
    left, right, win, sx, sy, step, p1, p2, cap = SC.pairs()[name]
    return ((_view(left, offset, extra, keep), _view(right, (offset * 2) % 4 if offset else 0, extra, keep), baseline),
            _style(0, step, win, sx, sy), hip_lib.sgm_params(p1, p2, cap))


def _cost_volume(handle, name, pair, style, gap=6):
    """the volume and count plane of a pair into a destination of GUARD16 words, guards before, between and after"""
    C_, count = SC.pair_volume(name)
    left, right, win, sx, sy, step, p1, p2, cap = SC.pairs()[name]
    vol_at, cnt_at = gap, gap + C_.size + gap
    total = cnt_at + count.size + gap
    dst = torch.from_numpy(np.full(total, GUARD16, np.uint16).view(np.int16)).cuda()
    torch.cuda.synchronize()
    handle.dense_cost_volume([pair], style, cap, [vol_at * 2], [cnt_at * 2], dst)
    got = dst.cpu().numpy().view(np.uint16)
    written = np.zeros(total, bool)
    written[vol_at:vol_at + C_.size] = True
    written[cnt_at:cnt_at + count.size] = True
    assert (got[~written] == GUARD16).all(), "a guard word changed"
    return got[vol_at:vol_at + C_.size].reshape(C_.shape), got[cnt_at:cnt_at + count.size].reshape(count.shape)


@pytest.mark.parametrize("band", ("half", "full"))
@pytest.mark.parametrize("name", sorted(SC.pairs()))
def test_cost_volume_against_statement(H, name, band, monkeypatch):
    """byte for byte, in both bands, plain and through views of stride width + 13 at bases 1 .. 3 bytes past a dword"""
    monkeypatch.setenv("SVO_DENSE_FEW_WORKGROUPS", "0" if band == "full" else "1000000")
    C_, count = SC.pair_volume(name)
    for offset, extra in ((0, 0), (1, 13), (2, 13), (3, 13)):
        keep = []
        pair, style, _ = _pair_views(name, keep, offset, extra)
        got_c, got_n = _cost_volume(H, name, pair, style)
        assert np.array_equal(got_n, count), (name, offset, "count")
        assert np.array_equal(got_c, C_), (name, offset, int((got_c != C_).sum()))


def _disparity_sgm(handle, pairs, style, sgm, gap=4):
    shapes = [(1 + style.cost, p[0][2] // style.step, p[0][1] // style.step) for p in pairs]
    offsets, dst = _guarded_floats(shapes, gap)
    handle.dense_disparity_sgm(pairs, offsets, style, sgm, dst)
    return _collect(dst, shapes, offsets)


@pytest.mark.parametrize("name", sorted(SC.pairs()))
def test_dense_disparity_sgm_against_statement(H, name):
    keep = []
    pair, style, sgm = _pair_views(name, keep, 3, 13)
    torch.cuda.synchronize()
    got = _disparity_sgm(H, [pair], style, sgm)[0]
    assert np.array_equal(_bits(got), _bits(SC.pair_reference(name))), name
    sgm.subpixel = 0
    assert np.array_equal(_bits(_disparity_sgm(H, [pair], style, sgm)[0]), _bits(SC.pair_reference(name, False))), name
    sgm.subpixel, style.value, style.cost = 1, hip_lib.DENSE_DEPTH, 0      # one plane: nothing behind it is written
    one = _disparity_sgm(H, [pair], style, sgm)[0]
    assert one.shape[0] == 1 and np.array_equal(_bits(one[0]), _bits(SC.pair_reference(name, True, SR.DEPTH, 20.0)[0])), name


def test_dense_disparity_sgm_flat_band_purpose(H):
    """the purpose on the GPU's own planes: winner takes all is right at no more than half of the band's points, SGM at
    no fewer than 0.95 of them"""
    keep = []
    pair, style, sgm = _pair_views("band", keep)
    torch.cuda.synchronize()
    shapes = [(2, 40, 96)]
    offsets, dst = _guarded_floats(shapes, 4)
    H.dense_disparity([pair], offsets, style, dst)
    wta = _collect(dst, shapes, offsets)[0][0]
    got = _disparity_sgm(H, [pair], style, sgm)[0][0]
    assert SC.band_score(wta) <= 0.5 and SC.band_score(got) >= 0.95, (SC.band_score(wta), SC.band_score(got))


def test_dense_disparity_sgm_three_sizes_in_one_call_and_chunked(H, monkeypatch):
    """the images of band, b and f (96x40, 97x53, 64x20) under band's settings in one call, in two orders; then the same
    with one and two pairs per chunk (and the full band)"""
    keep = []
    P = SC.pairs()
    imgs = [P[n][:2] for n in ("band", "b", "f")]
    pairs = [(_view(l, 0, 0, keep), _view(r, 0, 0, keep), 20.0 + i) for i, (l, r) in enumerate(imgs)]
    torch.cuda.synchronize()
    want = [SC.pair_reference("band")] + [SR.planes_fast(l, r, 7, 15, 1, 1, 32, 256, 4095) for l, r in imgs[1:]]
    for chunk in (None, "1", "2"):
        if chunk:
            monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", chunk)
            monkeypatch.setenv("SVO_DENSE_FEW_WORKGROUPS", "0")
        for order in ((0, 1, 2), (2, 0, 1)):
            got = _disparity_sgm(H, [pairs[i] for i in order], _style(0, 1, 7, 15, 1), hip_lib.sgm_params(32, 256, 4095), gap=8)
            for g, i in zip(got, order):
                assert np.array_equal(_bits(g), _bits(want[i])), (chunk, order, i)


def test_stage_entries_reject(H):
    """SVO_ERR_INVALID for each bad field of svo_sgm_params, the 16-bit bound, search_x = 64, paths = 8 and a non-zero
    _reserved; nothing is written, and the handle carries on"""
    keep = []
    pair, style, sgm = _pair_views("b", keep)
    lib = hip_lib.lib()
    dst = torch.full((8192,), float(GUARD), dtype=torch.float32, device="cuda")
    arr = (hip_lib.DenseSrc * 1)()
    arr[0].left, arr[0].right, arr[0].baseline = hip_lib.Image(*pair[0]), hip_lib.Image(*pair[1]), pair[2]
    offs = (C.c_int64 * 1)(0)

    def call(style=style, sgm=sgm):
        return lib.svo_dense_disparity_sgm(H._h, 1, arr, offs, C.byref(style), None if sgm is None else C.byref(sgm), C.c_void_p(dst.data_ptr()))

    def params(**kw):
        p = hip_lib.sgm_params(32, 256, 4095)
        for k, v in kw.items():
            if k == "reserved":
                p._reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    bad = [params(paths=8), params(paths=0), params(p1=0), params(p1=300), params(p2=-1), params(cost_cap=0), params(subpixel=2),
           params(cost_cap=16128), params(p2=12289, cost_cap=4095), params(reserved=0), params(reserved=2), None]
    for p in bad:
        assert call(sgm=p) == -1, p and [getattr(p, f[0]) for f in p._fields_[:5]]
        assert b"svo_dense_disparity_sgm" in lib.svo_last_error()
    assert call(sgm=params(p2=12288, cost_cap=4095)) == 0          # 4 * (4095 + 12288) = 65532
    dst.fill_(float(GUARD))
    assert call(style=_style(0, 3, 6, 64, 2)) == -1
    vol = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    assert lib.svo_dense_cost_volume(H._h, 1, arr, C.byref(_style(0, 3, 6, 64, 2)), 4095, offs, offs, C.c_void_p(vol.data_ptr())) == -1
    assert lib.svo_dense_cost_volume(H._h, 1, arr, C.byref(style), 0, offs, offs, C.c_void_p(vol.data_ptr())) == -1
    assert lib.svo_dense_cost_volume(H._h, 1, arr, C.byref(style), 4095, (C.c_int64 * 1)(1), offs, C.c_void_p(vol.data_ptr())) == -1
    shape = (hip_lib.SgmShape * 1)(hip_lib.SgmShape(4, 4, 65, 1.0))
    vols = (C.c_void_p * 1)(vol.data_ptr())
    assert lib.svo_sgm_aggregate(H._h, 1, shape, vols, None, 0, 0, C.byref(sgm), offs, C.c_void_p(dst.data_ptr())) == -1
    shape[0].D = 64
    assert lib.svo_sgm_aggregate(H._h, 1, shape, vols, None, 2, 0, C.byref(sgm), offs, C.c_void_p(dst.data_ptr())) == -1
    assert lib.svo_sgm_aggregate(H._h, 1, shape, vols, None, 0, 0, C.byref(params(paths=8)), offs, C.c_void_p(dst.data_ptr())) == -1
    shape[0].cols = shape[0].rows = 32768                          # a single volume beyond the stated bound
    assert lib.svo_sgm_aggregate(H._h, 1, shape, vols, None, 0, 0, C.byref(sgm), offs, C.c_void_p(dst.data_ptr())) == -4
    torch.cuda.synchronize()
    assert (_bits(dst) == _bits(np.full(1, GUARD))[0]).all() and int(vol.abs().max()) == 0
    got = _disparity_sgm(H, [pair], style, sgm)[0]                  # the handle carries on
    assert np.array_equal(_bits(got), _bits(SC.pair_reference("b")))


# ------------------------------------------------------------------ the job (svo_submit_export_disparity_sgm)
from test_dense_gpu import WIN, _batch, _frames, _np, _planes_of, played, tiny   # noqa: E402,F401 (played, tiny: fixtures)

SGM = dict(p1=32, p2=256, cost_cap=4095)


def _check_sgm_slot(tag, job, i, s, batch, what):
    """the planes of named slot i against the statement run on the planes that a view job exports of slot s; the segment
    against the view's"""
    seg = job.segments[i]
    left, right, vseg = _planes_of(batch, what, s)
    st, sgm = job.style, job.sgm
    cam = batch.slot_rig(s)[1]
    win = st.win or cam.window_size_depth_calculator
    sx, sy = st.search_x or cam.search_x, st.search_y or cam.search_y
    want = SR.planes_fast(np.ascontiguousarray(left), np.ascontiguousarray(right), win, sx, sy, st.step, sgm.p1, sgm.p2, sgm.cost_cap,
                          bool(sgm.subpixel), st.value, bool(st.cost), float(cam.baseline))
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, int(vseg["run"]), hip_lib.DISPARITY_OK), (tag, s)
    assert (int(seg["frame_id"]), int(seg["keyframe_id"])) == (int(vseg["frame_id"]), int(vseg["keyframe_id"])), (tag, s)
    assert int(seg["offset"]) == i * job.image_bytes and seg["pose"].tobytes() == vseg["pose"].tobytes(), (tag, s)
    assert F(seg["baseline"]) == F(cam.baseline), (tag, s)
    got = _np(job.planes(i))
    assert got.shape == want.shape == (job.n_planes, job.rows, job.cols)
    assert np.array_equal(_bits(got), _bits(want)), (tag, s, int((_bits(got) != _bits(want)).sum()))
    return got


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_job_against_the_statement_on_its_views(played, what, device, monkeypatch):
    """5 slots in 2 groups, rectified and converted input; slot 3 has its rig's baseline; slot 4 is empty and writes no
    plane byte; then three slots out of order across the two groups, one slot per chunk"""
    job = played.submit_disparity(what, None, step=7, cost=True, device=device, sgm=SGM, **WIN)
    job.wait()
    job._buf.fill_(float(GUARD))
    job.submit().wait()
    maps = [_check_sgm_slot(what, job, s, s, played, what) for s in range(4)]
    assert not np.array_equal(maps[0], maps[1]) and (maps[0][0] != np.floor(maps[0][0])).any()      # sub-pixel values
    seg = job.segments[4]
    assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"]), int(seg["keyframe_id"])) == (4, hip_lib.DISPARITY_NONE, -1, -1)
    assert job.planes(4) is None
    flat, guard = _bits(job._buf), _bits(np.full(1, GUARD))[0]
    assert (flat[4 * job.image_bytes // 4:] == guard).all()
    used = job.n_planes * job.rows * job.cols
    assert used * 4 < job.image_bytes
    assert all((flat[s * job.image_bytes // 4 + used:(s + 1) * job.image_bytes // 4] == guard).all() for s in range(4))
    plain = played.export_disparity(what, None, step=7, cost=True, device=device, **WIN)
    assert (plain.cols, plain.rows, plain.n_planes, plain.image_bytes) == (job.cols, job.rows, job.n_planes, job.image_bytes)
    assert plain.segments.tobytes() == job.segments.tobytes()
    monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", "1")
    job = played.export_disparity(what, [3, 0, 4, 2], value="depth", step=4, device=device, sgm=dict(SGM, subpixel=False), **WIN)
    for i, s in ((0, 3), (1, 0), (3, 2)):
        _check_sgm_slot("named", job, i, s, played, what)
    assert F(job.segments[0]["baseline"]) == F(23.5) and int(job.segments[2]["status"]) == hip_lib.DISPARITY_NONE


def _raw_submit_sgm(batch, style, sgm, dst, what=0, mem=0):
    return hip_lib.lib().svo_submit_export_disparity_sgm(batch._ctx, what, None, 0, C.byref(style), None if sgm is None else C.byref(sgm),
                                                         C.byref(dst), mem)


def test_job_rejects_memory_and_no_side_effects(tiny):
    """rejected calls queue nothing; the memory grows by the groups' blocks and by nothing else; an unchecked job before
    and after gives the bytes of a ctx that never ran SGM"""
    cfg, seqs = tiny
    n_slots = 4
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(2):
        batch.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
        twin.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
    st = _style(0, 4, 7, 9, 2, 1)
    cols, rows, planes, image_bytes = batch.disparity_size(st)
    seg = np.zeros(n_slots, hip_lib.DISPARITY_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = 0xA5
    dpx = torch.full((n_slots * image_bytes // 4 + 8,), float(GUARD), dtype=torch.float32, device="cuda")
    dst = hip_lib.DisparityDst(seg.ctypes.data, dpx.data_ptr(), n_slots * image_bytes)

    def params(**kw):
        p = hip_lib.sgm_params(32, 256, 4095)
        for k, v in kw.items():
            if k == "reserved":
                p._reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    bad = [params(paths=8), params(paths=5), params(p1=0), params(p1=257), params(p2=0), params(cost_cap=0), params(cost_cap=-3),
           params(subpixel=-1), params(subpixel=2), params(cost_cap=16128), params(p2=12289), params(reserved=0), params(reserved=1),
           params(reserved=2), None]
    for p in bad:
        assert _raw_submit_sgm(batch, st, p, dst, mem=1) == -1, p and [getattr(p, f[0]) for f in p._fields_[:5]]
        assert hip_lib.lib().svo_last_error()
    assert _raw_submit_sgm(batch, _style(0, 4, 7, 64, 2, 1), params(), dst, mem=1) == -1        # search_x = 64
    assert _raw_submit_sgm(batch, _style(0, 4, 36, 9, 2, 1), params(), dst, mem=1) == -1        # what the plain job rejects
    assert _raw_submit_sgm(batch, st, params(), dst, what=2, mem=1) == -1
    small = hip_lib.DisparityDst(seg.ctypes.data, dpx.data_ptr(), n_slots * image_bytes - 1)
    assert _raw_submit_sgm(batch, st, params(), small, mem=1) == -4
    with pytest.raises(ValueError):
        batch.submit_disparity("frames", None, step=4, lr_check=1.0, sgm=SGM, **WIN)
    batch.wait()
    assert (seg.view(np.uint8) == 0xA5).all() and (_bits(dpx) == _bits(np.full(1, GUARD))[0]).all()
    # the ctx carries on, and the memory
    kw = dict(step=4, cost=True, device=True, **WIN)
    before_plain = batch.export_disparity("frames", None, **kw)
    before = batch.memory().device_bytes
    assert before == twin.memory().device_bytes
    job = batch.export_disparity("frames", None, sgm=SGM, **kw)
    D = 10
    slot = 2 * ((cols * rows * D * 2 + 255) // 256 * 256) + (cols * rows * 2 + 255) // 256 * 256
    grown = batch.memory().device_bytes - before
    assert grown == n_slots * slot, (grown, slot)                                # per group: the block of its two slots
    batch.export_disparity("frames", None, sgm=SGM, **kw)
    batch.export_disparity("frames", [1], sgm=SGM, **dict(kw, step=8))
    assert batch.memory().device_bytes - before == grown                         # not again on a second or a smaller job
    _check_sgm_slot("device", job, 1, 1, batch, "frames")
    after_plain = batch.export_disparity("frames", None, **kw)
    twin_plain = twin.export_disparity("frames", None, **kw)
    assert _np(before_plain.values).tobytes() == _np(after_plain.values).tobytes() == _np(twin_plain.values).tobytes()
    assert not np.array_equal(_np(job.values), _np(after_plain.values))
    batch.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    twin.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    for s in range(n_slots):
        assert batch.pose(s).tobytes() == twin.pose(s).tobytes() and batch.stats(s).frame_id == 2
    batch.close(); twin.close()
