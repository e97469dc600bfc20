"""The dense disparity map (svo_dense_disparity / svo_submit_export_disparity) on the GPU, bit for bit. The yardsticks:
for the stage entry the numpy statement (tests/dense_ref.py) and the CPU oracle's per-keypoint search on the crafted
pairs of tests/dense_cases.py; for the ctx the oracle run on the LEFT and RIGHT planes that a view job exports of the
same slots. No comparison has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dense_cases as DC
import dense_ref as DR
import ingest_ref as IR
import rectify_ref as RR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch
from test_dense_cpu import oracle_plane

pytestmark = pytest.mark.gpu

GUARD = np.float32(-12345.5)                       # what the destination holds where nothing may be written
F = np.float32


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def _view(img, offset, extra, keep):
    """the image in device memory `offset` bytes past an allocation, `extra` bytes between its rows; the bytes around it
    hold a bright (or, for an image that holds 255, a dark) value: (address, w, h, stride)"""
    h, w = img.shape
    buf = np.full(offset + h * (w + extra) + 64, 0xFF if int(img.max()) < 255 else 0x01, np.uint8)
    rows = buf[offset:offset + h * (w + extra)].reshape(h, w + extra)
    rows[:, :w] = img
    t = torch.from_numpy(buf).cuda()
    keep.append(t)
    return t.data_ptr() + offset, w, h, w + extra


def _style(value=0, step=1, win=7, sx=9, sy=2, cost=1, reserved=(0, 0)):
    st = hip_lib.DisparityStyle(value, step, win, sx, sy, cost)
    st._reserved[0], st._reserved[1] = reserved
    return st


def _run(handle, pairs, style, gap=4):
    """pairs: [(left view, right view, baseline)] in one call into a destination of GUARD floats, `gap` guard floats
    (a multiple of 4) before, between and after the images; returns [planes [n, rows, cols]] and checks the guards"""
    shapes, offsets, at = [], [], gap
    for left, _, _ in pairs:
        cols, rows = left[1] // style.step, left[2] // style.step
        shapes.append((1 + style.cost, rows, cols))
        offsets.append(at * 4)
        at = (at + (1 + style.cost) * rows * cols + 3) // 4 * 4 + gap
    dst = torch.full((at,), float(GUARD), dtype=torch.float32, device="cuda")
    assert dst.data_ptr() % 16 == 0
    handle.dense_disparity(pairs, offsets, style, dst)
    got = dst.cpu().numpy()
    written = np.zeros(at, bool)
    out = []
    for shape, off in zip(shapes, offsets):
        n = int(np.prod(shape))
        out.append(got[off // 4:off // 4 + n].reshape(shape).copy())
        written[off // 4:off // 4 + n] = True
    assert (_bits(got[~written]) == _bits(np.full(1, GUARD))[0]).all(), "a guard float changed"
    return out


def _case_pair(name, keep, offset=0, extra=0, baseline=20.0):
    left, right, win, sx, sy, step = DC.cases()[name]
    return (_view(left, offset, extra, keep), _view(right, (offset * 2) % 4 if offset else 0, extra, keep), baseline), _style(0, step, win, sx, sy)


def _check_case(name, got, baseline=None):
    """got [2, rows, cols] of a case against the statement; with baseline: got[0] is the depth plane"""
    ref = DC.reference(name)
    want = ref[0]
    if baseline is not None:
        left, right, win, sx, sy, step = DC.cases()[name]
        want = DR.planes(left, right, win, sx, sy, step, DR.DEPTH, False, baseline)[0]
    bad = []
    if not np.array_equal(_bits(got[0]), _bits(want)):
        bad.append(("value", int((_bits(got[0]) != _bits(want)).sum())))
    if not np.array_equal(_bits(got[1]), _bits(ref[1])):
        bad.append(("cost", int((_bits(got[1]) != _bits(ref[1])).sum())))
    return bad


@pytest.mark.parametrize("band", ("half", "full"))
@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_every_case_against_statement_and_oracle(H, name, band, monkeypatch):
    """both launch forms: a launch of few workgroups runs with half the band of lattice rows per workgroup"""
    monkeypatch.setenv("SVO_DENSE_FEW_WORKGROUPS", "0" if band == "full" else "1000000")
    keep = []
    pair, style = _case_pair(name, keep)
    torch.cuda.synchronize()
    got = _run(H, [pair], style)[0]
    assert _check_case(name, got) == []
    left, right, win, sx, sy, step = DC.cases()[name]
    assert np.array_equal(_bits(got[0]), _bits(oracle_plane(left, right, win, sx, sy, step)))
    style.value = hip_lib.DENSE_DEPTH
    assert _check_case(name, _run(H, [pair], style)[0], baseline=20.0) == []
    style.value, style.cost = hip_lib.DENSE_DISPARITY, 0   # one plane: nothing behind it is written (_run's guards)
    one = _run(H, [pair], style)[0]
    assert one.shape[0] == 1 and np.array_equal(_bits(one[0]), _bits(got[0]))


def test_three_sizes_in_one_call_and_chunked(H, monkeypatch):
    """a, c and f have the settings 7/9/2, 7/9/2 and 31/60/6: a and c go with f's images under a's settings, so one call
    holds three sizes (97x53, 64x40, 64x20); then the same through a table of one image per launch"""
    keep = []
    cases = DC.cases()
    imgs = [cases[n][:2] for n in ("a", "c", "f")]
    pairs = [(_view(l, 0, 0, keep), _view(r, 0, 0, keep), 20.0 + i) for i, (l, r) in enumerate(imgs)]
    torch.cuda.synchronize()
    want = [DC.reference("a"), DC.reference("c"), DR.planes(*imgs[2], 7, 9, 2, 1, DR.DISPARITY, True)]
    for chunk in (None, "1", "2"):
        if chunk:
            monkeypatch.setenv("SVO_DENSE_TABLE_IMAGES", chunk)
            monkeypatch.setenv("SVO_DENSE_FEW_WORKGROUPS", "0")          # (and the full band)
        for order in ((0, 1, 2), (2, 0, 1)):
            got = _run(H, [pairs[i] for i in order], _style(0, 1, 7, 9, 2), gap=8)
            for g, i in zip(got, order):
                assert np.array_equal(_bits(g), _bits(want[i])), (chunk, order, i)
    # depth with a baseline per image
    got = _run(H, pairs, _style(1, 1, 7, 9, 2))
    for i, g in enumerate(got):
        valid = want[i][0] >= 0
        z = np.where(valid, F(20.0 + i) / np.where(valid, want[i][0], F(1)), F(0)).astype(F)
        assert np.array_equal(_bits(g[0]), _bits(z)) and np.array_equal(_bits(g[1]), _bits(want[i][1])), i


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_views_with_odd_strides_and_bases(H, offset):
    """case (g): every case through a view with stride = width + 13 whose first byte is 1, 2 or 3 past a dword"""
    keep = []
    for name in sorted(DC.cases()):
        pair, style = _case_pair(name, keep, offset=offset, extra=13)
        torch.cuda.synchronize()
        assert _check_case(name, _run(H, [pair], style)[0]) == [], (name, offset)


def test_stage_entry_rejects(H):
    keep = []
    pair, style = _case_pair("b", keep)
    lib = hip_lib.lib()
    dst = torch.full((4096,), float(GUARD), dtype=torch.float32, device="cuda")

    def call(pairs=(pair,), offs=(0,), style=style, values=dst.data_ptr(), n=None):
        arr = (hip_lib.DenseSrc * max(len(pairs), 1))()
        for i, (l, r, b) in enumerate(pairs):
            arr[i].left, arr[i].right, arr[i].baseline = hip_lib.Image(*l), hip_lib.Image(*r), b
        o = (C.c_int64 * max(len(offs), 1))(*offs)
        return lib.svo_dense_disparity(H._h, len(pairs) if n is None else n, arr, o, None if style is None else C.byref(style),
                                       C.c_void_p(values))

    assert call() == 0
    left, right, b = pair
    bad_pairs = [((0, *left[1:]), right, b), (left, (0, *right[1:]), b), (left, (right[0], right[1] - 1, right[2], right[3]), b),
                 (left, (right[0], right[1], right[2] + 1, right[3]), b), ((left[0], left[1], left[2], left[1] - 1), right, b),
                 ((left[0], 0, left[2], left[3]), (right[0], 0, right[2], right[3]), b),
                 ((left[0], 2, left[2], left[3]), (right[0], 2, right[2], right[3]), b)]          # no lattice point at step 3
    for p in bad_pairs:
        assert call(pairs=(p,)) == -1, p
    for st in (None, _style(2), _style(step=0), _style(step=17), _style(cost=2), _style(win=0), _style(sx=0), _style(sy=0),
               _style(win=36), _style(sx=65), _style(sy=9), _style(win=-1), _style(reserved=(0, 1))):
        assert call(style=st) == -1
    assert call(offs=(8,)) == -1 and call(offs=(-16,)) == -1
    assert call(values=0) == -1 and call(values=dst.data_ptr() + 4) == -1
    assert call(n=-1) == -1
    assert lib.svo_dense_disparity(H._h, 1, None, None, C.byref(style), C.c_void_p(dst.data_ptr())) == -1
    torch.cuda.synchronize()
    cols, rows = 32, 17
    assert (_bits(dst[2 * cols * rows:]) == _bits(np.full(1, GUARD))[0]).all()
    assert _check_case("b", dst[:2 * cols * rows].cpu().numpy().reshape(2, rows, cols)) == []   # only the good call wrote


# ---------------------------------------------------------------------------------- the ctx against its views

WIN = dict(win=7, search_x=9, search_y=2)          # the job's settings where the oracle runs on a whole lattice
RIG = dict(fx=212.0, fy=212.0, cx=151.5, cy=127.25, baseline=23.5)


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
    """tiny, 4 sequences of 5 frames of fast motion, gray on the device and coloured on the host: shared, never changed"""
    out = []
    for seed in (1, 11, 12, 13):
        cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", 5, seed, motion_scale=4.0)
        lc = [IR.colourize(L[k].cpu().numpy(), 2 * k + seed) for k in range(5)]
        rc = [IR.colourize(R[k].cpu().numpy(), 2 * k + 1 + seed) for k in range(5)]
        out.append((L, R, [float(t) for t in ts], lc, rc))
    torch.cuda.synchronize()
    return cfg, out


def _frames(n, seqs, k, slots, colour=False):
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for s in slots:
        L[s], R[s], ts[s] = seqs[s][3 if colour else 0][k], seqs[s][4 if colour else 1][k], seqs[s][2][k]
    return L, R, ts


@pytest.fixture(scope="module")
def played(tiny):
    """5 slots in 2 groups with rectification and a converting input format on: slots 0 .. 3 after 4 frames (slot 3 on
    a rig of its own), slot 4 empty"""
    cfg, seqs = tiny
    W, Hh = cfg["width"], cfg["height"]
    batch = _batch(cfg, 5, 2)
    batch.set_rectification(RR.euroc_like_maps(W, Hh, angle=0.012, shift=(1.5, -2.0), f_p=190.0, f_k=200.0),
                            RR.euroc_like_maps(W, Hh, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068, f_p=190.0, f_k=200.0))
    batch.set_input_format("bgr_pair")
    ids = batch.add_rigs([{k: dict(cfg, **RIG)[k] for k in hip_lib.RIG_FLOATS}])
    batch.assign_rigs([3], ids)
    for k in range(4):
        batch.new_images(*_frames(5, seqs, k, range(4), colour=True))
    yield batch
    batch.close()


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _planes_of(batch, what, s):
    """the LEFT level-0 and RIGHT planes a view job shows of slot s, and its segment"""
    left = batch.export_views(what, [s], plane="left", level=0, pixel="gray8")
    right = batch.export_views(what, [s], plane="right", pixel="gray8")
    return left.image(0), right.image(0), left.segments[0]


def _check_slot(tag, job, i, s, batch, what):
    seg = job.segments[i]
    left, right, vseg = _planes_of(batch, what, s)
    assert left is not None and right is not None, (tag, s)
    st = job.style
    cam = batch.slot_rig(s)[1]
    win = st.win or cam.window_size_depth_calculator
    sx, sy = st.search_x or cam.search_x, st.search_y or cam.search_y
    want = oracle_plane(np.ascontiguousarray(left), np.ascontiguousarray(right), win, sx, sy, st.step)
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, int(vseg["run"]), hip_lib.DISPARITY_OK), (tag, s)
    assert (int(seg["frame_id"]), int(seg["keyframe_id"])) == (int(vseg["frame_id"]), int(vseg["keyframe_id"])), (tag, s)
    assert int(seg["offset"]) == i * job.image_bytes and int(seg["_pad"]) == 0, (tag, s)
    assert seg["pose"].tobytes() == vseg["pose"].tobytes() and F(seg["time_stamp"]) == F(vseg["time_stamp"]), (tag, s)
    assert F(seg["baseline"]) == F(cam.baseline), (tag, s)
    got = _np(job.planes(i))
    assert got.shape == (job.n_planes, job.rows, job.cols)
    if st.value == hip_lib.DENSE_DEPTH:
        valid = want >= 0
        want = np.where(valid, F(cam.baseline) / np.where(valid, want, F(1)), F(0)).astype(F)
    assert np.array_equal(_bits(got[0]), _bits(want)), (tag, s, int((_bits(got[0]) != _bits(want)).sum()))
    if st.cost:
        assert np.array_equal(got[1] < 0, got[0] == (0 if st.value == hip_lib.DENSE_DEPTH else -1)), (tag, s)
    return got


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_ctx_against_the_oracle_on_its_views(played, what, device):
    """5 slots in 2 groups, rectified and converted input; slot 3 has its rig's baseline; slot 4 is empty"""
    job = played.submit_disparity(what, None, step=7, cost=True, device=device, **WIN)
    job.wait()
    job._buf.fill_(float(GUARD))
    job.submit().wait()
    maps = [_check_slot(what, job, s, s, played, what) for s in range(4)]
    assert not np.array_equal(maps[0], maps[1]) and len(np.unique(maps[0][0])) > 4
    seg = job.segments[4]
    assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"]), int(seg["keyframe_id"])) == (4, hip_lib.DISPARITY_NONE, -1, -1)
    assert job.planes(4) is None
    flat = _bits(job._buf)
    guard = _bits(np.full(1, GUARD))[0]
    assert (flat[4 * job.image_bytes // 4:] == guard).all()
    used = job.n_planes * job.rows * job.cols
    assert used * 4 < job.image_bytes                                              # (there are bytes between two slots)
    assert all((flat[s * job.image_bytes // 4 + used:(s + 1) * job.image_bytes // 4] == guard).all() for s in range(4))
    # a subset in shuffled order, depth: slot 3 divides its own rig's baseline
    job = played.export_disparity(what, [3, 0, 4, 2], value="depth", step=4, device=device, **WIN)
    for i, s in ((0, 3), (1, 0), (3, 2)):
        _check_slot("named", job, i, s, played, what)
    assert played.slot_rig(3)[0] != 0 and F(job.segments[0]["baseline"]) == F(23.5) and F(job.segments[1]["baseline"]) == F(20.0)
    assert int(job.segments[2]["status"]) == hip_lib.DISPARITY_NONE
    if what == "frames" and not device:
        # style zeros: the ctx's window and search ranges, on a coarse lattice
        job = played.export_disparity(what, [1], step=16)
        _check_slot("defaults", job, 0, 1, played, what)


def _raw_submit(batch, what, seqs, n, style, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_disparity(batch._ctx, what, arr, n, None if style is None else C.byref(style),
                                                     None if dst is None else C.byref(dst), mem)


def test_rejected_calls_queue_nothing_and_memory(tiny):
    cfg, seqs = tiny
    n_slots = 4
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(2):
        batch.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
        twin.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
    assert batch.memory().device_bytes == twin.memory().device_bytes
    st = _style(0, 4, 7, 9, 2, 0)
    cols, rows, planes, image_bytes = batch.disparity_size(st)
    seg = np.zeros(n_slots, hip_lib.DISPARITY_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = 0xA5
    px = torch.full((n_slots * image_bytes // 4 + 8,), float(GUARD), dtype=torch.float32).pin_memory()
    dpx = torch.full((n_slots * image_bytes // 4 + 8,), float(GUARD), dtype=torch.float32, device="cuda")
    dst = lambda p=px.data_ptr(), cap=n_slots * image_bytes, s=seg.ctypes.data: hip_lib.DisparityDst(s, p, cap)
    CAPACITY = _raw_submit(batch, 0, None, 0, st, dst(cap=n_slots * image_bytes - 1), 0)
    assert CAPACITY not in (0, -1)
    calls = [(0, [4], 1, st, dst(), 0), (0, [-1], 1, st, dst(), 0), (0, [0, 1, 0], 3, st, dst(), 0), (0, [0], -1, st, dst(), 0),
             (2, None, 0, st, dst(), 0), (-1, None, 0, st, dst(), 0), (0, None, 0, st, dst(), 2), (0, None, 0, st, dst(), -1),
             (0, None, 0, None, dst(), 0), (0, None, 0, _style(2, 4), dst(), 0), (0, None, 0, _style(0, 4, cost=2), dst(), 0),
             (0, None, 0, _style(step=0), dst(), 0), (0, None, 0, _style(step=17), dst(), 0), (0, None, 0, _style(win=36), dst(), 0),
             (0, None, 0, _style(sx=65), dst(), 0), (0, None, 0, _style(sy=9), dst(), 0), (0, None, 0, _style(sy=-1), dst(), 0),
             (0, None, 0, _style(reserved=(1, 0)), dst(), 0), (0, None, 0, _style(reserved=(0, 1)), dst(), 0),
             (0, None, 0, st, None, 0), (0, None, 0, st, dst(s=None), 0), (0, None, 0, st, dst(p=None), 0),
             (0, None, 0, st, dst(p=px.data_ptr() + 4), 0), (0, None, 0, st, dst(p=dpx.data_ptr() + 8), 1)]
    for c in calls:
        assert _raw_submit(batch, *c) == -1, c[:3]
        assert hip_lib.lib().svo_last_error()
    assert _raw_submit(batch, 1, [1, 2], 2, st, dst(cap=2 * image_bytes - 1), 0) == CAPACITY
    batch.wait()
    assert (seg.view(np.uint8) == 0xA5).all() and (_bits(px) == _bits(np.full(1, GUARD))[0]).all() and (_bits(dpx) == _bits(np.full(1, GUARD))[0]).all()
    # nothing else was queued and the ctx goes on: the next frame still tracks
    batch.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    twin.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    for s in range(n_slots):
        assert batch.pose(s).tobytes() == twin.pose(s).tobytes() and batch.stats(s).frame_id == 2
    before = batch.memory().device_bytes
    dev_job = batch.export_disparity("frames", [3, 0], step=4, device=True, **WIN)
    assert batch.memory().device_bytes == before                                 # device mode allocates nothing
    host_job = batch.export_disparity("frames", None, step=4, **WIN)
    grown = batch.memory().device_bytes - before
    assert grown == n_slots * host_job.image_bytes, grown                        # per group: the planes of its two slots
    batch.export_disparity("frames", None, step=4, **WIN)
    batch.export_disparity("frames", [1], step=8, **WIN)
    assert batch.memory().device_bytes - before == grown                         # not again on a second or a smaller job
    assert twin.memory().device_bytes == before                                  # (a ctx that never asks has nothing more)
    _check_slot("host", host_job, 1, 1, batch, "frames")
    _check_slot("device", dev_job, 0, 3, batch, "frames")
    batch.close(); twin.close()


def test_queue_order_and_no_side_effects(tiny):
    """a job queued between two frame sets sees the first and not the second; poses and keypoints are the same bits
    with and without disparity jobs between the steps"""
    cfg, seqs = tiny
    batch, twin = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    jobs = []
    for k in range(4):
        L, R, ts = _frames(3, seqs, k, range(3))
        packed = batch.pack_images(L, R, ts)
        batch.submit_packed(packed)
        # not waited for: ordered with the frame sets (the views next to it show what it reads)
        jobs.append((batch.submit_disparity("frames", [2, 0], step=5, **WIN), batch.submit_views("frames", [2, 0], plane="left"),
                     batch.submit_views("frames", [2, 0], plane="right"), packed))
        twin.new_images(L, R, ts)
    batch.wait()
    for k, (job, left, right, _) in enumerate(jobs):
        for i, s in enumerate((2, 0)):
            assert int(job.segments[i]["frame_id"]) == k == int(left.segments[i]["frame_id"])
            assert left.image(i).tobytes() == seqs[s][0][k].cpu().numpy().tobytes()
            want = oracle_plane(np.ascontiguousarray(left.image(i)), np.ascontiguousarray(right.image(i)), 7, 9, 2, 5)
            assert np.array_equal(_bits(job.planes(i)[0]), _bits(want)), (k, s)
    for s in range(3):
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes()
    batch.close(); twin.close()
