"""The left-right cross-check (the *_checked entries) on the GPU, bit for bit. The yardsticks: for the stage entries the
numpy statement (tests/lr_ref.py over tests/dense_ref.py and tests/cloud_ref.py, held to the CPU oracle by
tests/test_lr_cpu.py) on the crafted pairs of tests/lr_cases.py; for the ctx the statement run on the LEFT and RIGHT
planes that a view job exports of the same slots. No comparison has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_ref as CR
import dense_ref as DR
import ingest_ref as IR
import lr_cases as LC
import lr_ref as LR
import rectify_ref as RR
import test_cloud_gpu as CG
import test_dense_gpu as DG
from stereo_svo_slam_amd import hip_lib, synth

pytestmark = pytest.mark.gpu

GUARD = DG.GUARD
F = np.float32
_bits = DG._bits
POINT = hip_lib.MAP_POINT_DTYPE


def _guard_bits():
    return _bits(np.full(1, GUARD))[0]


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def _run(handle, pairs, style, check, gap=4):
    """pairs: [(left view, right view, baseline)] in one checked call into a destination of GUARD floats, `gap` guard
    floats (a multiple of 4) before, between and after the images; returns [planes [n, rows, cols]], checks the guards"""
    n_planes = 1 + style.cost + (1 if check is not None and check.lr else 0)
    shapes, offsets, at = [], [], gap
    for left, _, _ in pairs:
        cols, rows = left[1] // style.step, left[2] // style.step
        shapes.append((n_planes, rows, cols))
        offsets.append(at * 4)
        at = (at + n_planes * rows * cols + 3) // 4 * 4 + gap
    dst = torch.full((at,), float(GUARD), dtype=torch.float32, device="cuda")
    handle.dense_disparity(pairs, offsets, style, dst, check)
    got = dst.cpu().numpy()
    written = np.zeros(at, bool)
    out = []
    for shape, off in zip(shapes, offsets):
        n = int(np.prod(shape))
        out.append(got[off // 4:off // 4 + n].reshape(shape).copy())
        written[off // 4:off // 4 + n] = True
    assert (_bits(got[~written]) == _guard_bits()).all(), "a guard float changed"
    return out


def _case_pair(name, keep, offset=0, extra=0, baseline=20.0):
    left, right, win, sx, sy, step = LC.cases()[name]
    return (DG._view(left, offset, extra, keep), DG._view(right, (offset * 2) % 4 if offset else 0, extra, keep), baseline), (step, win, sx, sy)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# value, cost, max_lr_diff: report-only and masking, disparity and depth, with and without the cost plane
FORMS = ((0, 1, 0.0), (0, 1, 1.0), (1, 1, 1.0), (1, 0, 0.0), (0, 0, 1.0), (1, 0, 0.25))


@pytest.mark.parametrize("band", ("half", "full"))
@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_every_case_against_the_statement(H, name, band, monkeypatch):
    monkeypatch.setenv("SVO_DENSE_FEW_WORKGROUPS", "0" if band == "full" else "1000000")
    keep = []
    pair, (step, win, sx, sy) = _case_pair(name, keep)
    torch.cuda.synchronize()
    fwd, lr = LC.forward(name), LC.reference(name)
    for value, cost, diff in FORMS:
        got = _run(H, [pair], hip_lib.DisparityStyle(value, step, win, sx, sy, cost), hip_lib.stereo_check(True, diff))[0]
        want = LR.checked_planes(fwd, lr, value, bool(cost), 20.0, diff)
        assert _same(got, want), (name, value, cost, diff, int((_bits(got) != _bits(want)).sum()))


def test_three_sizes_in_one_call_and_chunked(H, monkeypatch):
    """a, c and the images of f under a's settings: one call holds 97x53, 64x40 and 64x20; then the same through a table
    of one and of two images per launch"""
    keep = []
    cases = LC.cases()
    imgs = [cases[n][:2] for n in ("a", "c", "f")]
    pairs = [(DG._view(l, 0, 0, keep), DG._view(r, 0, 0, keep), 20.0 + i) for i, (l, r) in enumerate(imgs)]
    torch.cuda.synchronize()
    f_fwd = DR.planes(*imgs[2], 7, 9, 2, 1, DR.DISPARITY, True)
    refs = [(LC.forward("a"), LC.reference("a")), (LC.forward("c"), LC.reference("c")), (f_fwd, LR.lr_plane(*imgs[2], 7, 9, 2, 1, f_fwd[0]))]
    for chunk in (None, "1", "2"):
        if chunk:
            monkeypatch.setenv("SVO_DENSE_TABLE_IMAGES", chunk)
            monkeypatch.setenv("SVO_DENSE_FEW_WORKGROUPS", "0")
        for order, (value, cost, diff) in (((0, 1, 2), (0, 1, 1.0)), ((2, 0, 1), (1, 0, 0.5))):
            got = _run(H, [pairs[i] for i in order], hip_lib.DisparityStyle(value, 1, 7, 9, 2, cost), hip_lib.stereo_check(True, diff), gap=8)
            for g, i in zip(got, order):
                assert _same(g, LR.checked_planes(*refs[i], value, bool(cost), 20.0 + i, diff)), (chunk, order, i)


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_views_with_odd_strides_and_bases(H, offset):
    """every case through views with stride = width + 13 whose first byte is 1, 2 or 3 past a dword: the mirrored
    staging reads its bytes at any base; the bytes around an image are bright"""
    keep = []
    for name in sorted(LC.cases()):
        pair, (step, win, sx, sy) = _case_pair(name, keep, offset=offset, extra=13)
        torch.cuda.synchronize()
        got = _run(H, [pair], hip_lib.DisparityStyle(0, step, win, sx, sy, 1), hip_lib.stereo_check(True, 1.0))[0]
        assert _same(got, LR.checked_planes(LC.forward(name), LC.reference(name), 0, True, 20.0, 1.0)), (name, offset)


def test_off_is_the_unchecked_entry_and_rejects(H):
    keep = []
    pair, (step, win, sx, sy) = _case_pair("b", keep)
    style = hip_lib.DisparityStyle(0, step, win, sx, sy, 1)
    plain = DG._run(H, [pair], style)[0]
    assert _same(_run(H, [pair], style, None)[0], plain) and _same(_run(H, [pair], style, hip_lib.stereo_check(False, 2.0))[0], plain)
    lib = hip_lib.lib()
    dst = torch.full((8192,), float(GUARD), dtype=torch.float32, device="cuda")
    packed = H.pack_dense([pair], [0])

    def call(check, style=style):
        return lib.svo_dense_disparity_checked(H._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(check), C.c_void_p(dst.data_ptr()))

    for ck in _bad_checks():
        assert call(ck) == -1 and lib.svo_last_error()
    assert call(hip_lib.stereo_check(True, 1.0), hip_lib.DisparityStyle(0, step, 36, sx, sy, 1)) == -1
    torch.cuda.synchronize()
    assert (_bits(dst) == _guard_bits()).all()                                                 # no rejected call wrote


def _bad_checks(cloud=False):
    out = [hip_lib.StereoCheck(2, 1.0), hip_lib.StereoCheck(-1, 1.0), hip_lib.StereoCheck(1, -1.0), hip_lib.StereoCheck(1, float("inf")),
           hip_lib.StereoCheck(1, float("nan")), hip_lib.StereoCheck(0, -1.0)]
    for lr in (0, 1):
        for r in (0, 5):
            ck = hip_lib.StereoCheck(lr, 1.0)
            ck._reserved[r] = 1
            out.append(ck)
    return out + ([hip_lib.StereoCheck(1, 0.0)] if cloud else [])


# ---------------------------------------------------------------------------------- clouds, stage entry

CLOUD_RIG = dict(fx=212.0, fy=209.0, cx=47.5, cy=21.25, baseline=23.5)
CLOUD_POSE = (0.5, -0.25, 1.0, 0.2, -0.1, 0.3)
CLOUD_FILTER = dict(min_disparity=1.0, max_depth=2000.0, max_mean_cost=900.0)


def _run_cloud(handle, srcs, style, check, gap=3):
    """CG._run with a check: per image (its cols * rows records, its count); checks the guard records between"""
    first, sizes, at = [], [], gap
    for left, _, _, _ in srcs:
        n = (left[1] // style.step) * (left[2] // style.step)
        first.append(at)
        sizes.append(n)
        at += n + gap
    dst = torch.full((at, 16), CG.GUARD, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(srcs) + 2,), -7, dtype=torch.int32, device="cuda")
    handle.cloud_points(srcs, first, style, dst, counts[1:], check)
    got, counts = dst.cpu().numpy(), counts.cpu().numpy()
    assert counts[0] == -7 and counts[-1] == -7
    outside = np.ones(at, bool)
    out = []
    for i, (lo, n) in enumerate(zip(first, sizes)):
        out.append((got[lo:lo + n].copy().view(POINT)[:, 0], int(counts[1 + i])))
        outside[lo:lo + n] = False
    assert (got[outside] == CG.GUARD).all(), "a guard record changed"
    return out


def _masked(fwd, lr, diff):
    """the disparity and cost planes the count and write launches of a checked cloud see"""
    return np.stack([LR.checked_planes(fwd, lr, DR.DISPARITY, False, max_lr_diff=diff)[0], fwd[1]])


@pytest.mark.parametrize("layout", (CR.COMPACT, CR.ORGANIZED))
def test_cloud_points_checked(H, layout, monkeypatch):
    """three cases in one call (and through a table of one image per launch) against cloud_ref on lr_ref's masked planes;
    a check that is off gives the unchecked records"""
    keep = []
    names = ("occl1", "a", "wide2")
    srcs, wants, plain = [], [], []
    for name in names:
        left, right, win, sx, sy, step = LC.cases()[name]
        srcs.append((DG._view(left, 0, 0, keep), DG._view(right, 0, 0, keep), CLOUD_RIG, CLOUD_POSE))
        planes = _masked(LC.forward(name), LC.reference(name), 1.0)
        wants.append(CR.cloud(left, planes, win, step, CLOUD_RIG, CLOUD_POSE, CR.WORLD, layout, **CLOUD_FILTER))
        plain.append(CR.cloud(left, LC.forward(name), win, step, CLOUD_RIG, CLOUD_POSE, CR.WORLD, layout, **CLOUD_FILTER))
    torch.cuda.synchronize()
    assert all(0 < w[1] < p[1] for w, p in zip(wants, plain))                                 # the check drops some and keeps some
    for chunk in (None, "1"):
        if chunk:
            monkeypatch.setenv("SVO_CLOUD_TABLE_IMAGES", chunk)
        for i, name in enumerate(names):
            left, right, win, sx, sy, step = LC.cases()[name]
            style = hip_lib.cloud_style(step, win, sx, sy, CR.WORLD, layout, **CLOUD_FILTER)
            # (the cases differ in their settings: a call per case, and one of two images where the settings agree)
            got = _run_cloud(H, [srcs[i]], style, hip_lib.stereo_check(True, 1.0))
            CG._check(got[0], wants[i], layout, (name, chunk))
            CG._check(_run_cloud(H, [srcs[i]], style, hip_lib.stereo_check(False, 1.0))[0], plain[i], layout, (name, "off"))
            CG._check(_run_cloud(H, [srcs[i]], style, None)[0], plain[i], layout, (name, "null"))
    # two sizes in one call: occl1's and a's images under a's settings (7 / 9 / 2, step 1)
    left, right = LC.cases()["occl1"][:2]
    fwd = DR.planes(left, right, 7, 9, 2, 1, DR.DISPARITY, True)
    want_o = CR.cloud(left, _masked(fwd, LR.lr_plane(left, right, 7, 9, 2, 1, fwd[0]), 1.0), 7, 1, CLOUD_RIG, CLOUD_POSE, CR.WORLD, layout, **CLOUD_FILTER)
    style = hip_lib.cloud_style(1, 7, 9, 2, CR.WORLD, layout, **CLOUD_FILTER)
    for order in ((0, 1), (1, 0)):
        got = _run_cloud(H, [srcs[i] for i in order], style, hip_lib.stereo_check(True, 1.0), gap=5)
        for g, i in zip(got, order):
            CG._check(g, (want_o, wants[1])[i], layout, ("two", order, i))
    lib = hip_lib.lib()
    packed = H.pack_cloud([srcs[1]], [0])
    dst = torch.full((6000, 16), CG.GUARD, dtype=torch.uint8, device="cuda")
    for ck in _bad_checks(cloud=True):
        assert lib.svo_cloud_points_checked(H._h, packed[0], packed[1], packed[2], C.byref(style), C.byref(ck), C.c_void_p(dst.data_ptr()), None) == -1
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CG.GUARD).all()


# ---------------------------------------------------------------------------------- the ctx against its views

WIN = DG.WIN
STEP = 8
DIFF = 1.0
FILTER = CG.FILTER


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


@pytest.fixture(scope="module")
def played(tiny):
    """5 slots in 2 groups with rectification and a converting input format on: slots 0 .. 3 after 4 frames (slot 3 on
    a rig of its own), slot 4 empty; and the statement's planes of the views of every (what, slot), computed once"""
    cfg, seqs = tiny
    W, Hh = cfg["width"], cfg["height"]
    batch = DG._batch(cfg, 5, 2)
    batch.set_rectification(RR.euroc_like_maps(W, Hh, angle=0.012, shift=(1.5, -2.0), f_p=190.0, f_k=200.0),
                            RR.euroc_like_maps(W, Hh, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068, f_p=190.0, f_k=200.0))
    batch.set_input_format("bgr_pair")
    ids = batch.add_rigs([{k: dict(cfg, **DG.RIG)[k] for k in hip_lib.RIG_FLOATS}])
    batch.assign_rigs([3], ids)
    for k in range(4):
        batch.new_images(*DG._frames(5, seqs, k, range(4), colour=True))
    yield batch, {}
    batch.close()


def _slot_ref(played, what, s):
    """of slot s: the LEFT plane a view job shows, its segment, dense_ref's planes of LEFT and RIGHT and lr_ref's plane"""
    batch, cache = played
    if (what, s) not in cache:
        left, right, vseg = DG._planes_of(batch, what, s)
        assert left is not None and right is not None, (what, s)
        l, r = np.ascontiguousarray(left), np.ascontiguousarray(right)
        fwd = DR.planes(l, r, WIN["win"], WIN["search_x"], WIN["search_y"], STEP, DR.DISPARITY, True)
        cache[(what, s)] = (l, vseg.copy(), fwd, LR.lr_plane(l, r, WIN["win"], WIN["search_x"], WIN["search_y"], STEP, fwd[0]))
    return cache[(what, s)]


def _check_disparity_slot(tag, job, i, s, played, what, diff):
    batch = played[0]
    seg = job.segments[i]
    _, vseg, fwd, lr = _slot_ref(played, what, s)
    cam = batch.slot_rig(s)[1]
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, int(vseg["run"]), hip_lib.DISPARITY_OK), (tag, s)
    assert (int(seg["frame_id"]), int(seg["keyframe_id"])) == (int(vseg["frame_id"]), int(vseg["keyframe_id"])), (tag, s)
    assert int(seg["offset"]) == i * job.image_bytes and seg["pose"].tobytes() == vseg["pose"].tobytes(), (tag, s)
    assert F(seg["baseline"]) == F(cam.baseline), (tag, s)
    want = LR.checked_planes(fwd, lr, job.style.value, bool(job.style.cost), cam.baseline, diff)
    got = DG._np(job.planes(i))
    assert got.shape == (job.n_planes, job.rows, job.cols) == want.shape, (tag, s)
    assert np.array_equal(_bits(got), _bits(want)), (tag, s, [int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)])
    assert np.array_equal(_bits(DG._np(job.lr(i))), _bits(lr)), (tag, s)
    return lr


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_disparity_job_against_the_statement_on_its_views(played, what, device, monkeypatch):
    """5 slots in 2 groups, rectified and converted input; slot 3 has its rig's baseline; slot 4 is empty"""
    batch = played[0]
    job = batch.submit_disparity(what, None, step=STEP, cost=True, device=device, lr_check=DIFF, **WIN)
    job.wait()
    job._buf.fill_(float(GUARD))
    job.submit().wait()
    assert job.n_planes == 3
    lrs = [_check_disparity_slot(what, job, s, s, played, what, DIFF) for s in range(4)]
    for lr in lrs:
        fails = LR.fails(lr, DIFF)
        assert fails.any() and not fails.all()                                               # the check drops some and keeps some
    seg = job.segments[4]
    assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"]), int(seg["keyframe_id"])) == (4, hip_lib.DISPARITY_NONE, -1, -1)
    assert job.planes(4) is None and job.lr(4) is None
    flat = _bits(job._buf)
    assert (flat[4 * job.image_bytes // 4:] == _guard_bits()).all()
    used = job.n_planes * job.rows * job.cols
    assert used * 4 < job.image_bytes                                                        # (there are bytes between two slots)
    assert all((flat[s * job.image_bytes // 4 + used:(s + 1) * job.image_bytes // 4] == _guard_bits()).all() for s in range(4))
    # a subset in shuffled order, depth, report only, no cost plane, a chunk of the reverse planes per slot
    monkeypatch.setenv("SVO_LR_CHUNK_SLOTS", "1")
    job = batch.export_disparity(what, [3, 0, 4, 2], value="depth", step=STEP, device=device, lr_check=True, **WIN)
    assert job.n_planes == 2
    for i, s in ((0, 3), (1, 0), (3, 2)):
        _check_disparity_slot("named", job, i, s, played, what, 0.0)
    assert int(job.segments[2]["status"]) == hip_lib.DISPARITY_NONE
    monkeypatch.setenv("SVO_DENSE_TABLE_IMAGES", "1")
    job = batch.export_disparity(what, [1, 2], value="depth", step=STEP, cost=True, device=device, lr_check=0.5, **WIN)
    for i, s in ((0, 1), (1, 2)):
        _check_disparity_slot("tables", job, i, s, played, what, 0.5)


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_cloud_job_against_the_statement_on_its_views(played, what, device, monkeypatch):
    batch = played[0]
    for layout, frame, chunk in (("compact", "world", None), ("organized", "camera", "1")):
        if chunk:
            monkeypatch.setenv("SVO_CLOUD_CHUNK_SLOTS", chunk)      # a chunk per slot
            monkeypatch.setenv("SVO_CLOUD_TABLE_IMAGES", chunk)
        job = batch.submit_cloud(what, None, step=STEP, frame=frame, layout=layout, device=device, lr_check=DIFF, **WIN, **FILTER)
        job.wait()
        job.points_buffer.fill_(CG.GUARD)
        job.submit().wait()
        st = job.style
        kept = plain = 0
        for s in range(4):
            left, vseg, fwd, lr = _slot_ref(played, what, s)
            seg = job.segments[s]
            cam = batch.slot_rig(s)[1]
            rig = {k: getattr(cam, k) for k in CR.RIG_KEYS}
            assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"])) == (s, hip_lib.CLOUD_OK, int(vseg["frame_id"])), (what, s)
            assert seg["pose"].tobytes() == vseg["pose"].tobytes() and int(seg["first_point"]) == s * job.points_per_slot
            args = (WIN["win"], st.step, rig, seg["pose"], st.frame, st.layout, st.min_disparity, st.max_depth, st.max_mean_cost)
            ref, n = CR.cloud(left, _masked(fwd, lr, DIFF), *args)
            kept, plain = kept + n, plain + CR.cloud(left, fwd, *args)[1]
            assert int(seg["n_points"]) == n, (what, layout, s, int(seg["n_points"]), n)
            raw = DG._np(job.points_buffer[s * job.points_per_slot:(s + 1) * job.points_per_slot])
            if st.layout == CR.ORGANIZED:
                assert raw.tobytes() == ref.tobytes(), (what, s)
            else:
                assert raw[:n].tobytes() == ref.tobytes() and (raw[n:] == CG.GUARD).all(), (what, s)
        assert 0 < kept < plain, (what, layout, kept, plain)                                   # the check drops some and keeps some
        seg = job.segments[4]
        assert (int(seg["status"]), int(seg["n_points"])) == (hip_lib.CLOUD_NONE, 0)
        assert (DG._np(job.points_buffer[4 * job.points_per_slot:]) == CG.GUARD).all()


# ---------------------------------------------------------------------------------- off, rejections, queue order


def _raw_disparity(batch, what, seqs, n, style, check, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_disparity_checked(batch._ctx, what, arr, n, None if style is None else C.byref(style),
                                                             None if check is None else C.byref(check), None if dst is None else C.byref(dst), mem)


def _raw_cloud(batch, what, seqs, n, style, check, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_cloud_checked(batch._ctx, what, arr, n, None if style is None else C.byref(style),
                                                         None if check is None else C.byref(check), None if dst is None else C.byref(dst), mem)


def test_off_rejections_and_memory(tiny):
    cfg, seqs = tiny
    n_slots = 4
    batch, twin = DG._batch(cfg, n_slots, 2), DG._batch(cfg, n_slots, 2)
    for k in range(2):
        batch.new_images(*DG._frames(n_slots, seqs, k, range(n_slots)))
        twin.new_images(*DG._frames(n_slots, seqs, k, range(n_slots)))
    st = hip_lib.DisparityStyle(1, 4, 7, 9, 2, 1)
    cst = hip_lib.cloud_style(4, 7, 9, 2, "world", "compact", **FILTER)
    good = hip_lib.stereo_check(True, 1.0)
    cols, rows, planes, image_bytes = batch.disparity_size(st, good)
    assert planes == 3
    points = batch.cloud_size(cst)[2]
    seg = np.zeros(n_slots, hip_lib.DISPARITY_SEGMENT_DTYPE)
    cseg = np.zeros(n_slots, hip_lib.CLOUD_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = 0xA5
    cseg.view(np.uint8)[:] = 0xA5
    px = torch.full((n_slots * image_bytes // 4 + 8,), float(GUARD), dtype=torch.float32).pin_memory()
    dpx = torch.full((n_slots * image_bytes // 4 + 8,), float(GUARD), dtype=torch.float32, device="cuda")
    pts = torch.full((n_slots * points, 16), CG.GUARD, dtype=torch.uint8).pin_memory()
    dst = lambda p=px.data_ptr(), cap=n_slots * image_bytes, s=seg.ctypes.data: hip_lib.DisparityDst(s, p, cap)
    cdst = lambda p=pts.data_ptr(), cap=n_slots * points, s=cseg.ctypes.data: hip_lib.CloudDst(s, p, cap)
    # every bad check, and what the unchecked entries reject, with a good check: nothing is queued or written
    for ck in _bad_checks():
        assert _raw_disparity(batch, 0, None, 0, st, ck, dst(), 0) == -1 and hip_lib.lib().svo_last_error()
        assert _raw_disparity(batch, 0, None, 0, st, ck, dst(p=dpx.data_ptr()), 1) == -1
    for ck in _bad_checks(cloud=True):
        assert _raw_cloud(batch, 0, None, 0, cst, ck, cdst(), 0) == -1 and hip_lib.lib().svo_last_error()
    CAPACITY = _raw_disparity(batch, 0, None, 0, st, good, dst(cap=n_slots * image_bytes - 1), 0)
    assert CAPACITY not in (0, -1)
    # (the unchecked job's capacity is too small: the lr plane counts)
    assert _raw_disparity(batch, 0, None, 0, st, good, dst(cap=n_slots * batch.disparity_size(st)[3]), 0) == CAPACITY
    for c in ((0, [4], 1, st, good, dst(), 0), (0, [0, 1, 0], 3, st, good, dst(), 0), (2, None, 0, st, good, dst(), 0),
              (0, None, 0, st, good, dst(), 2), (0, None, 0, None, good, dst(), 0), (0, None, 0, hip_lib.DisparityStyle(2, 4, 7, 9, 2, 0), good, dst(), 0),
              (0, None, 0, st, good, None, 0), (0, None, 0, st, good, dst(s=None), 0), (0, None, 0, st, good, dst(p=px.data_ptr() + 4), 0)):
        assert _raw_disparity(batch, *c) == -1, c[:3]
    for c in ((0, [4], 1, cst, good, cdst(), 0), (0, None, 0, None, good, cdst(), 0), (0, None, 0, cst, good, cdst(p=None), 0),
              (0, None, 0, hip_lib.cloud_style(4, 7, 9, 2, 2), good, cdst(), 0)):
        assert _raw_cloud(batch, *c) == -1, c[:3]
    assert _raw_cloud(batch, 0, None, 0, cst, good, cdst(cap=n_slots * points - 1), 0) == CAPACITY
    batch.wait()
    assert (seg.view(np.uint8) == 0xA5).all() and (cseg.view(np.uint8) == 0xA5).all()
    assert (_bits(px) == _guard_bits()).all() and (_bits(dpx) == _guard_bits()).all() and (pts.numpy() == CG.GUARD).all()
    assert batch.memory().device_bytes == twin.memory().device_bytes
    # check = NULL and lr = 0: the unchecked job's segments, bytes and memory
    before = batch.memory().device_bytes
    off = hip_lib.stereo_check(False, 3.0)
    plain_bytes = batch.disparity_size(st)[3]
    want_d = twin.submit_disparity("frames", None, style=st, device=True).wait()
    want_c = twin.submit_cloud("frames", None, style=cst).wait()
    want_d._buf.fill_(float(GUARD))                          # (again, into guards: what a job does not write compares too)
    want_c.points_buffer.fill_(CG.GUARD)
    want_d.submit().wait()
    want_c.submit().wait()
    for ck in (None, off):
        seg.view(np.uint8)[:] = 0xA5
        dpx.fill_(float(GUARD))
        assert _raw_disparity(batch, 0, None, 0, st, ck, dst(p=dpx.data_ptr(), cap=n_slots * plain_bytes), 1) == 0
        batch.wait()
        assert seg.tobytes() == want_d.segments.tobytes()
        assert np.array_equal(_bits(dpx[:n_slots * plain_bytes // 4]), _bits(want_d._buf)) and (_bits(dpx[n_slots * plain_bytes // 4:]) == _guard_bits()).all()
        assert batch.memory().device_bytes == before                                          # device mode allocates nothing
    mem_c = None
    for ck in (None, off):
        cseg.view(np.uint8)[:] = 0xA5
        pts.fill_(CG.GUARD)
        assert _raw_cloud(batch, 0, None, 0, cst, ck, cdst(), 0) == 0
        batch.wait()
        assert cseg.tobytes() == want_c.segments.tobytes() and pts.numpy().tobytes() == want_c.points_buffer.numpy().tobytes()
        mem_c = batch.memory().device_bytes if mem_c is None else mem_c
        assert batch.memory().device_bytes == mem_c
    twin_mem = twin.memory().device_bytes
    # a checked device-mode job: the reverse planes of the group's named slots, made once
    reverse = (rows * cfg["width"] * 4 + 255) // 256 * 256
    job = batch.export_disparity("frames", None, style=st, device=True, lr_check=1.0)
    assert batch.memory().device_bytes - mem_c == n_slots * reverse                          # per group: its two slots
    batch.export_disparity("frames", [1], style=st, device=True, lr_check=1.0)
    batch.export_cloud("frames", [0, 1], style=cst, lr_check=1.0)
    assert batch.memory().device_bytes - mem_c == n_slots * reverse                          # not again on a smaller job
    assert twin.memory().device_bytes == twin_mem
    assert job.n_planes == 3 and np.array_equal(_bits(DG._np(job.values[:, 1])), _bits(DG._np(want_d.values[:, 1])))   # the cost plane is never changed
    batch.close(); twin.close()


def test_queue_order_and_no_side_effects(tiny):
    """checked jobs queued between two frame sets see the first and not the second; poses and keypoints are the same
    bits with and without them between the steps"""
    cfg, seqs = tiny
    batch, twin = DG._batch(cfg, 3, 2), DG._batch(cfg, 3, 2)
    jobs = []
    for k in range(4):
        L, R, ts = DG._frames(3, seqs, k, range(3))
        packed = batch.pack_images(L, R, ts)
        batch.submit_packed(packed)
        jobs.append((batch.submit_disparity("frames", [2, 0], step=8, lr_check=1.0, **WIN), batch.submit_views("frames", [2, 0], plane="left"),
                     batch.submit_views("frames", [2, 0], plane="right"), batch.submit_cloud("frames", [1], step=8, lr_check=1.0, **WIN), packed))
        twin.new_images(L, R, ts)
    batch.wait()
    for k, (job, left, right, cloud, _) in enumerate(jobs):
        assert int(cloud.segments[0]["frame_id"]) == k
        for i in range(2):
            assert int(job.segments[i]["frame_id"]) == k == int(left.segments[i]["frame_id"])
        if k not in (0, 3):
            continue
        l, r = np.ascontiguousarray(left.image(0)), np.ascontiguousarray(right.image(0))
        assert l.tobytes() == seqs[2][0][k].cpu().numpy().tobytes()
        fwd = DR.planes(l, r, 7, 9, 2, 8, DR.DISPARITY, True)
        want = LR.checked_planes(fwd, LR.lr_plane(l, r, 7, 9, 2, 8, fwd[0]), 0, False, 1.0, 1.0)
        assert np.array_equal(_bits(job.planes(0)), _bits(want)), k
    for s in range(3):
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes()
    batch.close(); twin.close()
