"""The dense point cloud (svo_cloud_points / svo_submit_export_cloud) on the GPU, byte for byte. The yardstick is the
numpy statement (tests/cloud_ref.py, held to the CPU oracle by tests/test_cloud_cpu.py): for the stage entry on the
crafted cases of tests/cloud_cases.py, for the ctx evaluated on the LEFT and RIGHT planes that a view job exports of the
same slots, with the slot's rig and the segment's pose. No comparison has a tolerance."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import cloud_cases as CC
import cloud_ref as CR
import dense_ref as DR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu

GUARD = 0xA5                                         # every byte of a destination where nothing may be written
F = np.float32
POINT = hip_lib.MAP_POINT_DTYPE
FRAMES = {"world": CR.WORLD, "camera": CR.CAMERA}
LAYOUTS = {"compact": CR.COMPACT, "organized": CR.ORGANIZED}


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


def _style(c, frame=CR.WORLD, layout=CR.COMPACT):
    return hip_lib.cloud_style(c["step"], c["win"], c["search_x"], c["search_y"], frame, layout, **c["filter"])


def _src(c, keep, offset=0, extra=0):
    return (_view(c["left"], offset, extra, keep), _view(c["right"], (offset * 2) % 4 if offset else 0, extra, keep), c["rig"], c["pose"])


def _run(handle, srcs, style, with_counts=True, gap=3):
    """srcs in one call into a destination of GUARD bytes, `gap` guard records before, between and after the images'
    cols * rows records; returns per image (its cols * rows records, its count or None) and checks the guards between"""
    first, sizes, at = [], [], gap
    for left, _, _, _ in srcs:
        n = (left[1] // style.step) * (left[2] // style.step)
        first.append(at)
        sizes.append(n)
        at += n + gap
    dst = torch.full((at, 16), GUARD, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(srcs) + 2,), -7, dtype=torch.int32, device="cuda") if with_counts else None
    assert dst.data_ptr() % 16 == 0
    handle.cloud_points(srcs, first, style, dst, None if counts is None else counts[1:])
    got = dst.cpu().numpy()
    outside = np.ones(at, bool)
    out = []
    if counts is not None:
        counts = counts.cpu().numpy()
        assert counts[0] == -7 and counts[-1] == -7
    for i, (lo, n) in enumerate(zip(first, sizes)):
        out.append((got[lo:lo + n].copy().view(POINT)[:, 0], None if counts is None else int(counts[1 + i])))
        outside[lo:lo + n] = False
    assert (got[outside] == GUARD).all(), "a guard record changed"
    return out


def _check(got, want, layout, tag):
    """one image's records and count against the statement's (records, n): compact: the first n records, and guard
    bytes behind them; organized: every record"""
    rec, count = got
    ref, n = want
    assert count is None or count == n, (tag, count, n)
    if layout == CR.ORGANIZED:
        assert rec.tobytes() == ref.tobytes(), (tag, int((rec.view(np.uint8) != ref.view(np.uint8)).sum()))
    else:
        assert len(ref) == n and rec[:n].tobytes() == ref.tobytes(), tag
        assert (rec[n:].view(np.uint8) == GUARD).all(), (tag, "a record beyond n_points was written")


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", sorted(CC.cases()))
def test_every_case_against_the_statement(H, name, layout, frame):
    keep = []
    c = CC.cases()[name]
    src = _src(c, keep)
    torch.cuda.synchronize()
    want = CC.reference(name, FRAMES[frame], LAYOUTS[layout])
    for with_counts in (True, False):
        got = _run(H, [src], _style(c, FRAMES[frame], LAYOUTS[layout]), with_counts)[0]
        _check(got, want, LAYOUTS[layout], (name, layout, frame, with_counts))


# the pairs of the four sizes under one style: 97 x 53, 80 x 48, 64 x 40 and 64 x 20 at step 2, each with a rig and a pose
MIXED = dict(win=7, search_x=9, search_y=2, step=2, filter=dict(min_disparity=1.0, max_depth=15.0, max_mean_cost=22000.0))
MIXED_CASES = (("all", CC.RIG_CENTRED, CC.POSE_GENERAL), ("depth", CC.RIG_SKEWED, CC.POSE_ZERO), ("ties", CC.RIG_SKEWED, CC.POSE_GENERAL),
               ("invalid", CC.RIG_CENTRED, (-1.0, 0.5, 0.25, -0.3, 0.2, 0.1)))


@functools.lru_cache(maxsize=None)
def _mixed():
    out = []
    for name, rig, pose in MIXED_CASES:
        c = dict(CC.cases()[name], rig=rig, pose=pose, **MIXED)
        planes = DR.planes(c["left"], c["right"], c["win"], c["search_x"], c["search_y"], c["step"], DR.DISPARITY, True)
        out.append((c, planes))
    return out


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_four_sizes_in_one_call_and_chunked(H, layout, monkeypatch):
    keep = []
    mixed = _mixed()
    srcs = [_src(c, keep) for c, _ in mixed]
    torch.cuda.synchronize()
    want = [CR.cloud(c["left"], planes, c["win"], c["step"], c["rig"], c["pose"], CR.WORLD, LAYOUTS[layout], **c["filter"]) for c, planes in mixed]
    assert len({c["left"].shape for c, _ in mixed}) == 4 and all(0 < n < planes[0].size for (_, n), (_, planes) in zip(want, mixed))
    style = _style(mixed[0][0], CR.WORLD, LAYOUTS[layout])
    for chunk in (None, "1", "3"):
        if chunk:
            monkeypatch.setenv("SVO_CLOUD_TABLE_IMAGES", chunk)
        for order in ((0, 1, 2, 3), (3, 1, 0, 2)):
            got = _run(H, [srcs[i] for i in order], style, gap=5)
            for g, i in zip(got, order):
                _check(g, want[i], LAYOUTS[layout], (chunk, order, i))


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_views_with_odd_strides_and_bases(H, offset):
    """every case through views with stride = width + 13 whose first byte is 1, 2 or 3 past a dword"""
    keep = []
    for name in sorted(CC.cases()):
        c = CC.cases()[name]
        layout = CR.ORGANIZED if offset == 2 else CR.COMPACT
        src = _src(c, keep, offset=offset, extra=13)
        torch.cuda.synchronize()
        _check(_run(H, [src], _style(c, CR.WORLD, layout))[0], CC.reference(name, CR.WORLD, layout), layout, (name, offset))


def _bad_styles(base):
    def st(**kw):
        s = hip_lib.CloudStyle.from_buffer_copy(base)
        for k, v in kw.items():
            if k == "reserved":
                s._reserved[v] = 1
            else:
                setattr(s, k, v)
        return s
    return [st(step=0), st(step=17), st(win=36), st(win=-1), st(search_x=65), st(search_y=9), st(search_y=-1), st(frame=2), st(frame=-1),
            st(layout=2), st(layout=-1), st(min_disparity=-1.0), st(max_depth=float("inf")), st(max_mean_cost=float("nan")),
            st(max_depth=-0.0625), st(reserved=0), st(reserved=1), st(reserved=2)]


def test_stage_entry_rejects(H):
    keep = []
    c = CC.cases()["disparity"]
    left, right, rig, pose = _src(c, keep)
    style = _style(c)
    lib = hip_lib.lib()
    n = CC.planes("disparity")[0].size
    dst = torch.full((n + 8, 16), GUARD, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -7, dtype=torch.int32, device="cuda")

    def call(l=left, r=right, first=(0,), style=style, points=dst.data_ptr(), counts=cnt.data_ptr(), n=1, reserved=0, arrays=True):
        arr = (hip_lib.CloudSrc * 1)()
        arr[0].left, arr[0].right = hip_lib.Image(*l), hip_lib.Image(*r)
        for k in CR.RIG_KEYS:
            setattr(arr[0], k, rig[k])
        arr[0].pose = (C.c_float * 6)(*pose)
        arr[0]._reserved = reserved
        o = (C.c_int64 * 1)(*first)
        return lib.svo_cloud_points(H._h, n, arr if arrays else None, o if arrays else None, None if style is None else C.byref(style),
                                    C.c_void_p(points), C.c_void_p(counts))

    bad = [dict(l=(0, *left[1:])), dict(r=(0, *right[1:])), dict(r=(right[0], right[1] - 1, right[2], right[3])),
           dict(r=(right[0], right[1], right[2] + 1, right[3])), dict(l=(left[0], left[1], left[2], left[1] - 1)),
           dict(l=(left[0], 0, left[2], left[3]), r=(right[0], 0, right[2], right[3])),
           dict(l=(left[0], 3, left[2], left[3]), r=(right[0], 3, right[2], right[3])),          # no lattice point at step 4
           dict(first=(-1,)), dict(points=0), dict(points=dst.data_ptr() + 8), dict(counts=cnt.data_ptr() + 2), dict(n=-1),
           dict(reserved=1), dict(arrays=False), dict(style=None), dict(style=hip_lib.cloud_style(4, 0, 9, 2)),
           dict(style=hip_lib.cloud_style(4, 7, 0, 2)), dict(style=hip_lib.cloud_style(4, 7, 9, 0))]
    bad += [dict(style=s) for s in _bad_styles(style)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.svo_last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == GUARD).all() and (cnt.cpu().numpy() == -7).all()             # no rejected call wrote
    assert call(n=0) == 0 and call() == 0
    ref, kept = CC.reference("disparity", CR.WORLD, CR.COMPACT)
    got = dst.cpu().numpy()
    assert got[:kept].tobytes() == ref.tobytes() and (got[kept:] == GUARD).all() and cnt.cpu().numpy().tolist() == [kept, -7, -7, -7]


# ---------------------------------------------------------------------------------- the ctx against its views

WIN = dict(win=7, search_x=9, search_y=2)          # the job's settings where the statement runs on a whole lattice
STEP = 8
RIG = dict(fx=212.0, fy=209.0, cx=151.5, cy=127.25, baseline=23.5)
FILTER = dict(min_disparity=3.5, max_depth=5.0, max_mean_cost=45.0)


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
    """tiny, 4 sequences of 5 frames of fast motion, gray on the device: shared, never changed"""
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


@pytest.fixture(scope="module")
def played(tiny):
    """5 slots in 2 groups: slots 0 .. 3 after 4 frames (slot 3 on a rig of its own, slot 1 sat the last frame out),
    slot 4 empty; and the statement's planes of the views of every (what, slot), computed once"""
    cfg, seqs = tiny
    batch = _batch(cfg, 5, 2)
    ids = batch.add_rigs([{k: dict(cfg, **RIG)[k] for k in hip_lib.RIG_FLOATS}])
    batch.assign_rigs([3], ids)
    for k in range(4):
        batch.new_images(*_frames(5, seqs, k, (0, 2, 3) if k == 3 else range(4)))
    assert batch.stats(1).frame_id == 2 and batch.stats(0).frame_id == 3
    yield batch, {}
    batch.close()


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _slot_planes(played, what, s):
    """the LEFT level-0 plane a view job shows of slot s, its segment, and dense_ref's planes of LEFT and RIGHT"""
    batch, cache = played
    if (what, s) not in cache:
        left = batch.export_views(what, [s], plane="left", level=0, pixel="gray8")
        right = batch.export_views(what, [s], plane="right", pixel="gray8")
        assert left.image(0) is not None and right.image(0) is not None, (what, s)
        l, r = np.ascontiguousarray(left.image(0)), np.ascontiguousarray(right.image(0))
        cache[(what, s)] = (l, left.segments[0].copy(), DR.planes(l, r, WIN["win"], WIN["search_x"], WIN["search_y"], STEP, DR.DISPARITY, True))
    return cache[(what, s)]


def _check_slot(tag, job, i, s, played, what):
    batch = played[0]
    seg = job.segments[i]
    left, vseg, planes = _slot_planes(played, what, s)
    cam = batch.slot_rig(s)[1]
    st = job.style
    assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, int(vseg["run"]), hip_lib.CLOUD_OK), (tag, s)
    assert (int(seg["frame_id"]), int(seg["keyframe_id"])) == (int(vseg["frame_id"]), int(vseg["keyframe_id"])), (tag, s)
    assert int(seg["first_point"]) == i * job.points_per_slot, (tag, s)
    assert seg["pose"].tobytes() == vseg["pose"].tobytes() and F(seg["time_stamp"]) == F(vseg["time_stamp"]), (tag, s)
    assert F(seg["baseline"]) == F(cam.baseline), (tag, s)
    rig = {k: getattr(cam, k) for k in CR.RIG_KEYS}
    ref, n = CR.cloud(left, planes, WIN["win"], st.step, rig, seg["pose"], st.frame, st.layout, st.min_disparity, st.max_depth, st.max_mean_cost)
    assert int(seg["n_points"]) == n, (tag, s, int(seg["n_points"]), n)
    raw = _np(job.points_buffer[i * job.points_per_slot:(i + 1) * job.points_per_slot])
    if st.layout == CR.ORGANIZED:
        assert raw.tobytes() == ref.tobytes(), (tag, s)
        assert job.organized(i).shape == (job.rows, job.cols) and job.organized(i).tobytes() == ref.tobytes()
        assert job.points(i).tobytes() == ref[ref["flags"] == 0].tobytes()
    else:
        assert raw[:n].tobytes() == ref.tobytes(), (tag, s)
        assert (raw[n:] == GUARD).all(), (tag, s, "a record beyond n_points was written")
        assert job.points(i).tobytes() == ref.tobytes()
    return n, planes


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_ctx_against_the_statement_on_its_views(played, what, device, monkeypatch):
    """5 slots in 2 groups; slot 3 has its own rig; slot 1 sat the last frame out; slot 4 is empty"""
    batch = played[0]
    for layout, frame, chunk in (("compact", "world", None), ("organized", "camera", None), ("organized", "world", "1"), ("compact", "world", "1")):
        if chunk:
            monkeypatch.setenv("SVO_CLOUD_CHUNK_SLOTS", chunk)      # a chunk per slot
            monkeypatch.setenv("SVO_CLOUD_TABLE_IMAGES", chunk)
        job = batch.submit_cloud(what, None, step=STEP, frame=frame, layout=layout, device=device, **WIN, **FILTER)
        job.wait()
        job.points_buffer.fill_(GUARD)
        job.submit().wait()
        kept = [_check_slot((what, layout, frame), job, s, s, played, what) for s in range(4)]
        for n, planes in kept:
            assert 0.1 * (planes[0] >= 0).sum() < n < 0.9 * (planes[0] >= 0).sum()           # the filter keeps some and drops some
        seg = job.segments[4]
        assert (int(seg["seq"]), int(seg["status"]), int(seg["frame_id"]), int(seg["keyframe_id"]), int(seg["n_points"])) == \
               (4, hip_lib.CLOUD_NONE, -1, -1, 0)
        assert int(seg["first_point"]) == 4 * job.points_per_slot and job.points(4) is None
        assert (_np(job.points_buffer[4 * job.points_per_slot:]) == GUARD).all()               # only its segment is written
    assert played[1][("frames", 1)][1]["frame_id"] == 2                                           # (the slot that sat out)
    # a named subset in non-ascending order, unfiltered: slot 3 uses its own rig
    job = batch.submit_cloud(what, [3, 0, 4, 2], step=STEP, device=device, **WIN)
    job.wait()
    job.points_buffer.fill_(GUARD)
    job.submit().wait()
    for i, s in ((0, 3), (1, 0), (3, 2)):
        n, planes = _check_slot("named", job, i, s, played, what)
        assert n == int((planes[0] >= 0).sum())
    assert batch.slot_rig(3)[0] != 0 and F(job.segments[0]["baseline"]) == F(23.5) and F(job.segments[1]["baseline"]) == F(20.0)
    assert int(job.segments[2]["status"]) == hip_lib.CLOUD_NONE
    assert (_np(job.points_buffer[2 * job.points_per_slot:3 * job.points_per_slot]) == GUARD).all()
    if what == "last_keyframes":
        assert all(int(job.segments[i]["keyframe_id"]) >= 0 for i in (0, 1, 3))


def _raw_submit(batch, what, seqs, n, style, dst, mem):
    arr = None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)
    return hip_lib.lib().svo_submit_export_cloud(batch._ctx, what, arr, n, None if style is None else C.byref(style),
                                                 None if dst is None else C.byref(dst), mem)


def _staging(points, host, slots):
    """what include/svo_hip.h states of a group's staging block"""
    up = lambda v: (v + 255) // 256 * 256
    slot = up(8 * points) + up(4 * ((points + 255) // 256)) + 256 + (16 * points if host else 0)
    chunk = max(1, (256 << 20) // slot)
    m = min(slots, chunk)
    return m * slot + up(4 * m)


def test_rejected_calls_queue_nothing_and_memory(tiny):
    cfg, seqs = tiny
    n_slots = 4
    batch, twin = _batch(cfg, n_slots, 2), _batch(cfg, n_slots, 2)
    for k in range(2):
        batch.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
        twin.new_images(*_frames(n_slots, seqs, k, range(n_slots)))
    assert batch.memory().device_bytes == twin.memory().device_bytes
    st = hip_lib.cloud_style(4, 7, 9, 2)
    cols, rows, per_slot = batch.cloud_size(st)
    seg = np.zeros(n_slots, hip_lib.CLOUD_SEGMENT_DTYPE)
    seg.view(np.uint8)[:] = GUARD
    px = torch.full((n_slots * per_slot + 2, 16), GUARD, dtype=torch.uint8).pin_memory()
    dpx = torch.full((n_slots * per_slot + 2, 16), GUARD, dtype=torch.uint8, device="cuda")
    dst = lambda p=px.data_ptr(), cap=n_slots * per_slot, s=seg.ctypes.data: hip_lib.CloudDst(s, p, cap)
    CAPACITY = _raw_submit(batch, 0, None, 0, st, dst(cap=n_slots * per_slot - 1), 0)
    assert CAPACITY not in (0, -1)
    calls = [(0, [4], 1, st, dst(), 0), (0, [-1], 1, st, dst(), 0), (0, [0, 1, 0], 3, st, dst(), 0), (0, [0], -1, st, dst(), 0),
             (2, None, 0, st, dst(), 0), (-1, None, 0, st, dst(), 0), (0, None, 0, st, dst(), 2), (0, None, 0, st, dst(), -1),
             (0, None, 0, None, dst(), 0), (0, None, 0, st, None, 0), (0, None, 0, st, dst(s=None), 0), (0, None, 0, st, dst(p=None), 0),
             (0, None, 0, st, dst(p=px.data_ptr() + 4), 0), (0, None, 0, st, dst(p=dpx.data_ptr() + 8), 1)]
    calls += [(0, None, 0, s, dst(), 0) for s in _bad_styles(st)]
    for c in calls:
        assert _raw_submit(batch, *c) == -1, c[:3]
        assert hip_lib.lib().svo_last_error()
    assert _raw_submit(batch, 1, [1, 2], 2, st, dst(cap=2 * per_slot - 1), 0) == CAPACITY
    batch.wait()
    assert (seg.view(np.uint8) == GUARD).all() and (px.numpy() == GUARD).all() and (dpx.cpu().numpy() == GUARD).all()
    # nothing else was queued and the ctx goes on: the next frame still tracks
    batch.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    twin.new_images(*_frames(n_slots, seqs, 2, range(n_slots)))
    for s in range(n_slots):
        assert batch.pose(s).tobytes() == twin.pose(s).tobytes() and batch.stats(s).frame_id == 2
    before = batch.memory().device_bytes
    # a disparity job's memory behaviour is as before: device mode allocates nothing, host mode its planes
    batch.export_disparity("frames", [3, 0], step=4, device=True, **WIN)
    assert batch.memory().device_bytes == before
    disp = batch.export_disparity("frames", None, step=4, **WIN)
    assert batch.memory().device_bytes - before == n_slots * disp.image_bytes
    before = batch.memory().device_bytes
    # the cloud job's own block, per group: device mode, then (outgrown) host mode, as the header states
    dev_job = batch.export_cloud("frames", [3, 0], step=4, device=True, **WIN)
    assert batch.memory().device_bytes - before == 2 * _staging(per_slot, False, 1)      # one named slot in each group
    host_job = batch.export_cloud("frames", None, step=4, **WIN)
    grown = batch.memory().device_bytes - before
    assert grown == 2 * _staging(per_slot, True, 2), grown                                # per group: its two slots
    batch.export_cloud("frames", None, step=4, **WIN)
    batch.export_cloud("frames", [1], step=8, layout="organized", **WIN)
    batch.export_cloud("frames", None, step=4, device=True, **WIN)
    assert batch.memory().device_bytes - before == grown                                  # not again on a second or a smaller job
    batch.export_disparity("frames", None, step=4, **WIN)
    assert batch.memory().device_bytes - before == grown
    assert twin.memory().device_bytes == before - n_slots * disp.image_bytes              # (a ctx that never asks has nothing more)
    assert int(host_job.segments[1]["n_points"]) > 0 and int(dev_job.segments[0]["n_points"]) > 0
    assert host_job.points(1).tobytes() == batch.export_cloud("frames", [1], step=4, device=True, **WIN).points(0).tobytes()
    batch.close(); twin.close()


def test_queue_order_and_no_side_effects(tiny):
    """a job queued between two frame sets sees the first and not the second; poses and keypoints are the same bits
    with and without cloud jobs between the steps, and so is the memory of a twin that never asks"""
    cfg, seqs = tiny
    batch, twin = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    jobs = []
    for k in range(4):
        L, R, ts = _frames(3, seqs, k, range(3))
        packed = batch.pack_images(L, R, ts)
        batch.submit_packed(packed)
        # not waited for: ordered with the frame sets (the views next to it show what it reads)
        jobs.append((batch.submit_cloud("frames", [2, 0], step=16, layout="organized", **WIN), batch.submit_views("frames", [2, 0], plane="left"),
                     batch.submit_views("frames", [2, 0], plane="right"), packed))
        twin.new_images(L, R, ts)
    batch.wait()
    rig = {k: cfg[k] for k in CR.RIG_KEYS}
    for k, (job, left, right, _) in enumerate(jobs):
        for i, s in enumerate((2, 0)):
            assert int(job.segments[i]["frame_id"]) == k == int(left.segments[i]["frame_id"])
            assert left.image(i).tobytes() == seqs[s][0][k].cpu().numpy().tobytes()
            l, r = np.ascontiguousarray(left.image(i)), np.ascontiguousarray(right.image(i))
            planes = DR.planes(l, r, 7, 9, 2, 16, DR.DISPARITY, True)
            ref, n = CR.cloud(l, planes, 7, 16, rig, job.segments[i]["pose"], CR.WORLD, CR.ORGANIZED)
            assert int(job.segments[i]["n_points"]) == n and job.organized(i).tobytes() == ref.tobytes(), (k, s)
            assert job.segments[i]["pose"].tobytes() == left.segments[i]["pose"].tobytes()
    for s in range(3):
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes()
    batch.close(); twin.close()
