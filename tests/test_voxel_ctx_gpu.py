"""The voxel maps inside a ctx on the GPU, byte for byte against tests/voxel_ref.py: fuse jobs queued behind every
frame set beside a checked organized cloud job at the same queue position (the statement fuses exactly those records),
exports in host and device mode, the statuses, what leaves a map alone, the memory a map costs, the chunked path and
tracking that does not notice any of it."""
import os

import numpy as np
import pytest
import torch

import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu
WIN = dict(win=7, search_x=9, search_y=2)
STEP = 4
VOXEL, LOG2 = 0.1, 16
FRAMES = 30                                         # (tiny, seed 1, motion 4: the second keyframe fires inside 30 frames)
LR = 1.5                                            # the tolerance of the left-right check of every cloud and fuse job here


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
    """tiny, 2 sequences of 30 frames of fast motion, gray on the device: shared, never changed"""
    out = []
    for seed in (1, 11):
        cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", FRAMES, seed, motion_scale=4.0)
        out.append((L, R, [float(t) for t in ts]))
    torch.cuda.synchronize()
    return cfg, out


def _frames(n, seqs, k, slots):
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for s in slots:
        L[s], R[s], ts[s] = seqs[s][0][k], seqs[s][1][k], seqs[s][2][k]
    return L, R, ts


def _export_bytes(batch, seqs=None, **kw):
    job = batch.export_voxel_maps(seqs, **kw)
    return job, [None if job.points(i) is None else job.points(i).tobytes() for i in range(len(job.segments))]


@pytest.fixture(scope="module")
def played(tiny):
    """3 slots in 2 groups, slots 0 and 1 play 30 frames, slot 2 stays empty; all three have a map. Behind every frame
    set a fuse job and a checked organized cloud job are queued, nothing is waited for until the end. A twin plays
    the same frames without any of it."""
    cfg, seqs = tiny
    batch, twin = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    batch.set_voxel_maps(VOXEL, LOG2)
    jobs = []
    for k in range(FRAMES):
        L, R, ts = _frames(3, seqs, k, (0, 1))
        packed = batch.pack_images(L, R, ts)
        batch.submit_packed(packed)
        fuse = batch.submit_fuse("last_keyframes", None, stamp=k + 1, lr_check=LR, step=STEP, max_depth=40.0, **WIN)
        cloud = batch.submit_cloud("last_keyframes", None, step=STEP, layout="organized", max_depth=40.0, lr_check=LR, **WIN)
        jobs.append((fuse, cloud, packed))
        twin.new_images(L, R, ts)
    batch.wait()
    # the statement, fed with the cloud jobs' records
    refs = [VR.Map(VOXEL, LOG2) for _ in range(3)]
    expect = []
    for k, (fuse, cloud, _) in enumerate(jobs):
        row = []
        for s in range(3):
            before = (refs[s].n_fused, refs[s].n_outside)
            org = cloud.organized(s)
            if org is not None:
                assert refs[s].admits(org.size)
                refs[s].fuse(org.ravel(), k + 1)
            row.append((org is not None, refs[s].n_fused - before[0], refs[s].n_outside - before[1], refs[s].n_voxels))
        expect.append(row)
    yield dict(cfg=cfg, seqs=seqs, batch=batch, twin=twin, jobs=jobs, refs=refs, expect=expect)
    batch.close(); twin.close()


def test_ordering_and_info(played):
    jobs, expect = played["jobs"], played["expect"]
    keyframes = set()
    for k, (fuse, cloud, _) in enumerate(jobs):
        for s in range(3):
            f, e = fuse.info[s], cloud.segments[s]
            shown, n_fused, n_outside, n_voxels = expect[k][s]
            assert (int(f["seq"]), int(f["run"]), int(f["frame_id"]), int(f["keyframe_id"])) == \
                   (s, int(e["run"]), int(e["frame_id"]), int(e["keyframe_id"])), (k, s)
            if s == 2:
                assert int(f["status"]) == hip_lib.FUSE_NONE and not shown and int(f["n_voxels"]) == 0        # the empty slot
                continue
            assert int(f["frame_id"]) == k and shown and int(f["status"]) == hip_lib.FUSE_OK, (k, s)
            assert f["pose"].tobytes() == e["pose"].tobytes(), (k, s)
            assert (int(f["n_offered"]), int(f["n_fused"]), int(f["n_outside"]), int(f["n_voxels"])) == \
                   (int(e["n_points"]), n_fused, n_outside, n_voxels), (k, s)
            assert int(f["n_fused"]) + int(f["n_outside"]) == int(f["n_offered"]) > 0
            keyframes.add((s, int(f["keyframe_id"])))
    assert len({kf for s, kf in keyframes if s == 0}) >= 2                  # at least two keyframes fired
    batch = played["batch"]
    for s in (0, 1):
        info = batch.voxel_map_info(s)
        ref = played["refs"][s]
        assert (info["n_voxels"], info["n_fused"], info["n_outside"], info["overflow"]) == (ref.n_voxels, ref.n_fused, ref.n_outside, 0)
        assert info["log2_capacity"] == LOG2 and np.float32(info["voxel"]) == np.float32(VOXEL)
    assert batch.voxel_map_info(2)["n_voxels"] == 0


@pytest.mark.parametrize("device", [False, True])
def test_parity_with_the_statement(played, device):
    batch, refs = played["batch"], played["refs"]
    # (a keyframe is fused again behind every frame it stays the newest for, so the counts are large: the filter that
    # tells voxels apart asks for the largest count there is)
    most = int(refs[0].acc[:, 0].max())
    for kw in (dict(), dict(min_count=most), dict(min_stamp=FRAMES - 1), dict(min_count=2, min_stamp=5)):
        job, got = _export_bytes(batch, None, device=device, **kw)
        for s in range(3):
            want = refs[s].extract(**kw)
            seg = job.segments[s]
            assert (int(seg["seq"]), int(seg["status"]), int(seg["n_points"]), int(seg["n_voxels"])) == \
                   (s, hip_lib.VOXEL_OK, len(want), refs[s].n_voxels), (kw, s)
            assert got[s] == want.tobytes(), (kw, s)
        assert len(refs[0].extract()) > 500 and 0 < len(refs[0].extract(min_count=most)) < len(refs[0].extract())
    # named out of order, into regions with room to spare: exactly [first_point, first_point + n_points) is written
    job = batch.submit_voxel_maps([1, 0], device=device, capacities=[refs[1].n_voxels + 7, refs[0].n_voxels]).wait()
    job.points_buffer.fill_(0xA5)
    job.submit().wait()
    raw = job.points_buffer.cpu().numpy()
    n1 = refs[1].n_voxels
    assert raw[:n1].tobytes() == refs[1].extract().tobytes() and (raw[n1:n1 + 7] == 0xA5).all()
    assert raw[n1 + 7:].tobytes() == refs[0].extract().tobytes()
    assert job.segments["first_point"].tolist() == [0, n1 + 7]


def test_tracking_is_unchanged(played):
    batch, twin = played["batch"], played["twin"]
    for s in (0, 1):
        a, b = batch.get_frame(s), twin.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        assert batch.get_trajectory(s).tobytes() == twin.get_trajectory(s).tobytes()


def test_memory(tiny):
    cfg, seqs = tiny
    a, b = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    base = a.memory().device_bytes
    assert b.memory().device_bytes == base
    b.set_voxel_maps(VOXEL, 12, seqs=[0, 2])
    assert b.memory().device_bytes == base + 2 * hip_lib.voxel_map_bytes(12)
    b.set_voxel_maps(VOXEL, 14, seqs=[2])                                  # replaced, not added
    assert b.memory().device_bytes == base + hip_lib.voxel_map_bytes(12) + hip_lib.voxel_map_bytes(14)
    for k in range(2):
        L, R, ts = _frames(3, seqs, k, (0, 1))
        a.new_images(L, R, ts); b.new_images(L, R, ts)
    assert b.memory().device_bytes == a.memory().device_bytes + hip_lib.voxel_map_bytes(12) + hip_lib.voxel_map_bytes(14)
    assert b.voxel_map_info(1) is None and b.voxel_map_info(0)["log2_capacity"] == 12
    b.set_voxel_maps(None)
    assert b.memory().device_bytes == a.memory().device_bytes and b.voxel_map_info(0) is None
    for bad in (dict(voxel=0.0), dict(voxel=float("nan")), dict(log2_capacity=9), dict(log2_capacity=27), dict(drop_flags=8), dict(seqs=[3]),
                dict(seqs=[1, 1])):
        with pytest.raises(hip_lib.SvoError, match="error -1:"):
            b.set_voxel_maps(**dict(dict(voxel=VOXEL, log2_capacity=12), **bad))
    assert b.memory().device_bytes == a.memory().device_bytes
    a.close(); b.close()


def test_statuses_chunks_and_what_leaves_a_map_alone(tiny, monkeypatch):
    cfg, seqs = tiny
    batch = _batch(cfg, 3, 2)
    for k in range(2):
        batch.new_images(*_frames(3, seqs, k, (0, 1)))
    kw = dict(step=STEP, max_depth=40.0, lr_check=LR, **WIN)
    batch.set_voxel_maps(VOXEL, LOG2, seqs=[0, 2])
    job = batch.fuse_clouds("frames", None, stamp=3, **kw)
    assert job.info["status"].tolist() == [hip_lib.FUSE_OK, hip_lib.FUSE_NO_MAP, hip_lib.FUSE_NONE]
    cloud = batch.export_cloud("frames", [0, 1], layout="organized", **kw)
    ref = VR.Map(VOXEL, LOG2)
    ref.fuse(cloud.organized(0).ravel(), 3)
    want = ref.extract().tobytes()
    exp, got = _export_bytes(batch)
    assert exp.segments["status"].tolist() == [hip_lib.VOXEL_OK, hip_lib.VOXEL_NO_MAP, hip_lib.VOXEL_OK]
    assert got[0] == want and got[1] is None and got[2] == b"" and ref.n_voxels > 100
    # too small: the count needed, nothing written
    small = batch.submit_voxel_maps([0], capacities=[ref.n_voxels - 1]).wait()
    small.points_buffer.fill_(0xA5)
    small.submit().wait()
    assert (int(small.segments[0]["status"]), int(small.segments[0]["n_voxels"]), int(small.segments[0]["n_points"])) == \
           (hip_lib.VOXEL_TOO_SMALL, ref.n_voxels, 0)
    assert (small.points_buffer.numpy() == 0xA5).all() and small.points(0) is None
    # restart, trim and more frames leave the map alone
    batch.restart([0])
    batch.trim_keyframes()
    batch.new_images(*_frames(3, seqs, 2, (0, 1)))
    assert _export_bytes(batch, [0])[1][0] == want and batch.voxel_map_info(0)["n_fused"] == ref.n_fused
    # the chunked path: both slots with a map, one slot per chunk, against one chunk
    batch.set_voxel_maps(VOXEL, LOG2)
    one = batch.fuse_clouds("frames", None, stamp=1, **kw)
    a = _export_bytes(batch)[1]
    batch.clear_voxel_maps()
    assert [batch.voxel_map_info(s)["n_voxels"] for s in range(3)] == [0, 0, 0] and _export_bytes(batch)[1] == [b"", b"", b""]
    monkeypatch.setenv("SVO_CLOUD_CHUNK_SLOTS", "1")
    two = batch.fuse_clouds("frames", None, stamp=1, **kw)
    monkeypatch.delenv("SVO_CLOUD_CHUNK_SLOTS")
    assert _export_bytes(batch)[1] == a and one.info.tobytes() == two.info.tobytes() and len(a[0]) > 0 and len(a[1]) > 0
    cloud = batch.export_cloud("frames", [0, 1], layout="organized", **kw)
    for s in (0, 1):
        r = VR.Map(VOXEL, LOG2)
        r.fuse(cloud.organized(s).ravel(), 1)
        assert a[s] == r.extract().tobytes()
    # a tiny map: FULL, nothing fused, the ctx goes on
    batch.set_voxel_maps(VOXEL, 10, seqs=[0])
    full = batch.fuse_clouds("frames", None, stamp=2, **kw)
    assert full.info["status"].tolist() == [hip_lib.FUSE_FULL, hip_lib.FUSE_OK, hip_lib.FUSE_NONE]
    assert batch.voxel_map_info(0)["n_fused"] == 0 and int(full.info[0]["n_voxels"]) == 0
    assert batch.voxel_map_info(1)["n_fused"] == 2 * int(one.info[1]["n_fused"])
    # rejections queue nothing
    for bad in (dict(frame="camera"), dict(layout="organized")):
        style = hip_lib.cloud_style(STEP, frame=bad.get("frame", "world"), layout=bad.get("layout", "compact"))
        info = np.zeros(3, hip_lib.FUSE_INFO_DTYPE)
        assert hip_lib.lib().svo_submit_fuse_clouds(batch._ctx, 1, None, 3, hip_lib.C.byref(style), None, 1, info.ctypes.data) == -1
    batch.new_images(*_frames(3, seqs, 3, (0, 1)))
    batch.close()


def test_fuse_new_keyframes(tiny):
    cfg, seqs = tiny
    batch = _batch(cfg, 2, 1)
    batch.set_voxel_maps(VOXEL, LOG2)
    fused = []
    for k in range(FRAMES):
        batch.new_images(*_frames(2, seqs, k, (0, 1)))
        job = batch.fuse_new_keyframes(step=STEP, **WIN)
        if job is not None:
            fused += [(int(f["seq"]), int(f["keyframe_id"]), int(f["status"])) for f in job.info]
    assert len(fused) == len(set(fused)) and all(st == hip_lib.FUSE_OK for _, _, st in fused)     # every keyframe once
    for s in range(2):
        assert sorted(kf for q, kf, _ in fused if q == s) == list(range(batch.keyframe_range(s).count))
    assert batch.fuse_new_keyframes(step=STEP, **WIN) is None
    batch.close()
