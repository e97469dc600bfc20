"""The prune job inside a ctx on the GPU, byte for byte against tests/voxel_prune_ref.py: a ctx that prunes behind every
fuse, with nothing waited for, never goes full where its plain twin does, and its maps are the statement's; queue order
against the same calls with waits; the pose-mode centre against the pose of a cloud job at the same queue position;
given centres; the statuses across two groups in mixed order; the memory a prune costs; the rejections; and tracking
that does not notice any of it.

The frames are the `tiny` sequence cut to its central 256 x 192 pixels (the principal point moved with them): at the
largest step, 16, a cloud then has 16 x 12 = 192 points, a quarter of the 768 entries a map of 1 << 10 may hold, so a
map that keeps what its last three fuses reached always admits the next one."""
import os

import numpy as np
import pytest
import torch

import voxel_prune_ref as PR
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.jobs import Prune
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu
W, H, X0, Y0 = 256, 192, 32, 24
WIN = dict(win=7, search_x=9, search_y=2)
STEP = 16
POINTS = (W // STEP) * (H // STEP)
VOXEL, LOG2 = 0.1, 10
FRAMES = 30
KEEP_STAMPS = 3


def _batch(cfg, n_slots, groups):
    old = os.environ.get("SVO_GROUPS")
    os.environ["SVO_GROUPS"] = str(groups)
    try:
        b = StereoSlamBatch(cfg, W, H, n_slots)
    finally:
        if old is None:
            del os.environ["SVO_GROUPS"]
        else:
            os.environ["SVO_GROUPS"] = old
    assert b.groups() == groups
    return b


@pytest.fixture(scope="module")
def tiny():
    """tiny cut to 256 x 192, 2 sequences of 30 frames of fast motion, gray on the device: shared, never changed"""
    out = []
    for seed in (1, 11):
        cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", FRAMES, seed, motion_scale=4.0)
        cut = lambda imgs: [x[Y0:Y0 + H, X0:X0 + W].contiguous() for x in imgs]
        out.append((cut(L), cut(R), [float(t) for t in ts]))
    torch.cuda.synchronize()
    cfg = dict(cfg, width=W, height=H, cx=cfg["cx"] - X0, cy=cfg["cy"] - Y0)
    return cfg, out


def _frames(n, seqs, k, slots):
    """slots: {slot: sequence}"""
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for s, q in slots.items():
        L[s], R[s], ts[s] = seqs[q][0][k], seqs[q][1][k], seqs[q][2][k]
    return L, R, ts


def _export_bytes(batch, seqs=None, **kw):
    job = batch.export_voxel_maps(seqs, **kw)
    return [None if job.points(i) is None else job.points(i).tobytes() for i in range(len(job.segments))]


def _min_stamp(stamp):
    return max(0, stamp - KEEP_STAMPS + 1)


def test_the_shapes_are_what_the_docstring_says():
    assert POINTS == 192 and 4 * POINTS <= VR.load_limit(LOG2) == 768 and (KEEP_STAMPS + 1) * POINTS <= VR.load_limit(LOG2)


@pytest.fixture(scope="module")
def played(tiny):
    """3 slots in 2 groups, slots 0 and 1 play, slot 2 stays empty; all have a map of 1 << 10 entries. `plain` fuses the
    current frame's cloud behind every frame set; `pruned` does the same, queues a prune that keeps the last
    KEEP_STAMPS stamps behind every fuse and an organized cloud job for the statement, and waits for nothing until
    the end."""
    cfg, seqs = tiny
    plain, pruned = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    kw = dict(step=STEP, **WIN)
    for b in (plain, pruned):
        b.set_voxel_maps(VOXEL, LOG2)
    jobs, plain_jobs = [], []
    for k in range(FRAMES):
        L, R, ts = _frames(3, seqs, k, {0: 0, 1: 1})
        packed = pruned.pack_images(L, R, ts)
        pruned.submit_packed(packed)
        fuse = pruned.submit_fuse("frames", None, stamp=k + 1, **kw)
        cloud = pruned.submit_cloud("frames", None, layout="organized", **kw)
        prune = pruned.submit_prune(None, min_stamp=_min_stamp(k + 1))
        jobs.append((fuse, cloud, prune, packed))
        plain.new_images(L, R, ts)
        plain_jobs.append(plain.fuse_clouds("frames", None, stamp=k + 1, **kw))
    pruned.wait()
    # the statement: each ctx's maps from the cloud jobs' records
    refs = [VR.Map(VOXEL, LOG2) for _ in range(3)]
    refs_plain = [VR.Map(VOXEL, LOG2) for _ in range(3)]
    expect = []
    for k, (fuse, cloud, prune, _) in enumerate(jobs):
        row = []
        for s in range(3):
            org = cloud.organized(s)
            fused = full_plain = False
            if org is not None:
                assert org.size == POINTS
                fused = refs[s].admits(POINTS)
                if fused:
                    refs[s].fuse(org.ravel(), k + 1)
                full_plain = not refs_plain[s].admits(POINTS)
                if not full_plain:
                    refs_plain[s].fuse(org.ravel(), k + 1)
            n_before, n_kept = PR.prune(refs[s], min_stamp=_min_stamp(k + 1))
            row.append((org is not None, fused, full_plain, n_before, n_kept))
        expect.append(row)
    yield dict(cfg=cfg, seqs=seqs, plain=plain, pruned=pruned, jobs=jobs, plain_jobs=plain_jobs, refs=refs, refs_plain=refs_plain, expect=expect)
    plain.close(); pruned.close()


def test_a_pruned_map_runs_without_end(played):
    jobs, plain_jobs, expect = played["jobs"], played["plain_jobs"], played["expect"]
    went_full = set()
    removed = 0
    for k, (fuse, cloud, prune, _) in enumerate(jobs):
        for s in range(3):
            shown, fused, full_plain, n_before, n_kept = expect[k][s]
            f, p, q = fuse.info[s], prune.info[s], plain_jobs[k].info[s]
            assert (int(p["seq"]), int(p["run"]), int(p["frame_id"])) == (s, int(f["run"]), int(f["frame_id"])), (k, s)
            if s == 2:                                                   # the empty slot: its map stays empty, no box: pruned all the same
                assert (int(f["status"]), int(p["status"]), int(p["n_before"]), int(p["n_kept"])) == (hip_lib.FUSE_NONE, hip_lib.PRUNE_OK, 0, 0)
                continue
            assert shown and fused and int(f["status"]) == hip_lib.FUSE_OK, (k, s)              # the pruning ctx never goes full
            assert int(q["status"]) == (hip_lib.FUSE_FULL if full_plain else hip_lib.FUSE_OK), (k, s)
            went_full |= {s} if full_plain else set()
            assert (int(p["status"]), int(p["n_before"]), int(p["n_kept"])) == (hip_lib.PRUNE_OK, n_before, n_kept), (k, s)
            assert int(f["n_voxels"]) == n_before and p["center"].tolist() == [0, 0, 0] and p["center_voxel"].tolist() == [0, 0, 0]
            removed += n_before - n_kept
    assert went_full == {0, 1} and removed > 0                           # the plain ctx does go full, on both playing slots
    pruned, plain = played["pruned"], played["plain"]
    for kw in (dict(), dict(min_count=2), dict(min_stamp=FRAMES)):
        got, got_plain = _export_bytes(pruned, **kw), _export_bytes(plain, **kw)
        for s in range(3):
            assert got[s] == played["refs"][s].extract(**kw).tobytes(), (kw, s)
            assert got_plain[s] == played["refs_plain"][s].extract(**kw).tobytes(), (kw, s)
    for s in (0, 1):
        info, ref = pruned.voxel_map_info(s), played["refs"][s]
        assert (info["n_voxels"], info["n_fused"], info["n_outside"], info["overflow"]) == (ref.n_voxels, ref.n_fused, ref.n_outside, 0)
        assert 0 < ref.n_voxels <= KEEP_STAMPS * POINTS and ref.n_fused > VR.load_limit(LOG2)   # cumulative: more than a map ever held


def test_tracking_is_unchanged(played):
    a_, b_ = played["pruned"], played["plain"]
    for s in (0, 1):
        a, b = a_.get_frame(s), b_.get_frame(s)
        assert (a.kps2d.tobytes(), a.kps3d.tobytes(), a.info.tobytes(), a.pose.tobytes()) == \
               (b.kps2d.tobytes(), b.kps3d.tobytes(), b.info.tobytes(), b.pose.tobytes())
        assert a_.get_trajectory(s).tobytes() == b_.get_trajectory(s).tobytes()


def _radius_that_splits(points, center, voxel):
    """a radius in voxels with entries on both sides of the box, and metres that floor to it"""
    d = np.abs(np.floor(np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float64) / voxel) - np.floor(np.asarray(center, np.float64) / voxel)).max(1)
    rv = int(np.median(d))
    return rv, (rv + 0.5) * float(np.float32(voxel))


def test_pose_mode_and_queue_order(tiny):
    """fuse, prune around the camera, fuse, export, with no wait between them, against the same calls with waits and the
    statement; the centre is the pose of a cloud job at the same queue position"""
    cfg, seqs = tiny
    kw = dict(step=STEP, **WIN)
    a, b = _batch(cfg, 2, 1), _batch(cfg, 2, 1)
    for x in (a, b):
        x.set_voxel_maps(VOXEL, LOG2)
        for k in range(3):
            x.new_images(*_frames(2, seqs, k, {0: 0, 1: 1}))
    first = a.fuse_clouds("frames", None, stamp=1, **kw)
    cloud0 = a.export_cloud("frames", None, layout="organized", **kw)
    pts = a.export_voxel_maps([0]).points(0)
    rv, metres = _radius_that_splits(pts, cloud0.segments[0]["pose"][:3], VOXEL)
    b.fuse_clouds("frames", None, stamp=1, **kw)
    nxt = _frames(2, seqs, 3, {0: 0, 1: 1})
    # a: nothing waited for
    packed = a.pack_images(*nxt)
    a.submit_packed(packed)
    cloud = a.submit_cloud("frames", None, layout="organized", **kw)
    prune = Prune(a, None, hip_lib.voxel_keep(min_count=1, radius=rv), "pose").submit()
    fuse = a.submit_fuse("frames", None, stamp=2, **kw)
    exp = a.submit_voxel_maps(None, capacities=VR.load_limit(LOG2))
    a.wait()
    # b: the same calls, each waited for
    b.new_images(*nxt)
    prune_b = b.prune_voxel_maps(None, radius=metres, center="pose", min_count=1)
    fuse_b = b.fuse_clouds("frames", None, stamp=2, **kw)
    exp_b = b.export_voxel_maps(None, capacities=VR.load_limit(LOG2))
    assert prune.keep.radius == rv and prune.center_mode == hip_lib.PRUNE_CENTER_POSE
    assert prune.info.tobytes() == prune_b.info.tobytes() and fuse.info.tobytes() == fuse_b.info.tobytes()
    split = 0
    for s in (0, 1):
        ref = VR.Map(VOXEL, LOG2)
        ref.fuse(cloud0.organized(s).ravel(), 1)
        pose = cloud.segments[s]["pose"]
        p = prune.info[s]
        assert int(p["status"]) == hip_lib.PRUNE_OK and p["center"].tobytes() == pose[:3].tobytes()      # the cloud job's camera centre
        assert tuple(p["center_voxel"].tolist()) == PR.center_voxel(pose[:3], VOXEL)
        assert cloud.segments[s]["pose"].tobytes() != cloud0.segments[s]["pose"].tobytes()               # the pose at ITS queue position
        n_before, n_kept = PR.prune(ref, min_count=1, center=tuple(float(x) for x in pose[:3]), radius=rv)
        assert (int(p["n_before"]), int(p["n_kept"])) == (n_before, n_kept)
        split += 0 < n_kept < n_before
        assert ref.admits(POINTS)
        ref.fuse(cloud.organized(s).ravel(), 2)
        assert int(fuse.info[s]["n_voxels"]) == ref.n_voxels
        assert exp.points(s).tobytes() == exp_b.points(s).tobytes() == ref.extract().tobytes()
    assert split >= 1
    a.close(); b.close()


def test_statuses_given_centres_memory_and_rejections(tiny):
    cfg, seqs = tiny
    kw = dict(step=STEP, **WIN)
    batch = _batch(cfg, 4, 2)                                            # groups: slots 0, 1 and slots 2, 3
    for k in range(3):
        batch.new_images(*_frames(4, seqs, k, {0: 0, 2: 1}))             # slots 0 and 2 play, 1 and 3 stay empty
    batch.set_voxel_maps(VOXEL, LOG2, seqs=[0, 1, 2])                    # slot 3 has no map
    batch.fuse_clouds("frames", None, stamp=1, **kw)
    before = batch.export_voxel_maps([0, 2])
    refs = {}
    for i, s in enumerate((0, 2)):
        cloud = batch.export_cloud("frames", [s], layout="organized", **kw)
        refs[s] = VR.Map(VOXEL, LOG2)
        refs[s].fuse(cloud.organized(0).ravel(), 1)
        assert before.points(i).tobytes() == refs[s].extract().tobytes() and refs[s].n_voxels > 20
    base = batch.memory().device_bytes
    # pose mode, named across the two groups in mixed order: no map, ok, no pose (an empty slot), ok
    job = batch.prune_voxel_maps([3, 0, 1, 2], radius=1e6, center="pose")
    assert job.info["seq"].tolist() == [3, 0, 1, 2] and job.info["frame_id"].tolist() == [-1, 2, -1, 2]
    assert job.info["status"].tolist() == [hip_lib.PRUNE_NO_MAP, hip_lib.PRUNE_OK, hip_lib.PRUNE_NO_POSE, hip_lib.PRUNE_OK]
    assert job.info["n_before"].tolist() == job.info["n_kept"].tolist() == [0, refs[0].n_voxels, 0, refs[2].n_voxels]
    # memory: per group that had a slot to prune, the tile offsets and the staging of its largest map, and nothing else
    up256 = lambda v: (v + 255) // 256 * 256
    block = lambda n_voxels: up256(4 * ((1 << LOG2) // 256 + 1)) + up256(40 * n_voxels)
    grown = base + block(refs[0].n_voxels) + block(refs[2].n_voxels)
    assert batch.memory().device_bytes == grown
    # given centres, one per named slot, in another order: each slot against the statement
    centers, rvs = {}, {}
    for i, s in enumerate((0, 2)):
        pose = batch.get_frame(s).pose
        centers[s] = [float(x) for x in np.asarray(pose, np.float32).ravel()[:3]]
        rvs[s] = _radius_that_splits(before.points(i), centers[s], VOXEL)
    metres = rvs[0][1]
    rv = int(np.floor(metres / float(np.float32(VOXEL))))
    job = batch.prune_voxel_maps([2, 1, 0], radius=metres, center=[centers[2], [0.5, 0.5, 0.5], centers[0]], min_count=1)
    assert job.info["status"].tolist() == [hip_lib.PRUNE_OK] * 3 and job.keep.radius == rv == rvs[0][0]
    for i, s in ((0, 2), (2, 0)):
        p = job.info[i]
        n_before, n_kept = PR.prune(refs[s], min_count=1, center=centers[s], radius=rv)
        assert (int(p["n_before"]), int(p["n_kept"])) == (n_before, n_kept) and p["center"].tolist() == centers[s]
        assert tuple(p["center_voxel"].tolist()) == PR.center_voxel(centers[s], VOXEL)
    assert 0 < refs[0].n_voxels < int(job.info[2]["n_before"])
    assert _export_bytes(batch, [0, 2]) == [refs[0].extract().tobytes(), refs[2].extract().tobytes()]
    assert batch.memory().device_bytes == grown                          # smaller maps now: the blocks stay
    # one xyz for all
    job = batch.prune_voxel_maps([0], radius=0.0, center=centers[0])
    assert job.centers is not None and int(job.info[0]["n_kept"]) == PR.prune(refs[0], center=centers[0], radius=0)[1]
    # rejections queue nothing and change nothing
    lib, C = hip_lib.lib(), hip_lib.C
    info = np.zeros(4, hip_lib.PRUNE_INFO_DTYPE)
    keep = hip_lib.voxel_keep(radius=2, center=(0.5, 0.5, 0.5))
    call = lambda seqs, n, k, mode, centers, inf: lib.svo_submit_prune_voxel_maps(batch._ctx, seqs, n, k, mode, centers, inf)
    arr = lambda v: (C.c_int * len(v))(*v)
    assert call(None, 4, None, 0, None, info.ctypes.data) == -1                                          # no keep rule
    assert call(None, 4, C.byref(keep), 0, None, None) == -1                                             # no info
    assert call(None, 4, C.byref(keep), 2, None, info.ctypes.data) == -1                                 # no such mode
    assert call(arr([0, 0]), 2, C.byref(keep), 0, None, info.ctypes.data) == -1                          # named twice
    assert call(arr([4]), 1, C.byref(keep), 0, None, info.ctypes.data) == -1                             # out of range
    bad = hip_lib.voxel_keep(radius=2)
    bad._reserved[1] = 1
    assert call(None, 4, C.byref(bad), 0, None, info.ctypes.data) == -1
    for x in (float("nan"), float("inf"), 1e30, 1048576.0 * 0.1 * 1.01):
        assert call(None, 4, C.byref(hip_lib.voxel_keep(radius=2, center=(0.0, x, 0.0))), 0, None, info.ctypes.data) == -1
        per_slot = np.zeros((4, 3), np.float32)
        per_slot[2, 2] = x
        assert call(None, 4, C.byref(keep), 0, per_slot.ctypes.data, info.ctypes.data) == -1
    per_slot = np.zeros((4, 3), np.float32)
    per_slot[3, 0] = np.nan                                               # a slot without a map has no key rule to be outside of
    assert call(None, 4, C.byref(keep), 0, per_slot.ctypes.data, info.ctypes.data) == 0
    batch.wait()
    assert info["status"].tolist() == [hip_lib.PRUNE_OK, hip_lib.PRUNE_OK, hip_lib.PRUNE_OK, hip_lib.PRUNE_NO_MAP]
    assert call(None, 4, C.byref(hip_lib.voxel_keep(radius=-1, center=(np.nan, 0, 0))), 1, None, info.ctypes.data) == 0   # no box: not read
    batch.wait()
    assert info["status"].tolist() == [hip_lib.PRUNE_OK, hip_lib.PRUNE_NO_POSE, hip_lib.PRUNE_OK, hip_lib.PRUNE_NO_MAP]
    assert batch.memory().device_bytes == grown
    batch.new_images(*_frames(4, seqs, 3, {0: 0, 2: 1}))
    batch.close()


def test_fuse_new_keyframes_with_a_prune(tiny):
    cfg, seqs = tiny
    batch = _batch(cfg, 2, 1)
    batch.set_voxel_maps(VOXEL, 16)
    seen, last_min = 0, {}
    for k in range(FRAMES):
        batch.new_images(*_frames(2, seqs, k, {0: 0, 1: 1}))
        job = batch.fuse_new_keyframes(step=STEP, prune=dict(keep_stamps=2, min_count=1), **WIN)
        if job is None:
            continue
        seen += 1
        assert job.prune.keep.min_stamp == max(0, job.stamp - 1) and job.prune.seqs == [int(f["seq"]) for f in job.info]
        last_min.update({s: job.prune.keep.min_stamp for s in job.prune.seqs})
        assert all(int(p["status"]) == hip_lib.PRUNE_OK and int(p["n_before"]) == int(f["n_voxels"]) for p, f in zip(job.prune.info, job.info))
    assert seen >= 2
    for s in range(2):                                                    # what the slot's last prune kept is all there is
        everything = batch.export_voxel_maps([s], min_stamp=0).points(0)
        assert len(everything) > 0 and everything.tobytes() == batch.export_voxel_maps([s], min_stamp=last_min[s]).points(0).tobytes()
    batch.close()
