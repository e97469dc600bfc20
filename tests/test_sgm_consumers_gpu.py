"""The SGM forms of the cloud's consumers on the GPU (include/svo_hip.h, "sgm fusion", "sgm scene clouds", "sgm ar
occlusion"), byte for byte: each consumer against its own statement (tests/voxel_ref.py,
tests/scene_cloud_ref.py, tests/ar_occlusion_ref.py) fed with the records of the SGM cloud job at the same queue
position; sgm == NULL against the existing entries; the memory, the rejections, resubmission, and tracking that does not
notice any of it. No comparison has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import ar_occlusion_ref as OR
import test_ar_occlusion_gpu as ARO
import test_scene_cloud_gpu as SCN
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import ArPictures, Scenes
from test_sgm_lr_gpu import _bad_checks, _bad_params, _sgm_slot
from test_voxel_ctx_gpu import _batch, _export_bytes, _frames

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xA5
WIN = dict(win=7, search_x=9, search_y=2)
STEP = 4
VOXEL, LOG2 = 0.1, 16
FRAMES = 30                                         # (tiny, seed 1, motion 4: the second keyframe fires inside 30 frames)
SGM = dict(p1=32, p2=256, cost_cap=4095)
CHECKS = (1.0, None)                                # the SGM map's own check at tolerance 1, and unchecked
MESHES, INSTANCES = ARO.MESHES, ARO.INSTANCES
OCCLUSION = dict(step=4, margin=0.05, max_depth=20.0)
DENSE = SCN.DENSE


def _sgm(check):
    return dict(SGM, lr_check=check)


def _tracking(batch, s):
    f = batch.get_frame(s)
    return (f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes(), f.pose.tobytes(), batch.get_trajectory(s).tobytes())


@pytest.fixture(scope="module")
def tiny():
    """tiny, 2 sequences of 30 frames of fast motion, gray on the device: shared, never changed"""
    out = []
    for seed in (1, 11):
        cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", FRAMES, seed, motion_scale=4.0)
        out.append((L, R, [float(t) for t in ts]))
    torch.cuda.synchronize()
    return cfg, out


@pytest.fixture(scope="module")
def played(tiny):
    """3 slots in 2 groups: slots 0 and 1 after 4 frames, slot 2 empty; and a twin that runs none of the jobs of this
    file. The tests only read them."""
    cfg, seqs = tiny
    batch, twin = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    for k in range(4):
        for b in (batch, twin):
            b.new_images(*_frames(3, seqs, k, (0, 1)))
    yield batch, twin
    for s in (0, 1):                                                        # every test of the file has run by now
        assert _tracking(batch, s) == _tracking(twin, s)
    batch.close(); twin.close()


# ------------------------------------------------------------------ fuse

@pytest.fixture(scope="module", params=CHECKS, ids=("checked", "unchecked"))
def fused(tiny, request):
    """3 slots in 2 groups, slots 0 and 1 play 30 frames, slot 2 stays empty; all three have a map. Behind every frame
    set an SGM fuse job and an organized world-frame SGM cloud job with the same arguments are queued, nothing is
    waited for until the end. A twin plays the same frames without any of it."""
    cfg, seqs = tiny
    check = request.param
    batch, twin = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    batch.set_voxel_maps(VOXEL, LOG2)
    jobs = []
    for k in range(FRAMES):
        L, R, ts = _frames(3, seqs, k, (0, 1))
        packed = batch.pack_images(L, R, ts)
        batch.submit_packed(packed)
        fuse = batch.submit_fuse("last_keyframes", None, stamp=k + 1, sgm=_sgm(check), step=STEP, max_depth=40.0, **WIN)
        cloud = batch.submit_cloud("last_keyframes", None, step=STEP, layout="organized", max_depth=40.0, sgm=_sgm(check), **WIN)
        jobs.append((fuse, cloud, packed))
        twin.new_images(L, R, ts)
    batch.wait()
    refs = [VR.Map(VOXEL, LOG2) for _ in range(3)]
    for k, (fuse, cloud, _) in enumerate(jobs):
        for s in range(3):
            org = cloud.organized(s)
            if org is not None:
                assert refs[s].admits(org.size)
                refs[s].fuse(org.ravel(), k + 1)
    yield dict(check=check, batch=batch, twin=twin, jobs=jobs, refs=refs)
    batch.close(); twin.close()


def test_fuse_info_is_the_cloud_segments(fused):
    keyframes = set()
    for k, (fuse, cloud, _) in enumerate(fused["jobs"]):
        assert fuse.sgm is not None and cloud.sgm is not None and (fuse.check is None) == (fused["check"] is None)
        for s in range(3):
            f, e = fuse.info[s], cloud.segments[s]
            assert (int(f["seq"]), int(f["run"]), int(f["frame_id"]), int(f["keyframe_id"])) == \
                   (s, int(e["run"]), int(e["frame_id"]), int(e["keyframe_id"])), (k, s)
            if s == 2:
                assert int(f["status"]) == hip_lib.FUSE_NONE and int(e["status"]) == hip_lib.CLOUD_NONE and int(f["n_voxels"]) == 0
                continue
            assert int(f["frame_id"]) == k and int(f["status"]) == hip_lib.FUSE_OK and int(e["status"]) == hip_lib.CLOUD_OK, (k, s)
            assert f["pose"].tobytes() == e["pose"].tobytes(), (k, s)
            assert int(f["n_offered"]) == int(e["n_points"]) > 0, (k, s)                    # (not vacuous: every delivered slot offers)
            assert int(f["n_fused"]) + int(f["n_outside"]) == int(f["n_offered"])
            keyframes.add((s, int(f["keyframe_id"])))
    assert len({kf for s, kf in keyframes if s == 0}) >= 2                                  # at least two keyframes fused in one slot
    batch = fused["batch"]
    for s in (0, 1):
        info, ref = batch.voxel_map_info(s), fused["refs"][s]
        assert (info["n_voxels"], info["n_fused"], info["n_outside"], info["overflow"]) == (ref.n_voxels, ref.n_fused, ref.n_outside, 0)
        last = fused["jobs"][-1][0].info[s]
        assert int(last["n_voxels"]) == ref.n_voxels
    assert batch.voxel_map_info(2)["n_voxels"] == 0


@pytest.mark.parametrize("device", [False, True])
def test_fused_maps_against_the_statement(fused, device):
    batch, refs = fused["batch"], fused["refs"]
    for kw in (dict(), dict(min_count=2, min_stamp=5)):
        job, got = _export_bytes(batch, None, device=device, **kw)
        for s in range(3):
            want = refs[s].extract(**kw)
            seg = job.segments[s]
            assert (int(seg["seq"]), int(seg["status"]), int(seg["n_points"]), int(seg["n_voxels"])) == \
                   (s, hip_lib.VOXEL_OK, len(want), refs[s].n_voxels), (kw, s)
            assert got[s] == want.tobytes(), (kw, s)
    assert len(refs[0].extract()) > 500 and len(refs[2].extract()) == 0


def test_fuse_leaves_tracking_alone(fused):
    for s in (0, 1):
        assert _tracking(fused["batch"], s) == _tracking(fused["twin"], s)
        assert fused["batch"].num_keyframes(s) == fused["twin"].num_keyframes(s)


def test_fuse_chunks_of_one_and_fuse_new_keyframes(tiny, monkeypatch):
    cfg, seqs = tiny
    batch, hand = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    for k in range(2):
        for b in (batch, hand):
            b.new_images(*_frames(3, seqs, k, (0, 1)))
    kw = dict(step=STEP, max_depth=40.0, sgm=_sgm(1.0), **WIN)
    batch.set_voxel_maps(VOXEL, LOG2)
    one = batch.fuse_clouds("frames", None, stamp=1, **kw)
    a = _export_bytes(batch)[1]
    batch.clear_voxel_maps()
    monkeypatch.setenv("SVO_SGM_CHUNK_SLOTS", "1")
    monkeypatch.setenv("SVO_CLOUD_CHUNK_SLOTS", "1")
    two = batch.fuse_clouds("frames", None, stamp=1, **kw)
    monkeypatch.delenv("SVO_SGM_CHUNK_SLOTS")
    monkeypatch.delenv("SVO_CLOUD_CHUNK_SLOTS")
    assert _export_bytes(batch)[1] == a and one.info.tobytes() == two.info.tobytes() and len(a[0]) > 0 and len(a[1]) > 0 and a[2] == b""
    assert one.info["status"].tolist() == [hip_lib.FUSE_OK, hip_lib.FUSE_OK, hip_lib.FUSE_NONE]
    cloud = batch.export_cloud("frames", [0, 1], layout="organized", **kw)
    for s in (0, 1):
        r = VR.Map(VOXEL, LOG2)
        r.fuse(cloud.organized(s).ravel(), 1)
        assert a[s] == r.extract().tobytes()
    # a tiny map is FULL as before: settled ahead of any launch, nothing fused, the ctx goes on
    batch.set_voxel_maps(VOXEL, 10, seqs=[0])
    full = batch.fuse_clouds("frames", None, stamp=2, **kw)
    assert full.info["status"].tolist() == [hip_lib.FUSE_FULL, hip_lib.FUSE_OK, hip_lib.FUSE_NONE] and batch.voxel_map_info(0)["n_fused"] == 0
    # fuse_new_keyframes with sgm and a prune is the two jobs queued by hand
    prune = dict(min_count=1, radius=3.0)
    batch.set_voxel_maps(VOXEL, LOG2)
    hand.set_voxel_maps(VOXEL, LOG2)
    job = batch.fuse_new_keyframes(prune=prune, **kw)
    by_hand = hand.submit_fuse("last_keyframes", [0, 1], stamp=1, **kw)
    pruned = hand.submit_prune([0, 1], **prune)
    hand.wait()
    assert job.sgm is not None and job.stamp == 1 and job.seqs == [0, 1]
    assert job.info.tobytes() == by_hand.info.tobytes() and job.prune.info.tobytes() == pruned.info.tobytes()
    assert _export_bytes(batch)[1] == _export_bytes(hand)[1] and int(job.prune.info[0]["n_kept"]) > 0
    assert batch.fuse_new_keyframes(prune=prune, **kw) is None
    batch.close(); hand.close()


# ------------------------------------------------------------------ the scene's live layer

@pytest.mark.parametrize("check", CHECKS, ids=("checked", "unchecked"))
@pytest.mark.parametrize("what", ("frames", "last_keyframes"))
def test_scene_live_layer(played, what, check, monkeypatch):
    """a camera behind each slot's pose; host and device mode; each named slot against the restatement fed with the
    getters and the records of the SGM cloud job at the same queue position; chunks and span tables of one; an extra
    span as well"""
    batch, _ = played
    named = [1, 0]
    cams = [SCN._behind(batch.pose(s)) for s in named]
    dense = dict(DENSE, what=what, sgm=_sgm(check))
    cloud = batch.submit_cloud(what, named, step=DENSE["step"], layout="organized", sgm=_sgm(check))
    host = batch.submit_scenes(named, camera=cams, style=SCN._style_ctx(), dense=dense)
    dev = batch.submit_scenes(named, camera=cams, style=SCN._style_ctx("rgba8"), dense=dense, device=True)
    batch.wait()
    assert host.sgm is not None and (host._clouds[0].check.lr, host._clouds[0].check.max_lr_diff) == ((1, 1.0) if check else (0, 0.0))
    imgs = [SCN._check_slot((what, check, "host"), host, i, s, batch, cams[i], cloud) for i, s in enumerate(named)]
    for i in range(2):
        assert SCN._image(dev, i)[:, :, :3].tobytes() == imgs[i].tobytes() and (SCN._image(dev, i)[:, :, 3] == 255).all()
    assert dev.cloud_info.tobytes() == host.cloud_info.tobytes()
    assert all(int(c["status"]) == hip_lib.CLOUD_OK and int(c["live_points"]) > 0 for c in host.cloud_info)
    monkeypatch.setenv("SVO_SCENE_CHUNK_SLOTS", "1")
    monkeypatch.setenv("SVO_SCENE_TABLE_SPANS", "1")
    for device in (False, True):
        again = batch.export_scenes(named, camera=cams, style=SCN._style_ctx(), dense=dense, device=device)
        px = again.pixels.cpu().numpy() if device else again.pixels
        assert px[:host.capacity].tobytes() == host.pixels[:host.capacity].tobytes()
        assert again.segments.tobytes() == host.segments.tobytes() and again.cloud_info.tobytes() == host.cloud_info.tobytes()
    monkeypatch.delenv("SVO_SCENE_CHUNK_SLOTS")
    monkeypatch.delenv("SVO_SCENE_TABLE_SPANS")
    # with an extra span as well: the compact device cloud of another job; the empty slot in the middle writes its segment only
    comp = batch.export_cloud("last_keyframes", [0], step=8, layout="compact", device=True)
    n = int(comp.segments[0]["n_points"])
    assert n > 100
    three = [1, 2, 0]
    cams3 = [cams[0], SCN._behind(np.zeros(6)), cams[1]]
    cloud3 = batch.submit_cloud(what, three, step=DENSE["step"], layout="organized", sgm=_sgm(check))
    both = batch.submit_scenes(three, camera=cams3, style=SCN._style_ctx(), dense=dense, clouds=[None, None, (comp.points_buffer.data_ptr(), n)])
    batch.wait()
    SCN._check_slot("no extra", both, 0, 1, batch, cams3[0], cloud3)
    SCN._check_slot("extra", both, 2, 0, batch, cams3[2], cloud3, comp.points(0)[:n])
    assert both.image(0).tobytes() == imgs[0].tobytes() and both.image(2).tobytes() != imgs[1].tobytes()
    assert (int(both.segments[1]["status"]), int(both.cloud_info[1]["status"]), int(cloud3.segments[1]["status"])) == \
           (hip_lib.SCENE_NONE, hip_lib.CLOUD_NONE, hip_lib.CLOUD_NONE)


# ------------------------------------------------------------------ AR occlusion

def _ar_statement(batch, s, style, occlusion, cloud, i):
    """(image, covered, hidden, kept) of slot s by the statement: ar_occlusion_ref applied to the view job's left plane,
    svo_ar_camera_of_pose of the pose, and the organized camera-frame records of named slot i of the SGM cloud job"""
    gray = batch.export_views("frames", [s], plane="left", level=0, pixel="gray8").image(0)
    o = dict(ArPictures.OCCLUSION_DEFAULTS, **occlusion)
    _, cam = batch.slot_rig(s)
    camera = np.frombuffer(bytes(hip_lib.ar_camera_of_pose(batch.pose(s), cam)), F)
    draws = [(np.asarray(m, F), MESHES[k][0], MESHES[k][1], None, rgb) for m, k, rgb in INSTANCES]
    hidden = hip_lib.AR_HIDDEN.index(o["hidden"]) if isinstance(o["hidden"], str) else o["hidden"]
    img, covered, hid = OR.render(np.asarray(gray), camera, draws, tuple(style.light), style.ambient, style.near, style.pixel,
                                  (cloud.organized(i).reshape(-1), cloud.cols, cloud.rows, o["step"]), hidden, o["alpha"], o["margin"],
                                  o["drop_flags"])
    return img, covered, hid, int(cloud.segments[i]["n_points"])


def _check_ar(tag, job, named, batch, occlusion, cloud):
    """every named slot of the job against the statement; returns [(covered, hidden)] of the delivered ones"""
    out = []
    for i, s in enumerate(named):
        seg, vis = job.segments[i], job.visibility[i]
        if int(seg["frame_id"]) < 0:
            assert (int(seg["status"]), int(vis["status"]), int(vis["covered"]), int(vis["hidden"]), int(vis["occluder_points"])) == \
                   (hip_lib.AR_NONE, hip_lib.CLOUD_NONE, 0, 0, 0), (tag, s)
            assert job.image(i) is None and int(cloud.segments[i]["status"]) == hip_lib.CLOUD_NONE
            continue
        img, covered, hid, kept = _ar_statement(batch, s, job.style, occlusion, cloud, i)
        got = job.image(i)
        got = got.cpu().numpy() if job.device_mode else got
        print(tag, "slot", s, "covered", int(vis["covered"]), covered, "hidden", int(vis["hidden"]), hid, "occluder points",
              int(vis["occluder_points"]), kept, "pixels off", int((got != img).any(axis=2).sum()))
        assert (int(seg["status"]), int(vis["status"])) == (hip_lib.AR_OK, hip_lib.CLOUD_OK), (tag, s)
        assert (int(vis["covered"]), int(vis["hidden"]), int(vis["occluder_points"]), int(vis["_pad"])) == (covered, hid, kept, 0), (tag, s)
        assert kept > 0 and got.tobytes() == img.tobytes(), (tag, s, int((got != img).any(axis=2).sum()))
        out.append((covered, hid))
    return out


def _occluder_cloud(batch, named, occlusion):
    o = dict(ArPictures.OCCLUSION_DEFAULTS, **occlusion)
    return batch.submit_cloud("frames", named, step=o["step"], frame="camera", layout="organized", max_depth=o["max_depth"], sgm=o["sgm"])


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("hidden,alpha,pixel", (("drop", 128, "rgb8"), ("dim", 96, "rgba8")))
def test_ar_occluded_against_the_statement(played, hidden, alpha, pixel, device, monkeypatch):
    batch, _ = played
    named = [1, 2, 0]
    for check in CHECKS:
        occ = dict(OCCLUSION, hidden=hidden, alpha=alpha, sgm=_sgm(check))
        cloud = _occluder_cloud(batch, named, occ)
        job = ArPictures(batch, named, hip_lib.ar_style(pixel=pixel), MESHES, INSTANCES, None, device, occ)
        job._buf.fill_(FILL)
        job.submit().wait()
        assert job.sgm is not None and job._occlusion.check.lr == (1 if check else 0)
        counts = _check_ar((hidden, check), job, named, batch, occ, cloud)
        # the box straddles the floor: somewhere a part of it is hidden and a part is seen
        assert any(0 < h < c for c, h in counts), counts
        px = job.pixels.cpu().numpy() if device else job.pixels
        assert (px[job.image_bytes:2 * job.image_bytes] == FILL).all()        # the empty slot wrote only its segment
        monkeypatch.setenv("SVO_AR_CHUNK_SLOTS", "1")
        again = batch.export_ar(MESHES, INSTANCES, named, device=device, style=job.style, occlusion=occ)
        monkeypatch.delenv("SVO_AR_CHUNK_SLOTS")
        px2 = again.pixels.cpu().numpy() if device else again.pixels
        for i in (0, 2):
            assert px2[i * job.image_bytes:(i + 1) * job.image_bytes].tobytes() == px[i * job.image_bytes:(i + 1) * job.image_bytes].tobytes()
        assert again.visibility.tobytes() == job.visibility.tobytes() and again.segments.tobytes() == job.segments.tobytes()


# ------------------------------------------------------------------ the check bites, and SGM changes something

def test_the_check_drops_points_and_sgm_differs_from_winner_takes_all(played, tiny):
    batch, _ = played
    kw = dict(step=STEP, layout="organized", max_depth=40.0, **WIN)
    checked, unchecked = batch.submit_cloud("frames", None, sgm=_sgm(1.0), **kw), batch.submit_cloud("frames", None, sgm=_sgm(None), **kw)
    batch.wait()
    kept = [(int(a["n_points"]), int(b["n_points"])) for a, b in zip(checked.segments[:2], unchecked.segments[:2])]
    print("kept, checked and unchecked:", kept)
    assert any(0 < a < b for a, b in kept), kept
    # the scene picture and the AR picture
    cams = [SCN._behind(batch.pose(s)) for s in (0, 1)]
    wta = batch.submit_scenes([0, 1], camera=cams, style=SCN._style_ctx(), dense=dict(DENSE))
    sgm = batch.submit_scenes([0, 1], camera=cams, style=SCN._style_ctx(), dense=dict(DENSE, sgm=_sgm(None)))
    ar_wta = batch.submit_ar(MESHES, INSTANCES, [0, 1], occlusion=dict(OCCLUSION))
    ar_sgm = batch.submit_ar(MESHES, INSTANCES, [0, 1], occlusion=dict(OCCLUSION, sgm=_sgm(None)))
    batch.wait()
    assert wta.segments.tobytes() == sgm.segments.tobytes() and any(wta.image(i).tobytes() != sgm.image(i).tobytes() for i in range(2))
    assert ar_wta.segments.tobytes() == ar_sgm.segments.tobytes()
    assert any(ar_wta.image(i).tobytes() != ar_sgm.image(i).tobytes() or int(ar_wta.visibility[i]["hidden"]) != int(ar_sgm.visibility[i]["hidden"])
               for i in range(2))
    # the map
    cfg, seqs = tiny
    own = _batch(cfg, 2, 1)
    own.new_images(*_frames(2, seqs, 0, (0, 1)))
    own.set_voxel_maps(VOXEL, LOG2)
    fuse_kw = dict(step=STEP, max_depth=40.0, **WIN)
    own.fuse_clouds("frames", None, stamp=1, **fuse_kw)
    a = _export_bytes(own)[1]
    own.clear_voxel_maps()
    own.fuse_clouds("frames", None, stamp=1, sgm=_sgm(None), **fuse_kw)
    b = _export_bytes(own)[1]
    assert all(len(x) > 0 for x in a + b) and any(x != y for x, y in zip(a, b))
    own.close()


# ------------------------------------------------------------------ sgm == NULL, memory, rejections

def _arr(seqs):
    return None if seqs is None else (C.c_int * max(len(seqs), 1))(*seqs)


def _raw_fuse(batch, style, sgm, check, info, what=1, seqs=None):
    return hip_lib.lib().svo_submit_fuse_clouds_sgm(batch._ctx, what, _arr(seqs), 0 if seqs is None else len(seqs), C.byref(style),
                                                    None if sgm is None else C.byref(sgm), None if check is None else C.byref(check), 1,
                                                    info.ctypes.data)


def _raw_scenes(batch, sc, clouds, sgm, seqs=None, mem=hip_lib.MEM_HOST, style=None):
    return hip_lib.lib().svo_submit_export_scenes_clouds_sgm(batch._ctx, _arr(seqs), 0 if seqs is None else len(seqs),
                                                             C.byref(sc.style if style is None else style), None if clouds is None else C.byref(clouds),
                                                             None if sgm is None else C.byref(sgm), sc._cams, C.byref(sc._dst), mem)


def _raw_ar(batch, job, occlusion, sgm, seqs=None, mem=hip_lib.MEM_HOST):
    return hip_lib.lib().svo_submit_export_ar_occluded_sgm(batch._ctx, _arr(seqs), 0 if seqs is None else len(seqs), C.byref(job.style),
                                                           None if occlusion is None else C.byref(occlusion), None if sgm is None else C.byref(sgm),
                                                           job._meshes, job._n_meshes, job._inst, job._first, job._n_inst, C.byref(job._dst), mem)


def test_without_sgm_the_new_entries_are_the_existing_ones(tiny):
    """sgm == NULL through each new entry: the bytes, segments and infos of the existing entry, and the memory of a twin
    ctx that only ran the existing entries"""
    cfg, seqs = tiny
    new, old = _batch(cfg, 3, 2), _batch(cfg, 3, 2)
    for k in range(2):
        for b in (new, old):
            b.new_images(*_frames(3, seqs, k, (0, 1)))
    for b in (new, old):
        b.set_voxel_maps(VOXEL, LOG2)
    check = hip_lib.stereo_check(True, 1.5)
    style = hip_lib.cloud_style(STEP, 7, 9, 2, "world", "compact", 0.0, 40.0, 0.0)
    want = old.fuse_clouds("frames", None, stamp=1, lr_check=1.5, step=STEP, max_depth=40.0, **WIN)
    info = np.zeros(3, hip_lib.FUSE_INFO_DTYPE)
    assert _raw_fuse(new, style, None, check, info, what=0) == 0
    new.wait()
    assert info.tobytes() == want.info.tobytes() and _export_bytes(new)[1] == _export_bytes(old)[1]
    cams = [SCN._behind(old.pose(s) if s < 2 else np.zeros(6)) for s in range(3)]
    dense = dict(DENSE, lr_check=1.0)
    want = old.export_scenes(camera=cams, style=SCN._style_ctx(), dense=dense)
    sc = Scenes(new, None, SCN._style_ctx(), cams, False, dense)
    sc._buf.fill_(FILL)
    assert _raw_scenes(new, sc, sc._clouds[0], None) == 0
    new.wait()
    for i in (0, 1):
        assert sc.image(i).tobytes() == want.image(i).tobytes()
    assert sc.segments.tobytes() == want.segments.tobytes() and sc.cloud_info.tobytes() == want.cloud_info.tobytes()
    assert (sc.pixels[2 * sc.image_bytes:] == FILL).all()
    occ = dict(ARO.OCCLUSION)
    want = old.export_ar(MESHES, INSTANCES, occlusion=occ)
    job = ArPictures(new, None, hip_lib.ar_style(), MESHES, INSTANCES, None, False, occ)
    assert _raw_ar(new, job, job._occlusion, None) == 0
    new.wait()
    for i in (0, 1):
        assert job.image(i).tobytes() == want.image(i).tobytes()
    assert job.segments.tobytes() == want.segments.tobytes() and job.visibility.tobytes() == want.visibility.tobytes()
    assert new.memory().device_bytes == old.memory().device_bytes
    # live == 0 / on == 0 with params: the plain jobs; the params are checked all the same
    plain = old.export_scenes(camera=cams, style=SCN._style_ctx())
    nothing, keep = hip_lib.scene_clouds(live=False, point_size=4)
    p = hip_lib.sgm_params(**SGM)
    bad = hip_lib.sgm_params(**SGM)
    bad.paths = 8
    sc = Scenes(new, None, SCN._style_ctx(), cams, False)
    assert _raw_scenes(new, sc, nothing, bad) == -1 and _raw_scenes(new, sc, None, bad) == -1 and _raw_scenes(new, sc, nothing, p) == 0
    assert _raw_scenes(new, sc, None, p) == 0
    new.wait()
    assert sc.image(0).tobytes() == plain.image(0).tobytes() and sc.segments.tobytes() == plain.segments.tobytes()
    plain = old.export_ar(MESHES, INSTANCES)
    off = hip_lib.ar_occlusion(on=False, step=0)
    job = ArPictures(new, None, hip_lib.ar_style(), MESHES, INSTANCES, None, False)
    assert _raw_ar(new, job, off, bad) == -1 and _raw_ar(new, job, None, bad) == -1 and _raw_ar(new, job, off, p) == 0
    new.wait()
    assert job.image(1).tobytes() == plain.image(1).tobytes() and job.segments.tobytes() == plain.segments.tobytes()
    assert new.memory().device_bytes == old.memory().device_bytes
    new.close(); old.close()


def _one_of_each(batch, cams, **how):
    """one fuse job, one scene job with a live layer and one occluded AR job, all in device mode"""
    batch.fuse_clouds("frames", None, stamp=1, step=STEP, **WIN, **how)
    batch.export_scenes(camera=cams, style=SCN._style_ctx(), device=True, dense=dict(DENSE, step=STEP, **WIN, **how))
    batch.export_ar(MESHES, INSTANCES, device=True, occlusion=dict(OCCLUSION, **WIN, **how))


def test_memory_is_the_stated_sum(tiny):
    """A ctx after one job of each kind in its checked SGM form holds what a ctx holds after the unchecked winner-takes-all
    jobs, plus the block of "sgm" for its delivered slots at the checked slot size: no reverse block, which the checked
    winner-takes-all jobs add instead."""
    cfg, seqs = tiny
    wta, wta_checked, sgm = (_batch(cfg, 2, 1) for _ in range(3))
    for b in (wta, wta_checked, sgm):
        b.new_images(*_frames(2, seqs, 0, (0, 1)))
        b.set_voxel_maps(VOXEL, LOG2)
    base = wta.memory().device_bytes
    assert wta_checked.memory().device_bytes == sgm.memory().device_bytes == base
    cams = [SCN._behind(wta.pose(s)) for s in range(2)]
    _one_of_each(wta, cams)
    _one_of_each(wta_checked, cams, lr_check=1.0)
    _one_of_each(sgm, cams, sgm=_sgm(1.0))
    cols, rows, width = cfg["width"] // STEP, cfg["height"] // STEP, cfg["width"]
    up = lambda v: (v + 255) // 256 * 256
    assert wta_checked.memory().device_bytes - wta.memory().device_bytes == 2 * up(rows * width * 4)        # reverse_bytes per slot
    assert sgm.memory().device_bytes - wta.memory().device_bytes == 2 * _sgm_slot(cols, rows, WIN["search_x"] + 1, True)
    grown = sgm.memory().device_bytes
    _one_of_each(sgm, cams, sgm=_sgm(1.0))
    _one_of_each(sgm, cams, sgm=_sgm(None))
    assert sgm.memory().device_bytes == grown                                                           # not again
    for b in (wta, wta_checked, sgm):
        b.close()


def test_rejected_calls_queue_nothing(tiny):
    cfg, seqs = tiny
    n = 2
    batch = _batch(cfg, n, 1)
    batch.new_images(*_frames(n, seqs, 0, (0, 1)))
    batch.set_voxel_maps(VOXEL, LOG2)
    good, good_check = hip_lib.sgm_params(**SGM), hip_lib.stereo_check(True, 1.0)
    bad_params = [p for p in _bad_params() if p is not None]               # (a NULL sgm is the existing entry)
    bad_checks = _bad_checks(True)
    wide = dict(WIN, search_x=64)
    # fuse
    info = np.zeros(n, hip_lib.FUSE_INFO_DTYPE)
    info.view(np.uint8)[:] = FILL
    style = hip_lib.cloud_style(STEP, 7, 9, 2)
    for p in bad_params:
        assert _raw_fuse(batch, style, p, good_check, info) == -1 and _raw_fuse(batch, style, p, None, info) == -1
        assert b"svo_submit_fuse_clouds_sgm" in hip_lib.lib().svo_last_error()
    for c in bad_checks:
        assert _raw_fuse(batch, style, good, c, info) == -1, (c.lr, c.max_lr_diff)
    for st in (hip_lib.cloud_style(STEP, 7, 64, 2), hip_lib.cloud_style(STEP, 36, 9, 2), hip_lib.cloud_style(STEP, 7, 9, 2, "camera"),
               hip_lib.cloud_style(STEP, 7, 9, 2, "world", "organized"), hip_lib.cloud_style(0, 7, 9, 2)):
        assert _raw_fuse(batch, st, good, good_check, info) == -1
    assert _raw_fuse(batch, style, good, good_check, info, what=2) == -1 and _raw_fuse(batch, style, good, good_check, info, seqs=[0, 0]) == -1
    assert hip_lib.lib().svo_submit_fuse_clouds_sgm(batch._ctx, 1, None, 0, C.byref(style), C.byref(good), None, 1, None) == -1
    # scenes
    cams = [SCN._behind(batch.pose(s)) for s in range(n)]
    sc = Scenes(batch, None, SCN._style_ctx(), cams, False, dict(DENSE, step=STEP, **WIN, sgm=_sgm(1.0)))
    sc._buf.fill_(FILL); sc._seg.view(np.uint8)[:] = FILL; sc._info.view(np.uint8)[:] = FILL

    def clouds(check=None, **kw):
        c, keep = hip_lib.scene_clouds(live=True, info=sc._info, **dict(dict(step=STEP, **WIN), **kw))
        c.check = good_check if check is None else check
        return c

    for p in bad_params:
        assert _raw_scenes(batch, sc, clouds(), p) == -1
        assert b"svo_submit_export_scenes_clouds_sgm" in hip_lib.lib().svo_last_error()
    for c in bad_checks:
        assert _raw_scenes(batch, sc, clouds(check=c), good) == -1, (c.lr, c.max_lr_diff)
    assert _raw_scenes(batch, sc, clouds(**wide), good) == -1 and _raw_scenes(batch, sc, clouds(win=36), good) == -1
    assert _raw_scenes(batch, sc, clouds(point_size=0), good) == -1
    assert _raw_scenes(batch, sc, clouds(), good, seqs=[0, 0]) == -1 and _raw_scenes(batch, sc, clouds(), good, mem=2) == -1
    assert _raw_scenes(batch, sc, clouds(), good, style=hip_lib.scene_style(cols=0)) == -1
    # AR
    vis = np.zeros(n, hip_lib.AR_VISIBILITY_DTYPE)
    vis.view(np.uint8)[:] = FILL
    job = ArPictures(batch, None, hip_lib.ar_style(), MESHES, INSTANCES, None, False)
    job._buf.fill_(FILL); job._seg.view(np.uint8)[:] = FILL

    def occlusion(check=None, **kw):
        o = hip_lib.ar_occlusion(info=vis, **dict(dict(step=STEP, **WIN), **kw))
        o.check = good_check if check is None else check
        return o

    for p in bad_params:
        assert _raw_ar(batch, job, occlusion(), p) == -1
        assert b"svo_submit_export_ar_occluded_sgm" in hip_lib.lib().svo_last_error()
    for c in bad_checks:
        assert _raw_ar(batch, job, occlusion(check=c), good) == -1, (c.lr, c.max_lr_diff)
    assert _raw_ar(batch, job, occlusion(**wide), good) == -1 and _raw_ar(batch, job, occlusion(win=36), good) == -1
    assert _raw_ar(batch, job, occlusion(alpha=257), good) == -1 and _raw_ar(batch, job, occlusion(margin=-0.1), good) == -1
    assert _raw_ar(batch, job, occlusion(), good, seqs=[0, 0]) == -1 and _raw_ar(batch, job, occlusion(), good, mem=2) == -1
    # the Python layers refuse the two checks together before anything reaches the library
    with pytest.raises(ValueError, match="sgm dict"):
        batch.submit_fuse(lr_check=1.0, sgm=True, step=STEP, **WIN)
    with pytest.raises(ValueError, match="dense"):
        batch.submit_scenes(camera=cams, style=SCN._style_ctx(), dense=dict(DENSE, lr_check=1.0, sgm=True))
    with pytest.raises(ValueError, match="occlusion"):
        batch.submit_ar(MESHES, INSTANCES, occlusion=dict(OCCLUSION, lr_check=1.0, sgm=True))
    # a job queued behind all that: nothing was queued before it, and the ctx goes on
    last = batch.submit_voxel_maps(capacities=16)
    batch.wait()
    assert [int(s["n_voxels"]) for s in last.segments] == [0, 0] and batch.voxel_map_info(0)["n_fused"] == 0
    assert (info.view(np.uint8) == FILL).all() and (vis.view(np.uint8) == FILL).all()
    assert (sc._seg.view(np.uint8) == FILL).all() and (sc._info.view(np.uint8) == FILL).all() and (sc.pixels == FILL).all()
    assert (job._seg.view(np.uint8) == FILL).all() and (job.pixels == FILL).all()
    assert _raw_fuse(batch, style, good, good_check, info) == 0 and _raw_scenes(batch, sc, clouds(), good) == 0
    assert _raw_ar(batch, job, occlusion(), good) == 0
    batch.wait()
    assert [int(f["status"]) for f in info] == [hip_lib.FUSE_OK] * n and all(int(f["n_offered"]) > 0 for f in info)
    assert [int(s["status"]) for s in sc.segments] == [hip_lib.SCENE_OK] * n and [int(v["status"]) for v in vis] == [hip_lib.CLOUD_OK] * n
    batch.close()


# ------------------------------------------------------------------ resubmission

def test_resubmitted_jobs_give_the_same_bytes(played, tiny):
    batch, _ = played
    cams = [SCN._behind(batch.pose(s)) for s in range(2)]
    state = lambda job, info: ([bytes(job.image(i).cpu().numpy() if job.device_mode else job.image(i)) for i in range(2)],
                               job.segments.tobytes(), getattr(job, info).tobytes())
    for device in (False, True):
        sc = batch.export_scenes([0, 1], camera=cams, style=SCN._style_ctx(), device=device, dense=dict(DENSE, sgm=_sgm(1.0)))
        ar = batch.export_ar(MESHES, INSTANCES, [0, 1], device=device, occlusion=dict(OCCLUSION, sgm=_sgm(1.0)))
        for job, info in ((sc, "cloud_info"), (ar, "visibility")):
            first = state(job, info)
            job._buf.fill_(FILL)
            getattr(job, info).view(np.uint8)[:] = FILL
            job.submit().wait()
            assert state(job, info) == first and job.sgm is not None
            assert all(int(x["status"]) == hip_lib.CLOUD_OK for x in getattr(job, info))
    cfg, seqs = tiny
    own = _batch(cfg, 2, 1)
    own.new_images(*_frames(2, seqs, 0, (0, 1)))
    own.set_voxel_maps(VOXEL, LOG2)
    fuse = own.fuse_clouds("frames", None, stamp=1, sgm=_sgm(1.0), step=STEP, **WIN)
    first, maps = fuse.info.copy(), _export_bytes(own)[1]
    own.clear_voxel_maps()
    fuse.info.view(np.uint8)[:] = FILL
    fuse.submit().wait()
    assert fuse.info.tobytes() == first.tobytes() and _export_bytes(own)[1] == maps and all(len(m) > 0 for m in maps)
    own.close()
