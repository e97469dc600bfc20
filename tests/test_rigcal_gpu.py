"""Rectification maps built on the GPU from calibrations. The stage entry (svo_build_rectify_maps) against the f64
statement (tests/rigcal_ref.py) bit for bit, ragged sizes, planes between canaries, many cameras in one launch; the
ctx entries (svo_ctx_add_rigs_calibrated, svo_ctx_set_calibration: the fused kernel, no float plane) against a ctx
given the stage entry's float maps, byte for byte down to the rectified images; and bad calls, which change nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import rigcal_ref as RC
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.hip_lib import CameraCalibration, SvoError, lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu

CANARY = 0x5ca1ab1e                                       # (as float32: a finite value no map holds)
SIZES = [(1, 1), (5, 3), (64, 64), (70, 67), (130, 65)]   # ragged tiles both ways, widths that are no multiple of 4


@pytest.fixture(scope="module")
def handle():
    h = hip_lib.Handle(0, 16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def reference():
    """the statement's maps, computed once per (case, size)"""
    memo = {}

    def get(name, w, h):
        if (name, w, h) not in memo:
            memo[name, w, h] = RC.maps(RC.cases()[name], w, h)
        return memo[name, w, h]
    return get


def _cal(name):
    return CameraCalibration.from_mats(*RC.cases()[name])


def _build(handle, names, w, h, pad):
    """the maps of the named cases in ONE call, every plane inside one buffer with `pad` canary words before, between
    and after the planes; returns [(map_x, map_y)] numpy and checks the canaries"""
    n, plane = len(names), w * h
    words = pad + 2 * n * (plane + pad)
    buf = torch.full((words,), CANARY, dtype=torch.int32, device="cuda")
    at = lambda k: pad + k * (plane + pad)
    out = [tuple(buf[at(2 * c + s):at(2 * c + s) + plane].view(torch.float32).view(h, w) for s in range(2)) for c in range(n)]
    handle.build_rectify_maps([_cal(nm) for nm in names], w, h, out=out)
    handle.synchronize()
    host = buf.cpu().numpy()
    keep = np.ones(words, bool)
    for k in range(2 * n):
        keep[at(k):at(k) + plane] = False
    assert (host[keep] == CANARY).all(), "a canary word was written"
    return [tuple(host[at(2 * c + s):at(2 * c + s) + plane].view(np.float32).reshape(h, w) for s in range(2)) for c in range(n)]


def _same(tag, got, ref):
    for axis, g, r in zip("xy", got, ref):
        assert RC.same_bits(g, r), (tag, axis, int(np.sum(g.view(np.uint32) != r.view(np.uint32))))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_entry_equals_the_statement(handle, reference, size):
    """every case at this size, one call each; the planes 16-byte aligned (pad 64) and not (pad 1)"""
    w, h = size
    for k, name in enumerate(RC.cases()):
        got = _build(handle, [name], w, h, pad=1 if k % 2 else 64)
        _same(name, got[0], reference(name, w, h))
    for name in ("euroc_left", "horizon"):                # (each case sees both alignments at the vector width)
        if w % 4 == 0:
            _same(name, _build(handle, [name], w, h, pad=1)[0], reference(name, w, h))
            _same(name, _build(handle, [name], w, h, pad=64)[0], reference(name, w, h))


def test_stage_entry_equals_the_statement_on_euroc_full_size(handle):
    cams, (w, h) = RC.euroc()
    got = _build(handle, ["euroc_left", "euroc_right"], w, h, pad=64)
    for g, side in zip(got, ("LEFT", "RIGHT")):
        _same(side, g, RC.maps(cams[side], w, h))


def test_the_horizon_case_is_not_finite_in_its_column(handle, reference):
    """(the comparison above includes pixels that are not finite: this is where they are)"""
    mx, my = _build(handle, ["horizon"], 70, 67, pad=64)[0]
    bad = ~np.isfinite(mx) | ~np.isfinite(my)
    assert bad[:, RC.HORIZON_COLUMN].all() and bad.sum() == 67


def test_many_cameras_in_one_call_equal_lone_calls(handle, reference):
    names = ["rational", "horizon", "euroc_right", "outside", "tangential"]
    w, h = 70, 67
    batch = _build(handle, names, w, h, pad=64)
    for name, got in zip(names, batch):
        lone = _build(handle, [name], w, h, pad=64)[0]
        _same(name, got, lone)
        _same(name, got, reference(name, w, h))


def test_stage_entry_rejects_bad_calls(handle):
    w, h = 5, 3
    planes = [torch.full((h, w), 7.0, device="cuda") for _ in range(4)]
    px = (C.c_void_p * 2)(planes[0].data_ptr(), planes[1].data_ptr())
    py = (C.c_void_p * 2)(planes[2].data_ptr(), planes[3].data_ptr())
    hole = (C.c_void_p * 2)(planes[0].data_ptr(), None)
    K, D, R, P = RC.cases()["tangential"]
    good, singular = _cal("tangential"), CameraCalibration.from_mats(K, D, R, np.zeros((3, 3)))
    f = lib().svo_build_rectify_maps
    two = lambda a, b: (CameraCalibration * 2)(a, b)
    assert f(handle._h, -1, two(good, good), w, h, px, py) == -1
    assert f(handle._h, 2, two(good, good), 0, h, px, py) == -1
    assert f(handle._h, 2, two(good, singular), w, h, px, py) == -1
    assert f(handle._h, 2, two(good, good), w, h, hole, py) == -1
    assert f(handle._h, 2, None, w, h, px, py) == -1
    handle.synchronize()
    assert all((p == 7.0).all().item() for p in planes), "nothing was launched"
    assert f(handle._h, 0, None, w, h, None, None) == 0
    assert f(handle._h, 2, two(good, good), w, h, px, py) == 0
    handle.synchronize()
    assert RC.same_bits(planes[1].cpu().numpy(), RC.maps(RC.cases()["tangential"], w, h)[0])


# ------------------------------------------------------------------------------------------ ctx

CFG = synth.CONFIGS["tiny"]
W, H = CFG["width"], CFG["height"]
N_FRAMES = 5                                              # (the shortest run of test_rigs_gpu.py's mixed-rig test)


def _tiny_cal(seed, **d):
    """an EuRoC-like camera of the `tiny` size: radial and tangential distortion, a small rotation, P against a
    slightly longer K"""
    s = float(seed)
    K = [[208.0 + s, 0, 162.5 - 0.5 * s], [0, 207.25 + 0.5 * s, 116.5 + s], [0, 0, 1]]
    D = [d.get("k1", -0.28 + 0.01 * s), 0.07, 2.0e-4 * s, -1.5e-4, 0.0]
    return CameraCalibration.from_mats(K, D, RC.rotation(0.003 * s, -0.002, 0.001 * s), [[200.0, 0, 160.0], [0, 200.0, 120.0], [0, 0, 1]])


def _rig_cals():
    """(left, right) of rig 0 (set_calibration) and of the three added rigs; rig 2's left camera is the horizon case"""
    return [(_tiny_cal(1), _tiny_cal(2)), (_tiny_cal(3), _tiny_cal(-1)), (_cal("horizon"), _tiny_cal(-2)),
            (_tiny_cal(-3, k1=-0.31), _tiny_cal(4))]


RIG_FLOATS = [dict(), dict(fx=212.0, fy=212.0, cx=151.5, cy=127.25, baseline=23.5), dict(baseline=21.0),
              dict(k1=-0.01, p1=1.0e-4)]


def _rig(k, **extra):
    return dict({n: dict(CFG, **RIG_FLOATS[k])[n] for n in hip_lib.RIG_FLOATS}, **extra)


@pytest.fixture(scope="module")
def frames():
    """4 slots x N_FRAMES raw frames (noise-textured synthetic renders, every frame different), device tensors"""
    return [synth.make_sequence_gpu("tiny", N_FRAMES, 1200 + s, motion_scale=8.0) for s in range(4)]


def _state(slam, seqs):
    """what the ctx reports about the slots now, as comparable bytes: pose, keypoints, stats, and the level-0 images
    the tracker worked on (the rectified left and right frame)"""
    out = []
    for s in seqs:
        f = slam.get_frame(s)
        out.append((f.pose.tobytes(), f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes(), bytes(slam.stats(s)),
                    slam.num_keyframes(s)))
    for plane in ("left", "right"):
        v = slam.export_views("frames", seqs, plane=plane, level=0, pixel="gray8")
        out.append([v.image(i).tobytes() for i in range(len(seqs))])
    return out


def _step(slam, frames, k, seqs):
    n = slam.n
    L, R = [None] * n, [None] * n
    for s in seqs:
        L[s], R[s] = frames[s][1][k], frames[s][2][k]
    torch.cuda.synchronize()
    slam.new_images(L, R, [k / 20.0] * n)


def test_calibrated_rigs_equal_rigs_from_the_stage_entrys_maps(frames):
    """ctx A: rig 0 through set_calibration, three rigs through add_rigs with calibrations (the fused kernel). ctx B:
    the same four from the float maps svo_build_rectify_maps made. The same raw frames: the same bytes, slot by
    slot, frame by frame, rectified images included; the same rig count and map bytes."""
    cals = _rig_cals()
    a, b = StereoSlamBatch(CFG, W, H, 4), StereoSlamBatch(CFG, W, H, 4)
    before = a.memory().device_bytes
    a.set_calibration(*cals[0])
    ids_a = a.add_rigs([_rig(k, left_calibration=cals[k][0], right_calibration=cals[k][1]) for k in (1, 2, 3)])
    maps = StereoSlamBatch.build_rectify_maps([c for pair in cals for c in pair], W, H)
    assert not all(torch.isfinite(m).all().item() for m in maps[4]), "the horizon case is among the rigs"
    b.set_rectification(maps[0], maps[1])
    ids_b = b.add_rigs([_rig(k, left_maps=maps[2 * k], right_maps=maps[2 * k + 1]) for k in (1, 2, 3)])
    assert ids_a == ids_b == [1, 2, 3]
    assert a.rigs() == b.rigs() and a.rigs()[0] == 4 and a.rigs()[1] > 0
    assert a.memory().device_bytes == b.memory().device_bytes == before + a.rigs()[1], "a rig costs its maps, no float plane"
    for slam, ids in ((a, ids_a), (b, ids_b)):
        slam.assign_rigs([1, 2, 3], ids)
    images = set()
    for k in range(N_FRAMES):
        for slam in (a, b):
            _step(slam, frames, k, range(4))
        sa, sb = _state(a, range(4)), _state(b, range(4))
        for part_a, part_b in zip(sa, sb):
            assert part_a == part_b, k
        images.update(sa[-2])
    assert len(images) == 4 * N_FRAMES, "every slot saw different rectified frames"
    assert any(np.frombuffer(i, np.uint8).any() for i in images)
    # the rigs behave alike afterwards as well: freed rigs give their bytes back
    for slam, ids in ((a, ids_a), (b, ids_b)):
        slam.assign_rigs([1, 2, 3], [0, 0, 0])
        slam.remove_rigs(ids[:2])
    assert a.rigs() == b.rigs() and a.rigs()[0] == 2
    a.set_calibration(None, None)
    b.set_rectification(None, None)
    _step(a, frames, 0, range(4)); _step(b, frames, 0, range(4))
    assert _state(a, range(4)) == _state(b, range(4))
    a.close(); b.close()


def test_a_list_may_mix_maps_calibrations_and_neither(frames):
    """add_rigs routes each form to its entry and returns the ids in the order of the list"""
    cals = _rig_cals()
    maps = StereoSlamBatch.build_rectify_maps([*cals[1]], W, H)
    slam = StereoSlamBatch(CFG, W, H, 1)
    rigs = [_rig(1, left_calibration=cals[1][0], right_calibration=cals[1][1]), _rig(2),
            _rig(3, left_maps=maps[0], right_maps=maps[1])]
    ids = slam.add_rigs(rigs)
    assert sorted(ids) == [1, 2, 3] and slam.rigs()[0] == 4
    for k, rid in zip((1, 2, 3), ids):
        slam.assign_rigs([0], [rid])
        assert slam.slot_rig(0)[1].baseline == np.float32(_rig(k)["baseline"]) and slam.slot_rig(0)[1].fx == np.float32(_rig(k)["fx"])
    with pytest.raises(ValueError):
        slam.add_rigs([_rig(1, left_calibration=cals[1][0], right_calibration=cals[1][1], left_maps=maps[0], right_maps=maps[1])])
    with pytest.raises(ValueError):
        slam.add_rigs([_rig(1, left_calibration=cals[1][0])])
    K, D, R, P = RC.cases()["tangential"]
    singular = CameraCalibration.from_mats(K, D, R, np.zeros((3, 3)))
    with pytest.raises(SvoError):                         # (the plain rig of the list was added first: it is taken back)
        slam.add_rigs([_rig(2), _rig(1, left_calibration=singular, right_calibration=cals[1][1])])
    assert slam.rigs()[0] == 4
    slam.close()


def test_bad_calibrated_calls_leave_the_ctx_as_it_was(frames):
    """a singular calibration in the middle of a list, a rig with map pointers set, n < 0, a bad set_calibration:
    SVO_ERR_INVALID, the rig count and the maps unchanged, and the next frame is the frame of a ctx that never saw
    the calls"""
    cals = _rig_cals()
    K, D, R, P = RC.cases()["tangential"]
    singular = CameraCalibration.from_mats(K, D, R, np.zeros((3, 3)))
    seen, clean = StereoSlamBatch(CFG, W, H, 2), StereoSlamBatch(CFG, W, H, 2)
    for slam in (seen, clean):
        slam.set_calibration(*cals[0])
        assert slam.add_rigs([_rig(1, left_calibration=cals[1][0], right_calibration=cals[1][1])]) == [1]
        slam.assign_rigs([1], [1])
        _step(slam, frames, 0, range(2))
    rigs3 = (hip_lib.Rig * 3)(*[hip_lib.Rig.from_dict(_rig(k)) for k in (1, 2, 3)])
    arr = lambda *c: (CameraCalibration * len(c))(*c)
    good_l, good_r = arr(cals[1][0], cals[2][0], cals[3][0]), arr(cals[1][1], cals[2][1], cals[3][1])
    ids = (C.c_int * 3)(-5, -5, -5)
    f = lib().svo_ctx_add_rigs_calibrated
    count = seen.rigs()
    assert f(seen._ctx, rigs3, arr(cals[1][0], singular, cals[3][0]), good_r, 3, ids) == -1
    assert f(seen._ctx, rigs3, good_l, arr(cals[1][1], cals[2][1], singular), 3, ids) == -1
    assert f(seen._ctx, rigs3, good_l, good_r, -1, ids) == -1
    assert f(seen._ctx, rigs3, None, good_r, 3, ids) == -1
    plane = torch.zeros((H, W), device="cuda")
    with_maps = (hip_lib.Rig * 3)(*[hip_lib.Rig.from_dict(_rig(k)) for k in (1, 2, 3)])
    for name in ("left_map_x", "left_map_y", "right_map_x", "right_map_y"):
        setattr(with_maps[1], name, plane.data_ptr())
    with_maps[1].mem = hip_lib.MEM_DEVICE
    assert f(seen._ctx, with_maps, good_l, good_r, 3, ids) == -1
    nan_rig = (hip_lib.Rig * 3)(*[hip_lib.Rig.from_dict(_rig(k)) for k in (1, 2, 3)])
    nan_rig[2].fx = float("nan")
    assert f(seen._ctx, nan_rig, good_l, good_r, 3, ids) == -1
    assert list(ids) == [-5, -5, -5] and seen.rigs() == count == clean.rigs()
    g = lib().svo_ctx_set_calibration
    assert g(seen._ctx, C.byref(cals[2][0]), C.byref(singular)) == -1           # the old maps stay
    assert g(seen._ctx, C.byref(cals[2][0]), None) == -1
    with pytest.raises(SvoError):
        seen.add_rigs([_rig(2, left_calibration=cals[2][0], right_calibration=singular)])
    for slam in (seen, clean):
        _step(slam, frames, 1, range(2))
    assert _state(seen, range(2)) == _state(clean, range(2))
    assert f(seen._ctx, rigs3, good_l, good_r, 3, ids) == 0 and list(ids) == [2, 3, 4]
    seen.close(); clean.close()


# ------------------------------------------------------------------------------------------- replay

def _mat(key, m):
    m = np.asarray(m, np.float64)
    return (f"{key}: !!opencv-matrix\n   rows: {m.shape[0]}\n   cols: {m.shape[1]}\n   dt: d\n   data: [" +
            ", ".join(repr(float(v)) for v in m.ravel()) + "]\n")


def test_replay_gpu_maps_equals_replay_with_the_statements_maps(tmp_path):
    """a tiny EuRoC-layout dataset: `replay --gpu-maps` (calibrations to the library, no float map on the host) writes
    the poses of a Replay that is given the statement's float maps for the same raw frames"""
    from PIL import Image
    from stereo_svo_slam_amd import replay
    n = 3
    cfg, L, R, _, _ = synth.make_sequence("tiny", n, 0, device="cpu")
    mav = tmp_path / "mav0"
    for cam in ("cam0", "cam1"):
        (mav / cam / "data").mkdir(parents=True)
    lines = ["#timestamp [ns],filename"]
    for k in range(n):
        stamp = 1403636579763555584 + k * 50000000
        Image.fromarray(R[k].numpy()).save(str(mav / "cam0" / "data" / f"{stamp}.png"))
        Image.fromarray(L[k].numpy()).save(str(mav / "cam1" / "data" / f"{stamp}.png"))
        lines.append(f"{stamp},{stamp}.png")
    (mav / "cam0" / "data.csv").write_text("\n".join(lines) + "\n")
    cals = {"LEFT": _tiny_cal(2), "RIGHT": _tiny_cal(-1)}
    mats = ""
    for side, c in cals.items():
        P = np.concatenate([np.array(c.P).reshape(3, 3), np.zeros((3, 1))], 1)
        mats += _mat(f"{side}.K", np.array(c.K).reshape(3, 3)) + _mat(f"{side}.D", np.array(c.D)[None, :5]) + \
            _mat(f"{side}.R", np.array(c.R).reshape(3, 3)) + _mat(f"{side}.P", P) + f"{side}.width: {W}\n{side}.height: {H}\n"
    keys = "".join(f"{k}: {cfg[f]}\n" for k, f in replay._YAML_KEYS.items())
    y = tmp_path / "cam.yaml"
    y.write_text("%YAML:1.0\n" + keys + f"Camera.width: {W}\nCamera.height: {H}\n" + mats)
    out = tmp_path / "traj.csv"
    replay.main(["--settings", str(y), "--euroc", str(mav) + "/", "--gpu-maps", "--frames", str(n), "-t", str(out)])
    rows = np.loadtxt(str(out), delimiter=",")
    src = replay.EurocInput(str(mav) + "/", str(y), raw=True, host_maps=False)
    assert [bytes(c) for c in src.gpu_calibration()] == [bytes(cals["RIGHT"]), bytes(cals["LEFT"])]
    as_case = lambda c: tuple(np.array(m).reshape(s) for m, s in ((c.K, (3, 3)), (c.D, (8,)), (c.R, (3, 3)), (c.P, (3, 3))))
    maps = tuple(RC.maps(as_case(c), W, H) for c in src.gpu_calibration())
    ref = replay.Replay(replay.read_settings(str(y)), rectify_maps=maps)
    for k in range(n):
        ref.feed(*src.read(k))
    assert np.array_equal(rows[:, 1:], np.loadtxt(_written(ref, tmp_path), delimiter=",")[:, 1:])
    assert np.abs(rows[-1, 1:]).max() > 0


def _written(rp, tmp_path):
    path = tmp_path / "ref.csv"
    rp.write(str(path))
    return str(path)
