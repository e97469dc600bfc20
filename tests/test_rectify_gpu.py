"""GPU rectification (cv::remap INTER_LINEAR, constant 0 border; src/app/euroc_input.cpp:69-70):
svo_remap_linear against the fixed-point restatement (tests/rectify_ref.py) bit for bit, and the tracker
with svo_ctx_set_rectification fed RAW frames against the oracle fed restatement-rectified ones."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_py as O
import rectify_ref as RR
import util
from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.hip_lib import SvoError, lib
from stereo_svo_slam_amd.stereo_slam import StereoSlam, StereoSlamBatch

pytestmark = pytest.mark.gpu

W, H = 752, 480


@pytest.fixture(scope="module")
def handle():
    h = hip_lib.Handle(0, 1024)
    yield h
    h.close()


def _rand_img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _remap_all(handle, srcs, mx, my):
    outs = handle.remap_linear([_dev(s) if isinstance(s, np.ndarray) else s for s in srcs], _dev(mx), _dev(my))
    handle.synchronize()
    return [o.cpu().numpy() for o in outs]


def _check(handle, srcs, mx, my):
    got = _remap_all(handle, srcs, mx, my)
    for i, (g, s) in enumerate(zip(got, srcs)):
        ref = RR.remap_linear(s if isinstance(s, np.ndarray) else s.cpu().numpy(), mx, my)
        assert np.array_equal(g, ref), (i, int(np.sum(g != ref)))


# ------------------------------------------------------------------------------------------- stage

def test_remap_euroc_like_and_random_maps(handle):
    """EuRoC-like maps: every 64 x 64 tile's source box is small (the LDS path); random maps over
    [-3, W+2] x [-3, H+2]: every tile's box is the whole image (the global path) and taps fall outside."""
    srcs = [_rand_img(H, W, s) for s in range(7)]
    _check(handle, srcs, *RR.euroc_like_maps(W, H))
    _check(handle, srcs[:1], *RR.euroc_like_maps(W, H, angle=-0.02, shift=(4.0, -6.0)))
    rng = np.random.default_rng(3)
    mx = rng.uniform(-3, W + 2, (H, W)).astype(np.float32)
    my = rng.uniform(-3, H + 2, (H, W)).astype(np.float32)
    _check(handle, srcs, mx, my)
    # both paths in one map: EuRoC-like tiles, and a band of random tiles
    ex, ey = RR.euroc_like_maps(W, H)
    ex[128:192], ey[128:192] = mx[128:192], my[128:192]
    _check(handle, srcs[:3], ex, ey)


def test_remap_ties_non_finite_and_huge_entries(handle):
    mx, my = RR.euroc_like_maps(W, H)
    rng = np.random.default_rng(4)
    u, v = RR.identity_maps(W, H)
    ties = rng.random((H, W)) < 0.2                        # m * 32 = k + 0.5
    mx = np.where(ties, u + np.float32(0.5 / 32) + np.float32(3 / 32), mx).astype(np.float32)
    my = np.where(ties, v + np.float32(1.5 / 32), my).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e10, -1e10, 2.0 ** 31 / 32, -1.0, W - 0.5], np.float32)
    for arr, seed in ((mx, 5), (my, 6)):
        pick = np.random.default_rng(seed).random((H, W)) < 0.05
        arr[pick] = np.random.default_rng(seed).choice(special, int(pick.sum()))
    srcs = [_rand_img(H, W, 10 + s) for s in range(2)]
    _check(handle, srcs, mx, my)


@pytest.mark.parametrize("n", [1, 7, 300])
def test_remap_odd_sizes_strides_and_counts(handle, n):
    """333 x 217 map, sources of another size (and strides wider than the rows), dst with a wider stride"""
    mw, mh = 333, 217
    sw, sh = 301, 250
    mx, my = RR.euroc_like_maps(mw, mh, f_p=300.0, f_k=310.0)
    mx = mx * np.float32(sw / mw)
    my = my * np.float32(sh / mh)
    srcs = []
    for i in range(n):
        buf = torch.from_numpy(_rand_img(sh, sw + 7 + (i % 3), 100 + i)).cuda()
        srcs.append(buf[:, :sw])                          # stride sw + 7 .. sw + 9: not dword-aligned rows
    dst_buf = [torch.full((mh, mw + 5), 3, dtype=torch.uint8, device="cuda") for _ in range(n)]
    dsts = [d[:, :mw] for d in dst_buf]
    arr_s, arr_d = hip_lib._imgs(srcs), hip_lib._imgs(dsts)
    dmx, dmy = _dev(mx), _dev(my)                         # (alive until the kernel has run)
    hip_lib._check(lib().svo_remap_linear(handle._h, n, arr_s, arr_d, hip_lib._ptr(dmx), hip_lib._ptr(dmy)))
    handle.synchronize()
    for i in range(n):
        ref = RR.remap_linear(srcs[i].cpu().numpy(), mx, my)
        got = dst_buf[i].cpu().numpy()
        assert np.array_equal(got[:, :mw], ref), i
        assert (got[:, mw:] == 3).all(), "a store past the row"


def test_remap_rejects_bad_calls(handle):
    img = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    mx = torch.zeros((16, 16), dtype=torch.float32, device="cuda")
    arr = hip_lib._imgs([img])
    assert lib().svo_remap_linear(handle._h, 0, arr, arr, hip_lib._ptr(mx), hip_lib._ptr(mx)) == -1
    assert lib().svo_remap_linear(handle._h, 1, arr, arr, None, hip_lib._ptr(mx)) == -1
    two = hip_lib._imgs([img, img])
    mixed = hip_lib._imgs([img, torch.zeros((8, 8), dtype=torch.uint8, device="cuda")])
    assert lib().svo_remap_linear(handle._h, 2, two, mixed, hip_lib._ptr(mx), hip_lib._ptr(mx)) == -1
    assert lib().svo_remap_linear(handle._h, 2, two, two, hip_lib._ptr(mx), hip_lib._ptr(mx)) == 0


# ------------------------------------------------------------------------------------------ tracker

def _snapshot(slam, seq):
    """everything the tracker reports about sequence `seq` now, as comparable bytes"""
    f = slam.get_frame(seq)
    st = slam.stats(seq)
    return (f.pose.tobytes(), f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes(), bytes(st),
            slam.num_keyframes(seq))


def _final(slam, seq):
    kfs = [(k.pose.tobytes(), k.kps2d.tobytes(), k.kps3d.tobytes(), k.info.tobytes())
           for k in slam.get_keyframes(seq)]
    return slam.get_trajectory(seq).tobytes(), kfs


def _render(n_seq, n_frames, seed0=300, motion_scale=8.0):
    return [synth.make_sequence_gpu("euroc", n_frames, seed0 + s, motion_scale=motion_scale) for s in range(n_seq)]


def _run_batch(rendered, mode, maps=None, lengths=None, overwrite=False):
    """all sequences in one ctx; mode 'host' | 'device' | 'borrow'; lengths: frames per sequence (NULL
    pointers afterwards). overwrite: the raw device frames are copies that are scribbled over after each step.
    Returns per frame the snapshots of the active sequences, and the final trajectories / keyframes."""
    n_seq = len(rendered)
    cfg = rendered[0][0]
    lengths = lengths or [len(r[4]) for r in rendered]
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_seq)
    if maps is not None:
        slam.set_rectification(*maps)
    frames = []
    scratch = [(torch.empty_like(r[1][0]), torch.empty_like(r[2][0])) for r in rendered]
    for k in range(max(lengths)):
        act = [s for s in range(n_seq) if k < lengths[s]]
        if mode == "host":
            L = [rendered[s][1][k].cpu().numpy() if s in act else None for s in range(n_seq)]
            R = [rendered[s][2][k].cpu().numpy() if s in act else None for s in range(n_seq)]
            slam.new_images(L, R, [k / 20.0] * n_seq)
        else:
            L, R = [], []
            for s in range(n_seq):
                if s not in act:
                    L.append(None); R.append(None)
                elif overwrite:
                    scratch[s][0].copy_(rendered[s][1][k]); scratch[s][1].copy_(rendered[s][2][k])
                    L.append(scratch[s][0]); R.append(scratch[s][1])
                else:
                    L.append(rendered[s][1][k]); R.append(rendered[s][2][k])
            torch.cuda.synchronize()
            if mode == "device":
                slam.new_images(L, R, [k / 20.0] * n_seq)
            else:
                slam.submit_packed(slam.pack_images(L, R, [k / 20.0] * n_seq, borrow=True))
                slam.wait()
            if overwrite:
                for a, b in scratch:
                    a.fill_(0); b.random_(0, 255)
                torch.cuda.synchronize()
        frames.append({s: _snapshot(slam, s) for s in act})
    final = [_final(slam, s) for s in range(n_seq)]
    groups = slam.groups()
    slam.close()
    return frames, final, groups


@pytest.fixture(scope="module")
def c2_raw():
    return _render(16, 32)


def test_identity_maps_change_nothing(monkeypatch, c2_raw):
    """C2 (`euroc`), 16 sequences in 2 groups, 32 frames with keyframes: rectification with identity maps
    gives the same trajectories, keypoints, keyframes and frame stats as rectification off, bit for bit,
    in all three memory modes; and in the single-sequence svo_new_image."""
    monkeypatch.setenv("SVO_GROUPS", "2")
    off_frames, off_final, groups = _run_batch(c2_raw, "device")
    assert groups == 2
    assert any(snap[4] and StatsView(snap[4]).is_keyframe for fr in off_frames[1:] for snap in fr.values())
    ident = (RR.identity_maps(W, H), RR.identity_maps(W, H))
    for mode in ("host", "device", "borrow"):
        frames, final, _ = _run_batch(c2_raw, mode, maps=ident)
        assert frames == off_frames, mode
        assert final == off_final, mode
    # svo_new_image: the drop-in path of one StereoSlam
    cfg, L, R = c2_raw[0][0], c2_raw[0][1].cpu().numpy(), c2_raw[0][2].cpu().numpy()
    out = []
    for on in (False, True):
        one = StereoSlamBatch(cfg, W, H, 1)
        if on:
            one.set_rectification(*ident)
        snaps = []
        for k in range(len(L)):
            l, r = np.ascontiguousarray(L[k]), np.ascontiguousarray(R[k])
            hip_lib._check(lib().svo_new_image(one._ctx, l.ctypes.data_as(C.c_void_p), W, r.ctypes.data_as(C.c_void_p),
                                               W, W, H, C.c_float(k / 20.0)))
            snaps.append(_snapshot(one, 0))
        out.append((snaps, _final(one, 0)))
        one.close()
    assert out[0] == out[1]
    assert [f[0] for f in out[0][0]] == [off_frames[k][0][0] for k in range(len(L))]


class StatsView:
    def __init__(self, raw):
        from stereo_svo_slam_amd.stereo_slam import FrameStats
        self.st = FrameStats.from_buffer_copy(raw)

    @property
    def is_keyframe(self):
        return self.st.is_keyframe


def _oracle(raw_seqs, cfg, rectify_at):
    """the oracle over each sequence's frames, rectified by the restatement where rectify_at(k) gives maps"""
    from concurrent.futures import ThreadPoolExecutor
    cam = util.oracle_camera(cfg)

    def one(seq):
        L, R, n = seq
        ref = O.Slam(cam)
        out = []
        for k in range(n):
            l, r = L[k], R[k]
            maps = rectify_at(k)
            if maps is not None:
                l, r = RR.remap_linear(l, *maps[0]), RR.remap_linear(r, *maps[1])
            made = ref.new_image(l, r, float(np.float32(k / 20.0)))
            k2, k3, info = ref.keypoints()
            out.append((made, ref.pose().copy(), k2, k3, info))
        traj = np.array([o[1] for o in out])
        ref.close()
        return out, traj

    with ThreadPoolExecutor(min(16, len(raw_seqs))) as ex:
        return list(ex.map(one, raw_seqs))


def _same_as_oracle(tag, snap, o):
    made, pose, k2, k3, info = o
    st = StatsView(snap[4])
    assert st.is_keyframe == made, f"{tag}: keyframe decision"
    assert np.array_equal(np.frombuffer(snap[0], np.float32), pose), f"{tag}: pose"
    assert np.array_equal(np.frombuffer(snap[1], np.float32).reshape(-1, 2), k2), f"{tag}: kps2d"
    assert np.array_equal(np.frombuffer(snap[2], np.float32).reshape(-1, 3), k3), f"{tag}: kps3d"
    from stereo_svo_slam_amd.stereo_slam import KP_INFO_DTYPE
    g = np.frombuffer(snap[3], KP_INFO_DTYPE)
    for f in ("level", "type", "keyframe_id", "keypoint_index", "score", "outlier_count", "inlier_count",
              "ignore_during_refinement", "ignore_completely", "ignore_temporary"):
        assert np.array_equal(g[f], info[f]), f"{tag}: info.{f}"


def _euroc_maps():
    left = RR.euroc_like_maps(W, H, angle=0.012, shift=(1.5, -2.0))
    right = RR.euroc_like_maps(W, H, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068)
    return left, right


@pytest.fixture(scope="module")
def raw_unequal():
    rendered = _render(8, 14, seed0=500)
    lengths = [14, 14, 9, 14, 6, 14, 11, 14]
    maps = _euroc_maps()
    host = [(r[1].cpu().numpy(), r[2].cpu().numpy(), n) for r, n in zip(rendered, lengths)]
    oracle = _oracle(host, rendered[0][0], lambda k: maps)
    return rendered, lengths, maps, oracle


def test_euroc_like_maps_equal_the_oracle_on_rectified_frames(monkeypatch, raw_unequal):
    """raw frames into the ctx with rectification on (host and device memory, 2 groups, sequences of
    unequal length) == the oracle fed frames rectified by the restatement: pose, keypoints, keyframe
    decisions and trajectories bit for bit"""
    rendered, lengths, maps, oracle = raw_unequal
    monkeypatch.setenv("SVO_GROUPS", "2")
    for mode in ("host", "device"):
        frames, final, groups = _run_batch(rendered, mode, maps=maps, lengths=lengths)
        assert groups == 2
        for k, fr in enumerate(frames):
            for s, snap in fr.items():
                _same_as_oracle(f"{mode} seq {s} frame {k}", snap, oracle[s][0][k])
        for s in range(len(rendered)):
            assert np.array_equal(np.frombuffer(final[s][0], np.float32).reshape(-1, 6), oracle[s][1]), (mode, s)
    assert any(o[0] for seq in oracle for o in seq[0][1:]), "a keyframe inside the run"


def test_borrowed_raw_frames_may_be_reused_after_the_step(monkeypatch, raw_unequal):
    """SVO_MEM_DEVICE_BORROW with rectification: level 0 is the ctx's own image, so raw buffers that are
    overwritten after every step give the results of the copying mode"""
    rendered, lengths, maps, oracle = raw_unequal
    monkeypatch.setenv("SVO_GROUPS", "2")
    ref = _run_batch(rendered, "device", maps=maps, lengths=lengths)
    got = _run_batch(rendered, "borrow", maps=maps, lengths=lengths, overwrite=True)
    assert got[0] == ref[0] and got[1] == ref[1]


def test_switching_rectification_between_frames():
    """off for frames 0-3, on 4-8 (set through device tensors), other maps 9-11 (host arrays), off again
    12-15: each frame follows the setting in force, checked against the oracle"""
    cfg, L, R, _, _ = synth.make_sequence_gpu("euroc", 16, 77, motion_scale=4.0)
    m1, m2 = _euroc_maps(), (_euroc_maps()[1], _euroc_maps()[0])
    plan = lambda k: None if k < 4 or k >= 12 else (m1 if k < 9 else m2)
    Lh, Rh = L.cpu().numpy(), R.cpu().numpy()
    oracle, traj = _oracle([(Lh, Rh, 16)], cfg, plan)[0]
    slam = StereoSlam(cfg)                      # (its ctx comes with the first frame)
    for k in range(16):
        if k == 4:
            slam.set_rectification(*[tuple(_dev(a) for a in side) for side in m1])
        elif k == 9:
            slam.set_rectification(*m2)
        elif k == 12:
            slam.set_rectification(None, None)
        slam.new_image(Lh[k], Rh[k], k / 20.0)
        _same_as_oracle(f"frame {k}", _snapshot(slam, 0), oracle[k])
    assert np.array_equal(slam.get_trajectory(), traj)
    # maps given before the first frame apply to it
    first = StereoSlam(cfg)
    first.set_rectification(*m1)
    first.new_image(Lh[0], Rh[0], 0.0)
    o0 = _oracle([(Lh, Rh, 1)], cfg, lambda k: m1)[0][0][0]
    _same_as_oracle("first frame", _snapshot(first, 0), o0)
    slam.close(); first.close()


def test_invalid_rectification_calls_leave_the_ctx_usable():
    cfg, L, R, _, _ = synth.make_sequence_gpu("euroc", 3, 9)
    slam = StereoSlamBatch(cfg, W, H, 1)
    mx, my = RR.identity_maps(W, H)
    p = mx.ctypes.data_as(C.c_void_p)
    q = my.ctypes.data_as(C.c_void_p)
    f = lib().svo_ctx_set_rectification
    assert f(slam._ctx, p, q, p, None, 0) == -1            # only some maps
    assert f(slam._ctx, None, None, p, q, 0) == -1
    assert f(slam._ctx, p, q, p, q, 2) == -1               # bad mem
    assert f(slam._ctx, p, q, p, q, 7) == -1
    assert f(None, p, q, p, q, 0) == -1
    ref = StereoSlamBatch(cfg, W, H, 1)
    for k in range(3):
        slam.new_images([L[k]], [R[k]], [k / 20.0])
        ref.new_images([L[k]], [R[k]], [k / 20.0])
        assert _snapshot(slam, 0) == _snapshot(ref, 0)
    assert f(slam._ctx, p, q, p, q, 0) == 0 and f(slam._ctx, None, None, None, None, 1) == 0
    with pytest.raises(SvoError):
        hip_lib._check(f(slam._ctx, p, None, None, None, 0))
    slam.close(); ref.close()


# ------------------------------------------------------------------------------------------- replay

def _mat(key, rows, cols, data):
    return (f"{key}: !!opencv-matrix\n   rows: {rows}\n   cols: {cols}\n   dt: d\n   data: [" +
            ", ".join(repr(float(v)) for v in data) + "]\n")


def test_replay_gpu_rectify_equals_the_oracle(tmp_path):
    """a tiny EuRoC-layout dataset with a non-identity calibration: `replay --gpu-rectify` hands the raw
    frames to the library; its trajectory is the oracle's on frames rectified by the restatement"""
    from PIL import Image
    cfg, L, R, _, _ = synth.make_sequence("tiny", 4, 0, device="cpu")
    w, h = cfg["width"], cfg["height"]
    mav = tmp_path / "mav0"
    for cam in ("cam0", "cam1"):
        (mav / cam / "data").mkdir(parents=True)
    lines = ["#timestamp [ns],filename"]
    for k in range(4):
        stamp = 1403636579763555584 + k * 50000000
        Image.fromarray(R[k].numpy()).save(str(mav / "cam0" / "data" / f"{stamp}.png"))
        Image.fromarray(L[k].numpy()).save(str(mav / "cam1" / "data" / f"{stamp}.png"))
        lines.append(f"{stamp},{stamp}.png")
    (mav / "cam0" / "data.csv").write_text("\n".join(lines) + "\n")
    c, s = np.cos(0.01), np.sin(0.01)
    mats = ""
    for side, (dx, d1) in (("LEFT", (2.0, -0.28)), ("RIGHT", (-1.5, -0.27))):
        K = [cfg["fx"] * 1.05, 0, w / 2 + dx, 0, cfg["fy"] * 1.05, h / 2 - 1.0, 0, 0, 1]
        P = [cfg["fx"], 0, w / 2, 0, 0, cfg["fy"], h / 2, 0, 0, 0, 1, 0]
        Rm = [c, 0, s, 0, 1, 0, -s, 0, c]
        mats += _mat(f"{side}.K", 3, 3, K) + _mat(f"{side}.D", 1, 5, [d1, 0.07, 0, 0, 0]) + \
            _mat(f"{side}.R", 3, 3, Rm) + _mat(f"{side}.P", 3, 4, P) + f"{side}.width: {w}\n{side}.height: {h}\n"
    keys = "".join(f"{k}: {cfg[f]}\n" for k, f in replay._YAML_KEYS.items())
    y = tmp_path / "cam.yaml"
    y.write_text("%YAML:1.0\n" + keys + f"Camera.width: {w}\nCamera.height: {h}\n" + mats)
    out = tmp_path / "traj.csv"
    replay.main(["--settings", str(y), "--euroc", str(mav) + "/", "--gpu-rectify", "--frames", "4", "-t", str(out)])
    rows = np.loadtxt(str(out), delimiter=",")
    src = replay.EurocInput(str(mav) + "/", str(y))
    left_maps, right_maps = src.maps_r, src.maps_l
    ref = O.Slam(util.oracle_camera(replay.read_settings(str(y))))
    for k in range(4):
        raw = replay.EurocInput(str(mav) + "/", str(y), raw=True).read(k)
        ref.new_image(RR.remap_linear(raw[0], *left_maps), RR.remap_linear(raw[1], *right_maps),
                      float(np.float32(0.05 * k)))
        exp = np.concatenate([ref.pose()[:3], replay.csv_angles(ref.pose())])
        assert np.allclose(rows[k, 1:], exp, atol=1e-6), k
    assert not np.array_equal(RR.remap_linear(raw[0], *left_maps), raw[0])
