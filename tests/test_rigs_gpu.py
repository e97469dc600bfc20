"""Camera rigs: slots of one ctx with their own intrinsics and rectification maps (svo_ctx_add_rigs /
svo_ctx_assign_rigs), and the remap with a map per image behind them (svo_remap_linear_multi). The stage entry
against the fixed-point restatement (tests/rectify_ref.py) per image, the tracker against one oracle_py.Slam per
sequence under that sequence's settings (fed frames rectified by the restatement where its rig has maps), and
against ctxs that have a single rig. Everything bit for bit."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import oracle_py as O
import rectify_ref as RR
import util
from stereo_svo_slam_amd import hip_lib, multi_seq, synth
from stereo_svo_slam_amd.hip_lib import SvoError, lib
from stereo_svo_slam_amd.stereo_slam import KP_INFO_DTYPE, FrameStats, StereoSlamBatch

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


# ------------------------------------------------------------------------------------------- stage

def _multi(handle, srcs, maps, map_of):
    """srcs (numpy) through maps[map_of[i]] = (map_x, map_y): the outputs (numpy)"""
    outs = handle.remap_linear_multi([_dev(s) for s in srcs], [_dev(m[0]) for m in maps], [_dev(m[1]) for m in maps], map_of)
    handle.synchronize()
    return [o.cpu().numpy() for o in outs]


def _check_multi(handle, srcs, maps, map_of):
    got = _multi(handle, srcs, maps, map_of)
    for i, (g, s) in enumerate(zip(got, srcs)):
        ref = RR.remap_linear(s, *maps[map_of[i]])
        assert np.array_equal(g, ref), (i, map_of[i], int(np.sum(g != ref)))


def _small_maps(n_maps, mw, mh, sw, sh):
    """n_maps different EuRoC-like maps of mw x mh onto sources of sw x sh"""
    maps = []
    for m in range(n_maps):
        mx, my = RR.euroc_like_maps(mw, mh, f_p=120.0, f_k=126.0 + 0.5 * (m % 5), angle=0.01 * ((m % 7) - 3),
                                    shift=(0.75 * (m % 4) - 1.0, 1.25 * (m % 3) - 1.5), k1=-0.28 + 0.01 * (m % 6))
        maps.append((mx * np.float32(sw / mw), my * np.float32(sh / mh)))
    return maps


def _shuffled(groups, seed):
    """map_of_image with groups[m] images on map m, shuffled"""
    idx = [m for m, c in enumerate(groups) for _ in range(c)]
    np.random.default_rng(seed).shuffle(idx)
    return [int(i) for i in idx]


@pytest.mark.parametrize("groups", [[1], [3, 0, 4], [1] * 40, [19, 1, 0, 20]],
                         ids=["n1_maps1", "n7_maps3", "n40_maps40", "n40_run19"])
def test_remap_multi_small_map_many_runs(handle, groups):
    """130 x 70 map (3 x 2 tiles, partial right and bottom), sources of 121 x 83 whose rows are not dword aligned,
    dst with a wider stride whose guard columns keep their fill value; runs of 1 .. 20 images (one crosses the
    16-image chunk), a map per image (the kernel form without an image loop), shuffled indices, an unused map."""
    mw, mh, sw, sh = 130, 70, 121, 83
    maps = _small_maps(len(groups), mw, mh, sw, sh)
    map_of = _shuffled(groups, 11)
    n = len(map_of)
    srcs = []
    for i in range(n):
        buf = torch.from_numpy(_rand_img(sh, sw + 5 + (i % 3), 100 + i)).cuda()
        srcs.append(buf[:, :sw])                          # strides 126, 127, 128
    dst_buf = [torch.full((mh, mw + 3), 3, dtype=torch.uint8, device="cuda") for _ in range(n)]
    dsts = [d[:, :mw] for d in dst_buf]
    dmx, dmy = [_dev(m[0]) for m in maps], [_dev(m[1]) for m in maps]      # (alive until the kernel has run)
    px = (C.c_void_p * len(maps))(*[m.data_ptr() for m in dmx])
    py = (C.c_void_p * len(maps))(*[m.data_ptr() for m in dmy])
    hip_lib._check(lib().svo_remap_linear_multi(handle._h, n, hip_lib._imgs(srcs), hip_lib._imgs(dsts), len(maps), px, py,
                                                (C.c_int * n)(*map_of)))
    handle.synchronize()
    for i in range(n):
        ref = RR.remap_linear(srcs[i].cpu().numpy(), *maps[map_of[i]])
        got = dst_buf[i].cpu().numpy()
        assert np.array_equal(got[:, :mw], ref), (i, map_of[i])
        assert (got[:, mw:] == 3).all(), "a store past the row"


def _special_map():
    """the ties, NaN, +-inf and +-1e10 entries of test_rectify_gpu.test_remap_ties_non_finite_and_huge_entries"""
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
    return mx, my


def test_remap_multi_both_gather_paths_in_one_call(handle):
    """EuRoC-like maps (every tile's source box is small: the LDS path), a uniform-random map (every tile's box is
    the whole image: the global path, taps outside) and a map with ties and entries without a source, in one call"""
    rng = np.random.default_rng(3)
    maps = [RR.euroc_like_maps(W, H),
            RR.euroc_like_maps(W, H, angle=-0.02, shift=(4.0, -6.0), k1=-0.25),
            (rng.uniform(-3, W + 2, (H, W)).astype(np.float32), rng.uniform(-3, H + 2, (H, W)).astype(np.float32)),
            _special_map()]
    srcs = [_rand_img(H, W, s) for s in range(7)]
    _check_multi(handle, srcs, maps, [2, 0, 3, 1, 0, 2, 3])


def test_remap_multi_full_size(handle):
    maps = [RR.euroc_like_maps(W, H, angle=0.012, shift=(1.5, -2.0)),
            RR.euroc_like_maps(W, H, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068),
            RR.euroc_like_maps(W, H, angle=0.02, shift=(0.5, 2.5), k1=-0.3)]
    _check_multi(handle, [_rand_img(H, W, 20 + s) for s in range(4)], maps, [1, 2, 0, 1])


def test_remap_multi_with_one_map_equals_remap_linear(handle):
    mx, my = RR.euroc_like_maps(W, H, angle=0.015)
    srcs = [_rand_img(H, W, 40 + s) for s in range(19)]
    one = handle.remap_linear([_dev(s) for s in srcs], _dev(mx), _dev(my))
    handle.synchronize()
    got = _multi(handle, srcs, [(mx, my)], [0] * len(srcs))
    for i in range(len(srcs)):
        assert np.array_equal(got[i], one[i].cpu().numpy()), i


def test_remap_multi_rejects_bad_calls(handle):
    img = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    mx = torch.zeros((16, 16), dtype=torch.float32, device="cuda")
    f = lib().svo_remap_linear_multi
    two = hip_lib._imgs([img, img])
    mixed = hip_lib._imgs([img, torch.zeros((8, 8), dtype=torch.uint8, device="cuda")])
    maps2 = (C.c_void_p * 2)(mx.data_ptr(), mx.data_ptr())
    hole = (C.c_void_p * 2)(mx.data_ptr(), None)
    idx = lambda *v: (C.c_int * len(v))(*v)
    assert f(handle._h, 2, two, two, 0, maps2, maps2, idx(0, 0)) == -1            # n_maps = 0
    assert f(handle._h, 2, two, two, 2, maps2, maps2, idx(0, 2)) == -1            # an index out of range
    assert f(handle._h, 2, two, two, 2, maps2, maps2, idx(-1, 0)) == -1
    assert f(handle._h, 2, two, two, 2, hole, maps2, idx(0, 0)) == -1             # a null map (even an unused one)
    assert f(handle._h, 2, two, two, 2, maps2, None, idx(0, 0)) == -1
    assert f(handle._h, 2, two, mixed, 2, maps2, maps2, idx(0, 1)) == -1          # mixed sizes
    assert f(handle._h, 2, two, two, 2, maps2, maps2, idx(1, 0)) == 0
    handle.synchronize()


# ------------------------------------------------------------------------------------------ tracker

ECON_DISTORTION = {k: synth.CONFIGS["econ"][k] for k in ("k1", "k2", "k3", "p1", "p2")}
# what the three rigs of the `tiny` tests change of the preset (rig 0: nothing)
TINY_RIGS = [{}, dict(fx=212.0, fy=212.0, cx=151.5, cy=127.25, baseline=23.5), ECON_DISTORTION]


def _rig_cfg(config, changes):
    return dict(synth.CONFIGS[config], **changes)


class StatsView:
    def __init__(self, raw):
        self.st = FrameStats.from_buffer_copy(raw)

    @property
    def is_keyframe(self):
        return self.st.is_keyframe


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


def _same_as_oracle(tag, snap, o):
    made, pose, k2, k3, info = o
    st = StatsView(snap[4])
    assert st.is_keyframe == made, f"{tag}: keyframe decision"
    assert np.array_equal(np.frombuffer(snap[0], np.float32), pose), f"{tag}: pose"
    assert np.array_equal(np.frombuffer(snap[1], np.float32).reshape(-1, 2), k2), f"{tag}: kps2d"
    assert np.array_equal(np.frombuffer(snap[2], np.float32).reshape(-1, 3), k3), f"{tag}: kps3d"
    g = np.frombuffer(snap[3], KP_INFO_DTYPE)
    for f in ("level", "type", "keyframe_id", "keypoint_index", "score", "outlier_count", "inlier_count",
              "ignore_during_refinement", "ignore_completely", "ignore_temporary"):
        assert np.array_equal(g[f], info[f]), f"{tag}: info.{f}"


def _oracle(runs):
    """runs: [(cfg, lefts, rights (numpy [n, H, W]), frames, maps or None)]: one fresh oracle per run under its
    settings, fed frames rectified by the restatement where maps = ((lx, ly), (rx, ry)) are given. Per run:
    (per frame (keyframe made, pose, kps2d, kps3d, info), trajectory)."""
    def one(run):
        cfg, L, R, n, maps = run
        ref = O.Slam(util.oracle_camera(cfg))
        out = []
        for k in range(n):
            l, r = L[k], R[k]
            if maps is not None:
                l, r = RR.remap_linear(l, *maps[0]), RR.remap_linear(r, *maps[1])
            made = ref.new_image(l, r, float(np.float32(k / 20.0)))
            k2, k3, info = ref.keypoints()
            out.append((made, ref.pose().copy(), k2, k3, info))
        traj = np.array([o[1] for o in out])
        ref.close()
        return out, traj

    with ThreadPoolExecutor(min(16, len(runs))) as ex:
        return list(ex.map(one, runs))


def _rig_dict(cfg, maps=None):
    d = {k: cfg[k] for k in hip_lib.RIG_FLOATS}
    if maps is not None:
        d["left_maps"], d["right_maps"] = maps
    return d


def _play(slam, rendered, lengths, mode="device", scribble=()):
    """frame k of rendered[s] = (cfg, lefts, rights, ...) into slot s while k < lengths[s]; mode 'host' | 'device' |
    'borrow'. scribble: slots whose device frames are copies that are overwritten after every step. Returns per
    frame {slot: _snapshot}."""
    n = len(rendered)
    scratch = {s: (torch.empty_like(rendered[s][1][0]), torch.empty_like(rendered[s][2][0])) for s in scribble}
    frames = []
    for k in range(max(lengths)):
        act = [s for s in range(n) if k < lengths[s]]
        ts = [k / 20.0] * n
        if mode == "host":
            slam.new_images([rendered[s][1][k].cpu().numpy() if s in act else None for s in range(n)],
                            [rendered[s][2][k].cpu().numpy() if s in act else None for s in range(n)], ts)
        else:
            L, R = [None] * n, [None] * n
            for s in act:
                L[s], R[s] = rendered[s][1][k], rendered[s][2][k]
                if s in scratch:
                    scratch[s][0].copy_(L[s]); scratch[s][1].copy_(R[s])
                    L[s], R[s] = scratch[s]
            torch.cuda.synchronize()
            if mode == "device":
                slam.new_images(L, R, ts)
            else:
                slam.submit_packed(slam.pack_images(L, R, ts, borrow=True))
                slam.wait()
            for a, b in scratch.values():
                a.fill_(0); b.random_(0, 255)
            torch.cuda.synchronize()
        frames.append({s: _snapshot(slam, s) for s in act})
    return frames


def _host(r):
    return r[1].cpu().numpy(), r[2].cpu().numpy()


def test_intrinsics_per_slot_equal_the_oracle_under_each_rig(monkeypatch):
    """6 `tiny` slots in 2 groups on rigs [0, 1, 2, 1, 0, 2], each sequence rendered with its rig's intrinsics,
    unequal lengths: every frame of every slot is the oracle's under that rig's settings"""
    monkeypatch.setenv("SVO_GROUPS", "2")
    rig_of = [0, 1, 2, 1, 0, 2]
    lengths = [12, 12, 7, 12, 9, 12]
    rendered = [synth.make_sequence_gpu("tiny", 12, 900 + s, motion_scale=8.0, overrides=TINY_RIGS[r])
                for s, r in enumerate(rig_of)]
    oracle = _oracle([(r[0], *_host(r), n, None) for r, n in zip(rendered, lengths)])
    assert any(o[0] for run in oracle for o in run[0][1:]), "a keyframe inside the run"
    cfg = synth.CONFIGS["tiny"]
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 6)
    assert slam.groups() == 2 and slam.rigs() == (1, 0)
    ids = slam.add_rigs([_rig_dict(_rig_cfg("tiny", c)) for c in TINY_RIGS[1:]])
    assert ids == [1, 2] and slam.rigs() == (3, 0)
    slam.assign_rigs([s for s in range(6) if rig_of[s]], [r for r in rig_of if r])
    for s, r in enumerate(rig_of):
        rig, cam = slam.slot_rig(s)
        assert rig == r and bytes(cam) == bytes(hip_lib.CameraSettings.from_dict(rendered[s][0]))
    frames = _play(slam, rendered, lengths)
    for k, fr in enumerate(frames):
        for s, snap in fr.items():
            _same_as_oracle(f"slot {s} rig {rig_of[s]} frame {k}", snap, oracle[s][0][k])
    for s in range(6):
        assert np.array_equal(slam.get_trajectory(s), oracle[s][1]), s
    slam.close()


def _euroc_rig_maps():
    m1 = (RR.euroc_like_maps(W, H, angle=0.012, shift=(1.5, -2.0)),
          RR.euroc_like_maps(W, H, angle=-0.009, shift=(-3.0, 1.0), k1=-0.27, k2=0.068))
    m2 = (RR.euroc_like_maps(W, H, angle=-0.015, shift=(-2.0, 2.5), k1=-0.29),
          RR.euroc_like_maps(W, H, angle=0.007, shift=(2.5, -1.5), k1=-0.275, k2=0.072))
    return {1: m1, 2: m2}


def test_maps_per_rig_equal_the_oracle_on_rectified_frames(monkeypatch):
    """4 `euroc` slots on rigs [1, 0, 2, 1]: rigs 1 and 2 have maps of their own for both sides, rig 0 has none (and
    the ctx no rectification). Raw frames in host, device and borrow mode: the oracle fed frames rectified by the
    restatement with the slot's maps, and as given for the rig-0 slot. Borrow mode: the buffers of the slots that
    are remapped are overwritten after every step, the rig-0 slot's are used in place."""
    monkeypatch.setenv("SVO_GROUPS", "2")
    rig_of = [1, 0, 2, 1]
    n = 10
    maps = _euroc_rig_maps()
    rendered = [synth.make_sequence_gpu("euroc", n, 300 + s, motion_scale=8.0) for s in range(4)]
    cfg = rendered[0][0]
    oracle = _oracle([(cfg, *_host(r), n, maps.get(rig_of[s])) for s, r in enumerate(rendered)])
    for mode in ("host", "device", "borrow"):
        slam = StereoSlamBatch(cfg, W, H, 4)
        give = [tuple(tuple(_dev(a) for a in side) for side in maps[r]) if mode == "device" else maps[r] for r in (1, 2)]
        ids = slam.add_rigs([_rig_dict(cfg, m) for m in give])
        assert ids == [1, 2] and slam.rigs()[0] == 3 and slam.rigs()[1] > 0
        slam.assign_rigs([0, 2, 3], [1, 2, 1])
        frames = _play(slam, rendered, [n] * 4, mode, scribble=(0, 2, 3) if mode == "borrow" else ())
        for k, fr in enumerate(frames):
            for s, snap in fr.items():
                _same_as_oracle(f"{mode} slot {s} rig {rig_of[s]} frame {k}", snap, oracle[s][0][k])
        for s in range(4):
            assert np.array_equal(slam.get_trajectory(s), oracle[s][1]), (mode, s)
        slam.close()


def _tiny_maps(seed):
    w, h = synth.CONFIGS["tiny"]["width"], synth.CONFIGS["tiny"]["height"]
    return (RR.euroc_like_maps(w, h, f_p=200.0, f_k=208.0, angle=0.004 * seed, shift=(0.5 * seed, -0.75)),
            RR.euroc_like_maps(w, h, f_p=200.0, f_k=207.0, angle=-0.003 * seed, shift=(-1.0, 0.25 * seed), k1=-0.27))


def test_a_mixed_ctx_equals_single_rig_ctxs():
    """5 `tiny` slots on rigs [1, 0, 2, 1, 2] (rigs 1 and 2 with maps): every slot gives what a ctx created with
    its rig's settings (and set_rectification with its maps) gives: every frame, stats, keyframes, trajectory"""
    rig_of = [1, 0, 2, 1, 2]
    lengths = [8, 8, 8, 5, 8]
    maps = {1: _tiny_maps(1), 2: _tiny_maps(2)}
    rendered = [synth.make_sequence_gpu("tiny", 8, 950 + s, motion_scale=8.0, overrides=TINY_RIGS[r])
                for s, r in enumerate(rig_of)]
    cfg = synth.CONFIGS["tiny"]
    w, h = cfg["width"], cfg["height"]
    mixed = StereoSlamBatch(cfg, w, h, 5)
    ids = mixed.add_rigs([_rig_dict(_rig_cfg("tiny", TINY_RIGS[r]), maps[r]) for r in (1, 2)])
    mixed.assign_rigs([s for s in range(5) if rig_of[s]], [ids[r - 1] for r in rig_of if r])
    got = _play(mixed, rendered, lengths)
    got_final = [_final(mixed, s) for s in range(5)]
    mixed.close()
    for r in (0, 1, 2):
        slots = [s for s in range(5) if rig_of[s] == r]
        one = StereoSlamBatch(_rig_cfg("tiny", TINY_RIGS[r]), w, h, len(slots))
        if r:
            one.set_rectification(*maps[r])
        ref = _play(one, [rendered[s] for s in slots], [lengths[s] for s in slots])
        for k, fr in enumerate(ref):
            for j, snap in fr.items():
                assert got[k][slots[j]] == snap, (r, slots[j], k)
        for j, s in enumerate(slots):
            assert got_final[s] == _final(one, j), (r, s)
        one.close()


def test_mixed_rigs_behind_a_converting_input_format():
    """3 `tiny` slots on rigs [1, 0, 2] (1 and 2 with maps) fed B,G,R frames whose channels are the gray frame
    (cvtColor gives the gray value back): ingest -> remap -> pyramids for the slots that remap, ingest alone for
    the other, in one step; the bytes of the same ctx fed the gray frames"""
    rig_of = [1, 0, 2]
    maps = {1: _tiny_maps(1), 2: _tiny_maps(2)}
    rendered = [synth.make_sequence_gpu("tiny", 6, 960 + s, motion_scale=8.0, overrides=TINY_RIGS[r])
                for s, r in enumerate(rig_of)]
    colour = [(r[0], r[1].unsqueeze(-1).expand(-1, -1, -1, 3).contiguous(), r[2].unsqueeze(-1).expand(-1, -1, -1, 3).contiguous())
              for r in rendered]
    cfg = synth.CONFIGS["tiny"]
    out = []
    for fmt, frames in ((None, rendered), ("bgr_pair", colour)):
        slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 3)
        if fmt:
            slam.set_input_format(fmt)
        ids = slam.add_rigs([_rig_dict(_rig_cfg("tiny", TINY_RIGS[r]), maps[r]) for r in (1, 2)])
        slam.assign_rigs([0, 2], ids)
        out.append((_play(slam, frames, [6, 6, 4]), [_final(slam, s) for s in range(3)]))
        slam.close()
    assert out[0] == out[1]


def test_a_slot_alternates_between_rigs():
    """one slot plays five short runs on rigs 1, 2, 1, 2, 1 (rig 1 with maps), the assignments queued between the
    frame sets without a wait: each run is the oracle's under its rig, memory is bounded, and a rig goes only
    once no slot is bound to it"""
    cfg = synth.CONFIGS["tiny"]
    w, h = cfg["width"], cfg["height"]
    maps1 = _tiny_maps(3)
    seq = {r: synth.make_sequence_gpu("tiny", 5, 970 + r, motion_scale=8.0, overrides=TINY_RIGS[r]) for r in (1, 2)}
    oracle = {r: _oracle([(seq[r][0], *_host(seq[r]), 5, maps1 if r == 1 else None)])[0] for r in (1, 2)}
    slam = StereoSlamBatch(cfg, w, h, 2)
    before = slam.rigs()[1], slam.memory().device_bytes
    id1 = slam.add_rigs([_rig_dict(seq[1][0], maps1)])[0]
    took = slam.rigs()[1] - before[0]
    assert took == 2 * 492032, "two maps of 20 tiles: 4096 x (4 + 2) bytes and a box per tile, 256-byte aligned parts"
    assert slam.memory().device_bytes - before[1] == took
    id2 = slam.add_rigs([_rig_dict(seq[2][0])])[0]
    assert slam.rigs() == (3, took)
    plan = [id1, id2, id1, id2, id1]
    rig_of = {id1: 1, id2: 2}
    mem = {}
    for j, rid in enumerate(plan):
        slam.assign_rigs([0], [rid])                      # (queued behind the previous run's frames: no wait)
        r = rig_of[rid]
        for k in range(4):
            slam.submit_packed(slam.pack_images([seq[r][1][k], None], [seq[r][2][k], None], [k / 20.0, 0.0]))
        if j in (1, 3):
            m = slam.memory()                             # (waits)
            mem[j] = (m.device_bytes, m.image_sets, m.keyframe_slabs)
            _same_as_oracle(f"run {j} frame 3", _snapshot(slam, 0), oracle[r][0][3])
    assert mem[1] == mem[3], "a slot plays any number of sequences in bounded memory"
    done = slam.finished_runs(0)
    assert len(done) == 4 and [i.run for i, _ in done] == [0, 1, 2, 3]
    for j, (info, traj) in enumerate(done):
        o = oracle[rig_of[plan[j]]]
        assert info.frames == 4 and np.array_equal(traj, o[1][:4]), j
        assert info.keyframes == sum(f[0] for f in o[0][:4]), j
    assert np.array_equal(slam.get_trajectory(0), oracle[1][1][:4])
    assert slam.slot_rig(0)[0] == id1 and slam.slot_rig(1)[0] == 0
    # the binding survives a restart
    slam.restart([0])
    assert slam.slot_rig(0)[0] == id1
    for k in range(5):
        slam.new_images([seq[1][1][k], None], [seq[1][2][k], None], [k / 20.0, 0.0])
        _same_as_oracle(f"after the restart, frame {k}", _snapshot(slam, 0), oracle[1][0][k])
    # a bound rig stays, and the ctx carries on
    with pytest.raises(SvoError):
        slam.remove_rigs([id1])
    with pytest.raises(SvoError):
        slam.remove_rigs([0])
    assert slam.rigs() == (3, took)
    assert np.array_equal(slam.get_trajectory(0), oracle[1][1])
    slam.assign_rigs([0], [0])
    bytes_with_maps = slam.memory().device_bytes
    slam.remove_rigs([id1])
    assert slam.rigs() == (2, 0), "its maps are gone"
    assert slam.memory().device_bytes == bytes_with_maps - took
    with pytest.raises(SvoError):
        slam.assign_rigs([0], [id1])                      # the id is gone: nothing queued
    slam.close()


def test_snapshots_carry_the_slots_settings():
    """a slot on rig 1 saved and loaded into a slot of a second ctx whose rig has equal settings continues as the
    uninterrupted run; a slot on other settings rejects the snapshot at submit time, nothing changed"""
    cfg = synth.CONFIGS["tiny"]
    w, h = cfg["width"], cfg["height"]
    r1 = synth.make_sequence_gpu("tiny", 10, 990, motion_scale=8.0, overrides=TINY_RIGS[1])
    rig1, rig2 = _rig_dict(r1[0]), _rig_dict(_rig_cfg("tiny", TINY_RIGS[2]))
    feed = lambda slam, slot, k: slam.new_images([r1[1][k] if s == slot else None for s in range(slam.n)],
                                                 [r1[2][k] if s == slot else None for s in range(slam.n)], [k / 20.0] * slam.n)
    whole = StereoSlamBatch(cfg, w, h, 1)
    whole.assign_rigs([0], whole.add_rigs([rig1]))
    ref = []
    for k in range(10):
        feed(whole, 0, k)
        ref.append(_snapshot(whole, 0))
    ref_final = _final(whole, 0)
    whole.close()
    a = StereoSlamBatch(cfg, w, h, 2)
    a.assign_rigs([0], a.add_rigs([rig1]))
    for k in range(5):
        feed(a, 0, k)
        assert _snapshot(a, 0) == ref[k]
    snap = a.save([0])[0]
    assert bytes(snap.info.cam) == bytes(hip_lib.CameraSettings.from_dict(r1[0])), "the header has the slot's settings"
    b = StereoSlamBatch(cfg, w, h, 3)
    ids = b.add_rigs([rig2, rig1])                        # (equal settings under another id)
    b.assign_rigs([2, 1], [ids[1], ids[0]])
    for bad in (0, 1):                                    # rig 0 and rig 2: other settings
        with pytest.raises(SvoError):
            b.submit_load([bad], [snap])
        b.wait()
    assert b.stats(0).frame_id == 0 and b.num_keyframes(0) == 0 and b.get_trajectory(0).shape == (0, 6)
    assert _snapshot(a, 0) == ref[4]
    b.load([2], [snap])
    assert _snapshot(b, 2) == ref[4] and b.slot_rig(2)[0] == ids[1]
    for k in range(5, 10):
        feed(b, 2, k)
        assert _snapshot(b, 2) == ref[k], k
    assert _final(b, 2) == ref_final
    # multi_seq.move: the settings travel; the target ctx gets an equal rig when it has none
    c = StereoSlamBatch(cfg, w, h, 2)
    multi_seq.move(a, [0], c, [1])
    rig, cam = c.slot_rig(1)
    assert rig >= 1 and bytes(cam) == bytes(a.slot_rig(0)[1]) and c.rigs()[0] == 2
    for k in range(5, 10):
        feed(c, 1, k)
        assert _snapshot(c, 1) == ref[k], k
    a.close(); b.close(); c.close()


def test_rigs_that_no_slot_uses_change_nothing():
    """8 `tiny` slots, 8 frames: a ctx that adds rigs (one with maps) and binds none gives the bytes of a ctx that
    adds none, with the same launch shapes"""
    cfg = synth.CONFIGS["tiny"]
    w, h = cfg["width"], cfg["height"]
    rendered = [synth.make_sequence_gpu("tiny", 8, 1000 + s, motion_scale=8.0) for s in range(8)]
    out = []
    for add in (False, True):
        slam = StereoSlamBatch(cfg, w, h, 8)
        if add:
            slam.add_rigs([_rig_dict(_rig_cfg("tiny", TINY_RIGS[1]), _tiny_maps(1)), _rig_dict(_rig_cfg("tiny", TINY_RIGS[2]))])
        frames = _play(slam, rendered, [8] * 8)
        out.append((frames, [_final(slam, s) for s in range(8)], slam.launch_shapes(), [slam.slot_rig(s)[0] for s in range(8)]))
        slam.close()
    assert out[0] == out[1]
    assert any(StatsView(snap[4]).is_keyframe for fr in out[0][0][1:] for snap in fr.values()), "a keyframe inside the run"


def test_bad_rig_calls_leave_the_ctx_as_it_was():
    cfg = synth.CONFIGS["tiny"]
    w, h = cfg["width"], cfg["height"]
    slam = StereoSlamBatch(cfg, w, h, 2)
    good = _rig_dict(_rig_cfg("tiny", TINY_RIGS[1]))
    mx, my = RR.identity_maps(w, h)
    for change in (dict(fx=float("nan")), dict(p2=float("inf")), dict(fx=0.0), dict(fy=-1.0)):
        with pytest.raises(SvoError):
            slam.add_rigs([good, dict(good, **change)])
    three = hip_lib.Rig.from_dict(good)
    three.left_map_x, three.left_map_y, three.right_map_x = mx.ctypes.data, my.ctypes.data, mx.ctypes.data
    ids = (C.c_int * 1)(-5)
    assert lib().svo_ctx_add_rigs(slam._ctx, C.byref(three), 1, ids) == -1 and ids[0] == -5
    assert slam.rigs() == (1, 0), "nothing added"
    one = lambda v: (C.c_int * 1)(v)
    assert lib().svo_ctx_assign_rigs(slam._ctx, one(2), one(0), 1) == -1           # a bad slot
    assert lib().svo_ctx_assign_rigs(slam._ctx, one(0), one(1), 1) == -1           # an unknown rig
    assert lib().svo_ctx_remove_rigs(slam._ctx, one(0), 1) == -1 and lib().svo_ctx_remove_rigs(slam._ctx, one(3), 1) == -1
    assert slam.add_rigs([good]) == [1]
    slam.assign_rigs([1], [1])
    assert [slam.slot_rig(s)[0] for s in range(2)] == [0, 1]
    slam.close()
