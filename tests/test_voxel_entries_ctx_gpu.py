"""The voxel entries inside a ctx on the GPU, byte for byte against tests/voxel_entries_ref.py: the save job in host and
device mode (queued behind a fuse it must see), its statuses; the load job in replace and merge mode, FULL on the
mirror with nothing changed, a fuse queued right behind a load admitted on the loaded count, the rejections at the
call; the resize up and down and refused, with the memory following, and a fuse after it against a twin ctx that had
the larger map from the start; fuse_clouds(grow=); checkpoint and resume of a tracked and fused sequence through
Snapshot and tobytes / frombytes; and multi_seq.move(voxel_maps=True) between two ctxs.

The frames are the `tiny` sequence cut to its central 256 x 192 pixels (as tests/test_voxel_prune_ctx_gpu.py): at step 16
a cloud has 192 points, at step 4 it has 3072, four times the 768 entries a map of 1 << 10 may hold. The named slots
0 and 2 of a ctx of 3 slots lie in its two sequence groups; slot 1 has no map."""
import os

import numpy as np
import pytest
import torch

import voxel_entries_cases as EC
import voxel_entries_ref as ER
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib, multi_seq, synth
from stereo_svo_slam_amd.jobs import VoxelSaves
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu
W, H, X0, Y0 = 256, 192, 32, 24
WIN = dict(win=7, search_x=9, search_y=2)
KW = dict(step=16, **WIN)
POINTS = 192
VOXEL, LOG2 = 0.1, 10
LIMIT = 768
FRAMES = 8
MAPPED = [0, 2]
INVALID, CAPACITY = "error -1:", "error -4:"


def _batch(cfg, n_slots=3, groups=2, maps=MAPPED, log2=LOG2):
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
    if maps:
        b.set_voxel_maps(VOXEL, log2, seqs=maps)
    return b


@pytest.fixture(scope="module")
def tiny():
    """tiny cut to 256 x 192, 2 sequences of 8 frames of fast motion, gray on the device: shared, never changed"""
    out = []
    for seed in (1, 11):
        cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", FRAMES, seed, motion_scale=4.0)
        cut = lambda imgs: [x[Y0:Y0 + H, X0:X0 + W].contiguous() for x in imgs]
        out.append((cut(L), cut(R), [float(t) for t in ts]))
    torch.cuda.synchronize()
    cfg = dict(cfg, width=W, height=H, cx=cfg["cx"] - X0, cy=cfg["cy"] - Y0)
    return cfg, out


def _frames(n, seqs, k, slots):
    L, R, ts = [None] * n, [None] * n, [0.0] * n
    for s, q in slots.items():
        L[s], R[s], ts[s] = seqs[q][0][k], seqs[q][1][k], seqs[q][2][k]
    return L, R, ts


def _entries(job, i):
    e = job.entries(i)
    if e is None:
        return None
    return e.cpu().numpy().reshape(-1).view(ER.ENTRY).copy() if job.device_mode else e.copy()


def _state(b, seqs=None):
    """what a map is, per named slot: (packed entry bytes, exported point bytes, n_fused, n_outside)"""
    save, pts = b.save_voxel_maps(seqs), b.export_voxel_maps(seqs)
    named = range(b.n) if seqs is None else seqs
    out = []
    for i, s in enumerate(named):
        info = b.voxel_map_info(s)
        out.append(None if info is None else (_entries(save, i).tobytes(), pts.points(i).tobytes(), info["n_fused"], info["n_outside"], info["n_voxels"]))
    return out


@pytest.fixture(scope="module")
def played(tiny):
    """3 slots in 2 groups; slots 0 and 2 have a map and play 3 frames, each with a fuse and an organized cloud job for
    the statement; host and device saves are queued right behind the last fuse, nothing waited for until the end"""
    cfg, seqs = tiny
    b = _batch(cfg)
    clouds, packed = [], []
    for k in range(3):
        packed.append(b.pack_images(*_frames(3, seqs, k, {0: 0, 2: 1})))
        b.submit_packed(packed[-1])
        clouds.append(b.submit_cloud("frames", None, layout="organized", **KW))
        b.submit_fuse("frames", None, stamp=k + 1, **KW)
    host = b.submit_save_voxel_maps(None, capacities=LIMIT)
    dev = b.submit_save_voxel_maps(None, capacities=LIMIT, device=True)
    small = b.submit_save_voxel_maps(None, capacities=1)
    filt = b.submit_save_voxel_maps(MAPPED, capacities=LIMIT, min_count=2, min_stamp=[2, 3])
    b.wait()
    refs = {s: VR.Map(VOXEL, LOG2) for s in MAPPED}
    for k, cloud in enumerate(clouds):
        for s in MAPPED:
            org = cloud.organized(s)
            assert org is not None and org.size == POINTS and refs[s].admits(POINTS)
            refs[s].fuse(org.ravel(), k + 1)
    yield dict(cfg=cfg, seqs=seqs, b=b, clouds=clouds, host=host, dev=dev, small=small, filt=filt, refs=refs)
    b.close()


def test_save_in_host_and_device_mode_sees_the_fuse_in_front_of_it(played):
    refs, b = played["refs"], played["b"]
    assert all(r.n_voxels > 100 for r in refs.values())
    for job in (played["host"], played["dev"]):
        assert [job.status(i) for i in range(3)] == [hip_lib.VOXEL_OK, hip_lib.VOXEL_NO_MAP, hip_lib.VOXEL_OK]
        assert job.entries(1) is None and [int(job.info(i)["seq"]) for i in range(3)] == [0, 1, 2]
        for i in MAPPED:
            seg, want = job.info(i), ER.pack(refs[i])
            assert (int(seg["n_points"]), int(seg["n_voxels"]), int(seg["n_fused"]), int(seg["first_point"])) == (len(want), refs[i].n_voxels, refs[i].n_fused, LIMIT * i)
            assert _entries(job, i).tobytes() == want.tobytes() and job.voxel(i) == np.float32(VOXEL) and int(seg["log2_capacity"]) == LOG2
        # exactly [first_point, first_point + n_points) is written
        raw = job.entries_buffer.cpu().numpy()
        n0 = int(job.info(0)["n_points"])
        assert not raw[n0:2 * LIMIT].any() and not raw[2 * LIMIT + int(job.info(2)["n_points"]):].any()
    small = played["small"]
    assert [small.status(i) for i in range(3)] == [hip_lib.VOXEL_TOO_SMALL, hip_lib.VOXEL_NO_MAP, hip_lib.VOXEL_TOO_SMALL]
    assert [int(small.info(i)["n_voxels"]) for i in MAPPED] == [refs[s].n_voxels for s in MAPPED] and not small.entries_buffer.numpy().any()
    filt = played["filt"]
    for i, (s, stamp) in enumerate(zip(MAPPED, (2, 3))):
        want = ER.pack(refs[s], min_count=2, min_stamp=stamp)
        assert 0 < len(want) < refs[s].n_voxels and _entries(filt, i).tobytes() == want.tobytes()
    # the stage pack of the same state: a map of the caller's fused from the same records
    h = hip_lib.Handle(0, 1024)
    for s in MAPPED:
        m = h.voxel_new(hip_lib.voxel_params(VOXEL, LOG2))
        for k, cloud in enumerate(played["clouds"]):
            rec = np.ascontiguousarray(cloud.organized(s).ravel())
            h.voxel_fuse([(torch.from_numpy(rec.view(np.uint8).reshape(-1, 16)).cuda(), 0, k + 1)], [m])
        ent, n = h.voxel_pack(m)
        assert n == refs[s].n_voxels and ent.cpu().numpy().tobytes() == _entries(played["host"], s).tobytes() == _entries(played["dev"], s).tobytes()
    # the export of the same state is the extraction formula on the saved entries
    pts = b.export_voxel_maps(MAPPED)
    for i, s in enumerate(MAPPED):
        assert pts.points(i).tobytes() == ER.extract_of(_entries(played["host"], s), VOXEL).tobytes() == refs[s].extract().tobytes()


def test_tobytes_and_frombytes(played):
    host, dev = played["host"], played["dev"]
    with pytest.raises(ValueError):
        host.tobytes(2)                                                             # delivered by the ctx's wait: the header's counters were never read
    host.wait(), dev.wait()
    assert host.maps[1] is None and host.maps[2]["drop_flags"] == 0 and host.maps[2]["n_outside"] == played["refs"][2].n_outside
    blob = host.tobytes(2)
    assert blob == dev.tobytes(2) and len(blob) == 64 + 40 * played["refs"][2].n_voxels
    back = VoxelSaves.frombytes(blob)
    assert back.status(0) == hip_lib.VOXEL_OK and back.entries(0).tobytes() == _entries(host, 2).tobytes() and back.voxel(0) == np.float32(VOXEL)
    h = back.header
    assert (int(h["n"]), int(h["log2_capacity"]), int(h["n_fused"]), int(h["drop_flags"])) == (played["refs"][2].n_voxels, LOG2, played["refs"][2].n_fused, 0)
    assert np.uint32(h["voxel_bits"]).view(np.float32) == np.float32(VOXEL) and back.tobytes(0) == blob
    with pytest.raises(ValueError):
        host.tobytes(1)                                                             # a slot without a map
    for bad in (blob[:63], blob[:-1], blob + b"\0", b"\0" * 64):
        with pytest.raises(ValueError):
            VoxelSaves.frombytes(bad)
    with pytest.raises(ValueError):
        back.submit()


def test_load_in_replace_and_merge_mode(played):
    refs, host, dev = played["refs"], played["host"], played["dev"]
    b = _batch(played["cfg"])
    try:
        for job in (host, dev):                                                     # entries from the host, then from the device
            loads = b.load_voxel_maps(None, job)                                    # (the slot that had no map is left out)
            assert loads.seqs == MAPPED and [loads.status(i) for i in range(2)] == [hip_lib.VOXEL_LOADED] * 2 and loads.device_mode == job.device_mode
            for i, s in enumerate(MAPPED):
                e, n = loads.info[i], refs[s].n_voxels
                assert (int(e["seq"]), int(e["n_offered"]), int(e["n_merged"]), int(e["n_skipped"]), int(e["n_claimed"]), int(e["n_voxels"])) == (s, n, n, 0, n, n)
            state = _state(b)
            for s in MAPPED:                                                        # replace: exactly the entries, however often
                assert state[s][:3] == (ER.pack(refs[s]).tobytes(), refs[s].extract().tobytes(), refs[s].n_fused) and state[s][3] == 0
            assert state[1] is None
        # merge: what fusing the records twice would have given (the bound counts records: twice the entries need a larger map)
        assert any(2 * refs[s].n_voxels > LIMIT for s in MAPPED)
        b.resize_voxel_maps(11)
        loads = b.load_voxel_maps(MAPPED, [_entries(host, s) for s in MAPPED], merge=True, voxel=VOXEL)
        twice = {s: VR.Map(VOXEL, LOG2) for s in MAPPED}
        for i, s in enumerate(MAPPED):
            ER.merge(twice[s], ER.pack(refs[s]), VOXEL)
            want = ER.merge(twice[s], ER.pack(refs[s]), VOXEL)
            e = loads.info[i]
            assert {k: int(e[k]) for k in want} == want and want["n_claimed"] == 0 and int(e["n_voxels"]) == refs[s].n_voxels
        state = _state(b, MAPPED)
        for i, s in enumerate(MAPPED):
            assert state[i][0] == ER.pack(twice[s]).tobytes() and state[i][2] == 2 * refs[s].n_fused
        # skipped records and an empty span
        ent, which = EC.skipped_span()
        loads = b.load_voxel_maps(MAPPED, [ent, None], merge=True, voxel=VOXEL)
        assert (int(loads.info[0]["n_skipped"]), int(loads.info[0]["n_merged"]), int(loads.info[1]["n_offered"])) == (3, 5, 0)
        ER.merge(twice[0], ent, VOXEL)
        assert _state(b, [0])[0][0] == ER.pack(twice[0]).tobytes()
    finally:
        b.close()


def test_load_full_on_the_mirror_and_a_fuse_right_behind_a_load(played, tiny):
    cfg, seqs = tiny
    b = _batch(cfg)
    try:
        b.new_images(*_frames(3, seqs, 0, {0: 0, 2: 1}))
        many, few = EC.lattice_entries(LIMIT - POINTS + 1), EC.lattice_entries(10, first=100000)
        # the mirror says empty; the fuse right behind the load is admitted on the loaded count: 577 + 192 > 768
        loads = b.submit_load_voxel_maps(MAPPED, [many, few], voxel=VOXEL)
        fuse = b.submit_fuse("frames", MAPPED, stamp=5, **KW)
        b.wait()
        assert [loads.status(i) for i in (0, 1)] == [hip_lib.VOXEL_LOADED] * 2
        assert [int(f["status"]) for f in fuse.info] == [hip_lib.FUSE_FULL, hip_lib.FUSE_OK]
        # and the other way round: a replace load makes room for the fuse behind it
        loads = b.submit_load_voxel_maps([0], [few], voxel=VOXEL)
        fuse = b.submit_fuse("frames", [0], stamp=6, **KW)
        b.wait()
        assert loads.status(0) == hip_lib.VOXEL_LOADED and int(fuse.info[0]["status"]) == hip_lib.FUSE_OK and int(fuse.info[0]["n_voxels"]) > 10
        # FULL: on the bound, replace takes the map as empty, merge does not; nothing changes and the ctx carries on
        before = _state(b, MAPPED)
        n0 = before[0][4]
        assert 0 < n0 < LIMIT
        over = EC.lattice_entries(LIMIT + 1, first=200000)
        for srcs, merge, want in (([over, None], False, [hip_lib.VOXEL_LOAD_FULL, hip_lib.VOXEL_LOADED]),
                                  ([over[:LIMIT - n0 + 1], None], True, [hip_lib.VOXEL_LOAD_FULL, hip_lib.VOXEL_LOADED])):
            loads = b.load_voxel_maps(MAPPED, srcs, merge=merge, voxel=VOXEL)
            assert [loads.status(i) for i in (0, 1)] == want and int(loads.info[0]["n_voxels"]) == n0 and int(loads.info[0]["n_offered"]) == 0
            assert _state(b, [0]) == before[:1]
        loads = b.load_voxel_maps([0], [over[:LIMIT - n0]], merge=True, voxel=VOXEL)          # exactly on the limit
        assert loads.status(0) == hip_lib.VOXEL_LOADED and int(loads.info[0]["n_voxels"]) == LIMIT
        # rejected at the call with nothing queued
        last_bit = float(np.nextafter(np.float32(VOXEL), np.float32(1.0)))
        state = _state(b, MAPPED)
        for kw in (dict(seqs=MAPPED, saves=[few, few], voxel=[VOXEL, last_bit]), dict(seqs=[0, 0], saves=[few, few], voxel=VOXEL),
                   dict(seqs=[3], saves=[few], voxel=VOXEL)):
            with pytest.raises(hip_lib.SvoError, match=INVALID):
                b.load_voxel_maps(**kw)
        lib, ctx = hip_lib.lib(), b._ctx
        spans = np.zeros(1, hip_lib.VOXEL_ENTRY_SPAN_DTYPE)
        spans["voxel"] = VOXEL
        info = np.zeros(1, hip_lib.VOXEL_LOAD_INFO_DTYPE)
        one = (hip_lib.C.c_int * 1)(0)
        assert lib.svo_submit_load_voxel_maps(ctx, one, 1, spans.ctypes.data, 2, hip_lib.MEM_HOST, info.ctypes.data) == -1     # an unknown mode
        assert lib.svo_submit_load_voxel_maps(ctx, one, 1, spans.ctypes.data, 0, 7, info.ctypes.data) == -1                    # an unknown mem
        assert lib.svo_submit_load_voxel_maps(ctx, one, 1, spans.ctypes.data, 0, hip_lib.MEM_HOST, None) == -1                 # no info
        assert lib.svo_submit_load_voxel_maps(ctx, one, 1, None, 0, hip_lib.MEM_HOST, info.ctypes.data) == -1                  # no spans
        spans["n"], spans["entries"] = 3, few.ctypes.data + 4
        assert lib.svo_submit_load_voxel_maps(ctx, one, 1, spans.ctypes.data, 0, hip_lib.MEM_HOST, info.ctypes.data) == -1     # misaligned
        spans["n"] = -1
        assert lib.svo_submit_load_voxel_maps(ctx, one, 1, spans.ctypes.data, 0, hip_lib.MEM_HOST, info.ctypes.data) == -1
        b.wait()
        assert _state(b, MAPPED) == state
        # a slot without a map is not checked for its edge, and answers NO_MAP
        loads = b.load_voxel_maps([1], [few], voxel=0.5)
        assert loads.status(0) == hip_lib.VOXEL_LOAD_NO_MAP
    finally:
        b.close()


def test_resize_up_down_and_refused(played, tiny):
    cfg, seqs = tiny
    b, twin = _batch(cfg), _batch(cfg, log2=12)
    try:
        for x in (b, twin):
            x.load_voxel_maps(None, played["host"])
            x.new_images(*_frames(3, seqs, 0, {0: 0, 2: 1}))
        before, mem0 = _state(b), b.memory().device_bytes
        b.resize_voxel_maps(12)                                                     # every slot; slot 1 has no map and is skipped
        grown = hip_lib.voxel_map_bytes(12) - hip_lib.voxel_map_bytes(10)
        assert b.memory().device_bytes - mem0 == 2 * grown
        assert [None if i is None else i["log2_capacity"] for i in map(b.voxel_map_info, range(3))] == [12, None, 12]
        assert _state(b) == before == _state(twin)
        # a fuse after the resize: the twin that had the larger map from the start, byte for byte
        for x in (b, twin):
            x.fuse_clouds("frames", None, stamp=9, **KW)
        after = _state(b)
        assert after == _state(twin) and all(after[s][2] > before[s][2] for s in MAPPED)       # (n_fused grew)
        # down again where it fits; refused where it does not, with nothing changed
        mem1 = b.memory().device_bytes
        b.resize_voxel_maps(10, [2])
        assert mem1 - b.memory().device_bytes == grown
        assert b.voxel_map_info(2)["log2_capacity"] == 10 and _state(b) == after
        b.load_voxel_maps([0], [EC.lattice_entries(LIMIT + 1)], voxel=VOXEL)
        state, mem1 = _state(b), b.memory().device_bytes
        with pytest.raises(hip_lib.SvoError, match=CAPACITY):
            b.resize_voxel_maps(10)                                                 # slot 0 does not fit: slot 2 is not touched either
        with pytest.raises(hip_lib.SvoError, match=CAPACITY):
            b.resize_voxel_maps(10, [2, 0])
        for bad in (9, 27):
            with pytest.raises(hip_lib.SvoError, match=INVALID):
                b.resize_voxel_maps(bad)
        with pytest.raises(hip_lib.SvoError, match=INVALID):
            b.resize_voxel_maps(12, [0, 0])
        assert _state(b) == state and b.memory().device_bytes == mem1 and b.voxel_map_info(0)["log2_capacity"] == 12
        b.resize_voxel_maps(11, [0])                                                # 769 <= 1536
        assert _state(b, [0]) == state[:1]
    finally:
        b.close(); twin.close()


def test_fuse_clouds_grows_a_map_the_first_cloud_overfills(tiny):
    cfg, seqs = tiny
    b, twin = _batch(cfg), _batch(cfg, log2=12)
    kw = dict(step=4, **WIN)
    try:
        for x in (b, twin):
            x.new_images(*_frames(3, seqs, 0, {0: 0, 2: 1}))
        plain = b.fuse_clouds("frames", None, stamp=1, **kw)
        assert [int(f["status"]) for f in plain.info] == [hip_lib.FUSE_FULL, hip_lib.FUSE_NO_MAP, hip_lib.FUSE_FULL]    # 3072 points, limit 768
        assert b.voxel_map_info(0)["log2_capacity"] == 10
        short = b.fuse_clouds("frames", None, stamp=1, grow=11, **kw)               # 1536 is not enough either
        assert [int(f["status"]) for f in short.info] == [hip_lib.FUSE_FULL, hip_lib.FUSE_NO_MAP, hip_lib.FUSE_FULL]
        assert b.voxel_map_info(0)["log2_capacity"] == 11
        job = b.fuse_clouds("frames", None, stamp=1, grow=14, **kw)                 # stops at the first size that admits: 12
        want = twin.fuse_clouds("frames", None, stamp=1, **kw)
        assert [int(f["status"]) for f in job.info] == [hip_lib.FUSE_OK, hip_lib.FUSE_NO_MAP, hip_lib.FUSE_OK]
        assert job.info.tobytes() == want.info.tobytes()
        assert [None if i is None else i["log2_capacity"] for i in map(b.voxel_map_info, range(3))] == [12, None, 12]
        assert _state(b) == _state(twin)
    finally:
        b.close(); twin.close()


def test_checkpoint_and_resume(tiny):
    cfg, seqs = tiny
    k = FRAMES // 2
    whole, a, b = _batch(cfg, 1, 1, [0]), _batch(cfg, 1, 1, [0]), _batch(cfg, 1, 1, [0], log2=11)
    try:
        def play(x, frames):
            poses = []
            for f in frames:
                x.new_images(*_frames(1, seqs, f, {0: 0}))
                x.fuse_clouds("frames", None, stamp=f + 1, **KW)
                x.prune_voxel_maps(None, min_stamp=max(0, f - 1))                   # (what a resumed map must still know: its stamps)
                poses.append(x.pose(0).tobytes())
            return poses
        want = play(whole, range(2 * k))
        assert play(a, range(k)) == want[:k]
        snap, blob = a.save([0]), a.save_voxel_maps([0]).tobytes(0)
        b.load([0], snap)
        info = b.load_voxel_maps([0], VoxelSaves.frombytes(blob)).info[0]
        assert int(info["status"]) == hip_lib.VOXEL_LOADED and int(info["n_voxels"]) == a.voxel_map_info(0)["n_voxels"] > 0
        assert play(b, range(k, 2 * k)) == want[k:]
        sb, sw = _state(b), _state(whole)
        assert sb[0][:2] == sw[0][:2] and sb[0][4] == sw[0][4] and len(sb[0][0]) > 0
    finally:
        whole.close(); a.close(); b.close()


def test_move_with_voxel_maps(played, tiny):
    cfg, seqs = tiny
    src, dst = _batch(cfg), _batch(cfg, 2, 1, [1], log2=11)
    try:
        src.load_voxel_maps(None, played["host"])
        src.new_images(*_frames(3, seqs, 0, {0: 0, 2: 1}))
        was = _state(src)
        with pytest.raises(ValueError):
            multi_seq.move(src, [2], dst, [0], voxel_maps=True)                     # dst's slot 0 has no map
        with pytest.raises(ValueError):
            multi_seq.move(src, [1], dst, [1], voxel_maps=True)                     # src's slot 1 has none
        dst.set_voxel_maps(0.2, 11, seqs=[0])
        with pytest.raises(ValueError):
            multi_seq.move(src, [2], dst, [0], voxel_maps=True)                     # another edge
        pose = src.pose(2).tobytes()
        assert _state(src) == was and src.pose(2).tobytes() == pose                 # nothing moved
        snaps, loads = multi_seq.move(src, [2], dst, [1], voxel_maps=True)
        assert len(snaps) == 1 and loads.status(0) == hip_lib.VOXEL_LOADED and dst.pose(1).tobytes() == pose
        got = _state(dst, [1])[0]
        assert got[:3] == was[2][:3] and dst.voxel_map_info(1)["log2_capacity"] == 11
        now = _state(src)
        assert now[0] == was[0] and now[2][4] == 0 and now[2][0] == b""
        assert isinstance(multi_seq.move(dst, [1], src, [2]), list) and _state(dst, [1])[0][4] == got[4]     # without the flag maps stay
    finally:
        src.close(); dst.close()
