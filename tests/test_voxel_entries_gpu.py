"""svo_voxel_pack, svo_voxel_merge and svo_voxel_rehash on the GPU against tests/voxel_entries_ref.py, byte for byte,
at the smallest shapes at which each can go wrong: a table of 64 entries whose probe chain wraps, at 0, 1 and 48 entries;
a table of two tiles; spans of 0, 1, 255, 256 and 257 records; a key that repeats inside a wavefront, across
wavefronts and across workgroups; accumulators that wrap; the three kinds of skipped record; several spans into several
maps; the load bound on and past its limit; every rejection with nothing written. A packed span is also compared with
the raw table read back with torch and sorted on the host, which does not go through the pack kernel, and after every
merge and rehash every key is looked up from its home in the raw table and, where the load bound admits it, fused once
more."""
import copy

import numpy as np
import pytest
import torch

import voxel_cases as VC
import voxel_entries_cases as EC
import voxel_entries_ref as ER
import voxel_prune_cases as PC
import voxel_prune_ref as PR
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib

pytestmark = pytest.mark.gpu
GUARD = 256                      # bytes of 0xA5 before and after a buffer
FILTERS = (dict(), dict(min_count=2), dict(min_stamp=2), dict(min_count=3, min_stamp=2))
INVALID, CAPACITY = "error -1:", "error -4:"
Cp = hip_lib.C


@pytest.fixture(scope="module")
def handle():
    return hip_lib.Handle(0, 1024)


def _dev(rec):
    buf = np.zeros(len(rec) + 1, VR.POINT)
    buf[:len(rec)] = rec
    return torch.from_numpy(buf.view(np.uint8).reshape(-1, 16)).cuda()[:len(rec)]


def _edev(ent):
    buf = np.zeros(len(ent) + 1, ER.ENTRY)
    buf[:len(ent)] = ent
    return torch.from_numpy(buf.view(np.uint8).reshape(-1, 40)).cuda()[:len(ent)]


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _guarded_map(h, params):
    buf, data = _guarded(hip_lib.voxel_map_bytes(params.log2_capacity))
    m = (data, params)
    h.voxel_clear(m)
    return buf, m


def _guards_ok(buf):
    raw = buf.cpu().numpy()
    return bool((raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all())


def _fused(h, case, log2=None):
    """the case's map on the GPU (log2: under another capacity) and the statement's map"""
    voxel, lg, drop = case["maps"][0]
    lg = lg if log2 is None else log2
    buf, m = _guarded_map(h, hip_lib.voxel_params(voxel, lg, drop))
    ref = VR.Map(voxel, lg, drop)
    for call in case["calls"]:
        h.voxel_fuse([(_dev(r), mi, s) for r, mi, s in call], [m])
        for r, _, s in call:
            ref.fuse(r, s)
    return buf, m, ref


def _pack(h, m, **kw):
    ent, n = h.voxel_pack(m, **kw)
    assert ent.shape[0] == n
    return ent.cpu().numpy().reshape(-1).view(ER.ENTRY).copy()


def _extract(h, m, **kw):
    pts, n = h.voxel_extract(m, **kw)
    return pts.cpu().numpy()[:n].copy().view(VR.POINT).reshape(-1)


def _raw(m):
    """the table read back with torch: (keys uint64[capacity], acc uint32[capacity, 8])"""
    raw = m[0].cpu().numpy()
    cap = 1 << m[1].log2_capacity
    return raw[256:256 + 8 * cap].view("<u8").copy(), raw[256 + 8 * cap:256 + 40 * cap].view("<u4").reshape(cap, 8).copy()


def _raw_sorted(m):
    keys, acc = _raw(m)
    full = keys != np.uint64(VR.EMPTY)
    out = np.zeros(int(full.sum()), ER.ENTRY)
    order = np.argsort(keys[full], kind="stable")
    out["key"], out["acc"] = keys[full][order], acc[full][order]
    return out


def _check(h, m, ref, filters=FILTERS):
    """counters, the packed bytes three ways, the extraction, and every key reachable from its home in the raw table"""
    info = h.voxel_info(m)
    assert (info["n_voxels"], info["n_fused"], info["n_outside"], info["overflow"]) == (ref.n_voxels, ref.n_fused, ref.n_outside, 0)
    got = _pack(h, m)
    assert got.tobytes() == ER.pack(ref).tobytes() == _raw_sorted(m).tobytes()
    for kw in filters:
        packed = _pack(h, m, **kw)
        assert packed.tobytes() == ER.pack(ref, **kw).tobytes(), kw
        assert _extract(h, m, **kw).tobytes() == ref.extract(**kw).tobytes() == ER.extract_of(packed, ref.voxel).tobytes(), kw
    table = [int(k) for k in _raw(m)[0]]
    assert all(PR.lookup(table, int(k), ref.log2_capacity) is not None for k in ref.keys)


def _reach(h, m, ref):
    """a record per key fused afterwards raises each count by one and claims nothing (where the load bound admits it)"""
    assert ref.n_voxels and ref.admits(ref.n_voxels)
    rec = PC.records_of_keys(ref.keys, ref.voxel)
    h.voxel_fuse([(_dev(rec), 0, 0)], [m])
    after = copy.deepcopy(ref)
    after.fuse(rec, 0)
    assert after.n_voxels == ref.n_voxels and np.array_equal(after.acc[:, 0], (ref.acc[:, 0] + np.uint64(1)) & VR.MASK32)
    assert h.voxel_info(m)["n_voxels"] == ref.n_voxels and _pack(h, m).tobytes() == ER.pack(after).tobytes()


def _merge(h, m, ref, ent, voxel=None):
    voxel = ref.voxel if voxel is None else voxel
    res, = h.voxel_merge([(_edev(ent), 0, voxel)], [m])
    assert res == ER.merge(ref, ent, voxel)
    return res


# ---------------------------------------------------------------------------------------------------------- pack

@pytest.mark.parametrize("n", [0, 1, 48])
def test_pack_of_the_table_whose_chain_wraps(handle, n):
    buf, m, ref = _fused(handle, EC.small(n))
    assert ref.n_voxels == n
    keys, _ = _raw(m)
    if n == 48:
        assert keys[63] != np.uint64(VR.EMPTY) and keys[0] != np.uint64(VR.EMPTY) and VR.home(keys[0], 6) == VC.CHAIN_HOME   # the chain wrapped
    _check(handle, m, ref, (dict(), dict(min_stamp=2), dict(min_count=2)))
    assert handle.voxel_pack(m)[1] == n and _guards_ok(buf)


def test_pack_over_two_tiles_and_both_filter_edges(handle):
    buf, m, ref = _fused(handle, EC.tiles())
    keys, _ = _raw(m)
    full = keys != np.uint64(VR.EMPTY)
    assert full[:256].sum() > 64 and full[256:].sum() > 64                       # ranks cross wavefront and tile edges
    _check(handle, m, ref, FILTERS + (dict(min_count=1), dict(min_count=3, min_stamp=3), dict(min_stamp=4)))
    p2, s2 = _pack(handle, m, min_count=2), _pack(handle, m, min_stamp=2)
    assert (p2["acc"][:, 0] == 2).any() and (p2["acc"][:, 0] >= 2).all() and 0 < len(p2) < ref.n_voxels
    assert (s2["acc"][:, 7] == 2).any() and (s2["acc"][:, 7] >= 2).all() and 0 < len(s2) < ref.n_voxels
    assert len(_pack(handle, m, min_stamp=4)) == 0
    # a buffer of the caller's, larger than needed: only [0, n) is written
    gbuf, ent = _guarded(40 * (ref.n_voxels + 3))
    _, n = handle.voxel_pack(m, entries=ent)
    raw = ent.cpu().numpy()
    assert n == ref.n_voxels and raw[:40 * n].tobytes() == ER.pack(ref).tobytes() and (raw[40 * n:] == 0xA5).all() and _guards_ok(gbuf)


def test_pack_into_a_capacity_one_short(handle):
    _, m, ref = _fused(handle, EC.tiles())
    for kw, kept in ((dict(), ref.n_voxels), (dict(min_count=2), len(ER.pack(ref, min_count=2)))):
        gbuf, ent = _guarded(40 * (kept - 1))
        n = Cp.c_int64(-1)
        f = hip_lib.VoxelFilter(kw.get("min_count", 0), 0)
        rc = hip_lib.lib().svo_voxel_pack(handle._h, Cp.byref(hip_lib._voxel_map(m)), Cp.byref(f), Cp.c_void_p(ent.data_ptr()), Cp.c_int64(kept - 1),
                                          Cp.byref(n))
        assert rc == -4 and n.value == kept and (gbuf.cpu().numpy() == 0xA5).all()
        rc = hip_lib.lib().svo_voxel_pack(handle._h, Cp.byref(hip_lib._voxel_map(m)), Cp.byref(f), None, Cp.c_int64(0), Cp.byref(n))
        assert rc == 0 and n.value == kept                                         # entries == NULL only counts


def test_pack_rejections(handle):
    buf, m, ref = _fused(handle, EC.small(48))
    raw = buf.cpu().numpy().copy()
    data, params = m
    ent = torch.full((48 * 40 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip_lib.SvoError, match=INVALID):
        handle.voxel_pack(m, entries=ent.data_ptr() + 4, capacity=48)                # not 8-byte aligned
    assert handle.voxel_pack(m, entries=ent.data_ptr() + 8, capacity=48)[1] == 48    # 8-byte aligned is enough
    assert ent.cpu().numpy()[8:].tobytes() == ER.pack(ref).tobytes()
    ent.fill_(0xA5)
    with pytest.raises(hip_lib.SvoError, match=INVALID):
        handle.voxel_pack(m, entries=ent.data_ptr(), capacity=-1)
    for other in (hip_lib.voxel_params(0.5, 6), hip_lib.voxel_params(1.0, 7), hip_lib.voxel_params(1.0, 6, 2), hip_lib.voxel_params(1.0, 5)):
        with pytest.raises(hip_lib.SvoError, match=INVALID):
            handle.voxel_pack((data, other), entries=ent.data_ptr(), capacity=48)
    f = hip_lib.VoxelFilter(0, 0)
    f._reserved[1] = 1
    n = Cp.c_int64(-7)
    lib = hip_lib.lib()
    assert lib.svo_voxel_pack(handle._h, Cp.byref(hip_lib._voxel_map(m)), Cp.byref(f), Cp.c_void_p(ent.data_ptr()), Cp.c_int64(48), Cp.byref(n)) == -1
    assert lib.svo_voxel_pack(handle._h, Cp.byref(hip_lib._voxel_map(m)), None, Cp.c_void_p(ent.data_ptr()), Cp.c_int64(48), None) == -1
    assert n.value == -7 and (ent.cpu().numpy() == 0xA5).all() and np.array_equal(buf.cpu().numpy(), raw)


# ---------------------------------------------------------------------------------------------------------- merge

@pytest.mark.parametrize("src,log2", [("small", 6), ("tiles", 10), ("tiles", 9)])
def test_merge_of_a_pack_into_an_empty_map(handle, src, log2):
    _, a, aref = _fused(handle, EC.small(48) if src == "small" else EC.tiles())
    packed = _pack(handle, a)
    buf, m = _guarded_map(handle, hip_lib.voxel_params(float(aref.voxel), log2))
    ref = VR.Map(aref.voxel, log2)
    res = _merge(handle, m, ref, packed)
    assert res == {"n_offered": aref.n_voxels, "n_merged": aref.n_voxels, "n_skipped": 0, "n_claimed": aref.n_voxels}
    assert np.array_equal(ref.keys, aref.keys) and np.array_equal(ref.acc, aref.acc)
    _check(handle, m, ref)
    assert _pack(handle, m).tobytes() == packed.tobytes() and _extract(handle, m).tobytes() == _extract(handle, a).tobytes()
    if src == "small":
        assert ref.n_voxels == VR.load_limit(6)                                     # admitted exactly on the limit: no record more
        with pytest.raises(hip_lib.SvoError, match=CAPACITY):
            handle.voxel_merge([(_edev(packed[:1]), 0, 1.0)], [m])
    else:
        _reach(handle, m, ref)
    assert _guards_ok(buf)


def test_merge_into_a_map_that_holds_entries(handle):
    buf, m, ref = _fused(handle, EC.tiles(), log2=10)
    other = VR.Map(0.3, 10)
    rng = np.random.default_rng(53)
    rec = VR.records(VC._in_cell(rng.integers(-3, 5, (150, 3)), 0.3, rng), (90, 60, 30))
    other.fuse(rec, 7)
    spans = {"disjoint": EC.lattice_entries(50, first=40 * 40 * 20), "overlapping": ER.pack(other), "identical": ER.pack(ref)}
    have = set(ref.keys.tolist())
    assert not have & set(spans["disjoint"]["key"].tolist())
    assert have & set(spans["overlapping"]["key"].tolist()) and set(spans["overlapping"]["key"].tolist()) - have
    for name, ent in spans.items():
        n0 = ref.n_voxels
        res = _merge(handle, m, ref, ent)
        assert res["n_merged"] == len(ent) and res["n_claimed"] == ref.n_voxels - n0, name
        assert (res["n_claimed"] == len(ent)) == (name == "disjoint") and (res["n_claimed"] == 0) == (name == "identical")
        _check(handle, m, ref)
    _reach(handle, m, ref)
    assert _guards_ok(buf)


@pytest.mark.parametrize("n", EC.SPAN_SIZES)
def test_merge_spans_around_a_tile(handle, n):
    buf, m = _guarded_map(handle, hip_lib.voxel_params(0.3, 10))
    ref = VR.Map(0.3, 10)
    ent = EC.lattice_entries(n)
    for _ in range(2):                                                              # new keys, then the same keys found again
        res = _merge(handle, m, ref, ent)
        assert res["n_offered"] == n
    assert ref.n_voxels == n
    _check(handle, m, ref)
    if n:
        _reach(handle, m, ref)
    assert _guards_ok(buf)


def test_merge_a_key_that_repeats_across_lanes_wavefronts_and_workgroups(handle):
    ent = EC.dup_span()
    buf, m = _guarded_map(handle, hip_lib.voxel_params(0.3, 10))
    ref = VR.Map(0.3, 10)
    res = _merge(handle, m, ref, ent)
    assert res == {"n_offered": 257, "n_merged": 257, "n_skipped": 0, "n_claimed": 254}
    _check(handle, m, ref)
    # every record the same key: one entry, 257 adds
    one = ent.copy()
    one["key"] = ent[0]["key"]
    buf2, m2 = _guarded_map(handle, hip_lib.voxel_params(0.3, 10))
    ref2 = VR.Map(0.3, 10)
    assert _merge(handle, m2, ref2, one)["n_claimed"] == 1
    _check(handle, m2, ref2)
    _reach(handle, m, ref)
    assert _guards_ok(buf) and _guards_ok(buf2)


def test_merge_accumulators_that_wrap_and_last_as_a_max(handle):
    have, span = EC.wrap_pair()
    for first, second in ((have, span), (span, have)):
        buf, m = _guarded_map(handle, hip_lib.voxel_params(0.3, 6))
        ref = VR.Map(0.3, 6)
        _merge(handle, m, ref, first)
        _merge(handle, m, ref, second)
        got = {int(e["key"]): e["acc"].tolist() for e in _pack(handle, m)}
        k = [int(x) for x in span["key"]]
        assert got[k[0]] == [1, 0x10, 0, 1, 0, 0xFFFFFFFE, 0, 4] and got[k[1]][7] == 5 and got[k[2]][7] == 5 and got[k[3]][7] == 0
        info = handle.voxel_info(m)
        assert info["n_fused"] == ref.n_fused == 0xFFFFFFFF + 2 + 2 + 7 and info["n_voxels"] == 4      # a 64-bit sum of counts
        assert _pack(handle, m).tobytes() == ER.pack(ref).tobytes() == _raw_sorted(m).tobytes() and _guards_ok(buf)


def test_merge_skipped_records(handle):
    ent, which = EC.skipped_span()
    buf, m, ref = _fused(handle, EC.tiles())
    raw = buf.cpu().numpy().copy()
    res = _merge(handle, m, ref, ent[list(which)])
    assert res == {"n_offered": 3, "n_merged": 0, "n_skipped": 3, "n_claimed": 0}
    assert np.array_equal(buf.cpu().numpy(), raw)                                   # nothing but n_skipped
    res = _merge(handle, m, ref, ent)
    assert res == {"n_offered": 8, "n_merged": 5, "n_skipped": 3, "n_claimed": 5}
    _check(handle, m, ref)
    _reach(handle, m, ref)


def test_merge_three_spans_into_two_maps(handle):
    buf0, m0 = _guarded_map(handle, hip_lib.voxel_params(0.3, 10))
    buf1, m1 = _guarded_map(handle, hip_lib.voxel_params(1.0, 9))
    r0, r1 = VR.Map(0.3, 10), VR.Map(1.0, 9)
    a, b, c = EC.lattice_entries(300), EC.dup_span(), EC.lattice_entries(70, first=250)
    res = handle.voxel_merge([(_edev(a), 0, 0.3), (None, 1, 1.0), (_edev(b), 1, 1.0), (_edev(c), 0, 0.3)], [m0, m1])
    want0 = ER.merge(r0, a, 0.3)
    w = ER.merge(r0, c, 0.3)
    want0 = {k: want0[k] + w[k] for k in want0}
    assert res == [want0, ER.merge(r1, b, 1.0)] and want0["n_claimed"] == 320
    _check(handle, m0, r0)
    _check(handle, m1, r1)
    # no spans, and spans without records: nothing changes
    raw = (buf0.cpu().numpy().copy(), buf1.cpu().numpy().copy())
    assert handle.voxel_merge([], [m0, m1]) == [dict(n_offered=0, n_merged=0, n_skipped=0, n_claimed=0)] * 2
    assert handle.voxel_merge([(None, 0, 0.3), (None, 1, 1.0)], [m0, m1])[1]["n_offered"] == 0
    assert np.array_equal(buf0.cpu().numpy(), raw[0]) and np.array_equal(buf1.cpu().numpy(), raw[1])


def test_merge_load_bound_on_and_past_the_limit(handle):
    buf, m, ref = _fused(handle, EC.small(24))
    assert ref.n_voxels == 24
    more = EC.lattice_entries(25, first=3000)
    raw = buf.cpu().numpy().copy()
    with pytest.raises(hip_lib.SvoError, match=CAPACITY):                           # 24 + 25 > 48
        handle.voxel_merge([(_edev(more), 0, 1.0)], [m])
    with pytest.raises(hip_lib.SvoError, match=CAPACITY):                           # the records of all spans of the call count
        handle.voxel_merge([(_edev(more[:12]), 0, 1.0), (_edev(more[12:]), 0, 1.0)], [m])
    with pytest.raises(hip_lib.SvoError, match=CAPACITY):                           # on the bound: records, not new keys
        handle.voxel_merge([(_edev(np.repeat(more[:1], 25)), 0, 1.0)], [m])
    assert np.array_equal(buf.cpu().numpy(), raw)
    res, = handle.voxel_merge([(_edev(more[:12]), 0, 1.0), (_edev(more[12:24]), 0, 1.0)], [m])       # 24 + 24 == 48
    ER.merge(ref, more[:24], 1.0)
    assert res["n_claimed"] == 24 and ref.n_voxels == 48
    _check(handle, m, ref, (dict(),))
    assert _guards_ok(buf)


def test_merge_rejections(handle):
    buf, m, ref = _fused(handle, EC.tiles())
    buf2, m2 = _guarded_map(handle, hip_lib.voxel_params(0.3, 8))
    raw, raw2 = buf.cpu().numpy().copy(), buf2.cpu().numpy().copy()
    ent = _edev(EC.lattice_entries(20))
    voxel = np.float32(0.3)
    last_bit = float(np.nextafter(voxel, np.float32(1.0)))
    assert np.float32(last_bit).view(np.uint32) == voxel.view(np.uint32) + 1
    bad = [([(ent, 0, last_bit)], [m]),                                                              # the edge differs in its last bit
           ([(None, 0, last_bit)], [m]),                                                             # (of an empty span too)
           ([(ent, 0, 0.3), (ent, 1, 1.0)], [m, m2]),                                                # the second map's edge
           ([((ent.data_ptr() + 4, 19), 0, 0.3)], [m]),                                              # a misaligned address
           ([((0, 5), 0, 0.3)], [m]),                                                                # records and no address
           ([((ent.data_ptr(), -1), 0, 0.3)], [m]),
           ([(ent, 0, 0.3)], [m, m]),                                                                # a map named twice
           ([(ent, 1, 0.3)], [m]), ([(ent, -1, 0.3)], [m]),                                          # a span that names no map
           ([(ent, 0, 0.3)], [(m[0], hip_lib.voxel_params(0.3, 10))]),                               # not the params it was cleared with
           ([(ent, 0, 0.3)], [(m[0].data_ptr() + 8, m[1])])]
    for spans, maps in bad:
        with pytest.raises(hip_lib.SvoError, match=INVALID):
            handle.voxel_merge(spans, maps)
    assert np.array_equal(buf.cpu().numpy(), raw) and np.array_equal(buf2.cpu().numpy(), raw2)
    assert (ent.data_ptr() + 40) % 16 == 8
    res, = handle.voxel_merge([((ent.data_ptr() + 40, 19), 0, 0.3)], [m])                            # 8-byte aligned is enough: records 1 .. 19
    assert res == ER.merge(ref, EC.lattice_entries(20)[1:], 0.3) and res["n_merged"] == 19
    _check(handle, m, ref)


# ---------------------------------------------------------------------------------------------------------- equivalence

@pytest.mark.parametrize("lane_atomics", [0, 1])
def test_fusing_the_union_is_merging_the_maps(handle, monkeypatch, lane_atomics):
    monkeypatch.setenv("SVO_VOXEL_LANE_ATOMICS", str(lane_atomics))
    r1, r2, params = EC.union()
    p = hip_lib.voxel_params(*params)
    whole, m1, m2 = handle.voxel_new(p), handle.voxel_new(p), handle.voxel_new(p)
    handle.voxel_fuse([(_dev(np.concatenate([r1, r2])), 0, 3)], [whole])
    handle.voxel_fuse([(_dev(r1), 0, 3), (_dev(r2), 1, 3)], [m1, m2])
    n2 = handle.voxel_info(m2)["n_voxels"]
    res, = handle.voxel_merge([(handle.voxel_pack(m1)[0], 0, params[0])], [m2])
    ref = VR.Map(*params)
    ref.fuse(np.concatenate([r1, r2]), 3)
    assert res["n_claimed"] == ref.n_voxels - n2 and res["n_skipped"] == 0
    for kw in FILTERS:
        assert _extract(handle, m2, **kw).tobytes() == _extract(handle, whole, **kw).tobytes() == ref.extract(**kw).tobytes()
        assert _pack(handle, m2, **kw).tobytes() == _pack(handle, whole, **kw).tobytes() == ER.pack(ref, **kw).tobytes()
    a, b = handle.voxel_info(m2), handle.voxel_info(whole)
    assert (a["n_voxels"], a["n_fused"], a["overflow"]) == (b["n_voxels"], b["n_fused"], 0)


# ---------------------------------------------------------------------------------------------------------- rehash

def _with_an_outside_record(case):
    """the case with one record outside the key range fused first: n_outside = 1"""
    out = dict(case)
    out["calls"] = [[(VR.records([[3e38, 0.0, 0.0]]), 0, 1)]] + list(case["calls"])
    return out


def test_rehash_up_and_down_with_the_chain_that_wraps(handle):
    buf, m, ref = _fused(handle, _with_an_outside_record(EC.small(48)))
    assert (ref.n_voxels, ref.n_outside, ref.n_fused) == (48, 1, 48)
    before = _pack(handle, m)
    raw = buf.cpu().numpy().copy()
    up = handle.voxel_rehash(m, 10)                                                 # 6 -> 10
    assert up[1].log2_capacity == 10 and up[0].numel() == hip_lib.voxel_map_bytes(10) and np.array_equal(buf.cpu().numpy(), raw)
    ref_up = ER.rehash(ref, 10)
    _check(handle, up, ref_up, (dict(), dict(min_stamp=2)))
    assert _pack(handle, up).tobytes() == before.tobytes()
    assert len({VR.home(k, 10) for k in VC.chain_keys()}) > 1                       # the chain fell apart under the larger table
    down = handle.voxel_rehash(up, 6)                                               # 10 -> 6, exactly on the limit
    _check(handle, down, ER.rehash(ref_up, 6), (dict(), dict(min_stamp=2)))
    keys, _ = _raw(down)
    assert keys[63] != np.uint64(VR.EMPTY) and keys[0] != np.uint64(VR.EMPTY) and _pack(handle, down).tobytes() == before.tobytes()
    info = handle.voxel_info(down)
    assert (info["n_voxels"], info["n_fused"], info["n_outside"], info["overflow"], info["log2_capacity"]) == (48, 48, 1, 0, 6)
    _reach(handle, up, ref_up)
    # one entry more: refused, and dst untouched
    ref_up = ER.rehash(ref, 10)
    up = handle.voxel_rehash(m, 10)
    _merge(handle, up, ref_up, EC.lattice_entries(1, first=9000), 1.0)
    assert ref_up.n_voxels == 49 and ER.rehash(ref_up, 6) is None
    gbuf, dst = _guarded(hip_lib.voxel_map_bytes(7))
    rc = hip_lib.lib().svo_voxel_rehash(handle._h, Cp.byref(hip_lib._voxel_map(up)), Cp.c_void_p(dst.data_ptr()), 6)
    assert rc == -4 and (gbuf.cpu().numpy() == 0xA5).all()
    rc = hip_lib.lib().svo_voxel_rehash(handle._h, Cp.byref(hip_lib._voxel_map(up)), Cp.c_void_p(dst.data_ptr()), 7)
    assert rc == 0 and _guards_ok(gbuf)                                             # a dst that was never cleared is cleared by the call
    down7 = (dst, hip_lib.voxel_params(1.0, 7))
    _check(handle, down7, ER.rehash(ref_up, 7), (dict(),))


def test_rehash_of_two_tiles_and_a_fuse_that_follows(handle):
    _, m, ref = _fused(handle, EC.tiles())
    before = _pack(handle, m)
    for log2 in (8, 10, 12):                                                        # 8: shrinking where it fits
        out = handle.voxel_rehash(m, log2)
        rref = ER.rehash(ref, log2)
        assert rref is not None
        _check(handle, out, rref)
        assert _pack(handle, out).tobytes() == before.tobytes()
        more = VC.mixed(40, seed=24)[0][:VR.load_limit(log2) - rref.n_voxels]       # (what the load bound admits)
        assert len(more) >= 10
        handle.voxel_fuse([(_dev(more), 0, 8)], [out])                              # a fuse that follows finds every entry
        rref.fuse(more, 8)
        _check(handle, out, rref)
    empty = handle.voxel_new(hip_lib.voxel_params(0.3, 9, 2))
    out = handle.voxel_rehash(empty, 6)
    assert handle.voxel_info(out) == dict(handle.voxel_info(empty), log2_capacity=6) and out[1].drop_flags == 2
    assert np.array_equal(out[0].cpu().numpy(), handle.voxel_new(hip_lib.voxel_params(0.3, 6, 2))[0].cpu().numpy())


def test_rehash_rejections(handle):
    buf, m, ref = _fused(handle, EC.tiles())
    raw = buf.cpu().numpy().copy()
    gbuf, dst = _guarded(hip_lib.voxel_map_bytes(10) + 16)
    lib, vm = hip_lib.lib(), hip_lib._voxel_map(m)

    def call(map_, dst_ptr, log2):
        return lib.svo_voxel_rehash(handle._h, Cp.byref(map_) if map_ is not None else None, Cp.c_void_p(dst_ptr), log2)

    assert call(vm, vm.data, 9) == -1 and call(vm, vm.data, 10) == -1               # dst == src->data
    assert call(vm, vm.data + 16, 10) == -1                                         # dst inside src
    assert call(vm, dst.data_ptr() + 8, 10) == -1 and call(vm, None, 10) == -1      # misaligned, NULL
    assert call(vm, dst.data_ptr(), 5) == -1 and call(vm, dst.data_ptr(), 27) == -1 and call(None, dst.data_ptr(), 10) == -1
    assert call(vm, dst.data_ptr(), 7) == -4 and ref.n_voxels > VR.load_limit(7)    # the admission rule
    for other in (hip_lib.voxel_params(0.25, 9), hip_lib.voxel_params(0.3, 8), hip_lib.voxel_params(0.3, 9, 4)):
        assert call(hip_lib._voxel_map((m[0], other)), dst.data_ptr(), 10) == -1    # not the params it was cleared with
    assert (gbuf.cpu().numpy() == 0xA5).all() and np.array_equal(buf.cpu().numpy(), raw)
    assert call(vm, dst.data_ptr() + 16, 10) == 0 and _guards_ok(gbuf)              # 16-byte aligned is enough
