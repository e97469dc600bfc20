"""svo_voxel_prune on the GPU against tests/voxel_prune_ref.py, byte for byte: every crafted case of
tests/voxel_prune_cases.py (the extraction, the header's counters, the result), the raw bytes of the map and the guard
words around it across a prune that removes nothing, chain reachability (a record per kept key fused afterwards
claims no entry), fusing on after a prune in both forms of the fuse kernel, the full map pruned and refilled to its
load limit, a prune that keeps nothing against a cleared map, and every rejection with nothing written."""
import copy

import numpy as np
import pytest
import torch

import voxel_cases as VC
import voxel_prune_cases as PC
import voxel_prune_ref as PR
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib

pytestmark = pytest.mark.gpu
GUARD = 256                      # bytes of 0xA5 before and after a map
FILTERS = (dict(), dict(min_count=2), dict(min_stamp=2), dict(min_count=3, min_stamp=2))


@pytest.fixture(scope="module")
def handle():
    return hip_lib.Handle(0, 1024)


def _dev(rec):
    buf = np.zeros(len(rec) + 1, VR.POINT)
    buf[:len(rec)] = rec
    return torch.from_numpy(buf.view(np.uint8).reshape(-1, 16)).cuda()[:len(rec)]


def _guarded_map(h, params):
    """a cleared map between two guards: (whole buffer, (map tensor, params))"""
    n = hip_lib.voxel_map_bytes(params.log2_capacity)
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    m = (buf[GUARD:GUARD + n], params)
    h.voxel_clear(m)
    return buf, m


def _guards_ok(buf):
    raw = buf.cpu().numpy()
    return bool((raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all())


def _fused(h, case):
    buf, m = _guarded_map(h, hip_lib.voxel_params(*case["maps"][0]))
    for call in case["calls"]:
        h.voxel_fuse([(_dev(r), mi, s) for r, mi, s in call], [m])
    return buf, m


def _keep(case):
    return hip_lib.voxel_keep(**case["keep"])


def _extract(h, m, **kw):
    pts, n = h.voxel_extract(m, **kw)
    return pts.cpu().numpy()[:n].copy().view(VR.POINT).reshape(-1)


def _check_against(h, m, ref):
    info = h.voxel_info(m)
    assert (info["n_voxels"], info["n_fused"], info["n_outside"], info["overflow"]) == (ref.n_voxels, ref.n_fused, ref.n_outside, 0)
    for kw in FILTERS:
        want = ref.extract(**kw)
        got = _extract(h, m, **kw)
        assert len(got) == len(want) and got.tobytes() == want.tobytes(), kw


@pytest.fixture(scope="module")
def refs():
    """the statement's map of every case before its prune, computed once and never changed"""
    return {name: VR.run(PC.case(name))[0] for name in PC.NAMES}


@pytest.mark.parametrize("name", PC.NAMES)
def test_cases(handle, refs, name):
    case = PC.case(name)
    before = refs[name]
    buf, m = _fused(handle, case)
    _check_against(handle, m, before)
    # "F and K" on the untouched map, by the statement
    both = {i: PR.extract_both(before, case["keep"], **f) for i, f in enumerate(FILTERS)}
    ref = PR.pruned(before, **case["keep"])
    raw_before = buf.cpu().numpy().copy()
    res = handle.voxel_prune(m, _keep(case))
    cv = PR.center_voxel(case["keep"]["center"], before.voxel) if case["keep"].get("radius", -1) >= 0 else (0, 0, 0)
    assert res == {"n_before": before.n_voxels, "n_kept": ref.n_voxels, "center_voxel": cv}
    _check_against(handle, m, ref)
    for i, f in enumerate(FILTERS):
        assert _extract(handle, m, **f).tobytes() == both[i].tobytes()
    raw_once = buf.cpu().numpy().copy()
    assert _guards_ok(buf)
    if ref.n_voxels == before.n_voxels:
        assert np.array_equal(raw_once, raw_before)                  # nothing left: no byte of the map was written
    # again: the same rule removes nothing now, so it writes nothing
    res = handle.voxel_prune(m, _keep(case))
    assert (res["n_before"], res["n_kept"]) == (ref.n_voxels, ref.n_voxels)
    assert np.array_equal(buf.cpu().numpy(), raw_once)
    # every kept entry is reachable from its home: a record per kept key finds its entry and claims none
    if ref.n_voxels:
        assert ref.admits(ref.n_voxels)
        rec = PC.records_of_keys(ref.keys, ref.voxel)
        handle.voxel_fuse([(_dev(rec), 0, 9)], [m])
        assert handle.voxel_info(m)["n_voxels"] == ref.n_voxels
        after = copy.deepcopy(ref)
        after.fuse(rec, 9)
        _check_against(handle, m, after)
    assert _guards_ok(buf)


def test_keep_none_leaves_a_cleared_map_but_for_the_counters(handle, refs):
    case = PC.case("keep_none")
    buf, m = _fused(handle, case)
    handle.voxel_prune(m, _keep(case))
    raw = m[0].cpu().numpy().copy()
    fresh = handle.voxel_new(m[1])[0].cpu().numpy()
    counters = raw[24:48].view("<u8")                                 # n_fused, n_outside, overflow (svo_voxel_map_info's order)
    assert counters.tolist() == [refs["keep_none"].n_fused, refs["keep_none"].n_outside, 0] and counters[0] > 0
    raw[24:48] = 0
    assert np.array_equal(raw, fresh)


@pytest.mark.parametrize("lane_atomics", [0, 1])
def test_fusing_on_after_a_prune(handle, monkeypatch, lane_atomics):
    monkeypatch.setenv("SVO_VOXEL_LANE_ATOMICS", str(lane_atomics))
    # voxel_cases.chain: 40 keys of one home in 64 entries; a box keeps some of them, then the case's second call
    chain = VC.case("chain")
    ix = sorted(VR.key_parts(k)[0] - VR.BIAS for k in VC.chain_keys())
    mid = ix[len(ix) // 2]
    jobs = [(chain, dict(center=(mid + 0.5, 0.5, 0.5), radius=(ix[-1] - ix[0]) // 4))]
    # voxel_cases.spans, its map 1 (log2_capacity 10) and its map 2 (12): prune between two rounds of the same spans
    spans = VC.case("spans")
    for mi, keep in ((1, dict(min_count=2)), (2, dict(center=(0.5, 0.5, 0.5), radius=3))):
        call = [(r, 0, s) for r, m_, s in spans["calls"][0] if m_ == mi and len(r)]
        jobs.append(({"maps": [spans["maps"][mi]], "calls": [call, call]}, keep))
    rec, params = VC.mixed()
    jobs.append(({"maps": [params], "calls": [[(rec[:1500], 0, 1)], [(rec[1500:], 0, 2)]]}, dict(PC.case("mixed")["keep"], min_stamp=1)))
    for case, keep in jobs:
        ref = VR.Map(*case["maps"][0])
        buf, m = _guarded_map(handle, hip_lib.voxel_params(*case["maps"][0]))
        first, second = case["calls"]
        for r, _, s in first:
            ref.fuse(r, s)
            handle.voxel_fuse([(_dev(r), 0, s)], [m])
        n_before, n_kept = PR.prune(ref, **keep)
        assert 0 < n_kept < n_before
        res = handle.voxel_prune(m, hip_lib.voxel_keep(**keep))
        assert (res["n_before"], res["n_kept"]) == (n_before, n_kept)
        for r, _, s in second:
            assert ref.admits(len(r))
            ref.fuse(r, s + 10)
            handle.voxel_fuse([(_dev(r), 0, s + 10)], [m])
        _check_against(handle, m, ref)
        assert _guards_ok(buf)


def test_the_full_map_pruned_and_refilled(handle, refs):
    case = PC.case("full")
    buf, m = _fused(handle, case)
    one = _dev(VR.records(VC._in_cell([(50, 50, 50)], 0.3, np.random.default_rng(1))))
    with pytest.raises(hip_lib.SvoError, match="error -4:"):
        handle.voxel_fuse([(one, 0, 3)], [m])                                               # at the load limit: not one record more
    ref = PR.pruned(refs["full"], **case["keep"])
    assert handle.voxel_prune(m, _keep(case))["n_kept"] == ref.n_voxels == 24
    refill = VR.records(VC._in_cell(PC.full_cells()[48:72], 0.3, np.random.default_rng(2)), (9, 9, 9))
    handle.voxel_fuse([(_dev(refill), 0, 3)], [m])                                          # the load bound uses the new n_voxels
    ref.fuse(refill, 3)
    assert ref.n_voxels == 48
    _check_against(handle, m, ref)
    raw = buf.cpu().numpy().copy()
    with pytest.raises(hip_lib.SvoError, match="error -4:"):
        handle.voxel_fuse([(one, 0, 4)], [m])
    assert np.array_equal(buf.cpu().numpy(), raw)


def test_rejections(handle):
    case = PC.case("box")
    buf, m = _fused(handle, case)
    raw = buf.cpu().numpy().copy()
    data, params = m
    lib = hip_lib.lib()
    vm = hip_lib._voxel_map(m)
    out = hip_lib.VoxelPruneResult(-1, -1)
    assert lib.svo_voxel_prune(handle._h, hip_lib.C.byref(vm), None, hip_lib.C.byref(out)) == -1          # no keep rule
    assert lib.svo_voxel_prune(handle._h, None, hip_lib.C.byref(_keep(case)), hip_lib.C.byref(out)) == -1   # no map
    for i in (0, 1):
        k = _keep(case)
        k._reserved[i] = 1
        with pytest.raises(hip_lib.SvoError, match="error -1:"):
            handle.voxel_prune(m, k)
    for bad in (float("nan"), float("inf"), float("-inf"), 3e38, 1048576.0, -1048575.5):
        for axis in range(3):
            c = [0.5, 0.5, 0.5]
            c[axis] = bad
            with pytest.raises(hip_lib.SvoError, match="error -1:"):
                handle.voxel_prune(m, hip_lib.voxel_keep(center=c, radius=1))
    for other in (hip_lib.voxel_params(0.25, 8), hip_lib.voxel_params(1.0, 7), hip_lib.voxel_params(1.0, 8, 2)):
        with pytest.raises(hip_lib.SvoError, match="error -1:"):                                            # cleared with other params
            handle.voxel_prune((data, other), _keep(case))
    for bad in (hip_lib.voxel_params(0.0, 8), hip_lib.voxel_params(float("nan"), 8), hip_lib.voxel_params(1.0, 5), hip_lib.voxel_params(1.0, 27),
                hip_lib.voxel_params(1.0, 8, 8)):
        with pytest.raises(hip_lib.SvoError, match="error -1:"):
            handle.voxel_prune((data, bad), _keep(case))
    with pytest.raises(hip_lib.SvoError, match="error -1:"):
        handle.voxel_prune((data.data_ptr() + 8, params), _keep(case))                                      # a misaligned map
    never = torch.zeros(hip_lib.voxel_map_bytes(8), dtype=torch.uint8, device="cuda")
    with pytest.raises(hip_lib.SvoError, match="error -1:"):
        handle.voxel_prune((never, params), _keep(case))
    assert not never.cpu().numpy().any()
    assert (out.n_before, out.n_kept) == (-1, -1) and np.array_equal(buf.cpu().numpy(), raw)
    # without a box the centre is not read
    res = handle.voxel_prune(m, hip_lib.voxel_keep(center=(float("nan"), float("inf"), 3e38), radius=-5))
    assert res["n_kept"] == res["n_before"] > 0 and res["center_voxel"] == (0, 0, 0) and np.array_equal(buf.cpu().numpy(), raw)
