"""A handle that is used again: the grow-only workspaces of the table entries (svo_capi_tables.hip) and the device
ring of the argument blocks (svo_handle.hpp). Every entry is called small, then large, then small on ONE Handle, and
every call's output must equal, bit for bit, the same call on a Handle made for it; the ring is driven round more
than once. No reference but the library itself: the other GPU files hold each entry to its statement."""
import numpy as np
import pytest
import torch

import rigcal_ref as RC
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.hip_lib import CameraCalibration, Handle

pytestmark = pytest.mark.gpu

FILL = 0xA5
KP_PLANES = ("flags", "keyframe_id", "keypoint_index", "outlier_count", "inlier_count", "kf_inv_depth", "kf_variance",
             "score", "level_type", "color")
EXPORT_TILE = MAP_TILE = 256                     # keypoints a tile (svo_tracker.hpp)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(*tensors):
    torch.cuda.synchronize()
    return b"".join(t.cpu().numpy().tobytes() for t in tensors)


def _reused_equals_fresh(run, calls):
    """run(handle, call) -> bytes: every call of the sequence on one Handle equals that call on a Handle of its own"""
    reused = Handle(0, 64)
    for i, call in enumerate(calls):
        got = run(reused, call)
        fresh = Handle(0, 64)
        want = run(fresh, call)
        fresh.close()
        assert got == want, f"call {i} of {len(calls)} differs on the reused handle"
    reused.close()


def _kp_set(rng, n, names):
    """(n, {plane: device tensor}) of random 32-bit patterns; kps3d inside the unit cube so that a scene shows them"""
    fields = {}
    for name in names:
        if name == "kps2d":
            fields[name] = _dev(rng.uniform((-4, -4), (74, 24), (n, 2)).astype(np.float32))
        elif name == "kps3d":
            fields[name] = _dev(rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32))
        elif name == "level_type":
            fields[name] = _dev((rng.integers(0, 2, n) << 8 | rng.integers(0, 4, n)).astype(np.int32))
        elif name == "flags":
            fields[name] = _dev(rng.integers(0, 8, n).astype(np.uint32))
        else:
            fields[name] = _dev(rng.integers(0, 2**31, n).astype(np.uint32))
    return n, fields


# ---------------------------------------------------------------------------------- the workspaces

def test_remap_workspace_small_large_small():
    """svo_remap_linear: 1 image through a 40 x 24 map, 5 through an 80 x 48 map (the map part and the image table
    grow), 1 again; then svo_remap_linear_multi, which shares the workspace (2 maps, 3 images), and the first again"""
    rng = np.random.default_rng(1)
    src = [_dev(rng.integers(0, 256, (24, 40), dtype=np.uint8)) for _ in range(5)]

    def maps(w, h):
        return _dev(rng.uniform(-2, 42, (h, w)).astype(np.float32)), _dev(rng.uniform(-2, 26, (h, w)).astype(np.float32))
    small, large, other = maps(40, 24), maps(80, 48), maps(40, 24)
    calls = [("one", src[:1], small), ("one", src, large), ("one", src[:1], small),
             ("multi", src[:3], (small, other), (1, 0, 1)), ("one", src[1:2], small)]

    def run(h, call):
        if call[0] == "one":
            return _bytes(*h.remap_linear(call[1], *call[2]))
        return _bytes(*h.remap_linear_multi(call[1], [m[0] for m in call[2]], [m[1] for m in call[2]], call[3]))
    _reused_equals_fresh(run, calls)


def test_rectify_maps_workspace_small_large_small():
    """svo_build_rectify_maps: 1, 3, 1 cameras of 40 x 24 from the EuRoC calibration"""
    e = RC.euroc()[0]
    left, right = (CameraCalibration.from_mats(*e[side]) for side in ("LEFT", "RIGHT"))

    def run(h, cals):
        out = [tuple(torch.full((24, 40), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)) for _ in cals]
        h.build_rectify_maps(cals, 40, 24, out=out)
        return _bytes(*[m for pair in out for m in pair])
    _reused_equals_fresh(run, [[left], [left, right, left], [right]])


def test_convert_frames_workspace_small_large_small():
    """svo_convert_frames: 1, 4, 1 side-by-side gray frames of 32 x 16"""
    rng = np.random.default_rng(2)
    frames = [_dev(rng.integers(0, 256, (16, 64), dtype=np.uint8)) for _ in range(4)]
    fmt = hip_lib.INPUT_FORMATS.index("sbs_gray")

    def run(h, srcs):
        lefts, rights = h.convert_frames(fmt, srcs, None, 32)
        return _bytes(*lefts, *rights)
    _reused_equals_fresh(run, [frames[:1], frames, frames[3:]])


def test_pack_keypoints_workspace_small_large_small():
    """svo_pack_keypoints: one set below a tile, sets of several tiles each, one set again"""
    rng = np.random.default_rng(3)
    names = ("kps2d", "kps3d") + KP_PLANES
    calls = [[_kp_set(rng, 5, names)],
             [_kp_set(rng, n, names) for n in (EXPORT_TILE + 44, 2 * EXPORT_TILE + 188, 3)],
             [_kp_set(rng, 1, names)]]

    def run(h, sets):
        first = np.cumsum([0] + [n for n, _ in sets])
        outs = [torch.full((int(first[-1]) + 2, w), FILL, dtype=torch.uint8, device="cuda") for w in (8, 12, 44)]
        h.pack_keypoints(sets, first[:-1], *outs)
        return _bytes(*outs)
    _reused_equals_fresh(run, calls)


MAP_NAMES = ("kps3d", "flags", "keyframe_id", "inlier_count", "color")


def _regions(rng, counts):
    """a region per count: one set of so many keypoints whose own keyframe is the region's index"""
    return [[(n, r, _kp_set(rng, n, MAP_NAMES)[1])] for r, n in enumerate(counts)]


@pytest.mark.parametrize("table_tiles", [None, "2"])
def test_pack_map_points_workspace_small_large_small(monkeypatch, table_tiles):
    """svo_pack_map_points: 1 region, 3 regions of two tiles each, 1 region; then with a table of two tiles, so that
    the chunked launches run on a block that grew"""
    if table_tiles:
        monkeypatch.setenv("SVO_MAP_TABLE_TILES", table_tiles)
    rng = np.random.default_rng(4)
    calls = [_regions(rng, (3,)), _regions(rng, (MAP_TILE + 44, MAP_TILE + 1, 2 * MAP_TILE)), _regions(rng, (65,))]

    def run(h, regions):
        first = np.cumsum([0] + [r[0][0] for r in regions])
        points = torch.full((int(first[-1]) + 2, 16), FILL, dtype=torch.uint8, device="cuda")
        counts = torch.full((len(regions) + 1,), -7, dtype=torch.int32, device="cuda")
        h.pack_map_points(regions, first[:-1], None, points, counts)
        return _bytes(points, counts)
    _reused_equals_fresh(run, calls)


@pytest.mark.parametrize("table_tiles", [None, "2"])
def test_render_views_workspace_small_large_small(monkeypatch, table_tiles):
    """svo_render_views: 1, 3, 1 images of 70 x 20 (2 x 2 tiles each) as RGB with markers"""
    if table_tiles:
        monkeypatch.setenv("SVO_VIEW_TABLE_TILES", table_tiles)
    rng = np.random.default_rng(5)
    w, hgt = 70, 20
    images = [((_dev(rng.integers(0, 256, (hgt, w), dtype=np.uint8)), w, hgt, w),
               _kp_set(rng, 6, ("kps2d", "flags", "level_type", "color"))) for _ in range(3)]
    style = hip_lib.view_style(pixel="rgb8", markers=True, drop_flags=0, size=6, size_temporary=4)

    def run(h, srcs):
        pixels = torch.full((len(srcs) * w * hgt * 3 + 8,), FILL, dtype=torch.uint8, device="cuda")
        h.render_views(srcs, [i * w * hgt * 3 for i in range(len(srcs))], style, pixels)
        return _bytes(pixels)
    _reused_equals_fresh(run, [images[:1], images, images[2:]])


@pytest.mark.parametrize("table_tiles", [None, "2"])
def test_render_scene_workspace_small_large_small(monkeypatch, table_tiles):
    """svo_render_scene: 1, 3, 1 images of 70 x 20 (2 x 2 tiles each) of two point sets, from the front"""
    if table_tiles:
        monkeypatch.setenv("SVO_SCENE_TABLE_TILES", table_tiles)
    rng = np.random.default_rng(6)
    cols, rows = 70, 20
    images = [(cols, rows, [(n, j, _kp_set(rng, n, MAP_NAMES)[1]) for j, n in enumerate((40, 9))], None) for _ in range(3)]
    style = hip_lib.scene_style(cols, rows, pixel="rgb8")
    camera = hip_lib.scene_preset("front", cols, rows)
    image_bytes = hip_lib.scene_size(style)[1]
    assert image_bytes % 4 == 0

    def run(h, srcs):
        pixels = torch.full((len(srcs) * image_bytes + 8,), FILL, dtype=torch.uint8, device="cuda")
        h.render_scene(srcs, [camera] * len(srcs), [i * image_bytes for i in range(len(srcs))], style, pixels)
        return _bytes(pixels)
    _reused_equals_fresh(run, [images[:1], images, images[2:]])


def test_copy_segments_workspace_small_large_small():
    """svo_copy_segments: 1 segment of 64 bytes, 300 segments, 1"""
    src = _dev(np.random.default_rng(7).integers(0, 256, 300 * 64, dtype=np.uint8))

    def run(h, which):
        dst = torch.full((300 * 64,), FILL, dtype=torch.uint8, device="cuda")
        h.copy_segments([(src.data_ptr() + 64 * i, dst.data_ptr() + 64 * i, 64, 1, 64, 64) for i in which])
        return _bytes(dst)
    _reused_equals_fresh(run, [[7], range(300), [299]])


# ---------------------------------------------------------------------------------- the ring

def test_argument_ring_wraps():
    """every staging entry takes at least two 256-byte blocks of the 1 MiB ring a call (4 096 blocks), so 2 100 calls
    of svo_ssd_disparity go round it at least once: every 100th result and the last equal the first"""
    rng = np.random.default_rng(8)
    left = rng.integers(0, 256, (16, 32), dtype=np.uint8)
    right = np.roll(left, -3, axis=1)
    kps = np.stack([rng.uniform(14, 26, 8), rng.uniform(5, 10, 8)], 1).astype(np.float32)
    left, right, kps = _dev(left), _dev(right), _dev(kps)
    h = Handle(0, 64)
    first = None
    for i in range(2100):
        out = h.ssd_disparity(left, right, kps, 5, 8, 1)
        if i % 100 == 0 or i == 2099:
            got = _bytes(out)
            first = got if first is None else first
            assert got == first, f"call {i} differs from the first"
    h.close()
