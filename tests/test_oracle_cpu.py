"""CPU tests (no GPU): the oracle against the reference's own known answers,
against independent numpy/scipy formulations of the OpenCV primitives it
restates, and against the committed golden vectors (tests/golden/)."""
import os
import zlib

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial.transform import Rotation

import oracle_py as O
from stereo_svo_slam_amd import synth
import util
import window_cases


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


# ------------------------------------------------ the reference's known answer
def test_exponential_map_known_answer():
    """src/test/test_exponential_map.cpp:35-48: twist (0.1,0.2,0.3 | 0.4,0.5,0.6).
    The shipped header (src/include/exponential_map.hpp:14-35) writes the mapped
    translation into rows 0..2 and keeps w in rows 3..5."""
    out = O.exponential_map([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    expect = [0.12187591059875308, 0.173369312443241, 0.30760829923146377]
    assert np.all(np.abs(out[:3] - expect) < 0.01)          # the reference's tolerance
    assert np.all(np.abs(out[:3] - expect) < 1e-6)          # and float accuracy
    assert np.array_equal(out[3:], np.float32([0.4, 0.5, 0.6]))


def test_exponential_map_closed_form():
    """src/test/exponential_map_test.py: (I + (1-cos1) K + (1-sin1) K^2) v."""
    rng = np.random.RandomState(0)
    for _ in range(20):
        t = rng.normal(0, 0.3, 6)
        w = t[3:]
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        v = (np.eye(3) + (1 - np.cos(1.0)) * K + (1 - np.sin(1.0)) * K @ K) @ t[:3]
        out = O.exponential_map(t)
        assert np.allclose(out[:3], v, atol=1e-6)


# ------------------------------------------------------ restated OpenCV pieces
def test_rodrigues_matches_scipy():
    rng = np.random.RandomState(1)
    for _ in range(50):
        r = rng.normal(0, 0.5, 3).astype(np.float32)
        R = O.rodrigues(r)
        assert np.allclose(R, Rotation.from_rotvec(r.astype(np.float64)).as_matrix(), atol=1e-12)
    assert np.array_equal(O.rodrigues([0, 0, 0]), np.eye(3))


def test_inv_svd_is_the_inverse_and_zero_for_zero():
    rng = np.random.RandomState(2)
    for _ in range(20):
        J = rng.normal(0, 1, (40, 6))
        H = (J.T @ J).astype(np.float32)
        Hi, ok = O.inv_svd(H)
        assert ok
        assert np.allclose(Hi @ H.astype(np.float64), np.eye(6), atol=5e-3)
    Hi, ok = O.inv_svd(np.zeros((6, 6), np.float32))
    assert not ok and np.all(Hi == 0)


def test_solve_svd_least_squares():
    rng = np.random.RandomState(3)
    for _ in range(20):
        A = rng.normal(0, 1, (3, 2)).astype(np.float32)
        b = rng.normal(0, 1, 3).astype(np.float32)
        x = O.solve_svd(A, b)
        ref = np.linalg.lstsq(A.astype(np.float64), b.astype(np.float64), rcond=None)[0]
        assert np.allclose(x, ref, atol=1e-4)


def test_project_keypoints_formula():
    cfg = dict(synth.CONFIGS["econ"])           # non-zero distortion
    cam = util.oracle_camera(cfg)
    rng = np.random.RandomState(4)
    P = np.stack([rng.uniform(-1, 1, 50), rng.uniform(-1, 1, 50), rng.uniform(2, 6, 50)], 1).astype(np.float32)
    pose = np.float32([0.1, -0.05, 0.2, 0.02, -0.03, 0.01])
    out = O.project_keypoints(pose, P, cam)
    R = Rotation.from_rotvec(-pose[3:].astype(np.float64)).as_matrix()
    X = (R @ (P - pose[:3]).astype(np.float64).T).T
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    c = 1 + cfg["k1"] * r2 + cfg["k2"] * r2 ** 2 + cfg["k3"] * r2 ** 3
    xd = x * c + 2 * cfg["p1"] * x * y + cfg["p2"] * (r2 + 2 * x * x)
    yd = y * c + cfg["p1"] * (r2 + 2 * y * y) + 2 * cfg["p2"] * x * y
    ref = np.stack([cfg["fx"] * xd + cfg["cx"], cfg["fy"] * yd + cfg["cy"]], 1)
    assert np.allclose(out, ref, atol=2e-4)


@pytest.mark.parametrize("shape", [(48, 64), (37, 53), (5, 7)])
def test_halfsample_pyramid(shape):
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    lv = O.build_pyramid(img, 3)
    a = img.astype(np.int32)
    for l in (1, 2):
        h, w = a.shape[0] // 2, a.shape[1] // 2
        a = (a[0:2 * h:2, 0:2 * w:2] + a[0:2 * h:2, 1:2 * w:2] + a[1:2 * h:2, 0:2 * w:2] + a[1:2 * h:2, 1:2 * w:2]) // 4
        assert np.array_equal(lv[l], a.astype(np.uint8))


@pytest.mark.parametrize("shape", [(48, 64), (37, 53), (9, 11)])
def test_pyr_down_vs_scipy(shape):
    """cv::pyrDown: 5x5 binomial, reflect-101 ('mirror'), round half up, take even samples."""
    rng = np.random.RandomState(6)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    f = ndimage.correlate1d(img.astype(np.int64), k, axis=0, mode="mirror")
    f = ndimage.correlate1d(f, k, axis=1, mode="mirror")
    ref = ((f + 128) >> 8)[::2, ::2].astype(np.uint8)
    assert np.array_equal(O.pyr_down(img), ref)


def test_scharr_vs_scipy():
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (40, 56)).astype(np.uint8).astype(np.int64)
    sm, df = np.array([3, 10, 3]), np.array([-1, 0, 1])
    dx = ndimage.correlate1d(ndimage.correlate1d(img, sm, axis=0, mode="mirror"), df, axis=1, mode="mirror")
    dy = ndimage.correlate1d(ndimage.correlate1d(img, df, axis=0, mode="mirror"), sm, axis=1, mode="mirror")
    out = O.scharr(img.astype(np.uint8))
    assert np.array_equal(out[..., 0], dx) and np.array_equal(out[..., 1], dy)


def test_sobel_and_fast_brute_force():
    rng = np.random.RandomState(8)
    img = (ndimage.gaussian_filter(rng.uniform(0, 255, (60, 80)), 1.5) * 2 % 256).astype(np.uint8)
    a = img.astype(np.int64)
    k = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    ref = np.clip(ndimage.correlate(a, k, mode="mirror"), 0, 255).astype(np.uint8)
    assert np.array_equal(O.sobel_x_u8(img), ref)
    # FAST-9/16: brute-force arc test + score = max_t such that still a corner
    ring = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3),
            (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

    def is_corner(y, x, t):
        d = [int(img[y, x]) - int(img[y + dy, x + dx]) for dx, dy in ring]
        for s in range(16):
            arc = [d[(s + i) % 16] for i in range(9)]
            if all(v > t for v in arc) or all(v < -t for v in arc):
                return True
        return False

    raw = np.zeros(img.shape, np.int32)
    for y in range(3, img.shape[0] - 3):
        for x in range(3, img.shape[1] - 3):
            if is_corner(y, x, 6):
                t = 6
                while is_corner(y, x, t + 1):
                    t += 1
                raw[y, x] = t
    ref = np.zeros(img.shape, np.uint8)
    for y in range(3, img.shape[0] - 3):
        for x in range(3, img.shape[1] - 3):
            s = raw[y, x]
            nb = raw[y - 1:y + 2, x - 1:x + 2].copy()
            nb[1, 1] = -1
            if s and s > nb.max():
                ref[y, x] = s
    got = O.fast_score_nms(img, 6)
    assert (ref > 0).sum() > 5
    assert np.array_equal(got, ref)


def test_ssd_disparity_brute_force():
    rng = np.random.RandomState(9)
    left = rng.randint(0, 256, (60, 90)).astype(np.uint8)
    right = np.roll(left, 5, axis=1)
    kps = np.float32([[30.4, 30.9], [3, 3], [88, 58], [45, 10]])
    win, sx, sy = 11, 12, 2
    got = O.ssd_disparity(left, right, kps, win, sx, sy, 1)
    ref = window_cases.ssd_ref(left, right, kps, win, sx, sy, 1)     # brute-force int64 map, first float minimum
    for i in range(len(kps)):
        assert got[i] == ref["disparity"][i]
    assert got[0] == 5.0


def test_klt_recovers_translation():
    sc = util.scenario("tiny", 2, 0, 1)
    img = sc["L"][0]
    shifted = ndimage.shift(img.astype(np.float64), (1.5, -2.25), order=1, mode="mirror")
    shifted = np.clip(np.round(shifted), 0, 255).astype(np.uint8)
    win = 21
    a, b = O.build_lk_pyramid(img, win), O.build_lk_pyramid(shifted, win)
    rng = np.random.RandomState(10)
    pts = np.stack([rng.uniform(40, 280, 60), rng.uniform(40, 200, 60)], 1).astype(np.float32)
    out, st, err = O.klt_track(a, b, pts, pts.copy(), win)
    good = st > 0
    assert good.sum() >= 50
    flow = (out - pts)[good]
    assert np.abs(np.median(flow[:, 0]) + 2.25) < 0.1 and np.abs(np.median(flow[:, 1]) - 1.5) < 0.1
    assert np.all(err[good] < 10) and np.all(np.isinf(err[~good]))


def test_depth_filter_kalman_step():
    x, P = O.kf1_update(0.5, 0.04, 1e-4, 0.01, 0.6)
    Pp = 0.04 + 1e-4
    K = Pp / (Pp + 0.01)
    assert abs(x - (0.5 + K * 0.1)) < 1e-6 and abs(P - (1 - K) * Pp) < 1e-7


def test_pose_filter_matches_float64_kalman():
    cfg = dict(synth.CONFIGS["tiny"])
    s = O.Slam(util.oracle_camera(cfg))
    x, P = np.zeros(12), np.eye(12)
    Q = 100 * np.eye(12)
    rng = np.random.RandomState(11)
    for i in range(6):
        dt = 0.0 if i % 2 == 0 else 0.05
        A = np.eye(12)
        A[:6, 6:] = dt * np.eye(6)
        z = rng.normal(0, 0.2, 12)
        R = np.diag([0.1] * 6 + [1.0] * 6)
        x, P = A @ x, A @ P @ A.T + Q
        K = P @ np.linalg.inv(P + R)
        x, P = x + K @ (z - x), P - K @ P
        out = s.update_pose(z[:6], z[6:], [0.1] * 6, [1.0] * 6, dt)
        assert np.allclose(out, x[:6], atol=1e-4)


# -------------------------------------------------------------- system level
def test_oracle_tracker_follows_ground_truth():
    """Thesis-level envelope (doc/doc.tex:1231-1257: cm / sub-degree errors) on a synthetic
    sequence: the restated pipeline tracks the known camera path."""
    cfg, L, R, poses, ts = synth.make_sequence("tiny", 14, 0, device="cpu")
    s = O.Slam(util.oracle_camera(cfg))
    for k in range(14):
        s.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        k2, k3, info = s.keypoints()
        assert np.all(k3[:, 2] > 0) or k > 0               # intent of test_depth_calculator.cpp:56-58
        if k >= 3:
            assert np.max(np.abs(s.pose()[:3] - poses[k][:3])) < 0.06  # y and rx are weakly separable at 320x240
            assert np.max(np.abs(s.pose()[3:] - poses[k][3:])) < 0.03
    assert s.num_keyframes() >= 1


def test_first_keyframe_one_keypoint_per_cell():
    """Intent of the stale test_corner_detector.cpp:24-66: one keypoint per grid box."""
    left, right = util.real_pair()
    kps, score, typ = O.detect_keypoints(left, 40, 50, 0)
    assert len(kps) == (752 // 40) * (480 // 50)
    cells = {(int(x) // 40, int(y) // 50) for x, y in kps}
    assert len(cells) == len(kps)


# ------------------------------------------------------------- golden vectors
def test_golden_vectors_real_pair():
    g = np.load(os.path.join(util.GOLDEN, "golden_real_pair.npz"))
    left, right = util.real_pair()
    assert np.array_equal(np.array([crc(p) for p in O.build_pyramid(left, 6)], np.uint32), g["pyr_crc"])
    lk = O.build_lk_pyramid(left, 31)
    assert np.array_equal(np.array([crc(p) for p in lk], np.uint32), g["lk_crc"])
    assert np.array_equal(np.array([crc(O.scharr(p)) for p in lk], np.uint32), g["scharr_crc"])
    assert np.array_equal(O.ssd_disparity(left, right, g["kps"], 31, 60, 6, 1), g["disp_31"])
    assert np.array_equal(O.ssd_disparity(left, right, g["kps"], 35, 60, 6, 1), g["disp_35"])
    pts, st, err = O.klt_track(lk, O.build_lk_pyramid(right, 31), g["kps"],
                               (g["kps"] + np.float32([10, 0])).astype(np.float32), 31)
    assert np.array_equal(st, g["klt_status"]) and np.array_equal(pts, g["klt_pts"])
    assert np.array_equal(err, g["klt_err"])
    assert crc(O.fast_score_nms(left, 6)) == g["fast_crc"]
    dk, ds, dt = O.detect_keypoints(left, 40, 50, 0)
    assert np.array_equal(dk, g["det_kps"]) and np.array_equal(dt, g["det_type"])
    # the real pair is a plausible stereo pair: most disparities are positive and finite
    assert (g["disp_31"] > 0.5).mean() > 0.8
    # alignment of the pair against itself: the right image is the left camera moved by the baseline
    cfg = dict(synth.CONFIGS["econ"])
    cam = util.oracle_camera(cfg)
    slam = O.Slam(cam)
    slam.new_image(left, right, 0.0)
    k2, k3, info = slam.keypoints()
    assert np.array_equal(k2, g["kf0_kps2d"]) and np.array_equal(k3, g["kf0_kps3d"])
    nl = cfg["max_pyramid_levels"]
    pose, cost, tr = O.sparse_align(O.build_pyramid(left, nl), O.build_pyramid(right, nl), k2, k3,
                                    util.flags_of(info), cam, np.zeros(6, np.float32))
    assert np.array_equal(pose, g["sia_pose"]) and np.float32(cost) == g["sia_cost"]
    assert [[t["n_gradient"], t["n_cost"], t["n_accepted"], t["exit_small"]] for t in tr] == g["sia_trace"].tolist()
    assert abs(pose[0] + cfg["baseline"] / cfg["fx"]) < 0.01 and np.max(np.abs(pose[3:])) < 5e-3
    m2, mfl = O.refine_merge(g["rp_proj0"], util.flags_of(info), g["rp_tracked"], g["rp_err"])
    rpose, rcost, rtr = O.reproj_gn(m2, k3, mfl, cam, g["rp_start"])
    assert np.array_equal(m2, g["rp_merged"]) and np.array_equal(rpose, g["rp_pose"])
    assert [rtr["n_gradient"], rtr["n_cost"], rtr["n_accepted"], rtr["exit_small"]] == g["rp_trace"].tolist()


def test_golden_sequence():
    """The stored 5-frame sequence: the oracle tracker reproduces its committed poses, keypoints and
    GN traces (regression of the restatement itself; the GPU twin is tests/test_golden_gpu.py)."""
    s = np.load(os.path.join(util.GOLDEN, "golden_sequence.npz"))
    slam = O.Slam(util.oracle_camera(dict(synth.CONFIGS["tiny"])))
    for k in range(len(s["ts"])):
        assert slam.new_image(s["left"][k], s["right"][k], float(s["ts"][k])) == int(s[f"f{k}_kf"])
        k2, k3, info = slam.keypoints()
        assert np.array_equal(slam.pose(), s[f"f{k}_pose"])
        assert np.array_equal(k2, s[f"f{k}_kps2d"]) and np.array_equal(k3, s[f"f{k}_kps3d"])
        assert np.array_equal(info, s[f"f{k}_info"])


# ------------------------------------------------- the keyframe path's detector
def test_numpy_fast_statement_against_brute_force():
    """tests/keyframe_cases.py states FAST in closed form (largest over the arcs of the smallest difference);
    here it meets the arc test tried threshold by threshold, on small patches of the crafted textures"""
    import keyframe_cases as K
    ring = K.RING

    def is_corner(img, y, x, t):
        d = [int(img[y, x]) - int(img[y + dy, x + dx]) for dx, dy in ring]
        return any(all(d[(s + i) % 16] > t for i in range(9)) or all(d[(s + i) % 16] < -t for i in range(9))
                   for s in range(16))

    corners = 0
    for name in ("noise", "saturated", "lowc7", "bowls", "half_lr", "dots4"):
        img = K.texture(name, 22, 26)
        raw = np.zeros(img.shape, np.uint8)
        for y in range(3, 19):
            for x in range(3, 23):
                t = 5
                while t < 255 and is_corner(img, y, x, t + 1):
                    t += 1
                raw[y, x] = t if t >= 6 else 0
        assert np.array_equal(K.fast_raw(img), raw), name
        corners += int((raw > 0).sum())
    assert corners > 100


@pytest.mark.parametrize("grid", [(40, 40), (16, 16), (5, 7)])
def test_detect_keypoints_against_numpy_statement(grid):
    """O.detect_keypoints against corner_detector.cpp:27-78 written with numpy (closed-form FAST, scipy Sobel,
    explicit cell loops) on every crafted texture, ties for the best score included"""
    import keyframe_cases as K
    gw, gh = grid
    fast_ties = edge_ties = types = 0
    for name in K.TEXTURES:
        img = K.texture(name, 120, 160, gw, gh)
        nms, edge = K.fast_nms(K.fast_raw(img)), K.sobel_u8(img)
        assert np.array_equal(O.fast_score_nms(img, 6), nms), name
        assert np.array_equal(O.sobel_x_u8(img), edge), name
        kps, score, typ = O.detect_keypoints(img, gw, gh, 0)
        rk, rs, rt = K.detect_ref(img, gw, gh, nms, edge)
        assert len(kps) == (160 // gw) * (120 // gh)
        assert np.array_equal(kps, rk) and np.array_equal(score, rs) and np.array_equal(typ, rt), name
        fast_ties += len(K.tie_cells(nms, gw, gh))
        edge_ties += sum(1 for j, i in K.tie_cells(edge, gw, gh) if nms[j * gh:(j + 1) * gh, i * gw:(i + 1) * gw].max() == 0)
        types |= (1 << K.FAST if (typ == K.FAST).any() else 0) | (1 << K.EDGELET if (typ == K.EDGELET).any() else 0)
    assert types == 3
    if grid == (40, 40):                       # cells whose first best pixel depends on the scan order
        assert fast_ties > 0 and edge_ties > 0


def test_detect_keypoints_on_other_sizes_against_numpy_statement():
    import keyframe_cases as K
    for (w, h), (gw, gh) in (((203, 131), (43, 27)), ((16, 16), (4, 4)), ((16, 16), (16, 16)), ((113, 97), (54, 48)),
                             ((99, 64), (96, 64)), ((7, 9), (5, 7))):
        for name in ("noise", "binary", "const77", "checker7", "half_tb"):
            img = K.texture(name, h, w, gw, gh)
            for a, b in zip(O.detect_keypoints(img, gw, gh, 0), K.detect_ref(img, gw, gh)):
                assert np.array_equal(a, b), (w, h, gw, gh, name)


# first frame of O.Slam on crafted images (right = left rolled by 7 px): corners in the densest cell + 1 px
# (numpy), keypoints kept, cells, [FAST, edgelet], keypoints per level. Recorded from this oracle: they say
# when the oracle moves, and how far simple textures are from what a rendered frame reaches.
FIRST_FRAME_ANSWERS = [
    ("euroc", {}, "noise", 1047, 121, 130, [121, 0], [121, 0, 0]),
    ("euroc", {}, "bowls", 1652, 99, 130, [99, 0], [99, 0, 0]),
    ("euroc", {}, "const77", 0, 96, 130, [0, 96], [0, 0, 96]),
    ("euroc", {}, "half_lr", 1033, 115, 130, [102, 13], [66, 0, 49]),
    ("blender", {}, "noise", 1431, 93, 100, [93, 0], [93, 0, 0]),
    ("blender", {}, "bowls", 2288, 90, 100, [90, 0], [90, 0, 0]),
    ("euroc", {"grid_width": 96, "grid_height": 64}, "noise", 2376, 47, 49, [47, 0], [47, 0, 0]),
    ("euroc", {"grid_width": 96, "grid_height": 64}, "bowls", 3812, 20, 49, [20, 0], [20, 0, 0]),
    ("tiny", {}, "const77", 0, 0, 48, [0, 0], [0, 0, 0]),
    ("tiny", {}, "ramp_x", 0, 0, 48, [0, 0], [0, 0, 0]),
    ("tiny", {}, "stripes_x", 0, 0, 48, [0, 0], [0, 0, 0]),
    ("tiny", {}, "checker7", 0, 17, 48, [7, 10], [0, 17, 0]),
    ("tiny", {"grid_width": 4, "grid_height": 4}, "noise", 21, 2624, 4800, [2512, 112], [2534, 90, 0]),
]


@pytest.mark.parametrize("config,over,name,densest,n_kps,n_cells,types,levels", FIRST_FRAME_ANSWERS,
                         ids=[f"{a[0]}-{a[1].get('grid_width', '')}-{a[2]}" for a in FIRST_FRAME_ANSWERS])
def test_first_frame_known_answers(config, over, name, densest, n_kps, n_cells, types, levels):
    import keyframe_cases as K
    cfg = dict(synth.CONFIGS[config])
    cfg.update(over)
    gw, gh, w, h = cfg["grid_width"], cfg["grid_height"], cfg["width"], cfg["height"]
    img = K.texture(name, h, w, gw, gh)
    assert int(K.corners_per_cell(img, gw, gh).max()) == densest
    slam = O.Slam(util.oracle_camera(cfg))
    assert slam.new_image(img, np.roll(img, 7, axis=1), 0.0) == 1 and slam.num_keyframes() == 1
    k2, k3, info = slam.keypoints()
    assert (len(k2), (w // gw) * (h // gh)) == (n_kps, n_cells)
    assert np.bincount(info["type"], minlength=2).tolist() == types
    assert np.bincount(info["level"], minlength=3).tolist() == levels
    assert np.array_equal(slam.pose(), np.zeros(6, np.float32))
