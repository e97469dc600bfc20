"""The host-only side of the C++ facade (hostcpp/stereo_slam_types.hpp: PoseManager, KeyFrameManager, flags_of /
set_flags) in a stand-alone program (tests/cpp/pose_manager_check.cpp) built with g++, once plain and once with the
address and undefined-behaviour sanitizers; PoseManager against the oracle's Rodrigues and the statement of
tests/facade_ref.py, bit for bit. And the sequence of the facade's GPU tests, pinned from the oracle alone."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import facade_cases as FC
import facade_ref as FR
import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PI32 = F32(math.pi)
DBL_EPSILON = float(np.finfo(np.float64).eps)
REC_FLOATS, TEXT_BYTES = 33, 128
# measured here on the CPU over the poses below whose rotation is below 2.9 rad: the statement (float32 matrices and
# products) against its float64 twin, worst component difference 2.4e-4 (see test_robot_angles_close_to_the_float64_twin)
CLOSE_MARGIN = 1e-3


def _poses():
    """float32 [n, 6] poses (x y z rx ry rz) and what each family is for"""
    rng = np.random.default_rng(11)
    angles = [rng.uniform(-3.2, 3.2, (3000, 3))]                                    # random, up to past pi per axis
    single = np.zeros((300, 3))
    single[np.arange(300), np.arange(300) % 3] = rng.uniform(-3.2, 3.2, 300)          # single-axis poses
    angles.append(single)
    pi_lo, pi_hi = np.nextafter(PI32, F32(0)), np.nextafter(PI32, F32(4))
    fixed = [(0, 0, 0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.5), (-0.0, 1.0, 0.0), (0.25, 0.0, -0.0),
             (1e-17, 0, 0), (0, 1e-17, 1e-17), (1e-16, 0, 0), (2e-16, 0, 0), (0, 3e-16, 0), (2.3e-16, 0, 0),
             (1.2e-16, 1.2e-16, 1.2e-16), (1.3e-16, 1.3e-16, 1.3e-16),                 # theta either side of DBL_EPSILON
             (1e-8, 0, 0), (0, -1e-8, 0), (1e-8, 1e-8, -1e-8),
             (2 * math.pi, 0, 0), (0, 2 * math.pi, 0), (0, 0, -2 * math.pi), (4, 4, 4), (-4, 4, -4)]
    for axis in range(3):
        for v in (PI32, -PI32, pi_lo, pi_hi, -pi_lo, -pi_hi):                          # +-pi and the floats either side
            a = [0.0, 0.0, 0.0]
            a[axis] = float(v)
            fixed.append(tuple(a))
        # s of the composed rotation just below and just above 1e-5, near 0 and near pi
        for v in (1e-4, 2e-4, 2.4e-4, 2.5e-4, 3e-4, 3.5e-4, 4e-4, 5e-4, 7e-4, 1e-3, 3e-3, 1e-2,      # where float32 matrices lose theta
                  0.6e-5, 0.9e-5, 0.99e-5, 1.01e-5, 1.1e-5, 1.9e-5, math.pi - 0.6e-5, math.pi - 0.9e-5,
                  math.pi - 1.1e-5, math.pi - 1.9e-5, -math.pi + 0.9e-5, math.pi + 1.1e-5):
            a = [0.0, 0.0, 0.0]
            a[axis] = v
            fixed.append(tuple(a))
    # half turns about a general axis: a half turn about one axis composed with a turn about another one is a half
    # turn about an axis of the plane perpendicular to the second; these reach the sign rules of the pi arm
    for b in (-2.5, -1.0, -0.3, 0.3, 1.0, 2.5):
        fixed += [(PI32, b, 0), (-PI32, b, 0), (PI32, 0, b), (-PI32, 0, b), (b, 0, PI32), (b, 0, -PI32),
                  (0, PI32, b), (b, PI32, 0), (PI32, PI32, b), (PI32, b, PI32), (b, PI32, PI32)]
    fixed += [(PI32, PI32, 0), (PI32, 0, PI32), (0, PI32, PI32), (PI32, PI32, PI32), (-PI32, PI32, -PI32)]
    angles.append(np.array(fixed, np.float64))
    angles = np.concatenate(angles).astype(F32)
    poses = np.zeros((len(angles), 6), F32)
    poses[:, :3] = rng.uniform(-5, 5, (len(angles), 3)).astype(F32)
    poses[:, 3:] = angles
    poses[0, :3] = (-0.0, 1e-7, 123456.789)                                          # for the text of operator<<
    poses[1, :3] = (1e10, -2.5, 0.1)
    return poses


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("pose_manager")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "pose_manager_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", src]
    out = {"plain": str(d / "pose_manager_check"), "sanitized": str(d / "pose_manager_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


def _run_poses(exe, d, poses, through_stdin=False):
    src, dst = str(d / "poses.bin"), str(d / "out.bin")
    poses.tofile(src)
    if os.path.exists(dst):
        os.remove(dst)
    if through_stdin:
        with open(src, "rb") as fh:
            r = subprocess.run([exe, "poses", "-", dst], stdin=fh, capture_output=True, text=True, timeout=120)
    else:
        r = subprocess.run([exe, "poses", src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"poses {len(poses)}" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    raw = np.fromfile(dst, np.uint8).reshape(len(poses), REC_FLOATS * 4 + TEXT_BYTES)
    fl = np.ascontiguousarray(raw[:, :REC_FLOATS * 4]).view(F32).reshape(len(poses), REC_FLOATS)
    texts = [bytes(row).split(b"\0", 1)[0].decode() for row in raw[:, REC_FLOATS * 4:]]
    return dict(rot=fl[:, 0:9].reshape(-1, 3, 3), inv=fl[:, 9:18].reshape(-1, 3, 3), robot=fl[:, 18:21],
                translation=fl[:, 21:24], angles=fl[:, 24:27], vector=fl[:, 27:33], text=texts)


@pytest.fixture(scope="module")
def poses():
    p = _poses()
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def facade(built, poses, tmp_path_factory):
    return _run_poses(built["plain"], tmp_path_factory.mktemp("pm_run"), poses)


@pytest.fixture(scope="module")
def statement(poses):
    """the statement and its float64 twin per pose: computed once, shared"""
    st = [FR.robot_angles(p[3:]) for p in poses]
    tw = [FR.robot_angles64(p[3:]) for p in poses]
    return dict(v=np.stack([s[0] for s in st]), label=[s[1] for s in st], s=np.array([s[2] for s in st]),
                v64=np.stack([t[0] for t in tw]), label64=[t[1] for t in tw], angle64=np.array([t[2] for t in tw]))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_rotation_matrices_equal_the_oracles_rodrigues(facade, poses):
    """get_rotation_matrix = float(R(r)), get_inv_rotation_matrix = float(R(-r)) of the oracle, on bits"""
    want = np.stack([O.rodrigues(p[3:]) for p in poses]).astype(F32)
    want_inv = np.stack([O.rodrigues(-p[3:]) for p in poses]).astype(F32)
    bad = np.flatnonzero((_bits(facade["rot"]) != _bits(want)).any(axis=(1, 2)))
    assert len(bad) == 0, (len(bad), poses[bad[:5], 3:], facade["rot"][bad[:2]], want[bad[:2]])
    bad = np.flatnonzero((_bits(facade["inv"]) != _bits(want_inv)).any(axis=(1, 2)))
    assert len(bad) == 0, (len(bad), poses[bad[:5], 3:], facade["inv"][bad[:2]], want_inv[bad[:2]])
    theta = np.linalg.norm(poses[:, 3:].astype(np.float64), axis=1)
    zero = np.flatnonzero(theta == 0)                                                # +0 and -0 angles: the identity
    assert len(zero) >= 2 and all(np.array_equal(facade["rot"][i], np.eye(3, dtype=F32)) for i in zero)
    # the cases reach both sides of the identity cut at DBL_EPSILON, and past a whole turn
    assert ((theta > 0) & (theta < DBL_EPSILON)).any() and ((theta >= DBL_EPSILON) & (theta < 1e-15)).any()
    assert (theta > 2 * math.pi).any()


def test_the_getters_return_the_pose(facade, poses):
    assert np.array_equal(_bits(facade["translation"]), _bits(poses[:, :3]))
    assert np.array_equal(_bits(facade["angles"]), _bits(poses[:, 3:]))
    assert np.array_equal(_bits(facade["vector"]), _bits(poses))
    for p, text in zip(poses, facade["text"]):                                       # std::ostream << float is %g
        assert text == ",".join("%g" % float(v) for v in p), (p, text)
    assert facade["text"][0].startswith("-0,1e-07,123457,") and facade["text"][1].startswith("1e+10,-2.5,0.1,")


def test_robot_angles_equal_the_statement_on_bits(facade, poses, statement):
    """On the parent commit this fails at the half turns: the facade returned (0, 0, 0) for the pose angles
    (pi, 0, 0), (0, pi, 0) and (0, 0, -pi), where cv::Rodrigues takes its theta = pi arm."""
    got, want = facade["robot"], statement["v"]
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert len(bad) == 0, (len(bad), [(poses[i, 3:].tolist(), statement["label"][i], got[i].tolist(), want[i].tolist()) for i in bad[:8]])
    for angles, axis in (((PI32, 0, 0), 0), ((0, PI32, 0), 1), ((0, 0, -PI32), 2)):
        i = int(np.flatnonzero((poses[:, 3:] == np.array(angles, F32)).all(axis=1))[0])
        assert statement["label"][i].startswith(FR.PI) and abs(abs(got[i, axis]) - math.pi) < 1e-6, (angles, got[i])


def test_the_cases_reach_every_arm(poses, statement):
    labels, s = statement["label"], statement["s"]
    count = {name: labels.count(name) for name in set(labels)}
    assert count.get(FR.ZERO, 0) >= 10 and count.get(FR.GENERIC, 0) >= 3000, count
    for rule in ("+y", "+z", "+tie"):                                                # each sign rule of the pi arm
        assert sum(1 for l in labels if l.startswith(FR.PI) and rule in l) >= 2, (rule, count)
    assert count.get(FR.PI, 0) >= 3, count                                            # and the pi arm with none applied
    near_zero = np.array([l == FR.ZERO for l in labels])
    near_pi = np.array([l.startswith(FR.PI) for l in labels])
    generic = np.array([l == FR.GENERIC for l in labels])
    assert (near_zero & (s >= 0.5e-5) & (s < 1e-5)).any() and (near_pi & (s >= 0.5e-5) & (s < 1e-5)).any()
    assert (generic & (s >= 1e-5) & (s < 2e-5) & (statement["angle64"] < 1)).any()
    assert (generic & (s >= 1e-5) & (s < 2e-5) & (statement["angle64"] > 3)).any()
    assert (statement["angle64"] > 2.9).sum() >= 50 and (statement["angle64"] < 2.9).sum() >= 2000


def test_robot_angles_close_to_the_float64_twin(facade, poses, statement):
    """Below a rotation of 2.9 rad the statement (and so the facade, which equals it on bits) agrees with its float64
    twin within CLOSE_MARGIN = 1e-3. Measured here over these poses: worst component difference 2.4e-4, at the pose
    angles (2.4e-4, 0, 0). That is where the float32 matrices cost most: cos(theta) = 1 - theta^2 / 2 rounds to the
    float 1 up to theta = sqrt(2^-24) = 2.44e-4, and acos(1) = 0 loses the whole angle; above it acos moves by the
    rounding of c (about 6e-8) over sin(theta), which falls. A product of three float matrices rounds c a few times
    more (about 4 x 3e-8), which loses angles up to sqrt(2.4e-7) = 5e-4: hence 1e-3, not the measured figure. Past
    2.9 rad the same 6e-8 / sin(theta) grows without bound, and only the comparison on bits applies there."""
    below = statement["angle64"] < 2.9
    diff = np.abs(statement["v"].astype(np.float64) - statement["v64"]).max(axis=1)
    worst = int(np.argmax(np.where(below, diff, 0)))
    print("worst difference below 2.9 rad:", diff[worst], "at pose angles", poses[worst, 3:], "rotation", statement["angle64"][worst])
    print("worst difference above 2.9 rad:", diff[~below].max())
    assert diff[below].max() < CLOSE_MARGIN, (diff[worst], poses[worst, 3:])
    assert np.abs(facade["robot"].astype(np.float64) - statement["v64"]).max(axis=1)[below].max() < CLOSE_MARGIN


def test_sanitized_build_computes_the_same(built, facade, poses, tmp_path):
    """the same program under the address and undefined-behaviour sanitizers, poses through stdin: clean, same bytes"""
    san = _run_poses(built["sanitized"], tmp_path, poses, through_stdin=True)
    for key in ("rot", "inv", "robot", "translation", "angles", "vector"):
        assert np.array_equal(_bits(san[key]), _bits(facade[key])), key
    assert san["text"] == facade["text"]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_keyframe_manager_and_flags(built, which):
    """KeyFrameManager gives ids 0, 1, 2 ..., nullptr at and beyond size(), get_keyframes copies; flags_of / set_flags
    round-trip all eight combinations (the asserts are in the program)"""
    r = subprocess.run([built[which], "types"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "types ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_the_sequence_reaches_three_keyframes_and_mixed_frames():
    """The oracle alone over the sequence of the GPU tests (tiny, 14 frames, motion_scale 4, seed FC.SEED = 26, the
    first seed that gives this: seeds 0 .. 25 make one or two keyframes): at least three keyframes, and a later frame whose live keypoints come from two
    keyframe ids, with keyframes made before it, so PoseRefiner's grouping and DepthFilter's look-ups have work."""
    for colour in (False, True):
        frames, keyframes, trajectory = FC.oracle_run(colour)
        assert len(frames) == FC.FRAMES == len(trajectory) and frames[0]["made"]
        assert len(keyframes) >= 3, len(keyframes)
        mixed = FC.mixed_frames(frames)
        assert mixed, "no frame with keypoints of two keyframes"
        k = FC.stage_frame(frames)
        assert 2 <= k < FC.FRAMES and frames[k - 1]["n_keyframes"] >= 2
        live = frames[k - 1]["info"]["ignore_completely"] == 0
        ids, counts = np.unique(frames[k - 1]["info"]["keyframe_id"][live], return_counts=True)
        assert len(ids) >= 2 and counts.min() >= 1, (ids, counts)
        for f in frames:                                            # every IMU loop returned poses
            assert np.isfinite(f["updates"]).all()
        assert sum(len(f["updates"]) for f in frames) == 3 * len(FC.IMU_AFTER)
