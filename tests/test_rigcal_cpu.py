"""Rectification maps from calibrations, without a GPU: the f64 statement (tests/rigcal_ref.py) against the host
function the project had (replay.undistort_rectify_map) bit for bit on the EuRoC calibrations, against an independent
twin within one float32 ulp on every case, and the library's host half (svo_rectify_inverse, the struct) through
ctypes against the statement bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rigcal_ref as RC
from stereo_svo_slam_amd import hip_lib, replay

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svo_hip.h")
SMALL = (130, 65)                                         # (the size of the synthetic cases here)


def _cal(case):
    return hip_lib.CameraCalibration.from_mats(*case)


def test_statement_equals_the_host_maps_on_euroc():
    """752 x 480, both cameras, all four maps: the same float32 bits at every pixel (measured: 0 pixels differ)"""
    cams, (w, h) = RC.euroc()
    assert (w, h) == (752, 480)
    for side in ("LEFT", "RIGHT"):
        K, D, R, P = cams[side]
        assert not np.any(D[5:]), "a 5-coefficient model, as undistort_rectify_map takes"
        ref = replay.undistort_rectify_map(K, D[:5], R, P, (w, h))
        got = RC.maps(cams[side], w, h)
        for name, g, r in zip("xy", got, ref):
            differ = int(np.sum(g.view(np.uint32) != r.view(np.uint32)))
            print(f"{side} map_{name}: {differ} of {g.size} pixels differ")
            assert differ == 0, (side, name, differ)


def _ulps(a, b):
    """distance in float32 steps between finite values of one sign region (ordered integer view)"""
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("name", [n for n in RC.cases() if not n.startswith("euroc")])
def test_statement_is_within_one_ulp_of_the_twin(name):
    """two routes to the same maps agree to the last float32 step on every finite pixel; on the horizon case the
    pixels that are not finite are the one column where W = 0: fewer than 5 % of the image"""
    w, h = SMALL
    cal = RC.cases()[name]
    got, twin = RC.maps(cal, w, h), RC.twin_maps(cal, w, h)
    for axis, g, t in zip("xy", got, twin):
        bad = ~np.isfinite(g)
        if name == "horizon":
            assert bad[:, RC.HORIZON_COLUMN].all() and bad.sum() == h, "not finite exactly where W = 0"
            assert bad.mean() < 0.05
            assert np.array_equal(bad, ~np.isfinite(t))
        else:
            assert not bad.any() and np.isfinite(t).all()
        d = _ulps(g[~bad], t[~bad])
        print(f"{name} map_{axis}: {np.mean(d != 0):.4%} of the finite pixels differ, at most {d.max()} ulp")
        assert d.max() <= 1, (name, axis, int(d.max()))


def test_horizon_case_crosses_zero_inside_the_image():
    w, h = SMALL
    ir = RC.inverse(RC.cases()["horizon"])
    W = np.arange(w, dtype=np.float64)[None, :] * ir[6] + (np.arange(h, dtype=np.float64)[:, None] * ir[7] + ir[8])
    left, right = W[:, :RC.HORIZON_COLUMN], W[:, RC.HORIZON_COLUMN + 1:]
    assert (W[:, RC.HORIZON_COLUMN] == 0).all()
    assert ((left < 0).all() and (right > 0).all()) or ((left > 0).all() and (right < 0).all())


def test_calibration_struct_matches_the_header():
    text = open(HEADER).read()
    m = re.search(r"typedef struct svo_camera_calibration \{\s*/\* (\d+) bytes: K at (\d+), D at (\d+), R at (\d+), P at (\d+) \*/"
                  r"\s*double K\[9\], D\[8\], R\[9\], P\[9\];\s*\} svo_camera_calibration;", text)
    assert m, "the struct and the layout its comment states"
    size, *offs = (int(v) for v in m.groups())
    cc = hip_lib.CameraCalibration
    assert [n for n, _ in cc._fields_] == ["K", "D", "R", "P"]
    assert [getattr(cc, n).offset for n in "KDRP"] == offs == [0, 72, 136, 208]
    assert [getattr(cc, n).size for n in "KDRP"] == [72, 64, 72, 72]
    assert C.sizeof(cc) == size == 280


def test_from_mats_takes_the_forms_of_a_settings_file():
    cams, _ = RC.euroc()
    K, D, R, P = cams["LEFT"]
    full = np.concatenate([P, [[-47.9], [0.0], [0.0]]], 1)
    a = hip_lib.CameraCalibration.from_mats(K, D[:5], R, full)
    for d in (D[:4], D[:5].reshape(1, 5), D):
        assert bytes(hip_lib.CameraCalibration.from_mats(K, d, R, P)) == bytes(a)
    assert list(a.D) == list(D) and list(a.P) == list(P.ravel()) and list(a.K) == list(K.ravel())
    assert list(hip_lib.CameraCalibration.from_mats(K, D, None, P).R) == list(np.eye(3).ravel())
    for bad in (np.zeros(9), np.zeros(6), np.zeros(3)):
        with pytest.raises(ValueError):
            hip_lib.CameraCalibration.from_mats(K, bad, R, P)
    with pytest.raises(ValueError):
        hip_lib.CameraCalibration.from_mats(K, D, R, np.zeros((4, 4)))


@pytest.mark.parametrize("name", list(RC.cases()))
def test_rectify_inverse_equals_the_statement(name):
    cal = RC.cases()[name]
    got = hip_lib.rectify_inverse(_cal(cal))
    ref = RC.inverse(cal)
    assert np.isfinite(ref).all()
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (got, ref)


def test_rectify_inverse_rejects_and_leaves_ir_untouched():
    K, D, R, P = RC.cases()["euroc_left"]
    flat = P.copy()
    flat[2] = 0.0                                         # P R singular: a zero row, det exactly 0
    nan_d = D.copy()
    nan_d[3] = np.nan
    inf_k = K.copy()
    inf_k[0, 0] = np.inf
    nan_r = R.copy()
    nan_r[1, 2] = np.nan
    f = hip_lib.lib().svo_rectify_inverse
    for what, cal in (("NaN in D", (K, nan_d, R, P)), ("inf in K", (inf_k, D, R, P)), ("NaN in R", (K, D, nan_r, P)),
                      ("singular P R", (K, D, R, flat)), ("zero P", (K, D, R, np.zeros((3, 3))))):
        ir = (C.c_double * 9)(*range(1, 10))
        assert f(C.byref(_cal(cal)), ir) == -1, what
        assert list(ir) == list(range(1, 10)), what
        with pytest.raises(hip_lib.SvoError):
            hip_lib.rectify_inverse(_cal(cal))
    ir = (C.c_double * 9)()
    assert f(None, ir) == -1 and f(C.byref(_cal((K, D, R, P))), None) == -1
    assert f(C.byref(_cal((K, D, R, P))), ir) == 0


def test_euroc_input_hands_out_the_calibrations(tmp_path):
    """EurocInput.gpu_calibration(): left from RIGHT.*, right from LEFT.*, as gpu_maps(); host_maps=False computes none"""
    cams, _ = RC.euroc()
    lines = ["%YAML:1.0", "LEFT.width: 752", "LEFT.height: 480", "RIGHT.width: 752", "RIGHT.height: 480"]
    full = {"LEFT": np.concatenate([cams["LEFT"][3], np.zeros((3, 1))], 1),
            "RIGHT": np.concatenate([cams["RIGHT"][3], [[-47.90639384423901], [0.0], [0.0]]], 1)}
    for side in ("LEFT", "RIGHT"):
        K, D, R, _ = cams[side]
        for key, m in (("K", K), ("D", D[:5].reshape(1, 5)), ("R", R), ("P", full[side])):
            lines.append(f"{side}.{key}: !!opencv-matrix\n   rows: {m.shape[0]}\n   cols: {m.shape[1]}\n   dt: d\n"
                         f"   data: [{', '.join(repr(float(v)) for v in m.ravel())}]")
    settings = tmp_path / "settings.yaml"
    settings.write_text("\n".join(lines) + "\n")
    (tmp_path / "cam0").mkdir()
    (tmp_path / "cam0" / "data.csv").write_text("#timestamp [ns],filename\n")
    src = replay.EurocInput(str(tmp_path), str(settings), raw=True, host_maps=False)
    assert src.maps_l is None and src.maps_r is None
    left, right = src.gpu_calibration()
    assert bytes(left) == bytes(_cal(cams["RIGHT"])) and bytes(right) == bytes(_cal(cams["LEFT"]))
    with pytest.raises(ValueError):
        src.gpu_maps()
    with_maps = replay.EurocInput(str(tmp_path), str(settings), raw=True)
    assert RC.same_bits(with_maps.gpu_maps()[0][0], RC.maps(cams["RIGHT"], 752, 480)[0])
