"""The occluded AR picture without a GPU: the numpy statement (tests/ar_occlusion_ref.py) against its own second form
on the crafted cases (tests/ar_occlusion_cases.py), what the cases reach, the struct sizes of the binding and the
rejections that are decided before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import ar_occlusion_cases as CASES
import ar_occlusion_ref as OR
import ar_ref as AR
from stereo_svo_slam_amd import hip_lib

ALL = CASES.cases()
IDS = [c["name"] for c in ALL]


def _render(case, form, pixel=AR.RGB8, mode=OR.DROP, alpha=128, lattice="own"):
    lat = case["lattice"] if lattice == "own" else lattice
    return form(case["gray"], case["cam"], case["draws"], case["light"], case["ambient"], case["near"], pixel, lat, mode, alpha,
                case["margin"], case["drop_flags"])


@pytest.fixture(scope="module")
def winners():
    """the winner form of every case, drop and dim: computed once"""
    return {(c["name"], mode): _render(c, OR.render, AR.RGBA8, mode) for c in ALL for mode in (OR.DROP, OR.DIM)}


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_the_winner_form_is_the_every_fragment_form(case, winners):
    for mode in (OR.DROP, OR.DIM):
        img, covered, hidden = winners[(case["name"], mode)]
        img2, covered2, hidden2 = _render(case, OR.render_fragments, AR.RGBA8, mode)
        assert (covered, hidden) == (covered2, hidden2), (case["name"], mode)
        assert img.tobytes() == img2.tobytes(), (case["name"], mode, int((img != img2).any(axis=2).sum()))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_nothing_occludes_without_records_that_do(case, winners):
    """no occluder, and a lattice of dropped records: ar_ref.render byte for byte, nothing hidden"""
    plain = AR.render(case["gray"], case["cam"], case["draws"], case["light"], case["ambient"], case["near"], AR.RGBA8)
    lattices = [None] if case["lattice"] is None else [None, CASES.all_dropped(case)["lattice"]]
    for lat in lattices:
        for mode in (OR.DROP, OR.DIM):
            img, covered, hidden = _render(case, OR.render, AR.RGBA8, mode, lattice=lat)
            assert img.tobytes() == plain.tobytes() and hidden == 0 and covered == winners[(case["name"], mode)][1]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_what_the_cases_reach(case, winners):
    """a condition on the inputs: every case with a lattice hides some mesh pixels and shows others, and every probe
    names a covered pixel that the record of its kind decides as the statement says"""
    if case["lattice"] is None:
        assert winners[(case["name"], OR.DROP)][2] == 0
        return
    H, W = case["H"], case["W"]
    _, covered, hidden = winners[(case["name"], OR.DROP)]
    assert 0 < hidden < covered, (case["name"], covered, hidden)
    keys = AR.key_plane(H, W, case["cam"], case["draws"], case["light"], case["ambient"], case["near"])
    zo = OR.occluder_plane(H, W, case["lattice"], case["drop_flags"])
    cov, hid = OR.hidden_plane(keys, zo, case["margin"])
    rec, cols, rows, step = case["lattice"]
    for kind, px, py, want in case["probes"]:
        assert cov[py, px] and bool(hid[py, px]) == want, (case["name"], kind, px, py)
        ix, iy = px // step, py // step
        if kind in ("beyond cols", "beyond rows"):
            assert (ix >= cols) if kind == "beyond cols" else (iy >= rows)
            # ... and the pixel beside it, inside the lattice, is hidden: only the missing cell shows this one
            bx, by = (cols * step - 1, py) if kind == "beyond cols" else (px, rows * step - 1)
            assert hid[by, bx], (case["name"], kind)
            continue
        # the record of the probe's cell replaced by a plain near one hides the pixel: the probe decides it
        plain = rec.copy()
        plain[iy * cols + ix] = np.array((0, 0, CASES.NEAR_Z, (0, 0, 0), 0), OR.MAP_POINT)
        assert OR.hidden_plane(keys, OR.occluder_plane(H, W, (plain, cols, rows, step), case["drop_flags"]), case["margin"])[1][py, px]
        z = OR.depth_of(keys)[py, px]
        r = rec[iy * cols + ix]
        if kind in CASES.BOUNDARIES:
            limit = np.float32(r["z"] + np.float32(case["margin"]))
            assert {"equal": z == limit, "ulp above": np.nextafter(limit, np.float32(np.inf)) == z,
                    "ulp below": np.nextafter(limit, np.float32(-np.inf)) == z}[kind], (case["name"], kind)
        else:
            assert not OR.occludes(r, case["drop_flags"]), (case["name"], kind)


def test_every_listed_kind_has_a_probe():
    kinds = {k for c in ALL for k, _, _, _ in c["probes"]}
    assert kinds >= set(CASES.NON_OCCLUDING) | set(CASES.BOUNDARIES) | {"beyond cols", "beyond rows"}
    with_margin = {k for c in ALL if c["margin"] > 0 for k, _, _, _ in c["probes"]}
    without = {k for c in ALL if c["margin"] == 0 for k, _, _, _ in c["probes"]}
    assert with_margin >= set(CASES.BOUNDARIES) and without >= set(CASES.BOUNDARIES)
    assert {(c["W"], c["H"]) for c in ALL} >= {(64, 16), (67, 19), (130, 33), (5, 3)}
    assert {c["lattice"][3] for c in ALL if c["lattice"]} >= {1, 3, 4, 16}
    assert any(c["lattice"] and c["lattice"][1] * c["lattice"][2] == 1 for c in ALL)


def test_dim_rule():
    c = np.array([0, 255, 0, 255, 200, 17], np.uint8)
    g = np.array([0, 0, 255, 255, 100, 250], np.uint8)
    assert OR.dim(c, g, 0).tolist() == c.tolist() and OR.dim(c, g, 256).tolist() == g.tolist()
    assert OR.dim(c, g, 128).tolist() == [0, 128, 128, 255, 150, 134]
    assert OR.dim(c, g, 1).tolist() == [0, 254, 1, 255, 200, 18] and OR.dim(c, g, 255).tolist() == [0, 1, 254, 255, 100, 249]
    case = next(x for x in ALL if x["name"] == "dim ends")
    imgs = [_render(case, OR.render, AR.RGB8, OR.DIM, a)[0] for a in (0, 1, 128, 255, 256)]
    plain = AR.render(case["gray"], case["cam"], case["draws"], case["light"], case["ambient"], case["near"], AR.RGB8)
    dropped = _render(case, OR.render, AR.RGB8, OR.DROP)[0]
    assert imgs[0].tobytes() == plain.tobytes() and imgs[4].tobytes() == dropped.tobytes()
    assert len({i.tobytes() for i in imgs}) == 5


def test_struct_sizes():
    assert (C.sizeof(hip_lib.ArOcclusion), C.sizeof(hip_lib.ArOccluder), hip_lib.AR_VISIBILITY_DTYPE.itemsize) == (128, 24, 32)
    assert hip_lib.AR_VISIBILITY_DTYPE == OR.VISIBILITY and hip_lib.MAP_POINT_DTYPE == OR.MAP_POINT
    assert (hip_lib.ArOcclusion.cloud.offset, hip_lib.ArOcclusion.check.offset, hip_lib.ArOcclusion.info.offset) == (32, 80, 112)
    o = hip_lib.ar_occlusion(step=3, hidden="dim", alpha=7, margin=0.5, drop_flags=4, lr_check=1.5, max_depth=9.0)
    assert (o.on, o.hidden, o.alpha, o.margin, o.drop_flags) == (1, hip_lib.AR_HIDDEN_DIM, 7, 0.5, 4)
    assert (o.cloud.step, o.cloud.frame, o.cloud.layout, o.cloud.max_depth, o.check.lr, o.check.max_lr_diff) == (3, hip_lib.CLOUD_CAMERA, 0, 9.0, 1, 1.5)
    assert (hip_lib.AR_HIDDEN_DROP, hip_lib.AR_HIDDEN_DIM) == (OR.DROP, OR.DIM)


def test_an_occlusion_is_checked_before_the_device():
    """svo_render_ar_occluded checks the scalar fields of its occlusion first: a bad one is named, a good one gets as
    far as the handle"""
    lib = hip_lib.lib()
    lib.svo_last_error.restype = C.c_char_p
    st = hip_lib.ar_style()

    def message(o):
        assert lib.svo_render_ar_occluded(None, 0, None, None, None, C.byref(st), C.byref(o), None, None, None) == -1
        return lib.svo_last_error().decode()

    assert "null handle" in message(hip_lib.ar_occlusion())
    assert "null handle" in message(hip_lib.ar_occlusion(on=False, alpha=256, margin=3.0))
    bad = []
    for field, value in (("on", 2), ("on", -1), ("hidden", 2), ("hidden", -1), ("alpha", -1), ("alpha", 257), ("margin", -0.5),
                         ("margin", float("inf")), ("margin", float("nan")), ("_reserved2", 1)):
        o = hip_lib.ar_occlusion()
        setattr(o, field, value)
        bad.append(o)
    for k in range(3):
        o = hip_lib.ar_occlusion(on=False)
        o._reserved[k] = 1
        bad.append(o)
    for o in bad:
        assert "occlusion" in message(o)
