"""GPU parity of the two window kernels (csrc/klt.hip, csrc/depth.hip: ssd_disparity_kernel) against the CPU
oracle on the crafted images of tests/window_cases.py, bit for bit: stage entries svo_klt_track,
svo_build_lk_pyramid and svo_ssd_disparity, and the whole path through a ctx against O.Slam.

tests/test_window_cpu.py ties the oracle to plain numpy statements on the same cases and asserts, from the
statements' labels, what the cases reach (every way a KLT level can end, window sums above 2^32, a search
tile staged again in every direction, every template and match-map size, all-ties maps, SSDs above 2^24
whose float minimum is not the integer minimum). Here the kernels meet them:

  as plain device images (the shapes of test_parity_gpu.py's _klt_case / _ssd_case);
  as views into larger buffers: first byte 1, 2, 3 and 7 bytes past a dword boundary, row strides that are
  not multiples of 4 or 16, dword-aligned strides longer than the width; the bytes around a view hold a
  grey level that the image does not (window_cases.GUARD; the rarest one where a coarse level of a smooth
  image holds all 256), so a read outside the view changes the result.
  Every view lies inside its allocation with 64 bytes to spare. For KLT the oracle's pyramid levels are
  uploaded into such views, so that the track kernel sees them on every level;
  with 1, 63, 64, 65 and 1500 keypoints per call in shuffled order;
  through the batched tracker (template cache, batched SSD launch) on sequences of 0/255 textures.

No comparison has a tolerance. A test collects every case that differs and names them all.

Changes of the kernels that were tried in scratch builds on an MI355X:
  the integer (value, index) argmin key in ssd_disparity_kernel (the kernel before this file): the `parity`
    cases differ in exactly the keypoints that window_cases.ssd_ref marks (3 of 300 at window 31 / search_y 6,
    13 of 300 at 35 / 6, 1 of 100 at 31 / 7, 7 of 100 at 33 / 8), in every layout and keypoint count; the SSD
    and golden tests that existed before stay green;
  a11 of klt.hip's template summed over the wavefront in plain int32: 32 of the 76 KLT cases differ (the 0/255
    textures), in every layout, and all eight tracker sequences; the KLT and golden tests that existed before
    stay green;
  load_u8x16 without its `x + 16 <= im.w` fallback (the last 16-byte load of a row runs into the next row):
    NOT seen, and no value-based test can see it: the bytes past a template's or region's width are replaced by
    the pad value whichever way they were loaded, and a region ends at column w - 1 at the latest. The
    fallback only keeps the load of the image's last row inside the image.
"""
import numpy as np
import pytest
import torch

import oracle_py as O
import window_cases as WC
from stereo_svo_slam_amd import hip_lib, synth
from test_keyframe_gpu import Pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=4096)
    yield h
    h.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ layouts
# name -> (first byte's offset from a dword boundary, row stride as a function of the width)
def _odd_stride(w):
    s = w + 13
    while s % 4 == 0 or s % 16 == 0:
        s += 1
    return s


LAYOUTS = {"dense": (0, lambda w: w),
           "strided": (0, lambda w: (w + 3) // 4 * 4 + 16),        # aligned base and stride: the dword-staged tiles
           "off1": (1, lambda w: (w + 3) // 4 * 4 + 16),
           "off2": (2, lambda w: (w + 3) // 4 * 4),
           "off3": (3, _odd_stride),
           "off7": (7, lambda w: _odd_stride(w) + 2),
           "oddstride": (0, _odd_stride)}


def guard_value(img):
    """a grey level that img does not hold: GUARD for the generated images, another for their inverses; the
    rarest one for the coarse levels of a smooth image, which hold them all"""
    count = np.bincount(img.ravel(), minlength=256)
    return WC.GUARD if count[WC.GUARD] == 0 else int(np.argmin(count))


def place(img, layout):
    """img (numpy uint8 [h, w]) on the GPU as a view in that layout, surrounded by a grey level it does not hold"""
    h, w = img.shape
    off, stride = LAYOUTS[layout][0], LAYOUTS[layout][1](w)
    fill = guard_value(img)
    buf = torch.full((off + h * stride + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    view = buf[off:off + h * stride].view(h, stride)[:, :w]
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)))
    assert view.data_ptr() % 8 == off and view.stride(0) == stride and view.stride(1) == 1
    return view


# ------------------------------------------------------------------ the oracle's answers, once per case
_KLT_REF, _SSD_REF = {}, {}


def klt_expected(case):
    name, prev, cur, pts, init, win = case
    if name not in _KLT_REF:
        pl, cl = O.build_lk_pyramid(prev, win), O.build_lk_pyramid(cur, win)
        _KLT_REF[name] = (pl, cl) + tuple(O.klt_track(pl, cl, pts, init, win))
    return _KLT_REF[name]


def ssd_expected(case):
    name, left, right, kps, win, sx, sy, clamp = case
    if name not in _SSD_REF:
        _SSD_REF[name] = O.ssd_disparity(np.ascontiguousarray(left), np.ascontiguousarray(right), kps, win, sx, sy, clamp)
    return _SSD_REF[name]


def klt_differs(H, gp, gc, pts, init, win, ref_pts, ref_st, ref_err):
    """'' or what differs between svo_klt_track on the device levels gp / gc and the oracle's answer"""
    cur_pts = dev(init.copy())
    _, st, err = H.klt_track(gp, gc, dev(pts), cur_pts, win)
    st, err, got = st.cpu().numpy(), err.cpu().numpy(), cur_pts.cpu().numpy()
    if not np.array_equal(st, ref_st):
        return f"status of points {np.nonzero(st != ref_st)[0][:6].tolist()}"
    bad = np.nonzero(np.any(_bits(got) != _bits(ref_pts), axis=1))[0]
    if bad.size:
        return f"position of {bad.size} points, first {bad[:4].tolist()}: {got[bad[:2]].tolist()} for {ref_pts[bad[:2]].tolist()}"
    bad = np.nonzero(_bits(err) != _bits(ref_err))[0]
    if bad.size:
        return f"err of {bad.size} points, first {bad[:4].tolist()}: {err[bad[:2]].tolist()} for {ref_err[bad[:2]].tolist()}"
    return ""


def ssd_differs(H, left, right, kps, win, sx, sy, clamp, ref):
    got = H.ssd_disparity(left, right, dev(kps), win, sx, sy, clamp).cpu().numpy()
    bad = np.nonzero(_bits(got) != _bits(ref))[0]
    return f"{bad.size} keypoints, first {bad[:6].tolist()}: {got[bad[:6]].tolist()} for {ref[bad[:6]].tolist()}" if bad.size else ""


def _report(failed, total):
    assert not failed, f"{len(failed)} of {total} cases differ from the oracle:\n" + "\n".join(f"  {n}: {m}" for n, m in failed)


# ------------------------------------------------------------------ stage: every case
def test_klt_cases(H):
    """pyramids built by svo_build_lk_pyramid from the image, then svo_klt_track: _klt_case's shape"""
    failed = []
    for case in WC.klt_cases():
        name, prev, cur, pts, init, win = case
        pl, cl, ref_pts, ref_st, ref_err = klt_expected(case)
        gp, gc = H.build_lk_pyramid(dev(prev), win), H.build_lk_pyramid(dev(cur), win)
        if len(gp) != len(pl) or any(not np.array_equal(g.cpu().numpy(), r) for g, r in zip(gp + gc, pl + cl)):
            failed.append((name, "pyramid levels"))
            continue
        msg = klt_differs(H, gp, gc, pts, init, win, ref_pts, ref_st, ref_err)
        if msg:
            failed.append((name, msg))
    _report(failed, len(WC.klt_cases()))


def test_ssd_cases(H):
    failed = []
    for case in WC.ssd_cases():
        name, left, right, kps, win, sx, sy, clamp = case
        msg = ssd_differs(H, dev(left), dev(right), kps, win, sx, sy, clamp, ssd_expected(case))
        if msg:
            failed.append((name, msg))
    _report(failed, len(WC.ssd_cases()))


def test_cases_against_the_statements(H):
    """the kernels against the numpy statements themselves, without the oracle in between (the smaller cases)"""
    failed = []
    for case in WC.klt_cases():
        name, prev, cur, pts, init, win = case
        if len(pts) > 40 or win not in (5, 31, 35):
            continue
        pl, cl = klt_expected(case)[:2]
        rp, rs, re_, _ = WC.klt_ref(pl, cl, pts, init, win)
        msg = klt_differs(H, [dev(x) for x in pl], [dev(x) for x in cl], pts, init, win, rp, rs, re_)
        if msg:
            failed.append((name, msg))
    for case in WC.ssd_cases():
        name, left, right, kps, win, sx, sy, clamp = case
        if len(kps) > 100:
            continue
        ref = WC.ssd_ref(left, right, kps, win, sx, sy, clamp)["disparity"]
        msg = ssd_differs(H, dev(left), dev(right), kps, win, sx, sy, clamp, ref)
        if msg:
            failed.append((name, msg))
    _report(failed, "the small")


# ------------------------------------------------------------------ stage: layouts
@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_klt_layouts(H, layout):
    """the oracle's pyramid levels uploaded into views: svo_klt_track on every level of them; and
    svo_build_lk_pyramid reading its level 0 from such a view"""
    failed = []
    for case in WC.klt_cases():
        name, prev, cur, pts, init, win = case
        pl, cl, ref_pts, ref_st, ref_err = klt_expected(case)
        gp, gc = [place(x, layout) for x in pl], [place(x, layout) for x in cl]
        msg = klt_differs(H, gp, gc, pts, init, win, ref_pts, ref_st, ref_err)
        if msg:
            failed.append((name, msg))
        built = H.build_lk_pyramid(place(cur, layout), win)
        if len(built) != len(cl) or any(not np.array_equal(g.cpu().numpy(), r) for g, r in zip(built, cl)):
            failed.append((name, "pyramid levels from a view"))
    _report(failed, len(WC.klt_cases()))


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "dense"])
def test_ssd_layouts(H, layout):
    failed = []
    for case in WC.ssd_cases():
        name, left, right, kps, win, sx, sy, clamp = case
        msg = ssd_differs(H, place(left, layout), place(right, layout), kps, win, sx, sy, clamp, ssd_expected(case))
        if msg:
            failed.append((name, msg))
    _report(failed, len(WC.ssd_cases()))


def test_layouts_are_what_they_say():
    img = WC.texture("noise", 20, 203)
    seen = set()
    for layout in LAYOUTS:
        v = place(img, layout)
        seen.add((v.data_ptr() % 8, v.stride(0) % 4 == 0, v.stride(0) % 16 == 0, v.stride(0) > 203))
        assert np.array_equal(v.cpu().numpy(), img)
    assert {s[0] for s in seen} >= {0, 1, 2, 3, 7}
    assert (0, True, False, True) in seen or (0, True, True, True) in seen      # aligned base, aligned longer stride
    assert any(s[0] in (1, 3, 7) and not s[1] for s in seen) and any(s[0] == 0 and not s[1] for s in seen)
    assert 203 % 4 and 203 % 16 and WC.SSD_W % 4 and WC.SSD_W % 16                # widths with a tail


# ------------------------------------------------------------------ stage: keypoint counts
COUNTS = (1, 63, 64, 65, 1500)


@pytest.mark.parametrize("name", ["noise_far_start-w31", "antidiag_blocks_roll1-w35", "blur_roll40px-w31",
                                  "checker3_inv-w35", "diag4_edge-w21"])
def test_klt_keypoint_counts(H, name):
    """a point's answer does not depend on how many points share the call, or on which"""
    case = next(c for c in WC.klt_cases() if c[0] == name)
    _, prev, cur, pts, init, win = case
    pl, cl, ref_pts, ref_st, ref_err = klt_expected(case)
    gp, gc = [place(x, "off3") for x in pl], [place(x, "strided") for x in cl]
    rng = np.random.RandomState(31)
    failed = []
    for n in COUNTS:
        idx = rng.randint(0, len(pts), n)
        msg = klt_differs(H, gp, gc, pts[idx], init[idx], win, ref_pts[idx], ref_st[idx], ref_err[idx])
        if msg:
            failed.append((f"{name} n={n}", msg))
    _report(failed, len(COUNTS))


@pytest.mark.parametrize("name", ["parity-w35-sy6", "parity-w31-sy6", "walk35-c1", "walk5-c0", "noise-w31-sy7-c0",
                                  "const0v255-w35"])
def test_ssd_keypoint_counts(H, name):
    case = next(c for c in WC.ssd_cases() if c[0] == name)
    _, left, right, kps, win, sx, sy, clamp = case
    ref = ssd_expected(case)
    gl, gr = place(left, "off1"), place(right, "oddstride")
    rng = np.random.RandomState(32)
    failed = []
    for n in COUNTS:
        idx = rng.randint(0, len(kps), n)
        msg = ssd_differs(H, gl, gr, kps[idx], win, sx, sy, clamp, ref[idx])
        if msg:
            failed.append((f"{name} n={n}", msg))
    _report(failed, len(COUNTS))


# ------------------------------------------------------------------ whole path: ctx against O.Slam
def sequence(name, cfg):
    """four frames of a 0/255 texture: the image, moved by a pixel, by half pixels, by a pixel in x and two
    in y; the right image is the left one 7 px to the right (a true disparity of 7)"""
    img = WC.texture(name, cfg["height"], cfg["width"])
    lefts = [img, np.roll(img, 1, axis=1), WC.subpixel(img, 0.5, 1.5), np.roll(img, (1, 2), axis=(0, 1))]
    return lefts, [np.roll(f, 7, axis=1) for f in lefts]


@pytest.mark.parametrize("mode", ["borrow", "device"])
@pytest.mark.parametrize("name", ["binblocks2", "antidiag_blocks"])
@pytest.mark.parametrize("config", ["euroc", "econ"])         # windows 31 and 35: both shapes of both kernels
def test_tracker_on_high_contrast_frames(config, name, mode):
    """the batched tracker in its default mode: KLT with the keyframe's template cache, the batched SSD
    launch, the filter and the keyframe kernels on frames whose window sums leave int32; poses, keypoints
    and flags equal the oracle's after every frame, and the oracle still has keypoints to track at the end"""
    cfg = dict(synth.CONFIGS[config])
    lefts, rights = sequence(name, cfg)
    p = Pair(cfg)
    for k, (l, r) in enumerate(zip(lefts, rights)):
        made = p.feed([l], [r], 0.1 * k, mode, "off3")
        p.check(made, f"{config} {name} {mode}")
    info = p.ref[0].keypoints()[2]
    alive = int((info["ignore_completely"] == 0).sum())
    p.close()
    assert alive >= 20, f"{alive} keypoints alive in the oracle's last frame"
