"""GPU parity of csrc/pyramid.hip (pyr_stream_kernel<32 | 64>, pyr_fused_kernel) against the CPU oracle on the crafted
images and shapes of tests/pyramid_cases.py. Every comparison is np.array_equal on whole planes.

tests/test_pyramid_cpu.py ties the oracle to plain numpy statements on the same cases and asserts what the images
reach (the 16-bit ceiling 65408, both sides of (v + 128) >> 8, every residue of the truncating / 4, every impulse
visible on every level it can reach). Here the kernels meet them

  through the stage entries svo_build_pyramid (n_lk = 0) and svo_build_lk_pyramid (n_levels = 1), level 0 dense
  and as an unaligned view;
  through the ctx's own launch (launch_tracking, svo_group_step.hip), which no test compared densely before:
  n_levels and n_lk set together, three sequences on blockIdx.z, level 0 copied from the caller's frame and the
  right image copied by the extra workgroups (host and device frames), or level 0 being the caller's memory
  (borrowed views), or the ctx's own level 0 after rectification. Every plane of every slot's current image set is
  read back through a host-mode snapshot and compared with the oracle: left levels, right image, LK levels.

Which of the kernels a launch takes is decided by pyr_stream_rows and reported by nothing in the library: the case
table states the expected kernel from the rule (pyramid_cases.expected_kernel, checked against the table on the
CPU), and SVO_PYR_KERNEL forces the other two where the shape allows them.

Single-line errors that were seeded into pyramid.hip in scratch builds (MI355X; cases of this file's 156 that turn red,
and what the pyramid, golden, facade, gray-plane and first-frame tests that existed before made of it):
  `+ 127` for `+ 128` in the stream kernel's pyrDown level 2: 54 (stage 12, ctx 42); the earlier noise cases see it too;
  the `last_unit` selector of row_pass taking p[7] for p[6]: 75; the earlier noise cases see it too;
  the stream kernel's right-image copy written with the source's stride: 28, all ctx cases with host or device
    frames; earlier only the depths of the golden pair's first keyframe (752 wide: the ctx's pitch is 768) differed;
  the level-1 row reflection of pick5 off by one (tap -2): 75; the earlier noise cases see it too;
  the halfSample pair sums of row 2q + 2 kept only on the rows a block stores (right with n_lk = 0, wrong once the
    pyrDown window starts the walk two level-1 rows higher): 58, no stage case; earlier 8 whole-tracker cases;
  the tile kernel's right-image workgroups reading the left frame: 32, the ctx cases whose host or device frames
    take the tile kernel; every earlier test stayed green, none runs that copy.
"""
import functools

import numpy as np
import pytest
import torch

import oracle_py as O
import pyramid_cases as P
import rectify_ref as RR
import snapshot_ref as SR
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch
from test_keyframe_gpu import place as _place

pytestmark = pytest.mark.gpu

N_SLOTS = 3


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def place(img, layout):
    """test_keyframe_gpu's layouts, from a copy: the crafted images are shared and read-only"""
    return _place(np.array(img), layout)


@functools.lru_cache(maxsize=None)
def ref_planes(h, w, n_levels, name):
    """the oracle's (halfSample levels, LK levels) of one crafted image, computed once"""
    img = P.images(h, w)[name]
    return tuple(O.build_pyramid(img, n_levels)), tuple(O.build_lk_pyramid(img, P.lk_window(h, w)))


def differs(got, want):
    """None, or where two planes differ: shape, or count and the first pixels (y, x, got, want)"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    if got.shape != want.shape:
        return f"shape {got.shape}, oracle {want.shape}"
    if np.array_equal(got, want):
        return None
    ys, xs = np.nonzero(got != want)
    first = [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in zip(ys[:4], xs[:4])]
    return f"{len(ys)} pixels, first (y, x, got, oracle) {first}"


# ------------------------------------------------------------------ 1. stage entries
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_stage_entries(H, case, monkeypatch):
    """svo_build_pyramid and svo_build_lk_pyramid on every crafted image: level 0 dense (the kernel the case names),
    strided (the same kernel, rows further apart) and as a view 3 bytes past a dword boundary with an odd stride or
    with an odd stride alone (the tile kernel, whatever SVO_PYR_KERNEL says)"""
    monkeypatch.setenv("SVO_PYR_KERNEL", case.kernel)
    h, w, n = case.h, case.w, case.n_levels
    win = P.lk_window(h, w)
    bad = []
    for k, (name, img) in enumerate(P.images(h, w).items()):
        hs, lk = ref_planes(h, w, n, name)
        for layout in ("dense", "off3", ("strided", "oddstride")[k % 2]):
            got = H.build_pyramid(place(img, layout), n)
            H.synchronize()
            bad += [(name, layout, "halfSample", l, d) for l in range(n) if (d := differs(got[l], hs[l]))]
            got = H.build_lk_pyramid(place(img, layout), win)
            H.synchronize()
            if len(got) != len(lk) or len(got) != 3:
                bad.append((name, layout, "LK levels", len(got)))
            bad += [(name, layout, "pyrDown", l, d) for l in range(min(len(got), 3)) if (d := differs(got[l], lk[l]))]
    assert not bad, f"{len(bad)} planes differ: {bad[:12]}"


# ------------------------------------------------------------------ 2. the ctx's launch
def ctx_config(case):
    """the fewest cells the ctx takes at this size (one cell, or cells of the largest size): few keypoints or none"""
    h, w = case.h, case.w
    return dict(width=w, height=h, fx=float(w), fy=float(w), cx=w / 2.0, cy=h / 2.0, baseline=10.0,
                k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0, grid_width=min(w, 96), grid_height=min(h, 64),
                search_x=8, search_y=2, window_size_pose_estimator=4, window_size_opt_flow=P.lk_window(h, w),
                window_size_depth_calculator=9, max_pyramid_levels=case.n_levels,
                min_pyramid_level_pose_estimation=1 if case.n_levels <= 4 else 2)


def snapshot_planes(snap, n_levels):
    """(left levels, right, LK levels 1 ..) of the current frame's image set (set 0) of a host-mode Snapshot, in the
    directory order that snapshot_ref states"""
    ref = SR.parse(snap.host)
    assert ref["frame_id"] >= 0 and ref["n_image_sets"] >= 1
    assert (ref["pyramid_levels"], ref["lk_levels"]) == (n_levels, 3)
    base = 14 + 12 * ref["n_keyframes"]

    def plane(i):
        off, row_bytes, rows = ref["directory"][i]
        return snap.data[off:off + rows * row_bytes].reshape(rows, row_bytes)

    return ([plane(base + l) for l in range(n_levels)], plane(base + n_levels),
            [plane(base + n_levels + l) for l in (1, 2)])


class Run:
    """one ctx of three slots; every step feeds each slot its own crafted left and right image and compares every
    plane of every slot with the oracle"""

    def __init__(self, case, mode, layout, start, rectify=False):
        self.case, self.mode, self.layout = case, mode, layout
        self.names = list(P.images(case.h, case.w))
        self.at = start
        self.batch = StereoSlamBatch(ctx_config(case), case.w, case.h, N_SLOTS)
        if rectify:
            maps = RR.identity_maps(case.w, case.h)
            self.batch.set_rectification(maps, maps)
        self.keep = []                       # borrowed frames stay alive and unchanged until the ctx is gone
        self.current = [None] * N_SLOTS      # (left name, right name) of every slot's current frame
        self.step_no = 0
        self.bad = []

    def step(self, sit_out=()):
        c = self.case
        imgs = P.images(c.h, c.w)
        lefts, rights = [None] * N_SLOTS, [None] * N_SLOTS
        for s in range(N_SLOTS):
            if s in sit_out:
                continue
            # lefts walk through the images three per step, rights half the list further on: the six of a step differ
            left = self.names[(self.at + s) % len(self.names)]
            right = self.names[(self.at + s + len(self.names) // 2) % len(self.names)]
            lefts[s], rights[s] = imgs[left], imgs[right]
            self.current[s] = (left, right)
        self.at += N_SLOTS
        ts = [0.1 * self.step_no] * N_SLOTS
        if self.mode == "host":
            self.batch.new_images(lefts, rights, ts)
        else:
            dl = [None if x is None else place(x, self.layout) for x in lefts]
            dr = [None if x is None else place(x, self.layout) for x in rights]
            self.keep.append((dl, dr))
            torch.cuda.synchronize()
            if self.mode == "device":
                self.batch.new_images(dl, dr, ts)
            else:
                self.batch.new_images_packed(self.batch.pack_images(dl, dr, ts, borrow=True))
        self.check()
        self.step_no += 1

    def check(self):
        c = self.case
        imgs = P.images(c.h, c.w)
        for s, snap in enumerate(self.batch.save()):
            left, right = self.current[s]
            hs, lk = ref_planes(c.h, c.w, c.n_levels, left)
            levels, right_plane, lk_planes = snapshot_planes(snap, c.n_levels)
            where = (self.step_no, s, left, right)
            self.bad += [where + (f"left level {l}", d) for l in range(c.n_levels) if (d := differs(levels[l], hs[l]))]
            if d := differs(right_plane, imgs[right]):
                self.bad.append(where + ("right", d))
            self.bad += [where + (f"LK level {l}", d) for l in (1, 2) if (d := differs(lk_planes[l - 1], lk[l]))]

    def close(self):
        self.batch.close()

    def verdict(self):
        assert not self.bad, f"{len(self.bad)} planes differ (step, slot, left, right, plane, where): {self.bad[:12]}"


# host frames; device frames that are dense, strided (rows further apart than the ctx's own) and unaligned (the tile
# kernel ingests); borrowed views in four layouts
MEMORY = (("host", "dense"), ("device", "dense"), ("device", "strided"), ("device", "off3"),
          ("borrow", "dense"), ("borrow", "off3"), ("borrow", "strided"), ("borrow", "oddstride"))
STEPS = 6


def _ctx_cases():
    out = []
    for c in P.CASES:
        for m, (mode, layout) in enumerate(MEMORY):
            off, stride = P.layout_of(layout, c.w)
            runs = P.expected_kernel(c.h, c.w, c.n_levels, c.kernel, off, stride)
            if runs != c.runs and c.kernel != "stream":
                continue                     # an unaligned view takes the tile kernel anyway: once per shape will do
            out.append(pytest.param(c, mode, layout, m, runs, id=f"{P.case_id(c)}-{mode}-{layout}-{runs}"))
    return out


@pytest.mark.parametrize("case,mode,layout,m,runs", _ctx_cases())
def test_ctx_launch_dense(case, mode, layout, m, runs, monkeypatch):
    """Three slots in one launch (one group), six steps: step 0 only starts sequences (T == 0), step 1 is tracked
    while slot 1 sits it out and keeps its planes, the others are tracked steps of all three. The lefts of the eight
    memory kinds of a shape start 18 images apart, so that every crafted image is a left image in some ctx."""
    monkeypatch.setenv("SVO_GROUPS", "1")
    monkeypatch.setenv("SVO_PYR_KERNEL", case.kernel)
    run = Run(case, mode, layout, start=m * N_SLOTS * STEPS)
    try:
        assert run.batch.groups() == 1
        for k in range(STEPS):
            run.step(sit_out=(1,) if k == 1 else ())
    finally:
        run.close()
    run.verdict()


@pytest.mark.parametrize("mode", ("host", "device", "borrow"))
@pytest.mark.parametrize("case", [c for c in P.CASES if (c.h, c.w, c.kernel) in ((65, 129, "stream"), (34, 456, "stream"))],
                         ids=P.case_id)
def test_ctx_launch_after_rectification(case, mode, monkeypatch):
    """rectification on, identity maps: the remap writes the ctx's own level 0 and right image, the pyramid launch
    reads that level 0 in place (src_left = level 0: no copy branch, no right-image workgroups)"""
    monkeypatch.setenv("SVO_GROUPS", "1")
    monkeypatch.setenv("SVO_PYR_KERNEL", case.kernel)
    run = Run(case, mode, "off3" if mode == "borrow" else "dense", start=7, rectify=True)
    try:
        for k in range(3):
            run.step(sit_out=(0,) if k == 1 else ())
    finally:
        run.close()
    run.verdict()
