"""GPU parity of the keyframe path (csrc/keyframe.hip) against the CPU oracle on crafted images and layouts.

Stage level: svo_detect_keypoints (kf_detect_kernel launched as the tracker launches it) against
O.detect_keypoints, level by level, np.array_equal on count, x, y, score and type. Whole path:
kf_detect_kernel -> kf_select_merge_kernel -> SSD -> kf_init_kernel through a ctx against O.Slam, every
field of every keypoint bit for bit. No comparison here has a tolerance.

The images are ordinary 8-bit images (tests/keyframe_cases.py); what each must reach is asserted on the CPU
with a numpy FAST / Sobel statement that shares no code with the kernel or the oracle:

  branch of keyframe.hip                         reached by (asserted in)
  ---------------------------------------------  ---------------------------------------------------------
  corner list overflow, shape <56,48,1024>       bowls, weak_tiles 54x48 / 56x48; list_edge +1 (test_corner_list_edge)
  corner list overflow, shape <96,64,2048>       bowls 75x48 / 96x64, weak_tiles 96x64; list_edge +1 (same)
  list exactly full / one short                  list_edge 0 / -1 (test_corner_list_edge)
  every cell an edgelet (score 0 included)       const77, ramp_x (test_named_branches)
  FAST and edgelet cells in one frame            half_lr (test_named_branches)
  two pixels tie for the best FAST score         binary, saturated (test_named_branches)
  two pixels tie for the best Sobel response     checker7 (test_named_branches)
  dword-staged "inside" tile / byte-wise tile    layouts dense, strided / off1..3, oddstride on the same image
                                                 (test_detect_last_cells_and_layouts, test_detect_sizes)
  last column / row of cells around the halo     widths k*gw + {0,1,3,4,5,7,8}, heights k*gh + {0,1,3,4,5}
  zero keypoints from a keyframe                 `tiny` + const77 (test_zero_keypoint_frame)
  keyframe of score-0 edgelets of a coarse level `euroc` + const77 (test_first_frame)
  merge with n_old > 0, compaction, append order test_keyframe_on_half_flattened_frame
  enable flags of the five keyframe launches     test_one_sequence_of_three_makes_the_keyframe
  unaligned, odd-strided level 0 in every kernel test_borrowed_unaligned_frames_through_a_run

Changes of kf_detect_kernel's arithmetic that turn stage cases red (scratch builds, MI355X): `>=` in the
non-maximum suppression (49 cases), the edgelet scan in row-major order (110; the suite before this file
stayed green), the last best instead of the first best in the selection key (298), the overflow corners
scored with threshold 8 (8: `weak_tiles`, test_corner_list_edge). Threshold 7 there is no change at all: a
corner's score is at least 6 = 7 - 1 whichever way it is computed.

Found with these cases: the first HOST frame of a ctx could reach the kernels with 4 KB pieces zeroed, in
about one of a hundred ctxs (test_first_frame, host mode: `tiny` + dots4 gave keypoints (4, 28) and (4, 128)
for the oracle's (4, 4), which is what the image with bytes 0..8191 and 36864..40959 zeroed gives). The
staging buffer is allocated in the step that first fills it, and its clearing was left on the null stream,
which the ctx's non-blocking stream does not wait for (svo_group.hip, dev_alloc: now complete on return).
"""
import numpy as np
import pytest
import torch

import keyframe_cases as K
import oracle_py as O
import util
from stereo_svo_slam_amd import hip_lib, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


# ------------------------------------------------------------------ layouts
# dense: stride = width. strided: dword-aligned base and stride > width (the dword-staged tile of cells
# inside the image). off1..off3: first byte 1, 2, 3 bytes past a dword boundary (off1: aligned stride, off2:
# the tightest aligned stride, off3: odd stride too). oddstride: aligned base, stride not a multiple of 4.
LAYOUTS = ("dense", "strided", "off1", "off2", "off3", "oddstride")


def place(img, layout):
    """img (numpy uint8 [h, w]) on the GPU as a view in that layout; the bytes around it hold 0xA5"""
    h, w = img.shape
    up4 = (w + 3) // 4 * 4
    odd = w + 13 if (w + 13) % 4 else w + 14
    off, stride = {"dense": (0, w), "strided": (0, up4 + 16), "off1": (1, up4 + 16), "off2": (2, up4),
                   "off3": (3, odd), "oddstride": (0, odd)}[layout]
    buf = torch.full((off + h * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    view = buf[off:off + h * stride].view(h, stride)[:, :w]
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 4 == off and view.stride(0) == stride
    return view


def legal_levels(h, w, gw, gh, want=3):
    """levels (at most `want`) on which the reference's detector has a value: see svo_detect_keypoints"""
    n = 1
    while n < want and (gw >> n) > 0 and (gh >> n) > 0 and (w >> n) > 0 and (h >> n) >= (gh >> n):
        n += 1
    return n


def check_stage(H, img, gw, gh, n_levels, layout, tag=""):
    """svo_detect_keypoints on the halfSample pyramid of img against the oracle, level by level; returns
    the oracle's per-level (kps, score, type)"""
    h, w = img.shape
    pyr = O.build_pyramid(img, n_levels)
    views = [place(p, layout) for p in pyr]
    max_cells = hip_lib.detect_shape(w, h, n_levels, gw, gh)[0]
    cells, counts = H.detect_keypoints(views, gw, gh, max_cells)
    H.synchronize()
    got = hip_lib.detect_to_numpy(cells, counts)
    refs = []
    for l in range(n_levels):
        kps, score, typ = O.detect_keypoints(pyr[l], gw >> l, gh >> l, l)
        where = f"{tag} {w}x{h} grid {gw}x{gh} {layout} level {l}"
        assert len(got[l]) == len(kps), f"{where}: {len(got[l])} cells, oracle {len(kps)}"
        assert np.array_equal(got[l]["x"], kps[:, 0]) and np.array_equal(got[l]["y"], kps[:, 1]), f"{where}: position"
        assert np.array_equal(got[l]["score"], score), f"{where}: score"
        assert np.array_equal(got[l]["type"], typ), f"{where}: type"
        refs.append((kps, score, typ))
    return refs


# ------------------------------------------------------------- stage: textures x grids
GRIDS = ((4, 4), (5, 7), (16, 16), (40, 40), (54, 48), (56, 48), (57, 48), (56, 49), (75, 48), (96, 64), (43, 27))


@pytest.mark.parametrize("name", K.TEXTURES)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_detect_textures(H, grid, name):
    """every texture on every grid, three levels where the cell allows, the layouts in turn"""
    gw, gh = grid
    w, h = max(3 * gw + 5, 67), max(3 * gh + 3, 45)
    img = K.texture(name, h, w, gw, gh)
    layout = LAYOUTS[(GRIDS.index(grid) + K.TEXTURES.index(name)) % len(LAYOUTS)]
    check_stage(H, img, gw, gh, legal_levels(h, w, gw, gh), layout, name)


@pytest.mark.parametrize("n_levels", (1, 2, 3))
@pytest.mark.parametrize("name", ("noise", "half_tb", "checker7", "real"))
def test_detect_level_counts(H, name, n_levels):
    for gw, gh in ((43, 27), (54, 48), (5, 7)):
        check_stage(H, K.texture(name, 200, 260, gw, gh), gw, gh, n_levels, "dense", name)


# ------------------------------------------------------- stage: sizes, last cells, layouts
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", ((54, 48), (40, 40), (96, 64), (5, 7)), ids=lambda g: f"{g[0]}x{g[1]}")
def test_detect_last_cells_and_layouts(H, grid, layout):
    """the last column / row of cells just inside, on and past the 4 px halo and the row's last dword"""
    gw, gh = grid
    for dw in (0, 1, 3, 4, 5, 7, 8):
        for dh in (0, 1, 3, 4, 5):
            w, h = 2 * gw + dw, 2 * gh + dh
            check_stage(H, K.texture("noise", h, w, seed=dw * 8 + dh), gw, gh, legal_levels(h, w, gw, gh, 2), layout)


SIZES = {(16, 16): ((4, 4), (5, 7), (16, 16)),
         (203, 131): ((4, 4), (43, 27), (54, 48), (96, 64)),
         (752, 480): ((54, 48), (75, 48), (96, 64), (43, 27)),
         (1920, 1080): ((43, 24), (96, 64), (4, 4))}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_detect_sizes(H, size, layout):
    w, h = size
    for gw, gh in SIZES[size]:
        for name in ("noise", "bowls", "real"):
            check_stage(H, K.texture(name, h, w, gw, gh), gw, gh, legal_levels(h, w, gw, gh), layout, name)


# ----------------------------------------------------------------- stage: named branches
@pytest.mark.parametrize("grid", ((54, 48), (56, 48), (75, 48), (96, 64)), ids=lambda g: f"{g[0]}x{g[1]}")
def test_corner_list_edge(H, grid):
    """The corner list of the kernel shape: its densest cell + 1 px holds one corner fewer than the list,
    exactly as many, one more (the first corner scored where it is found) and, with `bowls`, 1.1 to 1.9
    times as many. Counted with the numpy FAST test."""
    gw, gh = grid
    _, cw, ch, cap = hip_lib.detect_shape(3 * gw, 3 * gh, 1, gw, gh)
    assert (cw, ch, cap) == ((56, 48, 1024) if gw <= 56 and gh <= 48 else (96, 64, 2048))
    for target in (cap - 1, cap, cap + 1):
        img = K.list_edge_image(gw, gh, target)
        assert K.corners_per_cell(img, gw, gh).max() == target
        for layout in LAYOUTS:
            check_stage(H, img, gw, gh, 1, layout, f"list {target}")
    img = K.texture("bowls", 4 * gh + 5, 4 * gw + 5)
    assert K.corners_per_cell(img, gw, gh).max() > 1.1 * cap
    for layout in LAYOUTS:
        check_stage(H, img, gw, gh, 2, layout, "bowls")
    if grid != (75, 48):
        # more corners than the list, all of score 6 and mostly neighbours: none but the isolated ones passes
        # the non-maximum suppression, so a corner that its place in the list gives another score stands out
        img = K.texture("weak_tiles", 4 * gh + 5, 4 * gw + 5)
        raw = K.fast_raw(img)
        assert K.corners_per_cell(img, gw, gh).max() > 1.2 * cap and set(np.unique(raw)) == {0, 6}
        for layout in LAYOUTS:
            check_stage(H, img, gw, gh, 2, layout, "weak_tiles")
    img = K.texture("noise", 4 * gh + 5, 4 * gw + 5)
    print(f"noise {gw}x{gh}: {K.corners_per_cell(img, gw, gh).max()} corners in the densest cell, list {cap}")
    check_stage(H, img, gw, gh, 2, "dense", "noise")


def test_named_branches(H):
    """every cell an edgelet; both types in one frame; ties for the best FAST score and for the best Sobel
    response whose first pixel differs between the two scan orders (found in the oracle's score maps, and the
    numpy statement agrees on the winner)"""
    gw, gh, w, h = 40, 40, 203, 131
    for name in ("const77", "ramp_x"):
        img = K.texture(name, h, w)
        assert (K.fast_raw(img) > 0).sum() == 0
        for layout in LAYOUTS:
            (kps, score, typ), = check_stage(H, img, gw, gh, 1, layout, name)
            assert len(typ) == (w // gw) * (h // gh) and np.all(typ == K.EDGELET)
    img = K.texture("half_lr", h, w)
    for layout in LAYOUTS:
        (kps, score, typ), = check_stage(H, img, gw, gh, 1, layout, "half_lr")
        assert (typ == K.FAST).sum() >= 3 and (typ == K.EDGELET).sum() >= 3
    for name in ("binary", "saturated"):
        img = K.texture(name, h, w)
        nms = O.fast_score_nms(img, 6)
        ties = K.tie_cells(nms, gw, gh)
        assert ties, f"{name}: no cell with a tie for the best FAST score"
        ref = K.detect_ref(img, gw, gh)
        for layout in LAYOUTS:
            got, = check_stage(H, img, gw, gh, 1, layout, name)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        for j, i in ties:                                  # the row-major first wins
            c = nms[j * gh:(j + 1) * gh, i * gw:(i + 1) * gw]
            y, x = np.unravel_index(np.argmax(c), c.shape)
            assert tuple(got[0][j * (w // gw) + i]) == (i * gw + x, j * gh + y)
    img = K.texture("checker7", h, w)
    nms, edge = O.fast_score_nms(img, 6), O.sobel_x_u8(img)
    ties = [(j, i) for j, i in K.tie_cells(edge, gw, gh) if nms[j * gh:(j + 1) * gh, i * gw:(i + 1) * gw].max() == 0]
    assert ties, "checker7: no edgelet cell with a tie for the best Sobel response"
    for layout in LAYOUTS:
        got, = check_stage(H, img, gw, gh, 1, layout, "checker7")
    for j, i in ties:                                      # the column-major first wins
        c = edge[j * gh:(j + 1) * gh, i * gw:(i + 1) * gw].T
        x, y = np.unravel_index(np.argmax(c), c.shape)
        assert tuple(got[0][j * (w // gw) + i]) == (i * gw + x, j * gh + y) and got[2][j * (w // gw) + i] == K.EDGELET


def test_detect_rejects_what_the_reference_has_no_value_for(H):
    img = place(K.texture("noise", 64, 64), "dense")
    for gw, gh, levels in ((3, 8, [img]), (8, 3, [img]), (97, 8, [img]), (8, 65, [img]),
                           (4, 4, [img, img, img, img]),             # cell 0 x 0 on level 3
                           (8, 64, [img, img[:31]])):                # level 1 lower than its cell of 32
        with pytest.raises(hip_lib.SvoError):
            H.detect_keypoints(levels, gw, gh, 4096)
    with pytest.raises(hip_lib.SvoError):                            # 256 cells do not fit 255
        H.detect_keypoints([img], 4, 4, 255)
    cells, counts = H.detect_keypoints([img, img[:, :7]], 16, 16)   # a level narrower than its cell: no cells
    assert hip_lib.detect_to_numpy(cells, counts)[1].size == 0 and counts.cpu().tolist() == [16, 0]


# ------------------------------------------------------------------ whole path: ctx vs O.Slam
def _config(name, **over):
    cfg = dict(synth.CONFIGS[name])
    cfg.update(over)
    return cfg


CTX_CONFIGS = {"euroc": _config("euroc"), "blender": _config("blender"), "tiny": _config("tiny"),
               "econ": _config("econ"), "euroc96x64": _config("euroc", grid_width=96, grid_height=64),
               "euroc32x32": _config("euroc", grid_width=32, grid_height=32),
               "tiny4x4": _config("tiny", grid_width=4, grid_height=4),
               "tiny8x8": _config("tiny", grid_width=8, grid_height=8)}
MODES = ("host", "device", "borrow")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Pair:
    """one ctx of n sequences next to n oracles, fed the same frames"""

    def __init__(self, cfg, n=1):
        self.cfg, self.n = cfg, n
        self.gpu = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n)
        self.ref = [O.Slam(util.oracle_camera(cfg)) for _ in range(n)]
        self.keep = []                     # borrowed frames stay alive and unchanged until the ctx is gone
        self.frames = 0

    def feed(self, lefts, rights, ts, mode, layout="off3"):
        made = [r.new_image(l, rr, ts) for r, l, rr in zip(self.ref, lefts, rights)]
        if mode == "host":
            self.gpu.new_images(lefts, rights, [ts] * self.n)
        elif mode == "device":
            self.gpu.new_images([torch.from_numpy(x).cuda() for x in lefts],
                                [torch.from_numpy(x).cuda() for x in rights], [ts] * self.n)
        else:
            dl, dr = [place(x, layout) for x in lefts], [place(x, layout) for x in rights]
            self.keep.append((dl, dr))
            torch.cuda.synchronize()
            self.gpu.new_images_packed(self.gpu.pack_images(dl, dr, [ts] * self.n, borrow=True))
        self.frames += 1
        return made

    def check(self, made, tag):
        """every sequence's frame, newest keyframe and statistics against its oracle, bit for bit"""
        for s in range(self.n):
            ref, t = self.ref[s], f"{tag} seq {s} frame {self.frames - 1}"
            st = self.gpu.stats(s)
            assert st.is_keyframe == made[s], f"{t}: keyframe decision"
            ok2, ok3, oinfo = ref.keypoints()
            f = self.gpu.get_frame(s)
            assert st.n_keypoints == len(ok2) == len(f.kps2d), \
                (f"{t}: {st.n_keypoints} keypoints (frame: {len(f.kps2d)}), oracle {len(ok2)}; the first of the frame: "
                 f"{f.kps2d[:12].tolist()} level {f.info['level'][:12].tolist()} type {f.info['type'][:12].tolist()} "
                 f"score {f.info['score'][:12].tolist()}")
            if np.isnan(ref.pose()).any() or np.isnan(ok2).any() or np.isnan(ok3).any():
                # NaN: the same bits, or a NaN in the same place (the convention of test_solve_lanes_gpu.py)
                util.compare_frame(t, f, f.kps2d, f.kps3d, oinfo, f.pose, tol=0.0)
                for a, b in ((f.pose, ref.pose()), (f.kps2d, ok2), (f.kps3d, ok3)):
                    assert np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))), t
            else:
                util.compare_frame(t, f, ok2, ok3, oinfo, ref.pose(), tol=0.0)
            for fld in ("color", "kf_inv_depth", "kf_variance"):
                assert np.array_equal(_bits(f.info[fld]), _bits(oinfo[fld])), f"{t}: info.{fld}"
            assert self.gpu.num_keyframes(s) == ref.num_keyframes(), t
            if self.frames > 1:
                assert util.same_trace(st, ref.stats(), self.cfg), f"{t}: GN trace differs from the oracle's"
            kid = ref.num_keyframes() - 1
            k2, k3, info, pose = ref.keyframe(kid)
            g = self.gpu.get_keyframe(kid, s)
            assert np.array_equal(g.kps2d.view(np.uint32), k2.view(np.uint32)), f"{t}: keyframe kps2d"
            assert np.array_equal(g.kps3d.view(np.uint32), k3.view(np.uint32)), f"{t}: keyframe kps3d"
            assert np.array_equal(g.pose.view(np.uint32), pose.view(np.uint32)), f"{t}: keyframe pose"
            for fld in util.INT_FIELDS + ("color", "score", "kf_inv_depth", "kf_variance"):
                assert np.array_equal(_bits(g.info[fld]), _bits(info[fld])), f"{t}: keyframe info.{fld}"

    def close(self):
        self.gpu.close()
        for r in self.ref:
            r.close()


def _first_frame(cfg_name, name, mode, same_right=False, layout="off3"):
    cfg = CTX_CONFIGS[cfg_name]
    left = K.texture(name, cfg["height"], cfg["width"], cfg["grid_width"], cfg["grid_height"])
    right = left.copy() if same_right else np.roll(left, 7, axis=1)
    p = Pair(cfg)
    made = p.feed([left], [right], 0.0, mode, layout)
    assert made == [1]
    p.check(made, f"{cfg_name} {name} {mode}")
    k2, k3, info = p.ref[0].keypoints()
    p.close()
    return k2, k3, info


@pytest.mark.parametrize("name", K.TEXTURES)
@pytest.mark.parametrize("cfg_name", CTX_CONFIGS)
def test_first_frame(cfg_name, name):
    """detection, index-wise choice across levels, merge into the swapped grid, SSD depth, filter and colour
    init, keyframe copy: the first frame of every texture on every configuration; host frames, device frames
    and borrowed unaligned views in turn"""
    mode = MODES[(list(CTX_CONFIGS).index(cfg_name) + K.TEXTURES.index(name)) % 3]
    _first_frame(cfg_name, name, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("noise", "const77", "half_lr", "bowls"))
def test_first_frame_every_memory_kind(name, mode):
    for cfg_name in ("euroc", "tiny", "euroc96x64"):
        for layout in (("off3", "strided", "oddstride") if mode == "borrow" else ("dense",)):
            _first_frame(cfg_name, name, mode, layout=layout)


def test_first_frame_right_equals_left():
    """the disparities are 0 and clamp to 0.5 in the depth init"""
    for cfg_name in ("euroc", "tiny"):
        k2, k3, info = _first_frame(cfg_name, "noise", "device", same_right=True)
        cfg = CTX_CONFIGS[cfg_name]
        clamped = np.float32(1) / (np.float32(cfg["baseline"]) / np.float32(0.5))
        assert len(k2) > 20 and (info["kf_inv_depth"] == clamped).mean() > 0.9   # (all but a keypoint at the bottom border)


def test_zero_keypoint_frame():
    """`tiny` on a constant image: every cell's edgelet sits on the cell's corner, the merge takes none: a
    keyframe of 0 keypoints, no error; `euroc` keeps 96 score-0 edgelets of level 2"""
    for mode in MODES:
        k2, k3, info = _first_frame("tiny", "const77", mode)
        assert len(k2) == 0
    k2, k3, info = _first_frame("euroc", "const77", "borrow")
    assert len(k2) == 96 and np.all(info["type"] == K.EDGELET) and np.all(info["score"] == 0) and np.all(info["level"] == 2)


def _cut(canvas, w, shift, flatten=None):
    """a frame of width w cut from the canvas `shift` px further right, one half set to 128"""
    f = canvas[:, 32 + shift:32 + shift + w].copy()
    if flatten == "right":
        f[:, w // 2:] = 128
    elif flatten == "bottom":
        f[f.shape[0] // 2:, :] = 128
    return f


def _canvas(cfg, kind, seed=0):
    h, w = cfg["height"], cfg["width"] + 64
    return K.blurred_noise(h, w, seed) if kind == "blur" else K.texture("noise", h, w, seed=seed)


@pytest.mark.parametrize("mode", MODES)
def test_constant_then_textured(mode):
    """tracking with few (`euroc`: 96 edgelets) or no (`tiny`) keypoints, then a keyframe from nothing"""
    for cfg_name in ("tiny", "euroc"):
        cfg = CTX_CONFIGS[cfg_name]
        tex = K.blurred_noise(cfg["height"], cfg["width"], 1)
        frames = (K.texture("const77", cfg["height"], cfg["width"]), tex, np.roll(tex, 2, axis=1))
        p = Pair(cfg)
        made_all = []
        for k, f in enumerate(frames):
            made = p.feed([f], [np.roll(f, 7, axis=1)], 0.1 * k, mode)
            p.check(made, f"{cfg_name} const->tex {mode}")
            made_all += made
        assert made_all[:2] == [1, 1] and len(p.ref[0].keypoints()[0]) > 40
        p.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg_name,kind,half", [("euroc", "blur", "right"), ("euroc", "noise", "bottom"),
                                                ("euroc", "blur", "bottom"), ("tiny", "blur", "right")])
def test_keyframe_on_half_flattened_frame(cfg_name, kind, half, mode):
    """frame 1 = frame 0 shifted by 2 px with one half flattened: a keyframe with n_old > 0 (occupied cells,
    find_bad_keypoints compaction, appended order); frame 2 tracks the mixed set"""
    cfg = CTX_CONFIGS[cfg_name]
    canvas = _canvas(cfg, kind)
    frames = [_cut(canvas, cfg["width"], 0), _cut(canvas, cfg["width"], 2, half), _cut(canvas, cfg["width"], 4, half)]
    p = Pair(cfg)
    for k, f in enumerate(frames):
        made = p.feed([f], [np.roll(f, 7, axis=1)], 0.1 * k, mode)
        p.check(made, f"{cfg_name} {kind} {half} {mode}")
        if k == 1:
            assert made == [1]
            info = p.ref[0].keypoints()[2]
            old, new = info["keyframe_id"] == 0, info["keyframe_id"] == 1
            assert old.sum() > 0 and new.sum() > 0
            if cfg_name == "euroc":        # (`tiny`: 20 old + 2 new, FAST only: the smaller case)
                assert old.sum() >= len(info) / 4 and new.sum() >= len(info) / 4
                assert (info["type"][new] == K.FAST).any() and (info["type"][new] == K.EDGELET).any()
    p.close()


def test_one_sequence_of_three_makes_the_keyframe():
    """one ctx of three sequences; on frame 1 only the middle one makes a keyframe (the enable flags and the
    packed argument slots of the five keyframe launches)"""
    for cfg_name, mode in (("euroc", "borrow"), ("tiny", "host"), ("euroc", "device")):
        cfg = CTX_CONFIGS[cfg_name]
        w = cfg["width"]
        canvases = [_canvas(cfg, "blur", s) for s in (3, 4, 5)]
        p = Pair(cfg, 3)
        for k in range(3):
            lefts = [_cut(c, w, 2 * k, "right" if (s == 1 and k > 0) else None) for s, c in enumerate(canvases)]
            made = p.feed(lefts, [np.roll(f, 7, axis=1) for f in lefts], 0.1 * k, mode)
            p.check(made, f"{cfg_name} 3 sequences {mode}")
            assert made == ([1, 1, 1] if k == 0 else [0, 1, 0] if k == 1 else made)
        p.close()


@pytest.mark.parametrize("config,n_frames,seed,motion", [("tiny", 12, 2, 4.0), ("euroc", 6, 0, 1.0)])
def test_borrowed_unaligned_frames_through_a_run(config, n_frames, seed, motion):
    """Borrowed frames are level 0 and the right image in place: views with stride = width + 13 that start 3
    bytes past a dword boundary through KLT, SSD, the alignment's level 0, the pyramids and the keyframe
    kernels, every frame bit for bit; `tiny` makes a keyframe inside the run"""
    cfg, L, R, poses, ts = synth.make_sequence(config, n_frames, seed, device="cpu", motion_scale=motion)
    p = Pair(cfg)
    kf = 0
    for k in range(n_frames):
        left, right = L[k].numpy(), R[k].numpy()
        h, w = left.shape
        buf = [torch.full((3 + h * (w + 13) + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
        views = [b[3:3 + h * (w + 13)].view(h, w + 13)[:, :w] for b in buf]
        views[0].copy_(torch.from_numpy(left))
        views[1].copy_(torch.from_numpy(right))
        assert all(v.data_ptr() % 4 == 3 and v.stride(0) == w + 13 for v in views)
        made = [p.ref[0].new_image(left, right, float(ts[k]))]
        p.keep.append(views)
        torch.cuda.synchronize()
        p.gpu.new_images_packed(p.gpu.pack_images([views[0]], [views[1]], [float(ts[k])], borrow=True))
        p.frames += 1
        p.check(made, f"{config} borrowed run")
        kf += made[0]
    assert kf >= (2 if config == "tiny" else 1)
    assert np.array_equal(p.gpu.get_trajectory(0).shape, (n_frames, 6))
    p.close()
