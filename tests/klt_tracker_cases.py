"""The KLT launch in the form the tracker makes it (csrc/klt.hip with proj_pose set, svo_klt_track_batch): the cases
of tests/test_klt_tracker_cpu.py and tests/test_klt_tracker_gpu.py, built from window_cases.klt_cases() by adding
the tracker's addressing, and the launches composed of them.

Nothing here calls the HIP library. numpy and the C oracle only.

A CASE is a stage case (keyframe image, current image, reference points, desired starts, window) plus
  the keyframe's kps2d array: longer than the point list, the case's points behind a shuffled, unique kp_index, the
  unused entries at positions inside the image that no point of the case has;
  a camera (pinhole, or with the econ distortion terms), a pose (zero or not) and kps3d at depths of 0.05 .. 500 whose
  projection lands near the desired start. The start that counts is O.project_keypoints(pose, kps3d, cam);
  a SECOND current image, pose and kps3d (`cur2`, `pose2`, `kps3d2`): the later frame that meets the templates the
  first one stored. Its starts are the first frame's moved by nothing, by a pixel or two, by tens of pixels (far
  from where the first frame looked) or out of the range in which a window is looked at at all;
  tmpl_cap: how many keypoints the keyframe's cache holds; for every fifth case the median kp_index, so that half of
  the points have no record and one point sits exactly on the limit (kp_index == tmpl_cap: the first without one).
The `absurd` cases replace some kps3d by points in the camera plane, behind the camera, 1e30 away, infinite and NaN:
as in alignment_cases.py, a position whose floor is not an int32 is "outside", and a NaN result equals a NaN.

A LAUNCH is a list of sequences, each a dict of host arrays in the shape of svo_klt_sequence (expected_sequence says
what the kernel must give for one; expected_flags which cache records a call stores). single() makes the launch of
one case; several_keyframes(), ignored_caches() and batch_of_five() the composed ones.
"""
import functools

import numpy as np

import oracle_py as O
import window_cases as WC
from geometry_cases import CAMERAS

F, D = np.float32, np.float64
LK_LEVELS = 3
KLT_OUTSIDE, KLT_FLAT, KLT_TRACK = 0, 1, 2
_INT_SETTINGS = dict(grid_height=40, grid_width=40, search_x=30, search_y=4, window_size_pose_estimator=4,
                     window_size_depth_calculator=21, max_pyramid_levels=4, min_pyramid_level_pose_estimation=1)
POSES = (np.zeros(6, F), np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.05], F), np.array([-1.5, 0.7, 0.1, -0.2, 0.1, 0.3], F))


def camera(kind, w, h, win):
    """camera settings (dict) for images of w x h: "pinhole", or "econ" with that camera's distortion terms"""
    cam = dict(_INT_SETTINGS, window_size_opt_flow=win, baseline=20.0, fx=0.9 * w, fy=0.93 * w, cx=0.5 * w - 0.3,
               cy=0.5 * h + 0.2, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0)
    if kind == "econ":
        cam.update({k: CAMERAS["econ"][k] for k in ("k1", "k2", "k3", "p1", "p2")})
    return cam


def oracle_camera(cam):
    return O.make_camera(**cam)


def back_project(target, depth, pose, cam):
    """float32 [n, 3]: world points at camera depth `depth` whose projection through `pose` lands near target [n, 2]
    (the distortion is undone by a few fixed-point rounds: near, not exact)"""
    x = (target[:, 0].astype(D) - cam["cx"]) / cam["fx"]
    y = (target[:, 1].astype(D) - cam["cy"]) / cam["fy"]
    xu, yu = x.copy(), y.copy()
    for _ in range(12):
        r2 = xu * xu + yu * yu
        cd = 1 + cam["k1"] * r2 + cam["k2"] * r2 * r2 + cam["k3"] * r2 * r2 * r2
        dx = 2 * cam["p1"] * xu * yu + cam["p2"] * (r2 + 2 * xu * xu)
        dy = cam["p1"] * (r2 + 2 * yu * yu) + 2 * cam["p2"] * xu * yu
        xu, yu = (x - dx) / cd, (y - dy) / cd
    wild = ~(np.isfinite(xu) & np.isfinite(yu)) | (np.hypot(xu, yu) > 2 * np.hypot(x, y) + 1)
    xu, yu = np.where(wild, x, xu), np.where(wild, y, yu)
    z = np.asarray(depth, D)
    xc = np.stack([xu * z, yu * z, z], 1)
    rot = O.rodrigues(np.asarray(pose[3:6], F))             # project_keypoints applies R(-r) to (P - t)
    return (xc @ rot.T + np.asarray(pose[:3], D)).astype(F)


def fit_points(target, depth, pose, cam, tries=24):
    """back_project at `depth` and at depths a few per cent off it, per point the one whose projection (the oracle's)
    comes closest to the target: for a pinhole camera most projections then ARE the target, bit for bit, which keeps
    the few points of the stage cases that end a level by a hair (final_window_outside) doing so"""
    ocam = oracle_camera(cam)
    best, err = None, None
    for j in range(tries):
        cand = back_project(target, np.asarray(depth, D) * (1 + 0.0137 * j), pose, cam)
        e = np.abs(O.project_keypoints(pose, cand, ocam).astype(D) - target).max(axis=1)
        if best is None:
            best, err = cand, e
        else:
            better = e < err
            best[better], err[better] = cand[better], e[better]
    return best


def keyframe_table(pts, seed, h, w):
    """(kps2d [m, 2], kp_index [n]): the points behind a shuffled unique index in a longer array whose other entries
    lie inside the image at positions of their own"""
    rng = np.random.RandomState(seed)
    n = len(pts)
    m = n + max(8, n // 4)
    kp_index = rng.permutation(m)[:n].astype(np.int32)
    table = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m)], 1).astype(F) + F(1 / 64)
    table[kp_index] = pts
    return table, kp_index


def second_starts(rng, init, h, w, win):
    """the later frame's desired starts, and what was done to each point: 0 nothing, 1 a pixel or two, 2 tens of pixels,
    3 out of the range of every level (floor(x / 4 - halfWin) and floor(x - halfWin) both outside [-win, w))"""
    n = len(init)
    kind = rng.choice(4, n, p=[0.15, 0.45, 0.25, 0.15])
    out = init.astype(D).copy()
    near = rng.uniform(-2, 2, (n, 2))
    far = rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(20, 60, (n, 2)) * (rng.randint(0, 3, (n, 1)) != np.arange(2))
    out += np.where((kind == 1)[:, None], near, 0) + np.where((kind == 2)[:, None], far, 0)
    side = rng.randint(0, 4, n)
    beyond = np.stack([np.where(side == 0, -5.0 * win, np.where(side == 1, w + 5.0 * win, out[:, 0])),
                       np.where(side == 2, -5.0 * win, np.where(side == 3, h + 5.0 * win, out[:, 1]))], 1)
    out = np.where((kind == 3)[:, None], beyond, out)
    return out.astype(F), kind


def _absurd(kps3d, pose, rng):
    """kps3d with every third point replaced by one of the absurd kinds; returns (kps3d, kind per point or -1)"""
    out = kps3d.copy()
    kind = np.full(len(out), -1)
    t = np.asarray(pose[:3], F)
    rot = O.rodrigues(np.asarray(pose[3:6], F))
    makers = (lambda p: t.copy(),                                              # camera plane: z = 0 exactly
              lambda p: (t.astype(D) - (p.astype(D) - t)).astype(F),         # behind the camera
              lambda p: p + (rot @ np.array([1e30, 0, 0])).astype(F),          # 1e30 to the side
              lambda p: p - (rot @ np.array([0, 1e30, 0])).astype(F),
              lambda p: np.array([np.inf, p[1], p[2]], F),
              lambda p: np.array([p[0], -np.inf, p[2]], F),
              lambda p: np.array([p[0], p[1], np.inf], F),
              lambda p: np.array([np.nan, p[1], p[2]], F),
              lambda p: np.array([p[0], p[1], np.nan], F),
              lambda p: np.full(3, np.nan, F))
    for i in range(0, len(out), 3):
        kind[i] = (i // 3) % len(makers)
        with np.errstate(all="ignore"):
            out[i] = makers[kind[i]](out[i])
    return out, kind


ABSURD_KINDS = ("camera_plane", "behind", "far_x", "far_y", "inf_x", "inf_y", "inf_z", "nan_x", "nan_z", "nan_all")


@functools.lru_cache(maxsize=None)
def cases():
    """list of dicts: name, win, prev, cur, cur2 (images), pts, init, init2, kind2, table (the keyframe's kps2d),
    kp_index, cam, pose, kps3d, pose2, kps3d2, tmpl_cap, absurd (kind per point, -1: none)"""
    out = []
    stage = WC.klt_cases()
    for k, (name, prev, cur, pts, init, win) in enumerate(stage):
        out.append(_case(k, name, prev, cur, pts, init, win, absurd=False))
    by_name = {c[0]: c for c in stage}
    for j, (src, pose_k) in enumerate((w, k) for w in ("noise_roll1-w31", "noise_roll1-w35") for k in range(len(POSES))):
        name, prev, cur, pts, init, win = by_name[src]
        out.append(_case(1000 + j, f"absurd{pose_k}-w{win}", prev, cur, pts, init, win, absurd=True, pose_k=pose_k))
    return out


def _case(k, name, prev, cur, pts, init, win, absurd, pose_k=None):
    h, w = prev.shape
    rng = np.random.RandomState(5000 + k)
    n = len(pts)
    cam = camera("econ" if k % 4 == 1 else "pinhole", w, h, win)
    pose = POSES[k % 3 if pose_k is None else pose_k]
    pose2 = POSES[(k + 1) % 3]
    table, kp_index = keyframe_table(pts, 100 + k, h, w)
    init2, kind2 = second_starts(rng, init, h, w, win)
    depth = np.exp(rng.uniform(np.log(0.05), np.log(500.0), n))
    kps3d, kps3d2 = fit_points(init, depth, pose, cam), fit_points(init2, depth[::-1], pose2, cam)
    kinds = np.full(n, -1)
    if absurd:
        kps3d, kinds = _absurd(kps3d, pose, rng)
        kps3d2, _ = _absurd(kps3d2, pose2, rng)
    shift = (1, -2) if min(h, w) > 9 else (0, 3)
    return dict(name=name, win=win, prev=prev, cur=cur, cur2=np.roll(cur, shift, axis=(0, 1)), pts=pts, init=init, init2=init2,
                kind2=kind2, table=table, kp_index=kp_index, cam=cam, pose=pose, kps3d=kps3d, pose2=pose2, kps3d2=kps3d2,
                tmpl_cap=len(table) if k % 5 != 2 else int(np.sort(kp_index)[n // 2]), absurd=kinds)


def case(name):
    return next(c for c in cases() if c["name"] == name)


_LEVELS = {}


def levels(c):
    """(keyframe levels, current levels, second current levels) of a case: the oracle's LK pyramids"""
    if c["name"] not in _LEVELS:
        _LEVELS[c["name"]] = tuple(O.build_lk_pyramid(c[k], c["win"]) for k in ("prev", "cur", "cur2"))
    return _LEVELS[c["name"]]


def starts(c, call):
    """what the kernel must start from in call 1 / 2 (the first frame) or 3 (the later one)"""
    pose, kps3d = (c["pose"], c["kps3d"]) if call < 3 else (c["pose2"], c["kps3d2"])
    return O.project_keypoints(pose, kps3d, oracle_camera(c["cam"]))


# ------------------------------------------------------------------ launches
def sequence(c, call=1, idx=None, seed=0, cache="own", n_lk=None, tmpl_cap=None):
    """one sequence of a launch from a case: all its points behind the case's own kp_index, or the points idx (may
    repeat) behind a fresh one. cache: "own" (a cache for this window), None, "wrong_win" (a cache made for another
    window, to be ignored). n_lk: the keyframe's levels (default: all)."""
    pl, cl, cl2 = levels(c)
    if idx is None:
        table, kp_index, sel = c["table"], c["kp_index"], np.arange(len(c["pts"]))
    else:
        sel = np.asarray(idx)
        table, kp_index = keyframe_table(c["pts"][sel], 900 + seed, *c["prev"].shape)
    pose, kps3d = (c["pose"], c["kps3d"]) if call < 3 else (c["pose2"], c["kps3d2"])
    kf = dict(levels=list(pl[:n_lk]), kps2d=table, cache=cache,
              tmpl_cap=(c["tmpl_cap"] if idx is None else len(table)) if tmpl_cap is None else tmpl_cap)
    return dict(win=c["win"], kfs=[kf], cur=list(cl if call < 3 else cl2), n=len(sel), kf_id=None, kp_index=kp_index,
                kps3d=np.ascontiguousarray(kps3d[sel]), pose=pose, cam=c["cam"], source=[(c["name"], call)])


def merge(seqs, cur_from=0):
    """one sequence whose points come from the keyframes of several: the keyframe tables side by side, kf_id says
    whose point it is, the points interleaved; the current image, pose and camera are those of seqs[cur_from]"""
    base = seqs[cur_from]
    kf_id = np.concatenate([np.full(s["n"], k, np.int32) for k, s in enumerate(seqs)])
    kp_index = np.concatenate([s["kp_index"] for s in seqs])
    kps3d = np.concatenate([s["kps3d"] for s in seqs])
    order = np.random.RandomState(77).permutation(len(kf_id))
    return dict(win=base["win"], kfs=[s["kfs"][0] for s in seqs], cur=base["cur"], n=len(order), kf_id=kf_id[order],
                kp_index=kp_index[order], kps3d=np.ascontiguousarray(kps3d[order]), pose=base["pose"], cam=base["cam"],
                source=sum((s["source"] for s in seqs), []))


def expected_sequence(s):
    """dict(tracked, status, err, proj, ref) [n]: the oracle's answer for a sequence of a launch"""
    n = s["n"]
    proj = O.project_keypoints(s["pose"], s["kps3d"][:n], oracle_camera(s["cam"])) if n else np.zeros((0, 2), F)
    kf_id = np.zeros(n, np.int32) if s["kf_id"] is None else s["kf_id"][:n]
    ref = np.zeros((n, 2), F)
    tracked, status, err = np.zeros((n, 2), F), np.zeros(n, np.uint8), np.zeros(n, F)
    for k, kf in enumerate(s["kfs"]):
        mine = np.nonzero(kf_id == k)[0]
        if mine.size == 0:
            continue
        ref[mine] = kf["kps2d"][s["kp_index"][mine]]
        tracked[mine], status[mine], err[mine] = O.klt_track(kf["levels"], s["cur"], ref[mine], proj[mine], s["win"])
    return dict(tracked=tracked, status=status, err=err, proj=proj, ref=ref)


def expected_flags(s):
    """per keyframe the uint8 [tmpl_cap, LK_LEVELS] flags that a call on an empty cache leaves: 1 at (kp_index, level)
    of the points present with kp_index < tmpl_cap for the levels that the call walks (None: the keyframe has no
    cache, or one for another window: nothing is stored)"""
    kf_id = np.zeros(s["n"], np.int32) if s["kf_id"] is None else s["kf_id"][:s["n"]]
    out = []
    for k, kf in enumerate(s["kfs"]):
        if kf["cache"] != "own":
            out.append(None)
            continue
        flags = np.zeros((kf["tmpl_cap"], LK_LEVELS), np.uint8)
        idx = s["kp_index"][:s["n"]][kf_id == k]
        flags[idx[idx < kf["tmpl_cap"]], :min(len(kf["levels"]), len(s["cur"]))] = 1
        out.append(flags)
    return out


def single(c, call=1, **kw):
    return [sequence(c, call, **kw)]


_THREE = {31: ("noise_roll1-w31", "binblocks2_sub-w31", "island-w31"), 35: ("noise_roll1-w35", "binblocks2_sub-w35", "island-w35")}


def several_keyframes(win, call=1):
    """one sequence whose points come from three keyframes with different images and 3, 2 and 1 levels (the current
    frame has 3), tracked into the first one's current image"""
    parts = [sequence(case(nm), call, n_lk=nl) for nm, nl in zip(_THREE[win], (3, 2, 1))]
    return [merge(parts)]


def ignored_caches(win, call=1):
    """one sequence over three keyframes: a cache made for another window (to be ignored whatever it holds), no
    cache at all, and a cache for fewer keypoints than the keyframe has (tmpl_cap below the largest kp_index)"""
    a, b, c = (case(nm) for nm in _THREE[win])
    return [merge([sequence(a, call, cache="wrong_win"), sequence(b, call, cache=None),
                   sequence(c, call, tmpl_cap=int(np.sort(c["kp_index"])[len(c["kp_index"]) // 3]))])]


BATCH_COUNTS = (0, 1, 63, 65, 70)
N_BOUND = 70


def batch_of_five(win, call=1):
    """five sequences with 0, 1, 63, 65 and n_bound points, their own images (three sizes) and keyframe tables"""
    names = {31: ("const77-w31", "small20x20-w31", "diag4_edge-w31", "blur_roll40px-w31", "noise_roll1-w31"),
             35: ("const77-w35", "small20x20-w35", "diag4_edge-w35", "blur_roll40ny-w35", "noise_roll1-w35")}[win]
    rng = np.random.RandomState(win)
    out = []
    for b, (nm, n) in enumerate(zip(names, BATCH_COUNTS)):
        c = case(nm)
        out.append(sequence(c, call, idx=rng.randint(0, len(c["pts"]), n), seed=10 * win + b))
    return out


# ------------------------------------------------------------------ what a call does, from the statement
def prefetch_rect(x, y, level_w, level_h, win, margin):
    """the rectangle (x0, y0, x1, y1) of the search tile that a cached level requests ahead for a start (x, y) at that
    level's scale, or None if it requests none because the window is not looked at (`look` is false)"""
    half = F(win - 1) * F(0.5)
    cx, cy = F(x) - half, F(y) - half
    if not (cx >= -win and cx < level_w and cy >= -win and cy < level_h):            # (NaN fails)
        return None
    px, py = int(np.floor(cx)), int(np.floor(cy))
    tj = win + 1 + 2 * margin
    tw = (tj + 6) & ~3
    x0, y0 = (px - margin) & ~3, py - margin
    return x0, y0, x0 + tw, y0 + tj


def top_level(c):
    pl, cl, _ = levels(c)
    return min(len(pl), len(cl)) - 1
