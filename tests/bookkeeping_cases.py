"""Plain statements of the keyframe path's bookkeeping (the two compactions, the selection across levels, the merge
into the grid, the depth and filter initialisation, the backup rule) and of the tracker's form of the SSD launch,
and the case lists of tests/test_bookkeeping_cpu.py and tests/test_bookkeeping_gpu.py.

Nothing here calls the HIP library. numpy only, written from the reference's source:

  compact_ref(mode 0)  remove_outliers, src/lib/stereo_slam.cpp:43-56
  compact_ref(mode 1)  find_bad_keypoints, src/lib/depth_calculator.cpp:67-86
  live_ref             the comment on CompactArgs::min_kf (csrc/svo_tracker.hpp): the project's own value
  select_ref           select_best_keypoints, src/lib/depth_calculator.cpp:37-65
  merge_ref            merge_keypoints, :88-130: the literal double loop over cells, the list growing inside it
  init_ref             the per-point part of DepthCalculator::calculate_depth, :241-289, and the copy of
                       KeyFrameManager::create_keyframe, src/lib/keyframe_manager.cpp:15-32
  backup_ref           src/lib/stereo_slam.cpp:237-245
  ssd_launch_ref       which entries of `disparity` a launch of grid (n_bound, batch) writes

A keypoint set is a dict of its twelve planes as uint32 arrays [cap, words] (PLANES) and "n": the tests compare bit
patterns, NaN payloads included. Every float step is one float32 operation (init_ref takes T: np.float64 is its twin,
the same expressions in double; a twin says whether the float formula is sound, not what the kernel must give).
The statements share no code with the oracle or the kernels, with one exception that geometry_cases.py set before:
the float statement's rotation matrix is geometry_cases.pose_mats, which rounds oracle_py.rodrigues (cv::Rodrigues in
double with the project's own sin and cos, tied down by tests/test_oracle_cpu.py) to float; the twin's is numpy's.
Every statement labels, per keypoint or per run, the branch it took.
"""
import functools

import numpy as np

import geometry_cases as GC
import window_cases as WC

F, D = np.float32, np.float64
U = np.uint32
IGNORE_DURING_REFINEMENT, IGNORE_COMPLETELY, IGNORE_TEMPORARY = 1, 2, 4
KP_FAST, KP_EDGELET = 0, 1
INT_MAX = 2**31 - 1
LCG_SEED = 12345
GUARD = U(0xA5C3F00D)

# the planes of a keypoint set in the order of svo_kps_planes: (name, words per keypoint, is float)
PLANES = (("kps2d", 2, True), ("kps3d", 3, True), ("flags", 1, False), ("kf_id", 1, False), ("kp_index", 1, False),
          ("outlier_count", 1, False), ("inlier_count", 1, False), ("kf_inv_depth", 1, True), ("kf_variance", 1, True),
          ("score", 1, True), ("level_type", 1, False), ("color", 1, False))
PLANE_NAMES = tuple(p[0] for p in PLANES)

COMPACT_LABELS = ("kept", "dropped_completely", "dropped_refinement", "outside_left", "outside_top", "outside_right",
                  "outside_bottom", "kept_nan", "kept_on_far_border", "kept_minus_zero", "kept_with_foreign_bits",
                  "kept_temporary", "empty", "all_kept", "none_kept", "started")
LIVE_LABELS = ("none_kept", "one_id", "bit_63", "beyond_mask", "across_words", "min_only_dropped", "id_0", "high_ids")
SELECT_LABELS = ("level0_stays", "fast_beats_edgelet", "higher_score_stays", "replaced", "equal_score_coarser_wins",
                 "edgelet_replaced_by_fast", "beyond_level_count", "replaced_twice", "level2_against_level1")
MERGE_LABELS = ("appended", "cell_occupied", "on_border_x", "on_border_y", "not_positive", "in_partial_last_cell",
                "shares_cell", "outside_grid", "old_inside", "old_on_border", "old_at_width", "old_at_height", "old_nan",
                "overflow", "exactly_cap", "no_old", "old_full", "nothing_selected")
INIT_LABELS = ("disparity_clamped", "disparity_half", "disparity_above_half", "disparity_nan", "disparity_inf",
               "first_frame", "no_new", "all_new", "backup_cleared", "backup_kept", "evicts", "no_evict")


def f32(words):
    return np.ascontiguousarray(words, U).view(F)


def bits(values):
    return np.ascontiguousarray(values, F).view(U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a == b
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ keypoint sets and device images of them
def coded_set(cap, n, salt=0):
    """a set whose every word says where it came from: plane, component, index; every seventh entry of a float
    plane is a NaN with a payload"""
    s = {"n": int(n)}
    i = np.arange(cap, dtype=np.uint64)
    for p, (name, w, is_float) in enumerate(PLANES):
        a = np.zeros((cap, w), U)
        for c in range(w):
            v = ((0x11 + p + salt) << 24) | (c << 20) | i
            if is_float:
                v = np.where(i % 7 == 3, 0x7F800000 | ((p + 1) << 16) | (c << 14) | (i + 1), v)
            a[:, c] = v.astype(U)
        s[name] = a
    return s


def copy_set(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


class Arena:
    """Named runs of 32-bit words, each 16-byte aligned with guard words behind it: one device buffer per test
    launch. `image(values)` lays values out; two images of one arena compare word for word, guards included."""

    def __init__(self):
        self.order, self.off, self.size = [], {}, 0

    def add(self, name, words):
        assert name not in self.off
        self.off[name] = (self.size, int(words))
        self.order.append(name)
        self.size += (int(words) + 1 + 3) // 4 * 4          # at least one guard word
        return name

    def add_set(self, prefix, cap):
        for name, w, _ in PLANES:
            self.add(f"{prefix}.{name}", cap * w)
        self.add(f"{prefix}.n", 1)

    def image(self, values):
        buf = np.full(self.size, GUARD, U)
        for name, v in values.items():
            o, w = self.off[name]
            v = np.ascontiguousarray(v).reshape(-1)
            v = v.view(U) if v.dtype.itemsize == 4 else v.astype(U)
            assert v.size == w, (name, v.size, w)
            buf[o:o + w] = v
        return buf

    def where(self, index):
        for name in self.order:
            o, w = self.off[name]
            if o <= index < o + w:
                return f"{name}[{index - o}]"
            if o + w <= index < o + (w + 1 + 3) // 4 * 4:
                return f"guard behind {name}"
        return "?"

    def mask(self, names):
        """True for the words that take part in a comparison: all but the runs in `names`"""
        m = np.ones(self.size, bool)
        for name in names:
            o, w = self.off[name]
            m[o:o + w] = False
        return m


def set_values(prefix, s):
    v = {f"{prefix}.{name}": s[name] for name in PLANE_NAMES}
    v[f"{prefix}.n"] = np.array([s["n"]], np.int32)
    return v


# ------------------------------------------------------------------ compaction
def compact_ref(src, mode, width=0, height=0):
    """(indices kept, label per keypoint)"""
    kept, labels = [], []
    for i in range(src["n"]):
        f = int(src["flags"][i, 0])
        if mode == 0:
            if f & IGNORE_COMPLETELY:
                labels.append("dropped_completely")
                continue
        else:
            x, y = f32(src["kps2d"][i])
            if x < 0:
                labels.append("outside_left")
                continue
            if y < 0:
                labels.append("outside_top")
                continue
            if x > F(width):
                labels.append("outside_right")
                continue
            if y > F(height):
                labels.append("outside_bottom")
                continue
            if f & IGNORE_COMPLETELY:
                labels.append("dropped_completely")
                continue
            if f & IGNORE_DURING_REFINEMENT:
                labels.append("dropped_refinement")
                continue
            if np.isnan(x) or np.isnan(y):
                labels.append("kept_nan")
            elif x == F(width) or y == F(height):
                labels.append("kept_on_far_border")
            elif (x == 0 and np.signbit(x)) or (y == 0 and np.signbit(y)):
                labels.append("kept_minus_zero")
        if len(labels) == i:
            labels.append("kept_with_foreign_bits" if f & ~7 else "kept_temporary" if f & IGNORE_TEMPORARY else "kept")
        kept.append(i)
    return kept, labels


def live_ref(src, kept):
    """[3] int32: the smallest origin keyframe among the keypoints kept (INT_MAX: none), then bit j of a 64-bit mask
    (low word first) = some kept keypoint comes from keyframe min + j; younger ones are not reported"""
    ids = [int(src["kf_id"][i, 0].view(np.int32)) for i in kept]
    if not ids:
        return np.array([INT_MAX, 0, 0], np.int32), ["none_kept"]
    base, mask = min(ids), 0
    for k in ids:
        if k - base < 64:
            mask |= 1 << (k - base)
    labels = []
    kept_set = set(kept)
    dropped = [int(src["kf_id"][i, 0].view(np.int32)) for i in range(src["n"]) if i not in kept_set]
    if len(set(ids)) == 1:
        labels.append("one_id")
    if mask >> 63:
        labels.append("bit_63")
    if any(k - base >= 64 for k in ids):
        labels.append("beyond_mask")
    if (mask >> 31) & 1 and (mask >> 32) & 1:
        labels.append("across_words")
    if dropped and min(dropped) < base:
        labels.append("min_only_dropped")
    if base == 0:
        labels.append("id_0")
    if base >= 4900:
        labels.append("high_ids")
    return np.array([base, mask & 0xFFFFFFFF, mask >> 32], U).view(np.int32), labels


def compact_expect(c, kept=None):
    """the words of every output of a compaction case after the launch (`kept`: from the oracle instead of the
    statement): dict of arena values"""
    out = compact_initial(c)
    if c["enable"] == 0:
        return out, ["disabled"]
    labels = []
    if c["start"]:
        kept_, labels = [], ["started"]
    else:
        kept_, labels = compact_ref(c["src"], c["mode"], c["width"], c["height"])
        labels = labels + (["empty"] if c["src"]["n"] == 0 else ["all_kept"] if len(kept_) == c["src"]["n"] else
                           ["none_kept"] if not kept_ else [])
    kept = kept_ if kept is None else list(kept)
    for name in PLANE_NAMES:
        d = c["dst"][name].copy()
        d[:len(kept)] = c["src"][name][kept]
        out[f"dst.{name}"] = d
    out["dst.n"] = np.array([len(kept)], np.int32)
    if c["start"]:
        out["src.n"] = np.array([0], np.int32)
    if c["min_kf"]:
        out["min_kf"], ll = live_ref(c["src"], kept)
        labels = labels + ll
    out["zero"] = np.zeros(c["zero_count"], np.int32)
    out["zero_res"] = np.zeros(c["zero_res_count"], np.int32)
    return out, labels


def compact_arena(c):
    a = Arena()
    a.add_set("src", c["cap"])
    a.add_set("dst", c["cap"])
    a.add("min_kf", 3)
    a.add("zero", c["zero_count"])
    a.add("zero_res", c["zero_res_count"])
    a.add("enable", 1)
    return a


def compact_initial(c):
    v = set_values("src", c["src"])
    v.update(set_values("dst", c["dst"]))
    v["min_kf"] = np.array([0x51515151] * 3, U)
    v["zero"] = np.full(c["zero_count"], 0x7A7A7A7A, U)
    v["zero_res"] = np.full(c["zero_res_count"], 0x7B7B7B7B, U)
    v["enable"] = np.array([0xFFFFFFFF if c["enable"] is None else c["enable"]], U)
    return v


def compact_threads(cap):
    """the rule of launch_compact, restated"""
    return 256 if cap <= 1024 else 1024


KEEP_PATTERNS = ("all", "none", "alternating", "first", "last", "thread_range", "rnd10", "rnd50", "rnd90")


def _keep_mask(pattern, n, cap, rng):
    k = np.zeros(n, bool)
    if pattern == "all":
        k[:] = True
    elif pattern == "alternating":
        k[::2] = True
    elif pattern == "first":
        k[:1] = True
    elif pattern == "last":
        k[n - 1:] = True
    elif pattern == "thread_range":              # everything but what thread 1 of the launch handles
        per = -(-n // compact_threads(cap)) if n else 0
        k[:] = True
        k[per:2 * per] = False
    elif pattern.startswith("rnd"):
        k = rng.rand(n) * 100 < int(pattern[3:])
    return k


def _compact_case(name, cap, n, mode, keep, rng, width=100, height=76, kf_ids=None, **kw):
    src, dst = coded_set(cap, n), coded_set(cap, 0x0BADBAD, salt=0x40)
    dst["n"] = 0x0BADBAD
    foreign = (rng.randint(0, 1 << 29, cap).astype(U) << U(3))
    fl = foreign | (rng.randint(0, 2, cap).astype(U) * U(IGNORE_TEMPORARY))
    if mode == 0:
        fl |= rng.randint(0, 2, cap).astype(U) * U(IGNORE_DURING_REFINEMENT)       # (remove_outliers does not look at it)
        fl[:n] = np.where(keep, fl[:n] & ~U(IGNORE_COMPLETELY), fl[:n] | U(IGNORE_COMPLETELY))
    else:
        xy = np.stack([rng.uniform(0, width, cap), rng.uniform(0, height, cap)], 1).astype(F)
        why = rng.randint(0, 6, cap)
        for i in np.nonzero(~keep)[0]:
            w = why[i]
            if w == 0:
                xy[i, 0] = -rng.uniform(0.01, 50)
            elif w == 1:
                xy[i, 1] = -rng.uniform(0.01, 50)
            elif w == 2:
                xy[i, 0] = width + rng.uniform(0.01, 50)
            elif w == 3:
                xy[i, 1] = height + rng.uniform(0.01, 50)
            elif w == 4:
                fl[i] |= U(IGNORE_COMPLETELY)
            else:
                fl[i] |= U(IGNORE_DURING_REFINEMENT)
        src["kps2d"] = bits(xy).reshape(cap, 2).copy()
    src["flags"] = fl.reshape(cap, 1)
    ids = rng.randint(3, 40, cap) if kf_ids is None else np.resize(np.asarray(kf_ids), cap)
    src["kf_id"] = ids.astype(np.int32).view(U).reshape(cap, 1)
    c = dict(name=name, cap=cap, mode=mode, width=width, height=height, src=src, dst=dst, start=0, zero_count=0,
             zero_res_count=0, enable=None, min_kf=mode == 0)
    c.update(kw)
    return c


@functools.lru_cache(maxsize=None)
def compact_cases():
    cases = []
    rng = np.random.RandomState(7)
    for cap in (1024, 1100, 2048):
        for n in sorted({0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025, cap}):
            if n > cap:
                continue
            for mode in (0, 1):
                for pat in KEEP_PATTERNS:
                    if n == 0 and pat != "all":
                        continue
                    cases.append(_compact_case(f"cap{cap}-n{n}-m{mode}-{pat}", cap, n, mode, _keep_mask(pat, n, cap, rng), rng))
    # mode 1: coordinates on the comparisons' edges, every combination of the three bits with foreign bits set
    cap, w, h = 1024, 100, 76
    tiny = -np.float32(1.4e-45)
    edge = [-0.0, tiny, 0.0, F(w), np.nextafter(F(w), F(np.inf)), F(h), np.nextafter(F(h), F(np.inf)), np.nan, np.inf, -np.inf, 50.0]
    xy = np.array([(x, 30.0) for x in edge] + [(30.0, y) for y in edge] + [(F(w), F(h)), (-0.0, -0.0), (np.nan, np.nan),
                                                                           (np.nan, -1.0), (-1.0, np.nan), (np.inf, np.nan)], F)
    for combo in range(8):
        c = _compact_case(f"edges-bits{combo}", cap, len(xy), 1, np.ones(len(xy), bool), rng, width=w, height=h)
        c["src"]["kps2d"][:len(xy)] = bits(xy).reshape(-1, 2)
        c["src"]["flags"][:len(xy), 0] = (c["src"]["flags"][:len(xy), 0] & ~U(7)) | U(combo) | U(0xFFFFFFF8 if combo % 2 else 0x80000008)
        cases.append(c)
    for combo in range(8):                  # the same bits under mode 0, with min_kf
        c = _compact_case(f"bits{combo}-m0", cap, 65, 0, np.ones(65, bool), rng)
        c["src"]["flags"][:65, 0] = (c["src"]["flags"][:65, 0] & ~U(7)) | U(combo)
        c["src"]["flags"][:65:2, 0] = U(combo)                  # (and without foreign bits)
        cases.append(c)
    # a sequence that starts
    for cap, n in ((1024, 777), (1024, 1024 + 5), (1100, 777), (2048, 2048 + 5)):
        for mode in (0, 1):
            c = _compact_case(f"start-cap{cap}-n{n}-m{mode}", cap, 0, mode, np.ones(0, bool), rng, start=1, min_kf=False)
            c["src"]["n"] = n
            cases.append(c)
    # the two zeroing jobs
    for k, (z, zr) in enumerate(((0, 1025), (1, 257), (5, 5), (257, 1), (1025, 0), (8, 27))):
        for cap in (1024, 2048):
            cases.append(_compact_case(f"zero{z}-res{zr}-cap{cap}", cap, 300, k % 2, _keep_mask("rnd50", 300, cap, rng), rng,
                                       zero_count=z, zero_res_count=zr, start=int(k == 5)))
    # the device predicate
    for en in (0, 0x100, 1):
        for mode in (0, 1):
            cases.append(_compact_case(f"enable{en:#x}-m{mode}", 1100, 513, mode, _keep_mask("rnd50", 513, 1100, rng), rng,
                                       enable=en, zero_count=5, zero_res_count=5))
    # min_kf: which keyframes the kept keypoints refer to
    def live(name, ids, keep, cap=1024):
        ids, keep = np.asarray(ids), np.asarray(keep, bool)
        c = _compact_case(f"live-{name}", cap, len(ids), 0, keep, rng)
        c["src"]["kf_id"][:len(ids), 0] = ids.astype(np.int32).view(U)
        cases.append(c)
    live("one-id", [17] * 70, [1] * 70)
    live("5-68", [5, 68] * 40, [1] * 80)
    live("5-69", [5, 69] * 40, [1] * 80)
    live("5-68-69", [69, 5, 68, 69] * 30, [1] * 120)
    live("31-32", [5, 36, 37, 5] * 33, [1] * 132)
    live("only-31", [5, 36] * 33, [1] * 66)
    live("only-32", [5, 37] * 33, [1] * 66)
    live("min-dropped", [2] + [9, 11, 72] * 100, [0] + [1] * 300)
    live("min-dropped-last", [9, 11, 72] * 100 + [2], [1] * 300 + [0], cap=2048)
    live("none-kept", [4, 5, 6] * 20, [0] * 60)
    live("id0", [0, 63, 64, 1] * 20, [1] * 80)
    live("id0-only", [0], [1])
    live("near-5000", list(range(4990, 5060)) * 3, ([1] * 69 + [0]) * 3, cap=1100)
    live("5000-spread", [5063, 5000, 5064, 5031, 5032], [1] * 5)
    live("every-bit", list(range(100, 164)) * 2, [1] * 128)
    live("every-bit-1024", rng.permutation(np.resize(np.arange(200, 264), 1024)), [1] * 1024)
    live("spread-2048", rng.randint(1000, 1100, 2048), rng.rand(2048) < 0.5, cap=2048)
    return cases


# ------------------------------------------------------------------ selection across levels and the merge
def select_ref(levels):
    """levels: per level an array [n_i, 4] of (x, y, score, type as a float-typed int32 bit pattern...) given as a
    dict(x, y, score, type). Returns dict(x, y, score, type, level) of n_0 entries and a label per entry."""
    l0 = levels[0]
    n = len(l0["x"])
    x, y, sc = l0["x"].astype(F).copy(), l0["y"].astype(F).copy(), l0["score"].astype(F).copy()
    ty, lv = l0["type"].astype(np.int32).copy(), np.zeros(n, np.int32)
    labels = [[] for _ in range(n)]
    for i in range(1, len(levels)):
        li = levels[i]
        for j in range(n):
            if j >= len(li["x"]):
                labels[j].append("beyond_level_count")          # (the reference would read out of bounds)
                continue
            if ty[j] == KP_FAST and li["type"][j] == KP_EDGELET:
                labels[j].append("fast_beats_edgelet")
                continue
            if ty[j] == li["type"][j] and sc[j] > li["score"][j]:
                labels[j].append("higher_score_stays")
                continue
            if ty[j] == li["type"][j] and sc[j] == li["score"][j]:
                labels[j].append("equal_score_coarser_wins")
            if ty[j] == KP_EDGELET and li["type"][j] == KP_FAST:
                labels[j].append("edgelet_replaced_by_fast")
            if lv[j] > 0:
                labels[j].append("replaced_twice")
            if i == 2 and lv[j] == 1:
                labels[j].append("level2_against_level1")
            labels[j].append("replaced")
            x[j] = F(li["x"][j]) * F(1 << i)
            y[j] = F(li["y"][j]) * F(1 << i)
            sc[j], ty[j], lv[j] = li["score"][j], li["type"][j], i
    for j in range(n):
        if lv[j] == 0:
            labels[j].append("level0_stays")
    return dict(x=x, y=y, score=sc, type=ty, level=lv), labels


def merge_ref(old_xy, cand_xy, image_width, image_height, grid_height, grid_width):
    """merge_keypoints with ITS argument names. Returns the candidates appended, in order (unbounded)."""
    lst = [tuple(p) for p in np.asarray(old_xy, F).reshape(-1, 2)]
    cand = np.asarray(cand_xy, F).reshape(-1, 2)
    picked = []
    for x in range(0, image_width, grid_width):
        left, right = F(x), F(x + grid_width)
        for y in range(0, image_height, grid_height):
            top, bottom = F(y), F(y + grid_height)
            a = np.array(lst, F).reshape(-1, 2)
            match = bool(np.any((a[:, 0] > left) & (a[:, 0] < right) & (a[:, 1] > top) & (a[:, 1] < bottom)))
            if not match:
                for i in np.nonzero((cand[:, 0] > left) & (cand[:, 0] < right) & (cand[:, 1] > top) & (cand[:, 1] < bottom))[0]:
                    lst.append(tuple(cand[i]))
                    picked.append(int(i))
    return picked


def _merge_labels(c, sel, picked):
    gh_arg, gw_arg = c["grid_width"], c["grid_height"]           # merge_keypoints' grid_height, grid_width
    W, Hh = c["width"], c["height"]
    labels = []
    ps = set(picked)
    cells = {}
    for j in range(len(sel["x"])):
        x, y = sel["x"][j], sel["y"][j]
        if not (x > 0 and y > 0):
            labels.append("not_positive")
            continue
        if not (np.isfinite(x) and np.isfinite(y)) or x >= -(-W // gw_arg) * gw_arg or y >= -(-Hh // gh_arg) * gh_arg:
            labels.append("outside_grid")
            continue
        cx, cy = int(x) // gw_arg, int(y) // gh_arg
        if x == cx * gw_arg:
            labels.append("on_border_x")
        elif y == cy * gh_arg:
            labels.append("on_border_y")
        elif j in ps:
            cells.setdefault((cx, cy), []).append(j)
            labels.append("appended")
            if (cx + 1) * gw_arg > W or (cy + 1) * gh_arg > Hh:
                labels.append("in_partial_last_cell")
        else:
            labels.append("cell_occupied")
    if any(len(v) > 1 for v in cells.values()):
        labels.append("shares_cell")
    for x, y in c["old_xy"]:
        if np.isnan(x) or np.isnan(y):
            labels.append("old_nan")
        elif x == F(W):
            labels.append("old_at_width")
        elif y == F(Hh):
            labels.append("old_at_height")
        elif x > 0 and y > 0 and np.isfinite(x) and np.isfinite(y) and (x == int(x) // gw_arg * gw_arg or y == int(y) // gh_arg * gh_arg):
            labels.append("old_on_border")
        else:
            labels.append("old_inside")
    return labels


def merge_expect(c, sel=None, picked=None):
    """arena values after the launch (sel, picked: from the oracle instead of the statements) and the labels"""
    sel_s, sel_labels = select_ref(c["levels"])
    sel = sel_s if sel is None else sel
    n_old, cap = c["kps"]["n"], c["cap"]
    old_xy = f32(c["kps"]["kps2d"][:n_old]).reshape(-1, 2)
    cand = np.stack([sel["x"], sel["y"]], 1) if len(sel["x"]) else np.zeros((0, 2), F)
    if picked is None:
        picked = merge_ref(old_xy, cand, c["width"], c["height"], c["grid_width"], c["grid_height"])
    labels = [l for ll in sel_labels for l in ll] + _merge_labels(dict(c, old_xy=old_xy), sel, picked)
    out = merge_initial(c)
    if c["enable"] == 0:
        return out, ["disabled"]
    kps = copy_set(c["kps"])
    n_new = len(picked)
    for k, j in enumerate(picked):
        if n_old + k >= cap:
            break
        kps["kps2d"][n_old + k] = bits([sel["x"][j], sel["y"][j]])
        kps["score"][n_old + k] = bits([sel["score"][j]])
        kps["level_type"][n_old + k] = U(int(sel["level"][j]) | (int(sel["type"][j]) << 8))
    if n_old + n_new > cap:
        n_new = cap - n_old
        out["overflow"] = np.array([1], np.int32)
        labels.append("overflow")
    elif n_old + n_new == cap and n_new > 0:
        labels.append("exactly_cap")
    labels += (["no_old"] if n_old == 0 else []) + (["old_full"] if n_old == cap else []) + (
        ["nothing_selected"] if len(sel["x"]) == 0 else [])
    kps["n"] = n_old + n_new
    out.update(set_values("kps", kps))
    out["old_count"] = np.array([n_old], np.int32)
    nsel = len(sel["x"])
    s = out["sel"].reshape(-1, 4).copy()
    s[:nsel, 0], s[:nsel, 1], s[:nsel, 2] = bits(sel["x"]), bits(sel["y"]), bits(sel["score"])
    s[:nsel, 3] = sel["type"].astype(np.int32).view(U)
    out["sel"] = s
    sl = out["sel_level"].copy()
    sl[:nsel] = sel["level"].astype(np.int32).view(U)
    out["sel_level"] = sl
    return out, labels


def merge_cells(c):
    """cells of the kernel's merge grid: x cells of grid_height, y cells of grid_width (the swap)"""
    return -(-c["width"] // c["grid_height"]) * -(-c["height"] // c["grid_width"])


def merge_arena(c):
    a = Arena()
    a.add("det", c["n_levels"] * c["max_cells"] * 4)
    a.add("n_det", 8)
    a.add_set("kps", c["cap"])
    a.add("sel", c["max_cells"] * 4)
    a.add("sel_level", c["max_cells"])
    a.add("sel_cell", c["max_cells"])
    a.add("occupied", merge_cells(c))
    a.add("old_count", 1)
    a.add("overflow", 1)
    a.add("enable", 1)
    return a


OVERFLOW_FILL = 0x0F10F10F          # `*overflow` before a launch: the kernel stores 1 on overflow and nothing otherwise
MERGE_SCRATCH = ("sel_cell", "occupied")       # workspaces whose contents after the launch nothing reads


def merge_initial(c):
    mc = c["max_cells"]
    det = np.full((c["n_levels"], mc, 4), 0x7FC00DE7, U)              # (entries beyond a level's count: NaN)
    n_det = np.full(8, 0x00BAD000, U)
    for i, l in enumerate(c["levels"]):
        k = len(l["x"])
        det[i, :k, 0], det[i, :k, 1], det[i, :k, 2] = bits(l["x"]), bits(l["y"]), bits(l["score"])
        det[i, :k, 3] = l["type"].astype(np.int32).view(U)
        n_det[i] = k
    v = set_values("kps", c["kps"])
    v.update(det=det, n_det=n_det, sel=np.full(mc * 4, 0x5E1EC7ED, U), sel_level=np.full(mc, 0x5E1EC7EE, U),
             sel_cell=np.full(mc, 0x5E1EC7EF, U), occupied=np.full(merge_cells(c), 0x0CC0CC0C, U),
             old_count=np.array([0x01DC0DE], U), overflow=np.array([OVERFLOW_FILL], U),      # (written on overflow only)
             enable=np.array([0xFFFFFFFF if c["enable"] is None else c["enable"]], U))
    return v


def merge_threads(max_cells):
    """the rule of launch_select_merge, restated"""
    return 256 if max_cells <= 512 else 1024


def _level(x, y, score, typ):
    return dict(x=np.asarray(x, F), y=np.asarray(y, F), score=np.asarray(score, F), type=np.asarray(typ, np.int32))


def _random_levels(rng, n_levels, counts, w, h, integral=True):
    levels = []
    for i in range(n_levels):
        k = counts[i]
        x, y = rng.uniform(0.2, (w >> i) - 0.2, k), rng.uniform(0.2, (h >> i) - 0.2, k)
        if integral:
            x, y = np.floor(x), np.floor(y)
        sc = rng.randint(0, 6, k) * 17.0            # few values: equal scores are common
        levels.append(_level(x, y, sc, rng.randint(0, 2, k)))
    return levels


def _merge_case(name, levels, old_xy, cap, max_cells, grid_width=9, grid_height=7, width=100, height=76, enable=None, seed=0):
    kps = coded_set(cap, len(old_xy), salt=0x20)
    if len(old_xy):
        kps["kps2d"][:len(old_xy)] = bits(np.asarray(old_xy, F)).reshape(-1, 2)
    assert all(len(l["x"]) <= max_cells for l in levels)
    return dict(name=name, levels=levels, n_levels=len(levels), kps=kps, cap=cap, max_cells=max_cells, grid_width=grid_width,
                grid_height=grid_height, width=width, height=height, enable=enable)


@functools.lru_cache(maxsize=None)
def merge_cases():
    cases = []
    rng = np.random.RandomState(11)
    W, Hh = 100, 76
    # selection: every rule, with counts of the coarser levels below, equal to and above level 0's
    for nl, counts in ((1, (40,)), (2, (40, 40)), (2, (40, 25)), (2, (40, 60)), (3, (40, 40, 40)), (3, (40, 25, 60)),
                       (3, (40, 60, 25)), (3, (30, 0, 30))):
        old = np.stack([rng.uniform(1, W - 1, 10), rng.uniform(1, Hh - 1, 10)], 1).astype(F)
        cases.append(_merge_case(f"select-{nl}-{'-'.join(map(str, counts))}", _random_levels(rng, nl, counts, W, Hh), old, 256, 64))
    # hand-made chains: (type, score) per level for one index each
    T, E = KP_FAST, KP_EDGELET
    chains = [((T, 50), (E, 90), (T, 50)), ((E, 50), (T, 10), (E, 99)), ((T, 50), (T, 50), (T, 50)), ((T, 50), (T, 60), (T, 55)),
              ((T, 50), (T, 40), (T, 50)), ((E, 50), (E, 50), (T, 1)), ((E, 9), (T, 9), (T, 9)), ((T, 9), (E, 9), (E, 200)),
              ((E, 30), (E, 31), (E, 30.5)), ((T, 0), (T, 0), (T, 0)), ((E, 255), (E, 255), (E, 254))]
    lv = []
    for i in range(3):
        lv.append(_level([(3 + 9 * j) >> i for j in range(len(chains))], [(3 + 6 * (j % 9)) >> i for j in range(len(chains))],
                         [ch[i][1] for ch in chains], [ch[i][0] for ch in chains]))
    cases.append(_merge_case("select-chains", lv, np.zeros((0, 2), F), 64, 16))
    cases.append(_merge_case("select-chains-2-levels", lv[:2], np.zeros((0, 2), F), 64, 16))
    # the merge grid: cells of 7 x 9 on 100 x 76 (cam 9 x 7 swapped): borders, zero, halves, the partial last cells
    xs = [0.0, 7.0, 7.5, 3.0, 14.0, 97.0, 98.0, 98.5, 99.5, 104.0, 105.0, 50.0, 51.5, 49.0, -3.0, np.nan, np.inf, 1e30]
    ys = [4.0, 4.0, 0.0, 9.0, 9.5, 30.0, 72.0, 72.5, 75.0, 80.0, 81.0, 18.0, 27.0, 27.5, 5.0, 5.0, 5.0, 5.0]
    cand = _level(xs, ys, np.arange(len(xs)) + 1.0, [j % 2 for j in range(len(xs))])
    cases.append(_merge_case("borders-no-old", [cand], np.zeros((0, 2), F), 64, 32))
    old = np.array([(3.5, 4.5), (7.0, 4.0), (14.5, 9.0), (100.0, 30.0), (50.0, 76.0), (np.nan, 5.0), (5.0, np.nan), (98.5, 73.0),
                    (0.0, 0.0), (-4.0, 5.0), (51.0, 22.0), (np.inf, 3.0), (99.0, 80.5)], F)
    cases.append(_merge_case("borders-old", [cand], old, 64, 32))
    for gw, gh in ((9, 7), (7, 9), (13, 6), (24, 11), (33, 40)):
        lvls = _random_levels(rng, 2, (120, 90), W, Hh, integral=False)
        lvls[0]["x"][::5] = np.floor(lvls[0]["x"][::5] / gh) * gh            # on a border of the merge grid
        lvls[0]["y"][1::5] = np.floor(lvls[0]["y"][1::5] / gw) * gw
        o = np.stack([rng.uniform(-2, W + 4, 40), rng.uniform(-2, Hh + 4, 40)], 1).astype(F)
        o[::4] = np.floor(o[::4])
        o[:3] = [(W, 10), (10, Hh), (np.nan, np.nan)]
        cases.append(_merge_case(f"grid{gw}x{gh}", lvls, o, 512, 128, grid_width=gw, grid_height=gh))
    # two and three candidates in one cell, in index order between candidates of other cells
    cand = _level([8.5, 30.5, 9.5, 8.6, 30.6, 60.5, 9.4, 30.4], [10.5, 40.5, 11.5, 12.5, 41.5, 60.5, 13.0, 42.0],
                  [5, 4, 3, 2, 1, 9, 8, 7], [0, 1, 0, 1, 0, 1, 0, 1])
    cases.append(_merge_case("shared-cells", [cand], np.array([(61.0, 61.0)], F), 64, 8))
    # capacity: n_old of 0, cap - 1, cap; n_old + n_new of cap and cap + 1
    def cap_case(name, cap, n_old, n_cand, max_cells, seed):
        r = np.random.RandomState(seed)
        # old keypoints in the cells of the left half, candidates strictly inside distinct cells of the right half
        o = np.stack([r.uniform(0.5, 48.5, n_old), r.uniform(0.5, 75.5, n_old)], 1).astype(F)
        cx, cy = np.meshgrid(np.arange(8, 14), np.arange(0, 8))
        cells = np.stack([cx.ravel(), cy.ravel()], 1)[r.permutation(48)]
        cells = np.resize(cells, (n_cand, 2))
        x = cells[:, 0] * 7 + r.randint(1, 7, n_cand) * 1.0
        y = cells[:, 1] * 9 + r.randint(1, 9, n_cand) * 1.0
        return _merge_case(name, [_level(x, y, r.randint(1, 200, n_cand), r.randint(0, 2, n_cand))], o, cap, max_cells)
    cases.append(cap_case("cap-old0", 64, 0, 30, 32, 1))
    cases.append(cap_case("cap-old-cap-1", 64, 63, 30, 32, 2))
    cases.append(cap_case("cap-old-cap", 64, 64, 30, 32, 3))
    cases.append(cap_case("cap-exact", 64, 34, 30, 32, 4))
    cases.append(cap_case("cap-plus-1", 64, 35, 30, 32, 5))
    cases.append(cap_case("cap-exact-1024", 1024, 1024 - 300, 300, 512, 6))
    cases.append(cap_case("cap-plus-1-1024", 1024, 1024 - 299, 300, 512, 7))
    cases.append(cap_case("cap-plus-many-2048", 2048, 2000, 1025, 1025, 8))
    # nsel around the thread counts of both launch shapes
    for nsel, mc in ((0, 256), (255, 256), (256, 256), (257, 512), (512, 512), (513, 513), (1025, 1025), (1025, 2000)):
        lvls = _random_levels(rng, 2, (nsel, max(nsel - 3, 0)), W, Hh)
        lvls[0]["x"] += F(0.5)
        o = np.stack([rng.uniform(1, W - 1, 20), rng.uniform(1, Hh - 1, 20)], 1).astype(F)
        cases.append(_merge_case(f"nsel{nsel}-mc{mc}", lvls, o, 2048, mc))
    cases.append(_merge_case("disabled", _random_levels(rng, 2, (50, 50), W, Hh), np.zeros((0, 2), F), 256, 64, enable=0))
    cases.append(_merge_case("enabled-0x100", _random_levels(rng, 2, (50, 50), W, Hh), np.zeros((0, 2), F), 256, 64, enable=0x100))
    return cases


# ------------------------------------------------------------------ initialisation of a keyframe's new keypoints
def lcg_next(st):
    return (st * 1664525 + 1013904223) & 0xFFFFFFFF


def backup_ref(flags):
    """(flags afterwards, label): stereo_slam.cpp:237-245 on the flag words"""
    flags = np.asarray(flags, U).copy()
    cnt = 0
    for f in flags:
        if not (int(f) & IGNORE_TEMPORARY):
            cnt += 1
    if cnt < len(flags) // 4:
        return flags & ~U(IGNORE_TEMPORARY), "backup_cleared"
    return flags, "backup_kept"


def init_ref(c, T=F):
    """dict(kps = the frame's set afterwards, record = the keyframe's copy, record_n, record_pose, lcg, n_out), labels;
    with T = np.float64 the float planes of the new keypoints are returned as float64 arrays under 'twin'"""
    cam = {k: T(F(c["cam"][k])) for k in ("fx", "fy", "cx", "cy", "baseline")}
    kps = copy_set(c["kps"])
    n, old = kps["n"], c["old_count"]
    labels = ["first_frame"] if c["first_frame"] else []
    labels += (["no_new"] if old == n else []) + (["all_new"] if old == 0 and n > 0 else [])
    pose = np.zeros(6, F) if c["first_frame"] else np.asarray(c["frame_pose"], F)
    R = GC.pose_mats(pose.astype(T), T)[0]
    st = LCG_SEED if c["first_frame"] else c["lcg"]
    twin = dict(kps3d=np.zeros((n, 3), D), kfx=np.zeros(n, D), kfP=np.zeros(n, D))
    half = T(0.5)
    for i in range(old, n):
        x, y = (T(v) for v in f32(kps["kps2d"][i]))
        d = T(f32(c["disparity"][i:i + 1])[0])
        labels.append("disparity_nan" if np.isnan(d) else "disparity_inf" if np.isinf(d) else "disparity_half" if d == half
                      else "disparity_above_half" if d > half else "disparity_clamped")
        with np.errstate(all="ignore"):
            m = d if half < d else half               # std::max<float>(0.5, d)
            _z = cam["baseline"] / m
            _x = (x - cam["cx"]) / cam["fx"] * _z
            _y = (y - cam["cy"]) / cam["fy"] * _z
            g = GC._matvec(R, [_x, _y, _z])
            p3 = [g[k] + T(pose[k]) for k in range(3)]
            deviation = T(F(D(0.5) / D(cam["baseline"] / cam["fx"]))) if T is F else D(0.5) / (cam["baseline"] / cam["fx"])
            kfP = deviation * deviation
            kfx = T(1) / _z
        st = lcg_next(st)
        if T is F:
            kps["kps3d"][i] = bits(np.array(p3, F))
            kps["kf_variance"][i] = bits([kfP])
            kps["kf_inv_depth"][i] = bits([kfx])
        else:
            twin["kps3d"][i], twin["kfx"][i], twin["kfP"][i] = p3, kfx, kfP
        kps["color"][i] = U((st >> 8) & 0xFFFFFF)
        kps["kf_id"][i] = np.int32(c["new_kf_id"]).view(U)
        kps["kp_index"][i] = U(i)
        kps["flags"][i] = U(IGNORE_TEMPORARY)
        kps["inlier_count"][i] = 0
        kps["outlier_count"][i] = 0
    record = {name: kps[name][:n].copy() for name in PLANE_NAMES}
    if c["first_frame"]:
        kps["flags"][:n] &= ~U(IGNORE_TEMPORARY)
    else:
        fl, lab = backup_ref(kps["flags"][:n, 0])
        kps["flags"][:n, 0] = fl
        labels.append(lab)
    labels.append("evicts" if c["evict_id"] >= 0 else "no_evict")
    out = dict(kps=kps, record=record, record_n=n, record_pose=pose, lcg=st, n_out=n)
    if T is not F:
        out["twin"] = twin
    return out, labels


def init_arena(c):
    a = Arena()
    a.add_set("kps", c["cap"])
    a.add_set("record", c["cap"])
    a.add("old_count", 1)
    a.add("disparity", c["cap"])
    a.add("frame_pose", 6)
    a.add("lcg", 1)
    a.add("n_out", 1)
    a.add("tmpl_valid", c["tmpl_valid_bytes"] // 4)
    a.add("enable", 1)
    return a


def init_initial(c):
    v = set_values("kps", c["kps"])
    rec = coded_set(c["cap"], 0x0EC0EC0, salt=0x60)
    v.update(set_values("record", rec))
    v.update(old_count=np.array([c["old_count"]], np.int32), disparity=c["disparity"], frame_pose=bits(c["frame_pose"]),
             lcg=np.array([c["lcg"]], U), n_out=np.array([0x0BAD0BAD], U),
             tmpl_valid=np.full(c["tmpl_valid_bytes"] // 4, 0x01010101, U),
             enable=np.array([0xFFFFFFFF if c["enable"] is None else c["enable"]], U))
    return v


def init_expect(c, ref=None):
    """arena values after the launch; ref: init_ref's result (or the oracle's in the same form)"""
    out = init_initial(c)
    if c["enable"] == 0:
        return out
    ref = init_ref(c)[0] if ref is None else ref
    out.update(set_values("kps", ref["kps"]))
    n = ref["record_n"]
    for name in PLANE_NAMES:
        r = out[f"record.{name}"].copy()
        r[:n] = ref["record"][name]
        out[f"record.{name}"] = r
    out["lcg"] = np.array([ref["lcg"]], U)
    out["n_out"] = np.array([ref["n_out"]], np.int32)
    out["tmpl_valid"] = np.zeros(c["tmpl_valid_bytes"] // 4, U)
    return out


INIT_CAMS = {"euroc": GC.CAMERAS["euroc"], "pow2": GC.CAMERAS["pow2"],
             "fxfy": dict(GC.CAMERAS["euroc"], fx=431.25, fy=470.5, cx=301.75, cy=255.125, baseline=41.0625)}
INIT_POSES = {"zero": (0, 0, 0, 0, 0, 0), "1rad": (12.5, -3.25, 40.0, 0.6, -0.64, 0.48),
              "small": (0.1, 0.2, -0.3, 0.01, -0.02, 0.03), "nan": (np.nan,) * 6}


def _init_case(name, n, old_count, rng, cap=None, cam="euroc", pose="1rad", first_frame=0, not_temp=None, new_kf_id=13,
               kf_mask=7, evict_id=-1, lcg=0xC0FFEE11, tmpl_valid_bytes=260, enable=None):
    cap = cap or max(8, n + 3)
    kps = coded_set(cap, n, salt=0x30)
    kps["kps2d"] = bits(np.stack([rng.uniform(0, 752, cap), rng.uniform(0, 480, cap)], 1).astype(F)).reshape(cap, 2).copy()
    fl = (rng.randint(0, 1 << 28, cap).astype(U) << U(3)) | U(IGNORE_TEMPORARY) | rng.randint(0, 4, cap).astype(U)
    if not_temp is not None:                       # exactly that many old keypoints without the temporary bit
        assert not_temp <= old_count
        fl[rng.permutation(old_count)[:not_temp]] &= ~U(IGNORE_TEMPORARY)
    else:
        fl[:old_count] &= ~(rng.randint(0, 2, old_count).astype(U) * U(IGNORE_TEMPORARY))
    kps["flags"] = fl.reshape(cap, 1)
    special = np.array([-1.0, 0.0, 0.5, np.nextafter(F(0.5), F(0)), np.nextafter(F(0.5), F(1)), 64.0, np.inf, np.nan], F)
    disp = rng.uniform(0.2, 64, cap).astype(F)
    k = min(len(special), n - old_count)
    if k > 0:
        disp[old_count:old_count + k] = special[:k]
    return dict(name=name, cap=cap, kps=kps, old_count=old_count, disparity=bits(disp), cam=INIT_CAMS[cam],
                frame_pose=np.array(INIT_POSES[pose], F), first_frame=first_frame, new_kf_id=new_kf_id, kf_mask=kf_mask,
                evict_id=evict_id, lcg=lcg, tmpl_valid_bytes=tmpl_valid_bytes, enable=enable)


@functools.lru_cache(maxsize=None)
def init_cases():
    cases = []
    rng = np.random.RandomState(13)
    for n in (0, 1, 3, 7, 8, 255, 256, 257, 1030):
        for old in sorted({0, max(n - 1, 0), n}):
            cases.append(_init_case(f"n{n}-old{old}", n, old, rng))
    for cam in INIT_CAMS:
        for pose in ("zero", "1rad", "small"):
            cases.append(_init_case(f"{cam}-{pose}", 40, 9, rng, cam=cam, pose=pose))
    cases.append(_init_case("first-frame-nan-pose", 70, 0, rng, cam="fxfy", pose="nan", first_frame=1))
    cases.append(_init_case("first-frame-old-kept", 70, 20, rng, pose="nan", first_frame=1, not_temp=0))
    cases.append(_init_case("first-frame-empty", 0, 0, rng, pose="nan", first_frame=1))
    for n, nt, in ((8, 1), (8, 2), (7, 0), (7, 1), (3, 0), (4, 0), (4, 1), (1030, 256), (1030, 257), (1030, 258)):
        cases.append(_init_case(f"backup-{n}-{nt}", n, min(n, max(nt, n - 1 if n < 100 else 600)), rng, not_temp=nt))
    cases.append(_init_case("ring-13-evict-none", 20, 5, rng, new_kf_id=13, kf_mask=7, evict_id=-1))
    cases.append(_init_case("ring-13-evict-9", 20, 5, rng, new_kf_id=13, kf_mask=7, evict_id=9))
    # its own slot: the tracker never asks for this (an evicted keyframe is still resident, so it lies in another
    # slot); kept as a record of what the kernel does then: the new record ends without a template block
    cases.append(_init_case("ring-13-evict-5", 20, 5, rng, new_kf_id=13, kf_mask=7, evict_id=5))
    cases.append(_init_case("ring-0-mask-0", 20, 5, rng, new_kf_id=0, kf_mask=0))
    cases.append(_init_case("ring-4100", 20, 5, rng, new_kf_id=4100, kf_mask=63, evict_id=4092))
    for vb in (0, 4, 256, 1028, 4096):
        cases.append(_init_case(f"valid-{vb}", 12, 3, rng, tmpl_valid_bytes=vb))
    cases.append(_init_case("disabled", 30, 4, rng, enable=0, evict_id=9))
    cases.append(_init_case("enabled-0x100", 30, 4, rng, enable=0x100))
    cases.append(_init_case("lcg-wraps", 300, 0, rng, lcg=0xFFFFFFFF))
    return cases


# ------------------------------------------------------------------ the tracker's form of the SSD launch
DISPARITY_FILL = 0x7FC5D15F         # a NaN with a payload: what entries that the launch does not write keep


def ssd_launch_ref(per_keypoint, first, n, n_bound, cap):
    """`disparity` [cap] as words after a launch of grid x = n_bound that starts at keypoint `first`"""
    out = np.full(cap, DISPARITY_FILL, U)
    hi = min(n, first + n_bound)
    if first < hi:
        out[first:hi] = bits(per_keypoint[first:hi])
    return out


def ssd_pick_max_win(win, search_y):
    """the rule of launch_ssd, restated"""
    return 31 if win <= 31 and 2 * search_y + 1 <= 13 else 35


def ssd_offsets(n):
    """(first, *first_ptr) pairs whose sums are 0, 1, n - 1, n and n + 3, both parts non-zero where the sum allows"""
    out = [(0, 0)]
    for total in (1, n - 1, n, n + 3):
        if total < 1:
            continue
        a = max(total // 3, 1) if total > 1 else 1
        out.append((a, total - a))
        out.append((0, total))
    return out
