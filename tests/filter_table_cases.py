"""The depth filter launch in the form the tracker makes it (csrc/depth.hip with FilterArgs::kfs set,
svo_filter_update_table_batch): its plain statement and the sequences of tests/test_filter_table_cpu.py and
tests/test_filter_table_gpu.py.

Nothing here calls the HIP library. numpy only. The per-point arithmetic is that of tests/geometry_cases.py
(outlier_ref, update_ref, writeback_ref, project_ref), which tests/test_geometry_cpu.py holds to the oracle and to its
float64 twin; what is stated here is what the tracker form adds, written from the reference's source:

  the gather      DepthFilter::update_depth, src/lib/depth_filter.cpp:40-50, and the loop of StereoSlam::new_image,
                  src/lib/stereo_slam.cpp:196-204: keypoint i belongs to keyframe info.keyframe_id, point
                  info.keypoint_index; the keyframe's pose and that point's kps3d (outlier_check's reference) and
                  kps2d (update_kps3d's) are read, while update_kps3d starts from the FRAME's kps3d
  the scatter     stereo_slam.cpp:205-229: the frame's kps3d, ignore_temporary, ignore_completely and the two counters
                  go into the keyframe's entry; its ignore_during_refinement is the keyframe's own and stays
  the counter     KeyFrameManager::keyframe_needed, src/lib/keyframe_manager.cpp:55-64; the kernel ADDS it to a word

The kernel finds the keyframe's record at kf_id & kf_mask of a table: a ring of kf_mask + 1 records over the ids (the
tracker's), or, with kf_mask -1, the id as it is (the reference's vector).

A SEQUENCE is a dict: name, cam, width, height, frame_pose, n, cap, kf_mask, inside0 (the counter's value before the
launch), `frame` (dict of arrays of `cap` entries: FRAME_KEYS; entries from n on are a pattern that must come back
untouched), `table` (one dict of TABLE_KEYS per record; a vacant record of a ring has arrays of no entries),
`explicit` (the gathered per-point references, a case in the form of geometry_cases.filter_cases) and `reaches` (the
situations of SITUATIONS the sequence is there for, derived from its arrays).
"""
import functools

import numpy as np

import geometry_cases as GC

F = np.float32
DURING, COMPLETELY, TEMPORARY = GC.IGNORE_DURING_REFINEMENT, GC.IGNORE_COMPLETELY, GC.IGNORE_TEMPORARY
FRAME_KEYS = ("kps2d", "kps3d", "flags", "outlier", "inlier", "kf_inv_depth", "kf_variance", "disparity", "kf_id", "kp_index")
FRAME_OUT = ("kps2d", "kps3d", "flags", "outlier", "inlier", "kf_inv_depth", "kf_variance")
TABLE_KEYS = ("pose", "kps2d", "kps3d", "flags", "outlier", "inlier")
SLAB_KEYS = TABLE_KEYS[1:]
DTYPES = dict(kps2d=F, kps3d=F, flags=np.uint32, outlier=np.int32, inlier=np.int32, kf_inv_depth=F, kf_variance=F,
              disparity=F, kf_id=np.int32, kp_index=np.int32, pose=F)
WIDTHS = dict(kps2d=2, kps3d=3)
ALL_SWITCHES = tuple((a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1))
SITUATIONS = ("ring", "wrap", "ids_as_they_are", "one_keyframe", "interleave", "slab_lengths_differ", "poses_differ",
              "keep_bit_keyframe_only", "keep_bit_frame_only", "temporary_differs", "completely_differs",
              "counter_disagreement", "kps3d_disagreement", "unreferenced_point", "unreferenced_keyframe", "vacant_record",
              "index_reversed", "index_strided", "index_sparse", "tail_beyond_n", "two_workgroups", "empty",
              "nothing_inside", "counter_starts_nonzero")
# poses of the keyframes of the layout sequences: every record its own
TABLE_POSES = ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.01, 0.0, 0.0, 0.001, 0.0, 0.0), (-0.3, 0.2, 0.1, 0.02, -0.03, 0.01),
               (0.25, -0.15, 0.05, -0.01, 0.02, 0.03))


# ------------------------------------------------------------------ the statement
def gather(seq):
    """the explicit per-point references of a sequence, read from its table: (record of every keypoint, ref3d,
    ref2d, kf_pose)"""
    n, fr, tb = seq["n"], seq["frame"], seq["table"]
    rec = [int(fr["kf_id"][i]) & seq["kf_mask"] for i in range(n)]
    idx = [int(k) for k in fr["kp_index"][:n]]
    ref3d = np.array([tb[r]["kps3d"][k] for r, k in zip(rec, idx)], F).reshape(n, 3)
    ref2d = np.array([tb[r]["kps2d"][k] for r, k in zip(rec, idx)], F).reshape(n, 2)
    kf_pose = np.array([tb[r]["pose"] for r in rec], F).reshape(n, 6)
    return rec, idx, ref3d, ref2d, kf_pose


def table_filter_ref(seq, switches=(1, 1, 1, 1)):
    """dict(frame, table, inside, labels, kp_labels): the frame's arrays (all `cap` entries), every record of the
    table, the counter's word after the launch, and the labels of geometry_cases' statements that the switches let
    the launch reach. Gather everything, run the per-point statements, scatter."""
    do_oc, do_up, do_flags, do_reproject = switches
    n, cam = seq["n"], seq["cam"]
    frame = {k: np.array(v) for k, v in seq["frame"].items()}
    table = [{k: np.array(v) for k, v in r.items()} for r in seq["table"]]
    if n == 0:
        return dict(frame=frame, table=table, inside=seq["inside0"], labels=set(), kp_labels=([], [], []))
    rec, idx, ref3d, ref2d, kf_pose = gather(seq)
    k2, k3, fl = frame["kps2d"][:n], frame["kps3d"][:n], frame["flags"][:n]
    outl, inl, kx, kP = frame["outlier"][:n], frame["inlier"][:n], frame["kf_inv_depth"][:n], frame["kf_variance"][:n]
    lo, lu = [set() for _ in range(n)], [set() for _ in range(n)]
    if do_oc:
        outl, inl, lo = GC.outlier_ref(k2, frame["disparity"][:n], cam, seq["frame_pose"], ref3d, kf_pose, outl, inl)
    if do_up:
        k3, outl, kx, kP, lu = GC.update_ref(k2, k3, fl, cam, seq["frame_pose"], ref2d, kf_pose, outl, kx, kP)
    if do_flags:
        fl, proj, inside, lw = GC.writeback_ref(fl, outl, inl, k3, cam, seq["frame_pose"], seq["width"], seq["height"])
        for i, (r, k) in enumerate(zip(rec, idx)):
            kf = table[r]
            kf["kps3d"][k] = k3[i]
            kf["flags"][k] = (kf["flags"][k] & DURING) | (fl[i] & (TEMPORARY | COMPLETELY))
            kf["inlier"][k], kf["outlier"][k] = inl[i], outl[i]
    else:       # equal counters change no flag: the projection and the counter on the flags as they are
        zero = np.zeros(n, np.int32)
        fl, proj, inside, lw = GC.writeback_ref(fl, zero, zero, k3, cam, seq["frame_pose"], seq["width"], seq["height"])
        assert np.array_equal(fl, frame["flags"][:n])
    flag_labels = {"flag_set_completely", "temporary_cleared", "counts_equal"}
    lw = [(l & flag_labels if do_flags else set()) | (l - flag_labels if do_reproject else set()) for l in lw]
    frame["kps3d"][:n], frame["flags"][:n], frame["outlier"][:n], frame["inlier"][:n] = k3, fl, outl, inl
    frame["kf_inv_depth"][:n], frame["kf_variance"][:n] = kx, kP
    if do_reproject:
        frame["kps2d"][:n] = proj
    return dict(frame=frame, table=table, inside=seq["inside0"] + (inside if do_reproject else 0),
                labels=GC.all_labels(lo, lu, lw), kp_labels=(lo, lu, lw))


def explicit_ref(seq, switches):
    """the frame outputs of the explicit-form statement (geometry_cases.filter_ref) on the gathered references"""
    return GC.filter_ref(seq["explicit"], F, switches[0], switches[1])


# ------------------------------------------------------------------ builders
def _cut(c, n, **over):
    """the first n keypoints of an explicit case"""
    out = dict(c)
    for k in ("kps2d", "kps3d", "flags", "disparity", "ref3d", "ref2d", "kf_pose", "outlier", "inlier", "kf_inv_depth",
              "kf_variance"):
        out[k] = c[k][:n].copy()
    for k, v in over.items():
        out[k][:] = v
    return out


def _base(name, n, seed, poses, cam="euroc", **over):
    """an explicit case of n keypoints whose keyframe poses are drawn from `poses`"""
    return _cut(GC._filter_case(name, cam=cam, n=max(n, 4), seed=seed, kf_poses=poses), n, **over)


def _tail(key, j, width):
    """entry j behind a frame array's n: a pattern per array that no result can equal"""
    if DTYPES[key] is F:
        return [F(-7000.5 - 8 * j - c) for c in range(width)] if width > 1 else F(-7000.5 - 8 * j)
    return DTYPES[key](0x5A5A0000 + j)


def make_sequence(name, c, ids=None, kf_mask=-1, table=None, index="reversed", poses=None, extra=7, inside0=1000,
                  disagree=True, seed=0):
    """scatter the per-point references of the explicit case c (ref3d, ref2d, kf_pose) into a keyframe table.
    poses: the keyframes (default: the distinct poses of c in order of appearance); ids: their ids (default 0, 1,
    ..); table: the number of records (default: what the ids need); index: how a keyframe's points are named.
    The frame's own arrays are c's, untouched, so every label of c is reached again; with `disagree` the keyframe's
    copies of flags and counters differ from the frame's."""
    rng = np.random.RandomState(4000 + seed)
    n = len(c["flags"])
    kf_pose = np.asarray(c["kf_pose"], F).reshape(n, 6)
    if poses is None:
        poses = []
        for p in kf_pose:
            if not any(p.tobytes() == q.tobytes() for q in poses):
                poses.append(p.copy())
    poses = [np.asarray(p, F) for p in poses]
    assert len({p.tobytes() for p in poses}) == len(poses) >= 1
    ids = list(range(len(poses))) if ids is None else list(ids)
    assert len(ids) == len(poses) and min(ids) >= 0
    if table is None:
        table = max(ids) + 1 if kf_mask == -1 else kf_mask + 1
    assert kf_mask == -1 or (table == kf_mask + 1 and table & kf_mask == 0)
    slot_of = [i & kf_mask for i in ids]
    assert len(set(slot_of)) == len(ids) and max(slot_of) < table, "two resident keyframes in one record"
    group = np.array([[p.tobytes() for p in poses].index(q.tobytes()) for q in kf_pose], np.int64).reshape(n)

    records = [dict(pose=np.zeros(6, F), kps2d=np.zeros((0, 2), F), kps3d=np.zeros((0, 3), F), flags=np.zeros(0, np.uint32),
                    outlier=np.zeros(0, np.int32), inlier=np.zeros(0, np.int32)) for _ in range(table)]
    kf_id, kp_index = np.zeros(n, np.int32), np.zeros(n, np.int32)
    free_point = []                                                  # per keyframe: an index no keypoint names
    for g, (kid, slot) in enumerate(zip(ids, slot_of)):
        members = np.nonzero(group == g)[0]
        m = len(members)
        if index == "reversed":
            length = m + 2 + g
            where = length - 1 - np.arange(m)
        elif index == "strided":
            length = 2 * m + 2 + g
            where = 1 + 2 * np.arange(m)
        else:
            assert index == "sparse"
            length = 3 * m + 5 + 2 * g
            where = rng.permutation(length)[:m]
        unused = sorted(set(range(length)) - set(int(w) for w in where))
        free_point.append(unused[len(unused) // 2])
        r = records[slot]
        r["pose"] = poses[g].copy()
        r["kps2d"] = rng.uniform(5, 400, (length, 2)).astype(F)
        r["kps3d"] = rng.uniform(-3, 9, (length, 3)).astype(F)
        r["flags"] = rng.randint(0, 8, length).astype(np.uint32)
        r["outlier"] = rng.randint(0, 50, length).astype(np.int32)
        r["inlier"] = rng.randint(0, 50, length).astype(np.int32)
        for j, i in enumerate(members):
            k = int(where[j])
            kf_id[i], kp_index[i] = kid, k
            r["kps2d"][k], r["kps3d"][k] = c["ref2d"][i], c["ref3d"][i]
            if disagree:
                # the three bits each in all four (keyframe, frame) combinations, and counters the frame does not have
                r["flags"][k] = np.uint32((int(c["flags"][i]) + 1 + (i % 7)) & 7)
                r["outlier"][k], r["inlier"][k] = c["outlier"][i] + 3 + i % 5, c["inlier"][i] + 11 + i % 3
            else:
                r["flags"][k], r["outlier"][k], r["inlier"][k] = c["flags"][i], c["outlier"][i], c["inlier"][i]
    pairs = {(int(a) & kf_mask, int(b)) for a, b in zip(kf_id, kp_index)}
    assert len(pairs) == n, "(keyframe, keypoint_index) pairs are unique within a sequence, as in the reference"

    cap = n + extra
    frame = {}
    for key in FRAME_KEYS:
        w = WIDTHS.get(key, 1)
        a = np.zeros((cap, w) if w > 1 else cap, DTYPES[key])
        for j in range(n, cap):
            a[j] = _tail(key, j, w)
        frame[key] = a
    # (a lane beyond n that ran would name a real, unreferenced keyframe point: the slabs would show it)
    frame["kf_id"][n:], frame["kp_index"][n:] = ids[0], free_point[0]
    for key, src in (("kps2d", "kps2d"), ("kps3d", "kps3d"), ("flags", "flags"), ("outlier", "outlier"), ("inlier", "inlier"),
                     ("kf_inv_depth", "kf_inv_depth"), ("kf_variance", "kf_variance"), ("disparity", "disparity")):
        frame[key][:n] = c[src]
    frame["kf_id"][:n], frame["kp_index"][:n] = kf_id, kp_index
    seq = dict(name=name, cam=c["cam"], width=c["width"], height=c["height"], frame_pose=np.asarray(c["frame_pose"], F),
               n=n, cap=cap, kf_mask=kf_mask, inside0=inside0, frame=frame, table=records, ids=ids, index=index,
               explicit=c)
    seq["reaches"] = situations(seq)
    return seq


def situations(seq):
    """which of SITUATIONS a sequence reaches, from its arrays alone"""
    n, fr, tb, mask, ids = seq["n"], seq["frame"], seq["table"], seq["kf_mask"], seq["ids"]
    out = set()
    rec, idx, ref3d, _, kf_pose = gather(seq)
    used = sorted(set(rec))
    if mask != -1:
        out.add("ring")
        if len({i // (mask + 1) for i in ids}) > 1:
            out.add("wrap")                                          # a younger keyframe sits in a lower record
    elif len(tb) > 1:
        out.add("ids_as_they_are")
    if len(ids) == 1:
        out.add("one_keyframe")
    if len(used) >= 3 and any(a > b for a, b in zip(fr["kf_id"][:max(n - 1, 0)], fr["kf_id"][1:n])):
        out.add("interleave")
    if len({len(tb[i & mask]["flags"]) for i in ids}) > 1:
        out.add("slab_lengths_differ")
    if len({kf_pose[i].tobytes() for i in range(n)}) > 1:
        out.add("poses_differ")
    kf_fl = np.array([tb[r]["flags"][k] for r, k in zip(rec, idx)], np.uint32)
    f_fl = fr["flags"][:n]
    if np.any((kf_fl & DURING != 0) & (f_fl & DURING == 0)):
        out.add("keep_bit_keyframe_only")
    if np.any((kf_fl & DURING == 0) & (f_fl & DURING != 0)):
        out.add("keep_bit_frame_only")
    if np.any((kf_fl ^ f_fl) & TEMPORARY):
        out.add("temporary_differs")
    if np.any((kf_fl ^ f_fl) & COMPLETELY):
        out.add("completely_differs")
    if any(tb[r]["outlier"][k] != fr["outlier"][i] and tb[r]["inlier"][k] != fr["inlier"][i]
           for i, (r, k) in enumerate(zip(rec, idx))):
        out.add("counter_disagreement")
    if n and np.any(~GC.same_bits(ref3d, fr["kps3d"][:n])):
        out.add("kps3d_disagreement")
    named = {(r, k) for r, k in zip(rec, idx)}
    if any((i & mask, k) not in named for i in ids for k in range(len(tb[i & mask]["flags"]))):
        out.add("unreferenced_point")
    if any((i & mask) not in used for i in ids):
        out.add("unreferenced_keyframe")
    if any(len(r["flags"]) == 0 for r in tb):
        out.add("vacant_record")
    if n:
        out.add("index_" + seq["index"])
    if seq["cap"] > n:
        out.add("tail_beyond_n")
    if n > 64:
        out.add("two_workgroups")
    if n == 0:
        out.add("empty")
    if seq["inside0"] != 0:
        out.add("counter_starts_nonzero")
    return out


# ------------------------------------------------------------------ the sequences
# how a table is made for the layout sequences: (ids, kf_mask, records)
TABLES = {
    "one": ((0,), -1, 1),
    "three": ((0, 1, 2), -1, 3),                 # ids as they are, in a table that is no power of two
    "ring_567": ((5, 6, 7), 3, 4),               # a ring of 4 records: record 0 is vacant
    "ring_6789": ((6, 7, 8, 9), 3, 4),           # it wraps: ids 8 and 9 sit in records 0 and 1, below 6 and 7
    "plain_0_2_3": ((0, 2, 3), -1, 4),           # kf_mask -1, ids used as they are, record 1 vacant
}
# (keypoints, table, how kp_index names a keyframe's points)
LAYOUTS = ((0, "one", "reversed"), (0, "ring_6789", "sparse"), (1, "ring_567", "sparse"), (63, "three", "strided"),
           (64, "ring_6789", "reversed"), (65, "plain_0_2_3", "sparse"), (128, "ring_567", "strided"),
           (130, "ring_6789", "sparse"), (130, "three", "reversed"), (130, "one", "strided"), (64, "plain_0_2_3", "strided"))
COUNTS = (0, 1, 63, 64, 65, 128, 130)


@functools.lru_cache(maxsize=None)
def layout_sequences():
    out = []
    for k, (n, tname, index) in enumerate(LAYOUTS):
        ids, mask, records = TABLES[tname]
        c = _base(f"n{n}_{tname}", n, 100 + k, TABLE_POSES[:len(ids)])
        out.append(make_sequence(f"n{n}_{tname}_{index}", c, ids=ids, kf_mask=mask, table=records, index=index,
                                 poses=TABLE_POSES[:len(ids)], extra=5 + k, inside0=1000 + 37 * k, seed=k))
    # nothing projects inside: every keypoint is ignored (the update leaves its point alone) and sits far off axis
    c = _base("nothing_inside", 70, 150, TABLE_POSES[:3], flags=COMPLETELY, kps3d=(50.0, 50.0, 1.0))
    out.append(make_sequence("nothing_inside", c, ids=(5, 6, 7), kf_mask=3, poses=TABLE_POSES[:3], index="sparse",
                             inside0=4242, seed=50))
    # a second ring whose resident ids sit in other records than ring_567's and ring_6789's do
    c = _base("ring_12_13", 40, 151, TABLE_POSES[2:4])
    out.append(make_sequence("ring_12_13", c, ids=(12, 13), kf_mask=3, poses=TABLE_POSES[2:4], index="reversed",
                             inside0=7, seed=51))
    c = _base("ring8_11_12_14_17", 50, 152, TABLE_POSES)
    out.append(make_sequence("ring8_11_12_14_17", c, ids=(11, 12, 14, 17), kf_mask=7, poses=TABLE_POSES, index="strided",
                             inside0=0, seed=52))
    assert {s["n"] for s in out} >= set(COUNTS)
    return out


@functools.lru_cache(maxsize=None)
def carried_sequences():
    """every labelled case of geometry_cases.filter_cases, its references scattered into a table of one record per
    distinct keyframe pose (ids as they are)"""
    out = []
    for k, c in enumerate(GC.filter_cases()):
        index = ("reversed", "strided", "sparse")[k % 3]
        out.append(make_sequence("carried_" + c["name"], c, index=index, extra=3 + k % 4, inside0=500 + k, seed=200 + k))
    return out


@functools.lru_cache(maxsize=None)
def switch_sequence():
    """the small sequence that all 16 switch combinations run on"""
    c = _base("switches", 24, 160, TABLE_POSES[:3])
    c["flags"][:] = np.arange(24) % 8                               # every flag combination, counters on both sides
    c["outlier"][:], c["inlier"][:] = (np.arange(24) // 8) % 3, 1
    return make_sequence("switches", c, ids=(5, 6, 7), kf_mask=3, poses=TABLE_POSES[:3], index="sparse", inside0=321, seed=60)


@functools.lru_cache(maxsize=None)
def sequences():
    out = layout_sequences() + carried_sequences() + [switch_sequence()]
    assert len({s["name"] for s in out}) == len(out)
    return out


def sequence(name):
    return [s for s in sequences() if s["name"] == name][0]


def reached(seq):
    """the situations of a sequence: those its arrays show, and `nothing_inside` from its statement"""
    quiet = seq["n"] > 0 and results()[seq["name"]]["inside"] == seq["inside0"]
    return seq["reaches"] | ({"nothing_inside"} if quiet else set())


# launches of several sequences: different counts (one of them 0), every sequence its own table; and rings with
# different resident ids side by side. One camera per batch is not required: every sequence has its own.
BATCHES = {
    "counts": ("n130_ring_6789_sparse", "n0_one_reversed", "n1_ring_567_sparse", "n65_plain_0_2_3_sparse",
               "n63_three_strided", "nothing_inside", "n64_ring_6789_reversed", "carried_border"),
    "rings": ("n128_ring_567_strided", "n130_ring_6789_sparse", "ring_12_13", "ring8_11_12_14_17", "n0_ring_6789_sparse",
              "switches"),
}


@functools.lru_cache(maxsize=None)
def results():
    """name -> table_filter_ref with every switch on"""
    return {s["name"]: table_filter_ref(s) for s in sequences()}


@functools.lru_cache(maxsize=None)
def switch_results():
    """switches -> table_filter_ref of switch_sequence()"""
    return {sw: table_filter_ref(switch_sequence(), sw) for sw in ALL_SWITCHES}
