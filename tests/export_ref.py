"""The bulk export of the tracker state (svo_submit_export, svo_pack_keypoints) restated in numpy: the svo_kp_info
record built from the SoA planes, the placement rule of the segments, and the segment layout. Written from
include/svo_hip.h and include/svo_types.h alone; the tests compare the library with it byte for byte."""
import numpy as np

# svo_kp_info, field by field: (name, byte offset, numpy type, count)
INFO_FIELDS = (("score", 0, "<f4", 1), ("level", 4, "<i4", 1), ("type", 8, "<i4", 1), ("keyframe_id", 12, "<i4", 1),
               ("keypoint_index", 16, "<i4", 1), ("color", 20, "u1", 3), ("ignore_during_refinement", 23, "u1", 1),
               ("ignore_completely", 24, "u1", 1), ("ignore_temporary", 25, "u1", 1), ("_pad", 26, "u1", 2),
               ("outlier_count", 28, "<i4", 1), ("inlier_count", 32, "<i4", 1), ("kf_inv_depth", 36, "<f4", 1),
               ("kf_variance", 40, "<f4", 1))
INFO_BYTES = 44
KP2D_BYTES, KP3D_BYTES = 8, 12

# svo_export_segment: (name, byte offset, numpy type, count); 64 bytes
SEGMENT_FIELDS = (("seq", 0, "<i4", 1), ("run", 4, "<i4", 1), ("frame_id", 8, "<i4", 1), ("keyframe_id", 12, "<i4", 1),
                  ("is_keyframe", 16, "<i4", 1), ("n", 20, "<i4", 1), ("first", 24, "<i8", 1), ("pose", 32, "<f4", 6),
                  ("time_stamp", 56, "<f4", 1), ("_pad", 60, "<i4", 1))
SEGMENT_BYTES = 64

# the ten 4-byte planes of an SoA keypoint set (svo_keypoints), besides kps2d and kps3d
PLANES = ("flags", "keyframe_id", "keypoint_index", "outlier_count", "inlier_count", "kf_inv_depth", "kf_variance",
          "score", "level_type", "color")
IGNORE_DURING_REFINEMENT, IGNORE_COMPLETELY, IGNORE_TEMPORARY = 1, 2, 4


def align_up(v, a):
    return (v + a - 1) // a * a


def capacity(cfg):
    """records one slot can take: 2 * grid cells + 128, rounded up to a multiple of 64"""
    cells = (cfg["width"] // cfg["grid_width"]) * (cfg["height"] // cfg["grid_height"])
    return align_up(2 * cells + 128, 64)


def info_records(planes):
    """planes: {name of PLANES: uint32 array [n] holding the plane's 4-byte values as bits} -> uint8 [n, 44]: the
    records the getters build (a cleared record, then its fields)"""
    p = {k: np.asarray(v).view(np.uint32) for k, v in planes.items()}
    n = len(p["flags"])
    out = np.zeros((n, INFO_BYTES), np.uint8)

    def put(offset, words):
        out[:, offset:offset + 4] = np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(n, 4)

    put(0, p["score"])
    put(4, p["level_type"] & 0xff)
    put(8, (p["level_type"] >> 8) & 0xff)
    put(12, p["keyframe_id"])
    put(16, p["keypoint_index"])
    for c in range(3):
        out[:, 20 + c] = (p["color"] >> (8 * c)) & 0xff
    out[:, 23] = (p["flags"] & IGNORE_DURING_REFINEMENT) != 0
    out[:, 24] = (p["flags"] & IGNORE_COMPLETELY) != 0
    out[:, 25] = (p["flags"] & IGNORE_TEMPORARY) != 0
    put(28, p["outlier_count"])
    put(32, p["inlier_count"])
    put(36, p["kf_inv_depth"])
    put(40, p["kf_variance"])
    return out


def group_ranges(n_slots, n_groups):
    """[(first slot, count)] of a ctx's groups: n // G slots each, the first n % G groups one more"""
    out, first = [], 0
    for g in range(n_groups):
        count = n_slots // n_groups + (1 if g < n_slots % n_groups else 0)
        out.append((first, count))
        first += count
    return out


def placement(seqs, counts, groups, per_seq):
    """first record of every segment. seqs[i]: the slot of segment i, counts[i]: its keypoints; groups: group_ranges;
    per_seq: capacity(cfg). Group g packs its named slots densely in named order from (named slots of earlier
    groups) * per_seq on, every first rounded up to a multiple of 4."""
    first = [None] * len(seqs)
    before = 0
    for lo, count in groups:
        mine = [i for i, s in enumerate(seqs) if lo <= s < lo + count]
        at = before * per_seq
        for i in mine:
            at = align_up(at, 4)
            first[i] = at
            at += counts[i]
        before += len(mine)
    return first


def pack(sets, first, records, fill=0xA5):
    """sets: [(n, kps2d float32 [n, 2], kps3d float32 [n, 3], planes)] -> the three arrays (uint8 [records, 8],
    [records, 12], [records, 44]) pre-filled with `fill`, set i at records first[i] .. first[i] + n - 1"""
    o2 = np.full((records, KP2D_BYTES), fill, np.uint8)
    o3 = np.full((records, KP3D_BYTES), fill, np.uint8)
    oi = np.full((records, INFO_BYTES), fill, np.uint8)
    for (n, k2, k3, planes), f in zip(sets, first):
        if n == 0:
            continue
        o2[f:f + n] = np.ascontiguousarray(k2[:n]).view(np.uint8).reshape(n, KP2D_BYTES)
        o3[f:f + n] = np.ascontiguousarray(k3[:n]).view(np.uint8).reshape(n, KP3D_BYTES)
        oi[f:f + n] = info_records({k: v[:n] for k, v in planes.items()})
    return o2, o3, oi
