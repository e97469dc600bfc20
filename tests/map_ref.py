"""The map export (svo_submit_export_map, svo_pack_map_points) restated in numpy: the filter, the 16-byte point and the
dense, stable compaction of many regions. Written from include/svo_hip.h alone; the tests compare the library with it
byte for byte."""
import numpy as np

# (name, byte offset, numpy type, count) of the structs of the C header
POINT_FIELDS = (("x", 0, "<f4", 1), ("y", 4, "<f4", 1), ("z", 8, "<f4", 1), ("color", 12, "u1", 3), ("flags", 15, "u1", 1))
FILTER_FIELDS = (("drop_flags", 0, "<u4", 1), ("own_only", 4, "<i4", 1), ("min_inliers", 8, "<i4", 1), ("_reserved", 12, "<i4", 1))
KEYFRAME_FIELDS = (("id", 0, "<i4", 1), ("n_total", 4, "<i4", 1), ("n", 8, "<i4", 1), ("_pad", 12, "<i4", 1),
                   ("first", 16, "<i8", 1), ("pose", 24, "<f4", 6))
SEGMENT_FIELDS = (("seq", 0, "<i4", 1), ("run", 4, "<i4", 1), ("frame_id", 8, "<i4", 1), ("status", 12, "<i4", 1),
                  ("n_keyframes", 16, "<i4", 1), ("keyframes_retired", 20, "<i4", 1), ("from_keyframe", 24, "<i4", 1),
                  ("n_exported", 28, "<i4", 1), ("n_points", 32, "<i8", 1), ("points_bound", 40, "<i8", 1),
                  ("time_stamp", 48, "<f4", 1), ("_pad", 52, "<i4", 3))
REGION_FIELDS = (("first_point", 0, "<i8", 1), ("point_capacity", 8, "<i8", 1), ("first_keyframe_entry", 16, "<i8", 1),
                 ("keyframe_capacity", 24, "<i4", 1), ("from_keyframe", 28, "<i4", 1))
POINT_BYTES, FILTER_BYTES, KEYFRAME_BYTES, SEGMENT_BYTES, REGION_BYTES = 16, 16, 48, 64, 32
COMPLETE, TOO_SMALL = 0, 1

IGNORE_DURING_REFINEMENT, IGNORE_COMPLETELY, IGNORE_TEMPORARY = 1, 2, 4
FLAG_BITS = 7
# the planes of an SoA keypoint set that the map reads, besides kps3d
PLANES = ("flags", "keyframe_id", "inlier_count", "color")
KEEP_ALL = dict(drop_flags=0, own_only=0, min_inliers=0)


def keep_mask(planes, own_id, filt):
    """bool [n]: which keypoints of a set held by keyframe own_id pass `filt` (a dict of svo_map_filter's fields).
    planes: {name of PLANES: uint32 array [n] holding the plane's 4-byte values as bits}"""
    flags = np.asarray(planes["flags"]).view(np.uint32)
    keep = (flags & np.uint32(filt.get("drop_flags", 0))) == 0
    if filt.get("own_only", 0):
        keep &= np.asarray(planes["keyframe_id"]).view(np.int32) == np.int32(own_id)
    keep &= np.asarray(planes["inlier_count"]).view(np.int32) >= np.int32(filt.get("min_inliers", 0))
    return keep


def point_records(kps3d, planes):
    """uint8 [n, 16]: kps3d (float32 or uint32 [n, 3]: the bits pass through), r g b (the colour word's low three
    bytes), the SVO_IGNORE_* bits of the flags word"""
    k3 = np.ascontiguousarray(kps3d).view(np.uint32).reshape(-1, 3)
    n = len(k3)
    out = np.zeros((n, POINT_BYTES), np.uint8)
    out[:, :12] = k3.astype("<u4").view(np.uint8).reshape(n, 12)
    color = np.asarray(planes["color"]).view(np.uint32)
    for c in range(3):
        out[:, 12 + c] = (color >> (8 * c)) & 0xff
    out[:, 15] = np.asarray(planes["flags"]).view(np.uint32) & FLAG_BITS
    return out


def pack(regions, first, filt, records, fill=0xA5):
    """regions: per region a list of sets (n, own_id, kps3d [n, 3], planes); first[r]: the record region r starts
    at. Returns (points uint8 [records, 16] pre-filled with `fill`, counts: the kept points of every set in call
    order): a region's kept points lie densely from first[r] on, set after set, in keypoint order."""
    points = np.full((records, POINT_BYTES), fill, np.uint8)
    counts = []
    for sets, at in zip(regions, first):
        for n, own_id, k3, planes in sets:
            p = {k: np.asarray(v)[:n] for k, v in planes.items()}
            keep = keep_mask(p, own_id, filt)
            m = int(keep.sum())
            points[at:at + m] = point_records(np.asarray(k3)[:n], p)[keep]
            counts.append(m)
            at += m
    return points, counts
