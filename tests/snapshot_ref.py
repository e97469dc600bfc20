"""The snapshot format of include/svo_hip.h stated independently in Python: the host part of a slot's saved
sequence state, built field by field with struct.pack from the header's description (no ctypes struct of the
binding, no library call). Tests feed what this writes to svo_snapshot_info and read what the library saves
with what this parses."""
import struct

import numpy as np

MAGIC, VERSION, BYTE_ORDER = 0x534F5653, 1, 0x01020304
COMPLETE, TOO_SMALL = 0, 1
CAM_FLOATS = ("baseline", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")
CAM_INTS = ("grid_height", "grid_width", "search_x", "search_y", "window_size_pose_estimator", "window_size_opt_flow",
            "window_size_depth_calculator", "max_pyramid_levels", "min_pyramid_level_pose_estimation")
COUNTS = ("width", "height", "capacity", "pyramid_levels", "lk_levels", "frame_id", "n_keypoints", "n_trajectory",
          "n_keyframes", "keyframes_retired", "n_image_sets", "n_planes", "_reserved")
HEADER = struct.Struct("<4I2q10f9i13i")
HEADER_FIELDS = ("magic", "version", "byte_order", "status", "host_bytes", "data_bytes") + CAM_FLOATS + CAM_INTS + COUNTS
FILTER_BYTES = 4 * (12 + 12 + 7 * 144)          # statePre, statePost, A, H, Q, R, errorCovPre, errorCovPost, gain
STATS_BYTES = 4 * (6 + 6 + 6 + 2 + 1 + 8) + 9 * 52
FRAME_BYTES = 8 + 4 * 6 + STATS_BYTES           # double time stamp, filtered pose, svo_frame_stats
POSE = struct.Struct("<6f")
KEYFRAME = struct.Struct("<6fii")               # pose, n, image set (-1: retired)
PLANE = struct.Struct("<qii")                   # offset, row_bytes, rows
KP_ELEM = (8, 12, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4)  # kps2d, kps3d, then the ten 4-byte arrays
MAX_KEYFRAMES = 4096
assert HEADER.size == 160 and FILTER_BYTES == 4128 and FRAME_BYTES == 616 and KEYFRAME.size == 32 and PLANE.size == 16


def capacity(cfg):
    """keypoints a slot holds: 2 * grid cells + 128, rounded up to 64"""
    cells = (cfg["width"] // cfg["grid_width"]) * (cfg["height"] // cfg["grid_height"])
    return (2 * cells + 128 + 63) // 64 * 64


def lk_levels(cfg):
    """cv::buildOpticalFlowPyramid stops at levels not larger than the window (at most 3 levels)"""
    w, h = cfg["width"], cfg["height"]
    for l in range(3):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= cfg["window_size_opt_flow"] or h <= cfg["window_size_opt_flow"]:
            return l + 1
    return 3


def plane_dims(cfg, n_keypoints, keyframe_ns, n_sets):
    """(row_bytes, rows) of every plane in directory order"""
    dims = [(e * n_keypoints, 1) for e in KP_ELEM] + [(4, 1), (4, 1)]
    for n in keyframe_ns:
        dims += [(e * n, 1) for e in KP_ELEM]
    for _ in range(n_sets):
        dims += [(cfg["width"] >> l, cfg["height"] >> l) for l in range(cfg["max_pyramid_levels"])]
        dims.append((cfg["width"], cfg["height"]))
        w, h = cfg["width"], cfg["height"]
        for _ in range(1, lk_levels(cfg)):
            w, h = (w + 1) // 2, (h + 1) // 2
            dims.append((w, h))
    return dims


def host_part(cfg, frame_id=-1, n_keypoints=0, keyframes=(), n_sets=0, retired=0, status=COMPLETE):
    """A minimal valid host part: keyframes = [(n, image set or -1)], planes packed at multiples of 16, the filter,
    frame and trajectory sections zero. Returns (bytes, {section name: offset}, {header field: value})."""
    dims = plane_dims(cfg, n_keypoints, [n for n, _ in keyframes], n_sets)
    directory, off = [], 0
    for row_bytes, rows in dims:
        directory.append((off, row_bytes, rows))
        off += (row_bytes * rows + 15) // 16 * 16
    n_traj = frame_id + 1
    sections = {"header": 0, "filter": HEADER.size}
    sections["frame"] = sections["filter"] + FILTER_BYTES
    sections["trajectory"] = sections["frame"] + FRAME_BYTES
    sections["keyframes"] = sections["trajectory"] + POSE.size * n_traj
    sections["directory"] = sections["keyframes"] + KEYFRAME.size * len(keyframes)
    sections["end"] = sections["directory"] + PLANE.size * len(dims)
    fields = dict(magic=MAGIC, version=VERSION, byte_order=BYTE_ORDER, status=status, host_bytes=sections["end"],
                  data_bytes=off, width=cfg["width"], height=cfg["height"], capacity=capacity(cfg),
                  pyramid_levels=cfg["max_pyramid_levels"], lk_levels=lk_levels(cfg), frame_id=frame_id,
                  n_keypoints=n_keypoints, n_trajectory=n_traj, n_keyframes=len(keyframes), keyframes_retired=retired,
                  n_image_sets=n_sets, n_planes=len(dims), _reserved=0)
    fields.update({k: cfg[k] for k in CAM_FLOATS + CAM_INTS})
    body = bytes(FILTER_BYTES + FRAME_BYTES) + b"".join(POSE.pack(*[0.0] * 6) for _ in range(n_traj))
    body += b"".join(KEYFRAME.pack(*[0.0] * 6, n, s) for n, s in keyframes)
    body += b"".join(PLANE.pack(*d) for d in directory)
    return pack_header(fields) + body, sections, fields


def pack_header(fields):
    return HEADER.pack(*[fields[k] for k in HEADER_FIELDS])


def with_header(part, fields, **changes):
    """the host part with some header fields replaced"""
    return pack_header(dict(fields, **changes)) + part[HEADER.size:]


def parse(part):
    """A host part as a dict: the header's fields, `filter` (float32 [1032]), `time_stamp`, `pose`, `stats` (raw
    bytes), `trajectory` [n, 6], `keyframes` [(pose, n, image set)], `directory` [(offset, row_bytes, rows)]."""
    part = bytes(part)
    out = dict(zip(HEADER_FIELDS, HEADER.unpack_from(part, 0)))
    p = HEADER.size
    out["filter"] = np.frombuffer(part, "<f4", FILTER_BYTES // 4, p)
    p += FILTER_BYTES
    out["time_stamp"] = struct.unpack_from("<d", part, p)[0]
    out["pose"] = np.frombuffer(part, "<f4", 6, p + 8)
    out["stats"] = part[p + 32:p + FRAME_BYTES]
    p += FRAME_BYTES
    out["trajectory"] = np.frombuffer(part, "<f4", 6 * out["n_trajectory"], p).reshape(-1, 6)
    p += POSE.size * out["n_trajectory"]
    out["keyframes"] = []
    for _ in range(out["n_keyframes"]):
        v = KEYFRAME.unpack_from(part, p)
        out["keyframes"].append((np.array(v[:6], np.float32), v[6], v[7]))
        p += KEYFRAME.size
    out["directory"] = [PLANE.unpack_from(part, p + PLANE.size * i) for i in range(out["n_planes"])]
    assert p + PLANE.size * out["n_planes"] == out["host_bytes"]
    return out
