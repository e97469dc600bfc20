"""Headless replay harness: the counterpart of SlamApp::process_image
(src/app/slam_app.cpp:160-196), of the trajectory CSV writer in SlamApp::stop
(:229-244), of the YAML reader ImageInput::read_settings (src/app/image_input.cpp:13-37)
and of the evaluation scripts test/extract_fps.py:26-34 / test/extract_extremas.py:31-54.

Host bookkeeping only; every frame goes through StereoSlam.new_image (libsvo_hip.so).

    python -m stereo_svo_slam_amd.replay --synthetic euroc --frames 100 -t traj.csv
    python -m stereo_svo_slam_amd.replay --settings EuRoC.yaml --euroc /data/MH_02_easy/mav0/ -t traj.csv
    python -m stereo_svo_slam_amd.replay --settings EuRoC.yaml --euroc /data/MH_02_easy/mav0/ --gpu-rectify
    python -m stereo_svo_slam_amd.replay --settings EuRoC.yaml --euroc /data/MH_02_easy/mav0/ --gpu-maps
    python -m stereo_svo_slam_amd.replay --settings Blender.yaml --sbs 'frames/%06d.png' -t traj.csv
    python -m stereo_svo_slam_amd.replay --settings Blender.yaml --sbs 'frames/%06d.png' --gpu-ingest
    python -m stereo_svo_slam_amd.replay --settings Econ.yaml --interleaved 'frames/%06d.png' --gpu-ingest
    python -m stereo_svo_slam_amd.replay --settings EuRoC.yaml --pairs 'seq/%06d_left.png,seq/%06d_right.png'
    python -m stereo_svo_slam_amd.replay --synthetic tiny --frames 20 --dump-views views/
    python -m stereo_svo_slam_amd.replay --synthetic tiny --frames 20 --dump-scene scene/
    python -m stereo_svo_slam_amd.replay --synthetic tiny --frames 20 --dump-ar ar/ --ar-box 0.2 --ar-at 0,0,0.5

Inputs follow the reference's conventions (the library's `left` is the physically RIGHT camera):
EurocInput (src/app/euroc_input.cpp:48-70,100-105), VideoInput (src/app/video_input.cpp:29-36), EconInput
(src/app/econ_input.cpp:102-106). Colour frames become gray with cvtColor's arithmetic (bgr2gray), on the host or,
with --gpu-ingest, inside the library from the raw frame (svo_ctx_set_input_format): both give the same CSV, and
frames that are gray already give the CSV they gave before colour frames were converted this way.
--dump-views DIR writes per frame the two halves of the reference app's window (draw_frame, src/app/main.cpp:40-118)
as binary PPM files, DIR/000000_keyframe.ppm (the last keyframe, a marker per keypoint) and DIR/000000_frame.ppm (the
current frame): the gray image the tracker worked on, which with --gpu-rectify / --gpu-ingest only the GPU has seen.
The text overlay and the x2 resize of the window are not drawn.
--dump-disparity DIR [--disparity-step S] [--disparity-depth] writes per frame DIR/000000_disparity.npy: the dense
disparity (or depth) map of the frame's rectified pair at every S-th pixel. With --disparity-sgm P1,P2[,CAP] the map is
aggregated semi-globally and the file stacks value and aggregated cost. With --disparity-lr D the map is
cross-checked left-right and the file is [3, rows, cols]: the value (invalid where the two searches differ by more than
D; D = 0 only reports), the cost and the lr plane; together with --disparity-sgm the check is the SGM map's own (a
second SGM map of the mirrored pair) and the file stacks value, aggregated cost and lr. --cloud-lr D drops such points
from the clouds of --dump-cloud; --cloud-sgm P1,P2[,CAP] makes those the clouds of the SGM map (and --cloud-lr its check).
The consumers of the clouds have the same switch: --dense-map-sgm (the map of --dump-dense-map / --scene-fused, with
--cloud-lr), --scene-dense-sgm (--scene-dense / --scene-accumulate, with --scene-dense-lr) and --ar-sgm (--ar-occlude,
with --ar-lr); each takes P1,P2[,CAP] and needs a search_x <= 63.
--dump-cloud DIR [--cloud-step S] [--cloud-max-depth Z] writes, whenever the newest keyframe changes,
DIR/kf000000_cloud.ply: the dense coloured point cloud of that keyframe in the world frame at every S-th pixel (binary
little-endian PLY, x y z float and red green blue uchar), so that the files of a run together are a dense map of it.
--dump-scene DIR writes per frame DIR/000000_scene.ppm: the 3-D viewer's picture of the map so far
(src/qt-viewer/PointCloudViewer.qml: points, trajectory, frusta) through its front camera. --scene-dense STEP
[--scene-dense-lr D] [--scene-dense-max-depth Z] draws the frame's dense cloud into it, --scene-accumulate N the dense
clouds of the keyframes so far (one device array of at most N records): the dense map growing.
--dump-dense-map FILE.ply --dense-map-voxel V [--dense-map-log2 N] [--dense-map-min-count K] fuses every new keyframe's
dense cloud (--cloud-step, --cloud-lr, --cloud-max-depth) into a voxel map of edge V kept inside the ctx (bounded,
every surface once, the keyframes that saw a voxel averaged) and writes it as one PLY at the end; --dense-map-window METRES
and --dense-map-keep N prune it behind every fuse (a box around the camera; what the last N fuses reached), --dense-map-carve
MARGIN carves it in front of every fuse (what the current frame's dense depth sees through leaves); --scene-fused V draws
that map in the pictures of --dump-scene. --save-dense-map FILE writes the map's raw entries (counts, sums, stamps) at the
end, --load-dense-map FILE merges such a file into the empty map before the first fuse (together: a run continues
yesterday's map), and --dense-map-grow N moves a map that is full into a larger table, up to 1 << N entries.
--dump-ar DIR writes per frame DIR/000000_ar.ppm: the AR demo's picture (src/ar-app/), a lit box of edge --ar-box
fixed at the world point --ar-at over the frame's left image, seen from the tracked pose; the default placement is the
demo's, half a metre in front of the first camera (AnimatedEntity.qml:56). If the pose is right the box stands still.
--ar-occlude STEP [--ar-hidden drop|dim] [--ar-alpha A] [--ar-margin M] [--ar-lr D] hides the box where the frame's
dense stereo depth (searched at every STEP-th pixel, left-right checked at tolerance D) lies in front of it, and prints
a line "ar NNNNNN covered C hidden H occluder_points P" per frame.
With $SVO_DATA set (a EuRoC `mav0/` directory, or a directory of side-by-side frames) and no
explicit input that data is used; otherwise the seeded synthetic sequence.
"""
import argparse
import math
import os
import re
import time

import numpy as np
import torch

from . import hip_lib, synth
from .jobs import VOXEL_SAVE_HEADER_DTYPE, VOXEL_SAVE_MAGIC, VOXEL_SAVE_VERSION, VoxelSaves
from .stereo_slam import StereoSlam

# key in the YAML -> CameraSettings field (src/app/image_input.cpp:16-36)
_YAML_KEYS = {
    "Camera1.fx": "fx", "Camera1.fy": "fy", "Camera1.cx": "cx", "Camera1.cy": "cy",
    "Camera.baseline": "baseline",
    "Camera.window_size_pose_estimator": "window_size_pose_estimator",
    "Camera.window_size_opt_flow": "window_size_opt_flow",
    "Camera.window_size_depth_calculator": "window_size_depth_calculator",
    "Camera.max_pyramid_levels": "max_pyramid_levels",
    "Camera.min_pyramid_level_pose_estimation": "min_pyramid_level_pose_estimation",
    "Camera1.k1": "k1", "Camera1.k2": "k2", "Camera1.k3": "k3", "Camera1.p1": "p1", "Camera1.p2": "p2",
    "Camera.grid_width": "grid_width", "Camera.grid_height": "grid_height",
    "Camera.search_x": "search_x", "Camera.search_y": "search_y",
}
_INT_FIELDS = {"window_size_pose_estimator", "window_size_opt_flow", "window_size_depth_calculator",
               "max_pyramid_levels", "min_pyramid_level_pose_estimation", "grid_width", "grid_height",
               "search_x", "search_y"}


def read_settings(path):
    """cv::FileStorage YAML (`%YAML:1.0` header, `key: value # comment` scalars; matrices are
    skipped) -> dict with the CameraSettings fields. Missing keys read as 0 like cv::FileNode."""
    out = {f: (0 if f in _INT_FIELDS else 0.0) for f in _YAML_KEYS.values()}
    with open(path) as fh:
        for line in fh:
            m = re.match(r"^([A-Za-z0-9_.]+)\s*:\s*([-+0-9.eE]+)\s*(#.*)?$", line.strip())
            if m and m.group(1) in _YAML_KEYS:
                f = _YAML_KEYS[m.group(1)]
                out[f] = int(float(m.group(2))) if f in _INT_FIELDS else float(m.group(2))
            m2 = re.match(r"^(Camera\.(width|height|image_width|image_height))\s*:\s*(\d+)", line.strip())
            if m2:
                out["width" if "width" in m2.group(1) else "height"] = int(m2.group(3))
    return out


def read_matrix(path, key):
    """A `key: !!opencv-matrix` entry of a cv::FileStorage YAML (rows, cols, data) as float64 array,
    or None (LEFT.K, LEFT.D, LEFT.R, LEFT.P ... of src/app/EuRoC.yaml)."""
    txt = open(path).read()
    m = re.search(re.escape(key) + r"\s*:\s*!!opencv-matrix\s*rows:\s*(\d+)\s*cols:\s*(\d+)\s*dt:\s*\w+\s*data:\s*\[([^\]]*)\]",
                  txt, re.S)
    if not m:
        return None
    return np.array([float(v) for v in m.group(3).replace("\n", " ").split(",")], np.float64).reshape(
        int(m.group(1)), int(m.group(2)))


def read_scalar(path, key, default=0):
    m = re.search(r"^" + re.escape(key) + r"\s*:\s*([-+0-9.eE]+)", open(path).read(), re.M)
    return float(m.group(1)) if m else default


def undistort_rectify_map(K, D, R, P, size):
    """cv::initUndistortRectifyMap(K, D, R, P[:3,:3], size, CV_32F): for every pixel of the rectified
    image the position in the raw image (map_x, map_y), 5-coefficient Brown model."""
    w, h = size
    iR = np.linalg.inv(np.asarray(P, np.float64)[:3, :3] @ np.asarray(R, np.float64))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    pts = np.stack([u, v, np.ones_like(u)], -1) @ iR.T
    x, y = pts[..., 0] / pts[..., 2], pts[..., 1] / pts[..., 2]
    d = list(np.ravel(D)) + [0.0] * 5
    k1, k2, p1, p2, k3 = d[:5]
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + p1 * 2 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * 2 * x * y
    K = np.asarray(K, np.float64)
    return (K[0, 0] * xd + K[0, 2]).astype(np.float32), (K[1, 1] * yd + K[1, 2]).astype(np.float32)


def remap_linear(img, map_x, map_y):
    """cv::remap(img, ., map_x, map_y, INTER_LINEAR) with a constant 0 border, 8-bit."""
    h, w = img.shape
    x0 = np.floor(map_x).astype(np.int64)
    y0 = np.floor(map_y).astype(np.int64)
    ax, ay = map_x - x0, map_y - y0
    src = np.pad(img.astype(np.float32), 1)

    def at(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, src[np.clip(yy, -1, h) + 1, np.clip(xx, -1, w) + 1], 0.0)

    v = (at(y0, x0) * (1 - ax) * (1 - ay) + at(y0, x0 + 1) * ax * (1 - ay) +
         at(y0 + 1, x0) * (1 - ax) * ay + at(y0 + 1, x0 + 1) * ax * ay)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def bgr2gray(img, order="bgr"):
    """cv::cvtColor(BGR2GRAY / RGB2GRAY) of a uint8 [..., 3] array, OpenCV 4.x's 15-bit fixed point:
    Y = (3735 B + 19235 G + 9798 R + 2^14) >> 15 (the weights sum to 2^15: R = G = B = v gives v)."""
    c = np.asarray(img).astype(np.uint32)
    b, r = (c[..., 0], c[..., 2]) if order == "bgr" else (c[..., 2], c[..., 0])
    return ((3735 * b + 19235 * c[..., 1] + 9798 * r + (1 << 14)) >> 15).astype(np.uint8)


def _load(path):
    """a decoded frame as the reference's cv::imread / VideoCapture hands it out: uint8 [H, W] for a gray file,
    [H, W, 3] in B, G, R order for a colour one (palette and alpha files are decoded to colour first)"""
    from PIL import Image
    im = Image.open(path)
    if im.mode == "L":
        return np.ascontiguousarray(np.array(im))
    if im.mode in ("1", "I", "I;16", "F", "LA"):
        return np.ascontiguousarray(np.array(im.convert("L")))
    return np.ascontiguousarray(np.array(im.convert("RGB"))[..., ::-1])


def _gray(path):
    img = _load(path)
    return img if img.ndim == 2 else np.ascontiguousarray(bgr2gray(img))


class EurocInput:
    """EurocInput (src/app/euroc_input.cpp): `image_path` is the mav0/ directory. cam0/data.csv lists
    time stamps [ns] and file names; the library's `right` image is cam0 rectified with the LEFT.*
    calibration of the settings file, `left` is cam1 rectified with RIGHT.* (:69-70, :100-101); time
    stamps are seconds since the first frame as float (:104-110). raw=True: read() hands out the
    unrectified frames, for the tracker to rectify on the GPU with gpu_maps() or gpu_calibration().
    host_maps=False: the float maps are not computed here (gpu_calibration() needs none)."""

    def __init__(self, image_path, settings, raw=False, host_maps=True):
        self.raw = raw
        self.right_images, self.left_images, self.timestamps = [], [], []
        t0 = None
        with open(os.path.join(image_path, "cam0", "data.csv")) as fh:
            for line in fh:
                line = line.strip()
                if not line or line.startswith("#"):
                    continue
                stamp, name = line.split(",")[0], line.split(",")[-1].strip()
                self.right_images.append(os.path.join(image_path, "cam0", "data", name))
                self.left_images.append(os.path.join(image_path, "cam1", "data", name))
                t = float(stamp) / 1.0e9
                t0 = t if t0 is None else t0
                self.timestamps.append(np.float32(t - t0))
        self.maps_l = self.maps_r = None
        mats = {k: read_matrix(settings, k) for k in ("LEFT.K", "LEFT.D", "LEFT.R", "LEFT.P",
                                                     "RIGHT.K", "RIGHT.D", "RIGHT.R", "RIGHT.P")}
        self.mats = mats if all(v is not None for v in mats.values()) else None
        if self.mats is not None and host_maps:
            size_l = (int(read_scalar(settings, "LEFT.width")), int(read_scalar(settings, "LEFT.height")))
            size_r = (int(read_scalar(settings, "RIGHT.width")), int(read_scalar(settings, "RIGHT.height")))
            self.maps_l = undistort_rectify_map(mats["LEFT.K"], mats["LEFT.D"], mats["LEFT.R"], mats["LEFT.P"], size_l)
            self.maps_r = undistort_rectify_map(mats["RIGHT.K"], mats["RIGHT.D"], mats["RIGHT.R"], mats["RIGHT.P"], size_r)

    def __len__(self):
        return len(self.left_images)

    def read(self, k):
        """(left, right, time_stamp) in the library's naming."""
        cam0, cam1 = _gray(self.right_images[k]), _gray(self.left_images[k])
        if self.maps_l is not None and not self.raw:
            cam0 = remap_linear(cam0, *self.maps_l)      # right <- remap(cam0, M1l, M2l)
            cam1 = remap_linear(cam1, *self.maps_r)      # left  <- remap(cam1, M1r, M2r)
        return cam1, cam0, float(self.timestamps[k])

    def gpu_maps(self):
        """(left maps, right maps) in the library's naming for StereoSlam.set_rectification: the library's
        left image is cam1 (RIGHT.* calibration, M1r/M2r), its right image cam0 (LEFT.*, M1l/M2l)."""
        if self.maps_l is None:
            raise ValueError("the settings file has no LEFT.* / RIGHT.* rectification matrices")
        return self.maps_r, self.maps_l

    def gpu_calibration(self):
        """(left, right) CameraCalibrations in the library's naming for StereoSlam.set_calibration, as gpu_maps():
        left from RIGHT.*, right from LEFT.*. The library builds the maps of gpu_maps() from them on the GPU."""
        if self.mats is None:
            raise ValueError("the settings file has no LEFT.* / RIGHT.* rectification matrices")
        from .hip_lib import CameraCalibration
        left, right = (CameraCalibration.from_mats(*(self.mats[f"{side}.{k}"] for k in "KDRP")) for side in ("RIGHT", "LEFT"))
        return left, right


class SideBySideInput:
    """VideoInput (src/app/video_input.cpp:25-45) on decoded frames: every image holds both cameras
    side by side; colour frames become gray first (cvtColor(BGR2GRAY), :29-31: bgr2gray); `right` is the LEFT
    half, `left` the RIGHT half; time stamps advance by 1/fps from 1/fps. raw=True: read() hands out the undivided
    frame ([H, 2W] gray or [H, 2W, 3] B, G, R) as `left` and None as `right`, for the library to convert and split
    (input_format())."""

    def __init__(self, pattern, n_frames, fps=30.0, raw=False):
        self.pattern, self.n, self.fps, self.raw = pattern, n_frames, fps, raw

    def __len__(self):
        return self.n

    def input_format(self, k=0):
        """the library's input format name for the raw frames (by the channels of frame k)"""
        return "sbs_gray" if _load(self.pattern % k).ndim == 2 else "sbs_bgr"

    def read(self, k):
        if self.raw:
            return _load(self.pattern % k), None, (k + 1) / self.fps
        img = _gray(self.pattern % k)
        w = img.shape[1] // 2
        right = np.ascontiguousarray(img[:, :w])
        left = np.ascontiguousarray(img[:, w:2 * w])
        return left, right, (k + 1) / self.fps


class InterleavedInput:
    """EconInput (src/app/econ_input.cpp:102-106) on decoded frames: every image is one 3-channel frame whose
    channel 1 is the `right` image and channel 2 the `left` one; time stamps advance by 1/fps from 1/fps.
    raw=True: read() hands out the frame itself ([H, W, 3]) as `left` and None as `right` (input format ch3_econ).
    The channels are those of the stored file read in B, G, R order."""

    def __init__(self, pattern, n_frames, fps=30.0, raw=False):
        self.pattern, self.n, self.fps, self.raw = pattern, n_frames, fps, raw

    def __len__(self):
        return self.n

    def input_format(self, k=0):
        return "ch3_econ"

    def read(self, k):
        img = _load(self.pattern % k)
        if img.ndim != 3:
            raise ValueError("InterleavedInput needs 3-channel frames")
        if self.raw:
            return img, None, (k + 1) / self.fps
        return np.ascontiguousarray(img[..., 2]), np.ascontiguousarray(img[..., 1]), (k + 1) / self.fps


# END_MEASUREMENT names of the reference (src/lib/stereo_slam.cpp:66-86,140,227,235;
# src/lib/pose_refinement.cpp:120) over the stage times of svo_frame_stats (HIP events)
def time_trace_lines(stats):
    st = list(stats.stage_ms)
    lines = [("Create pyramid", st[0]), ("estimator", st[2]), ("REFINEMENT: Optical flow", st[3]),
             ("pose refinement", st[3] + st[4]), ("Filter update", st[5] + st[6])]
    if stats.is_keyframe:
        lines.append(("Create new keyframe", st[7]))
    lines.append(("Stereo SLAM", sum(st)))
    return [f"{name} took: {ms:.4f}ms" for name, ms in lines]


def _rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-15:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return math.cos(th) * np.eye(3) + (1 - math.cos(th)) * np.outer(k, k) + math.sin(th) * K


def _rodrigues_inv(R):
    """Rotation matrix -> axis-angle vector (cv::Rodrigues, matrix input)."""
    c = min(1.0, max(-1.0, (np.trace(R) - 1) / 2))
    th = math.acos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v) / 2
    if s < 1e-5:                     # OpenCV's threshold (hostcpp/stereo_slam_types.hpp has the same arms)
        if c > 0:
            return np.zeros(3)
        # theta = pi: axis from the diagonal, signs from R(0,1), R(0,2) and the R(1,2) tie-break
        a = np.sqrt(np.maximum((np.diag(R) + 1) / 2, 0))
        if R[0, 1] < 0:
            a[1] = -a[1]
        if R[0, 2] < 0:
            a[2] = -a[2]
        if abs(a[0]) < abs(a[1]) and abs(a[0]) < abs(a[2]) and (R[1, 2] > 0) != (a[1] * a[2] > 0):
            a[2] = -a[2]
        return a * (th / math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
    return v / (2 * s) * th


def csv_angles(pose):
    """Angles written to the trajectory CSV: Rodrigues((R_y R_x) R_z), slam_app.cpp:232-241."""
    Rx = _rodrigues([pose[3], 0, 0])
    Ry = _rodrigues([0, pose[4], 0])
    Rz = _rodrigues([0, 0, pose[5]])
    return _rodrigues_inv((Ry @ Rx) @ Rz)


def write_trajectory_csv(path, cumulative_times, trajectory):
    """`t_cumulative_algorithm_seconds,x,y,z,rx',ry',rz'` per frame (slam_app.cpp:229-244)."""
    with open(path, "w") as fh:
        for t, pose in zip(cumulative_times, trajectory):
            a = csv_angles(pose)
            fh.write(",".join(f"{v:.6g}" for v in (t, pose[0], pose[1], pose[2], a[0], a[1], a[2])) + "\n")


def fps_from_csv_rows(rows):
    """test/extract_fps.py:26-34: n / (t_last - t_first) over the cumulative algorithm time."""
    rows = np.asarray(rows, np.float64)
    dt = rows[-1, 0] - rows[0, 0]
    return rows.shape[0] / dt if dt > 0 else float("nan")


def error_report(test_rows, reference_rows):
    """test/extract_extremas.py:31-54: max / mean absolute error (angles in degrees) and FPS."""
    t = np.asarray(test_rows, np.float64)
    r = np.asarray(reference_rows, np.float64)[: t.shape[0]]
    d = np.abs(t - r)
    d[:, 4:] = d[:, 4:] / math.pi * 180
    return dict(max=d.max(0)[1:].tolist(), mean=d.mean(0)[1:].tolist(), fps=fps_from_csv_rows(t))


def write_ppm(path, img):
    """a uint8 [H, W, 3] R, G, B image as a binary PPM (P6)"""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        fh.write(img.tobytes())


def read_ppm(path):
    """a binary PPM (P6, maxval 255, as write_ppm writes it) as uint8 [H, W, 3]"""
    with open(path, "rb") as fh:
        raw = fh.read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxval == b"255" and len(body) == w * h * 3
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(path, points):
    """map points (hip_lib.MAP_POINT_DTYPE) as a binary little-endian PLY: x y z float, red green blue uchar"""
    v = np.empty(len(points), PLY_VERTEX)
    for k in ("x", "y", "z"):
        v[k] = points[k]
    for i, k in enumerate(("red", "green", "blue")):
        v[k] = points["color"][:, i]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(v))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())


def read_ply(path):
    """a PLY as write_ply writes it, as an array of PLY_VERTEX"""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int(lines[2].split()[2])
    assert len(body) == n * PLY_VERTEX.itemsize
    return np.frombuffer(body, PLY_VERTEX)


AR_BOX, AR_RGB = 0.2, 0xc08040


def ar_objects(size=AR_BOX, at=hip_lib.AR_AT, rgb=AR_RGB):
    """the objects of --dump-ar for StereoSlam.get_ar: one box of edge `size` at the world point `at`"""
    return [(*hip_lib.ar_box(size), hip_lib.ar_model(at), rgb)]


class Replay:
    """process_image loop: only the time inside new_image is accumulated (slam_app.cpp:186-190)."""

    def __init__(self, settings, device=0, time_trace=False, fast=False, rectify_maps=None, input_format=None,
                 gpu_imu=False, dump_views=None, dump_scene=None, calibration=None, keyframe_window=None, dump_ar=None,
                 ar_box=AR_BOX, ar_at=hip_lib.AR_AT, dump_disparity=None, disparity_step=4, disparity_depth=False,
                 dump_cloud=None, cloud_step=4, cloud_max_depth=0.0, disparity_lr=None, cloud_lr=None, scene_dense=None,
                 scene_dense_lr=None, scene_dense_max_depth=0.0, scene_accumulate=0, dump_dense_map=None, dense_map_voxel=None,
                 dense_map_log2=20, dense_map_min_count=0, dense_map_window=None, dense_map_keep=None, dense_map_carve=None, scene_fused=None, ar_occlusion=None, disparity_sgm=None, cloud_sgm=None,
                 dense_map_sgm=None, scene_dense_sgm=None, ar_sgm=None, save_dense_map=None, load_dense_map=None, dense_map_grow=None):
        """fast=False keeps the library default: the reference-order Gauss-Newton (bit-exact traces).
        rectify_maps = (left maps, right maps): the frames fed are raw and are rectified on the GPU.
        calibration = (left, right) CameraCalibrations: the same, with the maps built on the GPU as well.
        input_format: the frames fed are raw buffers of that format (StereoSlam.set_input_format).
        gpu_imu: update_pose_from_imu is one svo_update_poses (the filter kernel) instead of a loop of
        svo_update_pose calls: the same bits.
        dump_views: a directory that receives, per frame, the last keyframe and the current frame with a marker per
        keypoint as the reference app's window shows them (write_ppm), outside the timed region.
        dump_scene: a directory that receives, per frame, the 3-D viewer's picture of the map (get_scene), likewise.
        scene_dense: None, or the lattice step (1 .. 16) of the dense cloud of the current frame that dump_scene draws into
        its picture (get_scene(dense=...)); scene_dense_lr: None, or the tolerance (> 0) of its left-right cross-check;
        scene_dense_max_depth: points deeper than this are dropped (0: none). scene_accumulate = N > 0: whenever the newest
        keyframe id changes, that keyframe's compact device cloud (the same step, check and depth; step 4 without
        scene_dense) is appended to one device tensor of at most N records, oldest dropped first, which dump_scene
        draws as the extra span: the pictures show the dense map growing.
        dump_ar: a directory that receives, per frame, the AR demo's picture (get_ar): a lit box of edge ar_box at the
        world point ar_at over the frame's left image, likewise. The default is the demo's placement, half a metre in
        front of the first camera. ar_occlusion: None, or the occlusion of StereoSlamBatch.submit_ar as a dict: the box
        is hidden behind the frame's dense stereo depth, and a line "ar NNNNNN covered C hidden H occluder_points P" per
        frame goes to the log (ar_log keeps the three numbers per frame).
        dump_disparity: a directory that receives, per frame, the dense disparity map of the frame (get_disparity at
        the lattice disparity_step; the depth map with disparity_depth) as NNNNNN_disparity.npy [rows, cols], likewise.
        dump_cloud: a directory that receives, whenever the newest keyframe id changes, that keyframe's dense point cloud
        in the world frame (get_cloud of "last_keyframes" at the lattice cloud_step, points deeper than cloud_max_depth
        dropped; 0: none dropped) as kfNNNNNN_cloud.ply (write_ply), likewise.
        disparity_lr: None, or the tolerance of the left-right cross-check of dump_disparity (0: report only); the file
        is then [3, rows, cols]: value, cost, lr. disparity_sgm: None, or (p1, p2[, cost_cap]) of semi-global aggregation
        for dump_disparity (cost_cap: hip_lib.SGM_DEFAULTS'); the file is then [2, rows, cols]: value, aggregated cost;
        together with disparity_lr the SGM map is cross-checked by its own rule and the file is [3, rows, cols]: value,
        aggregated cost, lr. cloud_lr: None, or the tolerance (> 0) of the cross-check of dump_cloud. cloud_sgm: None, or
        (p1, p2[, cost_cap]): dump_cloud writes the clouds of the SGM map, cloud_lr then being the SGM map's own check.
        dump_dense_map: a PLY file that receives, at finish(), the slot's voxel map (get_voxel_map with
        dense_map_min_count): every new keyframe's dense cloud (cloud_step, cloud_lr, cloud_max_depth) is fused into a map
        of edge dense_map_voxel and 1 << dense_map_log2 entries kept inside the ctx. scene_fused = V: dump_scene draws
        that fused map (edge V; the same map when both are given) as the extra span, exported to device memory.
        keyframe_window: the retired keyframes the tracker keeps (StereoSlamBatch.set_keyframe_window); None: all."""
        self.settings = settings
        self.dump_views, self.dump_scene, self.dump_ar = dump_views, dump_scene, dump_ar
        self.ar_objects = ar_objects(ar_box, ar_at)
        self.ar_occlusion, self.ar_log = ar_occlusion, []
        self.dump_disparity, self.disparity_step, self.disparity_depth = dump_disparity, int(disparity_step), bool(disparity_depth)
        self.dump_cloud, self.cloud_step, self.cloud_max_depth, self._cloud_kf = dump_cloud, int(cloud_step), float(cloud_max_depth), -1
        self.disparity_lr = None if disparity_lr is None else float(disparity_lr)

        def sgm_dict(spec, lr):
            """(p1, p2[, cost_cap]) and the tolerance of the SGM map's own check (None: off; 0: report only) as sgm="""
            p = [int(v) for v in spec]
            return dict(p1=p[0], p2=p[1], cost_cap=p[2] if len(p) > 2 else hip_lib.SGM_DEFAULTS["cost_cap"],
                        lr_check=None if lr is None else (lr if lr > 0 else True))

        self.disparity_sgm = None if disparity_sgm is None else sgm_dict(disparity_sgm, self.disparity_lr)
        self.cloud_lr = None if cloud_lr is None else float(cloud_lr)
        self.cloud_sgm = None if cloud_sgm is None else sgm_dict(cloud_sgm, self.cloud_lr)
        self.scene_dense = None if scene_dense is None else int(scene_dense)
        self.scene_dense_lr = None if scene_dense_lr is None else float(scene_dense_lr)
        # (the SGM forms of the cloud's consumers: the same flags' clouds from the SGM map, the flag's lr then being the SGM
        # map's own check)
        for flag, spec in (("dense_map_sgm", dense_map_sgm), ("scene_dense_sgm", scene_dense_sgm), ("ar_sgm", ar_sgm)):
            if spec is not None and int(settings["search_x"]) > 63:
                raise ValueError(f"--{flag.replace('_', '-')} needs a search_x <= 63 (the settings have {int(settings['search_x'])}): "
                                 "the cost volume of the semi-global search holds at most 64 candidates")
        self.dense_map_sgm = None if dense_map_sgm is None else sgm_dict(dense_map_sgm, self.cloud_lr)
        self.scene_dense_sgm = None if scene_dense_sgm is None else sgm_dict(scene_dense_sgm, self.scene_dense_lr)
        if ar_sgm is not None:
            if self.ar_occlusion is None:
                raise ValueError("--ar-sgm needs --ar-occlude")
            lr = self.ar_occlusion.get("lr_check") or None
            self.ar_occlusion = dict(self.ar_occlusion, lr_check=0.0, sgm=sgm_dict(ar_sgm, lr))
        self.scene_dense_max_depth, self.scene_accumulate = float(scene_dense_max_depth), int(scene_accumulate)
        self._scene_kf, self._scene_map = -1, None
        self.dump_dense_map, self.dense_map_log2, self.dense_map_min_count = dump_dense_map, int(dense_map_log2), int(dense_map_min_count)
        self.scene_fused = None if scene_fused is None else float(scene_fused)
        self.dense_map_voxel = float(dense_map_voxel) if dense_map_voxel is not None else self.scene_fused
        if dump_dense_map and self.dense_map_voxel is None:
            raise ValueError("dump_dense_map needs dense_map_voxel")
        if self.scene_fused is not None and self.scene_fused != self.dense_map_voxel:
            raise ValueError("scene_fused and dense_map_voxel name one map: give the same edge")
        # (a prune behind every fuse of the map: a box of dense_map_window metres around the camera, and only what the
        # last dense_map_keep fuses reached)
        self.dense_map_prune = None
        if dense_map_window is not None or dense_map_keep is not None:
            if self.dense_map_voxel is None:
                raise ValueError("dense_map_window and dense_map_keep need a dense map")
            self.dense_map_prune = dict(center="pose")
            if dense_map_window is not None:
                self.dense_map_prune["radius"] = float(dense_map_window)
            if dense_map_keep is not None:
                self.dense_map_prune["keep_stamps"] = int(dense_map_keep)
        # (a carve in front of every fuse of the map: what the current frame's dense depth sees through by more than
        # dense_map_carve metres leaves; the occluder is the fuse's own kind of cloud)
        self.dense_map_carve = None
        if dense_map_carve is not None:
            if self.dense_map_voxel is None:
                raise ValueError("dense_map_carve needs a dense map")
            if not 0 <= float(dense_map_carve) < float("inf"):
                raise ValueError("dense_map_carve must be finite and >= 0")
            self.dense_map_carve = float(dense_map_carve)
        # (the map kept across runs: its raw entries written at finish(), merged into the empty map before the first fuse;
        # dense_map_grow: a full map moves into a larger table, up to 1 << dense_map_grow entries)
        self.save_dense_map, self.load_dense_map = save_dense_map, load_dense_map
        self.dense_map_grow = None if dense_map_grow is None else int(dense_map_grow)
        if (save_dense_map or load_dense_map or dense_map_grow is not None) and self.dense_map_voxel is None:
            raise ValueError("save_dense_map, load_dense_map and dense_map_grow need a dense map")
        if self.dense_map_grow is not None and not self.dense_map_log2 <= self.dense_map_grow <= 26:
            raise ValueError("dense_map_grow must be dense_map_log2 .. 26")
        self._dense_map_set, self._fused_job = False, None
        for d in (dump_views, dump_scene, dump_ar, dump_disparity, dump_cloud):
            if d:
                os.makedirs(d, exist_ok=True)
        self.gpu_imu = gpu_imu
        self.slam = StereoSlam(settings, device=device)
        if fast:
            self.slam.set_fast_solver(True)
        if rectify_maps is not None:
            self.slam.set_rectification(*rectify_maps)
        if calibration is not None:
            self.slam.set_calibration(*calibration)
        if input_format is not None:
            self.slam.set_input_format(input_format)
        if keyframe_window is not None:
            self.slam.set_keyframe_window(keyframe_window)
        self.cumulative = []
        self._t = 0.0
        self.time_trace = time_trace
        if time_trace:
            self.slam.enable_timing(True)

    IMU_RATE = 104.0                              # samples per second the Econ camera's IMU thread delivers

    def update_pose_from_imu(self, gyro_deg_s, dt):
        """SlamApp::update_pose_from_imu (slam_app.cpp:111-135): between two frames the pose filter is fed
        the gyro rates of at most IMU_RATE * dt samples ([n, 3] degrees per second, x y z) as the speed
        measurement with the app's variances, one StereoSlam::update_pose call of 1 / IMU_RATE each;
        nothing happens before the first frame. Returns the filtered pose (the app discards it: the calls
        act through the filter's state)."""
        if self.slam._ctx is None:                # (the ctx is created by the first frame)
            return None
        if self.gpu_imu:
            out = self.slam.update_poses_from_gyro([gyro_deg_s], dt)
            return out[-1] if len(out) else np.asarray(self.slam.pose(), np.float32)
        gyro = np.asarray(gyro_deg_s, np.float32).reshape(-1, 3)
        pose_variance = np.full(6, 1000.0, np.float32)
        speed_variance = np.array([100.0, 100.0, 100.0, 0.1, 0.1, 0.1], np.float32)
        pose = np.asarray(self.slam.pose(), np.float32)
        n = min(len(gyro), int(np.float32(self.IMU_RATE) * np.float32(dt)))    # std::min<size_t>(size, f * dt): truncated
        for g in gyro[:n]:
            speed = np.zeros(6, np.float32)
            speed[3:] = (g.astype(np.float64) / 180.0 * math.pi).astype(np.float32)
            pose = self.slam.update_pose(pose, speed, pose_variance, speed_variance, 1.0 / self.IMU_RATE)   # double 1.0 / f
        return pose

    def feed(self, left, right, time_stamp, gyro_deg_s=None, images_read=1):
        """process_image (slam_app.cpp:160-196); with IMU samples: update_pose_from_imu(images_read / 30) first"""
        if gyro_deg_s is not None:
            self.update_pose_from_imu(gyro_deg_s, images_read / 30.0)
        t0 = time.perf_counter()
        self.slam.new_image(left, right, time_stamp)
        self._t += time.perf_counter() - t0
        self.cumulative.append(self._t)
        if self.dump_views:
            k = len(self.cumulative) - 1
            for what, name in (("last_keyframes", "keyframe"), ("frames", "frame")):
                img = self.slam.get_image(what, pixel="rgb8", markers=True)
                if img is not None:
                    write_ppm(os.path.join(self.dump_views, f"{k:06d}_{name}.ppm"), img)
        if self.dump_scene:
            img = self.slam.get_scene("front", pixel="rgb8", **self._scene_clouds())
            if img is not None:
                write_ppm(os.path.join(self.dump_scene, f"{len(self.cumulative) - 1:06d}_scene.ppm"), img)
        if self.dump_ar:
            img = self.slam.get_ar(self.ar_objects, pixel="rgb8", occlusion=self.ar_occlusion)
            if img is not None:
                write_ppm(os.path.join(self.dump_ar, f"{len(self.cumulative) - 1:06d}_ar.ppm"), img)
                if self.ar_occlusion is not None:
                    v = self.slam.ar_visibility
                    self.ar_log.append((int(v["covered"]), int(v["hidden"]), int(v["occluder_points"])))
                    print(f"ar {len(self.cumulative) - 1:06d} covered {self.ar_log[-1][0]} hidden {self.ar_log[-1][1]} "
                          f"occluder_points {self.ar_log[-1][2]}")
        if self.dump_disparity:
            value = "depth" if self.disparity_depth else "disparity"
            if self.disparity_sgm is not None:
                planes = self.slam.get_disparity(value=value, step=self.disparity_step, cost=True, sgm=self.disparity_sgm)
            elif self.disparity_lr is None:
                planes = self.slam.get_disparity(value=value, step=self.disparity_step)
            else:
                planes = self.slam.get_disparity(value=value, step=self.disparity_step, cost=True,
                                                 lr_check=self.disparity_lr if self.disparity_lr > 0 else True)
            if planes is not None:
                np.save(os.path.join(self.dump_disparity, f"{len(self.cumulative) - 1:06d}_disparity.npy"),
                        planes[0] if self.disparity_lr is None and self.disparity_sgm is None else planes)
        if self.dump_cloud:
            kf = int(self.slam.stats().n_keyframes) - 1
            if kf != self._cloud_kf:
                self._cloud_kf = kf
                points = self.slam.get_cloud("last_keyframes", step=self.cloud_step, max_depth=self.cloud_max_depth,
                                             **(dict(lr_check=self.cloud_lr) if self.cloud_sgm is None else dict(sgm=self.cloud_sgm)))
                if points is not None:
                    write_ply(os.path.join(self.dump_cloud, f"kf{kf:06d}_cloud.ply"), points)
        if self.dense_map_voxel is not None and not self.dump_scene:
            self._fuse_dense_map()
        if self.time_trace:                       # like PRINT_TIME_TRACE of the reference
            print("\n".join(time_trace_lines(self.slam.stats())))

    def _fuse_dense_map(self):
        """the newest keyframe's dense cloud into the ctx's voxel map, once per keyframe (the map is set after the first
        frame: the ctx exists from then on). True: the map changed."""
        if self.slam._ctx is None:
            return False
        if not self._dense_map_set:
            self.slam.set_voxel_maps(self.dense_map_voxel, self.dense_map_log2)
            self._dense_map_set = True
            if self.load_dense_map:
                self._load_dense_map()
        how = dict(lr_check=self.cloud_lr) if self.dense_map_sgm is None else dict(sgm=self.dense_map_sgm)
        carve = None if self.dense_map_carve is None else dict(margin=self.dense_map_carve, step=self.cloud_step, max_depth=self.cloud_max_depth, **how)
        return self.slam.fuse_new_keyframes(step=self.cloud_step, max_depth=self.cloud_max_depth, prune=self.dense_map_prune, carve=carve,
                                            grow=self.dense_map_grow, **how) is not None

    def _load_dense_map(self):
        """the entries of load_dense_map (VoxelSaves.tobytes) merged into the map that was just set: the same voxel edge,
        bit for bit; a map too small for them is resized first where dense_map_grow allows"""
        with open(self.load_dense_map, "rb") as f:
            saved = VoxelSaves.frombytes(f.read())
        if np.float32(saved.voxel(0)).tobytes() != np.float32(self.dense_map_voxel).tobytes():
            raise ValueError(f"{self.load_dense_map} was made with voxel edge {float(saved.voxel(0))!r}, the map has {self.dense_map_voxel!r}")
        log2 = self.dense_map_log2
        while len(saved.entries(0)) > (1 << log2) - (1 << log2) // 4 and self.dense_map_grow is not None and log2 < self.dense_map_grow:
            log2 += 1
        if log2 != self.dense_map_log2:
            self.slam.resize_voxel_maps(log2)
        info = self.slam.load_voxel_maps(None, saved, merge=True).info[0]
        if int(info["status"]) != hip_lib.VOXEL_LOADED:
            raise ValueError(f"{self.load_dense_map} holds {len(saved.entries(0))} entries: too many for a map of 1 << {log2} (dense_map_log2, dense_map_grow)")

    def finish(self):
        """what is written once, after the last frame: the dense map of dump_dense_map, the entries of save_dense_map"""
        if self.save_dense_map:
            if self._dense_map_set:
                blob = self.slam.save_voxel_maps([0]).tobytes(0)
            else:                                   # (no frame ever came: an empty map of these params)
                head = np.zeros((), VOXEL_SAVE_HEADER_DTYPE)
                head["magic"], head["version"], head["log2_capacity"] = VOXEL_SAVE_MAGIC, VOXEL_SAVE_VERSION, self.dense_map_log2
                head["voxel_bits"] = np.float32(self.dense_map_voxel).view(np.uint32)
                blob = head.tobytes()
            with open(self.save_dense_map, "wb") as f:
                f.write(blob)
        if self.dump_dense_map:
            points = self.slam.get_voxel_map(min_count=self.dense_map_min_count) if self._dense_map_set else None
            write_ply(self.dump_dense_map, points if points is not None else np.zeros(0, hip_lib.MAP_POINT_DTYPE))

    def _scene_clouds(self):
        """the dense and clouds arguments of dump_scene's get_scene ({}: the sparse picture)"""
        kw = {}
        step = self.scene_dense if self.scene_dense is not None else 4
        sgm = self.scene_dense_sgm
        if self.scene_dense is not None:
            kw["dense"] = dict(what="frames", step=step, max_depth=self.scene_dense_max_depth,
                               **(dict(lr_check=self.scene_dense_lr or 0.0) if sgm is None else dict(sgm=sgm)))
        if self.scene_accumulate > 0:
            kf = int(self.slam.stats().n_keyframes) - 1
            if kf != self._scene_kf:
                self._scene_kf = kf
                job = self.slam.export_cloud("last_keyframes", None, step=step, layout="compact", device=True,
                                             max_depth=self.scene_dense_max_depth,
                                             **(dict(lr_check=self.scene_dense_lr) if sgm is None else dict(sgm=sgm)))
                if int(job.segments[0]["status"]) == hip_lib.CLOUD_OK:
                    new = job.points_buffer[:int(job.segments[0]["n_points"])]
                    both = new if self._scene_map is None else torch.cat([self._scene_map, new])
                    self._scene_map = both[max(0, both.shape[0] - self.scene_accumulate):].contiguous()
            if self._scene_map is not None and self._scene_map.shape[0] > 0:
                kw["clouds"] = [self._scene_map]
        if self.dense_map_voxel is not None:
            changed = self._fuse_dense_map()
            if self.scene_fused is not None and self._dense_map_set:
                if changed or self._fused_job is None:          # (the export stays on the device; the job owns the records)
                    self._fused_job = self.slam.export_voxel_maps(None, min_count=self.dense_map_min_count, device=True)
                span = self._fused_job.span(0)
                if span[1] > 0:
                    kw["clouds"] = [span]
        return kw

    def rows(self):
        traj = self.slam.get_trajectory()
        return np.array([[t, p[0], p[1], p[2], *csv_angles(p)] for t, p in zip(self.cumulative, traj)])

    def write(self, path):
        write_trajectory_csv(path, self.cumulative, self.slam.get_trajectory())


def _load_pair(pattern, k):
    lp, rp = pattern.split(",")
    return _gray(lp % k), _gray(rp % k)


def _keyframe_window(text):
    k = int(text)
    if k < 0:
        raise argparse.ArgumentTypeError("a count >= 0")
    return k


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--settings", help="cv::FileStorage YAML with the Camera.* keys")
    ap.add_argument("--synthetic", choices=sorted(synth.CONFIGS), help="seeded synthetic sequence")
    ap.add_argument("--pairs", help="'left_%%06d.png,right_%%06d.png': the library's left / right images")
    ap.add_argument("--euroc", help="EuRoC mav0/ directory (cam0, cam1): EurocInput conventions")
    ap.add_argument("--sbs", help="'frames/%%06d.png' side-by-side frames: VideoInput conventions")
    ap.add_argument("--time-trace", action="store_true", help="print '<stage> took: X ms' per frame (reference names)")
    ap.add_argument("--fast", action="store_true",
                    help="svo_ctx_set_fast_solver(1): tree sums + LDL^T instead of the default reference-order Gauss-Newton")
    ap.add_argument("--exact", action="store_true", help="no-op (the reference-order mode is the default)")
    ap.add_argument("--gpu-rectify", action="store_true",
                    help="--euroc: hand the raw frames to the library and rectify them on the GPU (bit-exact cv::remap)")
    ap.add_argument("--gpu-maps", action="store_true",
                    help="--euroc: as --gpu-rectify, and the rectification maps are built on the GPU from the LEFT.* / RIGHT.* "
                         "calibrations of the settings file (initUndistortRectifyMap; no float map on the host)")
    ap.add_argument("--interleaved", help="'frames/%%06d.png' 3-channel frames: EconInput conventions (right = channel 1, left = channel 2)")
    ap.add_argument("--gpu-ingest", action="store_true",
                    help="--sbs / --interleaved: hand the raw frames to the library, which converts and splits them on the GPU")
    ap.add_argument("--gyro", help="text file, one row 'frame gx gy gz' per IMU sample (degrees per second), rows in time "
                                   "order: the samples of frame k feed the pose filter before frame k (update_pose_from_imu)")
    ap.add_argument("--gpu-imu", action="store_true",
                    help="--gyro: one svo_update_poses per frame interval (the filter kernel) instead of one svo_update_pose per sample")
    ap.add_argument("--dump-views", metavar="DIR",
                    help="write per frame DIR/NNNNNN_keyframe.ppm and DIR/NNNNNN_frame.ppm: the last keyframe and the current "
                         "frame as the reference app's window draws them (gray as RGB, a marker per keypoint)")
    ap.add_argument("--dump-scene", metavar="DIR",
                    help="write per frame DIR/NNNNNN_scene.ppm: the 3-D viewer's picture of the map so far (keyframe points, "
                         "trajectory, a frustum per keyframe and at the current pose) through its front camera")
    ap.add_argument("--scene-dense", metavar="STEP", type=int, default=None,
                    help="--dump-scene also draws the dense cloud of the current frame, every STEP-th pixel (1 .. 16)")
    ap.add_argument("--scene-dense-lr", metavar="D", type=float, default=None,
                    help="--scene-dense / --scene-accumulate drop points whose left-right cross-check differs by more than D (> 0)")
    ap.add_argument("--scene-dense-max-depth", metavar="Z", type=float, default=0.0,
                    help="--scene-dense / --scene-accumulate drop points deeper than Z in the camera frame (0: none)")
    ap.add_argument("--scene-dense-sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--scene-dense / --scene-accumulate draw the clouds of the semi-globally aggregated map with these "
                         "penalties (and cost cap); --scene-dense-lr D is then the SGM map's own cross-check; needs a search_x <= 63")
    ap.add_argument("--scene-accumulate", metavar="N", type=int, default=0,
                    help="--dump-scene also draws the dense clouds of the keyframes so far, kept on the device in one array of "
                         "at most N records (oldest dropped first): the dense map growing")
    ap.add_argument("--dump-ar", metavar="DIR",
                    help="write per frame DIR/NNNNNN_ar.ppm: the AR demo's picture, a lit box standing in the world over the "
                         "frame's left image, seen from the tracked pose")
    ap.add_argument("--ar-box", metavar="SIZE", type=float, default=AR_BOX, help="edge of the box of --dump-ar, metres")
    ap.add_argument("--ar-occlude", metavar="STEP", type=int, default=None,
                    help="--dump-ar hides the box behind the frame's dense stereo depth, searched at every STEP-th pixel (1 .. 16), "
                         "and prints the covered and hidden pixels of every frame")
    ap.add_argument("--ar-hidden", choices=hip_lib.AR_HIDDEN, default="drop",
                    help="hidden pixels of --ar-occlude show the image (drop) or the box blended into it (dim)")
    ap.add_argument("--ar-alpha", metavar="A", type=int, default=128, help="--ar-hidden dim: the image's weight, 0 .. 256")
    ap.add_argument("--ar-margin", metavar="M", type=float, default=0.0,
                    help="--ar-occlude hides what lies more than M behind the scene's depth (the unit of the baseline)")
    ap.add_argument("--ar-lr", metavar="D", type=float, default=None,
                    help="--ar-occlude trusts only depths that pass the left-right check at tolerance D pixels")
    ap.add_argument("--ar-sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--ar-occlude hides the box behind the depth of the semi-globally aggregated map with these penalties "
                         "(and cost cap); --ar-lr D is then the SGM map's own cross-check; needs a search_x <= 63")
    ap.add_argument("--ar-at", metavar="X,Y,Z", default=",".join(str(x) for x in hip_lib.AR_AT),
                    help="world point of the box's centre (default: half a metre in front of the first camera, as the demo)")
    ap.add_argument("--dump-disparity", metavar="DIR",
                    help="write per frame DIR/NNNNNN_disparity.npy: the dense disparity map of the frame's rectified pair "
                         "(float32 [rows, cols]; -1 where the search window leaves the image)")
    ap.add_argument("--disparity-step", metavar="S", type=int, default=4, help="lattice of --dump-disparity: every S-th pixel, 1 .. 16")
    ap.add_argument("--disparity-depth", action="store_true", help="--dump-disparity writes depth, baseline / disparity (0: none)")
    ap.add_argument("--disparity-sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--dump-disparity aggregates semi-globally with these penalties (and cost cap) and writes "
                         "[2, rows, cols]: the sub-pixel value and the aggregated cost; needs a search_x <= 63; with "
                         "--disparity-lr D the SGM map is cross-checked by its own rule and the lr plane is stacked behind them")
    ap.add_argument("--disparity-lr", metavar="D", type=float, default=None,
                    help="--dump-disparity cross-checks left-right and writes [3, rows, cols]: the value (invalid where the "
                         "two searches differ by more than D; 0: report only), the cost and the lr plane")
    ap.add_argument("--dump-cloud", metavar="DIR",
                    help="write DIR/kfNNNNNN_cloud.ply whenever the newest keyframe changes: its dense coloured point cloud in "
                         "the world frame (binary little-endian PLY: x y z float, red green blue uchar)")
    ap.add_argument("--cloud-step", metavar="S", type=int, default=4, help="lattice of --dump-cloud: every S-th pixel, 1 .. 16")
    ap.add_argument("--cloud-lr", metavar="D", type=float, default=None,
                    help="--dump-cloud drops points whose left-right cross-check differs by more than D (> 0)")
    ap.add_argument("--cloud-sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--dump-cloud writes the clouds of the semi-globally aggregated map with these penalties (and cost cap); "
                         "--cloud-lr D is then the SGM map's own cross-check; needs a search_x <= 63")
    ap.add_argument("--cloud-max-depth", metavar="Z", type=float, default=0.0,
                    help="--dump-cloud drops points deeper than Z in the camera frame (0: none)")
    ap.add_argument("--dump-dense-map", metavar="FILE.ply",
                    help="fuse every new keyframe's dense cloud (--cloud-step, --cloud-lr, --cloud-max-depth) into a voxel map "
                         "kept inside the ctx and write it as one binary PLY at the end; needs --dense-map-voxel")
    ap.add_argument("--dense-map-sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--dump-dense-map / --scene-fused fuse the clouds of the semi-globally aggregated map with these penalties "
                         "(and cost cap): sub-pixel depth; --cloud-lr D is then the SGM map's own cross-check; needs a search_x <= 63")
    ap.add_argument("--dense-map-voxel", metavar="V", type=float, default=None, help="voxel edge of --dump-dense-map, metres (> 0)")
    ap.add_argument("--dense-map-log2", metavar="N", type=int, default=20, help="the map holds 1 << N entries (10 .. 26)")
    ap.add_argument("--dense-map-min-count", metavar="K", type=int, default=0,
                    help="--dump-dense-map / --scene-fused keep only voxels that at least K records fell into")
    ap.add_argument("--dense-map-window", metavar="METRES", type=float, default=None,
                    help="prune the map of --dump-dense-map / --scene-fused behind every fuse to the voxels within METRES of the "
                         "camera on every axis (floor(METRES / V) voxels around the camera's voxel): the map follows the camera")
    ap.add_argument("--dense-map-keep", metavar="N", type=int, default=None,
                    help="prune the map behind every fuse to the voxels that one of the last N fuses reached")
    ap.add_argument("--dense-map-carve", metavar="MARGIN", type=float, default=None,
                    help="carve the map of --dump-dense-map / --scene-fused in front of every fuse: a voxel leaves when the current "
                         "frame's dense depth (that of --dense-map-sgm, if given) measures a surface more than MARGIN metres behind it")
    ap.add_argument("--scene-fused", metavar="V", type=float, default=None,
                    help="--dump-scene also draws the fused dense map of voxel edge V (the map of --dump-dense-map), exported to "
                         "device memory whenever a keyframe was fused")
    ap.add_argument("--save-dense-map", metavar="FILE", default=None,
                    help="write the raw entries of the fused dense map (counts, sums and stamps, not the means) at the end of the run: "
                         "what --load-dense-map takes; needs --dense-map-voxel")
    ap.add_argument("--load-dense-map", metavar="FILE", default=None,
                    help="merge the entries of a --save-dense-map file into the empty map before the first fuse (the same voxel edge): "
                         "together with --save-dense-map a run continues yesterday's map")
    ap.add_argument("--dense-map-grow", metavar="N", type=int, default=None,
                    help="a dense map that is full moves into a larger table, one step of --dense-map-log2 at a time, up to 1 << N entries")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rate", type=float, default=20.0, help="frames per second of the time stamps")
    ap.add_argument("-t", "--trajectory", help="output CSV")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--keyframe-window", metavar="K", type=_keyframe_window, default=None,
                    help="keep only K retired keyframes (svo_ctx_set_keyframe_window): a replay of any length runs in "
                         "bounded device memory; the poses do not change. Default: keep every keyframe")
    return ap


def check_dense_map_args(ap, args):
    """what --dump-dense-map and --scene-fused need of each other and of their values (ap.error: exits with status 2)"""
    if args.dump_dense_map and args.dense_map_voxel is None:
        ap.error("--dump-dense-map needs --dense-map-voxel")
    if args.dense_map_voxel is not None and not (args.dump_dense_map or args.scene_fused is not None or args.save_dense_map):
        ap.error("--dense-map-voxel needs --dump-dense-map")
    for name, v in (("--dense-map-voxel", args.dense_map_voxel), ("--scene-fused", args.scene_fused)):
        if v is not None and not (v > 0 and v < float("inf")):
            ap.error(f"{name} must be a finite edge > 0")
    if args.scene_fused is not None and not args.dump_scene:
        ap.error("--scene-fused needs --dump-scene")
    if args.scene_fused is not None and args.dense_map_voxel is not None and args.scene_fused != args.dense_map_voxel:
        ap.error("--scene-fused and --dense-map-voxel name one map: give the same edge")
    if not 10 <= args.dense_map_log2 <= 26:
        ap.error("--dense-map-log2 must be 10 .. 26")
    if (args.save_dense_map or args.load_dense_map or args.dense_map_grow is not None) and args.dense_map_voxel is None and args.scene_fused is None:
        ap.error("--save-dense-map, --load-dense-map and --dense-map-grow need --dense-map-voxel")
    if args.dense_map_grow is not None and not args.dense_map_log2 <= args.dense_map_grow <= 26:
        ap.error("--dense-map-grow must be --dense-map-log2 .. 26")
    if args.dense_map_min_count < 0:
        ap.error("--dense-map-min-count must be >= 0")
    if (args.dense_map_window is not None or args.dense_map_keep is not None) and not (args.dump_dense_map or args.scene_fused is not None):
        ap.error("--dense-map-window and --dense-map-keep need --dump-dense-map or --scene-fused")
    if args.dense_map_carve is not None and not (args.dump_dense_map or args.scene_fused is not None):
        ap.error("--dense-map-carve needs --dump-dense-map or --scene-fused")
    if args.dense_map_carve is not None and not (0 <= args.dense_map_carve < float("inf")):
        ap.error("--dense-map-carve must be finite and >= 0")
    if args.dense_map_window is not None and not (0 <= args.dense_map_window < float("inf")):
        ap.error("--dense-map-window must be finite and >= 0")
    if args.dense_map_keep is not None and args.dense_map_keep < 1:
        ap.error("--dense-map-keep must be >= 1")
    if args.dense_map_sgm is not None and not (args.dump_dense_map or args.scene_fused is not None):
        ap.error("--dense-map-sgm needs --dump-dense-map or --scene-fused")
    if args.scene_dense_sgm is not None and args.scene_dense is None and args.scene_accumulate <= 0:
        ap.error("--scene-dense-sgm needs --scene-dense or --scene-accumulate")
    if args.ar_sgm is not None and args.ar_occlude is None:
        ap.error("--ar-sgm needs --ar-occlude")


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_dense_map_args(ap, args)

    gt = None
    rect = cal = None
    data = os.environ.get("SVO_DATA")
    fmt = None
    if data and not (args.synthetic or args.pairs or args.euroc or args.sbs or args.interleaved):
        if os.path.exists(os.path.join(data, "cam0", "data.csv")):
            args.euroc = data
        else:
            args.sbs = os.path.join(data, "%06d.png")
    if args.euroc and args.settings:
        settings = read_settings(args.settings)
        src = EurocInput(args.euroc, args.settings, raw=args.gpu_rectify or args.gpu_maps, host_maps=not args.gpu_maps)
        if args.gpu_maps:
            cal = src.gpu_calibration()
        elif args.gpu_rectify:
            rect = src.gpu_maps()
        n = min(args.frames, len(src))
        frames = (src.read(k) for k in range(n))
    elif args.sbs and args.settings:
        settings = read_settings(args.settings)
        src = SideBySideInput(args.sbs, args.frames, args.rate, raw=args.gpu_ingest)
        fmt = src.input_format() if args.gpu_ingest else None
        frames = (src.read(k) for k in range(args.frames))
    elif args.interleaved and args.settings:
        settings = read_settings(args.settings)
        src = InterleavedInput(args.interleaved, args.frames, args.rate, raw=args.gpu_ingest)
        fmt = src.input_format() if args.gpu_ingest else None
        frames = (src.read(k) for k in range(args.frames))
    elif args.synthetic:
        cfg, L, R, gt, ts = synth.make_sequence(args.synthetic, args.frames, args.seed, device="cpu")
        settings = read_settings(args.settings) if args.settings else cfg
        frames = ((L[k].numpy(), R[k].numpy(), float(ts[k])) for k in range(args.frames))
    elif args.pairs and args.settings:
        settings = read_settings(args.settings)
        frames = ((*_load_pair(args.pairs, k), k / args.rate) for k in range(args.frames))
    else:
        ap.error("give --synthetic, or --settings with --euroc / --sbs / --interleaved / --pairs (or $SVO_DATA)")
    if args.gpu_rectify and rect is None and cal is None:
        ap.error("--gpu-rectify needs --euroc with --settings")
    if args.gpu_maps and cal is None:
        ap.error("--gpu-maps needs --euroc with --settings")
    if args.gpu_ingest and fmt is None:
        ap.error("--gpu-ingest needs --sbs or --interleaved with --settings")
    if args.gpu_imu and not args.gyro:
        ap.error("--gpu-imu needs --gyro")
    gyro = np.loadtxt(args.gyro, ndmin=2) if args.gyro else None
    occlusion = None
    if args.ar_occlude is not None:
        if not args.dump_ar:
            ap.error("--ar-occlude needs --dump-ar")
        if not 1 <= args.ar_occlude <= 16 or not 0 <= args.ar_alpha <= 256 or not 0 <= args.ar_margin < float("inf"):
            ap.error("--ar-occlude must be 1 .. 16, --ar-alpha 0 .. 256 and --ar-margin finite and >= 0")
        if args.ar_lr is not None and not 0 < args.ar_lr < float("inf"):
            ap.error("--ar-lr must be a finite tolerance > 0")
        occlusion = dict(step=args.ar_occlude, hidden=args.ar_hidden, alpha=args.ar_alpha, margin=args.ar_margin, lr_check=args.ar_lr or 0.0)
    split = lambda spec: None if spec is None else spec.split(",")
    for flag, spec in (("--dense-map-sgm", args.dense_map_sgm), ("--scene-dense-sgm", args.scene_dense_sgm), ("--ar-sgm", args.ar_sgm)):
        if spec is not None and int(settings["search_x"]) > 63:
            ap.error(f"{flag} needs a search_x <= 63 (the settings have {int(settings['search_x'])})")
    rp = Replay(settings, args.device, args.time_trace, args.fast, rectify_maps=rect, input_format=fmt, gpu_imu=args.gpu_imu,
                dump_views=args.dump_views, dump_scene=args.dump_scene, calibration=cal, dump_ar=args.dump_ar,
                ar_box=args.ar_box, ar_at=tuple(float(x) for x in args.ar_at.split(",")),
                keyframe_window=args.keyframe_window, dump_disparity=args.dump_disparity, disparity_step=args.disparity_step,
                disparity_depth=args.disparity_depth, dump_cloud=args.dump_cloud, cloud_step=args.cloud_step,
                cloud_max_depth=args.cloud_max_depth, disparity_lr=args.disparity_lr, cloud_lr=args.cloud_lr,
                disparity_sgm=None if args.disparity_sgm is None else args.disparity_sgm.split(","),
                cloud_sgm=None if args.cloud_sgm is None else args.cloud_sgm.split(","),
                scene_dense=args.scene_dense, scene_dense_lr=args.scene_dense_lr, scene_dense_max_depth=args.scene_dense_max_depth,
                scene_accumulate=args.scene_accumulate, dump_dense_map=args.dump_dense_map, dense_map_voxel=args.dense_map_voxel,
                dense_map_log2=args.dense_map_log2, dense_map_min_count=args.dense_map_min_count, dense_map_window=args.dense_map_window,
                dense_map_keep=args.dense_map_keep, dense_map_carve=args.dense_map_carve, scene_fused=args.scene_fused,
                save_dense_map=args.save_dense_map, load_dense_map=args.load_dense_map, dense_map_grow=args.dense_map_grow,
                ar_occlusion=occlusion, dense_map_sgm=split(args.dense_map_sgm), scene_dense_sgm=split(args.scene_dense_sgm),
                ar_sgm=split(args.ar_sgm))
    for k, (left, right, t) in enumerate(frames):
        rp.feed(left, right, t, None if gyro is None else gyro[gyro[:, 0] == k, 1:4])
    rp.finish()
    rows = rp.rows()
    print(f"frames {rows.shape[0]}  Average FPS: {fps_from_csv_rows(rows):.2f}  "
          f"keyframes {rp.slam.num_keyframes()}")
    if gt is not None:
        ref = np.array([[0, p[0], p[1], p[2], *csv_angles(p)] for p in gt])
        ref[:, 0] = rows[:, 0]
        rep = error_report(rows, ref)
        print("max  |err| x y z [m] rx ry rz [deg]:", " ".join(f"{v:.3f}" for v in rep["max"]))
        print("mean |err|                          :", " ".join(f"{v:.3f}" for v in rep["mean"]))
    if args.trajectory:
        rp.write(args.trajectory)


if __name__ == "__main__":
    main()
