"""The scene (svo_submit_export_scenes, svo_render_scene) restated in numpy: the camera, points and lines of
include/svo_hip.h's "scene" section in np.float32, a plain per-element, per-pixel loop with a sequential depth compare.
Written from the header alone; the tests compare the library with it byte for byte. Frusta come from
oracle_py.rodrigues, the point filter from map_ref."""
import numpy as np

import map_ref as MR
import oracle_py as O

F = np.float32
RGB8, RGBA8 = 1, 2
BYTES = {RGB8: 3, RGBA8: 4}
POINTS, TRAJECTORY, KEYFRAMES, POSE = 1, 2, 4, 8
CLASS_POSE, CLASS_KEYFRAME, CLASS_TRAJECTORY, CLASS_POINT = range(4)
FRUSTUM_EDGES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1))
VIEWER_DIMS = (0.1, 0.08, 0.07)
PRESETS = dict(front=((0, 0, -1), (0, 0, 0), (0, -1, 0)), top=((0, -5, 0), (0, 0, 0), (0, 0, 1)),
               side=((-5, 0, 0), (0, 0, 0), (0, -1, 0)))


def size(cols, rows, pixel):
    """(pitch, image_bytes)"""
    pitch = cols * BYTES[pixel]
    return pitch, (rows * pitch + 255) // 256 * 256


def camera(view, f, cx, cy, near):
    """float32 [16]: the bytes of svo_scene_camera"""
    return np.concatenate([np.asarray(view, F).reshape(12), np.asarray([f, cx, cy, near], F)])


def look_at(eye, centre, up, fov_y_deg, cols, rows, near):
    """svo_scene_look_at in float64: (view [3, 4], f, cx, cy, near), not rounded to float32"""
    eye, centre, up = (np.asarray(v, np.float64) for v in (eye, centre, up))
    z = centre - eye
    z = z / np.sqrt(z @ z)
    x = np.cross(-up, z)
    x = x / np.sqrt(x @ x)
    y = np.cross(z, x)
    view = np.zeros((3, 4))
    for k, a in enumerate((x, y, z)):
        view[k, :3] = a
        view[k, 3] = -(a @ eye)
    return view, (rows / 2) / np.tan(np.deg2rad(np.float64(fov_y_deg)) / 2), cols / 2, rows / 2, near


def frustum(pose, dims=VIEWER_DIMS):
    """float32 [8, 6]: the world lines of the frustum of pose (t, r)"""
    pose = np.asarray(pose, F)
    R = O.rodrigues(pose[3:6]).astype(F)                 # the float `rot` of PoseManager::set_pose
    w, h, d = (F(v) for v in dims)
    verts = ((F(0), F(0), F(0)), (-w, h, d), (-w, -h, d), (w, -h, d), (w, h, d))
    world = np.zeros((5, 3), F)
    with np.errstate(all="ignore"):
        for i, v in enumerate(verts):
            for k in range(3):
                world[i, k] = ((R[k, 0] * v[0] + R[k, 1] * v[1]) + R[k, 2] * v[2]) + pose[k]
    return np.array([np.concatenate([world[a], world[b]]) for a, b in FRUSTUM_EDGES], F)


def line_records(lines, cls, rgb):
    """[(a [3], b [3], cls << 24 | rgb)] of float32 [m, 6] lines"""
    return [(np.asarray(l[:3], F), np.asarray(l[3:6], F), cls << 24 | rgb) for l in lines]


def slot_lines(trajectory, keyframe_poses, pose, show, trajectory_rgb, keyframe_rgb, pose_rgb, dims=VIEWER_DIMS,
               trajectory_tail=0):
    """the lines of a slot: trajectory [n, >= 3] (the poses of svo_get_trajectory), the poses of the keyframes from
    from_keyframe on, the current pose. Returns (records, trajectory poses drawn)"""
    out, n_poses = [], 0
    if show & TRAJECTORY:
        t = np.asarray(trajectory, F).reshape(-1, 6)[:, :3]
        if trajectory_tail > 0:
            t = t[max(0, len(t) - trajectory_tail):]
        n_poses = len(t)
        out += line_records([np.concatenate([t[j], t[j + 1]]) for j in range(len(t) - 1)], CLASS_TRAJECTORY, trajectory_rgb)
    if show & KEYFRAMES:
        for p in keyframe_poses:
            out += line_records(frustum(p, dims), CLASS_KEYFRAME, keyframe_rgb)
    if show & POSE:
        out += line_records(frustum(pose, dims), CLASS_POSE, pose_rgb)
    return out, n_poses


def transform(cam, p):
    """c = T(p), float32 [3]"""
    V = cam[:12]
    x, y, z = (F(v) for v in p)
    return np.array([((V[4 * k] * x + V[4 * k + 1] * y) + V[4 * k + 2] * z) + V[4 * k + 3] for k in range(3)], F)


def project(cam, c):
    """(floor(u), floor(v)) or None (the 2^15 rule)"""
    f, cx, cy = cam[12], cam[13], cam[14]
    u = (f * c[0]) / c[2] + cx
    v = (f * c[1]) / c[2] + cy
    if not (abs(u) < 32768 and abs(v) < 32768):
        return None
    return int(np.floor(u)), int(np.floor(v))


def rdiv(p, n):
    return (2 * p + n) // (2 * n)


def line_pixels(X0, Y0, X1, Y1):
    """the n + 1 pixels of a projected line"""
    dx, dy = X1 - X0, Y1 - Y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(X0, Y0)]
    return [(X0 + rdiv(i * dx, n), Y0 + rdiv(i * dy, n)) for i in range(n + 1)]


def point_element(cam, p, rgb, s):
    """the covered pixels of a point as [(x, y, depth float32, low word)] (empty: dropped)"""
    with np.errstate(all="ignore"):
        c = transform(cam, p)
        if not np.all(np.isfinite(c)) or not c[2] >= cam[15]:
            return []
        at = project(cam, c)
    if at is None:
        return []
    x0, y0 = at[0] - (s - 1) // 2, at[1] - (s - 1) // 2
    low = CLASS_POINT << 24 | int(rgb[0]) << 16 | int(rgb[1]) << 8 | int(rgb[2])
    return [(x, y, c[2], low) for y in range(y0, y0 + s) for x in range(x0, x0 + s)]


def line_element(cam, A, B, low, cols, rows):
    """the pixels of a line inside the image as [(x, y, depth float32, low word)] (empty: dropped)"""
    near = cam[15]
    with np.errstate(all="ignore"):
        a, b = transform(cam, A), transform(cam, B)
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
            return []
        a_near, b_near = a[2] < near, b[2] < near
        if a_near and b_near:
            return []
        if a_near or b_near:
            if b_near:
                a, b = b, a                               # (a is the near end; swapped back below)
            t = (near - a[2]) / (b[2] - a[2])
            a = np.array([a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), near], F)
            if not np.all(np.isfinite(a)):
                return []
            if b_near:
                a, b = b, a
        pa, pb = project(cam, a), project(cam, b)
        if pa is None or pb is None:
            return []
        pix = line_pixels(pa[0], pa[1], pb[0], pb[1])
        n = len(pix) - 1
        out = []
        for i, (x, y) in enumerate(pix):
            if 0 <= x < cols and 0 <= y < rows:
                z = a[2] if n == 0 else a[2] + (b[2] - a[2]) * (F(i) / F(n))
                out.append((x, y, F(z), int(low)))
    return out


def elements(cols, rows, cam, sets, lines, filt, point_size):
    """every element of an image as a list of its (x, y, depth, low) inside the image. sets: map_ref sets (n,
    own_id, kps3d [n, 3] float32 or their bits, planes with flags, keyframe_id, inlier_count, color); lines: (a, b,
    cls_rgb) records"""
    out = []
    for n, own_id, k3, planes in sets:
        p = {k: np.asarray(v)[:n] for k, v in planes.items()}
        keep = MR.keep_mask(p, own_id, filt)
        xyz = np.ascontiguousarray(k3)[:n].view(F).reshape(-1, 3)
        col = np.asarray(p["color"]).view(np.uint32)
        for i in np.nonzero(keep)[0]:
            rgb = (col[i] & 0xff, (col[i] >> 8) & 0xff, (col[i] >> 16) & 0xff)
            e = [q for q in point_element(cam, xyz[i], rgb, point_size) if 0 <= q[0] < cols and 0 <= q[1] < rows]
            if e:
                out.append(e)
    for A, B, low in lines:
        e = line_element(cam, A, B, low, cols, rows)
        if e:
            out.append(e)
    return out


def _image(cols, rows, pixel, low, covered, background):
    img = np.zeros((rows, cols, BYTES[pixel]), np.uint8)
    word = np.where(covered, low & 0xffffff, background).astype(np.uint32)
    for c in range(3):
        img[:, :, c] = (word >> (16 - 8 * c)) & 0xff
    if pixel == RGBA8:
        img[:, :, 3] = 255
    return img


def render(cols, rows, pixel, cam, sets, lines, filt=MR.KEEP_ALL, point_size=1, background=0xffffff):
    """uint8 [rows, cols, 3 | 4]: element after element, pixel after pixel, a depth buffer: an element replaces what a
    pixel shows if it is nearer, or equally near and of a smaller class, or of the same class and a smaller colour"""
    depth = np.full((rows, cols), np.inf, np.float64)
    low = np.zeros((rows, cols), np.uint32)
    covered = np.zeros((rows, cols), bool)
    for e in elements(cols, rows, cam, sets, lines, filt, point_size):
        for x, y, z, w in e:
            if not covered[y, x] or z < depth[y, x] or (z == depth[y, x] and w < low[y, x]):
                depth[y, x], low[y, x], covered[y, x] = z, w, True
    return _image(cols, rows, pixel, low, covered, background)


def render_smallest_key(cols, rows, pixel, cam, sets, lines, filt=MR.KEEP_ALL, point_size=1, background=0xffffff, rng=None):
    """the same picture as "the smallest 64-bit key wins", the elements in a shuffled order"""
    key = np.full((rows, cols), 2**64 - 1, np.uint64)
    el = elements(cols, rows, cam, sets, lines, filt, point_size)
    for j in (rng.permutation(len(el)) if rng is not None else range(len(el))):
        for x, y, z, w in el[j]:
            k = np.uint64(int(F(z).view(np.uint32)) << 32 | w)
            key[y, x] = min(key[y, x], k)
    return _image(cols, rows, pixel, (key & np.uint64(0xffffffff)).astype(np.uint32), key != np.uint64(2**64 - 1), background)
