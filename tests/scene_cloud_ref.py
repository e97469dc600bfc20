"""Cloud points in the scene (svo_submit_export_scenes_clouds, svo_render_scene_clouds) restated in numpy, on top of
scene_ref.py: the "scene clouds" section of include/svo_hip.h and nothing else. A cloud point is a svo_map_point
record that goes through scene_ref's transform and project as a keypoint does and offers the key of class 4. Two forms
of the picture: element after element with a sequential depth compare, and "the smallest 64-bit key wins" in any
order."""
import numpy as np

import map_ref as MR
import scene_ref as SR

F = np.float32
CLASS_CLOUD = 4
CLOUD_DROPPED = 0x80
MAP_POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("color", "u1", (3,)), ("flags", "u1")])
assert MAP_POINT.itemsize == 16


def records(xyz, color=None, flags=None):
    """svo_map_point records of the points xyz [n, 3]; color [n, 3] (r, g, b) or [n] words r << 16 | g << 8 | b"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    r = np.zeros(len(xyz), MAP_POINT)
    r["x"], r["y"], r["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if color is not None:
        color = np.asarray(color)
        if color.ndim == 1:
            color = np.stack([(color >> 16) & 0xff, (color >> 8) & 0xff, color & 0xff], 1)
        r["color"] = color.astype(np.uint8)
    if flags is not None:
        r["flags"] = np.asarray(flags, np.uint8)
    return r


def cloud_point(cam, rec, s):
    """the pixels a record covers as [(x, y, depth float32, low word)], not clipped to an image (empty: dropped by
    the point rule; the flags are the caller's business)"""
    with np.errstate(all="ignore"):
        c = SR.transform(cam, (rec["x"], rec["y"], rec["z"]))
        if not np.all(np.isfinite(c)) or not c[2] >= cam[15]:
            return []
        at = SR.project(cam, c)
    if at is None:
        return []
    x0, y0 = at[0] - (s - 1) // 2, at[1] - (s - 1) // 2
    r, g, b = (int(v) for v in rec["color"])
    low = CLASS_CLOUD << 24 | r << 16 | g << 8 | b
    return [(x, y, c[2], low) for y in range(y0, y0 + s) for x in range(x0, x0 + s)]


def cloud_elements(cols, rows, cam, spans, drop_flags, s):
    """every drawn cloud point of the spans (arrays of MAP_POINT) as the list of its pixels inside the image"""
    out = []
    for span in spans:
        for rec in np.asarray(span).view(MAP_POINT).reshape(-1):
            flags = int(rec["flags"])
            if flags & CLOUD_DROPPED or flags & int(drop_flags):
                continue
            e = [q for q in cloud_point(cam, rec, s) if 0 <= q[0] < cols and 0 <= q[1] < rows]
            if e:
                out.append(e)
    return out


def elements(cols, rows, cam, sets, lines, spans, filt, point_size, cloud_size):
    """the elements of "scene" (scene_ref.elements) and the cloud points"""
    return SR.elements(cols, rows, cam, sets, lines, filt, point_size) + \
        cloud_elements(cols, rows, cam, spans, filt.get("drop_flags", 0), cloud_size)


def depth_buffer(cols, rows, els):
    """(low words uint32 [rows, cols], covered bool [rows, cols]): element after element, pixel after pixel; an element
    replaces what a pixel shows if it is nearer, or equally near and of a smaller class, or of the same class and a
    smaller colour"""
    depth = np.full((rows, cols), np.inf, np.float64)
    low = np.zeros((rows, cols), np.uint32)
    covered = np.zeros((rows, cols), bool)
    for e in els:
        for x, y, z, w in e:
            if not covered[y, x] or z < depth[y, x] or (z == depth[y, x] and w < low[y, x]):
                depth[y, x], low[y, x], covered[y, x] = z, w, True
    return low, covered


def smallest_key(cols, rows, els, rng=None):
    """the same two planes as "the smallest key wins", the elements in a shuffled order"""
    key = np.full((rows, cols), 2**64 - 1, np.uint64)
    for j in (rng.permutation(len(els)) if rng is not None else range(len(els))):
        for x, y, z, w in els[j]:
            key[y, x] = min(key[y, x], np.uint64(int(F(z).view(np.uint32)) << 32 | w))
    return (key & np.uint64(0xffffffff)).astype(np.uint32), key != np.uint64(2**64 - 1)


def picture(cols, rows, pixel, low, covered, background=0xffffff):
    """uint8 [rows, cols, 3 | 4] of the two planes"""
    return SR._image(cols, rows, pixel, low, covered, background)


def classes(low, covered):
    """int [rows, cols]: the class that won each pixel, -1 for the background"""
    return np.where(covered, (low >> 24).astype(np.int64), -1)


def render(cols, rows, pixel, cam, sets, lines, spans, filt=MR.KEEP_ALL, point_size=1, cloud_size=1, background=0xffffff):
    """the picture in the depth-buffer form"""
    low, covered = depth_buffer(cols, rows, elements(cols, rows, cam, sets, lines, spans, filt, point_size, cloud_size))
    return picture(cols, rows, pixel, low, covered, background)


def render_smallest_key(cols, rows, pixel, cam, sets, lines, spans, filt=MR.KEEP_ALL, point_size=1, cloud_size=1,
                        background=0xffffff, rng=None):
    """the picture in the smallest-key form"""
    low, covered = smallest_key(cols, rows, elements(cols, rows, cam, sets, lines, spans, filt, point_size, cloud_size), rng)
    return picture(cols, rows, pixel, low, covered, background)
