"""The AR picture (svo_submit_export_ar, svo_render_ar) restated in numpy from include/svo_hip.h's "ar" section alone:
the camera of a pose, a vertex, a triangle's drop rules, snap, int64 edge functions at the pixel centres, the depth
and the flat colour in np.float32 in the order written, and a sequential "a smaller key replaces" loop over the
triangles. The pixels of one triangle's box are evaluated together (int64 / float32 arrays: the same per-pixel
arithmetic). The tests compare the library with it byte for byte."""
import numpy as np

import oracle_py as O

F = np.float32
RGB8, RGBA8 = 1, 2
BYTES = {RGB8: 3, RGBA8: 4}
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LIMIT = F(32768.0)


def size(width, height, pixel):
    """(pitch, image_bytes)"""
    pitch = width * BYTES[pixel]
    return pitch, (height * pitch + 255) // 256 * 256


def camera_of_pose(pose, fx, fy, cx, cy):
    """float32 [16]: the bytes of svo_ar_camera at pose (t, r)"""
    pose = np.asarray(pose, F)
    R = O.rodrigues(pose[3:6]).astype(F).reshape(9)      # the float `rot` of PoseManager::set_pose
    view = np.zeros(12, F)
    with np.errstate(all="ignore"):
        for k in range(3):
            for j in range(3):
                view[4 * k + j] = R[3 * j + k]
            view[4 * k + 3] = -(((R[k] * pose[0]) + (R[3 + k] * pose[1])) + (R[6 + k] * pose[2]))
    return np.concatenate([view, np.asarray([fx, fy, cx, cy], F)])


def transform(m, v):
    """o_k = ((m[4k] * x + m[4k+1] * y) + m[4k+2] * z) + m[4k+3] in float32"""
    m, v = np.asarray(m, F).reshape(12), np.asarray(v, F)
    return np.array([((m[4 * k] * v[0] + m[4 * k + 1] * v[1]) + m[4 * k + 2] * v[2]) + m[4 * k + 3] for k in range(3)], F)


def shade_colour(w, rgb, light, ambient):
    """the flat colour r' << 16 | g' << 8 | b' of a triangle with world vertices w [3, 3]"""
    light, ambient = np.asarray(light, F), F(ambient)
    e1, e2 = w[1] - w[0], w[2] - w[0]
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F)
    q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    d = (n[0] * light[0] + n[1] * light[1]) + n[2] * light[2]
    with np.errstate(all="ignore"):
        t = np.abs(d) / np.sqrt(q)
    s = F(0) if (q == 0 or np.isnan(t)) else (t if t < 1 else F(1))
    shade = ambient + (F(1) - ambient) * s
    out = 0
    for sh in (16, 8, 0):
        c = F((rgb >> sh) & 255)
        out |= min(255, int(c * shade + F(0.5))) << sh
    return out


def screen_triangle(cam, model, verts, rgb, light, ambient, near):
    """the screen record of one triangle: None when it is dropped, else (X [3], Y [3], c2 [3] float32, colour)"""
    cam = np.asarray(cam, F)
    view, fx, fy, cx, cy = cam[:12], cam[12], cam[13], cam[14], cam[15]
    with np.errstate(all="ignore"):
        w = np.array([transform(model, v) for v in verts], F)
        c = np.array([transform(view, x) for x in w], F)
        if not (np.isfinite(w).all() and np.isfinite(c).all()):
            return None
        if (c[:, 2] < F(near)).any():
            return None
        u = (fx * c[:, 0]) / c[:, 2] + cx
        v = (fy * c[:, 1]) / c[:, 2] + cy
        if not ((np.abs(u) < LIMIT).all() and (np.abs(v) < LIMIT).all()):
            return None
        X = np.floor(u * F(16)).astype(np.int64)
        Y = np.floor(v * F(16)).astype(np.int64)
        return X, Y, c[:, 2].copy(), shade_colour(w, rgb, light, ambient)


def offer(keys, rec, depth=None):
    """one screen record into the key plane uint64 [H, W]: a smaller key replaces. depth: float32 [H, W] or None,
    receives the smallest z offered per pixel (for the tests of the depth rule). Returns the pixels covered."""
    X, Y, c2, colour = rec
    H, W = keys.shape
    A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if A == 0:
        return 0
    # the pixels whose centres lie in the bounding box (everything outside cannot be covered)
    x0, x1 = max(int(-((-(X.min() - 8)) // 16)), 0), min(int((X.max() - 8) // 16), W - 1)
    y0, y1 = max(int(-((-(Y.min() - 8)) // 16)), 0), min(int((Y.max() - 8) // 16), H - 1)
    if x0 > x1 or y0 > y1:
        return 0
    px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64), np.arange(y0, y1 + 1, dtype=np.int64))
    Px, Py = 16 * px + 8, 16 * py + 8
    E = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        E.append((X[b] - X[a]) * (Py - Y[a]) - (Y[b] - Y[a]) * (Px - X[a]))
    assert (E[0] + E[1] + E[2] == A).all()
    if A < 0:
        E, A = [-e for e in E], -A
    covered = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
    fA = np.int64(A).astype(F)
    l = [e.astype(F) / fA for e in E]
    z = (l[0] * c2[0] + l[1] * c2[1]) + l[2] * c2[2]
    assert z.dtype == F
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(colour)
    sub = keys[y0:y1 + 1, x0:x1 + 1]
    take = covered & (key < sub)
    sub[take] = key[take]
    if depth is not None:
        dsub = depth[y0:y1 + 1, x0:x1 + 1]
        lower = covered & (z < dsub)
        dsub[lower] = z[lower]
    return int(covered.sum())


def draw_triangles(draws):
    """(model, vertices [3, 3], rgb) of every triangle of draws = [(model [12], vertices [V, 3], triangles [T, 3],
    rgb [T] or None, the instance's colour)]; a triangle with a vertex index out of range gives vertices None"""
    for model, vertices, triangles, rgb, rgb_all in draws:
        vertices = np.asarray(vertices, F).reshape(-1, 3)
        for t, tri in enumerate(np.asarray(triangles, np.int64).reshape(-1, 3)):
            ok = ((tri >= 0) & (tri < len(vertices))).all()
            yield model, (vertices[tri] if ok else None), int(rgb_all if rgb is None else rgb[t])


def key_plane(height, width, cam, draws, light, ambient, near, order=None, depth=None):
    """uint64 [H, W]: the smallest key per pixel (EMPTY: nobody covers); order: a permutation of the triangles"""
    keys = np.full((height, width), EMPTY, np.uint64)
    tris = list(draw_triangles(draws))
    for i in (range(len(tris)) if order is None else order):
        model, verts, rgb = tris[i]
        rec = None if verts is None else screen_triangle(cam, model, verts, rgb, light, ambient, near)
        if rec is not None:
            offer(keys, rec, depth)
    return keys


def compose(gray, keys, pixel):
    """uint8 [H, W, 3 | 4]: the colour of the key, or (g, g, g) of the gray plane where the key is EMPTY"""
    H, W = keys.shape
    out = np.empty((H, W, BYTES[pixel]), np.uint8)
    out[..., :3] = np.asarray(gray, np.uint8)[:H, :W, None]
    hit = keys != EMPTY
    low = (keys & np.uint64(0xFFFFFF)).astype(np.uint32)
    for ch, sh in enumerate((16, 8, 0)):
        out[..., ch][hit] = ((low >> sh) & 255).astype(np.uint8)[hit]
    if pixel == RGBA8:
        out[..., 3] = 255
    return out


def render(gray, cam, draws, light, ambient, near, pixel, order=None):
    """the image of one slot / one image of the stage entry: uint8 [H, W, 3 | 4]"""
    H, W = np.asarray(gray).shape
    return compose(gray, key_plane(H, W, cam, draws, light, ambient, near, order), pixel)
