"""The occluded AR picture (svo_submit_export_ar_occluded, svo_render_ar_occluded) restated in numpy from
include/svo_hip.h's "ar occlusion" section alone, on top of ar_ref (key_plane, compose): the occluder of a pixel, the
hidden winner, drop and dim, and the two counts. render() tests the winner of every pixel, as the statement does;
render_fragments() is a second, scalar form that tests every covering fragment of every pixel on its own, with its own
pixel -> cell arithmetic. The tests compare the library with the first byte for byte, and the two with each other."""
import numpy as np

import ar_ref as AR

F = np.float32
DROP, DIM = 0, 1
DROPPED = 0x80                                             # SVO_CLOUD_DROPPED
MAP_POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("color", "u1", (3,)), ("flags", "u1")])
VISIBILITY = np.dtype([("status", "<i4"), ("occluder_points", "<i4"), ("covered", "<i8"), ("hidden", "<i8"), ("_pad", "<i8")])
assert MAP_POINT.itemsize == 16 and VISIBILITY.itemsize == 32


def occludes(rec, drop_flags):
    """bool, per record: it has an occluder depth (neither dropped nor a drop_flags bit; z finite and > 0)"""
    z = rec["z"]
    with np.errstate(invalid="ignore"):
        return ((rec["flags"] & np.uint8((DROPPED | drop_flags) & 0xff)) == 0) & np.isfinite(z) & (z > 0)


def occluder_plane(H, W, lattice, drop_flags=0):
    """float32 [H, W]: the occluder depth zo of every pixel, +inf where nothing occludes. lattice: None, or (records
    MAP_POINT [rows * cols], cols, rows, step)"""
    zo = np.full((H, W), np.inf, F)
    if lattice is None:
        return zo
    rec, cols, rows, step = lattice
    rec = np.asarray(rec).reshape(rows, cols)
    cell = np.where(occludes(rec, drop_flags), rec["z"], F(np.inf)).astype(F)
    iy, ix = np.arange(H) // step, np.arange(W) // step
    ys, xs = np.nonzero(iy < rows)[0], np.nonzero(ix < cols)[0]
    zo[np.ix_(ys, xs)] = cell[np.ix_(iy[ys], ix[xs])]
    return zo


def depth_of(keys):
    """float32: the float whose bits are key >> 32 (meaningless where the key is EMPTY)"""
    return (keys >> np.uint64(32)).astype(np.uint32).view(F)


def hidden_plane(keys, zo, margin):
    """(covered, hidden) bool [H, W]: a winner; a winner with z > zo + margin (one float32 add, one comparison)"""
    covered = keys != AR.EMPTY
    with np.errstate(all="ignore"):
        limit = zo + F(margin)
        assert limit.dtype == F
        hidden = covered & (depth_of(keys) > limit)
    return covered, hidden


def dim(channel, gray, alpha):
    """(c' * (256 - a) + g * a + 128) >> 8 in integers"""
    return ((channel.astype(np.int64) * (256 - alpha) + gray.astype(np.int64) * alpha + 128) >> 8).astype(np.uint8)


def compose(gray, keys, pixel, hidden, mode, alpha):
    """uint8 [H, W, 3 | 4]: ar_ref.compose, then the hidden pixels: the background (drop) or every channel dimmed"""
    out = AR.compose(gray, keys, pixel)
    H, W = keys.shape
    g = np.asarray(gray, np.uint8)[:H, :W]
    for ch in range(3):
        plane = out[..., ch]
        plane[hidden] = g[hidden] if mode == DROP else dim(plane[hidden], g[hidden], alpha)
    return out


def render(gray, cam, draws, light, ambient, near, pixel, lattice, mode=DROP, alpha=128, margin=0.0, drop_flags=0, order=None):
    """(image uint8 [H, W, 3 | 4], covered, hidden) of one image: the winner of every pixel against its occluder"""
    H, W = np.asarray(gray).shape
    keys = AR.key_plane(H, W, cam, draws, light, ambient, near, order)
    covered, hidden = hidden_plane(keys, occluder_plane(H, W, lattice, drop_flags), margin)
    return compose(gray, keys, pixel, hidden, mode, alpha), int(covered.sum()), int(hidden.sum())


def render_fragments(gray, cam, draws, light, ambient, near, pixel, lattice, mode=DROP, alpha=128, margin=0.0, drop_flags=0):
    """the same three, the long way: every covering fragment of every pixel is tested against the pixel's occluder
    by itself; the pixel shows the smallest key among the fragments that are not hidden, and is hidden when it is
    covered and none is left (drop: the background; dim: the smallest key of all, dimmed)"""
    gray = np.asarray(gray, np.uint8)
    H, W = gray.shape
    everyone = np.full((H, W), AR.EMPTY, np.uint64)
    visible = np.full((H, W), AR.EMPTY, np.uint64)
    for model, verts, rgb in AR.draw_triangles(draws):
        rec = None if verts is None else AR.screen_triangle(cam, model, verts, rgb, light, ambient, near)
        if rec is None:
            continue
        mine = np.full((H, W), AR.EMPTY, np.uint64)
        AR.offer(mine, rec)
        for py, px in zip(*np.nonzero(mine != AR.EMPTY)):
            key = mine[py, px]
            everyone[py, px] = min(everyone[py, px], key)
            z = np.array([int(key) >> 32], np.uint32).view(F)[0]
            hide = False
            if lattice is not None:
                records, cols, rows, step = lattice
                ix, iy = int(px) // step, int(py) // step
                if ix < cols and iy < rows:
                    r = records[iy * cols + ix]
                    zo = F(r["z"])
                    if not (int(r["flags"]) & (DROPPED | drop_flags)) and np.isfinite(zo) and zo > 0:
                        with np.errstate(over="ignore"):
                            hide = bool(z > F(zo + F(margin)))
            if not hide:
                visible[py, px] = min(visible[py, px], key)
    covered = everyone != AR.EMPTY
    hidden = covered & (visible == AR.EMPTY)
    out = AR.compose(gray, visible, pixel)
    if mode == DIM:
        dimmed = AR.compose(gray, everyone, pixel)
        for ch in range(3):
            out[..., ch][hidden] = dim(dimmed[..., ch][hidden], gray[:H, :W][hidden], alpha)
    return out, int(covered.sum()), int(hidden.sum())
