"""Crafted images, triangles and occluder lattices for the occluded AR picture ("ar occlusion", include/svo_hip.h) at
the smallest shapes that can go wrong. A case is a dict: name, W, H, gray [H, W], cam, draws (ar_ref's), light,
ambient, near, lattice (records, cols, rows, step) or None, margin, drop_flags, and probes: (kind, px, py, hidden)
names a pixel that a listed boundary or a non-occluding kind of record decides, and what the statement says of it.
Every lattice hides the meshes where its plain cells are near (z = NEAR_Z) and shows them where they are far (FAR_Z);
the probes sit in cells of their own inside the near part, so that a wrong rule changes the picture there."""
import numpy as np

import ar_occlusion_ref as OR
import ar_ref as AR

F = np.float32
LIGHT, AMBIENT, NEAR = (0.0, 0.0, 1.0), 0.25, 0.01
I12 = np.eye(3, 4, dtype=F).ravel()
PIX = np.concatenate([I12, np.asarray([1, 1, 0, 0], F)])   # a vertex (u z, v z, z) lands on (u, v) at depth z
NEAR_Z, FAR_Z = F(0.25), F(100.0)                          # every mesh below lies between them
FLAG = 0x04                                                # the drop_flags bit of the cases that have one
NON_OCCLUDING = ("dropped", "drop_flags", "z zero", "z negative", "z inf", "z nan")
BOUNDARIES = ("equal", "ulp above", "ulp below")


def tri(p0, p1, p2, z=(1.0, 1.0, 1.0)):
    """three vertices that PIX projects to the pixel coordinates p at depths z"""
    return [(F(p[0]) * F(d), F(p[1]) * F(d), F(d)) for p, d in zip((p0, p1, p2), z)]


def mesh(tris, rgb=None, rgb_all=0xc08040, model=I12):
    """a draw of independent triangles (vertices three by three)"""
    v = np.asarray([p for t in tris for p in t], F).reshape(-1, 3)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return (np.asarray(model, F), v, t, None if rgb is None else np.asarray(rgb, np.uint32), rgb_all)


def whole(W, H, z=(1.6, 1.7, 1.9)):
    """a triangle over every pixel, its depth within [1.5, 2): z - 0.25 then has the ulp of z"""
    return tri((-10, -10), (3 * W + 20, -10), (-10, 3 * H + 20), z)


def small_triangles(rng, n, W, H):
    tris, cols = [], []
    for _ in range(n):
        c = np.array([rng.uniform(-2, W + 2), rng.uniform(-2, H + 2)])
        p = c + rng.uniform(-3, 3, (3, 2))
        tris.append(tri(p[0], p[1], p[2], rng.uniform(0.5, 4, 3)))
        cols.append(int(rng.integers(0, 1 << 24)))
    return tris, cols


def gray_plane(rng, H, W):
    """random, with 0 and 255 sprinkled in (the ends of the dim rule)"""
    g = rng.integers(0, 256, (H, W), dtype=np.uint8)
    g[rng.random((H, W)) < 0.1] = 0
    g[rng.random((H, W)) < 0.1] = 255
    return g


def make(name, W, H, step, draws, cols=None, rows=None, margin=0.0, drop_flags=0, specials=(), near_is_left=True, ambient=AMBIENT,
         lattice=True, seed=0):
    """the case: a lattice of cols x rows cells (default: W // step, H // step) whose plain cells are near in the left
    (or right) half and far in the other; specials: (kind, ix, iy) puts a record of that kind into cell (ix, iy), which
    must lie in the near half with its first pixel covered"""
    rng = np.random.default_rng(seed + 1000 * W + H)
    case = dict(name=name, W=W, H=H, gray=gray_plane(rng, H, W), cam=PIX, draws=draws, light=LIGHT, ambient=ambient, near=NEAR,
                lattice=None, margin=float(margin), drop_flags=int(drop_flags), probes=[])
    if not lattice:
        return case
    cols, rows = (W // step if cols is None else cols), (H // step if rows is None else rows)
    rec = np.zeros((rows, cols), OR.MAP_POINT)
    rec["x"], rec["y"] = rng.uniform(-1, 1, (2, rows, cols)).astype(F)     # (never read)
    rec["color"] = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    left = np.arange(cols)[None, :] * step < W // 2
    rec["z"] = np.where(left == near_is_left, NEAR_Z, FAR_Z)
    z = OR.depth_of(AR.key_plane(H, W, PIX, draws, LIGHT, ambient, NEAR))
    m = F(margin)
    for kind, ix, iy in specials:
        px, py = ix * step, iy * step
        assert rec["z"][iy, ix] == NEAR_Z, (name, kind, "the cell is not in the near half")
        hidden = False
        if kind == "dropped":
            rec["flags"][iy, ix] = OR.DROPPED
        elif kind == "drop_flags":
            assert drop_flags & FLAG
            rec["flags"][iy, ix] = FLAG
        elif kind == "z zero":
            rec["z"][iy, ix] = 0.0
        elif kind == "z negative":
            rec["z"][iy, ix] = -1.0
        elif kind == "z inf":
            rec["z"][iy, ix] = np.inf
        elif kind == "z nan":
            rec["z"][iy, ix] = np.nan
        else:
            zo = F(z[py, px] - m)
            assert F(zo + m) == z[py, px] and zo > 0, (name, kind, "z - margin + margin is not z")
            if kind == "ulp above":                         # the winner lies one ulp above zo + margin: hidden
                zo = np.nextafter(zo, F(-np.inf))
                assert F(zo + m) == np.nextafter(z[py, px], F(-np.inf))
                hidden = True
            elif kind == "ulp below":
                zo = np.nextafter(zo, F(np.inf))
                assert F(zo + m) == np.nextafter(z[py, px], F(np.inf))
            else:
                assert kind == "equal"
            rec["z"][iy, ix] = zo
        case["probes"].append((kind, px, py, hidden))
    case["lattice"] = (rec.reshape(-1), cols, rows, step)
    return case


def every_kind(cols, rows, drop_flags, iy=0):
    """one cell per non-occluding kind and boundary, along lattice row iy from cell 0 on (cols permitting)"""
    kinds = [k for k in NON_OCCLUDING if k != "drop_flags" or drop_flags] + list(BOUNDARIES)
    return [(k, i % cols, iy + i // cols) for i, k in enumerate(kinds)]


def cases():
    rng = np.random.default_rng(7)
    out = []
    # one exact tile, a cell per pixel: every kind of record and every boundary, margin 0
    out.append(make("64x16 step 1", 64, 16, 1, [mesh([whole(64, 16)])], drop_flags=FLAG, specials=every_kind(32, 16, FLAG, 3)))
    # ... and with a margin, cells of 4 x 4
    out.append(make("64x16 step 4 margin", 64, 16, 4, [mesh([whole(64, 16)])], margin=0.25, drop_flags=FLAG,
                    specials=[(k, i % 8, i // 8) for i, (k, _, _) in enumerate(every_kind(8, 4, FLAG))]))
    # partial tiles in both directions; 3 does not divide: column 66 and row 18 have no cell, beside near cells
    c = make("67x19 step 3", 67, 19, 3, [mesh([whole(67, 19)])], margin=0.25, near_is_left=False,
             specials=[("equal", 12, 1), ("ulp above", 13, 2), ("ulp below", 14, 3), ("dropped", 21, 5), ("z nan", 20, 0)])
    c["probes"] += [("beyond cols", 66, 4, False), ("beyond rows", 50, 18, False)]
    out.append(c)
    # 16 does not divide 130 x 33: 8 x 2 cells; many small triangles (lane-rasterised) and two large ones (queued)
    tris, colours = small_triangles(rng, 300, 130, 33)
    big = [tri((-5, -3), (139, 2), (65, 53), (1.6, 1.9, 1.7)), tri((130, 33), (0, 32), (43, -4), (1.2, 2.5, 3))]
    tris[100:100] = big[:1]; colours[100:100] = [0x40c040]
    tris.append(big[1]); colours.append(0xc040c0)
    tris.append(whole(130, 33, (3.6, 3.7, 3.9))); colours.append(0x204060)      # behind them all: every pixel is covered
    c = make("130x33 step 16 small and large", 130, 33, 16, [mesh(tris[:200], rgb=colours[:200]), mesh(tris[200:], rgb=colours[200:])],
             near_is_left=False, specials=[("z inf", 5, 0), ("z zero", 7, 1)])
    c["probes"] += [("beyond cols", 129, 10, False), ("beyond rows", 100, 32, False)]
    out.append(c)
    out.append(make("130x33 step 4 small and large", 130, 33, 4, [mesh(tris, rgb=colours)], margin=0.5, drop_flags=FLAG,
                    specials=[("drop_flags", 3, 2), ("z negative", 4, 7), ("dropped", 15, 3)]))
    # the smallest image, a cell per pixel
    out.append(make("5x3 step 1", 5, 3, 1, [mesh([whole(5, 3)])], specials=[("equal", 0, 0), ("ulp above", 1, 1), ("ulp below", 0, 2), ("z nan", 1, 0)]))
    # a lattice of one cell, of 16 x 16 pixels, on two images
    c = make("64x16 one cell", 64, 16, 16, [mesh([whole(64, 16)])], cols=1, rows=1)
    c["probes"] += [("beyond cols", 16, 0, False)]
    out.append(c)
    c = make("5x3 one cell", 5, 3, 4, [mesh([whole(5, 3)])], cols=1, rows=1, specials=[("ulp above", 0, 0)])
    c["probes"] += [("beyond cols", 4, 0, False)]
    out.append(c)
    # two triangles at equal depth with different colours: the smaller colour word wins, hidden or not
    two = [tri((2, 2), (60, 3), (30, 15), (1.5, 1.5, 1.5)), tri((2, 2), (60, 3), (30, 15), (1.5, 1.5, 1.5))]
    out.append(make("equal depth", 64, 16, 2, [mesh(two, rgb=[0x808080, 0x7f8080])], specials=[("equal", 10, 3), ("ulp above", 11, 3)]))
    # channels and grays of 0 and 255 under the dim rule: unshaded colours
    out.append(make("dim ends", 67, 19, 4, [mesh([whole(67, 19), tri((1, 1), (40, 2), (20, 17), (1.2, 1.2, 1.2))], rgb=[0xff0080, 0x00ff00])],
                    ambient=1.0, specials=[("dropped", 2, 1)]))
    # no occluder at all
    out.append(make("no lattice", 67, 19, 1, [mesh([whole(67, 19)])], lattice=False))
    return out


def all_dropped(case):
    """the case with every record of its lattice dropped"""
    rec, cols, rows, step = case["lattice"]
    rec = rec.copy()
    rec["flags"] = OR.DROPPED
    return dict(case, lattice=(rec, cols, rows, step), probes=[])
