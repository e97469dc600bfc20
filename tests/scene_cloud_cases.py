"""Crafted inputs of the cloud points in the scene, shared by test_scene_cloud_cpu.py (which asserts from the
restatement alone that every case reaches what it is named for) and test_scene_cloud_gpu.py (which runs them). A case
is (cols, rows, camera float32 [16], sets, lines, spans): scene_ref's sets and lines and a list of MAP_POINT arrays.
Cameras have an identity view and a power-of-two f, so a point made by at() projects back exactly."""
import numpy as np

import scene_cloud_ref as CR
import scene_ref as SR

F = np.float32
SHAPES = ((1, 1), (63, 15), (65, 17), (130, 33))          # whole, partial, and more than one 64 x 16 tile each way
CLOUD_SIZES = (1, 4, 5, 16)
PIECE = 1024                                              # records of one workgroup of the splat pass
SPAN_LENGTHS = (0, 1, 255, 256, 257, PIECE + 1)
IGNORE_COMPLETELY = 2


def at(u, v, z, cam):
    """the world point that an identity-view camera projects to (u, v) at depth z"""
    f, cx, cy = cam[12], cam[13], cam[14]
    return F([(F(u) - cx) / f * F(z), (F(v) - cy) / f * F(z), z])


def kp_set(k3, color=None, own_id=0):
    """a map_ref set of the points k3 [n, 3] that every filter keeps; color: words b << 16 | g << 8 | r"""
    k3 = np.asarray(k3, F).reshape(-1, 3)
    n = len(k3)
    z = np.zeros(n, np.uint32)
    col = ((np.arange(n, dtype=np.uint64) * 2654435761 >> 8) & 0xffffff).astype(np.uint32) if color is None else np.asarray(color, np.uint32)
    return (n, own_id, k3, {"flags": z, "keyframe_id": z, "inlier_count": z, "color": col})


def line(a, b, cls, rgb):
    return (F(a), F(b), cls << 24 | rgb)


def random_records(rng, n, depths=(1.0, 1.5, 2.0, 3.0), spread=1.2):
    z = rng.choice(F(depths), n)
    xyz = np.stack([rng.uniform(-spread, spread, n).astype(F) * z, rng.uniform(-spread, spread, n).astype(F) * z, z], 1)
    return CR.records(xyz, rng.integers(0, 2**24, n))


def shape_case(w, h, seed=31):
    """the same keypoints, lines and two spans (200 and 57 records) through a camera that fits a w x h image"""
    rng = np.random.default_rng(seed)
    spans = [random_records(rng, 200), random_records(rng, 57)]
    k = random_records(rng, 30)
    sets = [kp_set(np.stack([k["x"], k["y"], k["z"]], 1))]
    ends = np.stack([rng.uniform(-1.3, 1.3, (6, 2)), rng.uniform(-1.3, 1.3, (6, 2)), rng.uniform(0.6, 3, (6, 2))], 2).astype(F)
    lines = [line(e[0], e[1], int(rng.integers(0, 3)), int(rng.integers(0, 2**24))) for e in ends]
    return (w, h, SR.camera(np.eye(3, 4), max(w, h) / 2, w / 2, h / 2, 0.5), sets, lines, spans)


def span_case(n, seed=32):
    """65 x 17, one span of n records and a few keypoints"""
    rng = np.random.default_rng(seed + n)
    cam = SR.camera(np.eye(3, 4), 32.0, 32.0, 8.0, 0.5)
    inside = lambda m: np.array([at(rng.uniform(0, 65), rng.uniform(0, 17), rng.choice(F([1.0, 1.5, 2.0, 3.0])), cam) for _ in range(m)], F).reshape(-1, 3)
    return (65, 17, cam, [kp_set(inside(9))], [], [CR.records(inside(n), rng.integers(0, 2**24, n))])


CAM_130 = SR.camera(np.eye(3, 4), 8.0, 64.0, 16.0, 0.5)
NEAR, BELOW_NEAR = F(0.5), np.nextafter(F(0.5), F(0))
BIG = F(32768) - F(1 / 256)
# name -> (world point, flags): the records of records_case; its pixels are at depth 1 unless said otherwise
RECORDS = {
    "plain": (at(10.5, 3.5, 1.0, CAM_130), 0),
    "dropped": (at(14.5, 3.5, 1.0, CAM_130), CR.CLOUD_DROPPED),
    "dropped_and_more": (at(18.5, 3.5, 1.0, CAM_130), CR.CLOUD_DROPPED | 1),
    "ignore_completely": (at(22.5, 3.5, 1.0, CAM_130), IGNORE_COMPLETELY),
    "ignore_other": (at(26.5, 3.5, 1.0, CAM_130), 1),
    "nan": (F([np.nan, 0, 1]), 0), "inf": (F([0, np.inf, 1]), 0), "minus_inf": (F([0, 0, -np.inf]), 0),
    "overflow_u": (F([3e38, 0, 1]), 0), "huge_depth": (F([0, 0, 1e30]), 0),
    "behind": (at(30.5, 10.5, -1.0, CAM_130), 0), "below_near": (at(34.5, 10.5, BELOW_NEAR, CAM_130), 0),
    "at_near": (at(38.5, 10.5, NEAR, CAM_130), 0),
    "below_2_15_x": (at(BIG, 5, 1.0, CAM_130), 0), "below_2_15_y": (at(5, -BIG, 1.0, CAM_130), 0),
    "at_2_15_x": (at(32768, 5, 1.0, CAM_130), 0), "at_minus_2_15_x": (at(-32768, 5, 1.0, CAM_130), 0),
    "at_2_15_y": (at(5, 32768, 1.0, CAM_130), 0), "beyond_2_15": (at(1e6, -1e6, 1.0, CAM_130), 0),
    "outside_left": (at(-20.5, 8.5, 1.0, CAM_130), 0), "outside_below": (at(40.5, 60.5, 1.0, CAM_130), 0),
    "straddles_left": (at(-1.5, 20.5, 1.0, CAM_130), 0), "straddles_corner": (at(130.5, 33.5, 1.0, CAM_130), 0),
}
RECORD_PIXEL = {"plain": (10, 3), "dropped": (14, 3), "dropped_and_more": (18, 3), "ignore_completely": (22, 3),
                "ignore_other": (26, 3), "behind": (30, 10), "below_near": (34, 10), "at_near": (38, 10),
                "huge_depth": (64, 16)}                                   # (finite, in front, at the principal point: drawn)


def records_case():
    """130 x 33: one record per name of RECORDS (colour: 0x10 + its index in every channel), no sparse element"""
    names = list(RECORDS)
    rec = CR.records([RECORDS[k][0] for k in names], [[0x10 + i] * 3 for i in range(len(names))], [RECORDS[k][1] for k in names])
    return (130, 33, CAM_130, [], [], [rec])


CAM_70 = SR.camera(np.eye(3, 4), 8.0, 32.0, 8.0, 0.5)
TIE = dict(keypoint=(10, 3), line=(25, 5), beside_line=(25, 7), smaller=(40, 12), larger=(44, 12), nearer=(50, 3))


def tie_case():
    """70 x 20, every square one pixel. At equal depth bits: a keypoint (class 3) over a black cloud point; a
    trajectory line (class 2) over a cloud point; of two cloud points the smaller colour word, whichever comes first.
    And a cloud point just nearer than a keypoint wins."""
    P = lambda name, z: at(TIE[name][0] + 0.5, TIE[name][1] + 0.5, z, CAM_70)
    sets = [kp_set([P("keypoint", 1.0), P("nearer", 1.0)], color=[0xfefefe, 0x0000ff])]
    lines = [line(at(20.5, 5.5, 2.0, CAM_70), at(30.5, 5.5, 2.0, CAM_70), SR.CLASS_TRAJECTORY, 0xff0000)]
    xyz = [P("keypoint", 1.0), P("line", 2.0), P("beside_line", 2.0), P("smaller", 1.5), P("smaller", 1.5), P("larger", 1.5), P("larger", 1.5),
           P("nearer", np.nextafter(F(1.0), F(0)))]
    rgb = [0x000000, 0x00aa00, 0x00aa00, 0x102030, 0x102031, 0x302011, 0x302010, 0x00ff00]
    return (70, 20, CAM_70, sets, lines, [CR.records(xyz[:4], rgb[:4]), CR.records(xyz[4:], rgb[4:])])


PILE_PIXEL, PILE_N = (5, 6), 4096


def pile_case(n=PILE_N, seed=33):
    """16 x 8: n records of distinct depths 1 + i / 8192 on one pixel, in a shuffled order; record i has colour i + 1"""
    cam = SR.camera(np.eye(3, 4), 8.0, 8.0, 4.0, 0.5)
    order = np.random.default_rng(seed).permutation(n)
    z = (F(1.0) + order.astype(F) / F(8192)).astype(F)
    xyz = np.array([at(PILE_PIXEL[0] + 0.5, PILE_PIXEL[1] + 0.5, zz, cam) for zz in z], F)
    return (16, 8, cam, [], [], [CR.records(xyz, (order + 1).astype(np.uint32))])


# pixel centres of edge_case's records: the image's corners and borders, the tile borders at x = 64 and y = 16 / 32
EDGE_CENTRES = ((0, 0), (129, 32), (0, 32), (129, 0), (63, 15), (64, 16), (63, 0), (64, 32), (-2, 10), (130, 10), (70, -2), (70, 33),
                (100, 15), (100, 16), (63, 24), (64, 24))


def edge_case():
    """130 x 33 (3 x 3 tiles): squares of CLOUD_SIZES > 1 that straddle the image's border and the tiles' borders"""
    xyz = [at(u + 0.5, v + 0.5, 1.0 + 0.125 * i, CAM_130) for i, (u, v) in enumerate(EDGE_CENTRES)]
    return (130, 33, CAM_130, [], [], [CR.records(xyz, [0x010101 * (i + 1) for i in range(len(xyz))])])
