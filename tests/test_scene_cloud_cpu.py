"""Cloud points in the scene without a GPU: the two forms of the restatement (tests/scene_cloud_ref.py) agree under
shuffled element orders, dropped records contribute nothing, the C ABI of the three structs, the planner header
(csrc/svo_scene_plan.hpp) in a stand-alone program, plain and under the address and undefined-behaviour sanitizers,
and every crafted case of tests/scene_cloud_cases.py reaches what it is named for."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_ref as MR
import scene_cloud_cases as CC
import scene_cloud_ref as CR
import scene_ref as SR
from stereo_svo_slam_amd import hip_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _elements(case, point_size=1, cloud_size=1, filt=MR.KEEP_ALL):
    cols, rows, cam, sets, lines, spans = case
    return CR.elements(cols, rows, cam, sets, lines, spans, filt, point_size, cloud_size)


def _planes(case, **kw):
    return CR.depth_buffer(case[0], case[1], _elements(case, **kw))


@pytest.mark.parametrize("name", ["shape", "records", "tie", "edge", "pile"])
def test_the_two_forms_agree_in_any_order(name):
    case = dict(shape=CC.shape_case(65, 17), records=CC.records_case(), tie=CC.tie_case(), edge=CC.edge_case(), pile=CC.pile_case(300))[name]
    size = dict(shape=4, edge=5).get(name, 1)
    els = _elements(case, point_size=3, cloud_size=size)
    assert els
    low, covered = CR.depth_buffer(case[0], case[1], els)
    rng = np.random.default_rng(5)
    for _ in range(3):
        shuffled = [els[j] for j in rng.permutation(len(els))]
        for form in (CR.depth_buffer(case[0], case[1], shuffled), CR.smallest_key(case[0], case[1], els, rng)):
            assert (form[1] == covered).all() and (form[0][covered] == low[covered]).all()
    cols, rows, cam, sets, lines, spans = case
    a = CR.render(cols, rows, SR.RGBA8, cam, sets, lines, spans, MR.KEEP_ALL, 3, size, 0x203040)
    b = CR.render_smallest_key(cols, rows, SR.RGBA8, cam, sets, lines, spans, MR.KEEP_ALL, 3, size, 0x203040, rng)
    assert a.tobytes() == b.tobytes() and a.shape == (rows, cols, 4) and (a[:, :, 3] == 255).all()


def test_without_drawn_records_it_is_the_scene():
    """no span, an empty span, and records that are all DROPPED or hit by drop_flags: scene_ref's picture"""
    cols, rows, cam, sets, lines, spans = CC.shape_case(65, 17)
    filt = dict(drop_flags=MR.IGNORE_COMPLETELY, own_only=0, min_inliers=0)
    want = SR.render(cols, rows, SR.RGB8, cam, sets, lines, filt, 3)
    gone = [s.copy() for s in spans]
    gone[0]["flags"] = CR.CLOUD_DROPPED
    gone[1]["flags"] = MR.IGNORE_COMPLETELY
    for sp in ([], [spans[0][:0]], gone):
        assert CR.cloud_elements(cols, rows, cam, sp, filt["drop_flags"], 5) == []
        assert CR.render(cols, rows, SR.RGB8, cam, sets, lines, sp, filt, 3, 5).tobytes() == want.tobytes()
    assert CR.render(cols, rows, SR.RGB8, cam, sets, lines, spans, filt, 3, 5).tobytes() != want.tobytes()
    # a class-4 element never changes a pixel's sparse winner at a smaller or equal depth: no key of "scene" changes
    low, covered = CR.depth_buffer(cols, rows, CR.elements(cols, rows, cam, sets, lines, spans, filt, 3, 5))
    low0, covered0 = CR.depth_buffer(cols, rows, SR.elements(cols, rows, cam, sets, lines, filt, 3))
    sparse = covered & (low >> 24 != CR.CLASS_CLOUD)
    assert (covered0[sparse]).all() and (low[sparse] == low0[sparse]).all() and (covered | ~covered0).all()


def test_struct_layouts_and_symbols(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to read the header's layout"
    ctypes_of = {"svo_scene_span": hip_lib.SceneSpan, "svo_scene_cloud_info": hip_lib.SceneCloudInfo, "svo_scene_clouds": hip_lib.SceneClouds}
    lines = []
    for name, cls in ctypes_of.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'  printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));\n' for f in cls._fields_]
    lines.append('  printf("enums %d %d %d %d\\n", SVO_SCENE_CLASS_CLOUD, SVO_SCENE_CLASS_POINT, SVO_CLOUD_DROPPED, (int)sizeof(svo_map_point));\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_hip.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.splitlines()}
    want = {"svo_scene_span": (16, dict(points=0, n=8)),
            "svo_scene_cloud_info": (32, dict(status=0, keyframe_id=4, live_points=8, _pad=12, extra_points=16, _pad2=24)),
            "svo_scene_clouds": (120, dict(live=0, what=4, cloud=8, check=56, point_size=88, _reserved=92, extra=104, info=112))}
    for name, cls in ctypes_of.items():
        assert c[name] == [C.sizeof(cls)] == [want[name][0]], name
        assert [f[0] for f in cls._fields_] == list(want[name][1])
        for f, off in want[name][1].items():
            assert c[f"{name}.{f}"] == [getattr(cls, f).offset] == [off], (name, f)
    info = hip_lib.SCENE_CLOUD_INFO_DTYPE
    assert info.itemsize == 32 and list(info.names) == [f[0] for f in hip_lib.SceneCloudInfo._fields_]
    for f in info.names:
        assert info.fields[f][1] == getattr(hip_lib.SceneCloudInfo, f).offset, f
    assert c["enums"] == [hip_lib.SCENE_CLASS_CLOUD, hip_lib.SCENE_CLASS_POINT, hip_lib.CLOUD_DROPPED, hip_lib.MAP_POINT_DTYPE.itemsize] == \
        [CR.CLASS_CLOUD, SR.CLASS_POINT, CR.CLOUD_DROPPED, CR.MAP_POINT.itemsize] == [4, 3, 0x80, 16]
    assert CR.MAP_POINT == hip_lib.MAP_POINT_DTYPE
    for sym in ("svo_submit_export_scenes_clouds", "svo_export_scenes_clouds", "svo_render_scene_clouds"):
        assert sym in hip_lib.SYMBOLS


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """the planner program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("scene_plan")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "scene_plan_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", src]
    out = {"plain": str(d / "scene_plan_check"), "sanitized": str(d / "scene_plan_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_planner(planner, which):
    r = subprocess.run([planner[which]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scene plan ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert CC.PIECE == int(open(os.path.join(ROOT, "stereo-svo-slam_amd", "csrc", "svo_scene_plan.hpp")).read()
                           .split("SCENE_PLAN_PIECE = ")[1].split(";")[0])


# ---------------------------------------------------------------------------------- the cases reach what they are named for

def test_case_tie():
    case = CC.tie_case()
    cols, rows, cam, sets, lines, spans = case
    low, covered = _planes(case)
    cls = CR.classes(low, covered)
    cloud = {}                                                        # pixel -> [(depth bits, low)] of the cloud points on it
    for e in CR.cloud_elements(cols, rows, cam, spans, 0, 1):
        assert len(e) == 1
        x, y, z, w = e[0]
        cloud.setdefault((x, y), []).append((int(F(z).view(np.uint32)), w))
    sparse = {}
    for e in SR.elements(cols, rows, cam, sets, lines, MR.KEEP_ALL, 1):
        for x, y, z, w in e:
            sparse.setdefault((x, y), []).append((int(F(z).view(np.uint32)), w))
    # a keypoint wins a pixel that a cloud point of equal depth bits and a smaller colour also covers
    x, y = CC.TIE["keypoint"]
    assert cls[y, x] == SR.CLASS_POINT and low[y, x] & 0xffffff == 0xfefefe
    assert [d for d, _ in cloud[(x, y)]] == [d for d, w in sparse[(x, y)] if w >> 24 == SR.CLASS_POINT] and cloud[(x, y)][0][1] & 0xffffff == 0
    # a trajectory line wins over a cloud point of its depth; beside the line the same cloud point shows
    x, y = CC.TIE["line"]
    assert cls[y, x] == SR.CLASS_TRAJECTORY and cloud[(x, y)][0][0] in [d for d, w in sparse[(x, y)] if w >> 24 == SR.CLASS_TRAJECTORY]
    x, y = CC.TIE["beside_line"]
    assert cls[y, x] == CR.CLASS_CLOUD and low[y, x] & 0xffffff == 0x00aa00 and (x, y) not in sparse
    # two cloud points at equal depth: the smaller colour word, whether it comes first (and in another span) or second
    for name, rgb, first in (("smaller", 0x102030, True), ("larger", 0x302010, False)):
        x, y = CC.TIE[name]
        (d0, w0), (d1, w1) = cloud[(x, y)]
        assert d0 == d1 and (w0 < w1) == first and cls[y, x] == CR.CLASS_CLOUD and low[y, x] & 0xffffff == rgb == min(w0, w1) & 0xffffff
    # a cloud point one ulp nearer than a keypoint wins
    x, y = CC.TIE["nearer"]
    assert cls[y, x] == CR.CLASS_CLOUD and cloud[(x, y)][0][0] + 1 == sparse[(x, y)][0][0]


def test_case_pile():
    case = CC.pile_case()
    cols, rows, cam, _, _, spans = case
    els = CR.cloud_elements(cols, rows, cam, spans, 0, 1)
    assert len(els) == CC.PILE_N == len(spans[0]) > 4 * CC.PIECE - 1
    assert {(e[0][0], e[0][1]) for e in els} == {CC.PILE_PIXEL} and all(len(e) == 1 for e in els)
    depths = [int(F(e[0][2]).view(np.uint32)) for e in els]
    assert len(set(depths)) == CC.PILE_N, "distinct depths"
    nearest = int(np.argmin(depths))
    assert nearest != 0 and nearest != CC.PILE_N - 1, "the nearest record is neither the first nor the last"
    low, covered = CR.depth_buffer(cols, rows, els)
    assert covered.sum() == 1 and low[CC.PILE_PIXEL[1], CC.PILE_PIXEL[0]] == (CR.CLASS_CLOUD << 24 | 1)   # record of depth 1.0: colour 1
    assert els[nearest][0][3] == (CR.CLASS_CLOUD << 24 | 1)


def test_case_edge():
    cols, rows, cam, _, _, spans = CC.edge_case()
    assert (cols, rows) == (130, 33)
    inside = lambda x, y: 0 <= x < cols and 0 <= y < rows
    for s in [v for v in CC.CLOUD_SIZES if v > 1]:
        image_border = tile_x = tile_y = 0
        for rec, (u, v) in zip(spans[0], CC.EDGE_CENTRES):
            px = CR.cloud_point(cam, rec, s)
            assert len(px) == s * s and (px[0][0], px[0][1]) == (u - (s - 1) // 2, v - (s - 1) // 2)
            ins = [q for q in px if inside(q[0], q[1])]
            assert ins, "no square is fully outside"
            image_border += len(ins) < len(px)
            tile_x += len({q[0] // 64 for q in ins}) > 1
            tile_y += len({q[1] // 16 for q in ins}) > 1
        assert image_border >= 8 and tile_x >= 3 and tile_y >= 3, (s, image_border, tile_x, tile_y)
    low, covered = _planes(CC.edge_case(), cloud_size=5)
    assert covered[0, 0] and covered[32, 129] and covered[0, 129] and covered[32, 0]


def test_case_records():
    case = CC.records_case()
    cols, rows, cam, _, _, spans = case
    names = list(CC.RECORDS)
    colour = {k: 0x010101 * (0x10 + i) for i, k in enumerate(names)}
    by = lambda size, drop: {int(e[0][3]) & 0xffffff: e for e in CR.cloud_elements(cols, rows, cam, spans, drop, size)}
    # size 1, no drop_flags: exactly these are drawn, each on its pixel
    drawn = by(1, 0)
    shown = ("plain", "ignore_completely", "ignore_other", "at_near", "huge_depth")
    assert set(drawn) == {colour[k] for k in shown}
    for k in shown:
        assert [(q[0], q[1]) for q in drawn[colour[k]]] == [CC.RECORD_PIXEL[k]]
    assert int(F(drawn[colour["at_near"]][0][2]).view(np.uint32)) == int(CC.NEAR.view(np.uint32))
    # drop_flags takes the record that carries the bit, and only that one
    assert set(by(1, CC.IGNORE_COMPLETELY)) == set(drawn) - {colour["ignore_completely"]}
    # the records that are not drawn fail for the reason they are named for
    rec = {k: spans[0][i] for i, k in enumerate(names)}
    with np.errstate(all="ignore"):
        c = {k: SR.transform(cam, (rec[k]["x"], rec[k]["y"], rec[k]["z"])) for k in names}
        for k in ("nan", "inf", "minus_inf"):
            assert not np.all(np.isfinite(c[k])), k
        for k in ("behind", "below_near"):
            assert np.all(np.isfinite(c[k])) and c[k][2] < cam[15], k
        assert c["below_near"][2] == CC.BELOW_NEAR and c["at_near"][2] == cam[15]
        for k in ("at_2_15_x", "at_minus_2_15_x", "at_2_15_y", "beyond_2_15", "overflow_u", "huge_depth", "below_2_15_x", "below_2_15_y"):
            assert np.all(np.isfinite(c[k])) and c[k][2] >= cam[15], k
        for k in ("at_2_15_x", "at_minus_2_15_x", "at_2_15_y", "beyond_2_15", "overflow_u"):     # (overflow_u: f * c_0 is +inf)
            assert SR.project(cam, c[k]) is None, k
        assert SR.project(cam, c["below_2_15_x"])[0] == 32767 and SR.project(cam, c["below_2_15_y"])[1] == -32768
    for k in ("dropped", "dropped_and_more"):
        assert int(rec[k]["flags"]) & CR.CLOUD_DROPPED and CR.cloud_point(cam, rec[k], 1), k          # (only the flag keeps them out)
    # at size 16 the squares outside stay outside and the straddling ones reach in
    big = by(16, 0)
    for k in ("outside_left", "outside_below", "below_2_15_x", "below_2_15_y"):
        assert CR.cloud_point(cam, rec[k], 16) and colour[k] not in big, k
    for k in ("straddles_left", "straddles_corner"):
        assert 0 < len(big[colour[k]]) < 256 and colour[k] not in by(1, 0), k


def test_case_shapes_and_spans():
    assert set(CC.SHAPES) == {(1, 1), (63, 15), (65, 17), (130, 33)} and CC.SPAN_LENGTHS == (0, 1, 255, 256, 257, CC.PIECE + 1)
    for w, h in CC.SHAPES:
        low, covered = _planes(CC.shape_case(w, h), point_size=2, cloud_size=4)
        cls = CR.classes(low, covered)
        case = CC.shape_case(w, h)
        assert CR.cloud_elements(w, h, case[2], case[5], 0, 4), (w, h)
        if w > 1:                                                    # (the one pixel of 1 x 1 goes to one element)
            assert (cls == CR.CLASS_CLOUD).any() and (cls == -1).any() and ((cls >= 0) & (cls < CR.CLASS_CLOUD)).any(), (w, h)
    for n in CC.SPAN_LENGTHS:
        case = CC.span_case(n)
        assert len(case[5][0]) == n
        if n:
            assert len(CR.cloud_elements(*case[:3], case[5], 0, 1)) > 0.3 * n
