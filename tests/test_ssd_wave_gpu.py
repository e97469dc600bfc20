"""ssd_disparity_kernel (csrc/depth.hip: one wavefront per keypoint) against the four-wave kernel it replaced
(ssd_disparity_ref_kernel, kept in csrc/svo_capi_check.hip) and against the CPU oracle, word for word, through
svo_ssd_disparity_check: both kernels run on the same batch in the tracker's launch form, each into an array of its
own that was filled with a NaN pattern first.

For every launch of tests/ssd_wave_cases.py:
  the entry reports zero differing words;
  the kernel's array equals, in bits, the oracle's disparities where the launch form says a keypoint is handled, and
  the fill pattern everywhere else: no keypoint is left out, none outside the range is written.
tests/test_ssd_wave_cases_cpu.py asserts what the launches contain (borders, skip conditions, both kernel shapes, one
to five column blocks and one and two row blocks, a 65-column map, image layouts, chunks that cross the right edge,
counts around 64, the tracker's offsets and predicates). No comparison has a tolerance.
"""
import numpy as np
import pytest
import torch

import oracle_py as O
import ssd_wave_cases as SW
from stereo_svo_slam_amd import hip_lib

pytestmark = pytest.mark.gpu

U = np.uint32


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=4096)
    yield h
    h.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_PLACED, _ORACLE = {}, {}


def place(img, layout):
    """img (numpy uint8 [h, w]) on the GPU as a view in that layout, surrounded by a grey level it holds least of"""
    h, w = img.shape
    off, stride = SW.LAYOUTS[layout][0], SW.LAYOUTS[layout][1](w)
    fill = int(np.argmin(np.bincount(img.ravel(), minlength=256)))
    buf = torch.full((off + h * stride + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    view = buf[off:off + h * stride].view(h, stride)[:, :w]
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)))
    assert view.data_ptr() % 8 == off and view.stride(0) == stride and view.stride(1) == 1
    return view


def placed(case, layout):
    key = (case[0], layout)
    if key not in _PLACED:
        _PLACED[key] = (place(case[1], layout), place(case[2], layout))
    return _PLACED[key]


def oracle(case):
    name, left, right, kps, win, sx, sy, clamp = case
    if name not in _ORACLE:
        _ORACLE[name] = O.ssd_disparity(np.ascontiguousarray(left), np.ascontiguousarray(right), kps, win, sx, sy, clamp)
    return _ORACLE[name]


def run_launch(H, launch):
    seqs = launch["seqs"]
    stride = max(len(s["idx"]) + s["extra"] for s in seqs) + 3
    keep, args = [], []
    for s in seqs:
        case = s["case"]
        n = len(s["idx"])
        cap = n + s["extra"]
        kps = np.full((max(cap, 1), 2), (-5000.0, 7.0e8), np.float32)        # (entries past n are never read)
        kps[:n] = case[3][s["idx"]]
        left, right = placed(case, s["layout"])
        d = dict(n=dev(np.array([n], np.int32)), kps=dev(kps),
                 first_dev=None if s["first_dev"] is None else dev(np.array([s["first_dev"]], np.int32)),
                 enable=None if s["enable"] is None else dev(np.array([s["enable"]], U).view(np.int32)))
        keep.append(d)
        args.append(dict(left=left, right=right, n=d["n"], kps2d=d["kps"], disparity=None, win=case[4], search_x=case[5],
                         search_y=case[6], clamp_half=case[7], first=s["first"], cap=cap, first_ptr=d["first_dev"],
                         enable=d["enable"]))
    n_diff, first, out, ref = H.ssd_disparity_check(args, launch["n_bound"], launch["win"], launch["search_y"], stride, fill=SW.FILL)
    got = out.cpu().numpy().view(U)
    problems = []
    if n_diff != 0 or first != -1:
        r = ref.cpu().numpy().view(U)
        bad = np.argwhere(got != r)
        problems.append(f"{n_diff} words differ from the four-wave kernel's, first {first}: (sequence, entry) "
                        f"{bad[:6].tolist()}: {got[got != r][:6].view(np.float32).tolist()} for {r[got != r][:6].view(np.float32).tolist()}")
    for b, s in enumerate(seqs):
        want = SW.expected(s, oracle(s["case"])[s["idx"]], launch["n_bound"], stride)
        bad = np.nonzero(got[b] != want)[0]
        if bad.size:
            problems.append(f"sequence {b} ({s['case'][0]}): {bad.size} words differ from the oracle / the fill, first entries "
                            f"{bad[:6].tolist()}: {got[b][bad[:6]].view(np.float32).tolist()} for {want[bad[:6]].view(np.float32).tolist()}")
    return problems


@pytest.mark.parametrize("group", ("case", "count", "tracker"))
def test_one_wave_kernel_equals_the_four_wave_kernel_and_the_oracle(H, group):
    todo = [l for l in SW.launches() if l["name"].startswith(group)]
    assert todo
    failed = []
    for launch in todo:
        p = run_launch(H, launch)
        if p:
            failed.append(launch["name"] + ": " + "; ".join(p))
    assert not failed, f"{len(failed)} of {len(todo)} launches:\n" + "\n".join(failed[:20])
