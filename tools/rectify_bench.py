"""Cost of the GPU rectification (svo_ctx_set_rectification / svo_remap_linear) on the MI355X.

  (a) python tools/rectify_bench.py --part a
      bench.py's default workload (C2 `euroc`, 3584 sequences in the ctx's default groups, borrowed device frames,
      pipelined submits) on one ctx, alternating rectification off and on (identity maps by default: the
      tracking work is the same in both legs, the remap costs what a calibrated map costs) in `--pairs`
      pairs; frames/s of every leg, the medians and the on/off ratio.
  (b) python tools/rectify_bench.py --part b
      the remap alone: 256 sequences x 2 images of 752 x 480 through one EuRoC-like map (svo_remap_linear,
      n = 512) timed with device events; bytes moved = raw read + rectified written + map entries fetched
      (6 B per output pixel per workgroup of 16 images), and their share of the 8 TB/s peak. Run it under
      `rocprofv3 --kernel-trace --stats -- python tools/rectify_bench.py --part b` for the kernel's own time
      (remap_linear_kernel; remap_prep_kernel is the per-call map conversion).
Prints one JSON line per part.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting: 14 groups of 256)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
import rectify_ref
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

HBM_PEAK_GBS = 8000.0


def part_a(args):
    device = torch.device("cuda", 0)
    B, n_loops, nF = args.seqs, min(args.seqs, args.loops), args.loop_frames
    plan = bench.loop_plan(B, n_loops, nF)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), nF, device)
    W, H = cfg["width"], cfg["height"]
    maps = (rectify_ref.identity_maps(W, H),) * 2 if args.maps == "identity" else \
        (rectify_ref.euroc_like_maps(W, H, angle=0.012), rectify_ref.euroc_like_maps(W, H, angle=-0.009))
    packs_for = bench.step_packer(lefts, rights, plan, True)
    slam = StereoSlamBatch(cfg, W, H, B, 0)
    groups = slam.groups()
    n_steps = args.warmup + 2 * args.pairs * args.steps
    packed = packs_for(slam, n_steps)
    for k in range(args.warmup):
        slam.submit_packed(packed[k])
    slam.wait()
    k0 = args.warmup
    legs = {"off": [], "on": []}
    for _ in range(args.pairs):
        for leg in ("off", "on"):
            slam.set_rectification(*maps) if leg == "on" else slam.set_rectification(None, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(k0, k0 + args.steps):
                slam.submit_packed(packed[k])
            slam.wait()
            torch.cuda.synchronize()
            legs[leg].append(B * args.steps / (time.perf_counter() - t0))
            k0 += args.steps
    slam.close()
    off, on = np.array(legs["off"]), np.array(legs["on"])
    ratios = on / off
    print(json.dumps({"part": "a", "config": "euroc", "seqs": B, "groups": groups, "steps_per_leg": args.steps,
                      "maps": args.maps, "frames_per_s_off": off.round(0).tolist(),
                      "frames_per_s_on": on.round(0).tolist(), "median_off": float(np.median(off)),
                      "median_on": float(np.median(on)), "ratio_median": float(np.median(ratios)),
                      "ratio_min": float(ratios.min()), "ratio_max": float(ratios.max())}))


def part_b(args):
    W, H, n = 752, 480, 2 * args.remap_seqs
    h = hip_lib.Handle(0, 64)
    mx, my = (torch.from_numpy(m).cuda() for m in rectify_ref.euroc_like_maps(W, H))
    gen = torch.Generator(device="cuda").manual_seed(0)
    srcs = [torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(n)]
    outs = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(n)]
    arr_s, arr_d = hip_lib._imgs(srcs), hip_lib._imgs(outs)
    pmx, pmy = hip_lib._ptr(mx), hip_lib._ptr(my)
    call = lambda: hip_lib._check(hip_lib.lib().svo_remap_linear(h._h, n, arr_s, arr_d, pmx, pmy))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    # calls queued back to back between two events (the argument arrays are built once): per call
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(5):
        ev[0].record()
        for _ in range(args.reps):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / args.reps)
    tiles = ((W + 63) // 64) * ((H + 63) // 64)
    image_bytes = 2 * n * W * H
    map_bytes = tiles * ((n + 15) // 16) * 64 * 64 * 6
    ms = float(np.median(times))
    moved = image_bytes + map_bytes
    print(json.dumps({"part": "b", "images": n, "size": [W, H], "call_ms_median": ms,
                      "call_ms_min": float(np.min(times)), "call_ms_max": float(np.max(times)),
                      "bytes_moved": moved, "image_bytes": image_bytes, "map_bytes": map_bytes,
                      "gb_per_s": moved / (ms * 1e-3) / 1e9,
                      "hbm_peak_fraction": moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "note": "device events around back-to-back svo_remap_linear calls: remap_prep_kernel + remap_linear_kernel"}))
    h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("a", "b"), required=True)
    ap.add_argument("--seqs", type=int, default=3584)
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="(a) steps per leg")
    ap.add_argument("--warmup", type=int, default=16, help="(a) untimed steps first")
    ap.add_argument("--pairs", type=int, default=3, help="(a) off/on pairs")
    ap.add_argument("--maps", choices=("identity", "euroc"), default="identity", help="(a) maps of the 'on' legs")
    ap.add_argument("--remap-seqs", type=int, default=256, help="(b) sequences (2 images each)")
    ap.add_argument("--reps", type=int, default=50, help="(b) timed calls")
    args = ap.parse_args()
    part_a(args) if args.part == "a" else part_b(args)


if __name__ == "__main__":
    main()
