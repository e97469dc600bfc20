"""Cost of camera rigs (svo_ctx_add_rigs / svo_ctx_assign_rigs, svo_remap_linear_multi) on the MI355X.

  (remap) python tools/rig_bench.py --part remap --variant single|shared|rigs16|rigs256
      the remap alone: 256 slots x 2 sides of 752 x 480 as one stage call of n = 512 images.
        single   svo_remap_linear: the single-map launch (remap_linear_kernel)
        shared   svo_remap_linear_multi with one map for all (remap_linear_multi_kernel)
        rigs16   ... 32 maps (16 rigs x 2 sides), 16 images each (remap_linear_multi_kernel)
        rigs256  ... 512 maps, a map per image (remap_linear_single_kernel)
      Device events around back-to-back calls (they include the per-call remap_prep_kernel launches of the stage
      entry, one per map: the tracker prepares a rig's maps once), the bytes moved (images read + written, map
      entries of 6 B per output pixel per chunk), their share of the 8 TB/s peak, and in the same process a plain
      device copy of the same byte count. For the kernel's own time run one variant per process under
      `rocprofv3 --kernel-trace --stats -- python tools/rig_bench.py --part remap --variant ...`.
  (intrinsics) python tools/rig_bench.py --part intrinsics
      bench.py's default workload on one ctx, alternating "every slot on rig 0" and "every slot bound to a rig of
      its own with the ctx's values" in `--pairs` pairs (each leg starts with the assignment, which restarts every
      slot, and untimed steps); frames/s of every leg, the medians and the ratio.
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

import ctypes as C

import numpy as np
import torch

import bench
import rectify_ref
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

HBM_PEAK_GBS = 8000.0
VARIANTS = {"single": 0, "shared": 1, "rigs16": 32, "rigs256": 512}       # maps of the call (0: svo_remap_linear)


def part_remap(args):
    W, H, n = 752, 480, 2 * args.remap_seqs
    n_maps = min(max(VARIANTS[args.variant], 1), n)
    h = hip_lib.Handle(0, 64)
    mx, my = (torch.from_numpy(m).cuda() for m in rectify_ref.euroc_like_maps(W, H))
    # a map per rig and side: the base map moved by a fraction of a pixel (different entries, the same access pattern)
    maps_x = [mx + 0.03125 * (m % 29) for m in range(n_maps)]
    maps_y = [my - 0.03125 * (m % 23) for m in range(n_maps)]
    gen = torch.Generator(device="cuda").manual_seed(0)
    srcs = [torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(n)]
    outs = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(n)]
    arr_s, arr_d = hip_lib._imgs(srcs), hip_lib._imgs(outs)
    if args.variant == "single":
        pmx, pmy = hip_lib._ptr(maps_x[0]), hip_lib._ptr(maps_y[0])
        call = lambda: hip_lib._check(hip_lib.lib().svo_remap_linear(h._h, n, arr_s, arr_d, pmx, pmy))
    else:
        px = (C.c_void_p * n_maps)(*[m.data_ptr() for m in maps_x])
        py = (C.c_void_p * n_maps)(*[m.data_ptr() for m in maps_y])
        idx = (C.c_int * n)(*[i * n_maps // n for i in range(n)])
        call = lambda: hip_lib._check(hip_lib.lib().svo_remap_linear_multi(h._h, n, arr_s, arr_d, n_maps, px, py, idx))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(f, reps):
        times = []
        for _ in range(5):
            ev[0].record()
            for _ in range(reps):
                f()
            ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]) / reps)
        return times

    times = timed(call, args.reps)
    tiles = ((W + 63) // 64) * ((H + 63) // 64)
    per_map = n // n_maps
    chunks = n_maps * ((per_map + 15) // 16)
    image_bytes = 2 * n * W * H
    map_bytes = tiles * chunks * 64 * 64 * 6
    moved = image_bytes + map_bytes
    # a plain device copy that moves the same bytes (half read, half written), as DESIGN 4.6 does
    a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    copy_times = timed(lambda: b.copy_(a), 20)
    ms, copy_ms = float(np.median(times)), float(np.median(copy_times))
    print(json.dumps({"part": "remap", "variant": args.variant, "images": n, "maps": n_maps, "chunks": chunks, "size": [W, H],
                      "call_ms_median": ms, "call_ms_min": float(np.min(times)), "call_ms_max": float(np.max(times)),
                      "bytes_moved": moved, "image_bytes": image_bytes, "map_bytes": map_bytes,
                      "bytes_per_output_pixel": moved / (n * W * H),
                      "gb_per_s": moved / (ms * 1e-3) / 1e9, "hbm_peak_fraction": moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "copy_ms_median": copy_ms, "copy_gb_per_s": moved / (copy_ms * 1e-3) / 1e9,
                      "note": "device events around back-to-back stage calls: the remap_prep_kernel launches (one per map) "
                              "and the remap kernel; the kernel's own time: rocprofv3 --kernel-trace --stats"}))
    h.close()


def part_intrinsics(args):
    device = torch.device("cuda", 0)
    B, n_loops, nF = args.seqs, min(args.seqs, args.loops), args.loop_frames
    plan = bench.loop_plan(B, n_loops, nF)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), nF, device)
    W, H = cfg["width"], cfg["height"]
    packs_for = bench.step_packer(lefts, rights, plan, True)
    slam = StereoSlamBatch(cfg, W, H, B, 0)
    groups = slam.groups()
    ids = slam.add_rigs([cfg] * B)                        # one rig per slot, the ctx's values
    per_leg = args.warmup + args.steps
    packed = packs_for(slam, 2 * args.pairs * per_leg)
    legs = {"rig0": [], "own_rig": []}
    k0 = 0
    for _ in range(args.pairs):
        for leg in ("rig0", "own_rig"):
            slam.assign_rigs(list(range(B)), ids if leg == "own_rig" else [0] * B)
            for k in range(k0, k0 + args.warmup):
                slam.submit_packed(packed[k])
            slam.wait()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(k0 + args.warmup, k0 + per_leg):
                slam.submit_packed(packed[k])
            slam.wait()
            torch.cuda.synchronize()
            legs[leg].append(B * args.steps / (time.perf_counter() - t0))
            k0 += per_leg
    slam.close()
    base, own = np.array(legs["rig0"]), np.array(legs["own_rig"])
    print(json.dumps({"part": "intrinsics", "config": "euroc", "seqs": B, "groups": groups, "steps_per_leg": args.steps,
                      "warmup_per_leg": args.warmup, "frames_per_s_rig0": base.round(0).tolist(),
                      "frames_per_s_own_rig": own.round(0).tolist(), "median_rig0": float(np.median(base)),
                      "median_own_rig": float(np.median(own)), "spread_rig0": float(base.max() - base.min()),
                      "ratio_of_medians": float(np.median(own) / np.median(base))}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("remap", "intrinsics"), required=True)
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="rigs256", help="(remap)")
    ap.add_argument("--remap-seqs", type=int, default=256, help="(remap) slots (2 images each)")
    ap.add_argument("--reps", type=int, default=20, help="(remap) timed calls")
    ap.add_argument("--seqs", type=int, default=3584, help="(intrinsics)")
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="(intrinsics) timed steps per leg")
    ap.add_argument("--warmup", type=int, default=8, help="(intrinsics) untimed steps at the start of every leg")
    ap.add_argument("--pairs", type=int, default=3, help="(intrinsics) rig0 / own_rig pairs")
    args = ap.parse_args()
    part_remap(args) if args.part == "remap" else part_intrinsics(args)


if __name__ == "__main__":
    main()
