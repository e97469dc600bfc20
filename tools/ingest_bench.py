"""Cost of the GPU input formats (svo_ctx_set_input_format / svo_convert_frames) on the MI355X.

  (a) python tools/ingest_bench.py --part a
      bench.py's default workload (C2 `euroc`, 3584 sequences in the ctx's default groups, borrowed device frames,
      pipelined submits) on one ctx, alternating the default format (two gray images per sequence) and the same
      frames packed as SVO_INPUT_SBS_BGR with R = G = B (one 1504 x 480 x 3 frame per sequence: the tracking work
      is the same in both legs) in `--pairs` pairs; frames/s of every leg, the medians and the on/off ratio, and
      the time per step that the frame's bytes would take at the copy rate of part (b) (--copy-gbs).
  (b) python tools/ingest_bench.py --part b
      the kernel alone: 256 SBS_BGR frames of 1504 x 480 -> 512 gray images (svo_convert_frames, n = 256) timed with
      device events around back-to-back calls; bytes moved = 3 B read + 1 B written per pixel, their share of the
      8 TB/s peak; and, in the same process with the same timing, a plain device-to-device copy that moves the
      same total bytes. Run it under `rocprofv3 --kernel-trace --stats -- python tools/ingest_bench.py --part b`
      for the kernel's own time (ingest_kernel).
Prints one JSON line per part.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting: 14 groups of 256)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

HBM_PEAK_GBS = 8000.0


def part_a(args):
    device = torch.device("cuda", 0)
    B, n_loops, nF = args.seqs, min(args.seqs, args.loops), args.loop_frames
    plan = bench.loop_plan(B, n_loops, nF)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), nF, device)
    W, H = cfg["width"], cfg["height"]
    # the same frames side by side with R = G = B, one loop at a time (right image = left half of the frame)
    sbs = [torch.cat([r, l], 2)[..., None].expand(-1, -1, -1, 3).contiguous() for l, r in zip(lefts, rights)]
    slam = StereoSlamBatch(cfg, W, H, B, 0)
    groups = slam.groups()
    n_steps = args.warmup + 2 * args.pairs * args.steps
    packed_gray = bench.step_packer(lefts, rights, plan, True)(slam, n_steps)
    slam.set_input_format("sbs_bgr")
    packed_sbs = bench.step_packer(sbs, sbs, plan, True)(slam, n_steps)
    slam.set_input_format("gray_pair")
    for k in range(args.warmup):
        slam.submit_packed(packed_gray[k])
    slam.wait()
    k0 = args.warmup
    legs = {"off": [], "on": []}
    for _ in range(args.pairs):
        for leg in ("off", "on"):
            slam.set_input_format("sbs_bgr" if leg == "on" else "gray_pair")
            packed = packed_sbs if leg == "on" else packed_gray
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
    frame_bytes = 4 * 2 * W * H                              # 3 B read + 1 B written per pixel of both images
    ms_off, ms_on = 1e3 * B / np.median(off), 1e3 * B / np.median(on)
    out = {"part": "a", "config": "euroc", "seqs": B, "groups": groups, "steps_per_leg": args.steps,
           "frames_per_s_off": off.round(0).tolist(), "frames_per_s_on": on.round(0).tolist(),
           "median_off": float(np.median(off)), "median_on": float(np.median(on)),
           "ratio_of_medians": float(np.median(on) / np.median(off)),
           "ms_per_step_off": float(ms_off), "ms_per_step_on": float(ms_on), "ms_per_step_added": float(ms_on - ms_off),
           "frame_bytes_moved": frame_bytes}
    if args.copy_gbs:
        out["copy_gb_per_s"] = args.copy_gbs
        out["ms_per_step_expected"] = B * frame_bytes / (args.copy_gbs * 1e9) * 1e3
    print(json.dumps(out))


def _timed(call, reps):
    """median / min / max ms per call over 5 batches of `reps` calls queued back to back between two events"""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(5):
        ev[0].record()
        for _ in range(reps):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / reps)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def part_b(args):
    W, H, n = 752, 480, args.frames
    h = hip_lib.Handle(0, 64)
    gen = torch.Generator(device="cuda").manual_seed(0)
    srcs = [torch.randint(0, 256, (H, 2 * W, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(n)]
    lefts = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(n)]
    rights = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(n)]
    arr_a = (hip_lib.Image * n)(*[hip_lib._raw_img(t, 3) for t in srcs])
    arr_l, arr_r = hip_lib._imgs(lefts), hip_lib._imgs(rights)
    call = lambda: hip_lib._check(hip_lib.lib().svo_convert_frames(h._h, hip_lib.INPUT_SBS_BGR, n, arr_a, None, arr_l, arr_r))
    ms, lo, hi = _timed(call, args.reps)
    read_bytes, written_bytes = 3 * 2 * W * H * n, 2 * W * H * n
    moved = read_bytes + written_bytes
    # a plain device-to-device copy that moves the same total bytes (reads half of them, writes half)
    a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    cms, clo, chi = _timed(lambda: b.copy_(a), args.reps)
    print(json.dumps({"part": "b", "frames": n, "images": 2 * n, "size": [W, H], "format": "sbs_bgr",
                      "call_ms_median": ms, "call_ms_min": lo, "call_ms_max": hi,
                      "bytes_moved": moved, "bytes_read": read_bytes, "bytes_written": written_bytes,
                      "gb_per_s": moved / (ms * 1e-3) / 1e9, "hbm_peak_fraction": moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "copy_ms_median": cms, "copy_ms_min": clo, "copy_ms_max": chi,
                      "copy_gb_per_s": moved / (cms * 1e-3) / 1e9,
                      "copy_hbm_peak_fraction": moved / (cms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "note": "device events around back-to-back calls: table upload + ingest_kernel; copy = torch copy_ of bytes_moved / 2"}))
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
    ap.add_argument("--copy-gbs", type=float, default=0.0, help="(a) the copy rate of part (b), GB/s: the expected cost")
    ap.add_argument("--frames", type=int, default=256, help="(b) side-by-side frames (2 images each)")
    ap.add_argument("--reps", type=int, default=50, help="(b) timed calls")
    args = ap.parse_args()
    part_a(args) if args.part == "a" else part_b(args)


if __name__ == "__main__":
    main()
