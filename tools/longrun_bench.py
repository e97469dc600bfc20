"""What a sequence that runs without end costs with and without trimming its retired keyframes.

C2 `euroc` slots on a steady forward turn of 0.015 rad per frame (the turn of
test_keyframe_images_are_released_when_no_keypoint_needs_them: what a keyframe saw leaves the image for good, so
keyframes retire), closed after 419 frames and played round and round from a frame of the slot's own, as borrowed
device frames, pipelined. Two legs on fresh ctxs: the default (keep = -1: every keyframe stays) and
svo_ctx_set_keyframe_window(0). Per chunk of steps: frames/s, svo_memory.device_bytes, keyframe slabs in use, and the
resident keyframes of slot 0. These are measurements to report, not thresholds. Prints one JSON line (and writes it
to --out).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from stereo_svo_slam_amd import synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

TURN = 0.015                                              # rad per frame


def render_turns(cfg, n_scenes, device):
    """per scene the left and right frames of one full turn: [frames, H, W] uint8 device tensors"""
    n = int(round(2 * np.pi / TURN))
    poses = np.zeros((n, 6), np.float32)
    poses[:, 4] = 2 * np.pi * np.arange(n) / n
    lefts, rights = [], []
    for seed in range(n_scenes):
        scene = synth.Scene(seed, device)
        seeds = 7919 * (seed + 1) + 2 * np.arange(n)
        lefts.append(synth.render_frames_gpu(scene, cfg, poses, False, 1.0, seeds))
        rights.append(synth.render_frames_gpu(scene, cfg, poses, True, 1.0, seeds + 1))
    torch.cuda.synchronize(device)
    return n, lefts, rights


def leg(cfg, lefts, rights, n_loop, slots, steps, chunk, keep, device):
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, 0)
    slam.set_keyframe_window(keep)
    n_scenes = len(lefts)
    rows = []
    for c0 in range(0, steps, chunk):
        packed = [slam.pack_images([lefts[s % n_scenes][(53 * s + k) % n_loop] for s in range(slots)],
                                   [rights[s % n_scenes][(53 * s + k) % n_loop] for s in range(slots)],
                                   [k / 20.0] * slots, borrow=True) for k in range(c0, min(c0 + chunk, steps))]
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for pk in packed:
            slam.submit_packed(pk)
        slam.wait()
        sec = time.perf_counter() - t0
        m, r = slam.memory(), slam.keyframe_range(0)
        rows.append({"steps": c0 + len(packed), "frames_per_s": slots * len(packed) / sec, "device_bytes": m.device_bytes,
                     "keyframe_slabs_in_use": m.keyframe_slabs - m.keyframe_slabs_free, "keyframe_slabs": m.keyframe_slabs,
                     "slot0": {"first": r.first, "retired": r.retired, "count": r.count}})
        print(json.dumps({"keep": keep, **rows[-1]}), file=sys.stderr, flush=True)     # (progress)
    out = {"keep": keep, "keyframes": slam.totals().keyframes, "chunks": rows}
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    cfg = dict(synth.CONFIGS["euroc"])
    n_loop, lefts, rights = render_turns(cfg, min(args.scenes, args.slots), device)
    out = {"metric": "trim_bench", "config": "euroc", "slots": args.slots, "turn_rad_per_frame": TURN, "loop_frames": n_loop,
           "steps": args.steps, "legs": [leg(cfg, lefts, rights, n_loop, args.slots, args.steps, args.chunk, keep, device)
                                         for keep in (-1, 0)]}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
