"""What reading the tracker's state out costs on the MI355X: the per-sequence getters against the bulk export
(DESIGN §4.7).

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), once
with 256 slots in one group and once with 3584 slots in the ctx's default groups, in one process. Per leg, after a
warm-up, on the same state:

  getters    wall time of get_frame for every slot (svo_get_frame_keypoints + svo_get_pose: every call waits for the
             queues and makes twelve blocking copies), and per call.
  export     export_frames into pinned host memory and into device memory: the first call (it allocates: pinned
             buffers, the groups' staging blocks) and the median of `--repeats` more into the same buffers, with the
             bytes of the records delivered and bytes/s. The host-mode result is compared with the getters' bytes.
  pipelined  frames/s over `--steps` queued steps, without and with a host-mode export of every slot queued behind
             every frame set (two Export buffers in turn), legs alternating, median of three each; the bytes per
             step and the host-link rate they would need at the measured frame rate.
Prints one JSON line. Times are host clocks around work that ends in svo_wait and a device synchronise.
"""
import argparse
import json
import os
import statistics
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
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

RECORD_BYTES = 8 + 12 + 44          # svo_kp2d + svo_kp3d + svo_kp_info
HOST_LINK_GBS = 63.0                # the host link's specification, one direction


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def same_as_getters(e, frames):
    for i, f in enumerate(frames):
        g = e.frame(i)
        if not (g.kps2d.tobytes() == f.kps2d.tobytes() and g.kps3d.tobytes() == f.kps3d.tobytes() and
                g.info.tobytes() == f.info.tobytes() and g.pose.tobytes() == f.pose.tobytes()):
            return False
    return True


def leg(args, device, cfg, lefts, rights, slots, groups):
    if groups:
        os.environ["SVO_GROUPS"] = str(groups)
    else:
        os.environ.pop("SVO_GROUPS", None)
    n_loops, nF = len(lefts), lefts[0].shape[0]
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    K, W = args.steps, args.warmup
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, n_loops, nF), True)(slam, W + 6 * K)
    for pk in packed[:W]:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "groups": slam.groups(), "records_per_slot": slam.export_capacity()}

    # the getter loop: today's way out
    frames = []
    sec = timed(device, lambda: frames.extend(slam.get_frame(s) for s in range(slots)))
    out["getters"] = {"seconds": sec, "seconds_per_call": sec / slots, "keypoints": int(sum(len(f.kps2d) for f in frames))}

    # the export of the same state
    for mode, dev in (("export_host", False), ("export_device", True)):
        box = []
        first = timed(device, lambda: box.append(slam.export_frames(device=dev)))
        e = box[0]
        reps = [timed(device, lambda: e.submit().wait()) for _ in range(args.repeats)]
        n = int(e.segments["n"].sum())
        sec = statistics.median(reps)
        out[mode] = {"first_call_seconds": first, "seconds": sec, "seconds_all": reps, "keypoints": n,
                     "record_bytes": n * RECORD_BYTES, "bytes_per_s": n * RECORD_BYTES / sec,
                     "speedup_over_getters": out["getters"]["seconds"] / sec}
        if not dev:
            out[mode]["equals_getters"] = same_as_getters(e, frames)
            out[mode]["fraction_of_host_link"] = n * RECORD_BYTES / sec / (HOST_LINK_GBS * 1e9)
        del e, box
    del frames

    # exporting every step of the pipelined loop
    ring = [slam.export_frames(), slam.export_frames()]
    runs = {"plain": [], "with_export": []}
    bytes_per_step = []
    for r in range(6):
        steps = packed[W + r * K:W + (r + 1) * K]
        with_export = r % 2 == 1

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if with_export:
                    ring[k % 2].submit()
            slam.wait()
        sec = timed(device, run)
        runs["with_export" if with_export else "plain"].append(slots * K / sec)
        if with_export:
            bytes_per_step.append(int(ring[(K - 1) % 2].segments["n"].sum()) * RECORD_BYTES)
    plain, exported = statistics.median(runs["plain"]), statistics.median(runs["with_export"])
    b = statistics.median(bytes_per_step)
    out["pipelined"] = {"steps": K, "frames_per_s": plain, "frames_per_s_all": runs["plain"],
                        "frames_per_s_with_export": exported, "frames_per_s_with_export_all": runs["with_export"],
                        "with_export_vs_plain": exported / plain, "export_bytes_per_step": b,
                        "host_link_bytes_per_s_needed": b * exported / slots,
                        "fraction_of_host_link": b * exported / slots / (HOST_LINK_GBS * 1e9),
                        "seconds_per_step": slots / plain, "seconds_per_step_with_export": slots / exported}
    m = slam.memory()
    out["device_GB"] = m.device_bytes / 1e9
    slam.close()
    del packed, ring
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="256:1,3584:0", help="slots:groups per leg (groups 0: the ctx's default)")
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run (six runs per leg)")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5, help="timed exports per mode")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",")]
    n_loops = min(max(s for s, _ in legs), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    out = {"metric": "export_bench", "config": "euroc", "record_bytes_per_keypoint": RECORD_BYTES,
           "host_link_spec_GBs": HOST_LINK_GBS,
           "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "legs": []}
    for slots, groups in legs:
        n = min(slots, n_loops)
        out["legs"].append(leg(args, device, cfg, lefts[:n], rights[:n], slots, groups))
        print(json.dumps(out["legs"][-1]), file=sys.stderr, flush=True)   # (progress)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
