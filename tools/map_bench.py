"""What reading the whole map out costs on the MI355X: the get_keyframe loop against the map export.

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), once
with 256 slots in one group and once with 3584 slots in the ctx's default groups, in one process. Per leg, after a
warm-up, on the same state:

  getters    wall time of get_keyframe for every keyframe of every slot (what wire.keyframes_message does: every
             call waits for the queues and makes twelve blocking copies), and per call.
  export     export_map of every slot, unfiltered and with own_only + drop_flags = IGNORE_COMPLETELY, into pinned
             host memory and into device memory: the first call (it sizes the regions and allocates: pinned buffers,
             the groups' counts and staging blocks) and the median of `--repeats` more into the same buffers, with
             the points delivered, their bytes (16 each) and bytes/s. The unfiltered host-mode result is compared
             with the getters' kps3d and colours.
  pipelined  frames/s over `--steps` queued steps, without and with a host-mode filtered map export of every slot
             queued behind every `--every`-th frame set (regions with room for `--room` more keyframes per slot), legs
             alternating, median of three each; the slots that came back TOO_SMALL are counted.
Prints one JSON line. Times are host clocks around work that ends in svo_wait and a device synchronise. The
kernels' own times (bytes / time against the HBM peak) come from a `rocprofv3 --kernel-trace --stats` run of this
tool, in a run of its own.
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
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import MapExport, StereoSlamBatch

POINT_BYTES = 16                    # svo_map_point
GETTER_RECORD_BYTES = 8 + 12 + 44   # what get_keyframe moves per keypoint
HOST_LINK_GBS = 63.0                # the host link's specification, one direction
FILTERS = {"all": None, "own_current": dict(drop_flags=hip_lib.IGNORE_COMPLETELY, own_only=1)}


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def same_as_getters(m, keyframes):
    """the unfiltered export against the getters: kps3d bits and colours of every keyframe of every slot"""
    for i, kfs in enumerate(keyframes):
        if len(m.keyframes(i)) != len(kfs):
            return False
        for k, f in enumerate(kfs):
            p = m.points_of_keyframe(i, k)
            got = np.stack([p["x"], p["y"], p["z"]], 1) if len(p) else np.zeros((0, 3), np.float32)
            if got.tobytes() != f.kps3d.tobytes() or p["color"].tobytes() != np.ascontiguousarray(f.info["color"]).tobytes():
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
    out = {"slots": slots, "groups": slam.groups(), "warmup_steps": W}

    # the getter loop: today's way to the whole map
    keyframes = []
    sec = timed(device, lambda: keyframes.extend(slam.get_keyframes(s) for s in range(slots)))
    calls = sum(len(k) for k in keyframes)
    points = int(sum(len(f.kps3d) for k in keyframes for f in k))
    out["getters"] = {"seconds": sec, "calls": calls, "seconds_per_call": sec / max(calls, 1), "keypoints": points,
                      "record_bytes": points * GETTER_RECORD_BYTES}

    # the map export of the same state
    for fname, filt in FILTERS.items():
        for mode, dev in (("host", False), ("device", True)):
            box = []
            first = timed(device, lambda: box.append(slam.export_map(filter=filt, device=dev)))
            m = box[0]
            reps = [timed(device, lambda: m.submit().wait()) for _ in range(args.repeats)]
            n = int(m.segments["n_points"].sum())
            sec = statistics.median(reps)
            r = {"first_call_seconds": first, "seconds": sec, "seconds_all": reps, "points": n,
                 "points_bound": int(m.segments["points_bound"].sum()), "point_bytes": n * POINT_BYTES,
                 "bytes_per_s": n * POINT_BYTES / sec, "speedup_over_getters": out["getters"]["seconds"] / sec,
                 "too_small": int((m.segments["status"] != hip_lib.MAP_COMPLETE).sum())}
            if not dev:
                r["fraction_of_host_link"] = n * POINT_BYTES / sec / (HOST_LINK_GBS * 1e9)
                if filt is None:
                    r["equals_getters"] = same_as_getters(m, keyframes)
            out[f"export_{fname}_{mode}"] = r
            del m, box
    del keyframes

    # a filtered map export every `every` steps of the pipelined loop; regions with room for `--room` more keyframes
    sizes = [slam.map_size(s) for s in range(slots)]
    cap = slam.export_capacity()
    room = args.room
    ring = [MapExport(slam, None, None, FILTERS["own_current"], False, [p + room * cap for _, p in sizes],
                      [k + room for k, _ in sizes]) for _ in range(2)]
    runs = {"plain": [], "with_map": []}
    too_small, bytes_per_export = 0, []
    for r in range(6):
        steps = packed[W + r * K:W + (r + 1) * K]
        with_map = r % 2 == 1
        used = []

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if with_map and k % args.every == args.every - 1:
                    used.append(ring[len(used) % 2].submit())
            slam.wait()
        sec = timed(device, run)
        runs["with_map" if with_map else "plain"].append(slots * K / sec)
        if used:
            too_small += int((used[-1].segments["status"] != hip_lib.MAP_COMPLETE).sum())
            bytes_per_export.append(int(used[-1].segments["n_points"].sum()) * POINT_BYTES)
    plain, mapped = statistics.median(runs["plain"]), statistics.median(runs["with_map"])
    out["pipelined"] = {"steps": K, "every": args.every, "frames_per_s": plain, "frames_per_s_all": runs["plain"],
                        "frames_per_s_with_map": mapped, "frames_per_s_with_map_all": runs["with_map"],
                        "with_map_vs_plain": mapped / plain, "map_bytes_per_export": statistics.median(bytes_per_export or [0]),
                        "slots_too_small_in_last_exports": too_small}
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    del packed, ring
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="256:1,3584:0", help="slots:groups per leg (groups 0: the ctx's default)")
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run (six runs per leg)")
    ap.add_argument("--every", type=int, default=10, help="a map export behind every so many frame sets")
    ap.add_argument("--room", type=int, default=4, help="keyframes a slot may add before its pipelined exports come back TOO_SMALL")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5, help="timed exports per filter and mode")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",")]
    n_loops = min(max(s for s, _ in legs), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    out = {"metric": "map_bench", "config": "euroc", "point_bytes": POINT_BYTES,
           "getter_record_bytes_per_keypoint": GETTER_RECORD_BYTES, "host_link_spec_GBs": HOST_LINK_GBS,
           "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "legs": []}
    for slots, groups in legs:
        n = min(slots, n_loops)
        out["legs"].append(leg(args, device, cfg, lefts[:n], rights[:n], slots, groups))
        print(json.dumps(out["legs"][-1]), file=sys.stderr, flush=True)   # (progress)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
