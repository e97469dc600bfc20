"""What looking at the maps costs on the MI355X: the scene job alone, the host path it replaces, and scenes queued
between the steps of bench.py's workload.

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), in one
process:

  kernel     256 slots in one group, after a warm-up that gives every slot a few keyframes: the slots' keyframes
             (through the getters, uploaded again as SoA planes), trajectories and frusta rendered through the stage
             entry svo_render_scene at 256 x 256 and 752 x 480 RGBA through the front camera; median of `--repeats`
             calls between two device events. A call is the upload of its set, image and tile tables, the kernel and
             a stream synchronise; bytes = image bytes written. The kernel's own time, without the uploads, comes from
             a `rocprofv3 --kernel-trace --stats` run of this tool with --kernel-only, in a run of its own: this tool
             cannot record it.
  job        the ctx's own device-mode scene job of every slot (submit + wait, host clock) at both sizes: the host's
             line and table building, one upload, the kernel and a stream synchronise. Beside it, on the same output
             bytes at 752 x 480: the device-mode RGBA view job of §4.11 and svo_copy_segments (device events).
  host path  what a dashboard does without the job: export_map of every slot into host memory (the points a host
             rasteriser would then draw; the rasterising itself is not timed), and the host-mode scene job.
  pipelined  frames/s over `--steps` queued steps without scenes and with a device-mode 256 x 256 scene of every slot
             queued behind every 10th frame set; legs alternate, median of `--repeats` each.
Prints one JSON line.
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
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

HBM_PEAK = 8.0e12
SIZES = ((256, 256), (752, 480))


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def median_ms(device, fn, repeats):
    fn()
    all_ms = [timed(device, fn) * 1e3 for _ in range(repeats)]
    return statistics.median(all_ms), all_ms


def start(cfg, lefts, rights, slots, groups, device, steps):
    if groups:
        os.environ["SVO_GROUPS"] = str(groups)
    else:
        os.environ.pop("SVO_GROUPS", None)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, len(lefts), lefts[0].shape[0]), True)(slam, steps)
    return slam, packed


def event_ms(fn, repeats):
    """median of the device time between two events around fn(), on the current stream"""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def kernel_leg(args, device, slam, slots):
    """the stage entry on the slots' own maps: what a scene job of every slot hands to the kernel"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    style0 = hip_lib.scene_style()
    sources, n_kps, n_lines = [], 0, 0
    for s in range(slots):
        sets, rec = [], []
        for k in range(slam.num_keyframes(s)):
            f = slam.get_keyframe(k, s)
            info = f.info
            flags = (info["ignore_during_refinement"].astype(np.uint32) | info["ignore_completely"].astype(np.uint32) << 1 |
                     info["ignore_temporary"].astype(np.uint32) << 2)
            col = info["color"].astype(np.uint32).reshape(-1, 3)
            sets.append((len(info), k, {"kps3d": dev(f.kps3d), "flags": dev(flags), "keyframe_id": dev(info["keyframe_id"]),
                                        "inlier_count": dev(info["inlier_count"]), "color": dev(col[:, 0] | col[:, 1] << 8 | col[:, 2] << 16)}))
            n_kps += len(info)
            rec += [(l[:3], l[3:], hip_lib.SCENE_CLASS_KEYFRAME << 24 | style0.keyframe_rgb, 0) for l in hip_lib.scene_frustum(f.pose)]
        t = slam.get_trajectory(s)[:, :3]
        rec += [(t[j], t[j + 1], hip_lib.SCENE_CLASS_TRAJECTORY << 24 | style0.trajectory_rgb, 0) for j in range(len(t) - 1)]
        rec += [(l[:3], l[3:], hip_lib.SCENE_CLASS_POSE << 24 | style0.pose_rgb, 0) for l in hip_lib.scene_frustum(slam.pose(s))]
        lines = np.array(rec, hip_lib.SCENE_LINE_DTYPE)
        n_lines += len(lines)
        sources.append((sets, dev(lines.view(np.uint8).reshape(-1))))
    h = hip_lib.Handle(device.index, 1024)
    out = {"slots": slots, "keypoints": n_kps, "lines": n_lines, "sizes": {}}
    for cols, rows in SIZES:
        style = hip_lib.scene_style(cols=cols, rows=rows, pixel="rgba8")
        pitch, image_bytes = hip_lib.scene_size(style)
        dst = torch.empty(slots * image_bytes, dtype=torch.uint8, device=device)
        cam = hip_lib.scene_preset("front", cols, rows)
        packed = h.pack_scene([(cols, rows, sets, lines) for sets, lines in sources], [cam] * slots,
                              [i * image_bytes for i in range(slots)], )
        call = lambda: h.render_scene_packed(packed, style, dst)
        call()
        if args.kernel_only:
            continue
        ms, all_ms = event_ms(call, args.repeats)
        written = slots * rows * pitch
        out["sizes"][f"{cols}x{rows}"] = {"call_ms": ms, "call_ms_all": all_ms, "bytes_written": written, "bytes_per_s": written / (ms * 1e-3),
                                          "fraction_of_hbm_peak": written / (ms * 1e-3) / HBM_PEAK,
                                          "tiles": slots * ((cols + 63) // 64) * ((rows + 15) // 16)}
        del dst
    h.close()
    return out


def job_leg(args, device, cfg, lefts, rights):
    slots = args.slots
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "warmup_steps": args.warmup, "sizes": {}, "kernel": kernel_leg(args, device, slam, slots)}
    for cols, rows in SIZES:
        sc = slam.submit_scenes(camera="front", device=True, cols=cols, rows=rows, pixel="rgba8").wait()
        if args.kernel_only:
            continue
        ms, all_ms = median_ms(device, lambda: sc.submit().wait(), args.repeats)
        written = slots * rows * sc.pitch
        seg = sc.segments
        out["sizes"][f"{cols}x{rows}"] = {
            "job_ms": ms, "job_ms_all": all_ms, "bytes_written": written, "bytes_per_s": written / (ms * 1e-3),
            "fraction_of_hbm_peak": written / (ms * 1e-3) / HBM_PEAK, "keyframes": int(seg["n_keyframes"].sum()),
            "keypoints": int(seg["n_keypoints"].sum()), "trajectory_poses": int(seg["n_poses"].sum())}
        if (cols, rows) == SIZES[0]:
            host = slam.submit_scenes(camera="front", cols=cols, rows=rows, pixel="rgba8").wait()
            out["host_mode_job_ms"], out["host_mode_job_ms_all"] = median_ms(device, lambda: host.submit().wait(), args.repeats)
            del host
        del sc
    if not args.kernel_only:
        # the same output bytes at 752 x 480 RGBA: the view job of §4.11 and the copy kernel
        W, H = cfg["width"], cfg["height"]
        v = slam.submit_views("frames", pixel="rgba8", device=True).wait()
        ms, all_ms = median_ms(device, lambda: v.submit().wait(), args.repeats)
        out["view_rgba8_job"] = {"cols": W, "rows": H, "job_ms": ms, "job_ms_all": all_ms, "bytes_written": v.capacity,
                                 "bytes_per_s": v.capacity / (ms * 1e-3)}
        h = hip_lib.Handle(device.index, 1024)
        copy = torch.empty(v.capacity, dtype=torch.uint8, device=device)
        row = 4 * W
        segs = [(v.pixels.data_ptr() + i * v.image_bytes, copy.data_ptr() + i * v.image_bytes, row, H, row, row) for i in range(slots)]
        h.copy_segments(segs)
        all_ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            h.copy_segments(segs)
            b.record()
            b.synchronize()
            all_ms.append(a.elapsed_time(b))
        ms = statistics.median(all_ms)
        out["copy_segments_rgba8"] = {"call_ms": ms, "call_ms_all": all_ms, "bytes_written": slots * row * H,
                                      "bytes_per_s": slots * row * H / (ms * 1e-3)}
        h.close()
        # the host path: every slot's points into host memory
        m = slam.export_map()
        ms, all_ms = median_ms(device, lambda: m.submit().wait(), args.repeats)
        out["export_map_to_host"] = {"job_ms": ms, "job_ms_all": all_ms, "points": int(m.segments["n_points"].sum()),
                                     "bytes": 16 * int(m.segments["n_points"].sum())}
    slam.close()
    return out


def pipelined_leg(args, device, cfg, lefts, rights, slots, groups):
    K, W, every = args.steps, args.warmup, 10
    n = min(slots, len(lefts))
    runs_n = 2 * args.pipelined_repeats
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, groups, device, W + runs_n * K)
    for pk in packed[:W]:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "groups": slam.groups(), "steps": K, "scene_every": every}
    ring = [slam.submit_scenes(camera="front", device=True, cols=256, rows=256, pixel="rgba8").wait() for _ in range(2)]
    runs = {"plain": [], "scenes": []}
    for r in range(runs_n):
        kind = ("plain", "scenes")[r % 2]
        steps = packed[W + r * K:W + (r + 1) * K]

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if kind == "scenes" and k % every == every - 1:
                    ring[(k // every) % 2].submit()
            slam.wait()
        runs[kind].append(slots * K / timed(device, run))
    for kind in runs:
        out[f"frames_per_s_{kind}"] = statistics.median(runs[kind])
        out[f"frames_per_s_{kind}_all"] = runs[kind]
    out["scenes_vs_plain"] = out["frames_per_s_scenes"] / out["frames_per_s_plain"]
    out["scene_bytes_per_job"] = ring[0].capacity
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--kernel-only", action="store_true", help="one job per size and nothing timed: for a kernel trace")
    ap.add_argument("--legs", default="256:1", help="slots:groups per pipelined leg (groups 0: the ctx's default); '' for none")
    ap.add_argument("--loops", type=int, default=64)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run")
    ap.add_argument("--warmup", type=int, default=60, help="steps before anything is timed (a keyframe every ~26 frames)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--pipelined-repeats", type=int, default=9, help="timed runs per kind of a pipelined leg")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",") if l] if not args.kernel_only else []
    n_loops = min(max([s for s, _ in legs] + [args.slots]), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    out = {"metric": "scene_bench", "config": "euroc", "hbm_peak_bytes_per_s": HBM_PEAK,
           "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "job": job_leg(args, device, cfg, lefts, rights), "legs": []}
    print(json.dumps(out["job"]), file=sys.stderr, flush=True)        # (progress)
    for slots, groups in legs:
        out["legs"].append(pipelined_leg(args, device, cfg, lefts, rights, slots, groups))
        print(json.dumps(out["legs"][-1]), file=sys.stderr, flush=True)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
