"""What looking at the slots costs on the MI355X: the view kernel alone, and views queued behind every step of
bench.py's workload.

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), in one
process:

  kernel     256 slots in one group, after a warm-up: the slots' current gray planes (a device-mode gray view) and
             their keypoints (a device-mode export) rendered through the stage entry svo_render_views, per pixel
             format, without and with markers, level 0; median of `--repeats` calls between two device events on the
             handle's stream. A call is the upload of its tile table, the kernel and a stream synchronise; bytes moved
             = gray bytes read + image bytes written (+ 16 bytes per keypoint and tile with markers: not counted),
             against the 8 TB/s HBM peak. For comparison svo_copy_segments on the same gray bytes (one segment per
             plane, dense to dense), a call of the same structure, and the ctx's own device-mode jobs
             (submit_views + wait, host clock). The kernel's own time, without the table upload, comes from a
             `rocprofv3 --kernel-trace --stats` run of this tool with --kernel-only, in a run of its own.
  pipelined  per leg (slots:groups) frames/s over `--steps` queued steps without views and with a device-mode view
             of every slot (RGB8 with markers, then gray) queued behind every frame set; legs alternate, median of
             three each.
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
from stereo_svo_slam_amd.stereo_slam import KP_INFO_DTYPE, StereoSlamBatch

HBM_PEAK = 8.0e12
CASES = (("gray8", False), ("rgb8", False), ("rgba8", False), ("rgb8", True), ("rgba8", True))


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


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


def start(cfg, lefts, rights, slots, groups, device, steps):
    if groups:
        os.environ["SVO_GROUPS"] = str(groups)
    else:
        os.environ.pop("SVO_GROUPS", None)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, len(lefts), lefts[0].shape[0]), True)(slam, steps)
    return slam, packed


def kernel_leg(args, device, cfg, lefts, rights):
    slots = args.kernel_slots
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    W, H = cfg["width"], cfg["height"]
    gray = slam.export_views("frames", device=True)                     # the planes the kernel reads: dense, 256-byte aligned
    exp = slam.export_frames(device=True)
    info = exp.info.cpu().numpy().view(KP_INFO_DTYPE)[:, 0]
    flags = (info["ignore_during_refinement"].astype(np.uint32) | info["ignore_completely"].astype(np.uint32) << 1 |
             info["ignore_temporary"].astype(np.uint32) << 2)
    color = (info["color"][:, 0].astype(np.uint32) | info["color"][:, 1].astype(np.uint32) << 8 | info["color"][:, 2].astype(np.uint32) << 16)
    d_flags = torch.from_numpy(flags).to(device)
    d_lt = torch.from_numpy((info["type"] << 8).astype(np.int32)).to(device)
    d_color = torch.from_numpy(color).to(device)
    h = hip_lib.Handle(device.index, 1024)
    srcs, n_kps = [], 0
    for i, e in enumerate(exp.segments):
        lo, n = int(e["first"]), int(e["n"])
        n_kps += n
        fields = {"kps2d": exp.kps2d[lo:].data_ptr(), "flags": d_flags[lo:].data_ptr(), "level_type": d_lt[lo:].data_ptr(),
                  "color": d_color[lo:].data_ptr()}
        srcs.append(((gray.pixels.data_ptr() + int(gray.segments[i]["offset"]), W, H, W), (n, fields)))
    out = {"slots": slots, "keypoints": n_kps, "gray_bytes": slots * W * H, "cases": {}}
    for pixel, markers in CASES:
        style = hip_lib.view_style(hip_lib.EXPORT_FRAMES, "left", 0, pixel, markers)
        _, _, pitch, image_bytes = slam.view_size(style)
        dst = torch.empty(slots * image_bytes, dtype=torch.uint8, device=device)
        offsets = [i * image_bytes for i in range(slots)]
        call = lambda: h.render_views(srcs, offsets, style, dst)
        call()
        if args.kernel_only:
            continue
        ms, all_ms = event_ms(call, args.repeats)
        moved = slots * (W * H + H * pitch)
        v = slam.submit_views("frames", pixel=pixel, markers=markers, device=True).wait()
        job = statistics.median([timed(device, lambda: v.submit().wait()) for _ in range(args.repeats)])
        out["cases"][f"{pixel}{'_markers' if markers else ''}"] = {
            "call_ms": ms, "call_ms_all": all_ms, "bytes_moved": moved, "bytes_per_s": moved / (ms * 1e-3),
            "fraction_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK, "ctx_job_ms": job * 1e3, "ctx_job_bytes_per_s": moved / job}
        del dst, v
    # svo_copy_segments on the same gray bytes
    copy = torch.empty(slots * W * H, dtype=torch.uint8, device=device)
    segs = [(s[0][0], copy.data_ptr() + i * W * H, W, H, W, W) for i, s in enumerate(srcs)]
    h.copy_segments(segs)
    if not args.kernel_only:
        ms, all_ms = event_ms(lambda: h.copy_segments(segs), args.repeats)
        moved = 2 * slots * W * H
        out["copy_segments_gray"] = {"call_ms": ms, "call_ms_all": all_ms, "bytes_moved": moved, "bytes_per_s": moved / (ms * 1e-3),
                                     "fraction_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK}
    h.close()
    slam.close()
    return out


def pipelined_leg(args, device, cfg, lefts, rights, slots, groups):
    K, W = args.steps, args.warmup
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, groups, device, W + 9 * K)
    for pk in packed[:W]:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "groups": slam.groups(), "steps": K}
    kinds = {"plain": None, "rgb8_markers": dict(pixel="rgb8", markers=True), "gray8": dict(pixel="gray8")}
    rings = {k: [slam.submit_views("frames", device=True, **kw).wait() for _ in range(2)] for k, kw in kinds.items() if kw}
    runs = {k: [] for k in kinds}
    for r in range(9):
        kind = list(kinds)[r % 3]
        steps = packed[W + r * K:W + (r + 1) * K]

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if kind != "plain":
                    rings[kind][k % 2].submit()
            slam.wait()
        runs[kind].append(slots * K / timed(device, run))
    for kind in kinds:
        out[f"frames_per_s_{kind}"] = statistics.median(runs[kind])
        out[f"frames_per_s_{kind}_all"] = runs[kind]
    for kind in rings:
        out[f"{kind}_vs_plain"] = out[f"frames_per_s_{kind}"] / out["frames_per_s_plain"]
        out[f"{kind}_image_bytes_per_step"] = rings[kind][0].capacity
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-slots", type=int, default=256)
    ap.add_argument("--kernel-only", action="store_true", help="one call per case and nothing timed: for a kernel trace")
    ap.add_argument("--legs", default="256:1,1024:0", help="slots:groups per pipelined leg (groups 0: the ctx's default); '' for none")
    ap.add_argument("--loops", type=int, default=64)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run (nine runs per leg)")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",") if l] if not args.kernel_only else []
    n_loops = min(max([s for s, _ in legs] + [args.kernel_slots]), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    out = {"metric": "view_bench", "config": "euroc", "hbm_peak_bytes_per_s": HBM_PEAK,
           "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "kernel": kernel_leg(args, device, cfg, lefts, rights), "legs": []}
    print(json.dumps(out["kernel"]), file=sys.stderr, flush=True)        # (progress)
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
