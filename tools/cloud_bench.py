"""What a dense point cloud costs on the MI355X: the two new kernels alone, the stage entry with the
search, and the job in a ctx against the two things it is set against.

One process, bench.py's rendered `euroc` stereo pairs (752 x 480), the EuRoC settings 31 / 60 / 6, lattice steps 1, 2
and 4, 1, 16 and 256 images:

  kernel   svo_cloud_points (compact, world frame, min_disparity 2): device time between two events around the call
           (two table uploads, the search, the count and write launches, a stream synchronise), per image; the same
           call with SVO_CLOUD_SKIP_SEARCH=1 (the count and write launches alone, on the planes of the call before);
           and svo_dense_disparity with the cost plane on the same pairs (what the cloud adds is the difference). The
           bytes the two kernels move per image are counted from the statement (17 B per lattice point in, 16 B per kept
           point out) and set against 8 TB/s. Every shape is warmed up first; the legs alternate, median of `--repeats`.
           With `--sgm P1,P2[,CAP]` a further leg: svo_cloud_points_sgm (the cloud of the SGM map) on the
           same pairs, with `--checked D` under the SGM map's own cross-check as well.
  job      in a ctx of 256 slots after `--warmup` steps of bench.py's workload, for the first 1, 16 and 256 slots:
           a cloud job into device and into host memory, (a) a disparity job with the cost plane into device memory, and
           (b) the host path the cloud job replaces: export_disparity(value="disparity", cost=True) into host memory
           followed by a numpy restatement of the triangulation, the filter and the compaction (the gray comes from a
           host copy of the left planes that is made outside the timed region). Wall time of submit + wait, per image;
           legs alternate, median of `--repeats` (the host path: `--host-repeats`).
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import Clouds, Disparities, StereoSlamBatch

POSE = (0.3, -0.2, 1.1, 0.05, -0.12, 0.2)
MIN_DISPARITY = 2.0
PEAK_BYTES_PER_S = 8e12
RIG_KEYS = ("baseline", "fx", "fy", "cx", "cy")


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_leg(args, device, cfg, lefts, rights):
    W, H = cfg["width"], cfg["height"]
    win, sx, sy = cfg["window_size_depth_calculator"], cfg["search_x"], cfg["search_y"]
    h = hip_lib.Handle(device.index, 4096)
    nF = lefts[0].shape[0]
    pair = lambda i: (lefts[i % len(lefts)][(i // len(lefts)) * 7 % nF], rights[i % len(rights)][(i // len(lefts)) * 7 % nF])
    rig = {k: cfg[k] for k in RIG_KEYS}
    out = {"width": W, "height": H, "win": win, "search_x": sx, "search_y": sy, "min_disparity": MIN_DISPARITY, "shapes": []}
    for step in args.lattice_steps:
        cols, rows = W // step, H // step
        P = cols * rows
        style = hip_lib.cloud_style(step, win, sx, sy, "world", "compact", min_disparity=MIN_DISPARITY)
        dstyle = hip_lib.DisparityStyle(hip_lib.DENSE_DISPARITY, step, win, sx, sy, 1)
        for n in args.images:
            pairs = [pair(i) for i in range(n)]
            points = torch.empty((n * P, 16), dtype=torch.uint8, device=device)
            counts = torch.zeros(n, dtype=torch.int32, device=device)
            planes = torch.empty(n * 2 * P, dtype=torch.float32, device=device)
            packed = h.pack_cloud([((l, W, H, l.stride(0)), (r, W, H, r.stride(0)), rig, POSE) for l, r in pairs], [i * P for i in range(n)])
            packed_d = h.pack_dense([((l, W, H, l.stride(0)), (r, W, H, r.stride(0)), cfg["baseline"]) for l, r in pairs],
                                    [i * 2 * P * 4 for i in range(n)])
            cloud = lambda: h.cloud_points_packed(packed, style, points, counts)
            dense = lambda: h.dense_disparity_packed(packed_d, dstyle, planes)

            def kernels():
                os.environ["SVO_CLOUD_SKIP_SEARCH"] = "1"
                try:
                    cloud()
                finally:
                    del os.environ["SVO_CLOUD_SKIP_SEARCH"]
            checked, kept_checked = None, None
            if args.checked is not None:                     # (the left-right cross-check of DESIGN 4.19 at that tolerance)
                check = hip_lib.stereo_check(True, args.checked)
                checked = lambda: h.cloud_points_packed(packed, style, points, counts, check)
                checked()
                torch.cuda.synchronize(device)
                kept_checked = int(counts.sum().item())
            sgm_legs, sgm_kept = {}, {}
            if args.sgm:                                     # (the cloud of the SGM map, and under its own cross-check)
                sp = hip_lib.sgm_params(args.sgm[0], args.sgm[1], args.sgm[2] if len(args.sgm) > 2 else hip_lib.SGM_DEFAULTS["cost_cap"])
                sgm_legs["sgm_cloud"] = lambda: h.cloud_points_sgm_packed(packed, style, sp, points, counts)
                if args.checked is not None:
                    sgm_legs["sgm_checked_cloud"] = lambda: h.cloud_points_sgm_packed(packed, style, sp, points, counts, check)
                for k, leg in sgm_legs.items():
                    leg()
                    torch.cuda.synchronize(device)
                    sgm_kept[k] = int(counts.sum().item())
            t_sgm = {k: [] for k in sgm_legs}
            cloud(); dense(); kernels()                      # warm-up of the legs
            torch.cuda.synchronize(device)
            kept = int(counts.sum().item())
            t_cloud, t_dense, t_kernels, t_checked = [], [], [], []
            for _ in range(args.repeats):                   # the legs alternate
                t_cloud.append(event_ms(cloud))
                t_dense.append(event_ms(dense))
                t_kernels.append(event_ms(kernels))
                if checked:
                    t_checked.append(event_ms(checked))
                for k, leg in sgm_legs.items():
                    t_sgm[k].append(event_ms(leg))
            c_ms, d_ms, k_ms = (statistics.median(t) / n for t in (t_cloud, t_dense, t_kernels))
            moved = 17 * P + 16 * kept / n                   # per image: both launches read the two planes, one reads the gray
            out["shapes"].append({"step": step, "images": n, "cols": cols, "rows": rows, "kept_fraction": kept / (n * P),
                                  "cloud_ms_per_image": c_ms, "cloud_call_ms_all": t_cloud,
                                  "search_ms_per_image": d_ms, "search_call_ms_all": t_dense,
                                  "kernels_ms_per_image": k_ms, "kernels_call_ms_all": t_kernels,
                                  "cloud_minus_search_ms_per_image": c_ms - d_ms,
                                  "kernels_bytes_per_image": moved, "kernels_bytes_per_s": moved / (k_ms * 1e-3),
                                  "kernels_fraction_of_8TBps": moved / (k_ms * 1e-3) / PEAK_BYTES_PER_S})
            if checked:
                out["shapes"][-1].update({"checked_cloud_ms_per_image": statistics.median(t_checked) / n, "checked_cloud_call_ms_all": t_checked,
                                          "checked_over_cloud": statistics.median(t_checked) / n / c_ms, "max_lr_diff": args.checked,
                                          "checked_kept_fraction": kept_checked / (n * P)})
            for k in sgm_legs:
                ms = statistics.median(t_sgm[k]) / n
                out["shapes"][-1].update({"sgm": args.sgm, f"{k}_ms_per_image": ms, f"{k}_call_ms_all": t_sgm[k], f"{k}_over_cloud": ms / c_ms,
                                          f"{k}_kept_fraction": sgm_kept[k] / (n * P)})
            if len(sgm_legs) == 2:
                out["shapes"][-1]["sgm_checked_over_sgm_cloud"] = statistics.median(t_sgm["sgm_checked_cloud"]) / statistics.median(t_sgm["sgm_cloud"])
            print(json.dumps(out["shapes"][-1]), file=sys.stderr, flush=True)      # (progress)
            del points, planes
    h.close()
    return out


def host_clouds(job, lefts, rig, poses, step, win):
    """the host path: a delivered host-mode disparity job with the cost plane, triangulated, filtered and compacted in
    numpy float32 as include/svo_hip.h ("clouds") states it"""
    F = np.float32
    v = job.values
    n, _, rows, cols = v.shape
    X = np.broadcast_to((np.arange(cols) * step + step // 2).astype(F)[None, :], (rows, cols))
    Y = np.broadcast_to((np.arange(rows) * step + step // 2).astype(F)[:, None], (rows, cols))
    b, fx, fy, cx, cy = (F(rig[k]) for k in RIG_KEYS)
    out = []
    for i in range(n):
        disp = v[i, 0]
        z = b / np.maximum(F(0.5), disp)
        x = (X - cx) / fx * z
        y = (Y - cy) / fy * z
        keep = (disp >= 0) & ~(disp < F(MIN_DISPARITY))
        R, t = poses[i]
        rec = np.empty(int(keep.sum()), hip_lib.MAP_POINT_DTYPE)
        x, y, z = x[keep], y[keep], z[keep]
        for k, name in enumerate(("x", "y", "z")):
            rec[name] = ((F(0) + R[k, 0] * x) + R[k, 1] * y) + R[k, 2] * z + t[k]
        rec["color"] = lefts[i][step // 2::step, step // 2::step][:rows, :cols][keep][:, None]
        rec["flags"] = 0
        out.append(rec)
    return out


def rotation(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def job_leg(args, device, cfg, lefts, rights):
    slots = max(args.images)
    n = min(slots, len(lefts))
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts[:n], rights[:n], bench.loop_plan(slots, n, lefts[0].shape[0]), True)(slam, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    win = cfg["window_size_depth_calculator"]
    rig = {k: cfg[k] for k in RIG_KEYS}
    out = {"slots": slots, "groups": slam.groups(), "shapes": []}
    for step in args.lattice_steps:
        for m in args.images:
            seqs = list(range(m))
            style = hip_lib.cloud_style(step, frame="world", layout="compact", min_disparity=MIN_DISPARITY)
            dstyle = hip_lib.disparity_style("disparity", step, cost=True)
            before = slam.memory().device_bytes
            jobs = {"cloud_device": Clouds(slam, hip_lib.EXPORT_FRAMES, seqs, style, True),
                    "cloud_host": Clouds(slam, hip_lib.EXPORT_FRAMES, seqs, style, False),
                    "disparity_device": Disparities(slam, hip_lib.EXPORT_FRAMES, seqs, dstyle, True),
                    "disparity_host": Disparities(slam, hip_lib.EXPORT_FRAMES, seqs, dstyle, False)}
            for j in jobs.values():
                j.submit().wait()                            # warm-up; the staging blocks exist afterwards
            views = slam.export_views("frames", seqs, plane="left", level=0, pixel="gray8")
            host_lefts = [np.ascontiguousarray(views.image(i)) for i in range(m)]
            poses = [(rotation(s["pose"][3:6]).astype(np.float32), s["pose"][:3].astype(np.float32)) for s in jobs["cloud_host"].segments]

            def host_path():
                jobs["disparity_host"].submit().wait()
                return host_clouds(jobs["disparity_host"], host_lefts, rig, poses, step, win)
            same = [int(len(a) == len(jobs["cloud_host"].points(i)) and
                        np.array_equal(a["color"], jobs["cloud_host"].points(i)["color"])) for i, a in enumerate(host_path())]
            t = {k: [] for k in ("cloud_device", "cloud_host", "disparity_device", "host_path")}
            for r in range(args.repeats):                   # the legs alternate
                for k in ("cloud_device", "cloud_host", "disparity_device"):
                    t[k].append(timed(device, lambda: jobs[k].submit().wait()) * 1e3)
                if r < args.host_repeats:
                    t["host_path"].append(timed(device, host_path) * 1e3)
            row = {"step": step, "slots_named": m, "points_per_slot": jobs["cloud_host"].points_per_slot,
                   "kept_fraction": float(jobs["cloud_host"].segments["n_points"].sum()) / (m * jobs["cloud_host"].points_per_slot),
                   "host_path_counts_and_grays_equal": bool(all(same)), "device_bytes_grown": slam.memory().device_bytes - before}
            for k, v in t.items():
                row[f"{k}_ms_per_image"] = statistics.median(v) / m
                row[f"{k}_ms_all"] = v
            row["cloud_device_minus_disparity_device_ms_per_image"] = row["cloud_device_ms_per_image"] - row["disparity_device_ms_per_image"]
            row["host_path_over_cloud_host"] = row["host_path_ms_per_image"] / row["cloud_host_ms_per_image"]
            out["shapes"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del jobs
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice-steps", type=lambda t: [int(x) for x in t.split(",")], default=[1, 2, 4])
    ap.add_argument("--images", type=lambda t: [int(x) for x in t.split(",")], default=[1, 16, 256])
    ap.add_argument("--loops", type=int, default=64)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--warmup", type=int, default=8, help="steps of the ctx before its jobs are timed")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1, help="timed runs of the host path (seconds each at step 1)")
    ap.add_argument("--no-job", action="store_true", help="the kernel leg only")
    ap.add_argument("--checked", type=float, default=None, metavar="D", help="also time svo_cloud_points_checked at the tolerance D")
    ap.add_argument("--sgm", type=lambda t: [int(x) for x in t.split(",")], default=None, metavar="P1,P2[,CAP]",
                    help="also time svo_cloud_points_sgm with these penalties (with --checked D: under the SGM map's own cross-check too)")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(min(max(args.images + [16]), args.loops))), args.loop_frames, device)
    out = {"metric": "cloud_bench", "config": "euroc", "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]),
           "kernel": kernel_leg(args, device, cfg, lefts, rights), "job": None if args.no_job else job_leg(args, device, cfg, lefts, rights)}
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
