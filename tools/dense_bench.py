"""What a dense disparity map costs on the MI355X: the kernel through its stage entry against the only
thing the library could do before it, and a disparity job queued behind every step of bench.py's workload.

One process, bench.py's rendered `euroc` stereo pairs (752 x 480), the EuRoC settings 31 / 60 / 6:

  kernel     svo_dense_disparity at steps 1, 2, 4 and 8 for 1, 16 and 256 image pairs in one call: the device time
             between two events around the call (the upload of one table entry per image, the launch, a stream
             synchronise), per image, and candidate-points per second (the sum of mw * mh over the lattice, over that
             time).
  baseline   svo_ssd_disparity with one keypoint per lattice point on the same images, one call per image (it takes one
             pair), on min(images, `--baseline-images`) images. At steps 1 and 2 only every `--baseline-rows`-th
             lattice row is run and the time scaled up by the rows left out: `baseline_rows_run` / `lattice_rows` in
             the JSON say so. The first image's rows are compared with the dense map, bit for bit.
             Every shape is warmed up first; the two legs alternate, median of `--repeats` each. `--no-baseline`
             leaves it out.
  checked    with `--checked D`: svo_dense_disparity_checked (the left-right cross-check of DESIGN §4.19 at the tolerance
             D, two planes) on the same pairs, a third leg alternating with the others. The unchecked figure of the
             parent commit comes from this tool run with SVO_HIP_LIB set to the parent's library, without --checked.
  sgm        with `--sgm P1,P2[,CAP]`: semi-global aggregation on the same pairs, three more legs
             alternating with the others: svo_dense_cost_volume (the cost-volume kernel), svo_sgm_aggregate on those
             volumes (the paths and the value rule; with the achieved bytes/s over 2 B of C and 4 B of S per entry and
             direction pair) and svo_dense_disparity_sgm (the whole stage entry). The baseline is dense_ms_per_image.
             Together with `--checked D` a fourth leg: svo_dense_disparity_sgm_checked (the SGM map's own cross-check,
             DESIGN §4.24, at the tolerance D), to be read against the unchecked whole (sgm_checked_over_sgm).
  job        frames/s over `--steps` queued steps of bench.py's workload without any job and with a device-mode
             step-4 disparity job of every slot queued behind every frame set; legs alternate, median of
             `--pipelined-repeats` each.
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting: 14 groups of 256)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import Disparities, StereoSlamBatch


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


def candidate_points(w, h, step, win, sx, sy):
    """the sum of mw * mh over the valid lattice points (the point rule of include/svo_hip.h)"""
    wb, wa = win // 2, (win + 1) // 2
    x = np.arange(w // step) * step + step // 2
    y = np.arange(h // step) * step + step // 2
    x11, x12, x22 = np.maximum(0, x - wb), np.minimum(w - 1, x + wa), np.minimum(w - 1, x + wa + sx)
    y11, y12 = np.maximum(0, y - wb), np.minimum(h, y + wa)
    y21, y22 = np.maximum(0, y - wb - sy), np.minimum(h - 1, y + wa + sy)
    tw, th = x12 - x11, y12 - y11
    mw, mh = (x22 - x11) - tw + 1, (y22 - y21) - th + 1
    okx = ~((x12 <= 0) | (x11 >= w - 1) | (x22 <= 0)) & (tw > 0) & (mw > 0)
    oky = ~((y12 <= 0) | (y11 >= h - 1) | (y22 <= 0) | (y21 >= h - 1)) & (th > 0) & (mh > 0)
    return int(np.where(okx, mw, 0).sum()) * int(np.where(oky, mh, 0).sum())


def kernel_leg(args, device, cfg, lefts, rights):
    W, H = cfg["width"], cfg["height"]
    win, sx, sy = cfg["window_size_depth_calculator"], cfg["search_x"], cfg["search_y"]
    h = hip_lib.Handle(device.index, 4096)
    lib = hip_lib.lib()
    nF = lefts[0].shape[0]
    pair = lambda i: (lefts[i % len(lefts)][(i // len(lefts)) * 7 % nF], rights[i % len(rights)][(i // len(lefts)) * 7 % nF])
    out = {"width": W, "height": H, "win": win, "search_x": sx, "search_y": sy, "shapes": []}
    for step in args.lattice_steps:
        cols, rows = W // step, H // step
        style = hip_lib.DisparityStyle(hip_lib.DENSE_DISPARITY, step, win, sx, sy, 0)
        every = args.baseline_rows if step <= 2 else 1
        run_rows = list(range(0, rows, every))
        xs = np.arange(cols) * step + step // 2
        kps = np.stack([np.tile(xs, len(run_rows)), np.repeat(np.asarray(run_rows) * step + step // 2, cols)], 1).astype(np.float32)
        d_kps = torch.from_numpy(kps).to(device)
        cand = candidate_points(W, H, step, win, sx, sy)
        for n in args.images:
            pairs = [pair(i) for i in range(n)]
            dst = torch.empty(n * cols * rows, dtype=torch.float32, device=device)
            packed = h.pack_dense([((l, W, H, l.stride(0)), (r, W, H, r.stride(0)), cfg["baseline"]) for l, r in pairs],
                                  [i * cols * rows * 4 for i in range(n)])
            dense = lambda: h.dense_disparity_packed(packed, style, dst)
            nb = min(n, args.baseline_images)
            imgs = [(hip_lib._img(l), hip_lib._img(r)) for l, r in pairs[:nb]]
            b_out = torch.empty(nb * len(kps), dtype=torch.float32, device=device)

            def baseline():
                for i, (a, b) in enumerate(imgs):
                    rc = lib.svo_ssd_disparity(h._h, C.byref(a), C.byref(b), C.c_void_p(d_kps.data_ptr()), len(kps), win, sx, sy, 1,
                                               C.c_void_p(b_out.data_ptr() + i * len(kps) * 4))
                    assert rc == 0
            if args.no_baseline:
                baseline = lambda: None
            checked = None
            if args.checked is not None:
                check = hip_lib.stereo_check(True, args.checked)
                dst_c = torch.empty(n * 2 * cols * rows, dtype=torch.float32, device=device)
                packed_c = h.pack_dense([((l, W, H, l.stride(0)), (r, W, H, r.stride(0)), cfg["baseline"]) for l, r in pairs],
                                        [i * 2 * cols * rows * 4 for i in range(n)])
                checked = lambda: h.dense_disparity_packed(packed_c, style, dst_c, check)
                checked()
            sgm = sgm_legs(args, h, device, cfg, pairs, style, cols, rows) if args.sgm else None
            dense(); baseline()                              # warm-up of the legs
            torch.cuda.synchronize(device)
            same = None if args.no_baseline else bool(torch.equal(dst[:cols * rows].view(rows, cols)[::every],
                                                                  b_out[:len(kps)].view(len(run_rows), cols)))
            t_dense, t_base, t_checked, t_sgm = [], [], [], {k: [] for k in (sgm or {})}
            for _ in range(args.repeats):                   # the legs alternate
                t_dense.append(event_ms(dense))
                t_base.append(event_ms(baseline))
                if checked:
                    t_checked.append(event_ms(checked))
                for k in t_sgm:
                    t_sgm[k].append(event_ms(sgm[k]))
            d_ms = statistics.median(t_dense) / n
            b_ms = statistics.median(t_base) / nb * (rows / len(run_rows))
            out["shapes"].append({"step": step, "images": n, "cols": cols, "rows": rows, "candidate_points_per_image": cand,
                                  "dense_ms_per_image": d_ms, "dense_call_ms_all": t_dense,
                                  "dense_candidate_points_per_s": cand / (d_ms * 1e-3),
                                  "baseline_ms_per_image": b_ms, "baseline_call_ms_all": t_base, "baseline_images": nb,
                                  "baseline_rows_run": len(run_rows), "lattice_rows": rows,
                                  "baseline_scaled_up": every > 1, "baseline_over_dense": b_ms / d_ms,
                                  "baseline_rows_equal_dense": same})
            if checked:
                c_ms = statistics.median(t_checked) / n
                lr = dst_c.view(n, 2, rows, cols)[:, 1]
                out["shapes"][-1].update({"checked_ms_per_image": c_ms, "checked_call_ms_all": t_checked, "checked_over_dense": c_ms / d_ms,
                                          "max_lr_diff": args.checked,
                                          "failing_fraction": float(((lr < 0) | (lr > args.checked)).float().mean().item())})
                del dst_c
            if sgm:
                entries = cols * rows * (sx + 1)
                ms = {k: statistics.median(v) / n for k, v in t_sgm.items()}
                out["shapes"][-1].update({"sgm": args.sgm, "candidates": sx + 1, "volume_entries_per_image": entries,
                                          "cost_volume_ms_per_image": ms["cost_volume"], "paths_ms_per_image": ms["paths"],
                                          "sgm_ms_per_image": ms["whole"], "sgm_call_ms_all": t_sgm,
                                          "paths_bytes_per_s": 2 * 6 * entries / (ms["paths"] * 1e-3),
                                          "cost_volume_over_dense": ms["cost_volume"] / d_ms, "sgm_over_dense": ms["whole"] / d_ms})
                if "checked" in ms:
                    lr = sgm["checked"].dst.view(n, 2, rows, cols)[:, 1]
                    out["shapes"][-1].update({"sgm_checked_ms_per_image": ms["checked"], "sgm_checked_over_sgm": ms["checked"] / ms["whole"],
                                              "sgm_checked_over_dense": ms["checked"] / d_ms, "max_lr_diff": args.checked,
                                              "sgm_failing_fraction": float(((lr < 0) | (lr > args.checked)).float().mean().item())})
                del sgm
            print(json.dumps(out["shapes"][-1]), file=sys.stderr, flush=True)      # (progress)
    h.close()
    return out


def sgm_legs(args, h, device, cfg, pairs, style, cols, rows):
    """the three SGM legs over `pairs` with their arguments built once: {name: callable}. The volumes of all pairs live
    in one tensor (volume | count plane per pair)"""
    W, H, lib, n = cfg["width"], cfg["height"], hip_lib.lib(), len(pairs)
    D = style.search_x + 1
    cap = args.sgm[2] if len(args.sgm) > 2 else hip_lib.SGM_DEFAULTS["cost_cap"]
    sp = hip_lib.sgm_params(args.sgm[0], args.sgm[1], cap)
    per = cols * rows * (D + 1)                            # uint16 words of a pair
    vols = torch.empty(n * per, dtype=torch.int16, device=device)
    dst = torch.empty(n * cols * rows, dtype=torch.float32, device=device)
    packed = h.pack_dense([((l, W, H, l.stride(0)), (r, W, H, r.stride(0)), cfg["baseline"]) for l, r in pairs],
                          [i * cols * rows * 4 for i in range(n)])
    vo = (C.c_int64 * n)(*[i * per * 2 for i in range(n)])
    co = (C.c_int64 * n)(*[(i * per + cols * rows * D) * 2 for i in range(n)])
    shapes = (hip_lib.SgmShape * n)(*[hip_lib.SgmShape(cols, rows, D, cfg["baseline"]) for _ in range(n)])
    vp = (C.c_void_p * n)(*[vols.data_ptr() + vo[i] for i in range(n)])
    cp = (C.c_void_p * n)(*[vols.data_ptr() + co[i] for i in range(n)])

    def cost_volume():
        assert lib.svo_dense_cost_volume(h._h, n, packed[1], C.byref(style), cap, vo, co, C.c_void_p(vols.data_ptr())) == 0

    def paths():
        assert lib.svo_sgm_aggregate(h._h, n, shapes, vp, cp, 0, 0, C.byref(sp), packed[2], C.c_void_p(dst.data_ptr())) == 0

    def whole():
        assert lib.svo_dense_disparity_sgm(h._h, n, packed[1], packed[2], C.byref(style), C.byref(sp), C.c_void_p(dst.data_ptr())) == 0
    legs = {"cost_volume": cost_volume, "paths": paths, "whole": whole}
    legs["cost_volume"](); legs["paths"]()
    mine = dst.clone()
    legs["whole"]()                                        # (and the warm-up: the two-step result is the whole's)
    assert torch.equal(mine, dst)
    if args.checked is not None:                           # value and lr planes per pair
        check = hip_lib.stereo_check(True, args.checked)
        dst_c = torch.empty(n * 2 * cols * rows, dtype=torch.float32, device=device)
        packed_c = h.pack_dense([((l, W, H, l.stride(0)), (r, W, H, r.stride(0)), cfg["baseline"]) for l, r in pairs],
                                [i * 2 * cols * rows * 4 for i in range(n)])

        def checked():
            h.dense_disparity_sgm_packed(packed_c, style, sp, dst_c, check)
        checked.dst = dst_c
        checked()
        kept = dst_c.view(n, 2, rows, cols)[:, 0] >= 0     # a point that does not fail has the unchecked map's bits
        assert torch.equal(dst_c.view(n, 2, rows, cols)[:, 0][kept], dst.view(n, rows, cols)[kept])
        legs["checked"] = checked
    return legs                                            # (the closures keep the tensors and arrays alive)


def start(cfg, lefts, rights, slots, groups, device, steps):
    if groups:
        os.environ["SVO_GROUPS"] = str(groups)
    else:
        os.environ.pop("SVO_GROUPS", None)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, len(lefts), lefts[0].shape[0]), True)(slam, steps)
    return slam, packed


def job_leg(args, device, cfg, lefts, rights, slots, groups):
    K, Wm = args.steps, args.warmup
    n = min(slots, len(lefts))
    runs_n = 2 * args.pipelined_repeats
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, groups, device, Wm + runs_n * K)
    for pk in packed[:Wm]:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "groups": slam.groups(), "steps": K, "disparity_step": args.job_step}
    style = hip_lib.disparity_style("disparity", args.job_step)
    ring = [Disparities(slam, hip_lib.EXPORT_FRAMES, None, style, True).submit().wait() for _ in range(2)]
    out["job_ms_alone"] = statistics.median([timed(device, lambda: ring[0].submit().wait()) * 1e3 for _ in range(5)])
    runs = {"plain": [], "disparity": []}
    for r in range(runs_n):
        kind = ("plain", "disparity")[r % 2]
        steps = packed[Wm + r * K:Wm + (r + 1) * K]

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if kind == "disparity":
                    ring[k % 2].submit()
            slam.wait()
        runs[kind].append(slots * K / timed(device, run))
    for kind in runs:
        out[f"frames_per_s_{kind}"] = statistics.median(runs[kind])
        out[f"frames_per_s_{kind}_all"] = runs[kind]
    out["disparity_vs_plain"] = out["frames_per_s_disparity"] / out["frames_per_s_plain"]
    out["bytes_per_job"] = ring[0].capacity
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice-steps", type=lambda t: [int(x) for x in t.split(",")], default=[1, 2, 4, 8])
    ap.add_argument("--images", type=lambda t: [int(x) for x in t.split(",")], default=[1, 16, 256])
    ap.add_argument("--baseline-images", type=int, default=4, help="images the per-keypoint baseline runs on at most")
    ap.add_argument("--baseline-rows", type=int, default=8, help="at steps 1 and 2 the baseline runs every n-th lattice row, scaled up")
    ap.add_argument("--no-baseline", action="store_true", help="leave the per-keypoint baseline out (its fields are then of no use)")
    ap.add_argument("--checked", type=float, default=None, metavar="D", help="also time svo_dense_disparity_checked at the tolerance D")
    ap.add_argument("--sgm", type=lambda t: [int(x) for x in t.split(",")], default=None, metavar="P1,P2[,CAP]",
                    help="also time the cost-volume kernel, the paths and svo_dense_disparity_sgm with these penalties")
    ap.add_argument("--legs", default="256:1,1024:3", help="slots:groups per job leg (groups 0: the ctx's default); '' for none")
    ap.add_argument("--job-step", type=int, default=4)
    ap.add_argument("--loops", type=int, default=64)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run")
    ap.add_argument("--warmup", type=int, default=8, help="steps before anything is timed")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pipelined-repeats", type=int, default=3, help="timed runs per kind of a job leg")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",") if l]
    n_loops = min(max([s for s, _ in legs] + [16]), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    out = {"metric": "dense_bench", "config": "euroc", "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]),
           "kernel": kernel_leg(args, device, cfg, lefts, rights), "job": []}
    for slots, groups in legs:
        out["job"].append(job_leg(args, device, cfg, lefts, rights, slots, groups))
        print(json.dumps(out["job"][-1]), file=sys.stderr, flush=True)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
