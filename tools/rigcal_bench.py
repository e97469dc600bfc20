"""Cost of adding camera rigs to a ctx at 752 x 480, three ways, on the MI355X.

  python tools/rigcal_bench.py [--counts 1 16 256] [--out profiles/rigcal_bench.json]

For n rigs (2n cameras: the EuRoC pair, every unit's focal lengths and centre moved a little):
  host         what a caller had to do before calibrations: the float maps in numpy (replay.undistort_rectify_map,
               4 planes per rig), then svo_ctx_add_rigs with host maps (upload, remap_prep_kernel, per rig)
  device       the float maps made on the GPU by svo_build_rectify_maps (one launch), then svo_ctx_add_rigs with
               device maps (remap_prep_kernel, a stream and a synchronise per rig)
  calibrated   svo_ctx_add_rigs_calibrated: one table upload, one fused launch, one synchronise
Every way runs on a fresh one-slot ctx; wall-clock milliseconds of each part, and what the device's free memory and
svo_ctx_get_memory say before and after the call. The kernel's own time: device events around the stage entry's
launch (the fused form does the same arithmetic and writes 6 instead of 8 bytes per pixel); per kernel:
`rocprofv3 --kernel-trace --stats -- python tools/rigcal_bench.py --counts 256`.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import rigcal_ref
from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

W, H = 752, 480


def unit(k):
    """(left, right) calibrations of unit k in the library's naming (left <- RIGHT.*), as (K, D, R, P) tuples"""
    cams, _ = rigcal_ref.euroc()
    out = []
    for side in ("RIGHT", "LEFT"):
        K, D, R, P = cams[side]
        K = K.copy()
        K[0, 0] += 0.01 * (k % 97); K[1, 1] -= 0.01 * (k % 89); K[0, 2] += 0.02 * (k % 53); K[1, 2] -= 0.02 * (k % 59)
        out.append((K, D, R, P))
    return out


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def run(way, n, cfg):
    rig = {f: cfg[f] for f in hip_lib.RIG_FLOATS}
    units = [unit(k) for k in range(n)]
    slam = StereoSlamBatch(cfg, W, H, 1)
    out = {"way": way, "rigs": n}
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    if way == "host":
        t0 = time.perf_counter()
        maps = [[replay.undistort_rectify_map(K, D[:5], R, P, (W, H)) for K, D, R, P in u] for u in units]
        out["maps_ms"] = ms(t0)
        rigs = [dict(rig, left_maps=m[0], right_maps=m[1]) for m in maps]
    elif way == "device":
        cals = [hip_lib.CameraCalibration.from_mats(*c) for u in units for c in u]
        t0 = time.perf_counter()
        maps = StereoSlamBatch.build_rectify_maps(cals, W, H)
        out["maps_ms"] = ms(t0)
        rigs = [dict(rig, left_maps=maps[2 * k], right_maps=maps[2 * k + 1]) for k in range(n)]
    else:
        rigs = [dict(rig, left_calibration=hip_lib.CameraCalibration.from_mats(*u[0]),
                     right_calibration=hip_lib.CameraCalibration.from_mats(*u[1])) for u in units]
    free0, ctx0 = torch.cuda.mem_get_info()[0], slam.memory().device_bytes
    t0 = time.perf_counter()
    slam.add_rigs(rigs)
    out["add_ms"] = ms(t0)
    out["total_ms"] = ms(t_all)
    out["device_free_drop_bytes"] = free0 - torch.cuda.mem_get_info()[0]
    out["ctx_device_bytes_added"] = slam.memory().device_bytes - ctx0
    out["map_bytes"] = slam.rigs()[1]
    slam.close()
    return out


def kernel_ms(n, reps=10):
    """device events around svo_build_rectify_maps of 2n cameras (one launch)"""
    h = hip_lib.Handle(0, 16)
    cals = [hip_lib.CameraCalibration.from_mats(*c) for k in range(n) for c in unit(k)]
    planes = h.build_rectify_maps(cals, W, H)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        h.build_rectify_maps(cals, W, H, out=planes)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    h.close()
    return {"cameras": 2 * n, "launch_ms_median": float(np.median(times)), "launch_ms_min": float(np.min(times)),
            "pixels_per_s": 2 * n * W * H / (float(np.median(times)) * 1e-3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigcal_bench.json"))
    args = ap.parse_args()
    cfg = dict(synth.CONFIGS["euroc"])
    run("calibrated", 1, cfg)                             # (untimed: the first launch of every kernel loads its code)
    run("host", 1, cfg)
    res = {"size": [W, H], "baseline": "host: the parent commit's only way from a calibration to a rig",
           "adds": [run(way, n, cfg) for n in args.counts for way in ("host", "device", "calibrated")],
           "stage_kernel": [kernel_ms(n) for n in args.counts]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
