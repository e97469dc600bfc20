"""What the app's IMU loop costs on the MI355X: one svo_update_pose per sample and slot against one batched
svo_update_poses / svo_submit_pose_updates per frame interval.

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), once
with 256 slots in one group and once with 3584 slots in the ctx's default groups, in one process. Per leg, after a
warm-up, with 1, 3 and 8 gyro samples per slot (SlamApp::update_pose_from_imu: the app's variances, dt = 1 / 104,
every sample measuring the previous filtered pose):

  loop       wall time of the per-slot loop: one svo_update_pose per sample (each waits for every queue of the ctx
             and runs the host filter on the calling thread), the argument arrays built beforehand.
  batched    one svo_update_poses of all slots: the first call (it allocates the groups' blocks) and the median of
             `--repeats` more.
  pipelined  frames/s over `--steps` queued steps in three forms, legs alternating, median of three each: without
             IMU, with one svo_submit_pose_updates in front of every frame set, with the per-slot loop in front of
             every frame set.
Prints one JSON line and writes it to --out. Times are host clocks around work that ends in svo_wait and a device
synchronise.
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
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
from stereo_svo_slam_amd.hip_lib import POSE_SAMPLE_DTYPE, _check, lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch

SAMPLES = (1, 3, 8)


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


class Imu:
    """the samples of one frame interval for every slot, as both calls take them"""

    def __init__(self, slam, per_slot, seed):
        rng = np.random.default_rng(seed)
        self.slam, self.per_slot, n = slam, per_slot, slam.n
        gyro = rng.normal(0, 2.0, (n * per_slot, 3)).astype(np.float32)
        self.samples = np.concatenate([StereoSlamBatch.gyro_samples(gyro[s * per_slot:(s + 1) * per_slot], 1.0) for s in range(n)])
        assert self.samples.dtype == POSE_SAMPLE_DTYPE and len(self.samples) == n * per_slot
        self.counts = (C.c_int * n)(*([per_slot] * n))
        self.filtered = np.zeros((n * per_slot, 6), np.float32)
        # the loop's arguments: per slot one pose buffer that is measurement and result (the chain), per sample its speed
        self.pose = np.zeros((n, 6), np.float32)
        self.pv = np.ascontiguousarray(self.samples["pose_var"][0])
        self.sv = np.ascontiguousarray(self.samples["speed_var"][0])
        self.speed = np.ascontiguousarray(self.samples["speed"])
        self.dt = C.c_double(1.0 / 104.0)

    def batched(self, wait=True):
        fn = lib().svo_update_poses if wait else lib().svo_submit_pose_updates
        _check(fn(self.slam._ctx, None, self.counts, self.slam.n, self.samples.ctypes.data, self.filtered.ctypes.data))

    def loop(self):
        f, ctx, n, m = lib().svo_update_pose, self.slam._ctx, self.slam.n, self.per_slot
        vp = C.c_void_p
        pv, sv, dt = vp(self.pv.ctypes.data), vp(self.sv.ctypes.data), self.dt
        for s in range(n):
            _check(lib().svo_get_pose(ctx, s, vp(self.pose[s].ctypes.data)))
            pose = vp(self.pose[s].ctypes.data)
            for k in range(m):
                _check(f(ctx, s, pose, vp(self.speed[s * m + k].ctypes.data), pv, sv, dt, pose))


def leg(args, device, cfg, lefts, rights, slots, groups):
    if groups:
        os.environ["SVO_GROUPS"] = str(groups)
    else:
        os.environ.pop("SVO_GROUPS", None)
    n_loops, nF = len(lefts), lefts[0].shape[0]
    K, W = args.steps, args.warmup
    packer = bench.step_packer(lefts, rights, bench.loop_plan(slots, n_loops, nF), True)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = packer(slam, W + 9 * K * len(SAMPLES))
    for pk in packed[:W]:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "groups": slam.groups(), "samples": {}}
    m0 = slam.memory().device_bytes
    at = W
    for per_slot in SAMPLES:
        imu = Imu(slam, per_slot, per_slot)
        res = {}
        first = timed(device, imu.batched)
        loops = [timed(device, imu.loop) for _ in range(args.loop_repeats)]
        reps = [timed(device, imu.batched) for _ in range(args.repeats)]
        sec_loop, sec = statistics.median(loops), statistics.median(reps)
        res["loop"] = {"seconds": sec_loop, "seconds_all": loops, "seconds_per_call": sec_loop / (slots * per_slot)}
        res["batched"] = {"first_call_seconds": first, "seconds": sec, "seconds_all": reps,
                          "seconds_per_sample": sec / (slots * per_slot), "speedup_over_loop": sec_loop / sec}
        # the pipelined loop: plain, one submit per step, the per-slot loop per step
        runs = {"plain": [], "batched": [], "loop": []}
        for r in range(9):
            form = ("plain", "batched", "loop")[r % 3]
            steps = packed[at:at + K]
            at += K

            def run():
                for pk in steps:
                    if form == "batched":
                        imu.batched(wait=False)
                    elif form == "loop":
                        imu.loop()
                    slam.submit_packed(pk)
                slam.wait()
            runs[form].append(slots * K / timed(device, run))
        med = {k: statistics.median(v) for k, v in runs.items()}
        res["pipelined"] = {"steps": K, "frames_per_s": med["plain"], "frames_per_s_all": runs["plain"],
                            "frames_per_s_with_batched": med["batched"], "frames_per_s_with_batched_all": runs["batched"],
                            "frames_per_s_with_loop": med["loop"], "frames_per_s_with_loop_all": runs["loop"],
                            "seconds_per_step": slots / med["plain"], "seconds_per_step_with_batched": slots / med["batched"],
                            "seconds_per_step_with_loop": slots / med["loop"],
                            "batched_cost_per_step_seconds": slots / med["batched"] - slots / med["plain"]}
        out["samples"][str(per_slot)] = res
        print(json.dumps({"slots": slots, "per_slot": per_slot, **res}), file=sys.stderr, flush=True)   # (progress)
    out["pose_blocks_device_bytes"] = slam.memory().device_bytes - m0
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="256:1,3584:0", help="slots:groups per leg (groups 0: the ctx's default)")
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=12, help="steps of one timed pipelined run (nine runs per sample count)")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5, help="timed batched calls per sample count")
    ap.add_argument("--loop-repeats", type=int, default=3, help="timed per-slot loops per sample count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_bench.json"))
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",")]
    n_loops = min(max(s for s, _ in legs), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    out = {"metric": "imu_bench", "config": "euroc", "samples_per_slot": list(SAMPLES),
           "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "legs": []}
    for slots, groups in legs:
        n = min(slots, n_loops)
        out["legs"].append(leg(args, device, cfg, lefts[:n], rights[:n], slots, groups))
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
