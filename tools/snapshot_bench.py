"""What saving and loading sequence state costs on the MI355X.

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), 256
slots in one group, after a warm-up of at least 60 steps so that several keyframes are live. In one process:

  save_device / load_device   every slot into / out of device memory: host clock around submit + wait + device
                              synchronise, median of `--repeats`, alternating with
  memcpy                      one plain device-to-device copy (torch's copy_: hipMemcpyAsync) of the same byte count,
                              timed the same way and with device events. (The ctx's own stream cannot be reached
                              from Python: the copy runs on the process's current stream while the ctx is idle.)
  save_host / load_host       the same through pinned host memory, with bytes/s against the host link.
  pipelined                   frames/s over `--steps` queued steps without and with a device-mode save of 8 slots
                              queued behind every frame set, legs alternating, median of three each.
`--profile` runs warm-up, three saves and three loads and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernel's own time.
Prints one JSON line and, with --out, writes it to that file.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting)
os.environ["SVO_GROUPS"] = "1"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
from stereo_svo_slam_amd.stereo_slam import Snapshot, StereoSlamBatch

HOST_LINK_GBS = 63.0                # the host link's specification, one direction
HBM_GBS = 8000.0                    # HBM3E peak of the MI355X; a copy moves every byte twice


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run (six runs)")
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.warmup >= 60
    device = torch.device("cuda", 0)
    slots, K, W = args.slots, args.steps, args.warmup
    n_loops = min(slots, args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, n_loops, lefts[0].shape[0]), True)(slam, W + 6 * K)
    for pk in packed[:W]:
        slam.submit_packed(pk)
    slam.wait()
    sizes = [slam.snapshot_size(s) for s in range(slots)]
    data_bytes = sum(d for _, d in sizes)
    out = {"metric": "snapshot_bench", "config": "euroc", "slots": slots, "groups": slam.groups(), "warmup": W,
           "host_bytes": sum(h for h, _ in sizes), "data_bytes": data_bytes, "host_link_spec_GBs": HOST_LINK_GBS}
    all_slots = list(range(slots))

    dev_snaps = [slam.new_snapshot(h, d, device=True) for h, d in sizes]
    save_dev = lambda: (slam.submit_save(all_slots, snapshots=dev_snaps), slam.wait())
    load_dev = lambda: slam.load(all_slots, dev_snaps)
    if args.profile:
        for _ in range(3):
            save_dev()
        for _ in range(3):
            load_dev()
        slam.close()
        return
    a = torch.empty(data_bytes, dtype=torch.uint8, device=device)
    b = torch.empty(data_bytes, dtype=torch.uint8, device=device)

    def memcpy_events():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3

    save_dev()                                                     # (first calls: not timed)
    infos = [s.info for s in dev_snaps]
    out["keyframes_per_slot"] = statistics.mean(i.n_keyframes for i in infos)
    out["image_sets_per_slot"] = statistics.mean(i.n_image_sets for i in infos)
    out["planes"] = sum(i.n_planes for i in infos)
    timed(device, lambda: b.copy_(a))
    t = {"save_device": [], "memcpy": [], "memcpy_events": [], "load_device": [], "memcpy_b": []}
    for _ in range(args.repeats):
        t["save_device"].append(timed(device, save_dev))
        t["memcpy"].append(timed(device, lambda: b.copy_(a)))
        t["memcpy_events"].append(memcpy_events())
    for _ in range(args.repeats):
        t["load_device"].append(timed(device, load_dev))
        t["memcpy_b"].append(timed(device, lambda: b.copy_(a)))
    t["memcpy"] += t.pop("memcpy_b")
    del a, b
    for name, v in t.items():
        sec = statistics.median(v)
        out[name] = {"seconds": sec, "seconds_all": v, "bytes_per_s": data_bytes / sec,
                     "fraction_of_hbm_copy_roof": 2 * data_bytes / sec / (HBM_GBS * 1e9)}
    for name in ("save_device", "load_device"):
        out[name]["vs_memcpy"] = out[name]["seconds"] / out["memcpy"]["seconds"]
        out[name]["target_2x_met"] = out[name]["vs_memcpy"] <= 2.0

    # host mode, pinned buffers
    pin = lambda n: torch.zeros(max(n, 1), dtype=torch.uint8, pin_memory=True).numpy()[:n]
    host_snaps = [Snapshot(np.zeros(h, np.uint8), pin(d)) for h, d in sizes]
    save_host = lambda: (slam.submit_save(all_slots, snapshots=host_snaps), slam.wait())
    load_host = lambda: slam.load(all_slots, host_snaps)
    first = timed(device, save_host)
    for name, fn in (("save_host", save_host), ("load_host", load_host)):
        v = [timed(device, fn) for _ in range(args.repeats)]
        sec = statistics.median(v)
        out[name] = {"seconds": sec, "seconds_all": v, "bytes_per_s": data_bytes / sec,
                     "fraction_of_host_link": data_bytes / sec / (HOST_LINK_GBS * 1e9)}
    out["save_host"]["first_call_seconds"] = first
    out["host_equals_device"] = all(h.data.tobytes() == d.data.cpu().numpy().tobytes() and h.host.tobytes() == d.host.tobytes()
                                    for h, d in list(zip(host_snaps, dev_snaps))[:8])
    del host_snaps

    # a save of 8 slots behind every step of the pipelined loop (two buffer sets in turn, room for growth)
    some = all_slots[:8]
    ring = [[slam.new_snapshot(2 * h, 2 * d, device=True) for h, d in sizes[:8]] for _ in range(2)]
    runs = {"plain": [], "with_save": []}
    for r in range(6):
        steps = packed[W + r * K:W + (r + 1) * K]
        with_save = r % 2 == 1

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if with_save:
                    slam.submit_save(some, snapshots=ring[k % 2])
            slam.wait()
        runs["with_save" if with_save else "plain"].append(slots * K / timed(device, run))
    plain, saved = statistics.median(runs["plain"]), statistics.median(runs["with_save"])
    complete = all(s.info.status == 0 for s in ring[(K - 1) % 2])
    out["pipelined"] = {"steps": K, "saved_slots": len(some), "frames_per_s": plain, "frames_per_s_all": runs["plain"],
                        "frames_per_s_with_save": saved, "frames_per_s_with_save_all": runs["with_save"],
                        "with_save_vs_plain": saved / plain, "saves_complete": complete,
                        "save_bytes_per_step": sum(s.info.data_bytes for s in ring[(K - 1) % 2])}
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
