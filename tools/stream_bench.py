"""What sequences that start and end inside a running ctx cost on the MI355X.

bench.py's workload (C2 `euroc`, 3584 slots in the ctx's default groups, borrowed device frames from bench.py's
rendered loops, pipelined submits) on ONE ctx, three legs in one process; the slots are restarted between the legs.
Every leg is warmed up and timed between device synchronisations; frames/s = sequence-frames / wall time.

  steady    no restarts: every slot has a frame at every step (the bench.py workload; a cross-check).
  streaming every slot plays sequences of 60..240 frames (seeded) back to back (multi_seq.pack_queue in the given
            order, pipelined). Timed over the steps at which every slot is busy, after the first restarts;
            reported against `steady` with the mean starts per step.
  finite    `--finite` x slots sequences of 60..240 frames, once as consecutive play_unequal-style passes of one
            sequence per slot (every slot restarted between passes) and once as one longest-first queue, with
            the step counts of the two schedules beside the wall times.
Prints one JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting: 14 groups of 256)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

import bench
from stereo_svo_slam_amd import multi_seq
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch


def timed(device, fn):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=3584)
    ap.add_argument("--loops", type=int, default=128)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=200, help="timed steps of the steady leg, at most as many of the streaming leg")
    ap.add_argument("--warmup", type=int, default=40, help="untimed steps of the steady leg")
    ap.add_argument("--finite", type=int, default=3, help="sequences per slot of the finite job")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--legs", default="steady,streaming,finite")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    B, n_loops, nF = args.slots, min(args.slots, args.loops), args.loop_frames
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), nF, device)
    lv = [list(x.unbind(0)) for x in lefts]
    rv = [list(x.unbind(0)) for x in rights]
    # sequence i: loop i % n_loops entered at a frame of its own, always forward (a closed path)
    frames_of = lambda s, k: (lv[s % n_loops][(37 * s + k) % nF], rv[s % n_loops][(37 * s + k) % nF])
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], B, 0)
    all_slots = list(range(B))
    out = {"metric": "stream_bench", "config": "euroc", "slots": B, "groups": slam.groups(), "lengths": "60..240 (seeded)"}

    def reset():
        slam.restart(all_slots)
        slam.drop_finished_runs()
        print(json.dumps(out), file=sys.stderr, flush=True)   # (progress)

    legs = args.legs.split(",")
    if "steady" in legs:
        packed = bench.step_packer(lefts, rights, bench.loop_plan(B, n_loops, nF), True)(slam, args.warmup + args.steps)
        for pk in packed[:args.warmup]:
            slam.submit_packed(pk)
        slam.wait()

        def run():
            for pk in packed[args.warmup:]:
                slam.submit_packed(pk)
            slam.wait()
        sec = timed(device, run)
        out["steady"] = {"steps": args.steps, "frames": B * args.steps, "seconds": sec, "frames_per_s": B * args.steps / sec}
        del packed
        reset()

    if "streaming" in legs:
        rng = random.Random(args.seed)
        lengths = [rng.randint(60, 240) for _ in range(3 * B)]
        steps, _, _ = multi_seq.pack_queue(slam, frames_of, lengths, order=range(len(lengths)), borrow=True)
        sched = multi_seq.queue_schedule(lengths, B, range(len(lengths)))
        first = 60                                        # the first restarts fall on step 60 at the earliest
        full = [len(st) == B for st in sched]
        last = first
        while last < len(sched) and full[last] and last - first < args.steps:
            last += 1
        multi_seq.submit_queue(slam, steps[:first])
        slam.wait()
        sec = timed(device, lambda: (multi_seq.submit_queue(slam, steps[first:last]), slam.wait()))
        frames = sum(len(st) for st in sched[first:last])
        starts = sum(len(r) for r, _ in steps[first:last])
        out["streaming"] = {"steps": last - first, "frames": frames, "seconds": sec, "frames_per_s": frames / sec,
                            "starts": starts, "starts_per_step": starts / max(last - first, 1)}
        if "steady" in out:
            out["streaming"]["vs_steady"] = out["streaming"]["frames_per_s"] / out["steady"]["frames_per_s"]
        del steps
        reset()

    if "finite" in legs:
        rng = random.Random(args.seed + 1)
        lengths = [rng.randint(60, 240) for _ in range(args.finite * B)]
        total = sum(lengths)
        # (a) passes of one sequence per slot in the given order, every slot restarted between passes
        passes = []
        for p in range(args.finite):
            ids = range(p * B, (p + 1) * B)               # (sequence ids stay global: frames_of goes by them)
            only = [n if i in ids else 0 for i, n in enumerate(lengths)]
            passes.append(multi_seq.pack_queue(slam, frames_of, only, order=ids, borrow=True)[0])

        def run_passes():
            for ps in passes:
                multi_seq.submit_queue(slam, ps)
                slam.restart(all_slots)
            slam.wait()
        sec_p = timed(device, run_passes)
        steps_p = sum(len(ps) for ps in passes)
        del passes
        slam.drop_finished_runs()
        # (b) one queue, longest first
        steps, _, frames = multi_seq.pack_queue(slam, frames_of, lengths, borrow=True)
        assert frames == total
        sec_q = timed(device, lambda: (multi_seq.submit_queue(slam, steps), slam.wait()))
        out["finite"] = {"sequences": len(lengths), "frames": total,
                         "passes": {"steps": steps_p, "seconds": sec_p, "frames_per_s": total / sec_p},
                         "queue": {"steps": len(steps), "seconds": sec_q, "frames_per_s": total / sec_q},
                         "lower_bound_steps": -(-total // B),
                         "step_ratio": len(steps) / steps_p, "time_ratio": sec_q / sec_p}
        reset()
    m = slam.memory()
    out["memory"] = {"device_GB": m.device_bytes / 1e9, "klt_cache_GB": m.klt_cache_bytes / 1e9,
                     "image_sets": m.image_sets, "image_sets_free": m.image_sets_free,
                     "keyframe_slabs": m.keyframe_slabs, "keyframe_slabs_free": m.keyframe_slabs_free}
    slam.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
