"""What fusing dense clouds into voxel maps costs on the MI355X. Writes profiles/voxel_bench.json.

  fuse       svo_voxel_fuse on organized world-frame clouds of bench.py's workload (C2 `euroc`, `--slots` slots after a
             warm-up, lattice step `--step`): fused records/s of the two forms of the kernel (one summed set of
             atomics per distinct key of a wavefront; every lane its own atomics: SVO_VOXEL_LANE_ATOMICS=1), with all
             spans into ONE map and with one map per slot (`--slots` maps per launch). Device events around a call:
             the header gather and its copy, the table uploads, the kernel and a stream synchronise. Every repeat
             starts from cleared maps.
  pile       one slot's record count on one voxel, both forms.
  extract    svo_voxel_extract of one map by occupancy (the map filled to 1/16, 1/4 and 3/4 of its entries with
             distinct voxels): count, scan, pairs, sort, gather and the two small copies.
  host path  what the job replaces: the organized clouds downloaded (a host-mode cloud job) and fused on the host
             with numpy (the vectorised statement of tests/voxel_ref.py).
  pipelined  frames/s over `--steps` queued steps of bench.py's workload without fusion and with a fuse job of every
             slot's newest keyframe queued behind every frame set; legs alternate, median of `--repeats` each.
Prints one JSON line.

  --sgm P1,P2[,CAP]  instead of all that (sets the key "fuse" of profiles/sgm_consumers_bench.json): the fuse
             job of `--slots` slots' newest keyframes at lattice step `--step` through svo_submit_fuse_clouds and through
             svo_submit_fuse_clouds_sgm, unchecked and checked at tolerance `--lr`, beside the cloud jobs alone; the legs
             alternate in one process, median of `--repeats` each.
  --prune    instead of all that (writes profiles/voxel_prune_bench.json): svo_voxel_prune of a map of
             1 << 16, 20 and 24 entries at 0.25, 0.5 and 0.75 load (distinct voxels, half of them fused with stamp 1 and
             half with stamp 2), keeping all (min_stamp 1: the early out) and keeping the newer half (min_stamp 2; the
             map is restored from a copy ahead of every repeat, untimed), beside what the library could do with the
             same map before: a count pass (svo_voxel_extract with points == NULL), svo_voxel_extract of the kept half,
             and the host path a prune replaces: that half extracted and downloaded, svo_voxel_clear, the records
             uploaded and fused again (wall clock; it loses the counts and stamps, which a prune keeps).
  --carve    instead of all that (writes profiles/voxel_carve_bench.json): svo_voxel_carve of a map of
             1 << 20 and 1 << 24 entries at 0.75 load (distinct voxels on a slab that a 752 x 480 camera sees whole) under
             occluder lattices of step 1 and 4: a carve that removes nothing (the occluder stands in front of every
             entry), a carve that removes about half (the right half of the lattice stands behind every entry), and
             beside them svo_voxel_prune of the same map keeping all and keeping half (by stamp), and svo_voxel_extract
             of the whole map, and the two carves again in the other form of the kernels (SVO_VOXEL_CARVE_REEVALUATE=1: no ballot
             words, the stage pass evaluates the rule again). The prune legs are this library's: its plain prune kernels have the
             parent's registers, LDS and occupancy (profiles/voxel_carve_registers.txt). The map is restored from a copy ahead of every timed call, untimed; the legs alternate in
             one process, median of `--repeats` each.
  --entries  instead of all that (writes profiles/voxel_entries_bench.json): a map of 1 << 24 entries at 0.75 and at
             0.25 load (distinct voxels, fused with two stamps). svo_voxel_pack beside svo_voxel_extract of the same map (the same
             passes; 40 B leave per entry, not 16). svo_voxel_merge of the packed span into an empty map (of 1 << 25 entries, so
             that the load bound admits the next leg too) and into one that holds half of its keys, beside svo_voxel_fuse of as many records in both forms of its kernel into the same two
             maps; and the same records as `--entries-slots` spans into as many maps of a quarter of the size in one launch
             (one map per slot). svo_voxel_rehash to log2 + 1 beside svo_voxel_prune keeping everything. And, wall clock, a
             ctx's svo_ctx_resize_voxel_maps to log2 + 1 beside the host path it replaces: the map exported to the host, a
             larger map set, the means uploaded and fused (svo_voxel_fuse into a map of the caller's: a ctx takes records
             only from its own clouds), which loses the counts, sums and stamps that the resize keeps. Targets are
             restored ahead of every timed call, untimed; the first round warms up; the legs alternate in one process,
             median of `--repeats` each.
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
import job_ab
import voxel_ref as VR
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import StereoSlamBatch


def event_ms(fn, repeats, before=None):
    """median of the device time between two events around fn(); before() runs untimed ahead of every repeat"""
    out = []
    for _ in range(repeats + 1):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:]), out[1:]


def start(cfg, lefts, rights, slots, groups, device, steps):
    os.environ["SVO_GROUPS"] = str(groups)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, len(lefts), lefts[0].shape[0]), True)(slam, steps)
    return slam, packed


def fuse_leg(args, h, clouds, points, log2_one, log2_each):
    n = len(clouds)
    out = {}
    for maps_name, n_maps, log2 in (("one_map", 1, log2_one), ("map_per_slot", n, log2_each)):
        params = hip_lib.voxel_params(args.voxel, log2)
        maps = [h.voxel_new(params) for _ in range(n_maps)]
        spans = [(c, i % n_maps, 1) for i, c in enumerate(clouds)]
        for form in (0, 1):
            os.environ["SVO_VOXEL_LANE_ATOMICS"] = str(form)
            ms, all_ms = event_ms(lambda: h.voxel_fuse(spans, maps), args.repeats, before=lambda: [h.voxel_clear(m) for m in maps])
            fused = sum(h.voxel_info(m)["n_fused"] for m in maps)
            voxels = sum(h.voxel_info(m)["n_voxels"] for m in maps)
            out[f"{maps_name}_{'lane_atomics' if form else 'group_sums'}"] = {
                "maps": n_maps, "log2_capacity": log2, "records": n * points, "fused": fused, "voxels": voxels, "ms": ms, "all_ms": all_ms,
                "fused_records_per_s": fused / (ms * 1e-3)}
        os.environ.pop("SVO_VOXEL_LANE_ATOMICS")
    return out


def pile_leg(args, h, points):
    rec = VR.records(np.tile(np.array([[0.5, 0.5, 0.5]], np.float32) * args.voxel, (points, 1)), (200, 100, 50))
    dev = torch.from_numpy(rec.view(np.uint8).reshape(-1, 16)).cuda()
    log2 = max(10, int(np.ceil(np.log2(points * 4 / 3 + 2))))
    m = h.voxel_new(hip_lib.voxel_params(args.voxel, log2))
    out = {"records": points}
    for form in (0, 1):
        os.environ["SVO_VOXEL_LANE_ATOMICS"] = str(form)
        ms, all_ms = event_ms(lambda: h.voxel_fuse([(dev, 0, 1)], [m]), args.repeats, before=lambda: h.voxel_clear(m))
        out["lane_atomics" if form else "group_sums"] = {"ms": ms, "all_ms": all_ms, "records_per_s": points / (ms * 1e-3)}
    os.environ.pop("SVO_VOXEL_LANE_ATOMICS")
    return out


def extract_leg(args, h, log2):
    out = []
    cap = 1 << log2
    for frac in (1 / 16, 1 / 4, 3 / 4):
        n = int(cap * frac)
        idx = np.arange(n)
        xyz = (np.stack([idx % 512, idx // 512 % 512, idx // (512 * 512)], 1) + 0.5) * args.voxel
        dev = torch.from_numpy(VR.records(xyz, (1, 2, 3)).view(np.uint8).reshape(-1, 16)).cuda()
        m = h.voxel_new(hip_lib.voxel_params(args.voxel, log2))
        h.voxel_fuse([(dev, 0, 1)], [m])
        assert h.voxel_info(m)["n_voxels"] == n
        pts = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        ms, all_ms = event_ms(lambda: h.voxel_extract(m, points=pts, capacity=n), args.repeats)
        out.append({"log2_capacity": log2, "voxels": n, "ms": ms, "all_ms": all_ms, "voxels_per_s": n / (ms * 1e-3)})
    return out


def host_leg(args, slam, slots):
    t0 = time.perf_counter()
    job = slam.export_cloud("last_keyframes", list(range(slots)), step=args.step, layout="organized")
    t1 = time.perf_counter()
    fused = 0
    for i in range(slots):
        org = job.organized(i)
        if org is None:
            continue
        m = VR.Map(args.voxel, 26)
        m.fuse(org.ravel(), 1)
        fused += m.n_fused
    t2 = time.perf_counter()
    return {"slots": slots, "download_ms": (t1 - t0) * 1e3, "numpy_fuse_ms": (t2 - t1) * 1e3, "fused": fused,
            "fused_records_per_s": fused / (t2 - t0)}


def pipelined_leg(args, device, cfg, lefts, rights):
    slam, packed = start(cfg, lefts, rights, args.pipe_slots, args.groups, device, args.steps + args.warmup)
    slam.set_voxel_maps(args.voxel, args.pipe_log2)
    for k in range(args.warmup):
        slam.submit_packed(packed[k])
    slam.wait()
    fps = {"plain": [], "fused": []}
    for _ in range(args.repeats):
        for leg in ("plain", "fused"):
            slam.clear_voxel_maps()
            keep = []
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for k in range(args.warmup, args.warmup + args.steps):
                slam.submit_packed(packed[k])
                if leg == "fused":
                    keep.append(slam.submit_fuse("last_keyframes", None, step=args.step))
            slam.wait()
            fps[leg].append(args.steps * args.pipe_slots / (time.perf_counter() - t0))
    statuses = np.bincount(np.concatenate([j.info["status"] for j in keep]), minlength=4).tolist() if keep else []
    out = {"slots": args.pipe_slots, "groups": args.groups, "steps": args.steps, "log2_capacity": args.pipe_log2,
           "frames_per_s": {k: statistics.median(v) for k, v in fps.items()}, "all": fps, "fuse_statuses_last_leg": statuses}
    slam.close()
    return out


def sgm_leg(args, device, cfg, lefts, rights):
    slam, packed = start(cfg, lefts, rights, args.slots, 1, device, args.warmup)
    slam.set_voxel_maps(args.voxel, args.pipe_log2)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    jobs = {}
    for name, how in (("wta", dict()), ("wta_checked", dict(lr_check=args.lr)), ("sgm", dict(sgm=job_ab.sgm_dict(args.sgm, None))),
                      ("sgm_checked", dict(sgm=job_ab.sgm_dict(args.sgm, args.lr)))):
        jobs[f"fuse_{name}"] = slam.submit_fuse("last_keyframes", None, stamp=1, step=args.step, **how).wait()
        jobs[f"cloud_{name}"] = slam.submit_cloud("last_keyframes", None, step=args.step, layout="organized", device=True, **how).wait()
    offered = {name: int(job.info["n_offered"].sum()) for name, job in jobs.items() if name.startswith("fuse")}
    statuses = {name: np.bincount(job.info["status"], minlength=4).tolist() for name, job in jobs.items() if name.startswith("fuse")}
    timed = job_ab.alternate_jobs(device, jobs, args.repeats)
    out = {"slots": args.slots, "step": args.step, "lr": args.lr, "sgm": args.sgm, "voxel": args.voxel, "log2_capacity": args.pipe_log2,
           "points_per_slot": jobs["cloud_wta"].points_per_slot, "offered": offered, "fuse_statuses": statuses, "jobs": timed,
           "ratios": job_ab.ratios(timed, [("fuse_sgm", "fuse_wta"), ("fuse_sgm_checked", "fuse_wta_checked"),
                                           ("cloud_sgm", "cloud_wta"), ("cloud_sgm_checked", "cloud_wta_checked")]),
           "device_GB": slam.memory().device_bytes / 1e9}
    slam.close()
    return out


def prune_leg(args, h):
    out = []
    for log2 in args.prune_log2:
        cap = 1 << log2
        for load in (0.25, 0.5, 0.75):
            n = int(cap * load)
            idx = np.arange(n)
            xyz = (np.stack([idx % 512, idx // 512 % 512, idx // (512 * 512)], 1) + 0.5) * args.voxel
            dev = torch.from_numpy(VR.records(xyz, (1, 2, 3)).view(np.uint8).reshape(-1, 16)).cuda()
            half = n // 2
            m = h.voxel_new(hip_lib.voxel_params(args.voxel, log2))
            h.voxel_fuse([(dev[:half], 0, 1), (dev[half:], 0, 2)], [m])
            assert h.voxel_info(m)["n_voxels"] == n
            pristine = m[0].clone()
            restore = lambda: m[0].copy_(pristine)
            keep_all, keep_half = hip_lib.voxel_keep(min_stamp=1), hip_lib.voxel_keep(min_stamp=2)
            row = {"log2_capacity": log2, "load": load, "voxels": n, "kept_half": n - half}
            row["count_ms"], row["count_all_ms"] = event_ms(lambda: h.voxel_count(m), args.repeats)
            row["prune_keep_all_ms"], row["prune_keep_all_all_ms"] = event_ms(lambda: h.voxel_prune(m, keep_all), args.repeats)
            assert torch.equal(m[0], pristine)                               # nothing left: nothing written
            row["prune_keep_half_ms"], row["prune_keep_half_all_ms"] = event_ms(lambda: h.voxel_prune(m, keep_half), args.repeats, before=restore)
            assert h.voxel_info(m)["n_voxels"] == n - half
            restore()
            pts = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
            row["extract_half_ms"], row["extract_half_all_ms"] = event_ms(lambda: h.voxel_extract(m, min_stamp=2, points=pts, capacity=n), args.repeats)

            def host_path():
                _, k = h.voxel_extract(m, min_stamp=2, points=pts, capacity=n)
                rec = pts[:k].cpu()
                h.voxel_clear(m)
                h.voxel_fuse([(rec.cuda(), 0, 2)], [m])
            host = []
            for _ in range(args.repeats + 1):
                restore()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_path()
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            assert h.voxel_info(m)["n_voxels"] == n - half
            row["host_path_ms"], row["host_path_all_ms"] = statistics.median(host[1:]), host[1:]
            row["keep_all_over_count"] = row["prune_keep_all_ms"] / row["count_ms"]
            row["keep_half_over_extract_half"] = row["prune_keep_half_ms"] / row["extract_half_ms"]
            row["host_path_over_keep_half"] = row["host_path_ms"] / row["prune_keep_half_ms"]
            out.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("all_ms")}), file=sys.stderr, flush=True)
            del m, pristine, pts, dev
            torch.cuda.empty_cache()
    return out


def reeval(fn):
    """fn() under the other form of the carve's kernels: no ballot words, the stage pass evaluates the rule again"""
    os.environ["SVO_VOXEL_CARVE_REEVALUATE"] = "1"
    try:
        return fn()
    finally:
        del os.environ["SVO_VOXEL_CARVE_REEVALUATE"]


def carve_leg(args, h):
    import ctypes as C
    W, H, depth = 752, 480, 20.0
    out = []
    for log2 in args.carve_log2:
        n = int((1 << log2) * 0.75)
        idx = np.arange(n)
        xyz = (np.stack([idx % 512, idx // 512 % 512, idx // (512 * 512)], 1) + 0.5) * args.voxel
        dev = torch.from_numpy(VR.records(xyz, (1, 2, 3)).view(np.uint8).reshape(-1, 16)).cuda()
        half = n // 2
        m = h.voxel_new(hip_lib.voxel_params(args.voxel, log2))
        h.voxel_fuse([(dev[:half], 0, 1), (dev[half:], 0, 2)], [m])
        assert h.voxel_info(m)["n_voxels"] == n
        pristine = m[0].clone()
        restore = lambda: m[0].copy_(pristine)
        side = 512 * args.voxel                                   # the slab is side x side, `depth` in front of the eye
        view = (C.c_float * 12)(1, 0, 0, -side / 2, 0, 1, 0, -side / 2, 0, 0, 1, depth)
        cam = hip_lib.ArCamera(view, W * depth / side, H * depth / side, W / 2, H / 2)
        rule = hip_lib.voxel_carve(args.voxel, near=0.01, ring=1)
        pts = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        for step in (1, 4):
            cols, rows = W // step, H // step
            z = np.ones((rows, cols), np.float32)
            occ_none = torch.from_numpy(VR.records(np.stack([np.zeros_like(z), np.zeros_like(z), z], -1).reshape(-1, 3)).view(np.uint8).reshape(-1, 16)).cuda()
            z[:, cols // 2:] = 1000.0
            occ_half = torch.from_numpy(VR.records(np.stack([np.zeros_like(z), np.zeros_like(z), z], -1).reshape(-1, 3)).view(np.uint8).reshape(-1, 16)).cuda()
            seen = {}
            legs = {"carve_none": lambda: seen.__setitem__("none", h.voxel_carve(m, cam, W, H, (occ_none, cols, rows, step), rule)),
                    "carve_half": lambda: seen.__setitem__("half", h.voxel_carve(m, cam, W, H, (occ_half, cols, rows, step), rule)),
                    "carve_none_reeval": lambda: reeval(lambda: h.voxel_carve(m, cam, W, H, (occ_none, cols, rows, step), rule)),
                    "carve_half_reeval": lambda: seen.__setitem__("half_reeval", reeval(lambda: h.voxel_carve(m, cam, W, H, (occ_half, cols, rows, step), rule))),
                    "prune_all": lambda: h.voxel_prune(m, hip_lib.voxel_keep(min_stamp=1)),
                    "prune_half": lambda: h.voxel_prune(m, hip_lib.voxel_keep(min_stamp=2)),
                    "extract_all": lambda: h.voxel_extract(m, points=pts, capacity=n)}
            ms = {k: [] for k in legs}
            for _ in range(args.repeats + 1):                     # the first round warms up
                for name, fn in legs.items():
                    restore()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    ms[name].append(a.elapsed_time(b))
            assert seen["none"]["n_carved"] == 0 and seen["none"]["n_tested"] == n and seen["none"]["n_kept"] == n, seen
            assert seen["half_reeval"] == seen["half"], seen
            row = {"log2_capacity": log2, "voxels": n, "step": step, "lattice": [cols, rows], "carve_half_result": seen["half"]}
            for name in legs:
                row[name + "_ms"], row[name + "_all_ms"] = statistics.median(ms[name][1:]), ms[name][1:]
            row["reeval_over_ballot_none"] = row["carve_none_reeval_ms"] / row["carve_none_ms"]
            row["reeval_over_ballot_half"] = row["carve_half_reeval_ms"] / row["carve_half_ms"]
            row["carve_none_over_prune_all"] = row["carve_none_ms"] / row["prune_all_ms"]
            row["carve_half_over_prune_half"] = row["carve_half_ms"] / row["prune_half_ms"]
            row["carve_half_over_prune_half_plus_extract"] = row["carve_half_ms"] / (row["prune_half_ms"] + row["extract_all_ms"])
            out.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("all_ms")}), file=sys.stderr, flush=True)
        del m, pristine, pts, dev
        torch.cuda.empty_cache()
    return out


def alternate(legs, repeats, wall=False):
    """{name: (fn, before)} in turn, repeats + 1 rounds (the first warms up): {name: ms of every counted round}; device
    events around fn, or with wall the host clock between two device synchronisations"""
    ms = {k: [] for k in legs}
    for _ in range(repeats + 1):
        for name, (fn, before) in legs.items():
            if before:
                before()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 if wall else a.elapsed_time(b))
    return {k: v[1:] for k, v in ms.items()}


def lane_form(fn):
    """fn() under the other form of the fuse kernel: every lane its own atomics"""
    os.environ["SVO_VOXEL_LANE_ATOMICS"] = "1"
    try:
        return fn()
    finally:
        del os.environ["SVO_VOXEL_LANE_ATOMICS"]


def entries_leg(args, h):
    import ctypes as C
    from stereo_svo_slam_amd import synth
    out = []
    log2, k = args.entries_log2, args.entries_slots
    cfg = synth.make_sequence("tiny", 1, 0, device="cpu")[0]
    for load in (0.75, 0.25):
        n = int((1 << log2) * load) // k * k
        idx = np.arange(n)
        xyz = (np.stack([idx % 512, idx // 512 % 512, idx // (512 * 512)], 1) + 0.5) * args.voxel
        dev = torch.from_numpy(VR.records(xyz, (1, 2, 3)).view(np.uint8).reshape(-1, 16)).cuda()
        half = n // 2
        params = hip_lib.voxel_params(args.voxel, log2)
        m = h.voxel_new(params)
        h.voxel_fuse([(dev[:half], 0, 1), (dev[half:], 0, 2)], [m])
        assert h.voxel_info(m)["n_voxels"] == n
        ent, got = h.voxel_pack(m)
        assert got == n
        pts = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        dst = h.voxel_new(hip_lib.voxel_params(args.voxel, log2 + 1))           # (log2 + 1: the load bound admits n records on top of n / 2 entries)
        h.voxel_fuse([(dev[:half], 0, 1)], [dst])
        half_full = dst[0].clone()                                # a map that holds half of the span's keys
        clear, to_half = (lambda: h.voxel_clear(dst)), (lambda: dst[0].copy_(half_full))
        small = [h.voxel_new(hip_lib.voxel_params(args.voxel, log2 - 2)) for _ in range(k)]       # one map per slot: n / k records each
        clear_small = lambda: [h.voxel_clear(x) for x in small]
        per = n // k
        ent_spans = [(ent[i * per:(i + 1) * per], i, args.voxel) for i in range(k)]
        rec_spans = [(dev[i * per:(i + 1) * per], i, 1) for i in range(k)]
        bigger = torch.empty(hip_lib.voxel_map_bytes(log2 + 1), dtype=torch.uint8, device="cuda")
        vm = hip_lib._voxel_map(m)
        seen = {}
        legs = {"pack": (lambda: h.voxel_pack(m, entries=ent, capacity=n), None),
                "extract": (lambda: h.voxel_extract(m, points=pts, capacity=n), None),
                "merge_empty": (lambda: seen.__setitem__("empty", h.voxel_merge([(ent, 0, args.voxel)], [dst])), clear),
                "fuse_empty_group_sums": (lambda: h.voxel_fuse([(dev, 0, 1)], [dst]), clear),
                "fuse_empty_lane_atomics": (lambda: lane_form(lambda: h.voxel_fuse([(dev, 0, 1)], [dst])), clear),
                "merge_half": (lambda: seen.__setitem__("half", h.voxel_merge([(ent, 0, args.voxel)], [dst])), to_half),
                "fuse_half_group_sums": (lambda: h.voxel_fuse([(dev, 0, 1)], [dst]), to_half),
                "fuse_half_lane_atomics": (lambda: lane_form(lambda: h.voxel_fuse([(dev, 0, 1)], [dst])), to_half),
                "merge_per_slot": (lambda: h.voxel_merge(ent_spans, small), clear_small),
                "fuse_per_slot_group_sums": (lambda: h.voxel_fuse(rec_spans, small), clear_small),
                "fuse_per_slot_lane_atomics": (lambda: lane_form(lambda: h.voxel_fuse(rec_spans, small)), clear_small),
                "rehash": (lambda: hip_lib._check(hip_lib.lib().svo_voxel_rehash(h._h, C.byref(vm), C.c_void_p(bigger.data_ptr()), log2 + 1)), None),
                "prune_keep_all": (lambda: h.voxel_prune(m, hip_lib.voxel_keep(min_stamp=1)), None)}
        ms = alternate(legs, args.repeats)
        assert seen["empty"][0]["n_claimed"] == n and seen["half"][0]["n_claimed"] == n - half and seen["half"][0]["n_merged"] == n, seen
        assert h.voxel_info(bigger)["n_voxels"] == n and h.voxel_info(m)["n_voxels"] == n
        row = {"log2_capacity": log2, "load": load, "entries": n, "slots": k}
        for name in legs:
            row[name + "_ms"], row[name + "_all_ms"] = statistics.median(ms[name]), ms[name]
        for a, b in (("pack", "extract"), ("merge_empty", "fuse_empty_group_sums"), ("merge_empty", "fuse_empty_lane_atomics"),
                     ("merge_half", "fuse_half_group_sums"), ("merge_half", "fuse_half_lane_atomics"), ("merge_per_slot", "fuse_per_slot_group_sums"),
                     ("merge_per_slot", "fuse_per_slot_lane_atomics"), ("rehash", "prune_keep_all")):
            row[f"{a}_over_{b}"] = row[a + "_ms"] / row[b + "_ms"]
        del dst, half_full, small, bigger
        torch.cuda.empty_cache()

        # the ctx: the resize beside the host path it replaces (wall clock)
        os.environ["SVO_GROUPS"] = "1"
        slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], 1, 0)
        stage = h.voxel_new(hip_lib.voxel_params(args.voxel, log2 + 1))

        def restore():
            slam.set_voxel_maps(args.voxel, log2)
            assert slam.load_voxel_maps([0], [ent], voxel=args.voxel).status(0) == hip_lib.VOXEL_LOADED

        def host_path():
            job = slam.export_voxel_maps([0])
            slam.set_voxel_maps(args.voxel, log2 + 1)
            rec = torch.from_numpy(job.points(0).view(np.uint8).reshape(-1, 16)).cuda()
            h.voxel_clear(stage)
            h.voxel_fuse([(rec, 0, 1)], [stage])
        ms = alternate({"ctx_resize": (lambda: slam.resize_voxel_maps(log2 + 1), restore), "ctx_host_path": (host_path, restore)}, args.repeats, wall=True)
        restore()
        slam.resize_voxel_maps(log2 + 1)
        info = slam.voxel_map_info(0)
        assert (info["n_voxels"], info["log2_capacity"], info["n_fused"]) == (n, log2 + 1, n) and h.voxel_info(stage)["n_voxels"] == n
        slam.close()
        for name in ms:
            row[name + "_wall_ms"], row[name + "_all_wall_ms"] = statistics.median(ms[name]), ms[name]
        row["ctx_host_path_over_ctx_resize"] = row["ctx_host_path_wall_ms"] / row["ctx_resize_wall_ms"]
        out.append(row)
        print(json.dumps({k_: v for k_, v in row.items() if "_all_" not in k_}), file=sys.stderr, flush=True)
        del m, ent, pts, dev, stage
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--entries", action="store_true", help="only the pack, merge, rehash and resize measurement (profiles/voxel_entries_bench.json)")
    ap.add_argument("--entries-log2", type=int, default=24)
    ap.add_argument("--entries-slots", type=int, default=4, help="--entries: the maps of the one-map-per-slot legs")
    ap.add_argument("--carve", action="store_true", help="only the carve measurement (profiles/voxel_carve_bench.json)")
    ap.add_argument("--carve-log2", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--prune", action="store_true", help="only the prune measurement (profiles/voxel_prune_bench.json)")
    ap.add_argument("--prune-log2", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--sgm", metavar="P1,P2[,CAP]", default=None, help="only the fuse job under SGM against winner-takes-all (profiles/sgm_consumers_bench.json)")
    ap.add_argument("--lr", type=float, default=1.0, help="--sgm: the tolerance of the checked legs")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pipe-slots", type=int, default=1024)
    ap.add_argument("--pipe-log2", type=int, default=18)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    if args.entries:
        out = {"tool": "tools/voxel_bench.py", "date": datetime.date.today().isoformat(), "command": " ".join(sys.argv),
               "device": torch.cuda.get_device_name(0), "voxel": args.voxel, "repeats": args.repeats,
               "entries": entries_leg(args, hip_lib.Handle(0, 1024))}
        with open(args.out or os.path.join(ROOT, "profiles", "voxel_entries_bench.json"), "w") as fh:
            json.dump(out, fh, indent=1)
        print(json.dumps(out))
        return
    if args.carve:
        out = {"tool": "tools/voxel_bench.py", "date": datetime.date.today().isoformat(), "command": " ".join(sys.argv),
               "device": torch.cuda.get_device_name(0), "voxel": args.voxel, "repeats": args.repeats, "view": [752, 480],
               "carve": carve_leg(args, hip_lib.Handle(0, 1024))}
        with open(args.out or os.path.join(ROOT, "profiles", "voxel_carve_bench.json"), "w") as fh:
            json.dump(out, fh, indent=1)
        print(json.dumps(out))
        return
    if args.prune:
        out = {"tool": "tools/voxel_bench.py", "date": datetime.date.today().isoformat(), "command": " ".join(sys.argv),
               "device": torch.cuda.get_device_name(0), "voxel": args.voxel, "repeats": args.repeats,
               "prune": prune_leg(args, hip_lib.Handle(0, 1024))}
        with open(args.out or os.path.join(ROOT, "profiles", "voxel_prune_bench.json"), "w") as fh:
            json.dump(out, fh, indent=1)
        print(json.dumps(out))
        return
    cfg, lefts, rights = bench.render_loops("euroc", list(range(min(8, args.slots))), args.loop_frames, device)
    if args.sgm:
        leg = dict(sgm_leg(args, device, cfg, lefts, rights), tool="tools/voxel_bench.py", command=" ".join(sys.argv), device=torch.cuda.get_device_name(0))
        job_ab.merge_result(args.out or os.path.join(ROOT, "profiles", "sgm_consumers_bench.json"), "fuse", leg)
        print(json.dumps(leg))
        return
    slam, packed = start(cfg, lefts, rights, args.slots, 1, device, args.warmup)
    for k in range(args.warmup):
        slam.submit_packed(packed[k])
    slam.wait()
    job = slam.export_cloud("last_keyframes", None, step=args.step, layout="organized", device=True)
    points = job.points_per_slot
    clouds = [job.points_buffer[i * points:(i + 1) * points] for i in range(args.slots) if int(job.segments[i]["status"]) == hip_lib.CLOUD_OK]
    h = hip_lib.Handle(0, 1024)
    total = len(clouds) * points
    log2_one = min(26, int(np.ceil(np.log2(total * 4 / 3 + 2))))
    log2_each = max(10, int(np.ceil(np.log2(points * 4 / 3 + 2))))
    out = {"tool": "tools/voxel_bench.py", "date": datetime.date.today().isoformat(), "command": " ".join(sys.argv),
           "device": torch.cuda.get_device_name(0), "step": args.step, "voxel": args.voxel, "points_per_slot": points,
           "fuse": fuse_leg(args, h, clouds, points, log2_one, log2_each), "pile": pile_leg(args, h, points),
           "extract": extract_leg(args, h, 22), "host_path": host_leg(args, slam, min(args.slots, 16))}
    slam.close()
    out["pipelined"] = pipelined_leg(args, device, cfg, lefts, rights)
    path = args.out or os.path.join(ROOT, "profiles", "voxel_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
