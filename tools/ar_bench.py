"""What the AR demo's picture costs on the MI355X: the two kernels through the stage entry, the ctx's job in device and
host mode, and pictures queued between the steps of bench.py's workload.

bench.py's workload (C2 `euroc`, borrowed device frames from bench.py's rendered loops, pipelined submits), in one
process:

  kernel     256 slots in one group after `--warmup` steps. Every slot shows one box (12 triangles, each face tens of
             tiles) and one tessellated sphere (`--sphere` x 2 `--sphere` bands: a few thousand small triangles), both
             placed a metre in front of the slot's own current pose, so that every image has them in view. The stage
             entry svo_render_ar on the slots' level-0 planes (through a device-mode view job), 752 x 480 RGBA; median
             of `--repeats` calls between two device events. A call is the upload of its tables, both kernels and a
             stream synchronise. The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this
             tool with --kernel-only, in a run of its own: this tool cannot record them.
  job        the ctx's own job of every slot (submit + wait, host clock) in device and in host mode: the host's table
             building, one upload, the kernels and a stream synchronise (host mode: and the copies out). Beside it, on
             the same output bytes: the device-mode RGBA view job of §4.11 (in this run).
  pipelined  frames/s over `--steps` queued steps without pictures and with a device-mode picture of every slot queued
             behind every 10th frame set; legs alternate, median of `--pipelined-repeats` each.
Prints one JSON line.

--occluded STEP[,STEP...] measures the occluded picture instead, per lattice step, on the same workload
and meshes, and writes profiles/ar_occlusion_bench.json unless --out names another file:

  kernel     the stage entry with an occluder (ar_render_kernel<true>; the lattices are the slots' checked camera-frame
             clouds, computed once by a device-mode cloud job) against the stage entry without (ar_render_kernel<false>),
             alternating, median of `--repeats` calls each between two device events.
  job        the occluded job of every slot (submit + wait, host clock, device mode) against the unoccluded job plus a
             checked device-mode cloud job of the same style, which it replaces; medians and every repeat, so that the
             spread can be read.
  host path  what a caller did before, for `--host-slots` slots: the cloud to the host, the picture to the host, a numpy
             rasteriser for the meshes' depths, the composition; seconds per slot beside the job's.
  pipelined  frames/s with nothing, with a plain picture and with an occluded picture of every slot behind every 10th
             frame set.

--occluded STEPS --sgm P1,P2[,CAP] measures only the occluded job (sets the key "ar" of
profiles/sgm_consumers_bench.json): at every step the job through svo_submit_export_ar_occluded and through
svo_submit_export_ar_occluded_sgm, unchecked and checked at tolerance `--lr`; the legs alternate in one process, median of
`--repeats` each.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting: 14 groups of 256)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
import job_ab
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.stereo_slam import ArPictures, StereoSlamBatch

HBM_PEAK = 8.0e12
BOX_RGB, SPHERE_RGB = 0xc08040, 0x4080c0


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


def sphere(radius, bands):
    """a UV sphere: (vertices float32 [V, 3], triangles int32 [T, 3]), 2 * bands * (bands - 1) * 2 triangles"""
    lat = np.linspace(0, np.pi, bands + 1)
    lon = np.linspace(0, 2 * np.pi, 2 * bands, endpoint=False)
    v = np.array([[np.sin(a) * np.cos(b), np.cos(a), np.sin(a) * np.sin(b)] for a in lat for b in lon], np.float32) * np.float32(radius)
    n = 2 * bands
    t = []
    for i in range(bands):
        for j in range(n):
            a, b, c, d = i * n + j, i * n + (j + 1) % n, (i + 1) * n + j, (i + 1) * n + (j + 1) % n
            if i > 0:
                t.append((a, b, c))
            if i < bands - 1:
                t.append((b, d, c))
    return v, np.array(t, np.int32)


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.sqrt(r @ r)
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def placed(slam, slots):
    """two instances per slot, a metre in front of its current pose: (instances, first)"""
    inst = []
    for s in range(slots):
        p = slam.pose(s)
        R = rodrigues(p[3:6])
        inst.append((hip_lib.ar_model(p[:3] + R @ np.array([-0.25, 0.0, 1.0]), 1.0, R @ rodrigues([0.4, 0.6, 0.0])), 0, BOX_RGB))
        inst.append((hip_lib.ar_model(p[:3] + R @ np.array([0.3, 0.0, 1.2])), 1, SPHERE_RGB))
    return inst, [2 * s for s in range(slots + 1)]


def start(cfg, lefts, rights, slots, groups, device, steps):
    if groups:
        os.environ["SVO_GROUPS"] = str(groups)
    else:
        os.environ.pop("SVO_GROUPS", None)
    slam = StereoSlamBatch(cfg, cfg["width"], cfg["height"], slots, device.index)
    packed = bench.step_packer(lefts, rights, bench.loop_plan(slots, len(lefts), lefts[0].shape[0]), True)(slam, steps)
    return slam, packed


def job_leg(args, device, cfg, lefts, rights, meshes):
    slots = args.slots
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    W, H = cfg["width"], cfg["height"]
    inst, first = placed(slam, slots)
    style = hip_lib.ar_style(pixel="rgba8")
    tri = sum(len(meshes[k][1]) for _, k, _ in inst[:2])
    out = {"slots": slots, "warmup_steps": args.warmup, "cols": W, "rows": H, "triangles_per_slot": tri,
           "box_triangles": len(meshes[0][1]), "sphere_triangles": len(meshes[1][1])}
    job = ArPictures(slam, None, style, meshes, inst, first, True).submit().wait()
    px = job.pixels.view(slots, -1)[:, :H * W * 4].view(slots, H, W, 4)
    out["covered_fraction"] = float(((px[..., 0] != px[..., 1]) | (px[..., 1] != px[..., 2])).float().mean())
    out["bytes_written"] = written = slots * H * job.pitch
    # the stage entry on the same planes
    views = slam.submit_views("frames", pixel="gray8", device=True).wait()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    dm = [(dev(m[0]), dev(m[1])) for m in meshes]
    h = hip_lib.Handle(device.index, 1024)
    srcs = [((views.pixels.data_ptr() + s * views.image_bytes, W, H, W),
             [(m, dm[k][0], dm[k][1], None, rgb) for m, k, rgb in inst[2 * s:2 * s + 2]]) for s in range(slots)]
    _, cam = slam.slot_rig(0)
    cams = [hip_lib.ar_camera_of_pose(slam.pose(s), cam) for s in range(slots)]
    dst = torch.empty(slots * job.image_bytes, dtype=torch.uint8, device=device)
    packed_ar = h.pack_ar(srcs, cams, [s * job.image_bytes for s in range(slots)])
    call = lambda: h.render_ar_packed(packed_ar, style, dst)
    call()
    out["stage_entry_equals_job"] = bool(torch.equal(dst, job.pixels))
    if not args.kernel_only:
        ms, all_ms = event_ms(call, args.repeats)
        out["stage_entry"] = {"call_ms": ms, "call_ms_all": all_ms, "bytes_per_s": written / (ms * 1e-3),
                              "tiles": slots * ((W + 63) // 64) * ((H + 15) // 16), "records": slots * tri}
        ms, all_ms = median_ms(device, lambda: job.submit().wait(), args.repeats)
        out["device_mode_job"] = {"job_ms": ms, "job_ms_all": all_ms, "bytes_per_s": written / (ms * 1e-3),
                                  "fraction_of_hbm_peak": written / (ms * 1e-3) / HBM_PEAK}
        host = ArPictures(slam, None, style, meshes, inst, first, False).submit().wait()
        ms, all_ms = median_ms(device, lambda: host.submit().wait(), args.repeats)
        out["host_mode_job"] = {"job_ms": ms, "job_ms_all": all_ms, "bytes_per_s": written / (ms * 1e-3)}
        del host
        box_only = ArPictures(slam, None, style, meshes, inst[0::2], list(range(slots + 1)), True).submit().wait()
        ms, all_ms = median_ms(device, lambda: box_only.submit().wait(), args.repeats)
        out["device_mode_job_box_only"] = {"job_ms": ms, "job_ms_all": all_ms}
        del box_only
        v = slam.submit_views("frames", pixel="rgba8", device=True).wait()
        ms, all_ms = median_ms(device, lambda: v.submit().wait(), args.repeats)
        out["view_rgba8_job"] = {"job_ms": ms, "job_ms_all": all_ms, "bytes_written": v.capacity, "bytes_per_s": v.capacity / (ms * 1e-3)}
    out["device_GB"] = slam.memory().device_bytes / 1e9
    h.close()
    slam.close()
    return out


def pipelined_leg(args, device, cfg, lefts, rights, slots, groups, meshes):
    K, W, every = args.steps, args.warmup, 10
    n = min(slots, len(lefts))
    runs_n = 2 * args.pipelined_repeats
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, groups, device, W + runs_n * K)
    for pk in packed[:W]:
        slam.submit_packed(pk)
    slam.wait()
    out = {"slots": slots, "groups": slam.groups(), "steps": K, "ar_every": every}
    inst, first = placed(slam, slots)
    style = hip_lib.ar_style(pixel="rgba8")
    ring = [ArPictures(slam, None, style, meshes, inst, first, True).submit().wait() for _ in range(2)]
    runs = {"plain": [], "ar": []}
    for r in range(runs_n):
        kind = ("plain", "ar")[r % 2]
        steps = packed[W + r * K:W + (r + 1) * K]

        def run():
            for k, pk in enumerate(steps):
                slam.submit_packed(pk)
                if kind == "ar" and k % every == every - 1:
                    ring[(k // every) % 2].submit()
            slam.wait()
        runs[kind].append(slots * K / timed(device, run))
    for kind in runs:
        out[f"frames_per_s_{kind}"] = statistics.median(runs[kind])
        out[f"frames_per_s_{kind}_all"] = runs[kind]
    out["ar_vs_plain"] = out["frames_per_s_ar"] / out["frames_per_s_plain"]
    out["ar_bytes_per_job"] = ring[0].capacity
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def host_depths(H, W, camera, draws, near):
    """float32 [H, W]: the smallest depth of the meshes per pixel (+inf: none), rasterised on the host in numpy with the
    arithmetic of include/svo_hip.h, "ar": what a caller needed before the job could occlude"""
    cam = np.frombuffer(bytes(camera), np.float32)
    V, fx, fy, cx, cy = cam[:12].reshape(3, 4).astype(np.float64), cam[12], cam[13], cam[14], cam[15]
    depth = np.full((H, W), np.inf, np.float32)
    for model, vertices, triangles in draws:
        M = np.asarray(model, np.float64).reshape(3, 4)
        w = vertices.astype(np.float64) @ M[:, :3].T + M[:, 3]
        c = w @ V[:, :3].T + V[:, 3]
        ok = c[:, 2] >= near
        z = np.where(ok, c[:, 2], 1.0)
        X = np.floor((fx * c[:, 0] / z + cx) * 16).astype(np.int64)
        Y = np.floor((fy * c[:, 1] / z + cy) * 16).astype(np.int64)
        for t in triangles:
            if not ok[t].all():
                continue
            x, y, d = X[t], Y[t], c[t, 2]
            A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
            x0, x1 = max((x.min() + 7) >> 4, 0), min((x.max() - 8) >> 4, W - 1)
            y0, y1 = max((y.min() + 7) >> 4, 0), min((y.max() - 8) >> 4, H - 1)
            if A == 0 or x0 > x1 or y0 > y1:
                continue
            px, py = np.meshgrid(16 * np.arange(x0, x1 + 1) + 8, 16 * np.arange(y0, y1 + 1) + 8)
            E = [((x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a])) * (1 if A > 0 else -1) for a, b in ((1, 2), (2, 0), (0, 1))]
            inside = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
            zz = ((E[0] * d[0] + E[1] * d[1] + E[2] * d[2]) / abs(A)).astype(np.float32)
            sub = depth[y0:y1 + 1, x0:x1 + 1]
            sub[inside & (zz < sub)] = zz[inside & (zz < sub)]
    return depth


def spread(all_ms):
    return {"min_ms": min(all_ms), "max_ms": max(all_ms), "spread_ms": max(all_ms) - min(all_ms)}


def occluded_leg(args, device, cfg, lefts, rights, meshes, step):
    slots = args.slots
    n = min(slots, len(lefts))
    K, every = args.steps, 10
    runs_n = 3 * args.pipelined_repeats
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup + (0 if args.kernel_only else runs_n * K))
    for pk in packed[:args.warmup]:
        slam.submit_packed(pk)
    slam.wait()
    W, H = cfg["width"], cfg["height"]
    progress = lambda what: print(f"step {step}: {what}", file=sys.stderr, flush=True)
    progress("warmed up")
    inst, first = placed(slam, slots)
    style = hip_lib.ar_style(pixel="rgba8")
    occ = dict(step=step, margin=args.margin, max_depth=args.max_depth, lr_check=args.lr)
    out = {"step": step, "slots": slots, "warmup_steps": args.warmup, "cols": W, "rows": H, "occlusion": occ,
           "triangles_per_slot": sum(len(meshes[k][1]) for _, k, _ in inst[:2])}
    plain = ArPictures(slam, None, style, meshes, inst, first, True).submit().wait()
    job = ArPictures(slam, None, style, meshes, inst, first, True, occ).submit().wait()
    cloud = slam.submit_cloud("frames", None, step=step, frame="camera", layout="organized", max_depth=args.max_depth, lr_check=args.lr or None,
                              device=True).wait()
    vis = job.visibility
    out["covered"], out["hidden"] = int(vis["covered"].sum()), int(vis["hidden"].sum())
    out["hidden_fraction"] = out["hidden"] / max(out["covered"], 1)
    out["occluder_points_per_slot"] = float(vis["occluder_points"].mean())
    out["lattice_bytes_per_slot"] = 16 * cloud.points_per_slot
    # the stage entry on the same planes, with the clouds as occluders
    views = slam.submit_views("frames", pixel="gray8", device=True).wait()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    dm = [(dev(m[0]), dev(m[1])) for m in meshes]
    h = hip_lib.Handle(device.index, 1024)
    srcs = [((views.pixels.data_ptr() + s * views.image_bytes, W, H, W),
             [(m, dm[k][0], dm[k][1], None, rgb) for m, k, rgb in inst[2 * s:2 * s + 2]]) for s in range(slots)]
    _, cam = slam.slot_rig(0)
    cams = [hip_lib.ar_camera_of_pose(slam.pose(s), cam) for s in range(slots)]
    dst = torch.empty(slots * job.image_bytes, dtype=torch.uint8, device=device)
    packed_ar = h.pack_ar(srcs, cams, [s * job.image_bytes for s in range(slots)])
    occluders = h.pack_ar_occluders([(cloud.points_buffer.data_ptr() + 16 * int(e["first_point"]), cloud.cols, cloud.rows, step)
                                     for e in cloud.segments])
    occlusion = hip_lib.ar_occlusion(step=step, margin=args.margin)
    with_occ = lambda: h.render_ar_packed(packed_ar, style, dst, occluders, occlusion)
    without = lambda: h.render_ar_packed(packed_ar, style, dst)
    v2 = with_occ()
    out["stage_entry_equals_job"] = bool(torch.equal(dst, job.pixels)) and bool((v2["covered"] == vis["covered"]).all() and (v2["hidden"] == vis["hidden"]).all())
    without()
    out["stage_entry_plain_equals_job"] = bool(torch.equal(dst, plain.pixels))
    if not args.kernel_only:
        a_all, b_all = [], []
        for _ in range(args.repeats):                                  # alternating
            b_all += event_ms(without, 1)[1]
            a_all += event_ms(with_occ, 1)[1]
        a, b = statistics.median(a_all), statistics.median(b_all)
        progress("stage entry timed")
        out["stage_entry"] = {"occluded_call_ms": a, "plain_call_ms": b, "ratio": a / b, "occluded_call_ms_all": a_all, "plain_call_ms_all": b_all}
        legs = {"occluded_job": lambda: job.submit().wait(), "plain_job": lambda: plain.submit().wait(), "cloud_job": lambda: cloud.submit().wait()}
        all_ms = {k: [] for k in legs}
        for k in legs:
            legs[k]()
        for _ in range(args.repeats):                                  # alternating
            for k in legs:
                all_ms[k].append(timed(device, legs[k]) * 1e3)
        med = {k: statistics.median(v) for k, v in all_ms.items()}
        out["job"] = {f"{k}_ms": med[k] for k in legs}
        out["job"].update({f"{k}_ms_all": all_ms[k] for k in legs})
        out["job"]["plain_plus_cloud_ms"] = med["plain_job"] + med["cloud_job"]
        out["job"]["occluded_vs_plain_plus_cloud"] = med["occluded_job"] / (med["plain_job"] + med["cloud_job"])
        out["job"]["spread"] = {k: spread(all_ms[k]) for k in legs}
        progress("jobs timed")
        # the host path it replaces, for a few slots
        hs = list(range(min(args.host_slots, slots)))
        t0 = time.perf_counter()
        hc = slam.export_cloud("frames", hs, step=step, frame="camera", layout="organized", max_depth=args.max_depth, lr_check=args.lr or None)
        hp = ArPictures(slam, hs, style, meshes, [x for s in hs for x in inst[2 * s:2 * s + 2]], [2 * i for i in range(len(hs) + 1)], False).submit().wait()
        t1 = time.perf_counter()
        gray = slam.export_views("frames", hs, plane="left", level=0, pixel="gray8")
        differ = 0
        for i, s in enumerate(hs):
            z = host_depths(H, W, cams[s], [(m, meshes[k][0], meshes[k][1]) for m, k, _ in inst[2 * s:2 * s + 2]], style.near)
            rec = hc.organized(i)
            zo = np.where(((rec["flags"] & 0x80) == 0) & np.isfinite(rec["z"]) & (rec["z"] > 0), rec["z"], np.inf).astype(np.float32)
            full = np.full((H, W), np.inf, np.float32)
            full[:hc.rows * step, :hc.cols * step] = zo.repeat(step, 0).repeat(step, 1)
            hide = np.isfinite(z) & (z > full + np.float32(args.margin))
            img = hp.image(i).copy()
            img[hide, :3] = gray.image(i)[hide][:, None]
            got = job.image(s).cpu().numpy()
            differ += int((img != got).any(axis=2).sum())
        t2 = time.perf_counter()
        out["host_path"] = {"slots": len(hs), "exports_s_per_slot": (t1 - t0) / len(hs), "rasterise_compose_s_per_slot": (t2 - t1) / len(hs),
                            "total_s_per_slot": (t2 - t0) / len(hs), "occluded_job_s_per_slot": med["occluded_job"] * 1e-3 / slots,
                            "pixels_differing_from_the_job": differ,
                            "note": "the host rasteriser computes in float64: a few pixels at depth ties may differ from the job"}
        progress("host path timed")
        # pictures behind every 10th frame set
        rings = {"plain": None, "ar": [plain, ArPictures(slam, None, style, meshes, inst, first, True).submit().wait()],
                 "occluded": [job, ArPictures(slam, None, style, meshes, inst, first, True, occ).submit().wait()]}
        runs = {k: [] for k in rings}
        for r in range(runs_n):
            kind = ("plain", "ar", "occluded")[r % 3]
            steps = packed[args.warmup + r * K:args.warmup + (r + 1) * K]

            def run():
                for k, pk in enumerate(steps):
                    slam.submit_packed(pk)
                    if rings[kind] and k % every == every - 1:
                        rings[kind][(k // every) % 2].submit()
                slam.wait()
            runs[kind].append(slots * K / timed(device, run))
        out["pipelined"] = {"steps": K, "every": every, "groups": slam.groups()}
        for kind in runs:
            out["pipelined"][f"frames_per_s_{kind}"] = statistics.median(runs[kind])
            out["pipelined"][f"frames_per_s_{kind}_all"] = runs[kind]
        out["pipelined"]["occluded_vs_plain"] = out["pipelined"]["frames_per_s_occluded"] / out["pipelined"]["frames_per_s_plain"]
    out["device_GB"] = slam.memory().device_bytes / 1e9
    h.close()
    slam.close()
    return out


def sgm_leg(args, device, cfg, lefts, rights, meshes, steps):
    slots = args.slots
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    inst, first = placed(slam, slots)
    style = hip_lib.ar_style(pixel="rgba8")
    out = {"slots": slots, "margin": args.margin, "max_depth": args.max_depth, "lr": args.lr, "sgm": args.sgm, "steps": {}}
    for step in steps:
        jobs = {}
        for name, how in (("wta", dict()), ("wta_checked", dict(lr_check=args.lr)), ("sgm", dict(sgm=job_ab.sgm_dict(args.sgm, None))),
                          ("sgm_checked", dict(sgm=job_ab.sgm_dict(args.sgm, args.lr)))):
            occ = dict(step=step, margin=args.margin, max_depth=args.max_depth, **how)
            jobs[name] = ArPictures(slam, None, style, meshes, inst, first, True, occ).submit().wait()
        timed = job_ab.alternate_jobs(device, jobs, args.repeats)
        out["steps"][str(step)] = {"hidden": {k: int(j.visibility["hidden"].sum()) for k, j in jobs.items()},
                                   "covered": int(jobs["wta"].visibility["covered"].sum()),
                                   "occluder_points": {k: int(j.visibility["occluder_points"].sum()) for k, j in jobs.items()}, "jobs": timed,
                                   "ratios": job_ab.ratios(timed, [("sgm", "wta"), ("sgm_checked", "wta_checked")])}
        print(json.dumps({str(step): out["steps"][str(step)]}), file=sys.stderr, flush=True)
        del jobs
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--occluded: only the occluded job under SGM against winner-takes-all (profiles/sgm_consumers_bench.json)")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sphere", type=int, default=32, help="bands of the sphere: 4 * bands * (bands - 1) triangles")
    ap.add_argument("--kernel-only", action="store_true", help="one job and one stage-entry call, nothing timed: for a kernel trace")
    ap.add_argument("--legs", default="256:1", help="slots:groups per pipelined leg (groups 0: the ctx's default); '' for none")
    ap.add_argument("--loops", type=int, default=64)
    ap.add_argument("--loop-frames", type=int, default=bench.LOOP_FRAMES)
    ap.add_argument("--steps", type=int, default=40, help="steps of one timed pipelined run")
    ap.add_argument("--warmup", type=int, default=60, help="steps before anything is timed")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--pipelined-repeats", type=int, default=5, help="timed runs per kind of a pipelined leg")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--occluded", metavar="STEP[,STEP...]", default=None,
                    help="measure the occluded picture at these lattice steps instead (writes profiles/ar_occlusion_bench.json unless --out)")
    ap.add_argument("--margin", type=float, default=0.05, help="--occluded: the margin")
    ap.add_argument("--max-depth", type=float, default=20.0, help="--occluded: the cloud's max_depth filter")
    ap.add_argument("--lr", type=float, default=1.5, help="--occluded: the left-right tolerance (0: unchecked)")
    ap.add_argument("--host-slots", type=int, default=2, help="--occluded: slots the host path is timed on")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    legs = [tuple(int(x) for x in l.split(":")) for l in args.legs.split(",") if l] if not args.kernel_only else []
    n_loops = min(max([s for s, _ in legs] + [args.slots]), args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    meshes = [hip_lib.ar_box(0.3), sphere(0.15, args.sphere)]
    if args.sgm and not args.occluded:
        ap.error("--sgm needs --occluded STEPS")
    if args.occluded and args.sgm:
        n_loops = min(args.slots, args.loops)
        leg = dict(sgm_leg(args, device, cfg, lefts[:n_loops], rights[:n_loops], meshes, [int(x) for x in args.occluded.split(",")]),
                   tool="tools/ar_bench.py", command=" ".join(sys.argv), device=torch.cuda.get_device_name(0))
        job_ab.merge_result(args.out or os.path.join(ROOT, "profiles", "sgm_consumers_bench.json"), "ar", leg)
        print(json.dumps(leg), flush=True)
        return
    if args.occluded:
        n_loops = min(args.slots, args.loops)
        out = {"metric": "ar_occlusion_bench", "config": "euroc", "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "steps": []}
        for step in (int(x) for x in args.occluded.split(",")):
            out["steps"].append(occluded_leg(args, device, cfg, lefts[:n_loops], rights[:n_loops], meshes, step))
            print(json.dumps(out["steps"][-1]), file=sys.stderr, flush=True)
        text = json.dumps(out)
        path = args.out or os.path.join(ROOT, "profiles", "ar_occlusion_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
        print(text, flush=True)
        return
    out = {"metric": "ar_bench", "config": "euroc", "hbm_peak_bytes_per_s": HBM_PEAK, "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]),
           "job": job_leg(args, device, cfg, lefts, rights, meshes), "legs": []}
    print(json.dumps(out["job"]), file=sys.stderr, flush=True)        # (progress)
    for slots, groups in legs:
        out["legs"].append(pipelined_leg(args, device, cfg, lefts, rights, slots, groups, meshes))
        print(json.dumps(out["legs"][-1]), file=sys.stderr, flush=True)
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
