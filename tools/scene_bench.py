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

--clouds STEPS (e.g. 1,2,4) measures the cloud points of DESIGN §4.20 instead and writes profiles/scene_cloud_bench.json:
`--cloud-slots` slots in one group at the ctx's 752 x 480, their dense clouds (device mode, organized) at every step,
drawn into 640 x 480 RGBA pictures from behind each slot's pose.
  stage      svo_render_scene_clouds on the clouds alone (no keypoints, no lines), device events around a call: the
             clear of the key planes, the splat pass and the CLOUDS tile kernel; records/s and the keys offered
             (8 bytes each) per second beside the guide's chip-wide atomic rate. `tiles_only`: the same images without
             spans (the CLOUDS = false kernel alone). `walked_by_every_tile`: the kept records as one keyframe set per
             image through svo_render_scene, the form the splat pass replaces. `pile`: one slot's record count on one
             pixel, distinct depths.
  job        the device-mode scene job without and with the live layer (submit + wait, host clock), and the cloud job
             that the layer runs first.

--clouds STEPS --sgm P1,P2[,CAP] measures only the job with the live layer (sets the key "scene" of
profiles/sgm_consumers_bench.json): at every step the scene job through svo_submit_export_scenes_clouds and through
svo_submit_export_scenes_clouds_sgm, unchecked and checked at tolerance `--lr`; the legs alternate in one process, median
of `--repeats` each.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")         # (bench.py's setting: 14 groups of 256)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stereo-svo-slam_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import bench
import job_ab
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


ATOMIC_RATE = 1.3e12        # chip-wide rate of global float atomic adds, bytes/s (the microarchitecture guide)
CLOUD_SIZE = (640, 480)


def behind(pose, cols, rows, back=1.0):
    """a camera `back` behind a pose, looking along its viewing direction"""
    r = np.asarray(pose[3:6], np.float64)
    angle = np.sqrt(r @ r)
    k = r / angle if angle > 0 else np.zeros(3)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)            # Rodrigues
    t = np.asarray(pose[:3], np.float64)
    return hip_lib.scene_look_at(t - back * R[:, 2], t + R[:, 2], -R[:, 1], 60.0, cols, rows, 0.05)


def offered_keys(rec, cam, cols, rows, size):
    """how many keys the splat pass offers for the records [n, 4] int32 (float64 on the device: a count, not the picture)"""
    v = torch.tensor(list(cam.view), dtype=torch.float64, device=rec.device).reshape(3, 4)
    xyz = rec[:, :3].contiguous().view(torch.float32).double()
    c = xyz @ v[:, :3].T + v[:, 3]
    ok = (((rec[:, 3] >> 24) & 0x80) == 0) & torch.isfinite(c).all(dim=1) & (c[:, 2] >= cam.near)
    z = torch.where(ok, c[:, 2], torch.ones_like(c[:, 2]))
    u, w = cam.f * c[:, 0] / z + cam.cx, cam.f * c[:, 1] / z + cam.cy
    ok &= (u.abs() < 32768) & (w.abs() < 32768)
    x0, y0 = torch.floor(u) - (size - 1) // 2, torch.floor(w) - (size - 1) // 2
    nx = (torch.clamp(x0 + size - 1, max=cols - 1) - torch.clamp(x0, min=0) + 1).clamp(min=0)
    ny = (torch.clamp(y0 + size - 1, max=rows - 1) - torch.clamp(y0, min=0) + 1).clamp(min=0)
    return int((nx * ny)[ok].sum().item()), int(ok.sum().item())


def clouds_leg(args, device, cfg, lefts, rights, steps):
    slots, (cols, rows) = args.cloud_slots, CLOUD_SIZE
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    cams = [behind(slam.pose(s), cols, rows) for s in range(slots)]
    style = hip_lib.scene_style(cols=cols, rows=rows, pixel="rgba8")
    pitch, image_bytes = hip_lib.scene_size(style)
    dst = torch.empty(slots * image_bytes, dtype=torch.uint8, device=device)
    offsets = [i * image_bytes for i in range(slots)]
    h = hip_lib.Handle(device.index, 1024)
    empty = h.pack_scene([(cols, rows, [], None)] * slots, cams, offsets)
    out = {"slots": slots, "picture": [cols, rows], "point_size": args.cloud_point_size, "atomic_rate_bytes_per_s": ATOMIC_RATE,
           "warmup_steps": args.warmup, "steps": {}}
    no_spans = h.pack_scene_spans([[] for _ in range(slots)])
    ms, all_ms = event_ms(lambda: h.render_scene_clouds_packed(empty, no_spans, style, args.cloud_point_size, dst), args.repeats)
    out["tiles_only"] = {"call_ms": ms, "call_ms_all": all_ms}
    plain = slam.submit_scenes(camera=cams, device=True, style=style).wait()
    out["job_without_layer"] = dict(zip(("job_ms", "job_ms_all"), median_ms(device, lambda: plain.submit().wait(), args.repeats)))
    for step in steps:
        cloud = slam.export_cloud("frames", None, step=step, layout="organized", device=True)
        per = cloud.points_per_slot
        rec = cloud.points_buffer.view(torch.int32).reshape(-1, 4)
        spans = h.pack_scene_spans([[(cloud.points_buffer[i * per:].data_ptr(), per)] for i in range(slots)])
        call = lambda: h.render_scene_clouds_packed(empty, spans, style, args.cloud_point_size, dst)
        call()
        ms, all_ms = event_ms(call, args.repeats)
        keys = drawn = 0
        for i in range(slots):
            k, d = offered_keys(rec[i * per:(i + 1) * per], cams[i], cols, rows, args.cloud_point_size)
            keys, drawn = keys + k, drawn + d
        leg = {"records": slots * per, "records_per_slot": per, "kept": int(cloud.segments["n_points"].sum()), "drawn": drawn, "keys_offered": keys,
               "call_ms": ms, "call_ms_all": all_ms, "records_per_s": slots * per / (ms * 1e-3), "atomic_bytes_per_s": 8 * keys / (ms * 1e-3),
               "fraction_of_atomic_rate": 8 * keys / (ms * 1e-3) / ATOMIC_RATE, "pieces": slots * ((per + 1023) // 1024),
               "tiles": slots * ((cols + 63) // 64) * ((rows + 15) // 16)}
        # the form the splat pass replaces: every tile walks the kept records as one keyframe set of its image
        sets, keep = [], []
        for i in range(slots):
            r = rec[i * per:(i + 1) * per]
            r = r[((r[:, 3] >> 24) & 0x80) == 0]
            z = torch.zeros(len(r), dtype=torch.int32, device=device)
            planes = {"kps3d": r[:, :3].contiguous(), "flags": z, "keyframe_id": z, "inlier_count": z, "color": (r[:, 3] & 0xffffff).contiguous()}
            keep.append(planes)
            sets.append((cols, rows, [(len(r), 0, planes)], None))
        walked = h.pack_scene(sets, cams, offsets)
        wstyle = hip_lib.scene_style(cols=cols, rows=rows, pixel="rgba8", point_size=args.cloud_point_size)
        h.render_scene_packed(walked, wstyle, dst)
        wms, wall = event_ms(lambda: h.render_scene_packed(walked, wstyle, dst), max(3, args.repeats // 3))
        leg["walked_by_every_tile"] = {"call_ms": wms, "call_ms_all": wall, "projections": leg["kept"] * ((cols + 63) // 64) * ((rows + 15) // 16)}
        # the pile: one slot's record count on one pixel of one image, distinct depths
        pile = torch.zeros((per, 4), dtype=torch.float32, device=device)
        pile[:, 2] = 1.0 + torch.arange(per, device=device, dtype=torch.float32) / (2.0 * per)
        pile = pile[torch.randperm(per, device=device)].contiguous()
        eye = hip_lib.scene_look_at((0, 0, 0), (0, 0, 1), (0, -1, 0), 60.0, cols, rows, 0.05)
        one = h.pack_scene([(cols, rows, [], None)], [eye], [0])
        pile_spans = h.pack_scene_spans([[(pile.data_ptr(), per)]])
        pcall = lambda: h.render_scene_clouds_packed(one, pile_spans, style, 1, dst)
        pcall()
        pms, pall = event_ms(pcall, args.repeats)
        ems, eall = event_ms(lambda: h.render_scene_clouds_packed(one, h.pack_scene_spans([[]]), style, 1, dst), args.repeats)
        leg["pile"] = {"records": per, "call_ms": pms, "call_ms_all": pall, "one_image_without_spans_ms": ems}
        # the job: the cloud job alone, and the scene job with the layer
        leg["cloud_job"] = dict(zip(("job_ms", "job_ms_all"), median_ms(device, lambda: cloud.submit().wait(), args.repeats)))
        sc = slam.submit_scenes(camera=cams, device=True, style=style, dense=dict(what="frames", step=step, point_size=args.cloud_point_size)).wait()
        leg["job_with_layer"] = dict(zip(("job_ms", "job_ms_all"), median_ms(device, lambda: sc.submit().wait(), args.repeats)))
        leg["live_points"] = int(sc.cloud_info["live_points"].sum())
        out["steps"][str(step)] = leg
        print(json.dumps({str(step): leg}), file=sys.stderr, flush=True)
        del cloud, sc, keep, walked
    h.close()
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def sgm_leg(args, device, cfg, lefts, rights, steps):
    slots, (cols, rows) = args.cloud_slots, CLOUD_SIZE
    n = min(slots, len(lefts))
    slam, packed = start(cfg, lefts[:n], rights[:n], slots, 1, device, args.warmup)
    for pk in packed:
        slam.submit_packed(pk)
    slam.wait()
    cams = [behind(slam.pose(s), cols, rows) for s in range(slots)]
    style = hip_lib.scene_style(cols=cols, rows=rows, pixel="rgba8")
    out = {"slots": slots, "picture": [cols, rows], "point_size": args.cloud_point_size, "lr": args.lr, "sgm": args.sgm, "steps": {}}
    for step in steps:
        jobs = {}
        for name, how in (("wta", dict()), ("wta_checked", dict(lr_check=args.lr)), ("sgm", dict(sgm=job_ab.sgm_dict(args.sgm, None))),
                          ("sgm_checked", dict(sgm=job_ab.sgm_dict(args.sgm, args.lr)))):
            jobs[name] = slam.submit_scenes(camera=cams, device=True, style=style,
                                            dense=dict(what="frames", step=step, point_size=args.cloud_point_size, **how)).wait()
        timed = job_ab.alternate_jobs(device, jobs, args.repeats)
        out["steps"][str(step)] = {"live_points": {k: int(j.cloud_info["live_points"].sum()) for k, j in jobs.items()}, "jobs": timed,
                                   "ratios": job_ab.ratios(timed, [("sgm", "wta"), ("sgm_checked", "wta_checked")])}
        print(json.dumps({str(step): out["steps"][str(step)]}), file=sys.stderr, flush=True)
        del jobs
    out["device_GB"] = slam.memory().device_bytes / 1e9
    slam.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sgm", metavar="P1,P2[,CAP]", default=None,
                    help="--clouds: only the job with the live layer under SGM against winner-takes-all (profiles/sgm_consumers_bench.json)")
    ap.add_argument("--lr", type=float, default=1.0, help="--sgm: the tolerance of the checked legs")
    ap.add_argument("--clouds", default=None, metavar="STEPS", help="measure the cloud points at these lattice steps (e.g. 1,2,4) and nothing else")
    ap.add_argument("--cloud-slots", type=int, default=16)
    ap.add_argument("--cloud-point-size", type=int, default=2)
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
    if args.clouds:
        n_loops = min(args.cloud_slots, args.loops)
    cfg, lefts, rights = bench.render_loops("euroc", list(range(n_loops)), args.loop_frames, device)
    if args.sgm and not args.clouds:
        ap.error("--sgm needs --clouds STEPS")
    if args.clouds and args.sgm:
        leg = dict(sgm_leg(args, device, cfg, lefts, rights, [int(x) for x in args.clouds.split(",")]), tool="tools/scene_bench.py",
                   command=" ".join(sys.argv), device=torch.cuda.get_device_name(0))
        job_ab.merge_result(args.out or os.path.join(ROOT, "profiles", "sgm_consumers_bench.json"), "scene", leg)
        print(json.dumps(leg), flush=True)
        return
    if args.clouds:
        out = {"metric": "scene_cloud_bench", "config": "euroc", "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]),
               "clouds": clouds_leg(args, device, cfg, lefts, rights, [int(x) for x in args.clouds.split(",")])}
        text = json.dumps(out)
        path = args.out or os.path.join(ROOT, "profiles", "scene_cloud_bench.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
        print(text, flush=True)
        return
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
