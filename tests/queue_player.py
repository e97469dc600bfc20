"""Plays a queue_cases.Schedule on a StereoSlamBatch and returns every delivered buffer in schedule order.

mode "pipelined": three groups, frames through pack_images / submit_packed, every job through its submit form with
every capacity given by the caller; wait() only where the schedule says so. Nothing that drains is called in between
(no per-slot getter, no map_size, no snapshot_size). Device-mode destinations are read after the last wait.
mode "twin": one group, the blocking form of every call; after every op the queue is drained and `on_op(i, op, job,
state)` may look at the ctx with the getters (job: the object that owns the delivered buffers, state: the model's slots
after the op).

Every destination is pre-filled with FILL, so the bytes between images and behind the used prefix are compared too."""
import copy
import os

import numpy as np
import torch

import queue_cases as Q
import snapshot_ref as SNR
from stereo_svo_slam_amd import hip_lib
from stereo_svo_slam_amd.hip_lib import POSE_SAMPLE_CHAIN, POSE_SAMPLE_DTYPE, SvoError
from stereo_svo_slam_amd.stereo_slam import (ArPictures, Clouds, Disparities, Export, MapExport, Scenes, Snapshot,
                                             StereoSlamBatch, Views)

FILL = 0xA5
GROUPS = dict(pipelined=3, twin=1)
F = np.float32
AR_BOX = hip_lib.ar_box(0.2)
AR_MESHES = [AR_BOX, (AR_BOX[0] * F(0.5), AR_BOX[1], np.arange(12, dtype=np.uint32) * 0x0a1408 + 0x202020)]
AR_INSTANCES = [(hip_lib.ar_model(hip_lib.AR_AT), 0, 0xc08040), (hip_lib.ar_model((0.12, -0.05, 0.4)), 1, 0)]


def rig_cfg(cfg, rig):
    return dict(cfg, **Q.RIG) if rig else dict(cfg)


def make_batch(cfg, mode, window=None, n_slots=Q.N_SLOTS):
    """the ctx of a mode: its groups, rig 1 added (its id is returned with it), the keyframe window set"""
    old = os.environ.get("SVO_GROUPS")
    os.environ["SVO_GROUPS"] = str(GROUPS[mode])
    try:
        b = StereoSlamBatch(cfg, cfg["width"], cfg["height"], n_slots)
    finally:
        if old is None:
            del os.environ["SVO_GROUPS"]
        else:
            os.environ["SVO_GROUPS"] = old
    assert b.groups() == GROUPS[mode]
    ids = b.add_rigs([{k: rig_cfg(cfg, 1)[k] for k in hip_lib.RIG_FLOATS}])
    if window is not None:
        b.set_keyframe_window(window)
    return b, {0: 0, 1: ids[0]}


def pose_samples(seed, slot, n):
    """the samples of one slot of a pose op: the app's IMU loop on queue_cases.gyro_rates, all chained"""
    gyro = Q.gyro_rates(seed, slot, n)
    out = np.zeros(n, POSE_SAMPLE_DTYPE)
    out["speed"][:, 3:] = (gyro.astype(np.float64) / 180.0 * np.pi).astype(np.float32)
    out["pose_var"] = 1000.0
    out["speed_var"] = np.array([100.0, 100.0, 100.0, 0.1, 0.1, 0.1], np.float32)
    out["dt"] = Q.POSE_DT
    out["flags"] = POSE_SAMPLE_CHAIN
    return out


def snapshot_bound(cfg, state, keyframes):
    """(host_bytes, data_bytes) that hold a save of a slot in `state` with at most `keyframes` keyframes, through
    snapshot_ref's layout: every keyframe resident with a full keypoint set and an image set of its own"""
    cap = SNR.capacity(cfg)
    _, _, fields = SNR.host_part(cfg, frame_id=max(state.frame, 0), n_keypoints=cap, keyframes=[(cap, i) for i in range(keyframes)],
                                 n_sets=keyframes + 1)
    return fields["host_bytes"], fields["data_bytes"]


def _fill(t):
    if isinstance(t, torch.Tensor):
        t.view(torch.uint8).fill_(FILL)
    else:
        t.view(np.uint8)[...] = FILL


def _bytes(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
    return np.ascontiguousarray(t).tobytes()


class Delivered:
    """what one op delivered: the object that owns the buffers and how to read them as {name: bytes}"""

    def __init__(self, op, job, read):
        self.op, self.job, self._read = op, job, read
        self.buffers = None

    def collect(self):
        if self.buffers is None:
            self.buffers = {k: _bytes(v) for k, v in self._read().items()}
        return self.buffers


def _reject(batch, op):
    """the rejected submit of a "reject" op: the error's text (queues nothing)"""
    what, slots = op.p["how"], list(op.slots)
    try:
        if what == "twice":
            Export(batch, hip_lib.EXPORT_FRAMES, slots + slots[:1], False, ("kps2d",)).submit()
        elif what == "capacity":
            e = Export(batch, hip_lib.EXPORT_FRAMES, slots, False, ("kps2d", "info"))
            e._dst.capacity -= 1
            e.submit()
        elif what == "reserved":
            job = Views(batch, hip_lib.EXPORT_FRAMES, slots, hip_lib.view_style(), False)
            job.style._reserved = 1
            job.submit()
        else:
            raise AssertionError(what)
    except SvoError as err:
        return str(err)
    raise AssertionError(f"the {what} submit was accepted")


REJECT_TEXT = dict(twice="named twice", capacity="capacity", reserved="reserved")


def play(batch, rig_ids, schedule, frames, mode, on_op=None, keyframes_of=None):
    """frames: (cfg, L, R) with L[scene][k], R[scene][k] device images. keyframes_of(state): an upper bound of the
    keyframes of a slot in that model state (default: its frames). Returns [Delivered or None] per op, collected."""
    cfg, L, R = frames
    pipelined = mode == "pipelined"
    keyframes_of = keyframes_of or (lambda st: st.frames_in_run)
    model = Q.Model(schedule.window)
    snaps, keep, out = {}, [], []
    per_slot = batch.export_capacity()
    for i, op in enumerate(schedule.ops):
        before = model.log[-1][1] if model.log else copy.deepcopy(model.slots)
        kind, slots, p = op.kind, list(op.slots), op.p
        what = hip_lib.EXPORT_WHAT.index(p["what"]) if "what" in p else None
        device = bool(p.get("device"))
        d = None
        if kind == "frames":
            ls, rs, ts = [None] * batch.n, [None] * batch.n, [0.0] * batch.n
            for s, sc in zip(slots, p["scenes"]):
                if sc is not None:
                    k = model.next_frame(s)
                    ls[s], rs[s], ts[s] = L[sc][k], R[sc][k], k / 20.0
            packed = batch.pack_images(ls, rs, ts)
            keep.append(packed)
            (batch.submit_packed if pipelined else batch.new_images_packed)(packed)
        elif kind == "restart":
            batch.restart(slots)
        elif kind == "rig":
            batch.assign_rigs(slots, [rig_ids[r] for r in p["rigs"]])
        elif kind == "trim":
            batch.trim_keyframes(slots, None if p["below"] is None else list(p["below"]), wait=not pipelined)
        elif kind == "export":
            job = Export(batch, what, slots, device, ("kps2d", "kps3d", "info"))
            for t in job._bufs.values():
                _fill(t)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, **job._bufs))
        elif kind == "map":
            kfs = [keyframes_of(before[s]) for s in slots]
            job = MapExport(batch, slots, None, dict(own_only=p["own_only"]), device, [k * per_slot for k in kfs], kfs)
            _fill(job.points_buffer)
            _fill(job._kfs)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, keyframes=job._kfs, points=job.points_buffer))
        elif kind == "views":
            job = Views(batch, what, slots, hip_lib.view_style(what, p["plane"], p["level"], p["pixel"], p["markers"]), device)
            _fill(job._buf)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, pixels=job._buf))
        elif kind == "disparity":
            job = Disparities(batch, what, slots, hip_lib.disparity_style(p["value"], p["step"], 0, 0, 0, p["cost"]), device)
            _fill(job._buf)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, values=job._buf))
        elif kind == "cloud":
            style = hip_lib.cloud_style(p["step"], 0, 0, 0, p["frame"], p["layout"], p["min_disparity"], p["max_depth"], 0.0)
            job = Clouds(batch, what, slots, style, device)
            _fill(job.points_buffer)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, points=job.points_buffer))
        elif kind == "scenes":
            style = hip_lib.scene_style(cols=Q.SCENE_COLS, rows=Q.SCENE_ROWS, pixel=p["pixel"], point_size=p["point_size"])
            job = Scenes(batch, slots, style, hip_lib.scene_preset(p["camera"], Q.SCENE_COLS, Q.SCENE_ROWS), device)
            _fill(job._buf)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, pixels=job._buf))
        elif kind == "ar":
            job = ArPictures(batch, slots, hip_lib.ar_style(pixel=p["pixel"]), AR_MESHES, AR_INSTANCES, None, device)
            _fill(job._buf)
            job.submit()
            d = Delivered(op, job, lambda job=job: dict(segments=job.segments, pixels=job._buf))
        elif kind == "save":
            made = [batch.new_snapshot(*snapshot_bound(cfg, before[s], keyframes_of(before[s])), device) for s in slots]
            for sn in made:
                _fill(sn.host)
                _fill(sn.data)
            batch.submit_save(slots, snapshots=made)
            snaps.update(zip(p["snaps"], made))
            d = Delivered(op, made, lambda made=made: {f"{part}{j}": getattr(sn, part) for j, sn in enumerate(made) for part in ("host", "data")})
        elif kind == "load":
            batch.submit_load(slots, [snaps[name].trimmed() for name in p["snaps"]])
        elif kind == "pose":
            filtered = batch.submit_pose_updates(slots, [pose_samples(p["seed"], s, n) for s, n in zip(slots, p["counts"])])
            d = Delivered(op, filtered, lambda filtered=filtered: dict(filtered=filtered))
        elif kind == "wait":
            batch.wait()
        elif kind == "reject":
            text = _reject(batch, op)
            assert REJECT_TEXT[p["how"]] in text, (p["how"], text)
            d = Delivered(op, text, lambda: {})
        else:
            raise AssertionError(kind)
        state = model.apply(op)
        out.append(d)
        if not pipelined:
            batch.wait()
            if d is not None:
                d.collect()
            if on_op is not None:
                on_op(i, op, d.job if d is not None else None, state, before)
    batch.wait()
    for d in out:
        if d is not None:
            d.collect()
    return out, snaps, model
