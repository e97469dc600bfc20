"""Mixed job queues (queue_cases.py) played in three groups against a lock-step twin, the numpy statements and the
oracle. Three links per schedule, none with a tolerance:

1. twin against the oracle: after every frame set (and load) every fed slot's frame, pose, stats and GN trace equal
   oracle_py.Slam's on the modelled history (a restart or a new rig: a fresh Slam with that camera; pose updates are
   followed with update_pose; a load: the saved slot's history), the retired count too;
2. twin against the statements: after every job the delivered buffers equal the numpy statement of that kind computed
   from the twin's getters after the drain (the helpers of the per-feature tests);
3. pipelined against the twin: every delivered buffer byte for byte (the bytes between images and behind the used
   prefix too: every destination is pre-filled), and after the last wait the getters of both ctxs; a snapshot saved on the
   way continues in a fresh one-slot ctx with the oracle's next frame.

Measured on an MI355X (s): see DESIGN.md, section 2."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import ar_ref as AR
import cloud_ref as CR
import export_ref as ER
import map_ref as MR
import oracle_py as O
import queue_cases as Q
import queue_player as P
import scene_ref as SR
import snapshot_ref as SNR
import test_ar_gpu as TA
import test_dense_gpu as TD
import test_export_gpu as TE
import test_map_gpu as TM
import test_trim_gpu as TT
import test_view_gpu as TV
import util
import view_ref as VR
from stereo_svo_slam_amd import hip_lib, synth
from test_dense_cpu import oracle_plane

pytestmark = pytest.mark.gpu

F = np.float32
PV = np.full(6, 1000.0, F)
SV = np.array([100.0, 100.0, 100.0, 0.1, 0.1, 0.1], F)
assert all(np.array_equal(a, b) for m, n in zip(P.AR_MESHES, TA.MESHES) for a, b in zip(m, n)), "test_ar_gpu's meshes"


class World:
    """The frames of the three scenes (device and host), and the oracle on every history a schedule's model reaches:
    cache[history] is what the history's last event gave — a frame: (keyframe made, kps2d, kps3d, info, pose, stats,
    (lo, hi) of the retired count, keyframes); pose updates: the filtered poses [n, 6].
    The retired count: a step retires the keyframes below the smallest origin id of the keypoints that its compaction
    keeps at its start (svo_group_step.hip), never the newest. Those keypoints lie between the previous frame's and
    this frame's, so the count lies between the smallest origin id of the previous frame (lo) and of this one (hi)."""

    def __init__(self):
        self.cfg = cfg = dict(synth.CONFIGS["tiny"])
        n = Q.N_FRAMES
        poses = np.zeros((n, 6), F)
        poses[:, 4] = 0.03 * np.arange(n)
        self.L, self.R = [], []
        for seed in range(Q.N_SCENES):
            scene = synth.Scene(seed, "cuda")
            seeds = 7919 * (seed + 1) + 2 * np.arange(n)
            self.L.append(synth.render_frames_gpu(scene, cfg, poses, False, 1.0, seeds))
            self.R.append(synth.render_frames_gpu(scene, cfg, poses, True, 1.0, seeds + 1))
        torch.cuda.synchronize()
        self.Lh = [x.cpu().numpy() for x in self.L]
        self.Rh = [x.cpu().numpy() for x in self.R]
        self.cache = {}
        self.seconds = 0.0

    @property
    def frames(self):
        return self.cfg, self.L, self.R

    def _run(self, history):
        ref = O.Slam(util.oracle_camera(P.rig_cfg(self.cfg, history[0][1])))
        out = {}
        before = retired = keyframes = 0
        for i, e in enumerate(history[1:]):
            if e[0] == "f":
                _, sc, k = e
                made = ref.new_image(self.Lh[sc][k], self.Rh[sc][k], k / 20.0)
                k2, k3, info = ref.keypoints()
                keyframes += int(made)
                before = retired
                if len(info):
                    retired = max(retired, min(int(info["keyframe_id"].min()), keyframes - 1))
                out[history[:i + 2]] = (made, k2, k3, info, ref.pose().copy(), ref.stats(), (before, retired), keyframes)
            else:
                _, seed, slot, n = e
                pose = ref.pose().astype(F)
                filtered = []
                for g in Q.gyro_rates(seed, slot, n):
                    speed = np.zeros(6, F)
                    speed[3:] = (g.astype(np.float64) / 180.0 * np.pi).astype(F)
                    pose = ref.update_pose(pose, speed, PV, SV, Q.POSE_DT)
                    filtered.append(np.array(pose, F))
                out[history[:i + 2]] = np.array(filtered, F).reshape(-1, 6)
        ref.close()
        return out

    def prepare(self, histories):
        """the oracle on every history not seen yet: the maximal ones run, in a thread pool"""
        t0 = time.perf_counter()
        todo = sorted({h for h in histories if len(h) > 1 and h not in self.cache}, key=len, reverse=True)
        runs = []
        for h in todo:
            if not any(r[:len(h)] == h for r in runs):
                runs.append(h)
        with ThreadPoolExecutor(12) as ex:
            for out in ex.map(self._run, runs):
                self.cache.update(out)
        self.seconds += time.perf_counter() - t0
        return len(runs)

    def last_frame(self, history):
        """the newest frame event's result and the event"""
        for i in range(len(history), 1, -1):
            if history[i - 1][0] == "f":
                return self.cache[history[:i]], history[i - 1]
        return None, None

    def keyframes(self, history):
        res, _ = self.last_frame(history)
        return 0 if res is None else res[7]

    def newest_keyframe_event(self, history):
        for i in range(len(history), 1, -1):
            if history[i - 1][0] == "f" and self.cache[history[:i]][0]:
                return history[i - 1]
        return None


@pytest.fixture(scope="module")
def world():
    w = World()
    # what the schedules rely on, read from the oracle: by the end of the longest run of a schedule (the prologue of
    # 60 and the 12 steps of trim_window; the circuit's runs are as long) at least two keyframes of scenes 0 and 1 have
    # retired, and one of them retires within trim_window's steps
    for scene in (0, 1):
        h = (("cam", 0),) + tuple(("f", scene, k) for k in range(72))
        w.prepare([h])
        retired = [w.cache[h[:k + 2]][6][0] for k in range(72)]
        print(f"scene {scene}: keyframes {w.cache[h][7]}, retired per frame {retired[::6]}")
        assert retired[-1] >= 2, (scene, retired)
    return w


def retire_steps(w, scene, lo, hi):
    """the frames in [lo, hi) at which a keyframe of the scene's plain run may retire: where the oracle's smallest
    origin id rises, and the frame after it"""
    h = (("cam", 0),) + tuple(("f", scene, k) for k in range(hi))
    w.prepare([h])
    r = [w.cache[h[:k + 2]][6][1] for k in range(hi)]
    rises = {k for k in range(1, hi) if r[k] > r[k - 1]}
    return {k for k in range(lo, hi) if k in rises or k - 1 in rises}


# ------------------------------------------------------------------------------------------ link 1: the oracle

def check_frame(w, tag, batch, slot, st):
    """the slot's current frame against the oracle on the state's history"""
    res, event = w.last_frame(st.history)
    made, k2, k3, info, pose, ost, retired, keyframes = res
    got = batch.stats(slot)
    assert got.frame_id == st.frame == event[2], (tag, got.frame_id, st.frame)
    f = batch.get_frame(slot)
    util.compare_frame(tag, f, k2, k3, info, pose, 0.0)
    assert np.array_equal(f.info["color"], info["color"]), f"{tag}: colours"
    if st.history[-1][0] == "f":                      # (pose updates leave the stats alone)
        assert got.is_keyframe == made, f"{tag}: keyframe decision"
    if st.frame > 0:
        assert util.same_trace(got, ost, w.cfg), f"{tag}: GN trace differs from the oracle's"
    r = batch.keyframe_range(slot)
    assert retired[0] <= r.retired <= retired[1] and r.count == keyframes and r.first >= st.floor, \
        (tag, (r.first, r.retired, r.count), retired, keyframes)


# ----------------------------------------------------------------------------------- link 2: the statements

def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _unfed(tag, seg, s, st, none):
    assert (int(seg["seq"]), int(seg["run"]), int(seg["frame_id"]), int(seg["status"])) == (s, st.run, -1, none), tag


class Statements:
    """on_op of the twin: every delivered job against its statement, every frame set against the oracle"""

    def __init__(self, w, batch, schedule):
        self.w, self.batch, self.schedule = w, batch, schedule
        self.first = [0] * Q.N_SLOTS
        self.checked = {}
        self.trimmed = dict(frames=0, trim=0)             # keyframes that a step's window, and a trim job, dropped

    def __call__(self, i, op, job, state, before):
        b, kind = self.batch, op.kind
        tag = f"{self.schedule.name} op {i} {kind}"
        if kind in ("frames", "load"):
            for s in op.named():
                if state[s].fed:
                    check_frame(self.w, f"{tag} slot {s}", b, s, state[s])
        elif kind in ("restart", "rig"):
            for s in op.slots:
                assert b.get_trajectory(s).shape == (0, 6) and len(b.finished_runs(s)) == state[s].finished, tag
                r = b.keyframe_range(s)
                assert (r.first, r.retired, r.count) == (0, 0, 0), tag
                if kind == "rig":
                    assert bytes(b.slot_rig(s)[1]) == bytes(hip_lib.CameraSettings.from_dict(P.rig_cfg(self.w.cfg, state[s].rig))), tag
        elif kind == "trim":
            below = op.p["below"] or [2 ** 31 - 1] * len(op.slots)
            for s, lim in zip(op.slots, below):
                r = b.keyframe_range(s)
                assert r.first == max(self.first[s], min(lim, r.retired)), (tag, s, r.first, self.first[s], lim, r.retired)
        elif kind == "pose":
            at = 0
            for s, n in zip(op.slots, op.p["counts"]):
                want = self.w.cache[state[s].history]
                assert np.array_equal(job[at:at + n].view(np.uint32), want.view(np.uint32)), (tag, s)
                at += n
        elif kind in Q.EXPORT_KINDS + ("save",):
            getattr(self, kind)(tag, op, job, state)
        self.checked[kind] = self.checked.get(kind, 0) + 1
        for s in range(Q.N_SLOTS):
            first = b.keyframe_range(s).first
            if first > self.first[s]:
                assert kind in self.trimmed or (kind == "load" and s in op.slots), (tag, s)
                self.trimmed[kind] = self.trimmed.get(kind, 0) + first - self.first[s]
            self.first[s] = first
            assert first >= state[s].floor

    def export(self, tag, op, job, state):
        b, slots = self.batch, list(op.slots)
        got = TE._getter_state(b, slots)
        if op.p["what"] == "frames":
            TE._check_frames(tag, job, got, slots, {s: (state[s].run, state[s].time_stamp if state[s].fed else None) for s in slots})
        else:
            TE._check_keyframes(tag, job, got, slots)
            assert [int(x) for x in job.segments["run"]] == [state[s].run for s in slots], tag
        TE._check_placement(job, b, slots)

    def map(self, tag, op, job, state):
        filt = dict(drop_flags=0, own_only=op.p["own_only"], min_inliers=0)
        for i, s in enumerate(op.slots):
            seg = job.segments[i]
            assert int(seg["run"]) == state[s].run, (tag, s)
            if state[s].fed:
                self._map_slot(tag, job, i, s, filt)
            else:
                assert (int(seg["frame_id"]), int(seg["n_keyframes"]), int(seg["n_exported"]), int(seg["n_points"]), int(seg["points_bound"]),
                        int(seg["status"])) == (-1, 0, 0, 0, 0, hip_lib.MAP_COMPLETE), (tag, s)

    def _map_slot(self, tag, m, i, s, filt):
        """test_map_gpu._check_slot for a slot whose oldest keyframes may be trimmed: the export starts at the first
        resident keyframe and the segment says which that is"""
        b = self.batch
        seg, r = m.segments[i], m.regions[i]
        first = b.keyframe_range(s).first
        sets, meta = TM._getter_sets(b, s, first)
        assert int(seg["seq"]) == s and int(seg["status"]) == hip_lib.MAP_COMPLETE, (tag, s)
        assert int(seg["n_keyframes"]) == b.num_keyframes(s) and int(seg["from_keyframe"]) == first == m.first_keyframe(i), (tag, s)
        assert int(seg["n_exported"]) == len(sets) >= 1 and not np.any(seg["_pad"][1:]), (tag, s)
        assert int(seg["frame_id"]) == b.stats(s).frame_id and int(seg["keyframes_retired"]) == b.keyframe_range(s).retired, (tag, s)
        bound = sum(n for n, *_ in sets)
        assert int(seg["points_bound"]) == bound, (tag, s)
        want, counts = MR.pack([sets], [0], filt, bound)
        assert int(seg["n_points"]) == sum(counts), (tag, s)
        assert m.points(i).tobytes() == want[:sum(counts)].tobytes(), (tag, s)
        kfs = m.keyframes(i)
        assert len(kfs) == len(sets)
        at = 0
        for j, (k, n_total, pose) in enumerate(meta):
            e = kfs[j]
            assert (int(e["id"]), int(e["n_total"]), int(e["n"]), int(e["_pad"])) == (k, n_total, counts[j], 0), (tag, s, k)
            assert int(e["first"]) == int(r["first_point"]) + at and e["pose"].tobytes() == pose, (tag, s, k)
            at += counts[j]

    def _image_of(self, what, st):
        """(left, right) input images of the frame, or of the frame that made the newest keyframe"""
        event = self.w.last_frame(st.history)[1] if what == hip_lib.EXPORT_FRAMES else self.w.newest_keyframe_event(st.history)
        return self.w.Lh[event[1]][event[2]], self.w.Rh[event[1]][event[2]]

    def views(self, tag, op, job, state):
        b, style = self.batch, job.style
        for i, s in enumerate(op.slots):
            seg, st = job.segments[i], state[s]
            TV._check_segment((tag, s), seg, b, job.what, s)
            assert int(seg["run"]) == st.run and int(seg["offset"]) == i * job.image_bytes, (tag, s)
            if not st.fed:
                assert int(seg["status"]) == hip_lib.VIEW_NONE and job.image(i) is None, (tag, s)
                continue
            gray = TV._chain(self._image_of(job.what, st)[0], style.level + 1)[style.level]
            f = b.get_frame(s) if job.what == hip_lib.EXPORT_FRAMES else b.get_keyframe(None, s)
            flags, types, colors = VR.info_arrays(f.info)
            want = VR.render(gray, style.pixel, f.kps2d if style.markers else None, flags, types, colors, style.level, style.drop_flags,
                             style.size, style.size_temporary)
            got = _np(job.image(i))
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, s)

    def disparity(self, tag, op, job, state):
        for i, s in enumerate(op.slots):
            if state[s].fed:
                TD._check_slot(tag, job, i, s, self.batch, job.what)
                assert F(job.segments[i]["baseline"]) == F(P.rig_cfg(self.w.cfg, state[s].rig)["baseline"]), (tag, s)
                left, right = self._image_of(job.what, state[s])        # (the planes the helper read are the input's)
                l, r, _ = TD._planes_of(self.batch, job.what, s)
                assert np.array_equal(l, left) and np.array_equal(r, right), (tag, s)
            else:
                _unfed((tag, s), job.segments[i], s, state[s], hip_lib.DISPARITY_NONE)

    def cloud(self, tag, op, job, state):
        b, st = self.batch, job.style
        pps = job.points_per_slot
        for i, s in enumerate(op.slots):
            seg = job.segments[i]
            raw = _np(job.points_buffer[i * pps:(i + 1) * pps])
            assert int(seg["first_point"]) == i * pps, (tag, s)
            if not state[s].fed:
                _unfed((tag, s), seg, s, state[s], hip_lib.CLOUD_NONE)
                assert int(seg["n_points"]) == 0 and (raw == P.FILL).all(), (tag, s)
                continue
            left, right = self._image_of(job.what, state[s])
            cam = b.slot_rig(s)[1]
            view = b.export_views(job.what, [s], plane="left", level=0, pixel="gray8")
            vseg = view.segments[0]
            assert np.array_equal(view.image(0), left), (tag, s)
            assert (int(seg["seq"]), int(seg["run"]), int(seg["status"])) == (s, state[s].run, hip_lib.CLOUD_OK), (tag, s)
            assert (int(seg["frame_id"]), int(seg["keyframe_id"])) == (int(vseg["frame_id"]), int(vseg["keyframe_id"])), (tag, s)
            assert seg["pose"].tobytes() == vseg["pose"].tobytes() and F(seg["time_stamp"]) == F(vseg["time_stamp"]), (tag, s)
            assert F(seg["baseline"]) == F(cam.baseline) == F(P.rig_cfg(self.w.cfg, state[s].rig)["baseline"]), (tag, s)
            win = cam.window_size_depth_calculator
            disp = oracle_plane(np.ascontiguousarray(left), np.ascontiguousarray(right), win, cam.search_x, cam.search_y, st.step)
            rig = {k: getattr(cam, k) for k in CR.RIG_KEYS}
            ref, n = CR.cloud(left, np.stack([disp, np.zeros_like(disp)]), win, st.step, rig, seg["pose"], st.frame, st.layout,
                              st.min_disparity, st.max_depth, 0.0)
            assert int(seg["n_points"]) == n, (tag, s, int(seg["n_points"]), n)
            if st.layout == CR.ORGANIZED:
                assert raw.tobytes() == ref.tobytes(), (tag, s)
            else:
                assert raw[:n].tobytes() == ref.tobytes() and (raw[n:] == P.FILL).all(), (tag, s)

    def scenes(self, tag, op, job, state):
        b, style = self.batch, job.style
        for i, s in enumerate(op.slots):
            seg = job.segments[i]
            assert int(seg["offset"]) == i * job.image_bytes, (tag, s)
            if not state[s].fed:
                _unfed((tag, s), seg, s, state[s], hip_lib.SCENE_NONE)
                assert job.image(i) is None and (_np(job.pixels[i * job.image_bytes:(i + 1) * job.image_bytes]) == P.FILL).all(), (tag, s)
                continue
            first, _, count, _ = TT._range(b, s)
            sets, poses = TT._getter_sets(b, s, first)
            lines, n_poses = SR.slot_lines(b.get_trajectory(s), poses, b.pose(s), style.show, style.trajectory_rgb, style.keyframe_rgb,
                                           style.pose_rgb, (style.frustum_w, style.frustum_h, style.frustum_d), style.trajectory_tail)
            want = SR.render(Q.SCENE_COLS, Q.SCENE_ROWS, style.pixel, np.frombuffer(bytes(job._cams[i]), F), sets, lines, MR.KEEP_ALL,
                             style.point_size, style.background)
            assert (int(seg["seq"]), int(seg["run"]), int(seg["status"]), int(seg["frame_id"])) == (s, state[s].run, hip_lib.SCENE_OK, state[s].frame), (tag, s)
            assert (int(seg["n_keyframes"]), int(seg["from_keyframe"]), int(seg["n_keypoints"]), int(seg["n_poses"])) == \
                   (count, 0, sum(n for n, *_ in sets), n_poses), (tag, s)
            assert seg["pose"].tobytes() == b.pose(s).tobytes(), (tag, s)
            assert _np(job.image(i)).tobytes() == want.tobytes(), (tag, s)

    def ar(self, tag, op, job, state):
        b, st = self.batch, job.style
        for i, s in enumerate(op.slots):
            seg = job.segments[i]
            assert int(seg["offset"]) == i * job.image_bytes, (tag, s)
            if not state[s].fed:
                _unfed((tag, s), seg, s, state[s], hip_lib.AR_NONE)
                assert job.image(i) is None, (tag, s)
                continue
            cam, pose = b.slot_rig(s)[1], b.pose(s)
            rc = P.rig_cfg(self.w.cfg, state[s].rig)
            assert (F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)) == (F(rc["fx"]), F(rc["fy"]), F(rc["cx"]), F(rc["cy"])), (tag, s)
            gray = self._image_of(hip_lib.EXPORT_FRAMES, state[s])[0]
            draws = [(np.asarray(m, F), P.AR_MESHES[k][0], P.AR_MESHES[k][1], P.AR_MESHES[k][2] if len(P.AR_MESHES[k]) > 2 else None, rgb)
                     for m, k, rgb in P.AR_INSTANCES]
            want = AR.render(gray, AR.camera_of_pose(pose, cam.fx, cam.fy, cam.cx, cam.cy), draws, tuple(st.light), st.ambient, st.near, st.pixel)
            assert (int(seg["seq"]), int(seg["run"]), int(seg["status"]), int(seg["frame_id"])) == (s, state[s].run, hip_lib.AR_OK, state[s].frame), (tag, s)
            assert (int(seg["n_instances"]), int(seg["n_triangles"])) == (2, 24) and seg["pose"].tobytes() == pose.tobytes(), (tag, s)
            assert _np(job.image(i)).tobytes() == want.tobytes(), (tag, s)

    def save(self, tag, op, job, state):
        b = self.batch
        for sn, s in zip(job, op.slots):
            st, info = state[s], sn.info
            assert info.status == hip_lib.SNAPSHOT_COMPLETE, (tag, s, info.host_bytes, info.data_bytes, sn.host.size)
            ref = _parse_snapshot(sn.host[:info.host_bytes])
            assert ref["first_keyframe"] == info.first_keyframe, (tag, s)
            r = b.keyframe_range(s)
            assert (ref["frame_id"], ref["n_trajectory"], ref["n_keyframes"], ref["keyframes_retired"]) == \
                   (st.frame, st.frame + 1 if st.fed else 0, r.count, r.retired), (tag, s)
            assert info.first_keyframe == r.first, (tag, s)
            assert np.array_equal(ref["trajectory"], b.get_trajectory(s)) and ref["pose"].tobytes() == b.pose(s).tobytes(), (tag, s)
            rc = P.rig_cfg(self.w.cfg, st.rig)
            assert all(F(ref[k]) == F(rc[k]) for k in SNR.CAM_FLOATS), (tag, s)
            if st.fed:
                n_kps = len(b.get_frame(s).kps2d)
                assert ref["n_keypoints"] == n_kps, (tag, s)
                kf_ns = [n for _, n, _ in ref["keyframes"]]
                assert kf_ns == [len(b.get_keyframe(k, s).kps2d) for k in range(r.first, r.count)], (tag, s)
                if not sn.device_mode:                    # the current frame's planes in the data part are the input images
                    left, right = self._image_of(hip_lib.EXPORT_FRAMES, st)
                    base = 14 + 12 * len(ref["keyframes"])           # image set 0: the current frame's
                    planes = [sn.data[off:off + rows * row_bytes].reshape(rows, row_bytes)
                              for off, row_bytes, rows in (ref["directory"][base], ref["directory"][base + ref["pyramid_levels"]])]
                    assert np.array_equal(planes[0], left) and np.array_equal(planes[1], right), (tag, s)


def _parse_snapshot(part):
    """snapshot_ref.parse for a slot whose oldest keyframes may be trimmed: the header's last count is the id of the
    first resident keyframe, and only the resident ones have entries and planes"""
    part = bytes(part)
    out = dict(zip(SNR.HEADER_FIELDS, SNR.HEADER.unpack_from(part, 0)))
    out["first_keyframe"] = out["_reserved"]
    p = SNR.HEADER.size + SNR.FILTER_BYTES
    out["pose"] = np.frombuffer(part, "<f4", 6, p + 8)
    p += SNR.FRAME_BYTES
    out["trajectory"] = np.frombuffer(part, "<f4", 6 * out["n_trajectory"], p).reshape(-1, 6)
    p += SNR.POSE.size * out["n_trajectory"]
    out["keyframes"] = []
    for _ in range(out["n_keyframes"] - out["first_keyframe"]):
        v = SNR.KEYFRAME.unpack_from(part, p)
        out["keyframes"].append((np.array(v[:6], F), v[6], v[7]))
        p += SNR.KEYFRAME.size
    out["directory"] = [SNR.PLANE.unpack_from(part, p + SNR.PLANE.size * i) for i in range(out["n_planes"])]
    assert p + SNR.PLANE.size * out["n_planes"] == out["host_bytes"] == len(part)
    return out


# ---------------------------------------------------------------------------------- link 3: pipelined == twin

def _slot_state(batch, s):
    f = batch.get_frame(s)
    r = batch.keyframe_range(s)
    kfs = [batch.get_keyframe(k, s) for k in range(r.first, r.count)]
    return dict(pose=batch.pose(s).tobytes(), stats=bytes(batch.stats(s)), trajectory=batch.get_trajectory(s).tobytes(),
                frame=(f.pose.tobytes(), f.kps2d.tobytes(), f.kps3d.tobytes(), f.info.tobytes()),
                keyframes=[(k.pose.tobytes(), k.kps2d.tobytes(), k.kps3d.tobytes(), k.info.tobytes()) for k in kfs],
                range=(r.first, r.retired, r.count, r.table), rig=bytes(batch.slot_rig(s)[1]),
                runs=[(bytes(info)[4:], traj.tobytes()) for info, traj in batch.finished_runs(s)])


def _in_use(batch):
    m = batch.memory()
    return m.keyframe_slabs - m.keyframe_slabs_free, m.image_sets - m.image_sets_free


def run_schedule(w, schedule):
    t = {}
    t0 = time.perf_counter()
    model = Q.run_model(schedule)
    histories = {st.history for _, slots in model.log for st in slots}
    # the snapshot that goes on in a fresh ctx: the last one saved of a fed slot; the oracle gets its next frame too
    resume = None
    for name, st in model.snaps.items():
        if st.fed and st.frame + 1 < Q.N_FRAMES:
            resume = (name, st, st.history + (("f", st.scene, st.frame + 1),))
    if resume:
        histories.add(resume[2])
    t["oracle runs"] = w.prepare(histories)
    t["oracle"] = time.perf_counter() - t0
    keyframes_of = lambda st: w.keyframes(st.history)

    t0 = time.perf_counter()
    twin, rigs = P.make_batch(w.cfg, "twin", schedule.window)
    check = Statements(w, twin, schedule)
    want, twin_snaps, _ = P.play(twin, rigs, schedule, w.frames, "twin", check, keyframes_of)
    t["twin and statements"] = time.perf_counter() - t0
    kinds = {op.kind for op in schedule.ops if op.kind in Q.KINDS}
    assert set(check.checked) >= kinds, kinds - set(check.checked)

    t0 = time.perf_counter()
    batch, rigs = P.make_batch(w.cfg, "pipelined", schedule.window)
    got, snaps, _ = P.play(batch, rigs, schedule, w.frames, "pipelined", None, keyframes_of)
    t["pipelined"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    assert len(got) == len(want) == len(schedule.ops)
    n_bytes = 0
    for i, (g, x) in enumerate(zip(got, want)):
        assert (g is None) == (x is None), i
        if g is None:
            continue
        assert g.buffers.keys() == x.buffers.keys(), (i, g.op.kind)
        mine, theirs = _export_pair(g.buffers, x.buffers, g.op) if g.op.kind == "export" else (g.buffers, x.buffers)
        for name in mine:
            a, b = mine[name], theirs[name]
            assert a == b, f"{schedule.name} op {i} {g.op.kind} {g.op.slots}: {name} differs from the twin's " \
                           f"({sum(p != q for p, q in zip(a, b))} of {len(a)} bytes)"
            n_bytes += len(a)
    for s in range(Q.N_SLOTS):
        a, b = _slot_state(batch, s), _slot_state(twin, s)
        for key in a:
            assert a[key] == b[key], f"{schedule.name}: slot {s}: {key} differs from the twin's after the last wait"
    assert _in_use(batch) == _in_use(twin)
    if resume:
        name, st, history = resume
        one, rig1 = P.make_batch(P.rig_cfg(w.cfg, st.rig), "twin", None, 1)
        one.load([0], [snaps[name].trimmed()])
        check_frame(w, f"{schedule.name}: {name} in a fresh ctx", one, 0, st)
        k = st.frame + 1
        one.new_images([w.L[st.scene][k]], [w.R[st.scene][k]], [k / 20.0])
        st2 = Q.SlotState(scene=st.scene, frame=k, rig=st.rig, history=history)
        check_frame(w, f"{schedule.name}: {name} goes on", one, 0, st2)
        one.close()
    t["comparison"] = time.perf_counter() - t0
    batch.close()
    twin.close()
    print(f"{schedule.name}: {len(schedule.ops)} ops, {n_bytes} bytes compared, trimmed {check.trimmed}, " + ", ".join(f"{k} {v:.2f}" if isinstance(v, float) else f"{k} {v}" for k, v in t.items()))
    return check


def _export_pair(mine, twins, op):
    """The buffers of an export as three groups delivered them, and the twin's (one group) as three groups deliver
    them: where a slot's records start depends on the groups (export_ref.placement: every group packs its named slots
    from its own base on), so the twin's records move to the three-group placement in buffers that hold FILL
    elsewhere; nothing else changes. Host mode copies a group's used prefix in one piece, so the up to 3 padding
    records between two segments of one group receive unspecified bytes (svo_hip.h): those, and only those, are set to
    FILL on both sides."""
    seg = np.frombuffer(twins["segments"], hip_lib.EXPORT_SEGMENT_DTYPE).copy()
    per_slot = ER.capacity(synth.CONFIGS["tiny"])
    groups = ER.group_ranges(Q.N_SLOTS, Q.N_GROUPS)
    first = ER.placement(list(op.slots), [int(n) for n in seg["n"]], groups, per_slot)
    padding = []
    if not op.p["device"]:
        for lo, count in groups:
            at = None
            for i, s in enumerate(op.slots):
                if lo <= s < lo + count:
                    if at is not None:
                        padding.append((at, first[i]))
                    at = first[i] + int(seg["n"][i])
    a, b = dict(mine), {}
    for name, width in (("kps2d", ER.KP2D_BYTES), ("kps3d", ER.KP3D_BYTES), ("info", ER.INFO_BYTES)):
        old = np.frombuffer(twins[name], np.uint8).reshape(-1, width)
        new = np.full_like(old, P.FILL)
        for e, f in zip(seg, first):
            new[f:f + int(e["n"])] = old[int(e["first"]):int(e["first"]) + int(e["n"])]
        got = np.frombuffer(mine[name], np.uint8).reshape(-1, width).copy()
        for lo, hi in padding:
            assert hi - lo < 4
            got[lo:hi] = P.FILL
        a[name], b[name] = got.tobytes(), new.tobytes()
    seg["first"] = first
    b["segments"] = seg.tobytes()
    return a, b


@pytest.mark.parametrize("variant", Q.VARIANTS)
def test_circuit(world, variant):
    check = run_schedule(world, Q.circuit(variant))
    assert check.trimmed["trim"] >= 2, "no trim job of the circuit dropped a keyframe"


@pytest.mark.parametrize("name", [n for n in Q.HAND_WRITTEN if n != "trim_window"])
def test_hand_written(world, name):
    run_schedule(world, Q.HAND_WRITTEN[name]())


def test_trim_window(world):
    """every export kind behind the frame sets at which a keyframe of scene 1 (slot b) or scene 0 (slot d) retires"""
    steps = retire_steps(world, 1, 60, 72) | retire_steps(world, 0, 60, 72)
    assert steps, "no keyframe retires within the steps of trim_window"
    check = run_schedule(world, Q.trim_window(steps))
    assert check.trimmed["frames"] >= 2, "no step trimmed a keyframe by itself"
