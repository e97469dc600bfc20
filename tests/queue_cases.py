"""Mixed job queues: schedules of queue entries of different kinds next to each other, and a model that says without a
GPU what every slot holds after every entry. Imports neither the HIP library nor the oracle.

A group's queue carries fourteen kinds of entry (KINDS). An Op is (kind, slots in named order, parameters); two more
kinds are marks of a schedule and no queue entries: "wait" (svo_wait) and "reject" (a submit that must fail and queue
nothing). A Schedule is a list of Ops for a ctx of six slots in three groups (slots 2g, 2g + 1 in group g); Model.apply
follows it.

Workload (test_trim_gpu.py's): `tiny`, three scenes, the steady turn ry = 0.03 k; frame k of scene s has time stamp
k / 20. Rig 0 is the ctx's camera, rig 1 is RIG over it."""
import copy
from dataclasses import dataclass, field

import numpy as np

KINDS = ("frames", "restart", "rig", "trim", "export", "map", "views", "disparity", "cloud", "scenes", "ar", "save",
         "load", "pose")
EXPORT_KINDS = ("export", "map", "views", "disparity", "cloud", "scenes", "ar")
ENDING = ("restart", "rig", "load")                  # these end the named slots' sequences
# the staging block(s) of a kind, "replaced when outgrown" (save and load share one)
BLOCK = dict(export="d_export", map="d_map_points", views="d_view", disparity="d_dense", cloud="d_cloud",
             scenes="d_scene", ar="d_ar, d_ar_rec", save="d_snap", load="d_snap", pose="d_pose")
N_SLOTS, N_GROUPS, N_SCENES = 6, 3, 3
N_FRAMES = 110                                        # frames rendered per scene
RIG = dict(fx=212.0, fy=212.0, cx=151.5, cy=127.25, baseline=23.5)
WIDTH, HEIGHT = 320, 240
SCENE_COLS, SCENE_ROWS = 96, 64
PIXEL_BYTES = dict(gray8=1, rgb8=3, rgba8=4)
POSE_DT = 1.0 / 104.0


def group_of(slot):
    return slot // (N_SLOTS // N_GROUPS)


@dataclass
class Op:
    kind: str
    slots: tuple = ()
    p: dict = field(default_factory=dict)

    def named(self):
        """the slots whose group gets a queue entry from this op (a frame set: the slots that are fed)"""
        if self.kind == "frames":
            return tuple(s for s, sc in zip(self.slots, self.p["scenes"]) if sc is not None)
        return self.slots if self.kind in KINDS else ()


@dataclass
class Schedule:
    name: str
    ops: list
    start: int = 0                                    # ops[start:] is the part the name is about (behind the prologue)
    window: object = None                             # set_keyframe_window of the ctx (None: never set)
    roles: dict = field(default_factory=dict)


def gyro_rates(seed, slot, n):
    """the n gyro rates (degrees per second) of a pose-update op for one slot: float32 [n, 3]"""
    return np.random.default_rng([seed, slot]).normal(0, 2.0, (n, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the model

@dataclass
class SlotState:
    scene: object = None              # the scene the slot plays (None: no sequence)
    frame: int = -1                   # its frame index there (-1: no frame yet)
    run: int = 0                      # ordinal of its current (or next) sequence
    finished: int = 0                 # sequences that ended here
    rig: int = 0
    floor: int = 0                    # keyframe_range().first >= floor (a lower bound: what explicit trims cannot undo)
    trims: int = 0                    # trims the run has received
    loaded_from: object = None        # the snapshot its run came from
    samples: int = 0                  # pose samples its filter has received since it was made
    history: tuple = (("cam", 0),)    # what an oracle has to see to stand where the slot stands

    @property
    def fed(self):
        return self.frame >= 0

    @property
    def empty(self):
        return self.frame < 0 and self.finished == 0

    @property
    def restarted(self):
        """ended a sequence and has had no frame since"""
        return self.frame < 0 and self.finished > 0

    @property
    def time_stamp(self):
        return self.frame / 20.0 if self.fed else 0.0

    @property
    def frames_in_run(self):
        return sum(1 for e in self.history if e[0] == "f")


class Model:
    def __init__(self, window=None):
        self.slots = [SlotState() for _ in range(N_SLOTS)]
        self.snaps = {}               # name -> the saved slot's state
        self.window = window
        self.log = []                 # (op, [SlotState copies]) after every op

    def _end(self, st):
        """end_sequence: nothing happens to a slot without a frame (its filter keeps what updates made of it)"""
        if st.frame < 0:
            return
        st.run += 1
        st.finished += 1
        st.scene, st.frame, st.floor, st.trims, st.loaded_from, st.samples = None, -1, 0, 0, None, 0
        st.history = (("cam", st.rig),)

    def next_frame(self, slot):
        return self.slots[slot].frame + 1

    def apply(self, op):
        S, p = self.slots, op.p
        if op.kind == "frames":
            for s, sc in zip(op.slots, p["scenes"]):
                if sc is None:
                    continue
                st = S[s]
                assert st.scene in (None, sc), f"slot {s} plays scene {st.scene}, fed scene {sc}"
                st.scene, st.frame = sc, st.frame + 1
                assert st.frame < N_FRAMES
                st.history += (("f", sc, st.frame),)
        elif op.kind == "restart":
            for s in op.slots:
                self._end(S[s])
        elif op.kind == "rig":
            for s, r in zip(op.slots, p["rigs"]):
                self._end(S[s])
                S[s].rig = r
                S[s].history = (("cam", r),) + S[s].history[1:]
        elif op.kind == "trim":
            below = p.get("below") or [None] * len(op.slots)
            for s, b in zip(op.slots, below):
                if S[s].fed:
                    S[s].trims += 1
        elif op.kind == "save":
            for s, name in zip(op.slots, p["snaps"]):
                assert name not in self.snaps, name
                self.snaps[name] = copy.deepcopy(S[s])
        elif op.kind == "load":
            for s, name in zip(op.slots, p["snaps"]):
                src = self.snaps[name]
                assert src.rig == S[s].rig, f"slot {s} on rig {S[s].rig}: snapshot {name} is of rig {src.rig}"
                self._end(S[s])
                if src.fed:
                    st = S[s]
                    st.scene, st.frame, st.floor, st.trims, st.samples = src.scene, src.frame, src.floor, src.trims, src.samples
                    st.history, st.loaded_from = src.history, name
        elif op.kind == "pose":
            for s, n in zip(op.slots, p["counts"]):
                if n:
                    S[s].samples += n
                    S[s].history += (("p", p["seed"], s, n),)
        else:
            assert op.kind in EXPORT_KINDS + ("wait", "reject"), op.kind
        self.log.append((op, copy.deepcopy(S)))
        return self.log[-1][1]


def run_model(schedule):
    m = Model(schedule.window)
    for op in schedule.ops:
        m.apply(op)
    return m


# ------------------------------------------------------------------------------------- staging need (a model too)

def staging_need(op, group):
    """what the op's share for `group` asks of its kind's staging block, in units that grow with the real bytes: named
    slots of the group times the size of one slot's part. Host mode only: a device-mode job writes straight into the
    caller's memory. 0: no staging."""
    n = sum(1 for s in op.named() if group_of(s) == group)
    p = op.p
    if op.kind not in BLOCK or n == 0:
        return 0
    if op.kind == "pose":
        return sum(c for s, c in zip(op.slots, p["counts"]) if group_of(s) == group)
    if p.get("device"):
        return 0
    if op.kind == "views":
        level = p["level"] if p["plane"] == "left" else 0
        return n * (WIDTH >> level) * (HEIGHT >> level) * PIXEL_BYTES[p["pixel"]]
    if op.kind == "disparity":
        return n * (2 if p["cost"] else 1)
    if op.kind == "scenes":
        return n * SCENE_COLS * SCENE_ROWS * PIXEL_BYTES[p["pixel"]]
    if op.kind == "ar":
        return n * WIDTH * HEIGHT * PIXEL_BYTES[p["pixel"]]
    return n


# ------------------------------------------------------------------------------------------------ the circuit

def euler_circuit(n, variant=0):
    """An Eulerian circuit of the complete directed graph with loops on n nodes (n * n edges, every node n in and n
    out): Hierholzer from node 0, the neighbours of u tried in the fixed order u + variant, u + variant + 1, ...
    (mod n). n * n + 1 nodes; every ordered pair occurs adjacently exactly once."""
    ptr = [0] * n
    stack, out = [0], []
    while stack:
        u = stack[-1]
        if ptr[u] < n:
            stack.append((u + variant + ptr[u]) % n)
            ptr[u] += 1
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == n * n + 1
    return out


def roles(variant):
    """the slots of a variant: common (named by every op) and mate share group `variant`; a (rig 1) and the slot that
    stays empty share the next group; b and d the third"""
    c = 2 * (variant % N_GROUPS)
    return dict(common=c, mate=c + 1, a=(c + 2) % 6, empty=(c + 3) % 6, b=(c + 4) % 6, d=(c + 5) % 6)


PROLOGUE_SCENE = dict(common=0, mate=1, a=2, b=1, d=0)
VIEW_PIXELS = ("gray8", "rgb8", "rgba8")
PRESETS = ("top", "front", "side")


def _frames_op(model, scenes_of):
    """a frame set: scenes_of {slot: scene to start with if the slot has none}; the others sit out"""
    scenes = []
    for s in range(N_SLOTS):
        if s not in scenes_of:
            scenes.append(None)
        else:
            st = model.slots[s]
            scenes.append(st.scene if st.scene is not None else scenes_of[s])
    return Op("frames", tuple(range(N_SLOTS)), dict(scenes=tuple(scenes)))


def prologue(model, r, n_frames, saves=True):
    """a -> rig 1; n_frames frame sets to the five running slots; (saves) b and a saved in host and in device mode as
    P0h, P1h, P0d, P1d; wait. The ops, applied to the model."""
    ops = [Op("rig", (r["a"],), dict(rigs=(1,)))]
    start = {r[k]: PROLOGUE_SCENE[k] for k in PROLOGUE_SCENE}
    model.apply(ops[0])
    for _ in range(n_frames):
        ops.append(_frames_op(model, start))
        model.apply(ops[-1])
    if saves:
        for mode in "hd":
            ops.append(Op("save", (r["b"], r["a"]), dict(snaps=(f"P0{mode}", f"P1{mode}"), device=mode == "d")))
            model.apply(ops[-1])
    ops.append(Op("wait"))
    model.apply(ops[-1])
    return ops


def _export_style(kind, j, large, variant):
    """the parameters of the j-th job of an export kind: small styles (a job costs about a millisecond); `large` ones
    need a bigger staging block per slot where the kind has a choice"""
    what = ("frames", "last_keyframes")[(j + variant) % 2]
    if kind == "export":
        return dict(what=what)
    if kind == "map":
        return dict(own_only=(j + variant) % 2)
    if kind == "views":
        pixel = VIEW_PIXELS[(j + variant) % 3 if not large else 1 + j % 2]
        return dict(what=what, plane="left", level=0 if large else 2, pixel=pixel, markers=j % 3 != 1 and pixel != "gray8")
    if kind == "disparity":
        return dict(what=what, value=("disparity", "depth")[j // 2 % 2], step=8, cost=bool(large))
    if kind == "cloud":
        return dict(what=what, step=8, frame=("world", "camera")[j // 2 % 2], layout=("compact", "organized")[(j + variant) % 2],
                    min_disparity=3.5, max_depth=5.0)
    if kind == "scenes":
        return dict(camera=PRESETS[(j + variant) % 3], pixel="rgba8" if large else "rgb8", point_size=1 + j % 3)
    if kind == "ar":
        return dict(pixel="rgba8" if large else "rgb8")
    raise AssertionError(kind)


def circuit(variant, prologue_frames=60):
    """The fourteen kinds in an Eulerian circuit: 197 ops behind a prologue, every ordered pair of kinds adjacent
    exactly once, every op naming the variant's common slot (so both ops of a pair stand next to each other in its
    group's queue). The j-th op of a kind is in device mode for odd j + variant. From its `grow`-th job on a kind
    names the common slot's mate too and takes its large style: that job is in host mode and stands behind a job of
    another kind, so its staging block is replaced there. No wait between the prologue's and the end."""
    r = roles(variant)
    c, mate, others = r["common"], r["mate"], (r["a"], r["b"], r["d"], r["empty"])
    model = Model()
    ops = prologue(model, r, prologue_frames)
    start = len(ops)
    nodes = euler_circuit(len(KINDS), variant)
    kinds = [KINDS[i] for i in nodes]
    # the job of each staged kind that grows its block: host mode, behind another kind
    grow = {}
    for kind in BLOCK:
        js = [i for i, k in enumerate(kinds) if k == kind]
        first = 2 + (variant + KINDS.index(kind)) % 3     # (behind an earlier host-mode job: there is a block to outgrow)
        grow[kind] = next(j for j in range(first, len(js)) if kinds[js[j] - 1] != kind and (kind == "pose" or (j + variant) % 2 == 0))
    seen = {k: 0 for k in KINDS}
    for i, kind in enumerate(kinds):
        j = seen[kind]
        seen[kind] += 1
        large = kind in grow and j >= grow[kind]
        device = (j + variant) % 2 == 1
        extra = (others[j % 4],) if not large else (mate, others[j % 4], others[(j + 1) % 4])
        slots = (c,) + extra if j % 2 == 0 else extra + (c,)
        if kind == "frames":
            feed = {c: (j + variant) % N_SCENES}
            for s in (mate, r["a"], r["b"], r["d"]):
                if (s + j) % 5 != 0:                         # (now and then a slot sits a step out)
                    feed[s] = PROLOGUE_SCENE[next(k for k in PROLOGUE_SCENE if r[k] == s)]
            op = _frames_op(model, feed)
        elif kind == "restart":
            op = Op(kind, (c,))
        elif kind == "rig":
            op = Op(kind, (c,), dict(rigs=(1 - model.slots[c].rig,)))
        elif kind == "trim":
            op = Op(kind, slots, dict(below=None if j % 2 == 0 else tuple(1 + j // 2 for _ in slots)))
        elif kind == "save":
            named = (c, mate) if large else (c,)
            op = Op(kind, named, dict(snaps=tuple(f"S{i}_{s}" for s in named), device=device))
        elif kind == "load":
            named = (c, mate) if large else (c,)
            op = Op(kind, named, dict(snaps=tuple(f"P{model.slots[s].rig}{'d' if device else 'h'}" for s in named), device=device))
        elif kind == "pose":
            named = (c, mate, others[j % 3]) if large else (c, others[j % 3])
            op = Op(kind, named, dict(seed=1000 * variant + i, counts=tuple(3 + (s == c) * (3 if large else 0) for s in named)))
        else:
            op = Op(kind, slots, dict(_export_style(kind, j, large, variant), device=device))
        model.apply(op)
        ops.append(op)
    ops.append(Op("wait"))
    return Schedule(f"circuit{variant}", ops, start, None, dict(r, grow=grow, kinds=kinds))


# --------------------------------------------------------------------------------------- hand-written schedules

def _every_export(slots, device, tag=0):
    """one job of every export kind on `slots`"""
    return [Op(kind, slots, dict(_export_style(kind, tag + i, False, 0), device=device)) for i, kind in enumerate(EXPORT_KINDS)]


def _build(name, make, window=None, prologue_frames=40, saves=False):
    """a schedule from make(model, roles, add): add(op) applies the op to the model and appends it"""
    r = roles(0)
    model = Model(window)
    ops = prologue(model, r, prologue_frames, saves)
    start = len(ops)

    def add(op):
        model.apply(op)
        ops.append(op)
        return op
    make(model, r, add)
    add(Op("wait"))
    return Schedule(name, ops, start, window, r)


def _running(model, r, sit_out=()):
    return {r[k]: PROLOGUE_SCENE[k] for k in PROLOGUE_SCENE if r[k] not in sit_out}


def save_wait_load():
    """save, wait, then a load of that very snapshot into a slot of another group with other jobs between; once in
    host and once in device mode"""
    def make(model, r, add):
        for mode, (src, dst) in zip("hd", ((r["b"], r["common"]), (r["a"], r["d"]))):
            if model.slots[dst].rig != model.slots[src].rig:
                add(Op("rig", (dst,), dict(rigs=(model.slots[src].rig,))))
            add(Op("save", (src,), dict(snaps=(f"X{mode}",), device=mode == "d")))
            add(Op("wait"))
            add(_frames_op(model, _running(model, r)))
            add(Op("views", (dst, src), dict(_export_style("views", 1, False, 0), device=mode == "h")))
            add(Op("pose", (src,), dict(seed=77, counts=(3,))))
            add(Op("load", (dst,), dict(snaps=(f"X{mode}",), device=mode == "d")))
            add(Op("export", (src, dst), dict(what="frames", device=mode == "d")))
            add(Op("scenes", (dst,), dict(_export_style("scenes", 0, False, 0), device=False)))
            for _ in range(2):
                add(_frames_op(model, _running(model, r)))
            add(Op("save", (dst, src), dict(snaps=(f"Y{mode}0", f"Y{mode}1"), device=mode == "h")))
    return _build("save_wait_load", make)


def restart_then_exports():
    """a restart of a slot, then every export kind (and a save) before its first frame; then frames and again"""
    def make(model, r, add):
        c, b = r["common"], r["b"]
        add(Op("restart", (c,)))
        for op in _every_export((c, b), False) + _every_export((r["empty"], c), True, 1):
            add(op)
        add(Op("save", (c,), dict(snaps=("R0",), device=False)))
        add(Op("trim", (c, b), dict(below=None)))
        for _ in range(2):
            add(_frames_op(model, {**_running(model, r), c: 2}))
        for op in _every_export((b, c), True, 2):
            add(op)
        add(Op("save", (c,), dict(snaps=("R1",), device=True)))
    return _build("restart_then_exports", make)


def trim_window(export_after=None, prologue_frames=60, steps=12):
    """set_keyframe_window(0) active: every export kind (and a save) behind the frame sets after which a keyframe of
    slot b or d retires and is trimmed by the step itself. export_after: the frame indices (of b and d, which never
    sit out) behind which the jobs go; None: behind every frame set."""
    def make(model, r, add):
        for t in range(steps):
            add(_frames_op(model, _running(model, r)))
            k = model.slots[r["b"]].frame
            if export_after is None or k in export_after:
                for op in _every_export((r["b"], r["d"]), t % 2 == 1, t):
                    add(op)
                add(Op("save", (r["d"], r["b"]), dict(snaps=(f"W{k}d", f"W{k}b"), device=t % 2 == 0)))
                add(Op("trim", (r["b"],), dict(below=None)))
    return _build("trim_window", make, 0, prologue_frames)


def rig_then_dense():
    """a rig assignment, then depth, cloud and AR on the slot's next frame, beside a slot of the ctx's own rig"""
    def make(model, r, add):
        c, b = r["common"], r["b"]
        for rig in (1, 0):
            add(Op("rig", (c,), dict(rigs=(rig,))))
            add(_frames_op(model, {**_running(model, r), c: 1}))
            add(Op("disparity", (c, b), dict(what="frames", value="depth", step=8, cost=False, device=rig == 0)))
            add(Op("cloud", (b, c), dict(_export_style("cloud", 0, False, 0), what="frames", device=rig == 1)))
            add(Op("ar", (c, b), dict(pixel="rgb8", device=rig == 0)))
            add(_frames_op(model, _running(model, r)))
    return _build("rig_then_dense", make)


def pose_between_frames():
    """pose updates between two frame sets of a slot, beside a slot of the same group that sits those steps out"""
    def make(model, r, add):
        c, mate = r["common"], r["mate"]
        for t in range(4):
            add(_frames_op(model, _running(model, r, sit_out=(mate,))))
            add(Op("pose", (c, r["b"]) if t % 2 else (r["b"], c), dict(seed=500 + t, counts=(3, 2 + t))))
        add(_frames_op(model, _running(model, r)))
        add(Op("export", (c, mate), dict(what="frames", device=False)))
    return _build("pose_between_frames", make)


REJECTS = ("twice", "capacity", "reserved")          # a slot named twice; a capacity too small; a reserved style field set


def rejected_between():
    """rejected submits between queued jobs that have not run yet: each fails with its error and queues nothing"""
    def make(model, r, add):
        c, b = r["common"], r["b"]
        for t, what in enumerate(REJECTS):
            add(_frames_op(model, _running(model, r)))
            add(Op("views", (c, b), dict(_export_style("views", t, True, 0), device=False)))
            add(Op("reject", (c, b), dict(how=what)))
            add(Op("export", (b, c), dict(what="last_keyframes", device=t % 2 == 1)))
            add(Op("reject", (c,), dict(how=REJECTS[(t + 1) % 3])))
            add(_frames_op(model, _running(model, r)))
    return _build("rejected_between", make)


HAND_WRITTEN = dict(save_wait_load=save_wait_load, restart_then_exports=restart_then_exports, trim_window=trim_window,
                    rig_then_dense=rig_then_dense, pose_between_frames=pose_between_frames, rejected_between=rejected_between)
VARIANTS = (0, 1, 2)
