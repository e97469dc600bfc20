"""Multi-sequence / multi-GPU driver logic.

The path shards across SEQUENCES only: frame t of a sequence needs the pose,
points and filter states of frame t-1 (src/lib/stereo_slam.cpp:125,183-196),
so a sequence never leaves its GPU and there is NO data-path collective.
One process per GPU owns `seqs_per_rank` sequences (one svo_ctx, sequence =
grid dimension); ranks only meet at the barriers around the timed region and
in one small all_gather of per-sequence summaries at the end (RCCL over xGMI
on the GPU box — backend "nccl" — or gloo in the CPU tests).
"""
import os
import time

import numpy as np
import torch
import torch.distributed as dist


def rank_info():
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def init_distributed(backend=None):
    """Process group from the torchrun environment; single process when WORLD_SIZE <= 1."""
    rank, local_rank, world = rank_info()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        kw = {}
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            kw["device_id"] = torch.device("cuda", local_rank)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
    return rank, local_rank, world


def sequence_ids(rank, world, seqs_per_rank):
    """Global ids (= scene seeds) of the sequences owned by `rank`: weak scaling,
    every rank owns the same number of independent sequences."""
    return list(range(rank * seqs_per_rank, (rank + 1) * seqs_per_rank))


def assign_longest_first(lengths, n_ranks):
    """Static longest-first assignment of whole sequences to ranks (a sequence cannot be
    split, frame t needs frame t-1): sequences by decreasing length, each to the rank with the least
    work so far. Returns one list of sequence indices per rank (ranks may stay empty: six EuRoC
    sequences on eight GPUs keep six busy)."""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    load = [0] * n_ranks
    out = [[] for _ in range(n_ranks)]
    for i in order:
        r = min(range(n_ranks), key=lambda k: (load[k], k))
        out[r].append(i)
        load[r] += lengths[i]
    return out


def play_unequal(slam, frames_of, lengths, time_of=lambda k: k / 20.0):
    """Drive the sequences of one ctx to their own ends: at step k every sequence that still has a
    frame gets it, the others sit the step out (svo_new_images with NULL pointers). frames_of(s, k)
    -> (left, right). Returns the number of sequence-frames processed."""
    done = 0
    for k in range(max(lengths) if lengths else 0):
        L, R = [], []
        for s, n in enumerate(lengths):
            if k < n:
                l, r = frames_of(s, k)
                L.append(l); R.append(r)
                done += 1
            else:
                L.append(None); R.append(None)
        slam.new_images(L, R, [time_of(k)] * len(lengths))
    return done


def queue_schedule(lengths, n_slots, order=None, rigs=None):
    """Sequences played back to back on the slots of one ctx: a slot whose sequence has ended takes the next
    sequence of `order` at the very next step (order=None: longest first, the index as tie-break: the order
    of assign_longest_first). Returns one list per step of (slot, sequence, frame index), in slot order;
    sequences without frames are never scheduled. No GPU involved.
    rigs: the camera rig (svo_ctx_add_rigs id, 0: the ctx's own) of every sequence. The same schedule (a rig costs
    no step), its entries (slot, sequence, frame index, rig, how): a freed slot takes the next sequence together with
    its rig, and `how` says what the ctx is asked before a sequence's first frame: "assign" where the rig differs
    from the one the slot is bound to (every slot starts on rig 0), "restart" where it is the same and the slot has
    played before, None otherwise and for every later frame."""
    if rigs is not None:
        bound, played = [0] * n_slots, [False] * n_slots
        steps = []
        for step in queue_schedule(lengths, n_slots, order):
            out = []
            for slot, seq, k in step:
                how = None
                if k == 0:
                    how = "assign" if rigs[seq] != bound[slot] else "restart" if played[slot] else None
                    bound[slot], played[slot] = rigs[seq], True
                out.append((slot, seq, k, rigs[seq], how))
            steps.append(out)
        return steps
    if order is None:
        order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    waiting = [i for i in order if lengths[i] > 0]
    waiting.reverse()                       # (pop() takes the next one)
    playing = [None] * n_slots              # per slot: [sequence, next frame]
    steps = []
    while True:
        step = []
        for slot in range(n_slots):
            if playing[slot] is None and waiting:
                playing[slot] = [waiting.pop(), 0]
            if playing[slot] is None:
                continue
            seq, k = playing[slot]
            step.append((slot, seq, k))
            playing[slot] = [seq, k + 1] if k + 1 < lengths[seq] else None
        if not step:
            return steps
        steps.append(step)


def _queue_steps(n, frames_of, lengths, time_of, order, rigs=None):
    """queue_schedule as calls on a ctx of n slots: [(slots to restart before the step, lefts, rights, time
    stamps)] with None for slots without a frame, {sequence: (slot, run ordinal in that slot)}, sequence-frames.
    A slot is restarted before the first frame of every sequence but its first. With rigs (one per sequence) a step
    has a fifth entry, (slots, rigs) to assign before it: a slot whose next sequence is on another rig is assigned
    instead of restarted (the assignment ends its sequence too)."""
    runs_started = [0] * n
    where, steps, frames = {}, [], 0
    for step in queue_schedule(lengths, n, order, rigs if rigs is not None else [0] * len(lengths)):
        L, R, ts = [None] * n, [None] * n, [0.0] * n
        restart, assign = [], ([], [])
        for slot, seq, k, rig, how in step:
            if k == 0:
                if how == "restart":
                    restart.append(slot)
                elif how == "assign":
                    assign[0].append(slot); assign[1].append(rig)
                where[seq] = (slot, runs_started[slot])
                runs_started[slot] += 1
            L[slot], R[slot] = frames_of(seq, k)
            ts[slot] = time_of(seq, k)
        steps.append((restart, L, R, ts) if rigs is None else (restart, L, R, ts, assign))
        frames += len(step)
    return steps, where, frames


def pack_queue(slam, frames_of, lengths, time_of=lambda s, k: k / 20.0, order=None, borrow=False, rigs=None):
    """The steps of a pipelined play_queue built ahead (keeps Python out of a timed loop): a list of (slots to
    restart before the step, packed frame set of slam.pack_images[, (slots, rigs) to assign before the step: with
    rigs]), then where and frames as play_queue returns them."""
    steps, where, frames = _queue_steps(slam.n, frames_of, lengths, time_of, order, rigs)
    return [(st[0], slam.pack_images(st[1], st[2], st[3], borrow=borrow)) + tuple(st[4:]) for st in steps], where, frames


def submit_queue(slam, steps):
    """Queue the steps of pack_queue on the ctx (restarts, rig assignments and frame sets in order); nothing is
    waited for."""
    for restart, packed, *assign in steps:
        if restart:
            slam.restart(restart)
        if assign and assign[0][0]:
            slam.assign_rigs(*assign[0])
        slam.submit_packed(packed)


def play_queue(slam, frames_of, lengths, time_of=lambda s, k: k / 20.0, order=None, pipelined=False, borrow=False,
               rigs=None, keyframe_window=None):
    """Drive a ctx through queue_schedule(lengths, slam.n, order): a slot is restarted before the first frame
    of every sequence but its first, slots without a frame get None, time stamps are per sequence
    (time_of(sequence, frame index)). frames_of(sequence, k) -> (left, right). pipelined: every frame set and
    restart is queued (svo_submit_images; torch frames, with borrow used in place) and waited for once at the
    end; otherwise one new_images call per step. rigs: the camera rig (an id of slam.add_rigs, 0: the ctx's own) of
    every sequence; a freed slot takes the next sequence together with its rig (slam.assign_rigs instead of the
    restart where the rig differs from the slot's). keyframe_window: None leaves the ctx's setting alone, else
    slam.set_keyframe_window(keyframe_window) before the first step (an int >= -1: the retired keyframes a slot keeps, so
    that sequences of any length play in bounded memory). Returns ({sequence: (slot, run ordinal in that slot)},
    number of sequence-frames)."""
    if keyframe_window is not None:
        if int(keyframe_window) != keyframe_window or keyframe_window < -1:
            raise ValueError(f"keyframe_window {keyframe_window!r}: an int >= -1 (or None)")
        slam.set_keyframe_window(int(keyframe_window))
    if pipelined:
        steps, where, frames = pack_queue(slam, frames_of, lengths, time_of, order, borrow, rigs)
        submit_queue(slam, steps)
        slam.wait()
        return where, frames
    steps, where, frames = _queue_steps(slam.n, frames_of, lengths, time_of, order, rigs)
    for restart, L, R, ts, *assign in steps:
        if restart:
            slam.restart(restart)
        if assign and assign[0][0]:
            slam.assign_rigs(*assign[0])
        slam.new_images(L, R, ts)
    return where, frames


def move(src, src_slots, dst, dst_slots, voxel_maps=False):
    """Move sequences between two ctxs (or two slots of one): a device-mode save of src's slots, their restart,
    then the load into dst's slots (any slot count, group layout or GPU of the same process: the data parts go
    through a copy to dst's device when it differs). Waits for both ctxs. Returns the Snapshots (in dst's memory).
    A slot's camera settings travel with it: a target slot that tracks with other settings is first bound to a rig
    of dst with the source slot's settings (added to dst if it has none). Rectification maps are not part of a
    snapshot and do not travel: such a rig of dst has none.
    voxel_maps=True: the slots' voxel maps go along. Every named slot of src and of dst must have a map, pairwise with
    the same voxel edge (ValueError before anything moves). After the sequences have moved: a device-mode save of
    src's maps, a copy to dst's device where it differs, a replace load into dst's maps, and src's maps are cleared.
    Returns (Snapshots, VoxelLoads); a dst map too small for the entries comes back VOXEL_LOAD_FULL in the VoxelLoads,
    is left unchanged, and src's map is then not cleared."""
    from . import hip_lib
    from .stereo_slam import Snapshot
    if voxel_maps:
        for s_slot, d_slot in zip(src_slots, dst_slots):
            a, b = src.voxel_map_info(s_slot), dst.voxel_map_info(d_slot)
            if a is None or b is None:
                raise ValueError(f"move(voxel_maps=True): slot {s_slot} of src or slot {d_slot} of dst has no voxel map")
            if np.float32(a["voxel"]).tobytes() != np.float32(b["voxel"]).tobytes():
                raise ValueError(f"move(voxel_maps=True): slot {d_slot} of dst has voxel edge {b['voxel']!r}, slot {s_slot} of src {a['voxel']!r}")
    snaps = _move_sequences(src, src_slots, dst, dst_slots, Snapshot)
    if not voxel_maps:
        return snaps
    saves = src.save_voxel_maps(src_slots, device=True)
    entries = [saves.entries(i) for i in range(len(src_slots))]
    if dst.device != src.device:
        entries = [e.to(dst.device) for e in entries]
    loads = dst.load_voxel_maps(dst_slots, entries, voxel=[saves.voxel(i) for i in range(len(src_slots))])
    moved = [s for i, s in enumerate(src_slots) if loads.status(i) == hip_lib.VOXEL_LOADED]
    if moved:
        src.clear_voxel_maps(moved)
    return snaps, loads


def _move_sequences(src, src_slots, dst, dst_slots, Snapshot):
    snaps = src.save(src_slots, device=True)
    src.restart(src_slots)
    if dst.device != src.device:
        snaps = [Snapshot(s.host, s.data.to(dst.device)) for s in snaps]
    for s_slot, d_slot in zip(src_slots, dst_slots):
        cam = src.slot_rig(s_slot)[1]
        if bytes(dst.slot_rig(d_slot)[1]) != bytes(cam):
            dst.assign_rigs([d_slot], [dst.find_rig(cam, add=True)])
    dst.load(dst_slots, snaps)
    return snaps


def _sync(device):
    if device is not None and device.type == "cuda":
        torch.cuda.synchronize(device)


def _barrier(world, device):
    if world > 1:
        if device is not None and device.type == "cuda":
            dist.barrier(device_ids=[device.index])
        else:
            dist.barrier()


def timed_steps(step_fn, steps, warmup, world, device=None, coll_device="same", finish_fn=None):
    """Driver contract: `warmup` untimed steps, then exactly `steps` steps bracketed
    by barrier + device synchronize on both sides; returns MAX-over-ranks seconds.
    `device` is synchronized; collectives run on `coll_device` (default: the same;
    None = host tensors, e.g. gloo). `finish_fn` drains work that step_fn only queued
    (svo_submit_images): it runs inside the timed region, before the closing synchronize."""
    if coll_device == "same":
        coll_device = device
    for k in range(warmup):
        step_fn(k)
    if finish_fn:
        finish_fn()
    _sync(device)
    _barrier(world, coll_device)
    _sync(device)
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        step_fn(k)
    if finish_fn:
        finish_fn()
    _sync(device)
    t1 = time.perf_counter()
    _barrier(world, coll_device)
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64,
                           device=coll_device if (coll_device is not None and coll_device.type == "cuda") else "cpu")
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    return float(elapsed.item())


def gather_summaries(local, world, device=None):
    """all_gather of the fixed-size per-sequence summaries ([n_local, k] float64):
    the one exchange of the multi-GPU path. Returns [world * n_local, k]."""
    t = torch.as_tensor(np.asarray(local, np.float64))
    if world <= 1:
        return t.numpy()
    if device is not None and device.type == "cuda":
        t = t.to(device)
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return torch.cat(out, 0).cpu().numpy()


def throughput(total_units, seconds):
    return total_units / seconds if seconds > 0 else float("nan")
