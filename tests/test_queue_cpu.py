"""The schedules of queue_cases.py reach what test_queue_gpu.py plays them for, and the model is consistent: no GPU,
no HIP library, no oracle."""
import itertools

import pytest

import queue_cases as Q

ALL_PAIRS = set(itertools.product(Q.KINDS, Q.KINDS))


def _body(schedule):
    """the ops behind the prologue, without the wait at the end"""
    assert schedule.ops[-1].kind == "wait"
    return schedule.ops[schedule.start:-1]


def _queue(ops, group):
    """the entries the ops leave in one group's queue, in order"""
    return [op for op in ops if any(Q.group_of(s) == group for s in op.named())]


def test_euler_circuit_has_every_ordered_pair_once():
    for variant in Q.VARIANTS:
        nodes = Q.euler_circuit(len(Q.KINDS), variant)
        pairs = list(zip(nodes, nodes[1:]))
        assert len(pairs) == 196 == len(set(pairs)) and nodes[0] == nodes[-1] == 0
    assert Q.euler_circuit(len(Q.KINDS), 0) != Q.euler_circuit(len(Q.KINDS), 1)


@pytest.mark.parametrize("variant", Q.VARIANTS)
def test_circuit_pairs_stand_next_to_each_other_in_the_common_slots_queue(variant):
    sc = Q.circuit(variant)
    body = _body(sc)
    c = sc.roles["common"]
    assert len(body) == 197 and Q.group_of(c) == variant and all(op.kind in Q.KINDS for op in body), "no wait inside the circuit"
    pairs = [(a.kind, b.kind) for a, b in zip(body, body[1:])]
    assert set(pairs) == ALL_PAIRS and len(pairs) == 196
    for a, b in zip(body, body[1:]):
        assert c in set(a.named()) & set(b.named()), (a, b)
    # the same in the queue of the common slot's group: nothing of another slot's gets between the two of a pair
    queue = _queue(body, Q.group_of(c))
    assert [op.kind for op in queue] == [op.kind for op in body]
    # the other groups see a mixture too, the slot that stays empty is named by jobs and never fed, loaded or assigned
    for g in range(Q.N_GROUPS):
        assert len({(a.kind, b.kind) for a, b in zip(_queue(body, g), _queue(body, g)[1:])}) >= 60, g
    empty = sc.roles["empty"]
    kinds_on_empty = {op.kind for op in body if empty in op.named()}
    assert kinds_on_empty >= set(Q.EXPORT_KINDS) and not kinds_on_empty & {"frames", "load", "rig", "pose"}
    assert all(st[empty].empty for _, st in Q.run_model(sc).log)
    # every export kind, save and load in host and in device mode
    for kind in Q.EXPORT_KINDS + ("save", "load"):
        assert {bool(op.p["device"]) for op in body if op.kind == kind} == {False, True}, kind


def test_the_variants_rotate_the_common_slot_through_all_groups():
    assert {Q.group_of(Q.circuit(v).roles["common"]) for v in Q.VARIANTS} == set(range(Q.N_GROUPS))
    assert len({tuple(Q.circuit(v).roles["kinds"]) for v in Q.VARIANTS}) == len(Q.VARIANTS)


def _outgrown_blocks(sc):
    """the staging blocks that are replaced by a larger one at least once, by a job that stands behind a job of another kind
    (and of another block) in its group's queue"""
    body = _body(sc)
    grown = set()
    for g in range(Q.N_GROUPS):
        queue = _queue(body, g)
        have = {}
        for i, op in enumerate(queue):
            block = Q.BLOCK.get(op.kind)
            need = Q.staging_need(op, g)
            if block is None or need == 0:
                continue
            if 0 < have.get(block, 0) < need and i > 0 and queue[i - 1].kind != op.kind and Q.BLOCK.get(queue[i - 1].kind) != block:
                grown.add(block)
            have[block] = max(have.get(block, 0), need)
    return grown


@pytest.mark.parametrize("variant", Q.VARIANTS)
def test_circuit_outgrows_every_staging_block_behind_another_kind(variant):
    sc = Q.circuit(variant)
    assert _outgrown_blocks(sc) == set(Q.BLOCK.values())
    body = _body(sc)
    for kind, j in sc.roles["grow"].items():              # the growing job is the one the builder says
        op = [o for o in body if o.kind == kind][j]
        assert sc.roles["mate"] in op.named() and not op.p.get("device"), (kind, j)


def _states(sc):
    """[(op, slots before, slots after)] of the schedule's part behind the prologue"""
    log = Q.run_model(sc).log
    return [(op, log[i - 1][1], after) for i, (op, after) in enumerate(log) if i >= sc.start]


def test_save_wait_load_into_another_group():
    sc = Q.save_wait_load()
    body = sc.ops[sc.start:]
    model = Q.run_model(sc)
    loads = [i for i, op in enumerate(body) if op.kind == "load"]
    assert len(loads) == 2 and {bool(body[i].p["device"]) for i in loads} == {False, True}
    for i in loads:
        name = body[i].p["snaps"][0]
        save = next(j for j, op in enumerate(body) if op.kind == "save" and name in op.p["snaps"])
        between = [op.kind for op in body[save + 1:i]]
        assert between[0] == "wait" and len(set(between) & set(Q.KINDS)) >= 3, between
        assert Q.group_of(body[save].slots[0]) != Q.group_of(body[i].slots[0])
        assert model.snaps[name].fed and model.snaps[name].frame >= 39


def test_restart_then_every_export_kind_before_the_first_frame():
    sc = Q.restart_then_exports()
    c = sc.roles["common"]
    seen, fed_again = set(), set()
    for op, before, after in _states(sc):
        if c in op.named() and op.kind in Q.EXPORT_KINDS + ("save",):
            if after[c].restarted:
                assert after[c].run == 1 and after[c].finished == 1
                seen.add((op.kind, bool(op.p["device"])))
            elif after[c].fed and after[c].run == 1:
                fed_again.add(op.kind)
    assert {k for k, _ in seen} == set(Q.EXPORT_KINDS) | {"save"}
    assert {k for k, d in seen if d} == set(Q.EXPORT_KINDS) and fed_again >= set(Q.EXPORT_KINDS)


def test_trim_window_exports_behind_the_frame_sets():
    for after_frames in (None, {62, 65}):
        sc = Q.trim_window(after_frames)
        assert sc.window == 0
        b = sc.roles["b"]
        states = _states(sc)
        behind = {}
        for i, (op, before, after) in enumerate(states):
            if op.kind == "frames":
                k = after[b].frame
                kinds = list(itertools.takewhile(lambda kd: kd != "frames", (o.kind for o, _, _ in states[i + 1:])))
                behind[k] = kinds
        hit = [k for k, kinds in behind.items() if set(kinds) >= set(Q.EXPORT_KINDS) | {"save", "trim"}]
        assert (len(hit) == 12 and min(hit) == 60) if after_frames is None else set(hit) == after_frames
        assert all(st[b].frames_in_run == st[b].frame + 1 for _, _, st in states), "b never sits out and never restarts"


def test_rig_assignment_then_dense_jobs_on_the_next_frame():
    sc = Q.rig_then_dense()
    c, b = sc.roles["common"], sc.roles["b"]
    states = _states(sc)
    seen = set()
    for i, (op, before, after) in enumerate(states):
        if op.kind == "rig":
            assert states[i + 1][0].kind == "frames" and states[i + 1][2][c].frame == 0
            kinds = [o.kind for o, _, _ in states[i + 2:i + 5]]
            assert kinds == ["disparity", "cloud", "ar"] and states[i + 2][0].p["value"] == "depth"
            for o, _, st in states[i + 2:i + 5]:
                assert {c, b} == set(o.named()) and st[c].rig == op.p["rigs"][0] and st[b].rig == 0 and st[c].frame == 0
            seen.add(op.p["rigs"][0])
    assert seen == {0, 1}


def test_pose_updates_between_two_frame_sets_beside_a_slot_that_sits_out():
    sc = Q.pose_between_frames()
    c, mate = sc.roles["common"], sc.roles["mate"]
    assert Q.group_of(c) == Q.group_of(mate)
    states = _states(sc)
    hits = 0
    for i, (op, before, after) in enumerate(states):
        if op.kind == "pose" and c in op.named():
            prev, nxt = states[i - 1], states[i + 1]
            assert prev[0].kind == nxt[0].kind == "frames" and c in prev[0].named() and c in nxt[0].named()
            assert mate not in prev[0].named() and after[mate].fed and after[c].samples > before[c].samples
            hits += 1
    assert hits == 4


def test_rejected_submits_stand_between_queued_jobs():
    sc = Q.rejected_between()
    body = sc.ops[sc.start:]
    rejects = [i for i, op in enumerate(body) if op.kind == "reject"]
    assert {body[i].p["how"] for i in rejects} == set(Q.REJECTS) and len(rejects) == 6
    for i in rejects:
        assert body[i - 1].kind in Q.KINDS and body[i + 1].kind in Q.KINDS, "queued jobs on both sides, no wait"
    assert [op.kind for op in body].count("wait") == 1


ALL_SCHEDULES = [lambda v=v: Q.circuit(v) for v in Q.VARIANTS] + list(Q.HAND_WRITTEN.values())


def test_the_model_is_consistent():
    for make in ALL_SCHEDULES:
        sc = make()
        model = Q.Model(sc.window)
        prev = [Q.SlotState() for _ in range(Q.N_SLOTS)]
        for op in sc.ops:
            now = model.apply(op)
            for s in range(Q.N_SLOTS):
                a, b = prev[s], now[s]
                assert b.run >= a.run and b.finished >= a.finished and b.run == b.finished
                if op.kind == "load" and s in op.slots:
                    src = model.snaps[op.p["snaps"][op.slots.index(s)]]
                    assert (b.scene, b.frame, b.history, b.samples, b.rig) == (src.scene, src.frame, src.history, src.samples, src.rig)
                    assert b.loaded_from is not None and b.run == a.run + a.fed
                elif b.run == a.run:                      # within a run frame ids go up by one, with a frame set only
                    assert b.frame - a.frame == (op.kind == "frames" and s in op.named()), (sc.name, op, s)
                    assert b.rig == a.rig or not a.fed
                else:
                    assert op.kind in Q.ENDING and s in op.slots and a.fed and not b.fed and b.history == (("cam", b.rig),)
                assert b.frames_in_run == b.frame + 1 or b.loaded_from is not None or any(e[0] == "f" for e in b.history) is False
                assert b.history[0] == ("cam", b.rig) and b.frame < Q.N_FRAMES
            prev = now
        assert len({id(st) for _, log in model.log for st in log}) == len(model.log) * Q.N_SLOTS, "the log holds copies"
