"""Host side of the sequence lifecycle, without a GPU: the schedule of sequences played back to back on the slots
of a ctx (multi_seq.queue_schedule), the driver that follows it (multi_seq.play_queue, against a ctx that only
records its calls), and the ctypes mirrors and NULL-ctx behaviour of the new entry points."""
import ctypes as C
import random

from stereo_svo_slam_amd import hip_lib, multi_seq, stereo_slam

EUROC = [2912, 1710, 2149, 2280, 2348, 1922]          # the EuRoC V1_01..V2_03 image counts of SURVEY §8d


def _passes_steps(lengths, n_slots):
    """steps of consecutive play_unequal passes of n_slots sequences each, in the given order"""
    return sum(max(lengths[i:i + n_slots]) for i in range(0, len(lengths), n_slots))


def _check_schedule(lengths, n_slots, order=None):
    steps = multi_seq.queue_schedule(lengths, n_slots, order)
    given = list(order) if order is not None else sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    seen = {}                                             # sequence -> (slot, frames so far)
    started = []
    for t, step in enumerate(steps):
        assert step, "no empty step"
        slots = [slot for slot, _, _ in step]
        assert slots == sorted(set(slots)) and all(0 <= s < n_slots for s in slots), (t, step)
        for slot, seq, k in step:
            if k == 0:
                assert seq not in seen
                started.append(seq)
                seen[seq] = (slot, 0)
            assert seen[seq] == (slot, k), "every frame once, in order, in one slot"
            seen[seq] = (slot, k + 1)
        # no slot is empty at a step at which a sequence still waits
        waiting = [i for i in given if lengths[i] > 0 and i not in seen]
        assert not waiting or len(step) == n_slots, (t, waiting)
    assert started == [i for i in given if lengths[i] > 0], "sequences start in the given order"
    assert {s: n for s, (_, n) in seen.items()} == {i: n for i, n in enumerate(lengths) if n > 0}
    total = sum(lengths)
    assert len(steps) >= -(-total // n_slots)
    return len(steps)


def test_queue_schedule_default_order_is_longest_first():
    rng = random.Random(0)
    cases = [(EUROC, n) for n in (1, 2, 3, 4, 6, 8)]
    for _ in range(2000):
        n_seq = rng.randint(0, 24)
        cases.append(([rng.randint(0, 40) for _ in range(n_seq)], rng.randint(1, 9)))
    for lengths, n_slots in cases:
        n_steps = _check_schedule(lengths, n_slots)
        load = [sum(lengths[i] for i in r) for r in multi_seq.assign_longest_first(lengths, n_slots)]
        assert n_steps == max(load), (lengths, n_slots)
        assert n_steps <= _passes_steps(sorted(lengths, reverse=True), n_slots)


def test_queue_schedule_given_order():
    rng = random.Random(1)
    for _ in range(500):
        lengths = [rng.randint(0, 30) for _ in range(rng.randint(1, 20))]
        n_slots = rng.randint(1, 8)
        order = list(range(len(lengths)))
        rng.shuffle(order)
        n_steps = _check_schedule(lengths, n_slots, order)
        assert n_steps <= _passes_steps([lengths[i] for i in order], n_slots), (lengths, n_slots, order)
    assert multi_seq.queue_schedule([], 4) == [] and multi_seq.queue_schedule([0, 0], 4) == []
    assert multi_seq.queue_schedule([2, 1, 1], 2, [0, 1, 2]) == [[(0, 0, 0), (1, 1, 0)], [(0, 0, 1), (1, 2, 0)]]


def test_queue_schedule_numbers_of_the_design_notes():
    """768 sequences of 60..240 frames on 256 slots (seeded): the queue needs fewer steps than three passes, and
    longest-first fewer still; the EuRoC lengths keep most slot-steps busy on few slots."""
    rng = random.Random(7)
    lengths = [rng.randint(60, 240) for _ in range(768)]
    passes = _passes_steps(lengths, 256)
    in_order = len(multi_seq.queue_schedule(lengths, 256, range(768)))
    longest_first = len(multi_seq.queue_schedule(lengths, 256))
    bound = -(-sum(lengths) // 256)
    assert bound <= longest_first <= in_order <= passes
    busy = lambda n: sum(EUROC) / (n * len(multi_seq.queue_schedule(EUROC, n)))
    assert busy(4) > busy(8) and busy(1) == 1.0


class _FakeCtx:
    """records what play_queue asks of a ctx"""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def restart(self, seqs):
        self.calls.append(("restart", list(seqs)))

    def new_images(self, L, R, ts):
        self.calls.append(("frames", list(L), list(R), list(ts)))

    def pack_images(self, L, R, ts, borrow=False):
        return ("packed", list(L), list(R), list(ts), borrow)

    def submit_packed(self, packed):
        self.calls.append(("frames",) + packed[1:4])

    def wait(self):
        self.calls.append(("wait",))


def test_play_queue_restarts_before_every_sequence_but_a_slots_first():
    lengths = [5, 2, 3, 1, 4, 2, 0, 3]
    for pipelined in (False, True):
        for order in (None, [3, 1, 0, 7, 2, 6, 5, 4]):
            ctx = _FakeCtx(3)
            where, done = multi_seq.play_queue(ctx, lambda s, k: (("L", s, k), ("R", s, k)), lengths,
                                               time_of=lambda s, k: 100.0 * s + k, order=order, pipelined=pipelined)
            assert done == sum(lengths) and sorted(where) == [s for s, n in enumerate(lengths) if n > 0]
            assert (ctx.calls[-1] == ("wait",)) == pipelined and ctx.calls.count(("wait",)) == int(pipelined)
            playing = [None] * 3                           # per slot: (sequence, next frame)
            runs = [0] * 3
            restarted = set()
            frames = 0
            for call in ctx.calls:
                if call[0] == "restart":
                    assert call[1] and not restarted & set(call[1])
                    restarted |= set(call[1])
                elif call[0] == "frames":
                    _, L, R, ts = call
                    for slot in range(3):
                        if L[slot] is None:
                            assert R[slot] is None and slot not in restarted
                            assert playing[slot] is None or playing[slot][1] == lengths[playing[slot][0]], "a slot is only empty after its sequence"
                            continue
                        _, s, k = L[slot]
                        assert R[slot] == ("R", s, k) and ts[slot] == 100.0 * s + k
                        if k == 0:
                            assert playing[slot] is None or playing[slot][1] == lengths[playing[slot][0]]
                            assert (slot in restarted) == (runs[slot] > 0), "restart before every sequence but the slot's first"
                            assert where[s] == (slot, runs[slot])
                            runs[slot] += 1
                            restarted.discard(slot)
                        else:
                            assert playing[slot] == (s, k) and slot not in restarted
                        playing[slot] = (s, k + 1)
                        frames += 1
                    assert not restarted, "a restarted slot gets the first frame of its next sequence in the same step"
            assert frames == done


def test_struct_layouts_and_null_ctx():
    assert C.sizeof(stereo_slam.RunInfo) == 4 * 4 + 4 + 6 * 4 == 44
    assert C.sizeof(stereo_slam.Memory) == 2 * 8 + 4 * 4 == 32
    lib = hip_lib.lib()
    invalid = -1                                          # SVO_ERR_INVALID
    n = C.c_int(7)
    assert lib.svo_ctx_restart_sequences(None, (C.c_int * 1)(0), 1) == invalid
    assert lib.svo_get_finished_runs(None, 0, C.byref(n)) == invalid and n.value == 7
    assert lib.svo_get_finished_run(None, 0, 0, None, None, 0, None) == invalid
    assert lib.svo_drop_finished_runs(None, -1) == invalid
    assert lib.svo_ctx_get_memory(None, C.byref(stereo_slam.Memory())) == invalid
    assert b"svo_ctx_get_memory" in lib.svo_last_error()
