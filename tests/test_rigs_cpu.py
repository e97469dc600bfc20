"""Host side of the camera rigs, without a GPU: the ctypes mirror of svo_rig against the header, the schedule of
sequences with a rig each (multi_seq.queue_schedule / play_queue, against a ctx that only records its calls), and
what the new entry points return without a device or a ctx."""
import ctypes as C
import os
import random
import re

from stereo_svo_slam_amd import hip_lib, multi_seq

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svo_hip.h")
EUROC = [2912, 1710, 2149, 2280, 2348, 1922]          # (the lengths and seeds of test_restart_cpu.py)


def test_rig_struct_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct svo_rig \{(.*?)\} svo_rig;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []                                           # (name, size, alignment) in declaration order
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if decl.startswith("const float *"):
            fields += [(n.strip(" *"), 8, 8) for n in decl[len("const float"):].split(",")]
        elif decl.startswith("float"):
            fields += [(n.strip(), 4, 4) for n in decl[len("float"):].split(",")]
        else:
            assert decl.startswith("int32_t"), decl
            fields += [(n.strip(), 4, 4) for n in decl[len("int32_t"):].split(",")]
    assert [f[0] for f in fields] == [n for n, _ in hip_lib.Rig._fields_]
    off = 0
    for name, size, align in fields:
        off = -(-off // align) * align
        assert getattr(hip_lib.Rig, name).offset == off and getattr(hip_lib.Rig, name).size == size, name
        off += size
    assert C.sizeof(hip_lib.Rig) == -(-off // 8) * 8 == 80
    assert [n for n, _ in hip_lib.Rig._fields_[:10]] == [n for n, _ in hip_lib.CameraSettings._fields_[:10]]
    r = hip_lib.Rig.from_dict(dict(baseline=1, fx=2, fy=3, cx=4, cy=5, k1=6, k2=7, k3=8, p1=9, p2=10, grid_width=40))
    assert [getattr(r, n) for n in hip_lib.RIG_FLOATS] == list(range(1, 11)) and not r.left_map_x and r.mem == 0


def _check_rig_schedule(lengths, n_slots, order, rigs):
    plain = multi_seq.queue_schedule(lengths, n_slots, order)
    steps = multi_seq.queue_schedule(lengths, n_slots, order, rigs)
    assert len(steps) == len(plain), "a rig costs no step"
    assert [[e[:3] for e in st] for st in steps] == plain, "the same schedule"
    bound = [0] * n_slots                                 # every slot starts on rig 0
    played = [False] * n_slots
    for st in steps:
        for slot, seq, k, rig, how in st:
            assert rig == rigs[seq]
            if k > 0:
                assert how is None and bound[slot] == rigs[seq], "every frame of a sequence under its rig"
                continue
            assert (how == "assign") == (rigs[seq] != bound[slot]), "assign exactly when the rig changes"
            assert (how == "restart") == (rigs[seq] == bound[slot] and played[slot])
            bound[slot], played[slot] = rigs[seq], True


def test_queue_schedule_with_rigs():
    rng = random.Random(0)
    cases = [(EUROC, n, None) for n in (1, 2, 3, 4, 6, 8)]
    for _ in range(600):
        lengths = [rng.randint(0, 40) for _ in range(rng.randint(0, 24))]
        cases.append((lengths, rng.randint(1, 9), None))
    rng = random.Random(1)
    for _ in range(300):
        lengths = [rng.randint(0, 30) for _ in range(rng.randint(1, 20))]
        order = list(range(len(lengths)))
        rng.shuffle(order)
        cases.append((lengths, rng.randint(1, 8), order))
    rng = random.Random(7)
    cases.append(([rng.randint(60, 240) for _ in range(768)], 256, None))
    for lengths, n_slots, order in cases:
        for n_rigs in (1, 2, 5):
            _check_rig_schedule(lengths, n_slots, order, [rng.randrange(n_rigs) for _ in lengths])
    assert multi_seq.queue_schedule([2, 1, 1], 2, [0, 1, 2], [1, 0, 0]) == \
        [[(0, 0, 0, 1, "assign"), (1, 1, 0, 0, None)], [(0, 0, 1, 1, None), (1, 2, 0, 0, "restart")]]


class _FakeCtx:
    """records what play_queue asks of a ctx"""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def restart(self, seqs):
        self.calls.append(("restart", list(seqs)))

    def assign_rigs(self, seqs, rigs):
        self.calls.append(("assign", list(seqs), list(rigs)))

    def new_images(self, L, R, ts):
        self.calls.append(("frames", list(L)))

    def pack_images(self, L, R, ts, borrow=False):
        return ("packed", list(L))

    def submit_packed(self, packed):
        self.calls.append(("frames", packed[1]))

    def wait(self):
        self.calls.append(("wait",))


def test_play_queue_takes_a_sequence_together_with_its_rig():
    lengths = [5, 2, 3, 1, 4, 2, 0, 3]
    rigs = [1, 1, 0, 2, 2, 0, 1, 1]
    for pipelined in (False, True):
        for order in (None, [3, 1, 0, 7, 2, 6, 5, 4]):
            ctx = _FakeCtx(3)
            where, done = multi_seq.play_queue(ctx, lambda s, k: (("L", s, k), ("R", s, k)), lengths, order=order,
                                               pipelined=pipelined, rigs=rigs)
            assert done == sum(lengths)
            bound, last, played, pending = [0] * 3, [0] * 3, [False] * 3, {}
            for call in ctx.calls:
                if call[0] == "restart":
                    for slot in call[1]:
                        assert slot not in pending
                        pending[slot] = None
                elif call[0] == "assign":
                    for slot, rig in zip(call[1], call[2]):
                        assert slot not in pending and rig != bound[slot]
                        pending[slot] = rig
                        bound[slot] = rig
                elif call[0] == "frames":
                    for slot, f in enumerate(call[1]):
                        if f is None:
                            continue
                        _, s, k = f
                        assert bound[slot] == rigs[s], "played under its rig"
                        if k == 0:
                            if rigs[s] != last[slot]:
                                assert pending.get(slot, "none") == rigs[s], "assigned where the rig differs"
                            elif played[slot]:
                                assert pending.get(slot, "none") is None, "restarted where it is the same"
                            else:
                                assert slot not in pending
                            pending.pop(slot, None)
                            played[slot], last[slot] = True, rigs[s]
                    assert not pending
    # without rigs the calls are what they were: no assignment
    ctx = _FakeCtx(3)
    multi_seq.play_queue(ctx, lambda s, k: (("L", s, k), ("R", s, k)), lengths)
    assert not [c for c in ctx.calls if c[0] == "assign"]


def test_entry_points_without_a_ctx_or_device():
    lib = hip_lib.lib()
    invalid = -1                                          # SVO_ERR_INVALID
    rig = hip_lib.Rig.from_dict(dict(baseline=20.0, fx=200.0, fy=200.0, cx=160.0, cy=120.0, k1=0, k2=0, k3=0, p1=0, p2=0))
    ids = (C.c_int * 1)(7)
    one = (C.c_int * 1)(0)
    n, b = C.c_int(7), C.c_int64(7)
    assert lib.svo_ctx_add_rigs(None, C.byref(rig), 1, ids) == invalid and ids[0] == 7
    assert b"svo_ctx_add_rigs" in lib.svo_last_error()
    assert lib.svo_ctx_remove_rigs(None, one, 1) == invalid
    assert lib.svo_ctx_assign_rigs(None, one, one, 1) == invalid
    assert lib.svo_ctx_get_slot_rig(None, 0, C.byref(n), None) == invalid and n.value == 7
    assert lib.svo_ctx_get_rigs(None, C.byref(n), C.byref(b)) == invalid and (n.value, b.value) == (7, 7)
    assert lib.svo_remap_linear_multi(None, 1, None, None, 1, None, None, None) == invalid
