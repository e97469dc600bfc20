"""filter_update_kernel in the form the tracker launches it (FilterArgs::kfs set: references gathered from a keyframe
table, results written back into the keyframes), through the diagnostic entry svo_filter_update_table_batch, whose
argument blocks are filled by the filling of the tracker's step. Every sequence of tests/filter_table_cases.py, alone
and in batches, under all 16 switch combinations, against the plain statement (which tests/test_filter_table_cpu.py
ties to the oracle), bit for bit, NaN equal to NaN. Every buffer of a launch (the frame's arrays, every keyframe
slab, the record table, the counters) lies in one block of device memory between bands of a canary byte; after the
launch the whole block is compared: outputs with the statement, everything else with what it held before."""
import copy

import numpy as np
import pytest
import torch

import filter_table_cases as TC
import geometry_cases as GC
from stereo_svo_slam_amd import hip_lib, synth

pytestmark = pytest.mark.gpu
CANARY, BAND, END_BAND = 0xA5, 2048, 16384
SLAB_PLANES = dict(kps2d="kps2d", kps3d="kps3d", flags="flags", outlier="outlier_count", inlier="inlier_count")
FRAME_PLANES = dict(kps2d="kps2d", kps3d="kps3d", flags="flags", outlier="outlier_count", inlier="inlier_count",
                    kf_inv_depth="kf_inv_depth", kf_variance="kf_variance", kf_id="kf_id", kp_index="kp_index")


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def hcam(cam):
    d = dict(synth.CONFIGS["euroc"])
    d.update(cam)
    return hip_lib.CameraSettings.from_dict(d)


class Arena:
    """host arrays laid out in one device block, a band of CANARY bytes before, between and behind them"""

    def __init__(self):
        self.items, self.size = {}, BAND

    def add(self, name, array):
        a = np.ascontiguousarray(array)
        assert name not in self.items and a.nbytes > 0
        self.items[name] = (self.size, a)
        self.size = (self.size + a.nbytes + 255) // 256 * 256 + BAND

    def upload(self):
        self.size += END_BAND
        self.before = np.full(self.size, CANARY, np.uint8)
        for off, a in self.items.values():
            self.before[off:off + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.dev = torch.from_numpy(self.before.copy()).cuda()
        return self

    def addr(self, name):
        return self.dev.data_ptr() + self.items[name][0]

    def download(self):
        self.after = self.dev.cpu().numpy()
        return self

    def got(self, name, before=False):
        off, a = self.items[name]
        return (self.before if before else self.after)[off:off + a.nbytes].view(a.dtype).reshape(a.shape)

    def check_bands(self, what):
        covered = np.zeros(self.size, bool)
        for off, a in self.items.values():
            covered[off:off + a.nbytes] = True
        bad = np.nonzero(~covered & (self.after != CANARY))[0]
        assert bad.size == 0, f"{what}: {bad.size} canary bytes written, the first at offset {bad[0]}"


def place(arena, b, seq):
    """the buffers of sequence b of a launch in the arena"""
    for key in TC.FRAME_KEYS:
        arena.add((b, "frame", key), seq["frame"][key])
    arena.add((b, "n"), np.array([seq["n"]], np.int32))
    arena.add((b, "frame_pose"), seq["frame_pose"])
    arena.add((b, "inside"), np.array([seq["inside0"]], np.int32))
    arena.add((b, "records"), np.full(len(seq["table"]) * hip_lib.keyframe_record_layout()["bytes"], 0x3C, np.uint8))
    for r, rec in enumerate(seq["table"]):
        if len(rec["flags"]):
            for key in TC.SLAB_KEYS:
                arena.add((b, "slab", r, key), rec[key])


def describe(arena, b, seq, **over):
    """sequence b as svo_filter_update_table_batch takes it"""
    kfs = []
    for r, rec in enumerate(seq["table"]):
        kf = dict(pose=rec["pose"], n=len(rec["flags"]))
        if len(rec["flags"]):
            kf.update({plane: arena.addr((b, "slab", r, key)) for key, plane in SLAB_PLANES.items()})
        kfs.append(kf)
    kps = {plane: arena.addr((b, "frame", key)) for key, plane in FRAME_PLANES.items()}
    kps["n"] = arena.addr((b, "n"))
    d = dict(cam=hcam(seq["cam"]), kps=kps, frame_pose=arena.addr((b, "frame_pose")),
             disparity=arena.addr((b, "frame", "disparity")), kfs=kfs, records=arena.addr((b, "records")),
             records_bytes=arena.items[(b, "records")][1].nbytes, kf_mask=seq["kf_mask"], width=seq["width"],
             height=seq["height"], inside_count=arena.addr((b, "inside")))
    d.update(over)
    return d


def expected_records(arena, b, seq):
    """the bytes of the record table after the entry filled it: pose, n and the five array pointers, all else 0"""
    L = hip_lib.keyframe_record_layout()
    out = np.zeros((len(seq["table"]), L["bytes"]), np.uint8)
    for r, rec in enumerate(seq["table"]):
        out[r, L["pose"]:L["pose"] + 24] = rec["pose"].view(np.uint8)
        out[r, L["n"]:L["n"] + 4] = np.array([len(rec["flags"])], np.int32).view(np.uint8)
        if len(rec["flags"]):
            for key, plane in SLAB_PLANES.items():
                o = L["planes"][plane]
                out[r, o:o + 8] = np.array([arena.addr((b, "slab", r, key))], np.uint64).view(np.uint8)
    return out.reshape(-1)


def launch(H, seqs, switches=(1, 1, 1, 1), n_bound=None):
    arena = Arena()
    for b, seq in enumerate(seqs):
        place(arena, b, seq)
    arena.upload()
    n_bound = max(s["cap"] for s in seqs) if n_bound is None else n_bound
    H.filter_update_table_batch([describe(arena, b, s) for b, s in enumerate(seqs)], n_bound, *switches)
    return arena.download()


def equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.nonzero(~GC.same_bits(got, want).reshape(len(got), -1).all(axis=1))[0] if got.size else np.zeros(0, int)
    assert bad.size == 0, f"{what}: entries {bad[:8]}: {got[bad[:4]]} against {want[bad[:4]]}"


def check(arena, b, seq, ref, what):
    """every buffer of sequence b after the launch: outputs against the statement `ref`, with no keypoint exempt;
    inputs, tails, unreferenced keyframe points and the record table byte for byte"""
    n = seq["n"]
    for key in TC.FRAME_KEYS:
        got = arena.got((b, "frame", key))
        equal(got, ref["frame"][key], f"{what}: the frame's {key}")
        assert got[n:].tobytes() == seq["frame"][key][n:].tobytes(), f"{what}: the frame's {key} behind n"
        if key not in TC.FRAME_OUT:
            assert got.tobytes() == seq["frame"][key].tobytes(), f"{what}: {key} is an input"
    for name in ("n", "frame_pose"):
        assert arena.got((b, name)).tobytes() == arena.got((b, name), before=True).tobytes(), f"{what}: {name} is an input"
    assert int(arena.got((b, "inside"))[0]) == ref["inside"], (what, arena.got((b, "inside")), ref["inside"])
    named = {(int(i) & seq["kf_mask"], int(k)) for i, k in zip(seq["frame"]["kf_id"][:n], seq["frame"]["kp_index"][:n])}
    for r, rec in enumerate(seq["table"]):
        for key in TC.SLAB_KEYS if len(rec["flags"]) else ():
            got = arena.got((b, "slab", r, key))
            equal(got, ref["table"][r][key], f"{what}: record {r}: {key}")
            free = [k for k in range(len(rec["flags"])) if (r, k) not in named]
            assert got[free].tobytes() == rec[key][free].tobytes(), f"{what}: record {r}: {key} of a point no keypoint names"
        assert ref["table"][r]["pose"].tobytes() == rec["pose"].tobytes()
    assert arena.got((b, "records")).tobytes() == expected_records(arena, b, seq).tobytes(), f"{what}: the record table"


def outputs(arena, b, seq):
    """the bytes of everything a launch may write for sequence b"""
    out = {("frame", key): arena.got((b, "frame", key)).tobytes() for key in TC.FRAME_KEYS}
    out["inside"] = arena.got((b, "inside")).tobytes()
    for r, rec in enumerate(seq["table"]):
        for key in TC.SLAB_KEYS if len(rec["flags"]) else ():
            out[("slab", r, key)] = arena.got((b, "slab", r, key)).tobytes()
    return out


LONE = {}


def lone(H, seq):
    if seq["name"] not in LONE:
        arena = launch(H, [seq])
        check(arena, 0, seq, TC.results()[seq["name"]], f"{seq['name']} alone")
        arena.check_bands(seq["name"])
        LONE[seq["name"]] = outputs(arena, 0, seq)
    return LONE[seq["name"]]


# ------------------------------------------------------------------ every sequence, one per launch
def test_every_sequence_alone(H):
    for seq in TC.sequences():
        lone(H, seq)
    assert len(LONE) == len(TC.sequences()) >= 30


def test_the_grid_may_be_cut_to_the_count(H):
    """the tracker bounds the grid by last frame's count: n_bound = n, and 1 for a sequence without keypoints"""
    for name in ("n64_ring_6789_reversed", "n65_plain_0_2_3_sparse", "n130_three_reversed", "n0_one_reversed"):
        seq = TC.sequence(name)
        arena = launch(H, [seq], n_bound=max(seq["n"], 1))
        check(arena, 0, seq, TC.results()[name], f"{name} with n_bound = n")
        arena.check_bands(name)


# ------------------------------------------------------------------ the four switches
@pytest.mark.parametrize("switches", TC.ALL_SWITCHES)
def test_every_switch_combination(H, switches):
    seq, ref = TC.switch_sequence(), TC.switch_results()[switches]
    arena = launch(H, [seq], switches)
    check(arena, 0, seq, ref, f"switches {switches}")
    arena.check_bands(f"switches {switches}")
    if not switches[2]:
        for r, rec in enumerate(seq["table"]):
            for key in TC.SLAB_KEYS if len(rec["flags"]) else ():
                assert arena.got((0, "slab", r, key)).tobytes() == rec[key].tobytes(), \
                    f"{switches}: without do_flags no keyframe byte changes (record {r}, {key})"
        assert arena.got((0, "frame", "flags")).tobytes() == seq["frame"]["flags"].tobytes()
    if not switches[3]:
        assert arena.got((0, "frame", "kps2d")).tobytes() == seq["frame"]["kps2d"].tobytes()
        assert int(arena.got((0, "inside"))[0]) == seq["inside0"]


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("name", sorted(TC.BATCHES))
def test_batch_equals_the_statement_and_each_sequence_alone(H, name):
    seqs = [TC.sequence(n) for n in TC.BATCHES[name]]
    arena = launch(H, seqs)
    nothing_inside = 0
    for b, seq in enumerate(seqs):
        ref = TC.results()[seq["name"]]
        check(arena, b, seq, ref, f"batch {name} sequence {b} ({seq['name']})")
        assert outputs(arena, b, seq) == lone(H, seq), f"batch {name} sequence {b} ({seq['name']}) differs from its lone launch"
        nothing_inside += seq["n"] > 0 and ref["inside"] == seq["inside0"]
    arena.check_bands(f"batch {name}")
    assert name != "counts" or nothing_inside >= 1


# ------------------------------------------------------------------ bad calls
BAD_CALLS = ("a ring of three records", "a ring mask one bit short", "a ring mask of eight for four records", "no records",
             "more records than the table holds", "a record table that is not 8-byte aligned", "no record table",
             "no frame pose", "no disparities", "a frame array missing", "a keyframe array missing",
             "a keyframe of negative length", "a count beyond n_bound", "a negative count", "a negative keyframe id",
             "an id whose record is vacant", "an id beyond a table indexed as it is", "an index beyond its keyframe",
             "a negative index", "a bad sequence behind a good one", "no sequences")


def bad_call(what):
    """(sequences of the launch, n_bound or None, what is wrong with the last sequence's description)"""
    good, other = TC.sequence("n1_ring_567_sparse"), TC.sequence("ring_12_13")
    three = TC.sequence("n63_three_strided")

    def edited(seq, **arrays):
        s = copy.deepcopy(seq)
        for key, (i, v) in arrays.items():
            s["frame"][key][i] = v
        return s
    return {
        "a ring of three records": ([three], None, dict(kf_mask=2)),
        "a ring mask one bit short": ([good], None, dict(kf_mask=1)),
        "a ring mask of eight for four records": ([good], None, dict(kf_mask=7)),
        "no records": ([good], None, dict(table=0)),
        "more records than the table holds": ([good], None, dict(records_bytes=3 * hip_lib.keyframe_record_layout()["bytes"])),
        "a record table that is not 8-byte aligned": ([good], None, "misaligned_records"),
        "no record table": ([good], None, dict(records=0)),
        "no frame pose": ([good], None, dict(frame_pose=0)),
        "no disparities": ([good], None, dict(disparity=0)),
        "a frame array missing": ([good], None, "no_kps3d"),
        "a keyframe array missing": ([good], None, "no_slab_flags"),
        "a keyframe of negative length": ([good], None, "negative_slab"),
        "a count beyond n_bound": ([other], other["n"] - 1, {}),
        "a negative count": ([good], None, "negative_n"),
        "a negative keyframe id": ([edited(other, kf_id=(3, -4))], None, {}),
        "an id whose record is vacant": ([edited(good, kf_id=(0, 8))], None, {}),
        "an id beyond a table indexed as it is": ([edited(three, kf_id=(5, 3))], None, {}),
        "an index beyond its keyframe": ([edited(other, kp_index=(7, 4000))], None, {}),
        "a negative index": ([edited(other, kp_index=(0, -1))], None, {}),
        "a bad sequence behind a good one": ([other, good], None, dict(kf_mask=1)),
        "no sequences": ([], None, {}),
    }[what]


@pytest.mark.parametrize("what", BAD_CALLS)
def test_bad_calls_are_refused_with_device_memory_untouched(H, what):
    seqs, n_bound, over = bad_call(what)
    arena = Arena()
    for b, seq in enumerate(seqs):
        place(arena, b, seq)
    arena.add("spare", np.zeros(16, np.uint8))
    arena.upload()
    descs = [describe(arena, b, s) for b, s in enumerate(seqs)]
    if isinstance(over, dict):
        if descs:
            descs[-1].update(over)
    elif over == "misaligned_records":
        descs[-1]["records"] += 4
        descs[-1]["records_bytes"] -= 4
    elif over == "no_kps3d":
        descs[-1]["kps"]["kps3d"] = None
    elif over == "no_slab_flags":
        [kf for kf in descs[-1]["kfs"] if kf["n"]][0]["flags"] = None
    elif over == "negative_slab":
        descs[-1]["kfs"][1]["n"] = -1
    elif over == "negative_n":
        o = arena.items[(0, "n")][0]
        arena.dev[o:o + 4] = 0xFF
        arena.before[o:o + 4] = 0xFF
    n_bound = max([s["cap"] for s in seqs] + [1]) if n_bound is None else n_bound
    with pytest.raises(hip_lib.SvoError):
        H.filter_update_table_batch(descs, n_bound)
    arena.download()
    assert arena.after.tobytes() == arena.before.tobytes(), f"{what}: device memory changed"


def test_null_arrays_are_accepted_where_nothing_reads_them(H):
    """without the outlier check no disparity is read; the counter is optional"""
    seq = TC.switch_sequence()
    arena = Arena()
    place(arena, 0, seq)
    arena.upload()
    H.filter_update_table_batch([describe(arena, 0, seq, disparity=None, inside_count=None)], seq["cap"], 0, 1, 1, 1)
    arena.download()
    ref = TC.switch_results()[(0, 1, 1, 1)]
    for key in TC.FRAME_OUT:
        equal(arena.got((0, "frame", key)), ref["frame"][key], f"no counter: the frame's {key}")
    assert int(arena.got((0, "inside"))[0]) == seq["inside0"]
    arena.check_bands("no counter")
