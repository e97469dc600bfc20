"""The oracle's depth filter over a keyframe table (svo_o_filter_table, the block that svo_o_slam_new_image runs)
against the plain statement of tests/filter_table_cases.py, bit for bit (NaN equal to NaN), on every sequence that
tests/test_filter_table_gpu.py launches; the sequences reach every situation they are there for and every label of
geometry_cases.FILTER_LABELS, asserted by name; and the frame outputs of the table form equal those of the
explicit-form statement on the gathered references, which tests/test_geometry_cpu.py holds to its float64 twin."""
import numpy as np
import pytest

import filter_table_cases as TC
import geometry_cases as GC
import oracle_py as O
from test_geometry_cpu import ocam, same


def oracle_table(seq, switches=(1, 1, 1, 1)):
    """the sequence through svo_o_filter_table: (frame arrays of n entries, table, the counter's word)"""
    n = seq["n"]
    fr = {k: seq["frame"][k][:n] for k in TC.FRAME_OUT}
    frame, table, inside = O.filter_table(fr, seq["frame"]["kf_id"][:n], seq["frame"]["kp_index"][:n], seq["table"],
                                          seq["kf_mask"], seq["frame"]["disparity"][:n], seq["frame_pose"],
                                          ocam(seq["cam"]), switches, seq["width"], seq["height"])
    return frame, table, seq["inside0"] + inside


def check(seq, switches, ref):
    what = f"{seq['name']} {switches}"
    n = seq["n"]
    frame, table, inside = oracle_table(seq, switches)
    for key in TC.FRAME_OUT:
        same(frame[key], ref["frame"][key][:n], f"{what}: the frame's {key}")
    assert len(table) == len(ref["table"])
    for r, (got, want) in enumerate(zip(table, ref["table"])):
        for key in TC.TABLE_KEYS:
            same(got[key], want[key], f"{what}: record {r}: {key}")
    assert inside == ref["inside"], (what, inside, ref["inside"])


def test_oracle_equals_the_statement_on_every_sequence():
    res = TC.results()
    for seq in TC.sequences():
        check(seq, (1, 1, 1, 1), res[seq["name"]])


@pytest.mark.parametrize("switches", TC.ALL_SWITCHES)
def test_oracle_equals_the_statement_under_every_switch_combination(switches):
    seq, ref = TC.switch_sequence(), TC.switch_results()[switches]
    check(seq, switches, ref)
    n = seq["n"]
    if not switches[2]:
        for got, was in zip(ref["table"], seq["table"]):
            for key in TC.TABLE_KEYS:
                assert got[key].tobytes() == was[key].tobytes(), f"{switches}: without do_flags no keyframe byte changes ({key})"
        assert np.array_equal(ref["frame"]["flags"], seq["frame"]["flags"])
    if not switches[3]:
        assert ref["frame"]["kps2d"].tobytes() == seq["frame"]["kps2d"].tobytes() and ref["inside"] == seq["inside0"]
    else:
        assert ref["inside"] > seq["inside0"]
    if switches[2]:       # the write-back is tied to do_flags, whatever the update does
        changed = sum(got[key].tobytes() != was[key].tobytes() for got, was in zip(ref["table"], seq["table"])
                      for key in TC.SLAB_KEYS)
        assert changed > 0, switches
    assert all(ref["frame"][k][n:].tobytes() == seq["frame"][k][n:].tobytes() for k in TC.FRAME_KEYS)


def test_every_situation_and_every_label_is_reached():
    seqs = TC.sequences()
    got = set().union(*[TC.reached(s) for s in seqs])
    for name in TC.SITUATIONS:
        assert name in got, f"no sequence reaches the situation `{name}`"
    assert {n for s in seqs for n in [s["n"]]} >= set(TC.COUNTS)
    for tname, (ids, mask, records) in TC.TABLES.items():
        assert any(tuple(s["ids"]) == ids and s["kf_mask"] == mask and len(s["table"]) == records for s in seqs), tname
    # the disagreeing copies must each be seen by a sequence whose write-back runs over two workgroups and a ring
    for name in ("keep_bit_keyframe_only", "keep_bit_frame_only", "temporary_differs", "completely_differs",
                 "counter_disagreement", "kps3d_disagreement", "unreferenced_point"):
        assert any({name, "wrap", "two_workgroups"} <= TC.reached(s) for s in seqs), name
    labels = set().union(*[r["labels"] for r in TC.results().values()])
    for name in GC.FILTER_LABELS:
        assert name in labels, f"no sequence reaches the label `{name}` in table form"
    explicit = set().union(*[r[(1, 1)]["labels"] for r in GC.filter_results().values()])
    assert set(GC.FILTER_LABELS) & explicit <= labels
    for sw in TC.ALL_SWITCHES:
        assert sw in TC.switch_results()
    for names in TC.BATCHES.values():
        counts = [TC.sequence(n)["n"] for n in names]
        assert len(names) >= 5 and 0 in counts and len(set(counts)) >= 4
    rings = [TC.sequence(n) for n in TC.BATCHES["rings"]]
    assert all(s["kf_mask"] != -1 for s in rings) and len({tuple(s["ids"]) for s in rings}) >= 4


def test_frame_outputs_equal_the_explicit_form_statement():
    """what the table form adds is the gather and the scatter: on the gathered references the frame's outputs are
    those of geometry_cases.filter_ref"""
    res = TC.results()
    for seq in TC.sequences():
        n = seq["n"]
        rec, idx, ref3d, ref2d, kf_pose = TC.gather(seq)
        c = seq["explicit"]
        same(ref3d, c["ref3d"], f"{seq['name']}: gathered ref3d")
        same(ref2d, c["ref2d"], f"{seq['name']}: gathered ref2d")
        same(kf_pose, c["kf_pose"].reshape(n, 6), f"{seq['name']}: gathered keyframe poses")
        if n == 0:
            continue
        want, got = TC.explicit_ref(seq, (1, 1, 1, 1)), res[seq["name"]]
        for key in TC.FRAME_OUT:
            same(got["frame"][key][:n], want[key], f"{seq['name']}: the frame's {key}")
        assert got["inside"] - seq["inside0"] == want["inside"], seq["name"]
    seq = TC.switch_sequence()
    for sw, got in TC.switch_results().items():
        want = TC.explicit_ref(seq, sw)
        for key in ("kps3d", "outlier", "inlier", "kf_inv_depth", "kf_variance") + (("flags",) if sw[2] else ()) + \
                (("kps2d",) if sw[3] else ()):
            same(got["frame"][key][:seq["n"]], want[key], f"switches {sw}: the frame's {key}")


def test_the_scatter_is_what_the_reference_writes():
    """on the ring that wraps: a keyframe entry named by keypoint i holds the frame's kps3d, counters, TEMPORARY and
    COMPLETELY and its own DURING_REFINEMENT bit; every other entry, and every pose, holds its bytes"""
    seq = TC.sequence("n130_ring_6789_sparse")
    ref = TC.results()[seq["name"]]
    n = seq["n"]
    rec, idx, *_ = TC.gather(seq)
    named = set(zip(rec, idx))
    for i, (r, k) in enumerate(zip(rec, idx)):
        got, was = ref["table"][r], seq["table"][r]
        assert got["kps3d"][k].tobytes() == ref["frame"]["kps3d"][i].tobytes()
        assert got["outlier"][k] == ref["frame"]["outlier"][i] and got["inlier"][k] == ref["frame"]["inlier"][i]
        assert got["flags"][k] & 1 == was["flags"][k] & 1 and got["flags"][k] & 6 == ref["frame"]["flags"][i] & 6
        assert got["kps2d"][k].tobytes() == was["kps2d"][k].tobytes()
    for r, (got, was) in enumerate(zip(ref["table"], seq["table"])):
        assert got["pose"].tobytes() == was["pose"].tobytes()
        for k in range(len(was["flags"])):
            if (r, k) not in named:
                assert all(got[key][k].tobytes() == was[key][k].tobytes() for key in TC.SLAB_KEYS), (r, k)
    assert n == 130 and len(named) == n
