"""What the cases of size_cases.py reach, asserted from the oracle alone (no GPU): a later change of a seed,
a preset or the renderer cannot quietly empty a case that test_sizes_gpu.py plays through the HIP ctx."""
import numpy as np
import pytest

import oracle_py as O
import size_cases as S
import snapshot_ref


def test_widths_cover_every_dword_remainder():
    assert {S.config(n)["width"] % 4 for n in S.CASES} >= {1, 2, 3}
    assert any(S.config(n)["width"] % 2 == 0 and (S.config(n)["width"] // 2) % 2 == 1 for n in S.CASES)


def test_the_two_rounding_rules_disagree_on_a_used_level():
    """halfSample (w >> l) against pyrDown ((w + 1) / 2 per level), on a level both pyramids of the case have"""
    in_w = in_h = False
    for name in S.CASES:
        cfg = S.config(name)
        n = min(cfg["max_pyramid_levels"], snapshot_ref.lk_levels(cfg))
        for (fw, fh), (cw, ch) in zip(S.floor_dims(cfg)[:n], S.ceil_dims(cfg, n)):
            in_w |= fw != cw
            in_h |= fh != ch
    assert in_w and in_h


def test_lk_level_counts_cover_three_two_one_and_the_oracle_agrees():
    counts = {}
    for name in S.CASES:
        cfg, L, R, ts = S.sequence(name, 1)
        counts[name] = snapshot_ref.lk_levels(cfg)
        pyr = O.build_lk_pyramid(L[0], cfg["window_size_opt_flow"], 3)
        assert len(pyr) == counts[name], name
        assert [p.shape[::-1] for p in pyr] == S.ceil_dims(cfg, counts[name]), name
    assert set(counts.values()) == {3, 2, 1}, counts
    assert counts["lk2_167"] == 2 and counts["lk1_61"] == 1


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_tracks_and_makes_keyframes(name):
    frames, keyframes = S.oracle_run(name)
    cfg = S.config(name)
    made = [k for k, f in enumerate(frames) if f[0]]
    counts = [len(f[1]) for f in frames]
    levels = sorted({int(l) for f in frames for l in f[3]["level"]})
    print(f"{name}: keyframes at {made}, keypoints {counts[0]} then {min(counts[1:])}..{max(counts[1:])}, levels {levels}")
    assert made[0] == 0 and len(keyframes) == len(made)
    assert min(counts) > 0, "the track was lost"
    if name != "euroc749":
        assert len(made) >= 3, made                          # at least two keyframes after frame 0
    for f in frames[1:]:                                     # every later frame was tracked: the GN ran
        assert f[5].reproj_trace.n_gradient > 0


def test_dense_case_passes_128_keypoints_and_leaves_the_image():
    frames, _ = S.oracle_run("dense327")
    cfg = S.config("dense327")
    assert max(len(f[1]) for f in frames) > 128
    outside = [k for k, f in enumerate(frames)
               if len(f[1]) and (f[1][:, 0].min() < 0 or f[1][:, 1].min() < 0 or
                                 f[1][:, 0].max() >= cfg["width"] or f[1][:, 1].max() >= cfg["height"])]
    assert outside, "no keypoint outside the image on any frame"


def test_partial_cells_and_the_swapped_merge_grid():
    cfg = S.config("cells321")
    assert cfg["width"] % cfg["grid_width"] and cfg["height"] % cfg["grid_height"]
    cells, merge = S.grid_cells(cfg)
    assert cells != merge, (cells, merge)
