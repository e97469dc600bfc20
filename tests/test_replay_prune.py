"""replay --dense-map-window / --dense-map-keep: the argument handling without a GPU, and on the GPU a short synthetic
replay whose windowed dense map holds a part, and only voxels, of the map the same replay dumps without a window."""
import numpy as np
import pytest

import voxel_ref as VR
from stereo_svo_slam_amd import replay

VOXEL = 0.1


def _args(*extra):
    return ["--synthetic", "tiny", "--frames", "2", *extra]


@pytest.mark.parametrize("extra", [
    ("--dense-map-window", "2.0"),                                                   # no map to prune
    ("--dense-map-keep", "3"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-window", "-1"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-window", "nan"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-window", "inf"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-keep", "0"),
])
def test_bad_arguments_end_before_anything_runs(extra, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        replay.main(_args(*extra))
    assert e.value.code == 2 and "error" in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


def test_good_arguments_parse():
    ap = replay.build_parser()
    a = ap.parse_args(_args("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.05", "--dense-map-window", "2.5", "--dense-map-keep", "4"))
    replay.check_dense_map_args(ap, a)
    assert (a.dense_map_window, a.dense_map_keep) == (2.5, 4)
    a = ap.parse_args(_args("--dump-scene", "d", "--scene-fused", "0.1", "--dense-map-window", "0"))
    replay.check_dense_map_args(ap, a)
    assert a.dense_map_window == 0.0 and a.dense_map_keep is None
    a = ap.parse_args(_args("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.05"))
    assert a.dense_map_window is None and a.dense_map_keep is None


def _voxels(path):
    """the keys of the voxels a dumped map's records lie in"""
    v = replay.read_ply(path)
    rec = VR.records(np.stack([v["x"], v["y"], v["z"]], 1))
    _, inside, key, _ = VR.classify(rec, VOXEL, 0)
    assert inside.all() and len(set(key.tolist())) == len(key)                       # a record per voxel
    return set(key.tolist())


@pytest.mark.gpu
def test_a_windowed_map_is_a_part_of_the_whole(tmp_path):
    common = ["--synthetic", "tiny", "--frames", "6", "--dense-map-voxel", str(VOXEL), "--dense-map-log2", "16", "--cloud-step", "8"]
    whole, window, kept = tmp_path / "whole.ply", tmp_path / "window.ply", tmp_path / "kept.ply"
    replay.main(common + ["--dump-dense-map", str(whole)])
    replay.main(common + ["--dump-dense-map", str(window), "--dense-map-window", "5.0"])
    replay.main(common + ["--dump-dense-map", str(kept), "--dense-map-keep", "1", "--dense-map-window", "1000"])
    a, b, c = _voxels(whole), _voxels(window), _voxels(kept)
    assert 0 < len(b) < len(a) and b < a                                             # the window took voxels away, and added none
    assert 0 < len(c) <= len(a) and c <= a
