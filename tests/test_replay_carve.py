"""replay --dense-map-carve: the argument handling without a GPU, and on the GPU a short synthetic replay whose carved
dense map holds a part, and only voxels, of the map the same replay dumps without a carve, with the winner-takes-all
cloud and with --dense-map-sgm."""
import numpy as np
import pytest

import voxel_ref as VR
from stereo_svo_slam_amd import replay

VOXEL = 0.1


def _args(*extra):
    return ["--synthetic", "tiny", "--frames", "2", *extra]


@pytest.mark.parametrize("extra", [
    ("--dense-map-carve", "0.2"),                                                    # no map to carve
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-carve", "-1"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-carve", "nan"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-carve", "inf"),
])
def test_bad_arguments_end_before_anything_runs(extra, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        replay.main(_args(*extra))
    assert e.value.code == 2 and "error" in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


def test_good_arguments_parse():
    ap = replay.build_parser()
    a = ap.parse_args(_args("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.05", "--dense-map-carve", "0.25", "--dense-map-sgm", "32,256"))
    replay.check_dense_map_args(ap, a)
    assert a.dense_map_carve == 0.25 and a.dense_map_sgm == "32,256"
    a = ap.parse_args(_args("--dump-scene", "d", "--scene-fused", "0.1", "--dense-map-carve", "0"))
    replay.check_dense_map_args(ap, a)
    assert a.dense_map_carve == 0.0
    assert ap.parse_args(_args("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.05")).dense_map_carve is None


def _voxels(path):
    v = replay.read_ply(path)
    rec = VR.records(np.stack([v["x"], v["y"], v["z"]], 1))
    _, inside, key, _ = VR.classify(rec, VOXEL, 0)
    assert inside.all() and len(set(key.tolist())) == len(key)
    return set(key.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("sgm", [(), ("--dense-map-sgm", "32,256")])
def test_a_carved_map_is_a_part_of_the_whole(tmp_path, sgm):
    common = ["--synthetic", "tiny", "--frames", "6", "--dense-map-voxel", str(VOXEL), "--dense-map-log2", "16", "--cloud-step", "8", *sgm]
    whole, carved = tmp_path / "whole.ply", tmp_path / "carved.ply"
    replay.main(common + ["--dump-dense-map", str(whole)])
    replay.main(common + ["--dump-dense-map", str(carved), "--dense-map-carve", "0.0"])
    a, b = _voxels(whole), _voxels(carved)
    assert b <= a and 0 < len(b) <= len(a)
