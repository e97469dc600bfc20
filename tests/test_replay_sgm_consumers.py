"""replay --dense-map-sgm, --scene-dense-sgm and --ar-sgm: each writes what the run without the flag writes, from the
clouds of the SGM map: the fused map is the map of a twin tracker that fuses with sgm=, the pictures differ from the
winner-takes-all ones, and each flag is refused with a plain message when the settings' search_x exceeds 63."""
import os

import pytest

from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam

P1, P2, CAP = 32, 256, 2047
SGM = f"{P1},{P2},{CAP}"
BASE = ["--synthetic", "tiny", "--seed", "3"]


@pytest.mark.gpu
def test_dense_map_sgm_writes_the_map_of_the_sgm_clouds(tmp_path):
    frames, step, voxel, log2, lr = 4, 8, 0.1, 14, 1.0
    common = BASE + ["--frames", str(frames), "--cloud-step", str(step), "--cloud-lr", str(lr), "--dense-map-voxel", str(voxel),
                     "--dense-map-log2", str(log2)]
    replay.main(common + ["--dump-dense-map", str(tmp_path / "wta.ply")])
    replay.main(common + ["--dump-dense-map", str(tmp_path / "sgm.ply"), "--dense-map-sgm", SGM])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 3, device="cpu")
    twin = StereoSlam(cfg)
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        if k == 0:
            twin.set_voxel_maps(voxel, log2)
        twin.fuse_new_keyframes(step=step, sgm=dict(p1=P1, p2=P2, cost_cap=CAP, lr_check=lr))
    points = twin.get_voxel_map()
    twin.close()
    replay.write_ply(tmp_path / "twin.ply", points)
    assert len(points) > 100 and (tmp_path / "sgm.ply").read_bytes() == (tmp_path / "twin.ply").read_bytes()
    assert (tmp_path / "sgm.ply").read_bytes() != (tmp_path / "wta.ply").read_bytes() and len(replay.read_ply(tmp_path / "wta.ply")) > 100


@pytest.mark.gpu
def test_scene_dense_sgm_and_ar_sgm_write_other_pictures(tmp_path):
    frames = 3
    scene = BASE + ["--frames", str(frames), "--scene-dense", "8", "--scene-dense-lr", "1.0", "--scene-accumulate", "4000"]
    replay.main(scene + ["--dump-scene", str(tmp_path / "scene_wta")])
    replay.main(scene + ["--dump-scene", str(tmp_path / "scene_sgm"), "--scene-dense-sgm", SGM])
    ar = BASE + ["--frames", str(frames), "--ar-box", "0.8", "--ar-at", "0,1.6,4", "--ar-occlude", "4", "--ar-margin", "0.05", "--ar-lr", "1.0"]
    replay.main(ar + ["--dump-ar", str(tmp_path / "ar_wta")])
    replay.main(ar + ["--dump-ar", str(tmp_path / "ar_sgm"), "--ar-sgm", f"{P1},{P2}"])
    for kind in ("scene", "ar"):
        names = [f"{k:06d}_{kind}.ppm" for k in range(frames)]
        assert sorted(os.listdir(tmp_path / f"{kind}_wta")) == sorted(os.listdir(tmp_path / f"{kind}_sgm")) == names
        pairs = [((tmp_path / f"{kind}_wta" / n).read_bytes(), (tmp_path / f"{kind}_sgm" / n).read_bytes()) for n in names]
        assert all(len(a) == len(b) > 1000 for a, b in pairs) and any(a != b for a, b in pairs), kind


@pytest.mark.parametrize("flags", (["--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-sgm", SGM],
                                   ["--dump-scene", "scene", "--scene-dense", "8", "--scene-dense-sgm", SGM],
                                   ["--dump-ar", "ar", "--ar-occlude", "4", "--ar-sgm", SGM]))
def test_a_search_beyond_63_is_refused(flags, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setitem(synth.CONFIGS, "tiny", dict(synth.CONFIGS["tiny"], search_x=64))
    with pytest.raises(SystemExit) as e:
        replay.main(BASE + ["--frames", "1"] + flags)
    err = capsys.readouterr().err
    assert e.value.code == 2 and flags[-2] in err and "search_x <= 63" in err and "64" in err
    assert os.listdir(tmp_path) == []                                       # refused before anything ran or was written


def test_the_flags_need_what_they_switch(capsys):
    for flags, needs in ((["--dense-map-sgm", SGM], "--dump-dense-map"), (["--scene-dense-sgm", SGM], "--scene-dense"), (["--ar-sgm", SGM], "--ar-occlude")):
        with pytest.raises(SystemExit):
            replay.main(BASE + ["--frames", "1"] + flags)
        assert f"{flags[0]} needs {needs}" in capsys.readouterr().err
    for name in ("--dense-map-sgm", "--scene-dense-sgm", "--ar-sgm"):
        assert "search_x <= 63" in " ".join(a.help for a in replay.build_parser()._actions if name in a.option_strings)
    assert hip_lib.SGM_DEFAULTS["cost_cap"] == 4095                         # (what P1,P2 without CAP stands for)
