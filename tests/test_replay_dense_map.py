"""replay --dump-dense-map / --scene-fused: the argument handling without a GPU, and on the GPU a 6-frame replay whose
PLY holds exactly the records export_voxel_maps gives a twin tracker that fused the same keyframes."""
import numpy as np
import pytest

from stereo_svo_slam_amd import hip_lib, replay, synth


def _args(*extra):
    return ["--synthetic", "tiny", "--frames", "2", *extra]


@pytest.mark.parametrize("extra", [
    ("--dump-dense-map", "m.ply"),                                                   # no voxel
    ("--dense-map-voxel", "0.1"),                                                    # a voxel and nothing that uses it
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "-0.1"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "nan"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "inf"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-log2", "9"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-log2", "27"),
    ("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1", "--dense-map-min-count", "-1"),
    ("--scene-fused", "0.1"),                                                        # no --dump-scene
    ("--dump-scene", "d", "--scene-fused", "0.1", "--dump-dense-map", "m.ply", "--dense-map-voxel", "0.2"),
])
def test_bad_arguments_end_before_anything_runs(extra, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        replay.main(_args(*extra))
    assert e.value.code == 2 and "error" in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


def test_good_arguments_parse():
    ap = replay.build_parser()
    a = ap.parse_args(_args("--dump-dense-map", "m.ply", "--dense-map-voxel", "0.05", "--dense-map-log2", "18", "--dense-map-min-count", "2",
                            "--cloud-step", "8", "--cloud-lr", "1.5", "--cloud-max-depth", "6"))
    replay.check_dense_map_args(ap, a)
    assert (a.dump_dense_map, a.dense_map_voxel, a.dense_map_log2, a.dense_map_min_count) == ("m.ply", 0.05, 18, 2)
    a = ap.parse_args(_args("--dump-scene", "d", "--scene-fused", "0.1"))
    replay.check_dense_map_args(ap, a)
    assert a.scene_fused == 0.1 and a.dense_map_log2 == 20 and a.scene_accumulate == 0
    a = ap.parse_args(_args("--dump-scene", "d", "--scene-fused", "0.1", "--dump-dense-map", "m.ply", "--dense-map-voxel", "0.1"))
    replay.check_dense_map_args(ap, a)


@pytest.mark.gpu
def test_the_ply_is_the_exported_map(tmp_path):
    from stereo_svo_slam_amd.stereo_slam import StereoSlam
    frames, step, max_depth, voxel, log2 = 6, 8, 6.0, 0.05, 16
    out = tmp_path / "map.ply"
    scenes = tmp_path / "scenes"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--dump-dense-map", str(out), "--dense-map-voxel", str(voxel),
                 "--dense-map-log2", str(log2), "--dense-map-min-count", "1", "--cloud-step", str(step), "--cloud-max-depth", str(max_depth),
                 "--dump-scene", str(scenes), "--scene-fused", str(voxel)])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    twin = StereoSlam(cfg)
    fused = 0
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        if k == 0:
            twin.set_voxel_maps(voxel, log2)
        fused += twin.fuse_new_keyframes(step=step, max_depth=max_depth) is not None
    want = twin.export_voxel_maps(None, min_count=1).points(0).copy()
    assert fused == int(twin.stats().n_keyframes) >= 1 and twin.get_voxel_map(min_count=1).tobytes() == want.tobytes()
    twin.close()
    v = replay.read_ply(out)
    assert len(v) == len(want) > 100
    assert all(v[k].tobytes() == want[k].tobytes() for k in ("x", "y", "z"))
    assert all(np.array_equal(v[k], want["color"][:, i]) for i, k in enumerate(("red", "green", "blue")))
    assert len(list(scenes.iterdir())) == frames
    # the fused map shows in the picture: the same replay without it draws other pixels
    plain = tmp_path / "plain"
    replay.main(["--synthetic", "tiny", "--frames", "2", "--dump-scene", str(plain)])
    assert (plain / "000001_scene.ppm").read_bytes() != (scenes / "000001_scene.ppm").read_bytes()
