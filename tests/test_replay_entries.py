"""replay --save-dense-map / --load-dense-map / --dense-map-grow: the argument handling without a GPU, and on the GPU a
6-frame replay whose saved file holds exactly the entries of a twin tracker that fused the same keyframes, a second run
that loads it and ends with every count doubled (the same frames fused into yesterday's map), and a map of 1 << 10
entries that the first keyframe's cloud overfills and --dense-map-grow moves into a larger table."""
import numpy as np
import pytest

from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.jobs import VoxelSaves


def _args(*extra):
    return ["--synthetic", "tiny", "--frames", "2", *extra]


@pytest.mark.parametrize("extra", [
    ("--save-dense-map", "m.svx"),                                                   # no voxel
    ("--load-dense-map", "m.svx"),
    ("--dense-map-grow", "20"),
    ("--save-dense-map", "m.svx", "--dense-map-voxel", "0.1", "--dense-map-log2", "12", "--dense-map-grow", "11"),
    ("--save-dense-map", "m.svx", "--dense-map-voxel", "0.1", "--dense-map-grow", "27"),
])
def test_bad_arguments_end_before_anything_runs(extra, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        replay.main(_args(*extra))
    assert e.value.code == 2 and "error" in capsys.readouterr().err
    assert list(tmp_path.iterdir()) == []


def test_good_arguments_parse():
    ap = replay.build_parser()
    a = ap.parse_args(_args("--save-dense-map", "a.svx", "--load-dense-map", "b.svx", "--dense-map-voxel", "0.05", "--dense-map-log2", "12",
                            "--dense-map-grow", "14"))
    replay.check_dense_map_args(ap, a)
    assert (a.save_dense_map, a.load_dense_map, a.dense_map_grow, a.dump_dense_map) == ("a.svx", "b.svx", 14, None)


@pytest.mark.gpu
def test_a_run_continues_the_saved_map(tmp_path):
    from stereo_svo_slam_amd.stereo_slam import StereoSlam
    frames, step, max_depth, voxel, log2 = 6, 8, 6.0, 0.05, 16
    common = ["--synthetic", "tiny", "--frames", str(frames), "--dense-map-voxel", str(voxel), "--dense-map-log2", str(log2), "--cloud-step", str(step),
              "--cloud-max-depth", str(max_depth)]
    first, second = tmp_path / "first.svx", tmp_path / "second.svx"
    replay.main(common + ["--save-dense-map", str(first)])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 0, device="cpu")
    twin = StereoSlam(cfg)
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        if k == 0:
            twin.set_voxel_maps(voxel, log2)
        twin.fuse_new_keyframes(step=step, max_depth=max_depth)
    want = twin.save_voxel_map()
    info = twin.voxel_map_info(0)
    twin.close()
    one = VoxelSaves.frombytes(first.read_bytes())
    assert first.read_bytes() == want.tobytes(0) and len(one.entries(0)) > 100
    assert (int(one.header["n_fused"]), int(one.header["log2_capacity"])) == (info["n_fused"], log2)
    # the same frames into yesterday's map: every key again, every count and sum twice, the stamps as they were
    replay.main(common + ["--load-dense-map", str(first), "--save-dense-map", str(second)])
    two = VoxelSaves.frombytes(second.read_bytes())
    a, b = one.entries(0), two.entries(0)
    assert np.array_equal(a["key"], b["key"]) and np.array_equal(2 * a["acc"][:, :7].astype(np.int64), b["acc"][:, :7]) and np.array_equal(a["acc"][:, 7], b["acc"][:, 7])
    assert int(two.header["n_fused"]) == 2 * int(one.header["n_fused"])
    # another edge is refused
    with pytest.raises(ValueError):
        replay.main(["--synthetic", "tiny", "--frames", "2", "--dense-map-voxel", "0.1", "--load-dense-map", str(first), "--save-dense-map", str(tmp_path / "x.svx")])


@pytest.mark.gpu
def test_a_full_map_grows(tmp_path):
    frames, step, voxel = 2, 8, 0.05
    common = ["--synthetic", "tiny", "--frames", str(frames), "--dense-map-voxel", str(voxel), "--cloud-step", str(step)]
    small, grown, large = tmp_path / "small.svx", tmp_path / "grown.svx", tmp_path / "large.svx"
    replay.main(common + ["--dense-map-log2", "10", "--save-dense-map", str(small)])
    replay.main(common + ["--dense-map-log2", "10", "--dense-map-grow", "16", "--save-dense-map", str(grown)])
    replay.main(common + ["--dense-map-log2", "16", "--save-dense-map", str(large)])
    s, g, l = (VoxelSaves.frombytes(p.read_bytes()) for p in (small, grown, large))
    assert len(s.entries(0)) == 0 and int(s.header["log2_capacity"]) == 10                  # the cloud never fitted: FUSE_FULL every time
    assert len(g.entries(0)) > 768 and g.entries(0).tobytes() == l.entries(0).tobytes()
    assert 10 < int(g.header["log2_capacity"]) <= 16 and int(g.header["n_fused"]) == int(l.header["n_fused"])
    assert len(g.entries(0)) <= hip_lib.voxel_map_bytes(int(g.header["log2_capacity"])) // 40
