"""replay --dump-scene: the PPM files of a short synthetic sequence hold the pixels that export_scenes of a twin run
gives, and StereoSlam.get_scene is that picture."""
import os

import pytest

from stereo_svo_slam_amd import replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam


@pytest.mark.gpu
def test_dump_scene_equals_export_scenes_of_a_twin(tmp_path):
    frames = 5
    out = tmp_path / "scene"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--seed", "3", "--dump-scene", str(out)])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 3, device="cpu")
    twin = StereoSlam(cfg)
    assert twin.get_scene() is None              # nothing before the first frame
    pictures = set()
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        got = replay.read_ppm(out / f"{k:06d}_scene.ppm")
        want = twin.export_scenes(camera="front", pixel="rgb8").image(0)
        assert got.shape == (256, 256, 3) and got.tobytes() == want.tobytes(), k
        assert twin.get_scene("front", pixel="rgb8").tobytes() == want.tobytes()
        assert (got == 255).all(axis=2).any() and (got != 255).any()          # background and something on it
        pictures.add(got.tobytes())
    assert len(pictures) > 1                      # the map grows, the pose moves
    assert twin.get_scene("top", cols=64, rows=48, pixel="rgba8").shape == (48, 64, 4)
    assert sorted(os.listdir(out)) == [f"{k:06d}_scene.ppm" for k in range(frames)]
