"""replay --dump-views: the PPM files of a short synthetic sequence hold the pixels that export_views of a twin run
gives, and the PPM writer is the format's."""
import os

import numpy as np
import pytest

from stereo_svo_slam_amd import replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam


def test_ppm_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    img[0, 0] = (10, 32, 13)                     # bytes that are white space in the header's syntax
    path = tmp_path / "a.ppm"
    replay.write_ppm(path, img)
    raw = path.read_bytes()
    assert raw[:11] == b"P6\n7 5\n255\n" and raw[11:] == img.tobytes()
    assert np.array_equal(replay.read_ppm(path), img)


@pytest.mark.gpu
def test_dump_views_equals_export_views_of_a_twin(tmp_path):
    frames = 6
    out = tmp_path / "views"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--seed", "3", "--dump-views", str(out)])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 3, device="cpu")
    twin = StereoSlam(cfg)
    assert twin.get_image() is None              # nothing before the first frame
    marked = False
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        for what, name in (("last_keyframes", "keyframe"), ("frames", "frame")):
            got = replay.read_ppm(out / f"{k:06d}_{name}.ppm")
            want = twin.export_views(what, pixel="rgb8", markers=True).image(0)
            assert got.shape == (cfg["height"], cfg["width"], 3) and got.tobytes() == want.tobytes(), (k, name)
            gray = twin.get_image(what)
            assert gray.shape == (cfg["height"], cfg["width"])
            marked = marked or got.tobytes() != np.repeat(gray[:, :, None], 3, 2).tobytes()
        assert twin.get_image("frames").tobytes() == L[k].numpy().tobytes()
    assert marked
    assert sorted(os.listdir(out)) == sorted(f"{k:06d}_{n}.ppm" for k in range(frames) for n in ("keyframe", "frame"))
