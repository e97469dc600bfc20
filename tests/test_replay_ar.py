"""replay --dump-ar: the PPM files of a short synthetic sequence hold the pixels that export_ar of a twin run gives,
and StereoSlam.get_ar is that picture."""
import os

import numpy as np
import pytest

from stereo_svo_slam_amd import hip_lib, replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam


@pytest.mark.gpu
def test_dump_ar_equals_export_ar_of_a_twin(tmp_path):
    frames = 5
    out = tmp_path / "ar"
    replay.main(["--synthetic", "tiny", "--frames", str(frames), "--seed", "3", "--dump-ar", str(out), "--ar-box", "0.15",
                 "--ar-at", "0.05,-0.02,0.6"])
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 3, device="cpu")
    objects = replay.ar_objects(0.15, (0.05, -0.02, 0.6))
    twin = StereoSlam(cfg)
    assert twin.get_ar(objects) is None                       # nothing before the first frame
    pictures = set()
    for k in range(frames):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        got = replay.read_ppm(out / f"{k:06d}_ar.ppm")
        want = twin.export_ar([objects[0][:2]], [(objects[0][2], 0, objects[0][3])], pixel="rgb8").image(0)
        assert got.shape == (cfg["height"], cfg["width"], 3) and got.tobytes() == want.tobytes(), k
        assert twin.get_ar(objects, pixel="rgb8").tobytes() == want.tobytes()
        gray = twin.get_image("frames", pixel="gray8")
        box = (got != gray[:, :, None]).any(axis=2)
        assert 500 < box.sum() < got.shape[0] * got.shape[1] // 2      # some pixels show the box and most the image
        assert (np.diff(got[box].astype(int), axis=1) != 0).any()      # ... in the box's colour, not a gray
        pictures.add(got.tobytes())
    assert len(pictures) == frames                             # the image moves under the box
    assert twin.get_ar(objects, pixel="rgba8", ambient=1.0).shape == (cfg["height"], cfg["width"], 4)
    assert sorted(os.listdir(out)) == [f"{k:06d}_ar.ppm" for k in range(frames)]
    assert replay.ar_objects()[0][2][[3, 7, 11]].tolist() == list(hip_lib.AR_AT)      # the demo's placement by default
