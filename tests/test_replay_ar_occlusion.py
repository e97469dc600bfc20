"""replay --dump-ar --ar-occlude: the PPM files of a short synthetic sequence differ from the unoccluded ones only at
pixels that the run's log counts as hidden, and there they show the camera image."""
import re

import pytest

from stereo_svo_slam_amd import replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam


@pytest.mark.gpu
def test_dump_ar_occluded_differs_only_at_hidden_pixels(tmp_path, capsys):
    frames = 4
    # a box that stands half in the floor of the synthetic room (y = 1.6, y is down), four metres ahead
    box = ["--ar-box", "0.8", "--ar-at", "0,1.6,4"]
    common = ["--synthetic", "tiny", "--frames", str(frames), "--seed", "3"]
    replay.main(common + ["--dump-ar", str(tmp_path / "plain")] + box)
    capsys.readouterr()
    replay.main(common + ["--dump-ar", str(tmp_path / "occluded"), "--ar-occlude", "4", "--ar-margin", "0.05", "--ar-lr", "1.5"] + box)
    log = capsys.readouterr().out
    lines = re.findall(r"^ar (\d{6}) covered (\d+) hidden (\d+) occluder_points (\d+)$", log, re.M)
    assert [int(l[0]) for l in lines] == list(range(frames))
    cfg, L, R, _, ts = synth.make_sequence("tiny", frames, 3, device="cpu")
    twin = StereoSlam(cfg)
    some_hidden = 0
    for k, (_, covered, hidden, points) in enumerate(lines):
        covered, hidden, points = int(covered), int(hidden), int(points)
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        gray = twin.get_image("frames", pixel="gray8")
        plain = replay.read_ppm(tmp_path / "plain" / f"{k:06d}_ar.ppm")
        got = replay.read_ppm(tmp_path / "occluded" / f"{k:06d}_ar.ppm")
        differs = (plain != got).any(axis=2)
        box_pixels = (plain != gray[:, :, None]).any(axis=2)
        assert 0 < points <= (cfg["width"] // 4) * (cfg["height"] // 4)
        assert box_pixels.sum() <= covered and 0 <= hidden <= covered, k
        # a hidden pixel shows the image (it differs unless the box has the image's gray there): no more pixels differ
        # than the log counts as hidden, all of them lie on the box, and they show the gray plane
        assert differs.sum() <= hidden and not (differs & ~box_pixels).any(), (k, int(differs.sum()), hidden)
        assert (got[differs] == gray[differs][:, None]).all(), k
        assert differs.sum() >= hidden - (covered - box_pixels.sum()), k
        some_hidden += hidden
    assert some_hidden > 0
    with pytest.raises(SystemExit):
        replay.main(common + ["--ar-occlude", "4"])                    # needs --dump-ar
    with pytest.raises(SystemExit):
        replay.main(common + ["--dump-ar", str(tmp_path / "bad"), "--ar-occlude", "17"])
