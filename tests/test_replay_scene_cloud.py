"""replay --dump-scene with --scene-dense and --scene-accumulate: the PPM files of a short synthetic sequence show the
frame's dense cloud (they differ from the plain ones and equal get_scene(dense=...) of a twin run), and with the
accumulated extra span the cloud-coloured pixels do not get fewer when a keyframe is added."""
import pytest

from stereo_svo_slam_amd import replay, synth
from stereo_svo_slam_amd.stereo_slam import StereoSlam

FRAMES, SEED = 6, 3


def _gray_pixels(img):
    """pixels that show a cloud point: the records carry the left image's gray in all three channels; the lines and
    the background have pure colours (a keypoint may be gray too; it is there in every picture alike)"""
    gray = (img[:, :, 0] == img[:, :, 1]) & (img[:, :, 1] == img[:, :, 2])
    return int((gray & ~(img == 255).all(axis=2)).sum())


@pytest.mark.gpu
def test_scene_dense_and_accumulate(tmp_path):
    plain, dense = tmp_path / "plain", tmp_path / "dense"
    common = ["--synthetic", "tiny", "--frames", str(FRAMES), "--seed", str(SEED)]
    replay.main(common + ["--dump-scene", str(plain)])
    replay.main(common + ["--dump-scene", str(dense), "--scene-dense", "8", "--scene-dense-lr", "1.0", "--scene-dense-max-depth", "50"])
    cfg, L, R, _, ts = synth.make_sequence("tiny", FRAMES, SEED, device="cpu")
    twin = StereoSlam(cfg)
    for k in range(FRAMES):
        twin.new_image(L[k].numpy(), R[k].numpy(), float(ts[k]))
        name = f"{k:06d}_scene.ppm"
        a, b = (replay.read_ppm(d / name) for d in (plain, dense))
        assert a.shape == b.shape == (256, 256, 3)
        assert a.tobytes() != b.tobytes(), k                                     # the dense layer shows
        want = twin.get_scene("front", pixel="rgb8", dense=dict(what="frames", step=8, max_depth=50.0, lr_check=1.0))
        assert b.tobytes() == want.tobytes(), k
        assert _gray_pixels(b) > _gray_pixels(a), k
    assert replay.build_parser().parse_args(common + ["--dump-scene", "d", "--scene-accumulate", "7"]).scene_accumulate == 7


@pytest.mark.gpu
def test_scene_accumulate_grows_with_the_keyframes(tmp_path):
    """fast motion (the recipe of test_scene_gpu.py), so that the 16 frames add keyframes: what replay.main runs per
    frame, on those frames"""
    frames = 16
    cfg, L, R, _, ts = synth.make_sequence_gpu("tiny", frames, 1, motion_scale=4.0)
    L, R = L.cpu().numpy(), R.cpu().numpy()
    grown, few = tmp_path / "grown", tmp_path / "few"
    rp = replay.Replay(cfg, dump_scene=str(grown), scene_accumulate=100000)
    capped = replay.Replay(cfg, dump_scene=str(few), scene_accumulate=500, scene_dense=8)
    counts, keyframes = [], []
    for k in range(frames):
        rp.feed(L[k], R[k], float(ts[k]))
        capped.feed(L[k], R[k], float(ts[k]))
        counts.append(_gray_pixels(replay.read_ppm(grown / f"{k:06d}_scene.ppm")))
        keyframes.append(rp.slam.num_keyframes())
        assert capped._scene_map.shape == (min(500, capped._scene_map.shape[0]), 16) and capped._scene_map.shape[0] <= 500
    print("cloud-coloured pixels per frame:", counts, "keyframes:", keyframes)
    assert keyframes[-1] > keyframes[0], "the sequence adds keyframes"
    assert rp._scene_map.shape[0] > 4000 and capped._scene_map.shape[0] == 500
    for k in range(1, frames):                                       # the camera is fixed (front) and records are only added
        if keyframes[k] > keyframes[k - 1]:
            assert counts[k] >= counts[k - 1], (k, counts)
    assert counts[-1] > counts[0]
