"""sia_prep_kernel (a wave per 16 keypoints, a lane per patch row, the taps from five 8-byte block rows) against the
kernel it replaced (a lane per patch pixel, every tap a byte load), through svo_sia_records_check: both run on the
same batch and every 32-bit word of both workspaces is compared, so values, NaN payloads and which words are written
at all must agree. Random-byte level images of the tiny preset (160x120 .. 40x30) and of the euroc preset
(188x120 .. 23x15); every comparison is exact."""
import numpy as np
import pytest
import torch

from stereo_svo_slam_amd import hip_lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
IGNORE_TEMPORARY = 4
COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65)
FILLS = (0x7FC00000, 0x42C80000)            # workspace patterns: NaN and 100.0


@pytest.fixture(scope="module")
def H():
    h = hip_lib.Handle(0, max_keypoints=1024)
    yield h
    h.close()


def cam_of(config):
    return hip_lib.CameraSettings.from_dict(synth.CONFIGS[config])


def used_levels(cfg):
    return range(cfg["min_pyramid_level_pose_estimation"], cfg["max_pyramid_levels"])


def level_images(config, seed, pitch_extra=0, offset=0, fill=0xCD):
    """random-byte images of every level of a preset, each a view of w columns at byte `offset` of a buffer of its
    own with rows of w + pitch_extra bytes, the bytes around the image set to `fill`"""
    cfg = synth.CONFIGS[config]
    rng = np.random.RandomState(seed)
    out = []
    for l in range(cfg["max_pyramid_levels"]):
        w, h = cfg["width"] >> l, cfg["height"] >> l
        pitch = w + pitch_extra
        buf = torch.full((offset + h * pitch + 16,), fill, dtype=torch.uint8, device="cuda")
        v = buf[offset:offset + h * pitch].view(h, pitch)[:, :w]
        v.copy_(torch.from_numpy(rng.randint(0, 256, (h, w)).astype(np.uint8)).cuda())
        assert v.data_ptr() % 4 == offset % 4 and v.stride(0) == pitch
        out.append(v)
    return out


def around(v):
    """v and the floats next to it"""
    v = F(v)
    return [v, np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))]


def crafted_keypoints(config):
    """full-resolution positions that are, at every level the alignment uses: 0 to 4 px from every border and corner
    (so each of the three bounds tests flips), at fractions 0 and 0.5 and the floats next to them, and in between;
    then negative, far outside and infinite ones (NaN: nan_keypoints)"""
    cfg = synth.CONFIGS[config]
    pts = []
    for l in used_levels(cfg):
        s, w, h = 1 << l, cfg["width"] >> l, cfg["height"] >> l
        xs = [k for k in range(5)] + [w - k for k in range(5)] + [2.5, w - 2.5]
        ys = [k for k in range(5)] + [h - k for k in range(5)] + [1.5, h - 3.5]
        for x in xs:
            for y in ys:
                pts.append((x * s, y * s))
        # the floor boundaries and the rounding case of the walk, inside the image and next to the borders
        for base in (7.0, 7.5, 3.0, 2.5, w - 4.0, w - 3.5):
            for x in around(base * s):
                for y in around(min(base, h - 4.0) * s) + [F(h / 2 * s + 0.3)]:
                    pts.append((x, y))
    bad = [-1.0, -7.5, -1e6, 1e6, 1e30, -1e30, 70000.0, np.inf, -np.inf]
    for b in bad:
        pts += [(b, 60.0), (60.0, b), (b, b)]
    pts += [(-np.inf, np.inf)]
    return np.array(pts, F)


def nan_keypoints():
    """NaN in one coordinate or in both, beside coordinates inside every level, infinite and far ones"""
    return np.array([(np.nan, 60.0), (60.0, np.nan), (np.nan, np.nan), (np.nan, np.inf), (np.inf, np.nan), (np.nan, -1e30),
                     (-5.0, np.nan)], F)


def random_keypoints(config, n, seed):
    """positions all over the image and a little outside, a third of them on quarter pixels"""
    cfg = synth.CONFIGS[config]
    rng = np.random.RandomState(seed)
    k = rng.uniform(-6, 1, (n, 2)) + rng.uniform(0, 1, (n, 2)) * (cfg["width"] + 10, cfg["height"] + 10)
    k[::3] = np.round(k[::3] * 4) / 4
    return k.astype(F)


def at_the_end(a):
    """a on the device as the last bytes of a larger allocation: what lies behind it is not the test's"""
    flat = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.zeros(4096 + flat.numel(), dtype=flat.dtype, device="cuda")
    buf[4096:] = flat.cuda()
    return buf[4096:].view(a.shape)


def run(H, config, seqs, images, rec_cap=None, fill=FILLS[0], stride=None, want_records=False, no_flags=False, tail=False):
    """seqs: per sequence (kps2d [n, 2], flags [n] or None). Slots past a sequence's n hold poison. no_flags: the
    launch gets no flags array at all; tail: the keypoint arrays end where their allocations end."""
    cam = cam_of(config)
    n = [len(k) for k, _ in seqs]
    n_bound = max(n)
    stride = stride or n_bound + 7
    k2 = np.full((len(seqs), max(stride, 1), 2), 1e30, F)
    fl = np.full((len(seqs), max(stride, 1)), 0xFFFFFFFB, np.uint32)           # (every bit but IGNORE_TEMPORARY)
    fl[:, 1::2] = 0xFFFFFFFF
    for b, (k, f) in enumerate(seqs):
        k2[b, :len(k)] = k
        fl[b, :len(k)] = 0 if f is None else f
    imgs = images if isinstance(images[0], list) else [images] * len(seqs)
    put = at_the_end if tail else (lambda a: torch.from_numpy(a).cuda())
    n_diff, first, rec = H.sia_records_check(
        torch.tensor(n, dtype=torch.int32, device="cuda"), n_bound, put(k2),
        None if no_flags else put(fl.view(np.int32)), imgs, cam, rec_cap=rec_cap, ws_fill=fill, want_records=want_records)
    assert (n_diff, first) == (0, -1), (config, n, n_diff, first)
    return rec


def some_flags(n, seed):
    """IGNORE_TEMPORARY on every third keypoint or so, between active ones; other bits at random"""
    rng = np.random.RandomState(seed)
    f = rng.randint(0, 256, n).astype(np.uint32) & ~np.uint32(IGNORE_TEMPORARY)
    f[rng.rand(n) < 0.3] |= IGNORE_TEMPORARY
    return f


@pytest.mark.parametrize("config", ["tiny", "euroc"])
def test_every_count_in_one_batch(H, config):
    """n = 0 .. 65 around the 4-keypoint span and the 16-keypoint wave, rows of 68 floats (no multiple of 16)"""
    imgs = level_images(config, 1)
    seqs = [(random_keypoints(config, n, 10 + n), some_flags(n, n)) for n in COUNTS]
    for fill in FILLS:
        run(H, config, seqs, imgs, rec_cap=68, fill=fill)
    run(H, config, seqs[:3], imgs, rec_cap=8, stride=5)                  # counts 0, 1, 3 with 5 slots each


@pytest.mark.parametrize("config", ["tiny", "euroc"])
def test_without_a_flags_array(H, config):
    """flags == NULL: every keypoint below n is active; the kernel's second start-up load then repeats the position's
    address and its result is dropped"""
    imgs = level_images(config, 3)
    k = np.concatenate([crafted_keypoints(config)[::5], random_keypoints(config, 37, 4)])
    run(H, config, [(k, None), (k[:21], None), (k[:0], None)], imgs, no_flags=True)


@pytest.mark.parametrize("n", [1, 13, 114])
def test_arrays_that_end_with_the_last_keypoint(H, n):
    """stride == n, no multiple of 16, kps2d and flags the last bytes of their allocations: the last wave's lanes past
    n ask for slot n - 1 (SiaArgs::cap is the readable length), never for one behind the arrays"""
    imgs = level_images("euroc", 6)
    k = random_keypoints("euroc", n, 40 + n)
    run(H, "euroc", [(k, some_flags(n, n))], imgs, stride=n, tail=True)
    run(H, "euroc", [(k, None)], imgs, stride=n, tail=True, no_flags=True)


@pytest.mark.parametrize("config", ["tiny", "euroc"])
def test_borders_fractions_and_bad_coordinates(H, config):
    cfg = synth.CONFIGS[config]
    imgs = level_images(config, 2)
    k = crafted_keypoints(config)
    rec = run(H, config, [(k, None), (k, some_flags(len(k), 3)), (k[::-1].copy(), some_flags(len(k), 4))], imgs,
              want_records=True)
    # the crafted set reaches all three outcomes of every field at every level: this is no comparison of NaN with NaN
    n = len(k)
    rec = rec.cpu().numpy()[0, :, :, :n]
    for slot, _ in enumerate(used_levels(cfg)):
        for field in (0, 1):
            r = rec[slot, field * 16:field * 16 + 16]
            assert np.isnan(r).any() and np.isfinite(r).any(), (slot, field)
        g = rec[slot, 32:64]
        assert (g == 0).any() and (g != 0).any() and np.isfinite(rec[slot, 64:67]).all(), slot


@pytest.mark.parametrize("config", ["tiny", "euroc"])
def test_nan_coordinates(H, config):
    """NaN positions between ordinary ones. A coordinate that is NaN passes the bounds tests (every comparison with it
    is false), so the taps are read at column or row 0 and a NaN goes into the reference patch sums, the gradients and
    sum g g^T of that keypoint. Its bits count too: 1 - x2 negates the NaN's sign, the patch sum then adds NaNs of both
    signs, and an add returns its first operand's. The kernel therefore forms 1 - x2 with the instruction the replaced
    kernel has there and keeps the running sum as the first operand of every add (prep_add in sia.hip): the records
    carry the first term's NaN, 0xFFC00000 for the default NaN, as they always did."""
    k = random_keypoints(config, 24, 12)
    k[2::3][:7] = nan_keypoints()
    rec = run(H, config, [(k, None)], level_images(config, 13), want_records=True)
    bits = rec.cpu().numpy().view(np.uint32)[0, :, 16:67, 2]          # keypoint 2 = (NaN, 60): patch sums, gradients, sums
    assert (bits == 0xFFC00000).any() and not (bits == 0x7FC00000)[:, 16:].any()


@pytest.mark.parametrize("config", ["tiny", "euroc"])
@pytest.mark.parametrize("pitch_extra,offset", [(5, 0), (3, 1), (8, 2), (1, 3)])
def test_image_layouts(H, config, pitch_extra, offset):
    """stride != width, euroc widths 47 and 23 that are no multiple of 4, base pointers 1, 2 and 3 bytes off a dword"""
    imgs = level_images(config, 5, pitch_extra, offset)
    k = np.concatenate([crafted_keypoints(config)[::3], random_keypoints(config, 40, 6)])
    run(H, config, [(k, some_flags(len(k), 7))], imgs)


@pytest.mark.parametrize("batch", [1, 5, 33])
def test_batches_of_unequal_counts(H, batch):
    rng = np.random.RandomState(batch)
    imgs = [level_images("euroc", 20 + b % 3, pitch_extra=b % 3) for b in range(min(batch, 3))]
    seqs = [(random_keypoints("euroc", int(n), 30 + b), some_flags(int(n), b))
            for b, n in enumerate(rng.randint(0, 130, batch))]
    run(H, "euroc", seqs, [imgs[b % len(imgs)] for b in range(batch)], fill=FILLS[1])


@pytest.mark.parametrize("config", ["tiny", "euroc"])
def test_bytes_around_the_image_do_not_matter(H, config):
    """the same images inside larger buffers whose surrounding bytes differ: the same records, word for word"""
    k = np.concatenate([crafted_keypoints(config), random_keypoints(config, 50, 8)])
    fl = some_flags(len(k), 9)
    recs = [run(H, config, [(k, fl)], level_images(config, 11, pitch_extra=9, offset=3, fill=fill), want_records=True)
            for fill in (0x00, 0xFF)]
    assert torch.equal(recs[0].view(torch.int32), recs[1].view(torch.int32))
