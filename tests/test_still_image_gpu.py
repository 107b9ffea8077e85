"""Still-image camera-motion clips on the GPU (``preprocess.StillImageClips`` / ``zsv_still_image_clips``) against
outputs of the reference's own ``ImageDataset.extract_camera_motion`` (``tests/golden/still_image_clips.npz``) and
against the numpy restatement pinned to them (``tests/still_image_oracle.py``).  PIL's uint8 resample is integer
arithmetic and the normalisation is three correctly rounded fp32 operations: every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import still_image_oracle as oracle
from helpers import make_opt
from zeroshotvideoclassification_amd import _lib, network, preprocess, synthetic

pytestmark = pytest.mark.gpu
golden_cases = oracle.golden_cases


def _image(h, w, seed):
    """Noise with hard 0 / 255 stripes: the clip and the rounding are reached, not only mid-greys."""
    img = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[:, (np.arange(w) // 5) % 4 == 0] = 255
    img[(np.arange(h) // 3) % 5 == 0] = 0
    return img


def _check(images, trajectories, clip_len, n_clips, crop=16):
    """Run the batch on the device and compare every image's clips with the restatement, bit for bit."""
    clips = preprocess.StillImageClips(clip_len=clip_len, n_clips=n_clips, crop_size=crop)
    out = clips([torch.from_numpy(im).cuda() for im in images], trajectories=trajectories)
    assert out.shape == (len(images), n_clips, 3, clip_len, crop, crop) and out.dtype == torch.float32 and out.is_contiguous()
    out = out.cpu().numpy()
    for b, (im, traj) in enumerate(zip(images, trajectories)):
        want = oracle.camera_motion_clips(im, np.asarray(traj), crop, n_clips, clip_len)
        assert np.array_equal(out[b], want), (b, float(np.abs(out[b] - want).max()))
    return out


def test_fixture_cases_match_the_reference_bit_for_bit():
    cases = list(golden_cases())
    for img, crop, clip_len, n_clips, _seed, traj, clip in cases:
        out = preprocess.StillImageClips(clip_len, n_clips, crop)([torch.from_numpy(img).cuda()], trajectories=[traj])
        assert torch.equal(out.cpu(), torch.from_numpy(clip)[None])
    small = [c for c in cases if c[1] == 32]                                # the three crop-32 images as one batch
    out = preprocess.StillImageClips(4, 2, 32)([torch.from_numpy(c[0]).cuda() for c in small], trajectories=[c[5] for c in small])
    assert torch.equal(out.cpu(), torch.from_numpy(np.stack([c[6] for c in small])))


def test_fixture_cases_with_drawn_trajectories():
    """Under the fixture's seed the transform draws the reference's trajectory itself."""
    for img, crop, clip_len, n_clips, seed, _traj, clip in golden_cases():
        np.random.seed(seed)
        out = preprocess.StillImageClips(clip_len, n_clips, crop)([torch.from_numpy(img).cuda()])
        assert torch.equal(out.cpu(), torch.from_numpy(clip)[None])


@pytest.mark.parametrize("crop,sides", [(16, range(16, 129)), (112, range(112, 513))])
def test_coefficient_tables_match_the_restatement(crop, sides):
    """``zsv_resample_coeffs`` is the device code the kernel uses: a divergence of its fp64 arithmetic shows here."""
    got = [preprocess.resample_coeffs(side, crop) for side in sides]        # enqueue everything, then read back
    for side, (coeffs, bounds) in zip(sides, got):
        want_coeffs, want_bounds = oracle.resample_tables(side, crop)
        assert coeffs.shape == want_coeffs.shape and coeffs.dtype == torch.int32, side
        assert np.array_equal(bounds.cpu().numpy(), want_bounds), side
        assert np.array_equal(coeffs.cpu().numpy(), want_coeffs), side


def _windows(h, w, sides, seed):
    """One window per side, placed inside an (h, w) image by a seeded draw."""
    rng = np.random.RandomState(seed)
    return np.array([[rng.randint(0, h - s + 1), rng.randint(0, w - s + 1), s] for s in sides])


GENERATED = {
    # name: (image sizes, sides of the frames of each image, clip_len, n_clips)
    "side_equals_crop": ([(40, 50)], [[16, 16]], 2, 1),
    "side_crop_plus_one": ([(40, 50)], [[17, 17]], 2, 1),
    "side_2x_and_8x": ([(130, 141)], [[32, 128]], 2, 1),
    "non_integer_ratios": ([(120, 131)], [[23, 37, 50, 77, 101, 119]], 6, 1),
    "odd_image_41x53": ([(41, 53)], [[16, 19, 33, 41]], 4, 1),
    "three_sizes_one_batch": ([(41, 53), (90, 64), (130, 129)], [[20, 41], [64, 17], [128, 100]], 2, 1),
    "two_clips_three_frames": ([(100, 111)], [[16, 29, 42, 55, 68, 81]], 3, 2),
}


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_cases_match_the_restatement(name):
    sizes, sides, clip_len, n_clips = GENERATED[name]
    images = [_image(h, w, seed=h * 1000 + w) for h, w in sizes]
    trajectories = [_windows(h, w, s, seed=h + w) for (h, w), s in zip(sizes, sides)]
    out = _check(images, trajectories, clip_len, n_clips)
    if name == "two_clips_three_frames":                                     # frame f lands at clip f // T, time f % T
        t, l, s = trajectories[0][4]
        want = oracle.normalise(oracle.resample_u8(images[0][t:t + s, l:l + s], 16))
        assert np.array_equal(out[0, 1, :, 1], want)


def test_windows_flush_with_the_corners():
    h, w = 41, 53
    img = _image(h, w, seed=7)
    traj = np.array([[0, 0, 16], [0, 0, 41], [h - 16, w - 16, 16], [h - 41, w - 41, 41], [0, w - 30, 30], [h - 30, 0, 30]])
    _check([img], [traj], clip_len=6, n_clips=1)


@pytest.mark.parametrize("kind", ["zeros", "full", "checkerboard"])
def test_constant_and_checkerboard_images(kind):
    h, w = 70, 75
    img = {"zeros": np.zeros((h, w, 3), np.uint8), "full": np.full((h, w, 3), 255, np.uint8),
           "checkerboard": (np.indices((h, w)).sum(0) % 2 * 255).astype(np.uint8)[:, :, None].repeat(3, 2)}[kind]
    out = _check([img], [_windows(h, w, [16, 17, 31, 32, 47, 70], seed=3)], clip_len=6, n_clips=1)
    if kind != "checkerboard":                                              # a constant image stays constant per channel
        u8 = 0 if kind == "zeros" else 255
        want = (np.float32(u8) / np.float32(255) - oracle.MEAN) / oracle.STD
        assert all((out[0, 0, c] == want[c]).all() for c in range(3))


def test_crop_112_side_512():
    img = _image(512, 520, seed=11)
    _check([img], [np.array([[0, 8, 512], [3, 0, 509]])], clip_len=2, n_clips=1, crop=112)


def test_two_calls_return_equal_tensors():
    imgs = [torch.from_numpy(_image(90, 101, seed=5)).cuda(), torch.from_numpy(_image(64, 70, seed=6)).cuda()]
    traj = [_windows(90, 101, [16, 40, 77, 90], seed=1), _windows(64, 70, [64, 33, 20, 16], seed=2)]
    clips = preprocess.StillImageClips(clip_len=2, n_clips=2, crop_size=16)
    a, b = clips(imgs, trajectories=traj), clips(imgs, trajectories=traj)
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_drawn_trajectories_equal_explicit_ones():
    sizes = [(100, 128), (90, 121)]
    imgs = [torch.from_numpy(_image(h, w, seed=h)).cuda() for h, w in sizes]
    clips = preprocess.StillImageClips(clip_len=3, n_clips=2, crop_size=16)
    np.random.seed(123)
    drawn = clips(imgs)
    np.random.seed(123)
    traj = [preprocess.camera_motion_trajectory(h, w, 16, 6) for h, w in sizes]     # image order, six draws each
    assert torch.equal(drawn, clips(imgs, trajectories=traj))


def test_refusals_happen_before_any_launch(monkeypatch):
    img = torch.zeros(60, 200, 3, dtype=torch.uint8, device="cuda")
    clips = preprocess.StillImageClips(clip_len=2, n_clips=1, crop_size=16)

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    for traj, message in [([[0, 0, 16], [45, 0, 16]], "outside the image"),            # bottom edge
                          ([[0, 0, 16], [0, 185, 16]], "outside the image"),           # right edge
                          ([[-1, 0, 16], [0, 0, 16]], "outside the image"),
                          ([[0, 0, 15], [0, 0, 16]], "smaller than the crop"),
                          ([[0, 0, 16], [0, 0, 129]], "larger than 8 x the crop"),
                          ([[0, 0, 16]], "trajectory")]:
        with pytest.raises(RuntimeError, match=message):
            clips([img], trajectories=[np.array(traj)])
    with pytest.raises(RuntimeError, match="trajectory"):
        clips([img], trajectories=[np.array([[0.0, 0.0, 16.0], [0.0, 0.0, 16.0]])])
    with pytest.raises(RuntimeError, match="one trajectory per image"):
        clips([img, img], trajectories=[np.array([[0, 0, 16], [0, 0, 16]])])
    with pytest.raises(RuntimeError, match="uint8 images"):
        clips([img.float()])
    with pytest.raises(RuntimeError, match="crop <= side"):
        preprocess.resample_coeffs(129, 16)


def test_output_feeds_the_model():
    img = torch.from_numpy(_image(180, 200, seed=9)).cuda()
    np.random.seed(0)
    x = preprocess.StillImageClips(clip_len=8, n_clips=1, crop_size=112)([img])
    assert x.shape == (1, 1, 3, 8, 112, 112)
    model = network.get_network(make_opt("r2plus1d_18"))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
    model.cuda().eval()
    with torch.no_grad():
        emb, _ = model(x)
    assert emb.shape == (1, 300) and torch.isfinite(emb).all()
    assert abs(emb.norm(dim=1).item() - 1.0) < 1e-5


def test_a_frame_that_breaks_the_contract_becomes_nan_and_is_never_read():
    """Straight through the C entry (``StillImageClips`` refuses such tables): windows outside the image, ``side < crop``
    and ``side > max_side`` give NaN frames; the valid frames of the same launch are untouched."""
    from ctypes import c_void_p
    h, w, crop = 40, 50, 16
    img_np = _image(h, w, seed=13)
    img = torch.from_numpy(img_np).cuda()
    table = np.array([[0, 0, 16], [30, 0, 16], [0, 40, 16], [-1, 0, 16], [0, 0, 15], [0, 0, 33], [5, 7, 32], [0, -2, 20]], dtype=np.int32)
    bad = [1, 2, 3, 4, 5, 7]                                                 # bottom, right, negative top, small, > max_side, negative left
    itab = torch.tensor([[img.data_ptr(), h, w]], dtype=torch.int64).cuda()
    ftab = torch.from_numpy(table).cuda()
    out = torch.zeros((1, 2, 3, 4, crop, crop), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().zsv_still_image_clips(itab.data_ptr(), ftab.data_ptr(), 1, 2, 4, crop, 32, out.data_ptr(),
                                                 c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_still_image_clips")
    out = out.cpu().numpy()
    for f, (t, l, s) in enumerate(table.tolist()):
        got = out[0, f // 4, :, f % 4]
        if f in bad:
            assert np.isnan(got).all(), f
        else:
            assert np.array_equal(got, oracle.normalise(oracle.resample_u8(img_np[t:t + s, l:l + s], crop))), f
