"""Still-image camera-motion clips (``main.py --dataset sun2both``), the CPU side: the numpy restatement
(``tests/still_image_oracle.py``) against outputs of the reference's own ``ImageDataset.extract_camera_motion``
(``tests/golden/still_image_clips.npz``, written by ``tools/make_still_image_golden.py``) and against PIL, the
trajectory draws, the host-side surface and the C ABI's declarations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import still_image_oracle as oracle
from zeroshotvideoclassification_amd import _lib, preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


golden_cases = oracle.golden_cases


def test_fixture_holds_the_cases_the_tool_writes():
    cases = list(golden_cases())
    assert [(c[1], c[2], c[3]) for c in cases] == [(32, 4, 2)] * 3 + [(112, 2, 1)]
    for img, crop, clip_len, n_clips, _seed, traj, clip in cases:
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and 172 <= min(img.shape[:2]) <= 200
        assert traj.shape == (n_clips * clip_len, 3) and clip.shape == (n_clips, 3, clip_len, crop, crop)
        assert clip.dtype == np.float32
    assert max(int(c[5][:, 2].max()) / c[1] for c in cases) > 5.0           # wide zooms: many taps per axis


def test_restatement_reproduces_the_reference_fixtures():
    """Bit for bit: PIL's two integer passes and three fp32 operations have one right answer."""
    n = 0
    for img, crop, clip_len, n_clips, _seed, traj, clip in golden_cases():
        assert np.array_equal(oracle.camera_motion_clips(img, traj, crop, n_clips, clip_len), clip)
        n += 1
    assert n == 4


def test_trajectory_draws_follow_the_reference_order():
    """Six ``np.random.randint`` draws in the reference's order (auxiliary_stillimages.py:118-122) and its linspace."""
    for img, crop, clip_len, n_clips, seed, traj, _clip in golden_cases():
        np.random.seed(seed)
        got = preprocess.camera_motion_trajectory(img.shape[0], img.shape[1], crop, n_clips * clip_len)
        assert got.shape == traj.shape and got.dtype.kind == "i"
        assert np.array_equal(got, traj)
        top, left, side = got.T
        assert (side >= crop).all() and (top >= 0).all() and (left >= 0).all()
        assert (top + side <= img.shape[0]).all() and (left + side <= img.shape[1]).all()


@pytest.mark.parametrize("crop,sides", [(112, [112, 113, 168, 224, 225, 511, 512]), (16, list(range(16, 74)))])
def test_restatement_equals_pil(crop, sides):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(crop)
    for side in sides:
        window = rng.randint(0, 256, (side, side, 3)).astype(np.uint8)
        if side % 2:                                                         # steep edges reach the clip and the rounding
            window[(np.add.outer(np.arange(side), np.arange(side)) // 3) % 2 == 0] = 255
        want = np.asarray(Image.fromarray(window).resize((crop, crop), Image.BILINEAR))
        assert np.array_equal(oracle.resample_u8(window, crop), want), (crop, side)


def test_restatement_tables_have_the_documented_shape():
    for side, crop, ks in [(16, 16, 3), (17, 16, 5), (32, 16, 5), (33, 16, 7), (128, 16, 17), (512, 112, 11)]:
        coeffs, bounds = oracle.resample_tables(side, crop)
        assert coeffs.shape == (crop, ks) and bounds.shape == (crop, 2) and coeffs.dtype == bounds.dtype == np.int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= side).all() and (bounds[:, 1] <= ks).all()
        assert (np.abs(coeffs.sum(axis=1) - (1 << 22)) <= ks).all()        # each row sums to one, up to its roundings
    coeffs, bounds = oracle.resample_tables(16, 16)
    assert np.array_equal(coeffs[:, 0], np.full(16, 1 << 22)) and not coeffs[:, 1:].any()   # the skipped pass is the identity


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    lib = _lib.load()
    P, i32 = _lib._P, _lib.c_int32
    want = {"zsv_still_image_clips": [P, P, i32, i32, i32, i32, i32, P, P], "zsv_resample_coeffs": [i32, i32, P, P, P]}
    for name, argtypes in want.items():
        assert re.search(r"\bint " + name + r"\(", header), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes)
        assert getattr(lib, name).argtypes == argtypes
    assert "auxiliary_stillimages.py" in header
    # argument checks run before anything touches a device
    assert lib.zsv_resample_coeffs(15, 16, None, None, None) == 1            # side < crop: ZSV_E_BAD_SHAPE
    assert lib.zsv_resample_coeffs(129, 16, None, None, None) == 1           # side > 8 * crop
    assert lib.zsv_resample_coeffs(128, 16, None, None, None) == 2           # ZSV_E_NULL
    assert lib.zsv_still_image_clips(None, None, 1, 1, 8, 112, 111, None, None) == 1
    assert lib.zsv_still_image_clips(None, None, 1, 1, 8, 112, 897, None, None) == 1
    assert lib.zsv_still_image_clips(None, None, 0, 1, 8, 112, 112, None, None) == 1
    assert lib.zsv_still_image_clips(None, None, 1, 1, 8, 112, 896, None, None) == 2


def test_prepare_still_image_channel_handling():
    rng = np.random.RandomState(0)
    grey = rng.randint(0, 256, (5, 7)).astype(np.uint8)
    out = preprocess.prepare_still_image(grey)
    assert out.shape == (5, 7, 3) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(out[:, :, c], grey) for c in range(3))
    assert np.array_equal(preprocess.prepare_still_image(grey[:, :, None]), out)
    rgba = rng.randint(0, 256, (5, 7, 4)).astype(np.uint8)
    out = preprocess.prepare_still_image(rgba)
    assert out.shape == (5, 7, 3) and out.flags["C_CONTIGUOUS"] and np.array_equal(out, rgba[:, :, :3])
    rgb = rgba[:, :, :3]
    assert np.array_equal(preprocess.prepare_still_image(rgb), rgb)
    with pytest.raises(ValueError, match="image"):
        preprocess.prepare_still_image(rng.randint(0, 256, (5, 7, 5)).astype(np.uint8))
    with pytest.raises(ValueError, match="image"):
        preprocess.prepare_still_image(rng.randint(0, 256, (5, 7, 2)).astype(np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        preprocess.prepare_still_image(rgb.astype(np.float32))


def test_cpu_tensors_are_refused():
    clips = preprocess.StillImageClips(clip_len=2, n_clips=1, crop_size=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clips([torch.zeros(40, 50, 3, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clips([torch.zeros(40, 50, 3, dtype=torch.uint8)], trajectories=[np.array([[0, 0, 16], [1, 1, 20]])])
    with pytest.raises(RuntimeError, match="uint8 images"):
        clips([torch.zeros(40, 50, 3)])
    with pytest.raises(RuntimeError, match="uint8 images"):
        clips([torch.zeros(2, 40, 50, 3, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess.resample_coeffs(32, 16, device="cpu")
