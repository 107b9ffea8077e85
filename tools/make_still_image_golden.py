#!/usr/bin/env python3
"""Write ``tests/golden/still_image_clips.npz`` from the reference's own ``ImageDataset.extract_camera_motion``.

BUILD MACHINE ONLY: it needs the reference checkout (``oracle.reference_import.REFERENCE_ROOT``) and PIL.  The
reference's ``auxiliary/auxiliary_stillimages.py`` is imported as it is; the modules it names that are absent offline
are replaced by the stand-ins below.  ``cv2`` and ``skimage`` are empty: they are only reached for images whose short
side is outside 172 ... 512, and every fixture image is inside.  ``torchvision.transforms`` is a handful of classes
that each state in a line or two, on PIL and torch, what torchvision does for a PIL image.  The trajectory draws, the
slicing and the frame order are therefore the reference's.

Each case ``i`` holds ``image_i``, ``meta_i`` = (crop, clip_len, n_clips, seed), ``trajectory_i`` (recovered by
re-seeding ``preprocess.camera_motion_trajectory``) and ``clip_i``, the reference's output.  The tool refuses to write
a fixture that the numpy restatement (``tests/still_image_oracle.py``) does not reproduce bit for bit.  Run it twice:
the file is byte-identical.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
sys.dont_write_bytecode = True

# (height, width, crop, clip_len, n_clips, seed)
# (the seeds were picked for wide zooms: the sides run from the crop itself up to 5.5 x the crop)
CASES = [(172, 231, 32, 4, 2, 474), (200, 183, 32, 4, 2, 3618), (189, 190, 32, 4, 2, 1638), (180, 243, 112, 2, 1, 40)]


def synthetic_image(h, w, seed):
    """Blocks with hard 0 / 255 edges under mild noise: the resample meets its clip, its rounding and steep gradients."""
    rng = np.random.RandomState(seed)
    blocks = np.kron(rng.randint(0, 256, (-(-h // 8), -(-w // 8), 3)), np.ones((8, 8, 1), dtype=np.int64))[:h, :w]
    blocks[h // 3:h // 3 + 24, : w // 2] = 255
    blocks[: h // 2, w // 3:w // 3 + 24] = 0
    return np.clip(blocks + rng.randint(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def _absent(name):
    def fail(*_a, **_k):
        raise RuntimeError(f"{name} is absent offline and must not be reached (image short side outside 172 ... 512?)")
    return fail


def install_stand_ins():
    from PIL import Image

    class Compose:                                    # apply in order
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x

    class ToPILImage:                                 # (H, W, 3) uint8 ndarray -> PIL RGB image
        def __call__(self, arr):
            return Image.fromarray(arr)

    class Resize:                                     # size is (h, w); PIL takes (w, h); bilinear, antialiased as PIL always is
        def __init__(self, size):
            self.size = tuple(size)

        def __call__(self, img):
            return img.resize(self.size[::-1], Image.BILINEAR)

    class ToTensor:                                   # HWC uint8 -> CHW float32 / 255
        def __call__(self, img):
            return torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Normalize:                                  # (x - mean) / std per channel, in float32
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, x):
            mean = torch.as_tensor(self.mean, dtype=x.dtype)[:, None, None]
            std = torch.as_tensor(self.std, dtype=x.dtype)[:, None, None]
            return x.clone().sub_(mean).div_(std)

    class Unused:                                     # RandomResizedCrop / RandomHorizontalFlip: built by __init__, used by extract_video only
        def __init__(self, *_a, **_k):
            pass

        def __call__(self, _x):
            raise RuntimeError("extract_video is not part of the fixture")

    def module(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    module("cv2")
    skimage = module("skimage")
    skimage.__path__ = []
    skimage.io = module("skimage.io", imread=_absent("skimage.io.imread"))
    skimage.transform = module("skimage.transform", resize=_absent("skimage.transform.resize"))
    tv = module("torchvision")
    tv.__path__ = []
    tv.transforms = module("torchvision.transforms", Compose=Compose, ToPILImage=ToPILImage, Resize=Resize, ToTensor=ToTensor,
                           Normalize=Normalize, RandomResizedCrop=Unused, RandomHorizontalFlip=Unused)


def write_npz(path, arrays):
    """``np.savez_compressed`` with a fixed timestamp on every member, so that a rerun gives the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, value in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fid:
                np.lib.format.write_array(fid, np.asanyarray(value), allow_pickle=False)


def main():
    from oracle import reference_import
    import still_image_oracle as oracle
    from zeroshotvideoclassification_amd import preprocess

    if not reference_import.reference_available():
        raise SystemExit(f"the reference is not at {reference_import.REFERENCE_ROOT}: this tool runs on the build machine only")
    install_stand_ins()
    if reference_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, reference_import.REFERENCE_ROOT)
    ref = importlib.import_module("auxiliary.auxiliary_stillimages")

    out = {"n_cases": np.int64(len(CASES))}
    for i, (h, w, crop, clip_len, n_clips, seed) in enumerate(CASES):
        img = synthetic_image(h, w, seed)
        ds = ref.ImageDataset(["x"], ["x"], None, ["x"], "sun", clip_len=clip_len, n_clips=n_clips, crop_size=crop)
        np.random.seed(seed)
        clip = ds.extract_camera_motion(img).contiguous().numpy()
        np.random.seed(seed)
        trajectory = preprocess.camera_motion_trajectory(h, w, crop, n_clips * clip_len)
        assert clip.shape == (n_clips, 3, clip_len, crop, crop) and clip.dtype == np.float32
        assert np.array_equal(oracle.camera_motion_clips(img, trajectory, crop, n_clips, clip_len), clip), \
            f"case {i}: the restatement (or the trajectory draw order) differs from the reference"
        print(f"case {i}: image {h}x{w}, crop {crop}, sides {trajectory[:, 2].min()} ... {trajectory[:, 2].max()} "
              f"({trajectory[:, 2].max() / crop:.2f} x crop)")
        out[f"image_{i}"] = img
        out[f"meta_{i}"] = np.array([crop, clip_len, n_clips, seed], dtype=np.int64)
        out[f"trajectory_{i}"] = trajectory.astype(np.int64)
        out[f"clip_{i}"] = clip
    path = os.path.join(ROOT, "tests", "golden", "still_image_clips.npz")
    write_npz(path, out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
