"""Integer restatement of the still-image chain (TEST INFRASTRUCTURE; never imported by the package).

``auxiliary/auxiliary_stillimages.py:56-62`` (``crop_transform``) resizes a square ``uint8`` window to
``crop x crop`` with PIL's antialiased bilinear filter and normalises it.  PIL's ``uint8`` resample is two
passes of integer arithmetic over coefficients that it derives in double precision, and the normalisation
is three correctly rounded fp32 operations, so the whole chain has one right answer per input.  This file
states it in numpy: ``tests/test_still_image_host.py`` pins it to the reference's outputs
(``tests/golden/still_image_clips.npz``) and to ``PIL.Image.resize``; the GPU tests compare the kernel
with it bit for bit.

Order of operations of the coefficients (all float64, nothing fused):
    scale = side / crop;  filterscale = max(scale, 1);  support = filterscale;  ss = 1 / filterscale
    center = (xx + 0.5) * scale
    first = max(int(center - support + 0.5), 0);  last = min(int(center + support + 0.5), side)
    w[x] = triangle((x + first - center + 0.5) * ss);  ww = w[0] + w[1] + ... (left to right)
    k[x] = int(0.5 + (w[x] / ww) * 2**22)
Each pass: ``clip((2**21 + sum(pixel * k)) >> 22, 0, 255)`` into ``uint8``; horizontal first.
"""
import numpy as np

PRECISION_BITS = 22
MEAN = np.array([0.43216, 0.394666, 0.37645], dtype=np.float32)
STD = np.array([0.22803, 0.22145, 0.216989], dtype=np.float32)


def ksize(side: int, crop: int) -> int:
    """Row length of the coefficient table: ``2 * ceil(support) + 1``."""
    return 2 * max(-(-side // crop), 1) + 1


def resample_tables(side: int, crop: int):
    """``(coeffs int32 [crop][ksize], bounds int32 [crop][2] = (first, count))`` for ``side -> crop``."""
    ks = ksize(side, crop)
    scale = np.float64(side) / np.float64(crop)
    filterscale = max(scale, np.float64(1.0))
    support = filterscale
    ss = np.float64(1.0) / filterscale
    center = (np.arange(crop, dtype=np.float64) + 0.5) * scale
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates toward zero like (int)
    last = np.minimum((center + support + 0.5).astype(np.int64), side)
    count = last - first
    w = np.zeros((crop, ks), dtype=np.float64)
    ww = np.zeros(crop, dtype=np.float64)
    for x in range(ks):                                                       # left-to-right sum, as the C loop
        arg = np.abs(((x + first).astype(np.float64) - center + 0.5) * ss)
        wx = np.where((arg < 1.0) & (x < count), 1.0 - arg, 0.0)
        w[:, x] = wx
        ww = ww + wx
    k = (0.5 + (w / ww[:, None]) * np.float64(1 << PRECISION_BITS)).astype(np.int64)
    k[np.arange(ks)[None, :] >= count[:, None]] = 0
    return k.astype(np.int32), np.stack([first, count], axis=1).astype(np.int32)


def _pass(src: np.ndarray, coeffs: np.ndarray, bounds: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of ``src`` (uint8, (side, ...)) -> (crop, ...) uint8."""
    out = np.empty((coeffs.shape[0],) + src.shape[1:], dtype=np.uint8)
    wide = src.astype(np.int64)
    for xx in range(coeffs.shape[0]):
        first, count = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.tensordot(coeffs[xx, :count].astype(np.int64), wide[first:first + count], axes=(0, 0))
        out[xx] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def resample_u8(window: np.ndarray, crop: int) -> np.ndarray:
    """``Image.fromarray(window).resize((crop, crop), BILINEAR)`` for a square ``(side, side, C)`` uint8 window."""
    side = window.shape[0]
    assert window.dtype == np.uint8 and window.shape[1] == side
    if side == crop:                                                          # both passes skipped
        return window.copy()
    coeffs, bounds = resample_tables(side, crop)
    horizontal = _pass(window.transpose(1, 0, 2), coeffs, bounds).transpose(1, 0, 2)   # (side, crop, C)
    return _pass(horizontal, coeffs, bounds)                                             # (crop, crop, C)


def normalise(frame_u8: np.ndarray) -> np.ndarray:
    """ToTensor + Normalize: (H, W, 3) uint8 -> (3, H, W) fp32, ``((u8 / 255) - mean) / std`` in fp32."""
    x = frame_u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return (x - MEAN[:, None, None]) / STD[:, None, None]


def camera_motion_clips(img: np.ndarray, trajectory: np.ndarray, crop: int, n_clips: int, clip_len: int) -> np.ndarray:
    """``extract_camera_motion`` from the trajectory on: ``(n_clips, 3, clip_len, crop, crop)`` fp32."""
    assert len(trajectory) == n_clips * clip_len
    frames = [normalise(resample_u8(img[t:t + s, l:l + s], crop)) for t, l, s in np.asarray(trajectory).tolist()]
    out = np.stack(frames).reshape(n_clips, clip_len, 3, crop, crop).transpose(0, 2, 1, 3, 4)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def golden_cases():
    """The cases of ``tests/golden/still_image_clips.npz`` (``tools/make_still_image_golden.py``):
    ``(image, crop, clip_len, n_clips, seed, trajectory, reference output)``."""
    from helpers import load_golden
    g = load_golden("still_image_clips")
    for i in range(int(g["n_cases"])):
        crop, clip_len, n_clips, seed = (int(v) for v in g[f"meta_{i}"])
        yield g[f"image_{i}"], crop, clip_len, n_clips, seed, g[f"trajectory_{i}"], g[f"clip_{i}"]
