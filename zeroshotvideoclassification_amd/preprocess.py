"""Clip pre-processing on the GPU behind the reference's ``get_transform`` surface.

``get_transform(is_validation, crop_size=112)`` (auxiliary/transforms.py:41-56) returns a callable
like the reference's ``Compose``; the difference is what it accepts and where it runs: the
reference transforms one ``(T, H, W, 3)`` uint8 clip on a CPU worker and ships fp32 to the GPU
(53 MB per 22-clip batch); here a batch of uint8 clips (13 MB) is uploaded and the whole chain
-- (u8/255-1)/2, THWC->CTHW, bilinear short-side-128 resize, 112 crop, horizontal flip -- is one
HIP kernel writing the ``(N, 3, T, 112, 112)`` model input.  Random crop / flip parameters are
drawn on the host with Python's ``random`` exactly like ``RandomCrop.get_params`` /
``RandomHorizontalFlip`` (transforms.py:137-147,192-195), one draw per clip.

``StillImageClips`` is the same move for the still-image source (``main.py --dataset sun2both``,
``auxiliary/auxiliary_stillimages.py:92-138``): the uint8 images are uploaded once and one HIP launch
crops, resamples (PIL's antialiased bilinear, bit for bit) and normalises every frame of every
camera-motion clip of the batch.

``VideoClips`` / ``get_batch_transform`` is ``ClipTransform`` for what the reference's loader really yields
(``auxiliary/auxiliary_dataset.py:158-208,498-510``): videos decoded at their native, DIFFERENT frame sizes, one crop / flip
draw per video shared by its ``n_clips`` clips, collated to ``(bs, nc, 3, T, 112, 112)``.  A device table describes the
videos, one launch transforms them all; ``VideoClips.stage`` is the loader-side upload (one pinned buffer, one copy).
"""
from __future__ import annotations

import random
import warnings
from ctypes import c_void_p
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def resized_hw(h: int, w: int, size: int):
    """Output size and source step of ``resize(vid, size)`` (transforms.py:99-107): scale =
    size / min(h, w) handed to ``F.interpolate(scale_factor=...)``."""
    scale = float(size) / min(h, w)
    return int(h * scale), int(w * scale), 1.0 / scale       # floor(in * scale); torch keeps 1/scale as float


class ClipTransform:
    def __init__(self, is_validation: bool, crop_size: int = 112):
        self.is_validation = bool(is_validation)
        self.crop_size = int(crop_size)
        self.size = 128 if crop_size == 112 else 256           # transforms.py:42

    def draw_params(self, n: int, hres: int, wres: int):
        th = tw = self.crop_size
        rows = []
        for _ in range(n):
            if self.is_validation:                               # CenterCrop (transforms.py:80-85)
                i, j = int(round((hres - th) / 2.)), int(round((wres - tw) / 2.))
                flip = 0
            else:                                                # RandomCrop + RandomHorizontalFlip
                i = 0 if hres == th and wres == tw else random.randint(0, hres - th)
                j = 0 if hres == th and wres == tw else random.randint(0, wres - tw)
                flip = 1 if random.random() < 0.5 else 0
            rows.append((i, j, flip))
        return rows

    def __call__(self, frames_u8: torch.Tensor, params: Optional[Sequence[Sequence[int]]] = None) -> torch.Tensor:
        """``frames_u8``: ``(N, T, H, W, 3)`` (or one clip ``(T, H, W, 3)``) uint8 on a HIP device.
        Returns ``(N, 3, T, crop, crop)`` fp32 (``(3, T, crop, crop)`` for a single clip)."""
        single = frames_u8.dim() == 4
        if single:
            frames_u8 = frames_u8.unsqueeze(0)
        if frames_u8.dim() != 5 or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8:
            raise RuntimeError("expected (N, T, H, W, 3) uint8 frames")
        if not frames_u8.is_cuda:
            raise RuntimeError("ClipTransform runs on an MI355X HIP device only (no CPU fallback; "
                               "the CPU restatement lives in oracle/)")
        frames_u8 = frames_u8.contiguous()
        n, t, h, w, _ = (int(v) for v in frames_u8.shape)
        hres, wres, inv_scale = resized_hw(h, w, self.size)
        if hres < self.crop_size or wres < self.crop_size:
            raise RuntimeError("clip too small for the crop")
        if params is None:
            params = self.draw_params(n, hres, wres)
        if len(params) != n:
            raise RuntimeError("one (top, left, flip) triple per clip expected")
        for (i, j, _f) in params:
            if not (0 <= i <= hres - self.crop_size and 0 <= j <= wres - self.crop_size):
                raise RuntimeError("crop window outside the resized frame")
        # pinned + non_blocking: a pageable upload would drain the stream every call (the host could no longer run ahead)
        ptab = torch.tensor(params, dtype=torch.int32).pin_memory().to(frames_u8.device, non_blocking=True)
        out = torch.empty((n, 3, t, self.crop_size, self.crop_size), dtype=torch.float32, device=frames_u8.device)
        with torch.cuda.device(frames_u8.device):
            _lib.check(_lib.load().zsv_clip_transform(frames_u8.data_ptr(), n, t, h, w, hres, wres, float(inv_scale),
                                                      self.crop_size, ptab.data_ptr(), out.data_ptr(),
                                                      c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "zsv_clip_transform")
        return out[0] if single else out


def get_transform(is_validation, crop_size=112):
    return ClipTransform(is_validation, crop_size)


# ---- batches of videos of different frame sizes (auxiliary/auxiliary_dataset.py:158-208,498-510) -------------------------
CLIP_ROW = 8                # int64 words per row of the video table (ZSV_CLIP_ROW, include/zsv_hip.h)


def video_table(pointers: Sequence[int], sizes: Sequence[Sequence[int]], params: Sequence[Sequence[int]], size: int) -> np.ndarray:
    """The ``(B, 8)`` int64 table of ``zsv_clip_transform_batch`` (row format: include/zsv_hip.h), a pure host function:
    ``[pointer, Hin, Win, Hres, Wres, top, left, flip | bits of float32(1 / scale) << 32]`` per video, with
    ``Hres, Wres, 1 / scale = resized_hw(Hin, Win, size)``."""
    table = np.empty((len(pointers), CLIP_ROW), dtype=np.int64)
    for b, (ptr, (h, w), (top, left, flip)) in enumerate(zip(pointers, sizes, params)):
        hres, wres, inv_scale = resized_hw(int(h), int(w), size)
        bits = int(np.float32(inv_scale).view(np.uint32))
        table[b] = (int(ptr), int(h), int(w), hres, wres, int(top), int(left), (bits << 32) | (1 if flip else 0))
    return table


class VideoClips:
    """The reference loader's per-video transform (``auxiliary/auxiliary_dataset.py:498-510``) for a whole batch of
    videos of DIFFERENT frame sizes in one HIP launch: every video gets one crop / flip draw shared by its ``n_clips``
    clips, and the ``(nc*T) -> (nc, 3, T)`` reshuffle of :506-510 is done by the kernel's store."""

    def __init__(self, is_validation: bool, n_clips: int = 1, clip_len: int = 16, crop_size: int = 112):
        self.n_clips, self.clip_len = int(n_clips), int(clip_len)
        if self.n_clips <= 0 or self.clip_len <= 0 or int(crop_size) <= 0:
            raise ValueError("n_clips, clip_len and crop_size must be positive")
        self._clip = ClipTransform(is_validation, crop_size)
        self.is_validation, self.crop_size, self.size = self._clip.is_validation, self._clip.crop_size, self._clip.size
        self._staging = [None, None]        # two pinned buffers in alternation, each [buffer, event of its last upload]
        self._turn = 0

    def draw_params(self, sizes: Sequence[Sequence[int]]):
        """One ``(top, left, flip)`` per video, in video order; ``sizes``: the ``(H, W)`` of every video's frames.
        Consumes Python's ``random`` exactly as ``ClipTransform.draw_params(1, hres, wres)`` per video in turn."""
        rows = []
        for h, w in sizes:
            hres, wres, _ = resized_hw(int(h), int(w), self.size)
            if hres < self.crop_size or wres < self.crop_size:
                raise RuntimeError("clip too small for the crop")
            rows.extend(self._clip.draw_params(1, hres, wres))
        return rows

    def _check(self, videos, params):
        """Everything ``__call__`` refuses, before any device is touched.  Returns the ``(H, W)`` of every video."""
        frames, crop = self.n_clips * self.clip_len, self.crop_size
        if not videos:
            raise RuntimeError("expected at least one video")
        sizes = []
        for v in videos:
            if not isinstance(v, torch.Tensor) or v.dim() not in (4, 5) or v.shape[-1] != 3 or v.dtype != torch.uint8:
                raise RuntimeError("expected (n_clips*clip_len, H, W, 3) or (n_clips, clip_len, H, W, 3) uint8 videos")
            lead = tuple(int(d) for d in v.shape[:-3])
            if lead != (frames,) and lead != (self.n_clips, self.clip_len):
                raise RuntimeError(f"expected {self.n_clips} x {self.clip_len} = {frames} frames per video, got {lead}")
            h, w = int(v.shape[-3]), int(v.shape[-2])
            hres, wres, _ = resized_hw(h, w, self.size) if min(h, w) > 0 else (0, 0, 0.0)
            if hres < crop or wres < crop:
                raise RuntimeError("clip too small for the crop")
            sizes.append((h, w))
        if params is not None:
            if len(params) != len(videos):
                raise RuntimeError("one (top, left, flip) triple per video expected")
            for (h, w), (i, j, _f) in zip(sizes, params):
                hres, wres, _ = resized_hw(h, w, self.size)
                if not (0 <= i <= hres - crop and 0 <= j <= wres - crop):
                    raise RuntimeError("crop window outside the resized frame")
        for v in videos:
            if not v.is_cuda:
                raise RuntimeError("VideoClips runs on an MI355X HIP device only (no CPU fallback; "
                                   "the CPU restatement lives in oracle/)")
            if v.device != videos[0].device:
                raise RuntimeError("all videos must live on one device")
        return sizes

    def __call__(self, videos: Sequence[torch.Tensor], params: Optional[Sequence[Sequence[int]]] = None) -> torch.Tensor:
        """``videos``: a sequence of uint8 tensors on one HIP device, each ``(n_clips*clip_len, H_i, W_i, 3)`` or
        ``(n_clips, clip_len, H_i, W_i, 3)``; ``params``: one ``(top, left, flip)`` per video (drawn by ``draw_params`` when
        not given).  Returns ``(B, n_clips, 3, clip_len, crop, crop)`` fp32, the input of ``Model.forward``."""
        videos = list(videos)
        sizes = self._check(videos, params)
        if params is None:
            params = self.draw_params(sizes)
        device = videos[0].device
        videos = [v.contiguous() for v in videos]                # (a copy made here is freed in stream order, after the launch)
        table = video_table([v.data_ptr() for v in videos], sizes, params, self.size)
        # pinned + non_blocking: a pageable upload would drain the stream every call (the host could no longer run ahead)
        vtab = torch.from_numpy(table).pin_memory().to(device, non_blocking=True)
        out = torch.empty((len(videos), self.n_clips, 3, self.clip_len, self.crop_size, self.crop_size), dtype=torch.float32,
                          device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.load().zsv_clip_transform_batch(vtab.data_ptr(), len(videos), self.n_clips, self.clip_len, self.crop_size,
                                                            out.data_ptr(), c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "zsv_clip_transform_batch")
        return out

    def stage(self, arrays: Sequence, device="cuda"):
        """The loader-side half: ``arrays`` (CPU uint8 arrays or tensors of different sizes) are copied back to back into
        one pinned staging buffer and uploaded with ONE ``non_blocking`` copy on the current stream; returns the device
        views, one per video, in the shapes given.  Two staging buffers alternate; each carries the event of its last
        upload, which is waited for on the host before the buffer is overwritten, and a buffer is replaced only when a
        batch needs more room.  The device buffer behind the views is the caller's: the launch reads it in stream order."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("VideoClips.stage uploads to an MI355X HIP device only (no CPU fallback)")
        sources = []
        for a in arrays:
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a)
                with warnings.catch_warnings():                  # a read-only array from a loader is a fine source: it is only read
                    warnings.simplefilter("ignore", UserWarning)
                    a = torch.from_numpy(a) if a.dtype == np.uint8 else None
            if a is None or a.dtype != torch.uint8 or a.is_cuda:
                raise RuntimeError("expected CPU uint8 arrays")
            sources.append(a)
        if not sources:
            raise RuntimeError("expected at least one video")
        offsets, total = [], 0
        for a in sources:
            offsets.append(total)
            total += -(-a.numel() // 256) * 256                  # every video starts on a 256-byte boundary
        slot = self._staging[self._turn]
        if slot is not None:
            slot[1].synchronize()                                # the upload that last read this buffer has finished
        if slot is None or slot[0].numel() < total:
            slot = self._staging[self._turn] = [torch.empty(total, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self._turn ^= 1
        pinned = slot[0]
        for a, off in zip(sources, offsets):
            pinned[off:off + a.numel()].view(a.shape).copy_(a)   # (torch's copy uses the host's threads)
        with torch.cuda.device(device):
            dev = torch.empty(total, dtype=torch.uint8, device=device)
            dev.copy_(pinned[:total], non_blocking=True)
            slot[1].record()
        return [dev[off:off + a.numel()].view(a.shape) for a, off in zip(sources, offsets)]


def get_batch_transform(is_validation, n_clips=1, clip_len=16, crop_size=112):
    return VideoClips(is_validation, n_clips, clip_len, crop_size)


# ---- still images (auxiliary/auxiliary_stillimages.py) ---------------------------------------------------------------
MAX_SIDE_RATIO = 8          # side / crop the kernel supports (17 taps per axis); the reference never exceeds 512 / 112


def prepare_still_image(img: np.ndarray) -> np.ndarray:
    """The channel handling of ``extract_camera_motion`` (auxiliary_stillimages.py:105-112) that has a defined
    result: a grey ``(H, W)`` or one-channel ``(H, W, 1)`` image is repeated to three channels, RGBA loses its
    alpha, RGB passes through; anything else raises (the reference's two-channel branch at :108-109 cannot run).
    Returns a contiguous ``(H, W, 3)`` uint8 array.

    NOT done here: the rescale of :93-103 (short side below 172 is enlarged by an integer factor, above 512 reduced
    to 512, through ``skimage.transform.resize``).  That is loader work next to the image decode; do it before this
    call for images outside 172 ... 512."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f"expected a uint8 image, got {img.dtype}")
    if img.ndim == 2:
        img = img[:, :, None]
    if img.ndim != 3 or img.shape[2] not in (1, 3, 4):
        raise ValueError(f"expected a (H, W), (H, W, 1), (H, W, 3) or (H, W, 4) image, got {img.shape}")
    if img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    return np.ascontiguousarray(img[:, :, :3])


def _draw_window(h: int, w: int, crop: int):
    top = np.random.randint(0, max(h - crop, 1))
    left = np.random.randint(0, max(w - crop, 1))
    side = np.random.randint(crop, max(min(h - top, w - left), crop + 1))
    return top, left, side


def camera_motion_trajectory(h: int, w: int, crop: int, frames: int) -> np.ndarray:
    """The window trajectory of ``extract_camera_motion`` (auxiliary_stillimages.py:118-127): a start and an end
    window, each drawn as top, left, side with ``np.random.randint`` (six draws, in the reference's order), joined
    by ``np.linspace(...).astype(int)``.  Under the same ``np.random.seed`` this is the reference's trajectory.
    Returns ``(frames, 3)`` int rows ``(top, left, side)``."""
    start, end = _draw_window(h, w, crop), _draw_window(h, w, crop)
    return np.ascontiguousarray(np.stack([np.linspace(a, b, frames).astype(int) for a, b in zip(start, end)]).T)


class StillImageClips:
    """``ImageDataset.extract_camera_motion`` for a batch of images in one HIP launch
    (``ImageDataset(..., clip_len=8, n_clips=1, crop_size=112)``, auxiliary_stillimages.py:33-34)."""

    def __init__(self, clip_len: int = 8, n_clips: int = 1, crop_size: int = 112):
        self.clip_len, self.n_clips, self.crop_size = int(clip_len), int(n_clips), int(crop_size)
        if self.clip_len <= 0 or self.n_clips <= 0 or self.crop_size <= 0:
            raise ValueError("clip_len, n_clips and crop_size must be positive")

    def __call__(self, images: Sequence[torch.Tensor], trajectories: Optional[Sequence] = None) -> torch.Tensor:
        """``images``: a sequence of ``(H, W, 3)`` uint8 tensors on one HIP device (``prepare_still_image`` output,
        sizes may differ).  ``trajectories``: one ``(n_clips * clip_len, 3)`` int array of ``(top, left, side)`` per
        image; drawn with ``camera_motion_trajectory`` (``np.random``) in image order when not given.
        Returns ``(B, n_clips, 3, clip_len, crop, crop)`` fp32, the input of ``Model.forward``."""
        crop, frames = self.crop_size, self.n_clips * self.clip_len
        images = list(images)
        if not images:
            raise RuntimeError("expected at least one image")
        for img in images:
            if not isinstance(img, torch.Tensor) or img.dim() != 3 or img.shape[-1] != 3 or img.dtype != torch.uint8:
                raise RuntimeError("expected (H, W, 3) uint8 images")
            if not img.is_cuda:
                raise RuntimeError("StillImageClips runs on an MI355X HIP device only (no CPU fallback; "
                                   "the CPU restatement lives in tests/still_image_oracle.py)")
            if img.device != images[0].device:
                raise RuntimeError("all images must live on one device")
        if trajectories is None:
            trajectories = [camera_motion_trajectory(int(img.shape[0]), int(img.shape[1]), crop, frames) for img in images]
        if len(trajectories) != len(images):
            raise RuntimeError("one trajectory per image expected")
        table = np.empty((len(images), frames, 3), dtype=np.int32)
        for b, (img, traj) in enumerate(zip(images, trajectories)):
            traj = np.asarray(traj)
            if traj.shape != (frames, 3) or traj.dtype.kind not in "iu":
                raise RuntimeError(f"expected an integer ({frames}, 3) trajectory of (top, left, side) per image")
            top, left, side = traj[:, 0], traj[:, 1], traj[:, 2]
            if (side < crop).any():
                raise RuntimeError("window side smaller than the crop")
            if (side > MAX_SIDE_RATIO * crop).any():
                raise RuntimeError(f"window side larger than {MAX_SIDE_RATIO} x the crop")
            if (top < 0).any() or (left < 0).any() or (top + side > img.shape[0]).any() or (left + side > img.shape[1]).any():
                raise RuntimeError("window outside the image")
            table[b] = traj
        device = images[0].device
        images = [img.contiguous() for img in images]            # (a copy made here is freed in stream order, after the launch)
        itab = torch.tensor([[img.data_ptr(), img.shape[0], img.shape[1]] for img in images], dtype=torch.int64)
        # pinned + non_blocking: a pageable upload would drain the stream every call (the host could no longer run ahead)
        itab = itab.pin_memory().to(device, non_blocking=True)
        ftab = torch.from_numpy(table).pin_memory().to(device, non_blocking=True)
        out = torch.empty((len(images), self.n_clips, 3, self.clip_len, crop, crop), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.load().zsv_still_image_clips(itab.data_ptr(), ftab.data_ptr(), len(images), self.n_clips, self.clip_len,
                                                         crop, int(table[:, :, 2].max()), out.data_ptr(),
                                                         c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "zsv_still_image_clips")
        return out


def resample_coeffs(side: int, crop: int, device="cuda"):
    """The integer tables of one ``side -> crop`` resample as the kernel derives them (``zsv_resample_coeffs``):
    ``(coeffs (crop, ksize) int32, bounds (crop, 2) int32 = (first, count))`` on ``device``."""
    side, crop = int(side), int(crop)
    if crop <= 0 or side < crop or side > MAX_SIDE_RATIO * crop:
        raise RuntimeError(f"expected crop <= side <= {MAX_SIDE_RATIO} x crop")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("resample_coeffs runs on an MI355X HIP device only (no CPU fallback)")
    ksize = 2 * -(-side // crop) + 1
    coeffs = torch.empty((crop, ksize), dtype=torch.int32, device=device)
    bounds = torch.empty((crop, 2), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().zsv_resample_coeffs(side, crop, coeffs.data_ptr(), bounds.data_ptr(),
                                                   c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_resample_coeffs")
    return coeffs, bounds
