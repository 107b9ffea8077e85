"""``preprocess.VideoClips`` / ``zsv_clip_transform_batch`` on the GPU: a batch of videos of different frame sizes in one
launch, against the CPU restatement of the reference's chain (``oracle/transforms_oracle.py``, pinned bit for bit to the
reference's own ``get_transform``) followed by the loader's ``reshape(3, nc, T, c, c).transpose(0, 1)``
(``auxiliary/auxiliary_dataset.py:510``).  Tolerance: the chain's own, max abs difference below 2e-6
(``tests/test_preprocess.py``)."""
import random
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from oracle import transforms_oracle as TO
from zeroshotvideoclassification_amd import _lib, preprocess

pytestmark = pytest.mark.gpu
TOL = 2e-6


def _videos(sizes, frames, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (frames, h, w, 3), dtype=torch.uint8, generator=g) for h, w in sizes]


def _expected(v, top, left, flip, nc, T, crop=112, size=128):
    return TO.clip_transform(v, top, left, bool(flip), crop, size).reshape(3, nc, T, crop, crop).transpose(0, 1)


def _check_against_oracle(clips, videos, params, out):
    nc, T, crop = clips.n_clips, clips.clip_len, clips.crop_size
    assert out.shape == (len(videos), nc, 3, T, crop, crop) and out.dtype == torch.float32
    out = out.cpu()
    for b, (v, (top, left, flip)) in enumerate(zip(videos, params)):
        err = (out[b] - _expected(v, top, left, flip, nc, T, crop, clips.size)).abs().max().item()
        assert err < TOL, (b, tuple(v.shape), err)
    assert out.min() >= -0.5 - 1e-6 and out.max() <= 1e-6                   # input contract of the model


def test_mixed_sizes_match_the_oracle():
    """Landscape, portrait, scale exactly 1, a size where floor(in * scale) matters, and a downscale."""
    sizes = [(120, 160), (200, 130), (128, 171), (113, 200), (240, 320)]
    clips = preprocess.VideoClips(False, n_clips=2, clip_len=3)
    videos = _videos(sizes, 6, seed=1)
    res = [preprocess.resized_hw(h, w, 128)[:2] for h, w in sizes]
    random.seed(5)
    drawn = clips.draw_params(sizes[3:])
    params = [TO.center_crop_params(res[0][0], res[0][1], 112, 112) + (0,), (0, 0, 1), (res[2][0] - 112, res[2][1] - 112, 1)] + drawn
    out = clips([v.cuda() for v in videos], params=params)
    assert out.shape == (5, 2, 3, 3, 112, 112)
    _check_against_oracle(clips, videos, params, out)


def test_smallest_batch():
    clips = preprocess.VideoClips(True, n_clips=1, clip_len=1)
    videos = _videos([(128, 128)], 1, seed=2)
    out = clips([videos[0].cuda()])
    _check_against_oracle(clips, videos, [(8, 8, 0)], out)


def test_five_dimensional_and_non_contiguous_input():
    clips = preprocess.VideoClips(False, n_clips=2, clip_len=3)
    sizes = [(120, 160), (200, 130)]
    videos = [v.cuda() for v in _videos(sizes, 6, seed=3)]
    params = [(3, 40, 1), (60, 9, 0)]
    flat = clips(videos, params=params)
    five = clips([v.view(2, 3, *v.shape[1:]) for v in videos], params=params)
    assert torch.equal(flat, five)
    wide = [torch.randint(0, 256, (6, h + 5, w + 7, 3), dtype=torch.uint8, device="cuda") for h, w in sizes]
    for big, v in zip(wide, videos):
        big[:, 2:-3, 4:-3] = v
    views = [big[:, 2:-3, 4:-3] for big in wide]
    assert not any(v.is_contiguous() for v in views)
    assert torch.equal(flat, clips(views, params=params))
    assert torch.equal(flat, clips([videos[0], views[1].view(2, 3, *views[1].shape[1:])], params=params))


def test_bit_identical_to_the_dense_kernel_on_one_size():
    """Both kernels call one device function per pixel, so on videos of one size they agree bit for bit."""
    videos = [v.cuda() for v in _videos([(120, 160)] * 3, 4, seed=4)]
    params = [(8, 29, 0), (0, 58, 1), (16, 0, 1)]
    batch = preprocess.VideoClips(False, n_clips=1, clip_len=4)(videos, params=params)
    dense = preprocess.ClipTransform(False)(torch.stack(videos), params=params)
    assert batch.shape == (3, 1, 3, 4, 112, 112)
    assert torch.equal(batch, dense.unsqueeze(1))


def test_the_other_resolution():
    sizes = [(240, 320), (300, 260)]
    clips = preprocess.VideoClips(False, n_clips=1, clip_len=2, crop_size=224)
    assert clips.size == 256
    videos = _videos(sizes, 2, seed=6)
    res = [preprocess.resized_hw(h, w, 256)[:2] for h, w in sizes]
    params = [(res[0][0] - 224, 7, 1), (11, res[1][1] - 224, 0)]
    out = clips([v.cuda() for v in videos], params=params)
    _check_against_oracle(clips, videos, params, out)


def test_own_draws_are_the_draws_of_draw_params():
    sizes = [(120, 160), (200, 130), (113, 200)]
    clips = preprocess.VideoClips(False, n_clips=1, clip_len=2)
    videos = [v.cuda() for v in _videos(sizes, 2, seed=7)]
    random.seed(9)
    params = clips.draw_params(sizes)
    random.seed(9)
    out = clips(videos)
    assert torch.equal(out, clips(videos, params=params))
    val = preprocess.VideoClips(True, n_clips=1, clip_len=2)
    assert torch.equal(val(videos), val(videos, params=val.draw_params(sizes)))


def test_staging_rounds_reuse_and_grow_the_pinned_buffers():
    clips = preprocess.VideoClips(True, n_clips=1, clip_len=2)
    rounds = [[(120, 160), (128, 171)], [(113, 200)], [(200, 130), (120, 160), (240, 320)]]       # bytes: 246 k, 136 k, 732 k
    kept, buffers = [], []
    for r, sizes in enumerate(rounds):
        arrays = [v.numpy() for v in _videos(sizes, 2, seed=20 + r)]
        if r == 1:
            arrays = [torch.from_numpy(arrays[0]).view(1, 2, 113, 200, 3)]                     # a tensor, five-dimensional
        staged = clips.stage(arrays)
        assert [tuple(s.shape) for s in staged] == [tuple(a.shape) for a in arrays]
        assert all(s.is_cuda and s.dtype == torch.uint8 for s in staged)
        out = clips(staged)
        plain = clips([torch.as_tensor(a).cuda() for a in arrays])
        assert torch.equal(out, plain), r
        kept.append((out, plain.clone()))
        buffers.append([None if s is None else s[0].data_ptr() for s in clips._staging])
    # two buffers in alternation: round 2 filled the second, round 3 came back to the first and had to replace it
    assert buffers[0][1] is None and buffers[1][0] == buffers[0][0] and buffers[2][1] == buffers[1][1]
    assert buffers[2][0] != buffers[0][0] and clips._staging[0][0].is_pinned() and clips._staging[1][0].is_pinned()
    torch.cuda.synchronize()
    for out, plain in kept:                                                 # no later round changed an earlier result
        assert torch.equal(out, plain)
    # a smaller batch fits the buffer it meets: nothing is replaced
    before = [s[0].data_ptr() for s in clips._staging]
    clips.stage([np.zeros((2, 113, 200, 3), np.uint8)])
    assert [s[0].data_ptr() for s in clips._staging] == before


def test_raw_c_abi_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    table = torch.zeros(preprocess.CLIP_ROW, dtype=torch.int64, device="cuda")
    out = torch.zeros(3 * 16 * 16, dtype=torch.float32, device="cuda")
    assert lib.zsv_clip_transform_batch(None, 1, 1, 1, 16, out.data_ptr(), stream) == 2          # ZSV_E_NULL
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 1, 1, 1, 16, None, stream) == 2
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 0, 1, 1, 16, out.data_ptr(), stream) == 1   # ZSV_E_BAD_SHAPE
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 1, 1, 1, 0, out.data_ptr(), stream) == 1
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 1, 0, 1, 16, out.data_ptr(), stream) == 1
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 1, 1, -1, 16, out.data_ptr(), stream) == 1
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 1, 1, 1, 65536, out.data_ptr(), stream) == 4   # ZSV_E_TOO_LARGE: 2^33 values
    assert lib.zsv_clip_transform_batch(table.data_ptr(), 1, 4096, 16, 16, out.data_ptr(), stream) == 4  # 65536 frames per video
    torch.cuda.synchronize()
    assert not out.any()                                                    # nothing was launched


def test_a_row_that_breaks_the_contract_is_not_read():
    """The caller validates the table; the kernel still does not read a video whose window lies outside the resized
    frame: it becomes NaN and its neighbours are untouched.  (Every pointer in the table is a live video.)"""
    clips = preprocess.VideoClips(False, n_clips=1, clip_len=2, crop_size=16)              # (short side 256)
    videos = [v.cuda() for v in _videos([(40, 50)] * 3, 2, seed=8)]
    good = [(5, 7, 1)] * 3
    want = clips(videos, params=good)
    table = preprocess.video_table([v.data_ptr() for v in videos], [(40, 50)] * 3, good, clips.size)
    assert table[0, 3:5].tolist() == [256, 320]
    table[0, 5] = 256 - 15                                                  # top + crop = Hres + 1
    table[2, 6] = -1                                                        # left < 0
    vtab = torch.from_numpy(table).cuda()
    out = torch.zeros_like(want)
    _lib.check(_lib.load().zsv_clip_transform_batch(vtab.data_ptr(), 3, 1, 2, 16, out.data_ptr(),
                                                    c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_clip_transform_batch")
    assert torch.isnan(out[0]).all() and torch.isnan(out[2]).all()
    assert torch.equal(out[1], want[1])
