"""CPU-side checks of the e4m3 inference surface: the C-ABI geometry queries, the dtype routing of
engine_for / train.evaluate, and the refusals that need no GPU."""
import ctypes

import pytest
import torch

from helpers import make_opt
from zeroshotvideoclassification_amd import _lib, amp, inference, network, synthetic, train

FP8 = torch.float8_e4m3fn


def test_channel_pitch_is_one_64_channel_chunk():
    lib = _lib.load()
    assert [lib.zsv_fp8_channel_pitch(c) for c in (3, 45, 64, 144, 230, 512, 921)] == [4, 64, 64, 192, 256, 512, 960]
    assert [lib.zsv_bf16_channel_pitch(c) for c in (3, 45, 144, 921)] == [4, 64, 160, 928]       # unchanged


def test_blob_bytes():
    lib = _lib.load()
    # S1 of layer1: 64 -> 144, 1x3x3 -- 9 taps x 1 chunk x 144 rows x 64 bytes + 144 shifts + 144 factors
    d = _lib.ConvDesc(22, 64, 32, 56, 56, 144, 32, 56, 56, 1, 3, 3, 1, 1, 1, 0, 1, 1)
    assert lib.zsv_conv3d_fp8_blob_bytes(ctypes.byref(d)) == 9 * 144 * 64 + 144 * 8
    # T1: 144 -> 64, 3x1x1 -- K pitch 192 = 3 chunks
    d = _lib.ConvDesc(22, 144, 32, 56, 56, 64, 32, 56, 56, 3, 1, 1, 1, 1, 1, 1, 0, 0)
    assert lib.zsv_conv3d_fp8_blob_bytes(ctypes.byref(d)) == 3 * 3 * 64 * 64 + 64 * 8
    # the clip convolution keeps the bf16 folded form: 7 (kh) taps x 64 rows x 32 bf16 + shifts + factors
    d = _lib.ConvDesc(1, 3, 8, 118, 120, 45, 8, 56, 56, 1, 7, 7, 1, 2, 2, 0, 0, 0)
    assert lib.zsv_conv3d_fp8_blob_bytes(ctypes.byref(d)) == 7 * 64 * 32 * 2 + 64 * 8
    bad = _lib.ConvDesc(22, 64, 32, 56, 56, 144, 32, 57, 56, 1, 3, 3, 1, 1, 1, 0, 1, 1)     # Ho inconsistent
    assert lib.zsv_conv3d_fp8_blob_bytes(ctypes.byref(bad)) == 0
    assert lib.zsv_conv3d_fp8_fwd(ctypes.byref(bad), None, None, None, 0, None, None) == 1      # ZSV_E_BAD_SHAPE
    d = _lib.ConvDesc(22, 64, 32, 56, 56, 144, 32, 56, 56, 1, 3, 3, 1, 1, 1, 0, 1, 1)
    assert lib.zsv_conv3d_fp8_fwd(ctypes.byref(d), None, None, None, 0, None, None) == 2        # ZSV_E_NULL
    assert lib.zsv_meanpool_fp8(None, 1, 1, 4, None, None) == 1


def test_dtype_routing_without_a_gpu():
    model = network.get_network(make_opt("r2plus1d_18")).eval()
    with pytest.raises(RuntimeError, match="Fp8Engine: the model must live on the MI355X HIP device"):
        inference.engine_for(model, FP8)
    c3d = network.get_network(make_opt("c3d")).eval()
    with pytest.raises(RuntimeError, match="C3D has no fp8"):
        inference.engine_for(c3d, FP8)
    batches = [(synthetic.synthetic_clips(1, 4, 16), torch.zeros(1, dtype=torch.long), torch.zeros(1, 300))]
    table = synthetic.class_table(5)
    with pytest.raises(RuntimeError, match="Fp8Engine"):
        train.evaluate(model, batches, table, device=torch.device("cpu"), dtype=FP8)
    with pytest.raises(RuntimeError, match="not supported"):
        train.evaluate(model, batches, table, device=torch.device("cpu"), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="not supported"):
        amp.autocast(dtype=FP8)                   # autocast stays bf16: fp8 is asked for by dtype only
