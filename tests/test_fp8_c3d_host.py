"""CPU-side checks of the calibrated e4m3 engine of network.C3D: the scale rule, the scales kept on the module,
the two new C entry points' surface and argument checks, and the refusals that need no GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from helpers import make_opt
from zeroshotvideoclassification_amd import _lib, inference, network

FP8 = torch.float8_e4m3fn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c3d():
    return network.get_network(make_opt("c3d")).eval()


def test_fp8_scale_values():
    assert inference.fp8_scale(112.0) == 1.0
    assert inference.fp8_scale(112.0001) == 2.0
    assert inference.fp8_scale(0.727) == 2.0 ** -7
    assert inference.fp8_scale(1820.0) == 32.0
    assert inference.fp8_scale(0.0) == 1.0
    assert inference.fp8_scale(448.0, headroom=1.0) == 1.0
    assert inference.fp8_scale(math.nextafter(448.0, math.inf), headroom=1.0) == 2.0
    assert inference.fp8_scale(448.0001, headroom=1.0) == 2.0
    # the definition, on every binade a layer can land in: the stored maximum lies in (448 / (2 * headroom), 448 / headroom]
    for e in range(-30, 31):
        for m in (1.0, 1.0 + 2.0 ** -20, 1.37, 2.0 - 2.0 ** -20):
            amax = m * 2.0 ** e
            for headroom in (1.0, 2.0, 4.0, 8.0):
                s = inference.fp8_scale(amax, headroom)
                assert math.frexp(s)[0] == 0.5, "a power of two"
                assert 448.0 / (2 * headroom) < amax / s <= 448.0 / headroom, (amax, headroom, s)


@pytest.mark.parametrize("bad", [-1.0, -0.001, float("inf"), float("-inf"), float("nan")])
def test_fp8_scale_refuses(bad):
    with pytest.raises(ValueError):
        inference.fp8_scale(bad)


def test_fp8_scale_refuses_a_bad_headroom():
    for bad in (0.0, -4.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            inference.fp8_scale(1.0, headroom=bad)


def test_scales_round_trip_outside_the_state_dict():
    model = _c3d()
    assert inference.fp8_scales(model) is None
    before = set(model.state_dict())
    scales = [2.0 ** -7, 2.0 ** -6, 0.25, 0.5, 1.0, 2.0, 4.0, 32.0]
    inference.set_fp8_scales(model, scales)
    assert inference.fp8_scales(model) == tuple(scales)
    assert set(model.state_dict()) == before, "the checkpoint format stays the reference's"
    assert not any("fp8" in k for k in model.state_dict())
    inference.set_fp8_scales(torch.nn.DataParallel(model), [1.0] * 8)       # stored on the unwrapped module
    assert inference.fp8_scales(model) == (1.0,) * 8


@pytest.mark.parametrize("bad", [[1.0] * 7, [1.0] * 9, [], [1.0] * 7 + [0.0], [1.0] * 7 + [-2.0], [float("inf")] + [1.0] * 7,
                                 [1.0] * 3 + [float("nan")] + [1.0] * 4, 1.0],
                         ids=["seven", "nine", "empty", "zero", "negative", "inf", "nan", "scalar"])
def test_set_fp8_scales_refuses(bad):
    model = _c3d()
    with pytest.raises(ValueError):
        inference.set_fp8_scales(model, bad)
    assert inference.fp8_scales(model) is None
    with pytest.raises(ValueError):
        inference.Fp8EngineC3D(model, scales=bad)


def test_scales_belong_to_c3d_only():
    model = network.get_network(make_opt("r2plus1d_18"))
    with pytest.raises(RuntimeError, match="network.C3D"):
        inference.set_fp8_scales(model, [1.0] * 8)


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    declared = set(re.findall(r"\b(zsv_[a-z0-9_]+)\s*\(", header))
    for sym in ("zsv_maxpool3d_fp8", "zsv_absmax_bf16"):
        assert sym in declared, f"{sym} is not declared in include/zsv_hip.h"
        assert sym in _lib.SIGNATURES
        assert getattr(lib, sym).argtypes == _lib.SIGNATURES[sym][1]
    assert _lib.SIGNATURES["zsv_maxpool3d_fp8"] == _lib.SIGNATURES["zsv_maxpool3d_bf16"]


POOL_ARGS = {
    "ok geometry, null pointers": ((2, 64, 4, 12, 12, 1, 2, 2, 0, 0, 0, 4, 6, 6), 2),
    "no clips": ((0, 64, 4, 12, 12, 1, 2, 2, 0, 0, 0, 4, 6, 6), 1),
    "a clip's channel count": ((2, 3, 4, 12, 12, 1, 2, 2, 0, 0, 0, 4, 6, 6), 1),
    "zero kernel": ((2, 64, 4, 12, 12, 0, 2, 2, 0, 0, 0, 4, 6, 6), 1),
    "negative padding": ((2, 64, 4, 12, 12, 1, 2, 2, 0, -1, 0, 4, 6, 6), 1),
    "2 * pad > kernel": ((2, 64, 4, 12, 12, 1, 2, 2, 1, 0, 0, 6, 6, 6), 1),
    "output extent": ((2, 64, 4, 12, 12, 1, 2, 2, 0, 0, 0, 4, 6, 7), 1),
    "padded output extent": ((3, 512, 2, 7, 7, 2, 2, 2, 0, 1, 1, 1, 4, 4), 2),
    "empty output": ((1, 64, 1, 4, 4, 2, 2, 2, 0, 0, 0, 0, 2, 2), 1),
}


@pytest.mark.parametrize("what", list(POOL_ARGS))
def test_maxpool3d_fp8_argument_checks_are_the_bf16_pool_s(what):
    lib = _lib.load()
    args, status = POOL_ARGS[what]
    assert lib.zsv_maxpool3d_fp8(None, *args, None, None) == status
    assert lib.zsv_maxpool3d_bf16(None, *args, None, None) == status


def test_maxpool3d_fp8_size_guard():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                       # never dereferenced: both calls return before a launch
    # 2^31 16-byte pieces of input (e4m3: 16 channels each) and the bf16 pool's 2^31 pieces (8 channels each)
    assert lib.zsv_maxpool3d_fp8(one, 2048, 64, 64, 64, 64, 2, 2, 2, 0, 0, 0, 32, 32, 32, one, None) == 4        # ZSV_E_TOO_LARGE
    assert lib.zsv_maxpool3d_bf16(one, 1024, 64, 64, 64, 64, 2, 2, 2, 0, 0, 0, 32, 32, 32, one, None) == 4


def test_absmax_bf16_argument_checks():
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.zsv_absmax_bf16(None, 8, None, None) == 2            # ZSV_E_NULL
    assert lib.zsv_absmax_bf16(one, 8, None, None) == 2
    assert lib.zsv_absmax_bf16(None, 8, one, None) == 2
    assert lib.zsv_absmax_bf16(one, -1, one, None) == 1             # ZSV_E_BAD_SHAPE
    assert lib.zsv_absmax_bf16(one, 0, one, None) == 0              # nothing to read: *amax stays


def test_uncalibrated_c3d_is_refused_with_what_to_do():
    model = _c3d()
    for make in (lambda: inference.engine_for(model, FP8), lambda: inference.Fp8EngineC3D(model)):
        with pytest.raises(RuntimeError, match="C3D has no fp8") as e:
            make()
        assert str(e.value).startswith("C3D has no fp8 (float8_e4m3fn) engine")
        assert "inference.calibrate_fp8(model, clips)" in str(e.value)


def test_calibrated_c3d_on_the_cpu_is_refused():
    model = _c3d()
    inference.set_fp8_scales(model, [1.0] * 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.engine_for(model, FP8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.Fp8EngineC3D(model, scales=[2.0] * 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.calibrate_fp8(model, torch.zeros(1, 3, 16, 112, 112))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.maxpool3d_fp8(torch.zeros((1, 2, 4, 4, 64), dtype=torch.uint8).view(FP8), 64, (1, 2, 2), (0, 0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.absmax_bf16(torch.zeros(8, dtype=torch.bfloat16), torch.zeros(1))
