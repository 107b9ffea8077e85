"""Host side of the one-launch bf16 input gradient (``zsv_conv3d_bf16_dgrad_blob_bytes`` / ``_pack`` / ``zsv_conv3d_bf16_dgrad``; no
GPU needed): the C ABI is declared, exported and bound; the blob size per geometry; what is refused, before any launch; the
residue classes of ``Bf16TrainPath._axis_classes`` partition an axis and name the right taps; the cases
``test_bf16_dgrad_gpu.py`` adds to ``bf16_exact_cases.DGRAD_CASES`` meet the precondition of exact fp32 accumulation."""
import ctypes
import os
import re
from ctypes import byref

import pytest
import torch

import bf16_exact_cases as X
from zeroshotvideoclassification_amd import _lib, amp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BAD_SHAPE, E_NULL, E_UNSUPPORTED = 0, 1, 2, 6

# the cases added to X.DGRAD_CASES by the GPU test (the issue's table): (N, Cin, T, H, W), Cout, kernel, stride, padding
EXTRA_CASES = [
    X.GradCase("x0", (2, 96, 5, 6, 6), 64, (3, 1, 1), (2, 1, 1), (1, 0, 0)),       # odd T: two classes of 3 and 2 frames
    X.GradCase("x1", (3, 45, 2, 7, 5), 72, (1, 3, 3), (1, 2, 2), (0, 1, 1)),       # 45 dx channels (pitch 64), three clips, odd H and W
    X.GradCase("x2", (1, 64, 3, 5, 5), 128, (1, 1, 1), (2, 2, 2), (0, 0, 0)),      # shortcut on odd extents
    X.GradCase("x3", (1, 32, 2, 4, 4), 32, (3, 3, 3), (2, 2, 2), (1, 1, 1)),       # eight classes, each far below one tile
]
ALL_CASES = X.DGRAD_CASES + EXTRA_CASES


def forward_desc(case):
    """The FORWARD descriptor of a case (what the three entry points take)."""
    n, cin, t, h, w = case.xs
    to, ho, wo = X.out_dims((t, h, w), case.kernel, case.stride, case.padding)
    return _lib.ConvDesc(n, cin, t, h, w, case.cout, to, ho, wo, *case.kernel, *case.stride, *case.padding)


def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    P, D = ctypes.c_void_p, ctypes.POINTER(_lib.ConvDesc)
    want = {"zsv_conv3d_bf16_dgrad_blob_bytes": (ctypes.c_size_t, [D]),
            "zsv_conv3d_bf16_dgrad_pack": (ctypes.c_int, [D, P, P, P]),
            "zsv_conv3d_bf16_dgrad": (ctypes.c_int, [D, P, P, P, P, P])}
    for name, (res, args) in want.items():
        proto = re.search(r"\b(size_t|int) %s\((.*?)\);" % name, header, re.S)
        assert proto, f"{name} is not declared in include/zsv_hip.h"
        assert _lib.SIGNATURES[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args
        params = [p.strip() for p in proto.group(2).split(",")]
        assert len(params) == len(args) and all("*" in p for p in params)
        assert (proto.group(1) == "size_t") == (res is ctypes.c_size_t)
    assert "resnet.py:40-52" in header and "resnet.py:266-273" in header      # the reference call sites, like every entry point


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_blob_bytes(case):
    lib = _lib.load()
    d = forward_desc(case)
    nb = int(lib.zsv_conv3d_bf16_dgrad_blob_bytes(byref(d)))
    assert nb > 0
    n, cin, t, h, w = case.xs
    # today's per-class descriptors (Bf16TrainPath._dgrad_composed): the blob is their packed weights one after the other + ONE row of shifts
    axes = [amp.Bf16TrainPath._axis_classes(k, p, s, n_in, n_out) for k, p, s, n_in, n_out in
            zip(case.kernel, case.padding, case.stride, (t, h, w), (d.To, d.Ho, d.Wo))]
    one = _lib.ConvDesc(n, case.cout, d.To, d.Ho, d.Wo, cin, d.To, d.Ho, d.Wo, 1, 1, 1, 1, 1, 1, 0, 0, 0)
    per_tap = int(lib.zsv_conv3d_bf16_blob_bytes(byref(one)))                 # Mp * (pitch(Cout) * 2 + 4)
    cp = int(lib.zsv_bf16_channel_pitch(case.cout))
    shifts = per_tap // (cp * 2 + 4) * 4
    assert shifts > 0 and (per_tap - shifts) % (cp * 2) == 0
    weights = 0
    for ct in axes[0]:
        for ch in axes[1]:
            for cw in axes[2]:
                taps = ct[2] * ch[2] * cw[2]
                if taps == 0:
                    continue
                if case.stride == (1, 1, 1):
                    dims = (t, h, w)
                else:
                    dims = tuple(n_out + 2 * c[3] - c[2] + 1 for c, n_out in zip((ct, ch, cw), (d.To, d.Ho, d.Wo)))
                d2 = _lib.ConvDesc(n, case.cout, d.To, d.Ho, d.Wo, cin, *dims, ct[2], ch[2], cw[2], 1, 1, 1, ct[3], ch[3], cw[3])
                b2 = int(lib.zsv_conv3d_bf16_blob_bytes(byref(d2)))
                assert b2 == taps * (per_tap - shifts) + shifts
                weights += b2 - shifts
                if case.stride == (1, 1, 1):
                    assert nb == b2, "stride 1: the blob of today's input-gradient descriptor"
    assert nb == weights + shifts


def test_unsupported_geometries_have_no_blob_and_are_refused():
    lib = _lib.load()
    p = 0x1000
    clip = _lib.ConvDesc(2, 3, 4, 26, 30, 45, 4, 10, 12, 1, 7, 7, 1, 2, 2, 0, 0, 0)              # the folded clip form (Cin = 3)
    assert int(lib.zsv_conv3d_bf16_blob_bytes(byref(clip))) > 0, "the forward takes this descriptor"
    twelve = forward_desc(X.GradCase("s322", (1, 64, 7, 8, 8), 64, (3, 3, 3), (3, 2, 2), (1, 1, 1)))      # 12 residue classes
    wide_pad = forward_desc(X.GradCase("pad", (1, 64, 4, 8, 8), 64, (1, 1, 1), (1, 1, 1), (0, 1, 1)))     # padding > kernel - 1
    for d in (clip, twelve, wide_pad):
        assert int(lib.zsv_conv3d_bf16_dgrad_blob_bytes(byref(d))) == 0
        assert lib.zsv_conv3d_bf16_dgrad_pack(byref(d), p, p, None) == E_UNSUPPORTED
        assert lib.zsv_conv3d_bf16_dgrad(byref(d), p, p, None, p, None) == E_UNSUPPORTED
    bad = forward_desc(X.DGRAD_CASES[2])
    bad.Wo += 1                                                                                     # inconsistent extents
    assert int(lib.zsv_conv3d_bf16_dgrad_blob_bytes(byref(bad))) == 0
    assert lib.zsv_conv3d_bf16_dgrad(byref(bad), p, p, None, p, None) == E_BAD_SHAPE
    assert int(lib.zsv_conv3d_bf16_dgrad_blob_bytes(None)) == 0


@pytest.mark.parametrize("case", [X.DGRAD_CASES[0], X.DGRAD_CASES[2], X.DGRAD_CASES[4]], ids=lambda c: c.name)
def test_null_arguments_are_refused_before_any_launch(case):
    """No device is needed (or touched): every refusal returns before the first HIP call.  The pointers are never dereferenced on the
    host; any non-NULL value stands for one."""
    lib = _lib.load()
    d = forward_desc(case)
    p = 0x1000
    assert lib.zsv_conv3d_bf16_dgrad_pack(None, p, p, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad_pack(byref(d), None, p, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad_pack(byref(d), p, None, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad(None, p, p, p, p, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad(byref(d), None, p, p, p, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad(byref(d), p, None, p, p, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad(byref(d), p, p, p, None, None) == E_NULL
    assert lib.zsv_conv3d_bf16_dgrad(byref(d), p, p, None, None, None) == E_NULL                     # (fanin alone may be NULL)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("p", [0, 1])
def test_axis_classes_partition_the_axis_and_name_the_taps(k, s, p):
    for n_in in range(3, 10):
        n_out = (n_in + 2 * p - k) // s + 1
        if n_out < 1 or p > k - 1:
            continue
        classes = amp.Bf16TrainPath._axis_classes(k, p, s, n_in, n_out)
        seen = []
        for rho, r, taps, pad, first, count in classes:
            assert 0 <= rho < s and count > 0
            c = first - pad + taps - 1                       # position j reads dz[j + c - m] for forward tap r + s*m
            for j in range(count):
                i = s * j + rho
                seen.append(i)
                got = {(j + c - m, r + s * m) for m in range(taps) if 0 <= j + c - m < n_out}
                want = {(o, kk) for o in range(n_out) for kk in range(k) if o * s - p + kk == i}
                assert got == want, (k, s, p, n_in, i)
        assert sorted(seen) == list(range(n_in)), "every input position exactly once"


@pytest.mark.parametrize("case", EXTRA_CASES, ids=[c.name for c in EXTRA_CASES])
def test_added_cases_meet_the_precondition(case):
    """The reference alone: operands on the grid, bf16 values, sum |terms| below 2^(24 - q) -- and with the fan-in of the GPU test
    (multiples of 1/2 within +-3, added to the ROUNDED gradient) the sum stays exact too."""
    w, dz = X.dgrad_operands(case)
    dx64, total, reached = X.dgrad_reference(case, w, dz)
    X.assert_exact_in_fp32(X.DGRAD_Q, total + 3.0, w, dz)
    X.assert_faces_nonzero(dz, case.name)
    assert bool(reached.any())
    if case.kernel == (1, 1, 1):
        assert not bool(reached.all()), "the shortcut has positions no tap reaches"
    share, up, down = X.rounding_profile(dx64)
    assert share > 0.01, "some outputs must need rounding"
