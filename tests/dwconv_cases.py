"""The depthwise-convolution cases and their fp64 references, shared by the depthwise GPU tests.

A case is (N,C,T,H,W), kernel, stride, padding: the smallest shapes at which the tiling, halo, frame-ring or residue-class logic
of csrc/conv_depthwise.hip can go wrong.  The reference is torch itself: ``F.conv3d(..., groups=C)`` and its autograd on the CPU
in fp64.  Two kinds of operands:

* ``exact``: integers in [-4, 4].  Every partial sum is an integer far below 2^24, so the result does not depend on the order of
  addition and the fp32 kernels must reproduce the fp64 reference bit for bit.
* ``normal``: standard normal operands.  A length-L fp32 dot product summed in ANY order, with or without fused multiply-adds,
  is within (L + 2) * 2^-24 * sum |a_i b_i| of the exact value for the L these cases have (gamma_L = L u / (1 - L u), u = 2^-24;
  the bias is one more term of the sum: gamma_(L+1) < (L + 2) u still holds, so the factor stays and |bias| joins the sum).  The
  right-hand side is the same fp64 reference on absolute values, so the bound is per element; where it is 0 (a voxel no output touches, a tap that only meets padding) the result must be exactly 0.
"""
import functools

import torch
import torch.nn.functional as F

CASES = [
    ((2, 5, 4, 9, 11), (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # 1  odd everything
    ((1, 3, 1, 7, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1)),       # 2  T = 1: only the centre frame tap is live
    ((2, 4, 2, 6, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # 3  T = 2: ring shorter than the kernel
    ((2, 6, 5, 9, 13), (3, 3, 3), (2, 2, 2), (1, 1, 1)),      # 4  odd extents at stride 2
    ((1, 8, 4, 8, 8), (3, 3, 3), (1, 2, 2), (1, 1, 1)),       # 5  spatial stride only
    ((2, 4, 6, 5, 67), (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # 6  a row wider than a wave
    ((1, 2, 3, 70, 6), (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # 7  more rows than a tile
    ((1, 3, 5, 6, 6), (3, 1, 1), (1, 1, 1), (1, 0, 0)),       # 8  temporal-only depthwise
    ((1, 3, 2, 9, 9), (1, 3, 3), (1, 2, 2), (0, 1, 1)),       # 9  spatial-only depthwise, strided
    ((1, 2, 3, 5, 5), (3, 3, 3), (1, 1, 1), (0, 0, 0)),       # 10 no padding
    ((1, 2, 3, 6, 6), (3, 3, 3), (2, 2, 2), (0, 0, 0)),       # 11 66 of the 216 dx elements are touched by no output
    ((3, 70, 2, 4, 4), (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # 12 more channels than lanes, tiny planes
    ((2, 64, 4, 14, 14), (3, 3, 3), (1, 1, 1), (1, 1, 1)),    # 13 layer-3-like, stride 1
    ((2, 64, 4, 14, 14), (3, 3, 3), (2, 2, 2), (1, 1, 1)),    # 14 layer-3-like, stride 2
    ((70, 2, 1, 4, 4), (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # 15 few channels, many clips: more than 64 weight-gradient slices (two-level slab sum)
]
IDS = [f"case{i + 1}" for i in range(len(CASES))]
U = 2.0 ** -24


def out_shape(case):
    (n, c, t, h, w), k, s, p = case
    return (n, c) + tuple((e + 2 * pp - kk) // ss + 1 for e, kk, ss, pp in zip((t, h, w), k, s, p))


@functools.lru_cache(maxsize=None)
def operands(index, kind, bias=False):
    """x, w, b (or None), dy of case ``index`` as fp32 CPU tensors; the same for every caller."""
    case = CASES[index]
    shape, k = case[0], case[1]
    g = torch.Generator().manual_seed(1000 + 10 * index + (kind == "exact"))
    wshape, oshape = (shape[1], 1) + k, out_shape(case)
    if kind == "exact":
        draw = lambda s: torch.randint(-4, 5, s, generator=g).float()
    else:
        draw = lambda s: torch.randn(s, generator=g)
    x, w, dy = draw(shape), draw(wshape), draw(oshape)
    b = draw((shape[1],)) if bias else None
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def reference(index, kind, bias=False, relu=False):
    """fp64 results and the per-element bounds: dict of y, dx, dw, db (None without bias), y_bound, dx_bound, dw_bound."""
    case = CASES[index]
    shape, k, s, p = case
    c = shape[1]
    x, w, b, dy = (None if t is None else t.double() for t in operands(index, kind, bias))
    x.requires_grad_(True)
    w.requires_grad_(True)
    if b is not None:
        b.requires_grad_(True)
    z = F.conv3d(x, w, b, s, p, 1, c)
    y = torch.relu(z) if relu else z
    y.backward(dy)
    g = dy * (z > 0) if relu else dy                       # the gradient that reaches the convolution
    taps = k[0] * k[1] * k[2]
    n_pos = g.numel() // c
    with torch.no_grad():
        y_abs = F.conv3d(x.abs(), w.abs(), None if b is None else b.abs(), s, p, 1, c)
        dx_abs = torch.nn.grad.conv3d_input(x.shape, w.abs(), g.abs(), s, p, 1, c)
        dw_abs = torch.nn.grad.conv3d_weight(x.abs(), w.shape, g.abs(), s, p, 1, c)
    return {"y": y.detach(), "z": z.detach(), "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad,
            "y_bound": (taps + 2) * U * y_abs, "dx_bound": (taps + 2) * U * dx_abs,
            "dw_bound": (n_pos + 2) * U * dw_abs}


def check(name, got, ref, bound, kind):
    """``exact``: bit for bit; ``normal``: |got - ref| <= bound per element (and exactly 0 where the bound is 0)."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    if kind == "exact":
        assert torch.equal(got, ref.float()), f"{name}: {int((got != ref.float()).sum())} of {got.numel()} elements differ from the exact result"
        return 0.0
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    bad = err > bound
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {got.numel()} elements beyond the bound, worst {worst:.3g} x bound"
    return worst
