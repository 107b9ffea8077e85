"""Tensors that are only element-aligned (include/zsv_hip.h, Conventions: fp32 tensors need 4 bytes, each on its own; channels-last
bf16 / e4m3 tensors need 16 and are refused otherwise), one operand at a time and through the Python surfaces.

tests/test_workspace_contract_gpu.py moves every fp32 operand of a call at once; it cannot tell x from dy.  Here every entry point
that tests `pointer & 15` on its launch path, and every kernel that makes 16-byte accesses on the strength of the shape alone, is
called on guarded buffers (tests/guarded.py) with EXACTLY ONE operand 4 bytes past a 256-byte boundary and the others on it, for
each operand in turn, on the smallest row of the existing tables that reaches the kernel.  Asserted per call: status 0, bands
intact, inputs unchanged, every output element written, the result within the table's own tolerance of its own fp64 reference,
and -- wherever the header promises that alignment selects only the width of the loads and stores -- the bits of the all-aligned
call.  The weight gradients whose kernel family follows x | dy (header: "the result is that kernel's") are held to the reference
alone.

The channels-last entry points get one operand at +2 and +8 and must answer ZSV_E_UNSUPPORTED with every output still at its
prefill.  The last part goes through ops / torch.ops.zsv on ``flat[1:1 + n].view(shape)`` operands and trains an R(2+1)D-18
whose parameters all live in one flat buffer, one float apart.
"""
import ctypes
from ctypes import byref

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_exact_cases as X
import guarded as G
import test_fp8_gpu as F8
import test_ops_gpu as T
import test_workspace_contract_gpu as WC
from helpers import make_opt, rel_err

pytestmark = pytest.mark.gpu

from zeroshotvideoclassification_amd import _lib, inference, network, ops, optim, synthetic, torch_ops, train  # noqa: E402

DEV = "cuda"
F32, I32, BF16, U8 = torch.float32, torch.int32, torch.bfloat16, torch.uint8
ZSV_E_UNSUPPORTED = 6


def lib():
    return _lib.load()


def raw(t):
    return t.contiguous().view(-1).view(U8)


def call(launch, ins, outs, works=None, off=(), shift=4):
    """One call on guarded buffers: the operands named in ``off`` start ``shift`` bytes past a 256-byte boundary, every other one
    on it; outputs and workspaces are prefilled with 0xFF.  Bands and inputs are checked.  Returns (status, name -> output view)."""
    bufs, views, src = {}, {}, {}
    for name, t in ins.items():
        if t is not None:
            bufs[name] = src[name] = G.guarded_copy(t, DEV, shift=shift if name in off else 0)
    for name, spec in outs.items():                   # (dtype, shape) or, for an in / out argument, (dtype, shape, initial tensor)
        dtype, shape = spec[:2]
        bufs[name] = G.guarded_like(dtype, shape, DEV, 0xFF, shift=shift if name in off else 0)
        views[name] = bufs[name].view(dtype, shape)
        if len(spec) > 2:
            views[name].copy_(spec[2])
    for name, nbytes in (works or {}).items():
        bufs[name] = G.guarded(nbytes, DEV, 0xFF, shift=shift if name in off else 0)
    assert set(off) <= set(bufs), f"no operand named {sorted(set(off) - set(bufs))}"
    for name in off:
        assert bufs[name].ptr % 256 == shift
    p = {name: b.ptr for name, b in bufs.items()}
    p.update({name: None for name, t in ins.items() if t is None})
    status = launch(p)
    torch.cuda.synchronize()
    where = f"operands at +{shift}: {sorted(off)}"
    for name, b in bufs.items():
        b.check(f"{name} ({where})")
    for name, b in src.items():
        assert torch.equal(b.payload, raw(ins[name].detach().to(DEV))), f"the input {name} was written ({where})"
    return status, views


def each_operand(what, launch, ins, outs, works, operands, check, same_bits=True):
    """The all-aligned call, then one call per name in ``operands`` with that operand alone at +4.  ``check(outputs, tag)`` compares
    with the fp64 reference; ``same_bits``: True, or the operands whose misalignment must leave the all-aligned call's bits."""
    base = None
    for off in [()] + [(name,) for name in operands]:
        tag = f"{what}, {off[0] + ' at +4' if off else 'all operands aligned'}"
        status, views = call(launch, ins, outs, works, off)
        assert status == 0, f"{tag}: {lib().zsv_status_string(int(status)).decode()} (status {status})"
        for name, v in views.items():
            G.assert_all_written(v, f"{tag}: {name}")
        check(views, tag)
        got = {name: v.clone() for name, v in views.items()}
        if base is None:
            base = got
        elif same_bits is True or off[0] in same_bits:
            for name, v in got.items():
                assert torch.equal(raw(v), raw(base[name])), f"{tag}: {name} differs from the all-aligned call's bits"
    return base


def conv_operands(seed, xs, ws, stride, pad):
    g = torch.Generator().manual_seed(seed)
    d = ops.conv_desc(xs, ws, ops._triple(stride), pad)
    ys = (d.N, d.Cout, d.To, d.Ho, d.Wo)
    o = dict(x=torch.randn(xs, generator=g), w=torch.randn(ws, generator=g) / np.sqrt(np.prod(ws[1:])), bias=torch.randn(ws[0], generator=g),
             res=torch.randn(ys, generator=g), dy=torch.randn(ys, generator=g), add=torch.randn(xs, generator=g))
    return d, ys, o


# =========================================================================================================================
# the weight gradients: conv_wgrad.hip:564 (wgrad_dispatch's one aligned16(x, dy) in front of the route table: frame ring, Winograd
# form, LDS-DMA), conv_wgrad_generic.hip:397 (stem rows), conv_wgrad.hip:427 (av4 on dy)
# =========================================================================================================================
WGRAD_SITES = [
    # site, the row, (N, Cin, T, H, W), (Cout, Cin, k), stride, padding, tolerance of the row's own test, switches that pin the route,
    # the switch that takes the kernel away (None: the register-staged kernel itself)
    ("temporal ring", "WGRAD_TRING_CASES/t1_like", (2, 144, 8, 32, 32), (64, 144, 3, 1, 1), 1, (1, 0, 0), 2e-5, (), "ZSV_NO_WGRAD_TRING"),
    ("Winograd form", "WGRAD_WINO_CASES/partial_chunk_aligned_w", (24, 16, 3, 20, 12), (128, 16, 1, 3, 3), 1, (0, 1, 1), 2e-5, (), "ZSV_NO_WGRAD_WINO"),
    ("LDS-DMA", "WGRAD_DMA_CASES/s1_like", (2, 64, 2, 12, 12), (144, 64, 1, 3, 3), 1, (0, 1, 1), 2e-5, ("ZSV_NO_WGRAD_WINO",), "ZSV_NO_WGRAD_DMA"),
    ("stem rows", "test_stem_weight_gradient_row_kernel/fewer_output_channels", (2, 3, 3, 24, 40), (20, 3, 1, 7, 7), (1, 2, 2), (0, 3, 3), 5e-5, (),
     "ZSV_NO_STEM_WGRAD"),
    ("register-staged, 16-byte dY loads", "CONV_CASES/pointwise_s2", (2, 24, 4, 8, 8), (40, 24, 1, 1, 1), (2, 2, 2), (0, 0, 0), 2e-5, (), None),
]


@pytest.mark.parametrize("site", WGRAD_SITES, ids=[s[0].replace(" ", "_").replace(",", "") for s in WGRAD_SITES])
def test_weight_gradient_dispatch_sites_one_operand_at_a_time(site, monkeypatch):
    """x, dy and dw in turn at +4.  x or dy off the boundary sends the call to another kernel family (the header names these entry
    points): its result is held to the fp64 reference; dw off the boundary changes nothing."""
    name, row, xs, ws, stride, pad, rtol, pins, off_switch = site
    for k in pins:
        monkeypatch.setenv(k, "1")
    L = lib()
    d, ys, o = conv_operands(len(row), xs, ws, stride, pad)
    nw = int(L.zsv_conv3d_wgrad_workspace_bytes(byref(d)))
    ref = torch.nn.grad.conv3d_weight(o["x"].double(), ws, o["dy"].double(), stride=ops._triple(stride), padding=pad)

    def launch(p):
        return L.zsv_conv3d_wgrad(byref(d), p["x"], p["dy"], p["dw"], p["ws"], nw, None)

    base = each_operand(f"zsv_conv3d_wgrad, {row}", launch, dict(x=o["x"], dy=o["dy"]), {"dw": (F32, ws)}, {"ws": nw}, ["x", "dy", "dw"],
                        lambda v, tag: T.close(v["dw"], ref, rtol=rtol, what=tag), same_bits={"dw"})
    if off_switch:                      # the row reaches the kernel the site belongs to: without it the bits are other bits
        monkeypatch.setenv(off_switch, "1")
        assert int(L.zsv_conv3d_wgrad_workspace_bytes(byref(d))) <= nw
        status, views = call(launch, dict(x=o["x"], dy=o["dy"]), {"dw": (F32, ws)}, {"ws": nw})
        assert status == 0
        T.close(views["dw"], ref, rtol=rtol, what=f"{row} without the {name} kernel")
        assert not torch.equal(views["dw"], base["dw"]), f"{row} does not reach the {name} kernel"


# =========================================================================================================================
# forward and input gradient: conv_api.hip:203 (avec on w), conv_tap.hip:560 (LDS epilogue on y), conv_tap.hip:453 (split-K
# reduce), conv_dgrad_s2.hip:364 (x4 on dy) and the pair stores on dx; the linear entry points
# =========================================================================================================================
FWD_SITES = [
    # site, row, xs, ws, stride, padding
    ("generic kernel, 3-channel 7x7 stem", "CONV_CASES/stem_7x7", (2, 3, 2, 30, 30), (45, 3, 1, 7, 7), (1, 2, 2), (0, 3, 3)),
    ("generic kernel, K % 4 == 0: 16-byte weight loads", "CONV_CASES/spatial_s1", (2, 8, 3, 10, 12), (20, 8, 1, 3, 3), 1, (0, 1, 1)),
    ("tap kernel, LDS epilogue", "CONV_CASES/spatial_144", (1, 64, 2, 12, 12), (144, 64, 1, 3, 3), 1, (0, 1, 1)),
    ("tap kernel, K parts + ordered reduce", "test_conv3d_split_k_small_grid/256_320", (2, 256, 2, 7, 7), (320, 256, 1, 3, 3), 1, (0, 1, 1)),
    ("stride-2 input gradient in one launch", "S2_DGRAD_CASES/ragged_16_byte_pieces", (3, 70, 2, 12, 16), (37, 70, 1, 3, 3), (1, 2, 2), (0, 1, 1)),
]


@pytest.mark.parametrize("site", FWD_SITES, ids=[s[1].split("/")[1] for s in FWD_SITES])
def test_forward_and_input_gradient_sites_one_operand_at_a_time(site):
    """Forward (+ bias + ReLU) with x, w, bias, y and the input gradient with dy, w, dx in turn at +4: the fp64 reference of the
    row's own test, and the all-aligned call's bits (alignment selects a load / store width here, never another sum)."""
    name, row, xs, ws, stride, pad = site
    L = lib()
    d, ys, o = conv_operands(len(row), xs, ws, stride, pad)
    nf, nd = int(L.zsv_conv3d_fwd_workspace_bytes(byref(d))), int(L.zsv_conv3d_dgrad_workspace_bytes(byref(d)))
    st = ops._triple(stride)
    yref = F.relu(F.conv3d(o["x"].double(), o["w"].double(), o["bias"].double(), st, pad))
    dxref = torch.nn.grad.conv3d_input(xs, o["w"].double(), o["dy"].double(), stride=st, padding=pad)
    each_operand(f"zsv_conv3d_fwd, {row}", lambda p: L.zsv_conv3d_fwd(byref(d), p["x"], p["w"], p["bias"], p["y"], 1, p["ws"], nf, None),
                 dict(x=o["x"], w=o["w"], bias=o["bias"]), {"y": (F32, ys)}, {"ws": nf}, ["x", "w", "bias", "y"],
                 lambda v, tag: T.close(v["y"], yref, what=tag))
    each_operand(f"zsv_conv3d_dgrad, {row}", lambda p: L.zsv_conv3d_dgrad(byref(d), p["dy"], p["w"], p["dx"], p["ws"], nd, None),
                 dict(dy=o["dy"], w=o["w"]), {"dx": (F32, xs)}, {"ws": nd}, ["dy", "w", "dx"],
                 lambda v, tag: T.close(v["dx"], dxref, what=tag))
    for sub_st in (1, 2):               # the strided shortcut's gradient added by the same launch (the stride-2 row only)
        if L.zsv_conv3d_dgrad_add_strided_supported(byref(d), sub_st, 2, 2):
            sub = torch.randn((d.N, d.Cin, -(-d.Ti // sub_st), d.Hi // 2, d.Wi // 2), generator=torch.Generator().manual_seed(sub_st))
            ref = dxref.clone()
            ref[:, :, ::sub_st, :2 * (d.Hi // 2):2, :2 * (d.Wi // 2):2] += sub.double()
            each_operand(f"zsv_conv3d_dgrad_add_strided (st = {sub_st}), {row}",
                         lambda p: L.zsv_conv3d_dgrad_add_strided(byref(d), p["dy"], p["w"], p["sub"], sub_st, 2, 2, p["dx"], p["ws"], nd, None),
                         dict(dy=o["dy"], w=o["w"], sub=sub), {"dx": (F32, xs)}, {"ws": nd}, ["dy", "sub", "dx"],
                         lambda v, tag: T.close(v["dx"], ref, what=tag))
        else:
            assert "S2_DGRAD" not in row


def test_weight_gradient_through_a_folded_batchnorm_one_operand_at_a_time():
    """zsv_conv3d_wgrad_pre (x read through relu(x * scale[c] + shift[c])) has one kernel, the frame ring's PRE form: x, dy and dw in
    turn at +4 give the all-aligned call's bits; pre_coef keeps the 16 bytes the header asks for.  The first row and the tolerance
    of test_batchnorm_relu_folded_into_the_temporal_convolution."""
    L = lib()
    xs, ws, pad = (2, 144, 8, 32, 32), (64, 144, 3, 1, 1), (1, 0, 0)
    d, ys, o = conv_operands(5, xs, ws, 1, pad)
    assert L.zsv_conv3d_pre_supported(byref(d))
    g = torch.Generator().manual_seed(6)
    cin, pitch = xs[1], (xs[1] + 15) // 16 * 16
    coef = torch.zeros(2, pitch)
    coef[0, :cin], coef[1, :cin] = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    nw = int(L.zsv_conv3d_wgrad_workspace_bytes(byref(d)))
    act = F.relu(o["x"].double() * coef[0, :cin].double().view(1, cin, 1, 1, 1) + coef[1, :cin].double().view(1, cin, 1, 1, 1))
    ref = torch.nn.grad.conv3d_weight(act, ws, o["dy"].double(), padding=pad)
    each_operand("zsv_conv3d_wgrad_pre", lambda p: L.zsv_conv3d_wgrad_pre(byref(d), p["x"], p["coef"], pitch, p["dy"], p["dw"], p["ws"], nw, None),
                 dict(x=o["x"], coef=coef, dy=o["dy"]), {"dw": (F32, ws)}, {"ws": nw}, ["x", "dy", "dw"],
                 lambda v, tag: T.close(v["dw"], ref, rtol=5e-5, what=tag))


def test_statistics_epilogue_follows_the_alignment_of_y():
    """zsv_conv3d_fwd_stat_tiles(d, y) answers for the y it is given (conv_tap.hip:560): tiles for an aligned y, 0 for the same
    geometry at +4, where the caller runs the plain form (ops.conv3d does).  Tiles asked for an aligned y and passed with another
    one are refused before any launch."""
    L = lib()
    row, xs, ws, pad = "test_conv_epilogue_statistics_feed_batchnorm", (3, 32, 4, 12, 12), (48, 32, 1, 3, 3), (0, 1, 1)
    d, ys, o = conv_operands(len(row), xs, ws, 1, pad)
    nf = int(L.zsv_conv3d_fwd_workspace_bytes(byref(d)))
    yref = F.conv3d(o["x"].double(), o["w"].double(), None, 1, pad)
    seen = {}

    def launch(p):
        seen["tiles"] = tiles = int(L.zsv_conv3d_fwd_stat_tiles(byref(d), p["y"]))
        return L.zsv_conv3d_fwd_stats(byref(d), p["x"], p["w"], None, p["y"], 0, p["bn_partials"] if tiles else None, tiles, p["ws"], nf, None)

    aligned_tiles = int(L.zsv_conv3d_fwd_stat_tiles(byref(d), G.guarded_like(F32, ys, DEV, 0).ptr))
    assert aligned_tiles > 0, "the row must reach the statistics epilogue"
    outs = {"y": (F32, ys), "bn_partials": (F32, (2, d.Cout, aligned_tiles))}
    status, v = call(launch, dict(x=o["x"], w=o["w"]), outs, {"ws": nf})
    assert status == 0 and seen["tiles"] == aligned_tiles
    T.close(v["y"], yref, what="forward with statistics")
    T.close(v["bn_partials"][0].double().sum(1), yref.sum(dim=(0, 2, 3, 4)), rtol=1e-4, what="sum y")
    T.close(v["bn_partials"][1].double().sum(1), (yref * yref).sum(dim=(0, 2, 3, 4)), rtol=1e-4, what="sum y^2")
    y_aligned = v["y"].clone()
    for off in (("x",), ("w",), ("bn_partials",)):                    # these do not decide the route: same tiles, same bits
        status, v2 = call(launch, dict(x=o["x"], w=o["w"]), outs, {"ws": nf}, off)
        assert status == 0 and seen["tiles"] == aligned_tiles, off
        assert torch.equal(v2["y"], y_aligned) and torch.equal(v2["bn_partials"], v["bn_partials"]), off
    status, v3 = call(launch, dict(x=o["x"], w=o["w"]), outs, {"ws": nf}, ("y",))
    assert status == 0 and seen["tiles"] == 0, "y at +4 cannot take the transposing epilogue: the query must say so"
    assert torch.equal(v3["y"], y_aligned), "the plain form stores the same sums"
    assert G.unwritten(v3["bn_partials"]) == v3["bn_partials"].numel(), "no statistics were promised: none may be written"
    # stale tiles: asked for an aligned y, used with y at +4
    status, v4 = call(lambda p: L.zsv_conv3d_fwd_stats(byref(d), p["x"], p["w"], None, p["y"], 0, p["bn_partials"], aligned_tiles, p["ws"], nf, None),
                      dict(x=o["x"], w=o["w"]), outs, {"ws": nf}, ("y",))
    assert status == ZSV_E_UNSUPPORTED
    assert G.unwritten(v4["y"]) == v4["y"].numel() and G.unwritten(v4["bn_partials"]) == v4["bn_partials"].numel()


def test_linear_entry_points_one_operand_at_a_time():
    """(3, 37, 11) of test_linear: odd sizes, every operand in turn."""
    L = lib()
    rows, fin, fout = 3, 37, 11
    g = torch.Generator().manual_seed(rows + fin)
    x, w, b, dy = (torch.randn(rows, fin, generator=g), torch.randn(fout, fin, generator=g) / np.sqrt(fin), torch.randn(fout, generator=g),
                   torch.randn(rows, fout, generator=g))
    nf, nd, nw = (int(f(rows, fin, fout)) for f in (L.zsv_linear_fwd_workspace_bytes, L.zsv_linear_dgrad_workspace_bytes, L.zsv_linear_wgrad_workspace_bytes))
    each_operand("zsv_linear_fwd", lambda p: L.zsv_linear_fwd(p["x"], p["w"], p["bias"], p["y"], rows, fin, fout, 0, p["ws"], nf, None),
                 dict(x=x, w=w, bias=b), {"y": (F32, (rows, fout))}, {"ws": nf}, ["x", "w", "bias", "y"],
                 lambda v, tag: T.close(v["y"], F.linear(x.double(), w.double(), b.double()), what=tag))
    each_operand("zsv_linear_dgrad", lambda p: L.zsv_linear_dgrad(p["dy"], p["w"], p["dx"], rows, fin, fout, p["ws"], nd, None),
                 dict(dy=dy, w=w), {"dx": (F32, (rows, fin))}, {"ws": nd}, ["dy", "w", "dx"],
                 lambda v, tag: T.close(v["dx"], dy.double() @ w.double(), what=tag))
    each_operand("zsv_linear_wgrad", lambda p: L.zsv_linear_wgrad(p["x"], p["dy"], p["dw"], rows, fin, fout, p["ws"], nw, None),
                 dict(x=x, dy=dy), {"dw": (F32, (fout, fin))}, {"ws": nw}, ["x", "dy", "dw"],
                 lambda v, tag: T.close(v["dw"], dy.double().t() @ x.double(), what=tag))


# =========================================================================================================================
# kernels that make 16-byte accesses on the strength of the shape alone: the Winograd family (conv_wino.hip:1639 and the F(4,3) /
# temporal kernels' image DMAs, buffer_store_b128 epilogues, f32x4 loads of `add`), BatchNorm (batchnorm.hip: S % 4 == 0), the
# max-pool backward (elementwise_pool.hip: Wi % 4 == 0)
# =========================================================================================================================
WINO_ROWS = [
    # name, xs, Cout, kT, switches (small shapes: below the production thresholds, as the VW_CASES rows are)
    ("F(2,3) with 16-byte image pieces", (2, 16, 3, 10, 12), 20, 1, (("ZSV_WINO_MIN_TILES", "1"), ("ZSV_WINO_NO_F43", "1"))),
    ("F(4,3)", (2, 16, 3, 10, 12), 20, 1, (("ZSV_WINO_MIN_TILES", "1"),)),
    ("F(4,3) on a virtual row width (VW_CASES/w15_small)", (3, 32, 3, 9, 15), 40, 1, (("ZSV_WINO_VW_MIN_WGS", "1"),)),
    ("temporal F(4,3)", (2, 16, 4, 8, 8), 32, 3, (("ZSV_WINOT_MIN_TILES", "1"),)),
]


@pytest.mark.parametrize("case", WINO_ROWS, ids=["f23_x4", "f43", "f43_virtual_width", "temporal"])
def test_winograd_kernels_one_operand_at_a_time(case, monkeypatch):
    """Forward with bias + residual + ReLU and the input gradient with the shortcut gradient added, every operand in turn at +4,
    against torch CPU fp64 (the tolerance of the rows' own tests) and the all-aligned call's bits."""
    name, xs, cout, kt, knobs = case
    for k, v in knobs:
        monkeypatch.setenv(k, v)
    L = lib()
    ws = (cout, xs[1], 3, 1, 1) if name.startswith("temporal") else (cout, xs[1], kt, 3, 3)
    pad = (1, 0, 0) if name.startswith("temporal") else (kt // 2, 1, 1)
    d, ys, o = conv_operands(len(name), xs, ws, 1, pad)
    nf, nd = int(L.zsv_conv3d_fwd_workspace_bytes(byref(d))), int(L.zsv_conv3d_dgrad_workspace_bytes(byref(d)))
    assert L.zsv_conv3d_fwd_add_supported(byref(d)) and L.zsv_conv3d_dgrad_add_supported(byref(d))
    yref = F.relu(F.conv3d(o["x"].double(), o["w"].double(), o["bias"].double(), 1, pad) + o["res"].double())
    dxref = torch.nn.grad.conv3d_input(xs, o["w"].double(), o["dy"].double(), padding=pad) + o["add"].double()

    def fwd(p):
        return L.zsv_conv3d_fwd_full(byref(d), p["x"], p["w"], p["bias"], p["res"], p["y"], 1, None, 0, p["ws"], nf, None)

    def dgrad(p):
        return L.zsv_conv3d_dgrad_add(byref(d), p["dy"], p["w"], p["add"], p["dx"], p["ws"], nd, None)

    y = each_operand(f"zsv_conv3d_fwd_full, {name}", fwd, dict(x=o["x"], w=o["w"], bias=o["bias"], res=o["res"]), {"y": (F32, ys)}, {"ws": nf},
                     ["x", "w", "bias", "res", "y"], lambda v, tag: T.close(v["y"], yref, what=tag))["y"]
    dx = each_operand(f"zsv_conv3d_dgrad_add, {name}", dgrad, dict(dy=o["dy"], w=o["w"], add=o["add"]), {"dx": (F32, xs)}, {"ws": nd},
                      ["dy", "w", "add", "dx"], lambda v, tag: T.close(v["dx"], dxref, what=tag))["dx"]
    # the row reaches the Winograd kernels: the direct kernel gives other bits (its workspace may be larger: queried again)
    monkeypatch.setenv("ZSV_NO_WINO", "1")
    nf, nd = int(L.zsv_conv3d_fwd_workspace_bytes(byref(d))), int(L.zsv_conv3d_dgrad_workspace_bytes(byref(d)))
    _, v = call(fwd, dict(x=o["x"], w=o["w"], bias=o["bias"], res=o["res"]), {"y": (F32, ys)}, {"ws": nf})
    _, v2 = call(dgrad, dict(dy=o["dy"], w=o["w"], add=o["add"]), {"dx": (F32, xs)}, {"ws": nd})
    assert not torch.equal(v["y"], y) and not torch.equal(v2["dx"], dx), f"{name}: the row does not reach the Winograd kernels"


# (2, 64, (4, 8, 8)): S % 4 == 0, the float4 routes; (2, 5, (3, 4, 4)): odd channel count; (1, 3, (4, 32, 32)): S = 4096, one full
# ROW_CHUNK per row -- the route whose 16-byte loads are all issued up front (batchnorm.hip bn_apply_kernel / bn_bwd_apply_kernel)
BN_SHAPES = [(2, 64, 4, 8, 8), (2, 5, 3, 4, 4), (1, 3, 4, 32, 32)]


@pytest.mark.parametrize("shape", BN_SHAPES, ids=["x".join(map(str, s)) for s in BN_SHAPES])
def test_batchnorm_one_operand_at_a_time(shape):
    """Forward (training and frozen statistics) with residual + ReLU and both backwards with the residual gradient: x, residual,
    y / dy, x, y, dx, d_residual in turn at +4, against F.batch_norm in fp64 with the tolerance of test_batchnorm_train_fwd_bwd."""
    L = lib()
    o = {k: v.cpu() for k, v in WC._bn_operands(shape).items()}
    n, c = shape[:2]
    s = int(np.prod(shape[2:]))
    nb = int(L.zsv_bn_workspace_bytes(n, c, s))

    def reference(training):
        t = {k: o[k].double().requires_grad_() for k in ("x", "gamma", "beta", "res")}
        rm, rv = o["rm"].double().clone(), o["rv"].double().clone()
        y = F.relu(F.batch_norm(t["x"], rm, rv, t["gamma"], t["beta"], training=training, momentum=0.1, eps=1e-5) + t["res"])
        y.backward(o["dy"].double())
        return dict(y=y.detach(), running_mean=rm, running_var=rv, dx=t["x"].grad, dgamma=t["gamma"].grad, dbeta=t["beta"].grad, d_residual=t["res"].grad)

    def check(ref, names):
        def inner(v, tag):
            for k in names:
                T.close(v[k], ref[k], rtol=1e-4, what=f"{tag}: {k}")
        return inner

    vec = {"save_mean": (F32, (c,)), "save_invstd": (F32, (c,)), "running_mean": (F32, (c,), o["rm"]), "running_var": (F32, (c,), o["rv"])}
    ref = reference(True)
    fwd = each_operand("zsv_bn_fwd_train",
                       lambda p: L.zsv_bn_fwd_train(p["x"], n, c, s, p["gamma"], p["beta"], p["res"], 1, p["y"], p["save_mean"], p["save_invstd"],
                                                    p["running_mean"], p["running_var"], 0.1, 1e-5, p["ws"], nb, None),
                       dict(x=o["x"], gamma=o["gamma"], beta=o["beta"], res=o["res"]), dict(vec, y=(F32, shape)), {"ws": nb},
                       ["x", "res", "y", "gamma", "save_mean", "running_var"], check(ref, ["y", "running_mean", "running_var"]))
    grads = {"dx": (F32, shape), "d_residual": (F32, shape), "dgamma": (F32, (c,)), "dbeta": (F32, (c,))}
    each_operand("zsv_bn_bwd",
                 lambda p: L.zsv_bn_bwd(p["dy"], p["x"], p["y"], n, c, s, p["gamma"], p["beta"], p["save_mean"], p["save_invstd"], 1, p["dx"],
                                        p["d_residual"], p["dgamma"], p["dbeta"], p["ws"], nb, None),
                 dict(dy=o["dy"], x=o["x"], y=fwd["y"], gamma=o["gamma"], beta=o["beta"], save_mean=fwd["save_mean"], save_invstd=fwd["save_invstd"]),
                 grads, {"ws": nb}, ["dy", "x", "y", "dx", "d_residual", "dgamma"], check(ref, ["dx", "dgamma", "dbeta", "d_residual"]))
    ref = reference(False)
    ye = each_operand("zsv_bn_fwd_eval",
                      lambda p: L.zsv_bn_fwd_eval(p["x"], n, c, s, p["gamma"], p["beta"], p["rm"], p["rv"], p["res"], 1, 1e-5, p["y"], p["ws"], nb, None),
                      dict(x=o["x"], gamma=o["gamma"], beta=o["beta"], rm=o["rm"], rv=o["rv"], res=o["res"]), {"y": (F32, shape)}, {"ws": nb},
                      ["x", "res", "y", "rv"], check(ref, ["y"]))["y"]
    each_operand("zsv_bn_bwd_eval",
                 lambda p: L.zsv_bn_bwd_eval(p["dy"], p["x"], p["y"], n, c, s, p["gamma"], p["beta"], p["rm"], p["rv"], 1e-5, 1, p["dx"], p["d_residual"],
                                             p["dgamma"], p["dbeta"], p["ws"], nb, None),
                 dict(dy=o["dy"], x=o["x"], y=ye, gamma=o["gamma"], beta=o["beta"], rm=o["rm"], rv=o["rv"]), grads, {"ws": nb},
                 ["dy", "x", "y", "dx", "d_residual", "dbeta"], check(ref, ["dx", "dgamma", "dbeta", "d_residual"]))


def test_max_pool_one_operand_at_a_time():
    """POOL_CASES[0] ((1, 2, 2) windows on 8 x 8 frames: the float4 store of the backward): exact against F.max_pool3d."""
    L = lib()
    k, p_, shape = T.POOL_CASES[0]
    assert shape[-1] % 4 == 0
    g = torch.Generator().manual_seed(sum(shape))
    x = F.relu(torch.randn(*shape, generator=g))
    geom, (to, ho, wo) = WC._pool_geometry(shape, k, p_)
    ys = shape[:2] + (to, ho, wo)
    dy = torch.randn(ys, generator=g)
    xr = x.double().requires_grad_()
    yr = F.max_pool3d(xr, k, k, p_)
    yr.backward(dy.double())
    out = each_operand("zsv_maxpool3d_fwd", lambda q: L.zsv_maxpool3d_fwd(q["x"], *geom, q["y"], q["argmax"], None), dict(x=x),
                       {"y": (F32, ys), "argmax": (I32, ys)}, None, ["x", "y", "argmax"],
                       lambda v, tag: T.close(v["y"], yr.detach(), rtol=0.0, what=tag))
    each_operand("zsv_maxpool3d_bwd", lambda q: L.zsv_maxpool3d_bwd(q["dy"], q["argmax"], *geom, q["dx"], None), dict(dy=dy, argmax=out["argmax"]),
                 {"dx": (F32, shape)}, None, ["dy", "argmax", "dx"], lambda v, tag: T.close(v["dx"], xr.grad, rtol=0.0, what=tag))


# =========================================================================================================================
# channels-last bf16 / e4m3 tensors off a 16-byte boundary are refused before any launch
# =========================================================================================================================
def _pitch(c):
    return inference.channel_pitch(c)


def _rejections():
    """name -> (launch, operand name -> (dtype, shape, role), work name -> bytes, the channels-last operands): one row of each entry
    point's contract test.  Roles: "in", "out"."""
    L = lib()
    rows = {}
    # ---- bf16 forward (+ residual), statistics epilogue, input gradient, weight gradient ----
    c = X.FORWARD_CASES[1]
    d = ops.conv_desc((c.n, c.cin) + c.thw, (c.cout, c.cin) + c.kernel, c.stride, c.padding)
    xs, ys = (c.n,) + c.thw + (_pitch(c.cin),), (d.N, d.To, d.Ho, d.Wo, _pitch(c.cout))
    nb = int(L.zsv_conv3d_bf16_blob_bytes(byref(d)))
    rows["zsv_conv3d_bf16_fwd"] = (lambda p, d=d: L.zsv_conv3d_bf16_fwd(byref(d), p["x"], p["blob"], p["residual"], 1, p["y"], None),
                                   dict(x=(BF16, xs, "in"), residual=(BF16, ys, "in"), y=(BF16, ys, "out")), {"blob": nb}, ["x", "residual", "y"])
    c = X.STATS_CASES[3]
    d = ops.conv_desc((c.n, c.cin) + c.thw, (c.cout, c.cin) + c.kernel, c.stride, c.padding)
    xs, ys = (c.n,) + c.thw + (_pitch(c.cin),), (d.N, d.To, d.Ho, d.Wo, _pitch(c.cout))
    nb, cap = int(L.zsv_conv3d_bf16_blob_bytes(byref(d))), int(L.zsv_conv3d_bf16_stat_rows(byref(d)))
    got_rows = ctypes.c_int32(0)
    rows["zsv_conv3d_bf16_fwd_stats"] = (lambda p, d=d, cap=cap: L.zsv_conv3d_bf16_fwd_stats(byref(d), p["x"], p["blob"], p["y"], p["bn_partials"], cap,
                                                                                           byref(got_rows), None),
                                         dict(x=(BF16, xs, "in"), y=(BF16, ys, "out"), bn_partials=(F32, (cap, 2, ys[-1]), "out")), {"blob": nb}, ["x", "y"])
    for c in (X.DGRAD_CASES[1], X.DGRAD_CASES[2]):                  # stride 1 (the forward's kernels) and the strided launch
        n, cin, t, h, w = c.xs
        d = ops.conv_desc(c.xs, (c.cout, cin) + c.kernel, c.stride, c.padding)
        xs, zs = (n, t, h, w, _pitch(cin)), (d.N, d.To, d.Ho, d.Wo, _pitch(c.cout))
        nb = int(L.zsv_conv3d_bf16_dgrad_blob_bytes(byref(d)))
        assert nb > 0
        rows[f"zsv_conv3d_bf16_dgrad, stride {c.stride}"] = (lambda p, d=d: L.zsv_conv3d_bf16_dgrad(byref(d), p["dz"], p["blob"], p["fanin"], p["dx"], None),
                                                            dict(dz=(BF16, zs, "in"), fanin=(BF16, xs, "in"), dx=(BF16, xs, "out")), {"blob": nb},
                                                            ["dz", "fanin", "dx"])
    c = X.WGRAD_CASES[4]
    n, cin, t, h, w = c.xs
    d = ops.conv_desc(c.xs, (c.cout, cin) + c.kernel, c.stride, c.padding)
    nw = int(L.zsv_conv3d_bf16_wgrad_workspace_bytes(byref(d)))
    assert nw > 0
    rows["zsv_conv3d_bf16_wgrad"] = (lambda p, d=d, nw=nw: L.zsv_conv3d_bf16_wgrad(byref(d), p["x"], p["dz"], p["dw"], p["ws"], nw, None),
                                     dict(x=(BF16, (n, t, h, w, _pitch(cin)), "in"), dz=(BF16, (d.N, d.To, d.Ho, d.Wo, _pitch(c.cout)), "in"),
                                          dw=(F32, (c.cout, cin) + tuple(c.kernel), "out")), {"ws": nw}, ["x", "dz"])
    # ---- e4m3 forward ----
    n, cin, cout, thw, k, s, pd, _res, _relu = F8.CASES[1]
    d = ops.conv_desc((n, cin) + thw, (cout, cin) + k, s, pd)
    xs, ys = (n,) + thw + (inference.fp8_channel_pitch(cin),), (d.N, d.To, d.Ho, d.Wo, inference.fp8_channel_pitch(cout))
    nb = int(L.zsv_conv3d_fp8_blob_bytes(byref(d)))
    rows["zsv_conv3d_fp8_fwd"] = (lambda p, d=d: L.zsv_conv3d_fp8_fwd(byref(d), p["x"], p["blob"], p["residual"], 1, p["y"], None),
                                  dict(x=(U8, xs, "in"), residual=(U8, ys, "in"), y=(U8, ys, "out")), {"blob": nb}, ["x", "residual", "y"])
    # ---- the folded clip ----
    (n, ch, t, h, w), pads, padded = WC.CLIP_CASES[0]
    rows["zsv_clip_to_bf16"] = (lambda p: L.zsv_clip_to_bf16(p["x"], n, ch, t, h, w, pads[0], pads[1], padded[0], padded[1], p["out"], None),
                                dict(x=(F32, (n, ch, t, h, w), "in"), out=(BF16, (n, t) + padded + (4,), "out")), {}, ["out"])
    # ---- pools ----
    shape, kernel, pad = WC.CL_POOL_CASES[0]
    pn, pc, pt, ph, pw = shape
    geom, (to, ho, wo) = WC._pool_geometry(shape, kernel, pad)
    cp, cp8, ps = _pitch(pc), inference.fp8_channel_pitch(pc), pt * ph * pw
    xs, ys = (pn, pt, ph, pw, cp), (pn, to, ho, wo, cp)
    rows["zsv_maxpool3d_bf16"] = (lambda q: L.zsv_maxpool3d_bf16(q["x"], *geom, q["y"], None), dict(x=(BF16, xs, "in"), y=(BF16, ys, "out")), {}, ["x", "y"])
    rows["zsv_maxpool3d_bf16_bwd"] = (lambda q: L.zsv_maxpool3d_bf16_bwd(q["dy"], q["x"], *geom, q["dx"], None),
                                      dict(dy=(BF16, ys, "in"), x=(BF16, xs, "in"), dx=(BF16, xs, "out")), {}, ["dy", "x", "dx"])
    rows["zsv_maxpool3d_fp8"] = (lambda q: L.zsv_maxpool3d_fp8(q["x"], *geom, q["y"], None),
                                 dict(x=(U8, (pn, pt, ph, pw, cp8), "in"), y=(U8, (pn, to, ho, wo, cp8), "out")), {}, ["x", "y"])
    rows["zsv_meanpool_bf16"] = (lambda q: L.zsv_meanpool_bf16(q["x"], pn, ps, pc, q["out"], None), dict(x=(BF16, xs, "in"), out=(F32, (pn, pc), "out")), {}, ["x"])
    rows["zsv_meanpool_fp8"] = (lambda q: L.zsv_meanpool_fp8(q["x"], pn, ps, pc, q["out"], None),
                                dict(x=(U8, (pn, pt, ph, pw, cp8), "in"), out=(F32, (pn, pc), "out")), {}, ["x"])
    rows["zsv_meanpool_bf16_bwd"] = (lambda q: L.zsv_meanpool_bf16_bwd(q["dpooled"], pn, ps, pc, q["dx"], None),
                                     dict(dpooled=(F32, (pn, pc), "in"), dx=(BF16, xs, "out")), {}, ["dx"])
    # ---- channels-last BatchNorm, the C3D ReLU + bias backward, the layout converters ----
    shape = (2, 45, 2, 7, 7)
    bn_n, bn_c = shape[:2]
    cp = _pitch(bn_c)
    cl = (bn_n,) + shape[2:] + (cp,)
    r = int(np.prod(cl[:-1]))
    nb = int(L.zsv_bn_cl_workspace_bytes(r, bn_c))
    assert nb > 0
    vec, act = (F32, (bn_c,), "in"), (BF16, cl, "in")
    stats = dict(save_mean=(F32, (bn_c,), "out"), save_invstd=(F32, (bn_c,), "out"), save_coef=(F32, (2, cp), "out"), running_mean=(F32, (bn_c,), "out"),
                 running_var=(F32, (bn_c,), "out"))
    rows["zsv_bn_cl_fwd_train"] = (lambda p: L.zsv_bn_cl_fwd_train(p["z"], p["residual"], r, bn_c, p["gamma"], p["beta"], p["running_mean"], p["running_var"], 0.1,
                                                                  1e-5, 1, p["y"], p["save_mean"], p["save_invstd"], p["save_coef"], p["ws"], nb, None),
                                   dict(stats, z=act, residual=act, gamma=vec, beta=vec, y=(BF16, cl, "out")), {"ws": nb}, ["z", "residual", "y"])
    rows["zsv_bn_cl_fwd_train_stats"] = (lambda p: L.zsv_bn_cl_fwd_train_stats(p["z"], p["residual"], r, bn_c, p["gamma"], p["beta"], p["running_mean"],
                                                                              p["running_var"], 0.1, 1e-5, 1, p["y"], p["save_mean"], p["save_invstd"],
                                                                              p["save_coef"], p["conv_partials"], 1, p["ws"], nb, None),
                                         dict(stats, z=act, residual=act, gamma=vec, beta=vec, conv_partials=(F32, (1, 2, cp), "in"), y=(BF16, cl, "out")),
                                         {"ws": nb}, ["z", "residual", "y"])
    grads = dict(dz=(BF16, cl, "out"), g_out=(BF16, cl, "out"), dgamma=(F32, (bn_c,), "out"), dbeta=(F32, (bn_c,), "out"))
    rows["zsv_bn_cl_bwd"] = (lambda p: L.zsv_bn_cl_bwd(p["dy"], p["y"], p["z"], r, bn_c, p["gamma"], p["save_mean"], p["save_invstd"], None, 1, p["dz"], p["g_out"],
                                                      p["dgamma"], p["dbeta"], p["ws"], nb, None),
                             dict(grads, dy=act, y=act, z=act, gamma=vec, save_mean=vec, save_invstd=vec), {"ws": nb}, ["dy", "y", "z", "dz", "g_out"])
    rows["zsv_bn_cl_fwd_eval"] = (lambda p: L.zsv_bn_cl_fwd_eval(p["z"], p["residual"], r, bn_c, p["gamma"], p["beta"], p["rm"], p["rv"], 1e-5, 1, p["y"], p["coef"],
                                                                None),
                                  dict(z=act, residual=act, gamma=vec, beta=vec, rm=vec, rv=vec, y=(BF16, cl, "out"), coef=(F32, (4, cp), "out")), {},
                                  ["z", "residual", "y"])
    rows["zsv_bn_cl_bwd_eval"] = (lambda p: L.zsv_bn_cl_bwd_eval(p["dy"], p["y"], p["z"], r, bn_c, p["coef"], 1, p["dz"], p["g_out"], p["dgamma"], p["dbeta"],
                                                                p["ws"], nb, None),
                                  dict(grads, dy=act, y=act, z=act, coef=(F32, (4, cp), "in")), {"ws": nb}, ["dy", "y", "z", "dz", "g_out"])
    rows["zsv_relu_bias_bwd_cl"] = (lambda p: L.zsv_relu_bias_bwd_cl(p["dy"], p["y"], r, bn_c, p["g_out"], p["dbias"], p["ws"], nb, None),
                                    dict(dy=act, y=act, g_out=(BF16, cl, "out"), dbias=(F32, (bn_c,), "out")), {"ws": nb}, ["dy", "y", "g_out"])
    cn, cc, ct, ch_, cw = WC.CONVERTER_SHAPES[0]
    cs, ccp = ct * ch_ * cw, _pitch(cc)
    rows["zsv_cl_bf16_to_ncs_f32"] = (lambda q: L.zsv_cl_bf16_to_ncs_f32(q["x"], cn, cs, cc, q["out"], None),
                                      dict(x=(BF16, (cn, ct, ch_, cw, ccp), "in"), out=(F32, (cn, cc, ct, ch_, cw), "out")), {}, ["x"])
    rows["zsv_ncs_f32_to_cl_bf16"] = (lambda q: L.zsv_ncs_f32_to_cl_bf16(q["x"], cn, cs, cc, q["out"], None),
                                      dict(x=(F32, (cn, cc, ct, ch_, cw), "in"), out=(BF16, (cn, ct, ch_, cw, ccp), "out")), {}, ["out"])
    return rows


REJECTIONS = ["zsv_conv3d_bf16_fwd", "zsv_conv3d_bf16_fwd_stats", "zsv_conv3d_bf16_dgrad, stride (1, 1, 1)", "zsv_conv3d_bf16_dgrad, stride (1, 2, 2)",
              "zsv_conv3d_bf16_wgrad", "zsv_conv3d_fp8_fwd", "zsv_clip_to_bf16", "zsv_maxpool3d_bf16", "zsv_maxpool3d_bf16_bwd", "zsv_maxpool3d_fp8",
              "zsv_meanpool_bf16", "zsv_meanpool_fp8", "zsv_meanpool_bf16_bwd", "zsv_bn_cl_fwd_train", "zsv_bn_cl_fwd_train_stats", "zsv_bn_cl_bwd",
              "zsv_bn_cl_fwd_eval", "zsv_bn_cl_bwd_eval", "zsv_relu_bias_bwd_cl", "zsv_cl_bf16_to_ncs_f32", "zsv_ncs_f32_to_cl_bf16"]


@pytest.mark.parametrize("entry", REJECTIONS, ids=[e.replace(", stride ", "_s").replace("(", "").replace(")", "").replace(", ", "") for e in REJECTIONS])
def test_channels_last_operands_off_a_16_byte_boundary_are_refused(entry):
    """Each channels-last operand in turn at +2 and at +8, in real guarded buffers of the operand's extent: ZSV_E_UNSUPPORTED, no
    band touched and every output payload -- the fp32 ones too -- still at its 0xFF prefill: nothing was launched.  The same
    operands on their boundaries are accepted (status 0), so the refusal is the alignment's."""
    rows = _rejections()
    assert sorted(rows) == sorted(REJECTIONS)
    launch, operands, works, channels_last = rows[entry]
    ins = {name: torch.zeros(shape, dtype=dtype) for name, (dtype, shape, role) in operands.items() if role == "in"}
    outs = {name: (dtype, shape) for name, (dtype, shape, role) in operands.items() if role == "out"}
    for name in ("gamma", "rv"):                           # (an accepted call divides by these)
        if name in ins:
            ins[name] += 1
    status, _ = call(launch, ins, outs, works)
    assert status == 0, f"{entry} on aligned operands: {lib().zsv_status_string(int(status)).decode()}"
    for name in channels_last + [w for w in works if w == "blob"]:          # (the packed weights are fetched in 16-byte pieces too)
        for shift in (2, 8):
            status, views = call(launch, ins, outs, works, (name,), shift)
            assert status == ZSV_E_UNSUPPORTED, f"{entry}, {name} at +{shift}: status {status} ({lib().zsv_status_string(int(status)).decode()})"
            for out, v in views.items():
                assert bool((raw(v) == 0xFF).all()), f"{entry}, {name} at +{shift}: the output {out} was written"


def test_absmax_bf16_takes_any_two_byte_address():
    """The one bf16 entry point without the 16-byte rule (its head / body / tail split starts at the address)."""
    L = lib()
    x = torch.randn(1027, generator=torch.Generator().manual_seed(1)).to(BF16)
    for shift in (2, 8, 14):
        status, v = call(lambda p: L.zsv_absmax_bf16(p["x"], x.numel(), p["amax"], None), dict(x=x), {"amax": (F32, (1,))}, None, ("x",), shift)
        assert status == 0                                   # (*amax holds the 0xFF.. prefill, a NaN pattern above every finite one)
    amax = G.guarded_copy(torch.zeros(1), DEV)
    xb = G.guarded_copy(x, DEV, shift=6)
    assert L.zsv_absmax_bf16(xb.ptr, x.numel(), amax.ptr, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(amax.payload.view(F32).cpu(), x.float().abs().max().reshape(1))


# =========================================================================================================================
# the Python surfaces: ops.* and torch.ops.zsv.* on contiguous views that start one float into a buffer
# =========================================================================================================================
def flat_view(t, requires_grad=False):
    """``t``'s values as ``flat[1:1 + n].view(shape)``: contiguous, 4 bytes past the allocation's 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, device=DEV)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.requires_grad_(requires_grad)


SURFACE_CONVS = [((1, 3, 3), (1, 1, 1), (0, 1, 1)), ((3, 1, 1), (1, 1, 1), (1, 0, 0)), ((3, 3, 3), (2, 2, 2), (1, 1, 1))]


@pytest.mark.parametrize("surface", ["ops", "torch.ops.zsv"])
@pytest.mark.parametrize("k,s,p", SURFACE_CONVS, ids=["1x3x3", "3x1x1", "3x3x3_s2"])
def test_convolution_wrappers_on_views_of_a_flat_buffer(k, s, p, surface):
    """(2, 16, 4, 12, 12) -> 32 channels, forward and backward through autograd: x, weight, bias and the upstream gradient are all
    views at +4; against F.conv3d in fp64."""
    g = torch.Generator().manual_seed(sum(k) * 7 + s[0])
    x, w, b = torch.randn(2, 16, 4, 12, 12, generator=g), torch.randn(32, 16, *k, generator=g) / np.sqrt(16 * np.prod(k)), torch.randn(32, generator=g)
    xr, wr, br = (v.double().requires_grad_() for v in (x, w, b))
    yr = F.conv3d(xr, wr, br, s, p)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())
    xd, wd, bd = (flat_view(v, True) for v in (x, w, b))
    y = ops.conv3d(xd, wd, bd, s, p) if surface == "ops" else torch_ops.load().conv3d(xd, wd, bd, list(s), list(p))
    y.backward(flat_view(gy))
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    T.close(y, yr, what=f"{surface} forward")
    T.close(xd.grad, xr.grad, what=f"{surface} input gradient")
    T.close(wd.grad, wr.grad, what=f"{surface} weight gradient")
    T.close(bd.grad, br.grad, what=f"{surface} bias gradient")


@pytest.mark.parametrize("surface,training", [("ops", True), ("ops", False), ("torch.ops.zsv", True)])
def test_batch_norm_wrappers_on_views_of_a_flat_buffer(surface, training):
    """BatchNorm + residual + ReLU (the torch operator has no residual input: BatchNorm + ReLU) on views at +4, running statistics
    included; against F.batch_norm in fp64."""
    g = torch.Generator().manual_seed(23)
    shape, c = (2, 16, 4, 12, 12), 16
    x, res, gy = (torch.randn(shape, generator=g) for _ in range(3))
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    rm, rv = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    use_res = surface == "ops"
    t = {k: v.double().requires_grad_() for k, v in dict(x=x, gamma=gamma, beta=beta, res=res).items()}
    rmr, rvr = rm.double().clone(), rv.double().clone()
    yr = F.batch_norm(t["x"], rmr, rvr, t["gamma"], t["beta"], training=training, momentum=0.1, eps=1e-5)
    yr = F.relu(yr + t["res"] if use_res else yr)
    yr.backward(gy.double())
    d = {k: flat_view(v, True) for k, v in dict(x=x, gamma=gamma, beta=beta, res=res).items()}
    rmd, rvd = flat_view(rm), flat_view(rv)
    if surface == "ops":
        y = ops.batch_norm_act(d["x"], d["gamma"], d["beta"], rmd, rvd, d["res"], training, 0.1, 1e-5, True)
    else:
        y = torch_ops.load().batch_norm_relu(d["x"], d["gamma"], d["beta"], rmd, rvd, 0.1, 1e-5, True)
    y.backward(flat_view(gy))
    torch.cuda.synchronize()
    T.close(y, yr, what=f"{surface} forward")
    for k in ("x", "gamma", "beta") + (("res",) if use_res else ()):
        T.close(d[k].grad, t[k].grad, what=f"{surface} gradient of {k}")
    T.close(rmd, rmr, what="running_mean")
    T.close(rvd, rvr, what="running_var")


def test_model_whose_parameters_are_views_of_one_flat_buffer(monkeypatch):
    """R(2+1)D-18 as in test_odd_clip_sizes_forward_backward_match_the_oracle, every parameter re-pointed at
    ``flat[off:off + n].view_as(p)`` with one float of padding in front (what a caller who flattens its parameters hands the
    library).  Train-mode embedding, loss and every parameter gradient against the CPU oracle with that test's thresholds, the panel
    cache on (panels are keyed by the weight's address); then one FusedAdam step against torch.optim.Adam over the oracle's
    parameters GIVEN THE DEVICE'S GRADIENTS (Adam's first step is lr * sign(g): on the oracle's own gradients, 5e-2 away, every
    near-zero gradient would flip a whole step), with test_optim_gpu.py's 2e-6 of the largest parameter."""
    from oracle import restatement as R
    monkeypatch.delenv("ZSV_NO_PANEL_CACHE", raising=False)
    opt = make_opt("r2plus1d_18")
    model = network.get_network(opt)
    weights = synthetic.keyed_state_dict(model.state_dict(), seed=4, bn_jitter=True)
    model.load_state_dict(weights)
    oracle = R.oracle_network(opt)
    oracle.load_state_dict(weights)
    n, t, h, w = 2, 4, 40, 40
    g = torch.Generator().manual_seed(h * w + t)
    x = (torch.randint(0, 256, (n, 1, 3, t, h, w), generator=g).float() / 255.0 - 1.0) / 2.0
    _, z = synthetic.synthetic_targets(n)
    oracle.train()
    y_ref = R.embed(oracle, x)
    loss_ref = F.mse_loss(y_ref, z)
    loss_ref.backward()

    model.to(DEV).train()
    params = list(model.parameters())
    flat = torch.zeros(sum(p.numel() + 1 for p in params), device=DEV)
    off = 0
    for p in params:
        off += 1                                             # one float of padding in front of every parameter
        view = flat[off:off + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
        off += p.numel()
    named = dict(model.named_parameters())
    assert any(p.dim() == 5 and p.data_ptr() % 16 for p in params), "no convolution weight off a 16-byte boundary"
    bn_vectors = [v for m in model.modules() if type(m).__name__.startswith("BatchNorm") for v in (m.weight, m.bias)]
    assert any(v.data_ptr() % 16 for v in bn_vectors), "no BatchNorm vector off a 16-byte boundary"
    assert sum(1 for p in params if p.data_ptr() % 16) > len(params) // 2

    y = train.embed(model, x.to(DEV))
    loss = F.mse_loss(y, z.to(DEV))
    loss.backward()
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    assert rel_err(y.detach().cpu().numpy(), y_ref.detach().numpy()) < 1e-4
    assert abs(loss.item() / loss_ref.item() - 1) < 1e-4
    ref_grads = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
    got = {k: p.grad for k, p in named.items() if p.grad is not None}
    assert set(got) == set(ref_grads)
    worst = 0.0
    for k, gr in ref_grads.items():
        a, b = got[k].detach().cpu().double().flatten(), gr.double().flatten()
        worst = max(worst, ((a - b).norm() / (b.norm() + 1e-30)).item())
    assert worst < 5e-2, f"worst per-parameter gradient rel-L2 {worst:.3e}"

    for k, p in oracle.named_parameters():                 # the same gradients on both sides
        p.grad = got[k].detach().cpu().clone() if k in got else None
    torch.optim.Adam(oracle.parameters(), lr=1e-3).step()
    optim.FusedAdam(model.parameters(), lr=1e-3).step()
    torch.cuda.synchronize()
    for k, q in oracle.named_parameters():
        p = named[k]
        assert flat.data_ptr() < p.data_ptr() < flat.data_ptr() + 4 * flat.numel(), f"{k} left the flat buffer"
        err = (p.detach().cpu() - q.detach()).abs().max().item()
        assert err <= 2e-6 * q.detach().abs().max().item() + 1e-12, (k, err)
