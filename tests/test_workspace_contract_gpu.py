"""The C ABI's memory contract (include/zsv_hip.h: "kernels never allocate: workspaces are passed in (query the size first)",
the caller owns every output), entry point by entry point, with guard bands (tests/guarded.py).

Every (entry point, case) is called through ctypes five to seven times.  Each run gets a workspace / blob / panel / mask table /
partials buffer of EXACTLY the queried size and every output in a buffer of exactly its shape, each between two 1 MiB guard
bands in an allocation of its own; the payloads are prefilled with 0x00 in the first run and 0xFF (NaN / -1 / the e4m3 NaN
code) in the second; the convolution and weight-gradient cases run a third time with the workspace 16 bytes past a 256-byte
boundary, the alignment the header promises to accept.  Every INPUT (x, w, dy, residuals, BatchNorm vectors, coefficient rows,
partials that are consumed) is handed over the same way: its bytes are the payload of a guarded buffer of exactly the extent the
header states, so the launch sees no tensor of the caching allocator.  Two more runs (prefill 0x00) poison the bands of EVERY
buffer of the run -- inputs, workspaces, blobs, panels, mask tables, outputs -- with 0xFF and then 0x7F (guarded.BAND_BYTES: a
NaN that survives every sum and product, then a huge finite value that wins every max and passes every ``> 0``).  Many kernels
fetch past the logical data on purpose (16-byte pieces, halo voxels, clamped loads) and rely on a mask, a clamp or a buffer
descriptor's range to keep the value out of the result: these runs pin that.  A last run (prefill 0xFF, ordinary bands) has every
fp32 / uint8 tensor operand, inputs and outputs alike, 4, 8 or 12 (1, 2 or 3) bytes past a 256-byte boundary -- the header asks
only for the element's alignment, each operand on its own -- while workspaces, panels, blobs, mask tables, coefficient rows and the
channels-last bf16 / e4m3 tensors keep theirs (guarded.element_shift).  Asserted after one synchronize:

(a) the call returns ZSV_OK;
(b) no guard band changed (nothing written before or past a buffer);
(c) the outputs of the runs are equal as raw bytes: the library has no floating-point atomics and fixed-order reductions, so a
    result may not depend on what a workspace held before the call;
(d) no output element of the 0xFF run still holds the prefill: the inputs are finite, a NaN / -1 is an element nobody wrote, or
    computed from workspace bytes nobody wrote;
(e) the outputs equal, as raw bytes, what the package's own wrapper (ops / amp / inference / train) returns for the same operands
    under the same switches (the other suites pin those wrappers to fp64 references); where no wrapper exposes the call, the
    comparison is the one the existing test of that entry point makes, with its tolerance;
(f) the outputs of the two poisoned runs equal the first run's as raw bytes: no byte outside the stated extent of an input (or
    of a workspace) may influence a result;
(g) no input's band changed and every input's payload holds the bytes it held before the call: inputs are const;
(h) the element-aligned run returns ZSV_OK, keeps (b), (d) and (g), fits workspaces of exactly the queried size (the queries see no
    pointer: they must cover the route an unaligned call falls back to) and gives the first run's bytes -- except for the calls
    ROUTE_CHANGES lists, whose kernel family follows the alignment: those are held to the fp64 reference of the row's own test.

A case is left out for an entry point only where that entry point's own ``*_supported`` / size query says it cannot run the
geometry.  The case tables are the ones of the other suites (rows with N = 22 or more than about 2 M output elements left out:
GPU_ROW_LIMIT).  The last test of the file asserts that every entry point ran, and on every row of its table, that each had its
element-aligned run, and that ROUTE_CHANGES is exact, and prints the counts: run the file as a whole.
"""
import collections
import ctypes
import zlib
from ctypes import byref

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_exact_cases as X
import guarded as G
import test_accuracy as TA
import test_amp_gpu as TAMP
import test_bf16_exact_gpu as BX
import test_bf16_gpu as TB
import test_fp8_gpu as F8
import test_ops_gpu as T

pytestmark = pytest.mark.gpu

from zeroshotvideoclassification_amd import _lib, amp, inference, ops, preprocess, train  # noqa: E402

DEV = "cuda"
F32, F64, I32, BF16, U8 = torch.float32, torch.float64, torch.int32, torch.bfloat16, torch.uint8
GPU_ROW_LIMIT = 2.5e6            # "about 2 M output elements"
# rows above the limit that stay, because no smaller row of their table reaches their kernel (the F(4,3) weight-gradient form)
KEPT_LARGE_ROWS = {"two_144_row_tiles", "m200_ragged_second_tile"}

COUNTS = collections.Counter()                 # entry point -> (case, switch) combinations run
ROWS_RUN = collections.defaultdict(set)        # (table, plain call) -> row names run


@pytest.fixture(autouse=True)
def _plain_wrappers(monkeypatch):
    """The wrappers the results are compared with run the same entry points as the test: no cached weight panel, no side stream."""
    monkeypatch.setenv("ZSV_NO_PANEL_CACHE", "1")
    monkeypatch.setenv("ZSV_WGRAD_STREAM", "0")


def lib():
    return _lib.load()


def numel(shape):
    return int(np.prod(shape)) if len(shape) else 1


# ---- (h): the only exceptions to bit equality under the element-aligned run ----------------------------------------------------------
# The calls whose KERNEL FAMILY follows the alignment of an fp32 operand (include/zsv_hip.h names the entry points): (entry point,
# "table/row") -- every switch combination of the row -- or (entry point, "table/row SWITCH=1"), mapped to the dispatch that sends the
# call elsewhere; None: the exception to a row's entry, a switch under which the aligned call already runs the kernel the unaligned
# one falls back to.  For a listed call the element-aligned run is held to the fp64 reference and the tolerance of the row's own test
# in test_ops_gpu.py, never to the first run.  The last test of the file fails for an entry no call matched and for a listed call
# whose bytes equalled the first run's after all: the list cannot grow slack.
TRING = "conv_wgrad.hip:564 (wgrad_dispatch: aligned16(x, dy) in front of the route table; the frame ring's entry)"
WINO = "conv_wgrad.hip:564 (wgrad_dispatch: aligned16(x, dy) in front of the route table; the Winograd form's entry)"
DMA = "conv_wgrad.hip:564 (wgrad_dispatch: aligned16(x, dy) in front of the route table; the LDS-DMA entry, sized at :490)"
STEM = "conv_wgrad_generic.hip:397 (the stem row kernel: aligned16(x, dy))"
STATS = "conv_tap.hip:560 (tap_lds_epilogue_ok: y -- zsv_conv3d_fwd_stat_tiles(d, y) answers 0, the plain form runs, no statistics)"
BIAS = "elementwise_pool.hip:384 (zsv_relu_bwd_bias: the float4 route sums db in another order; dx is the same bits)"
ROUTE_CHANGES = {}


def _listed(entries, line, rows, unless=()):
    for entry in entries:
        for row in rows:
            ROUTE_CHANGES[(entry, row)] = line
        for route in unless:
            ROUTE_CHANGES[(entry, route)] = None


_WGRAD = ("zsv_conv3d_wgrad", "zsv_conv3d_wgrad_masked")                    # one dispatch: wgrad_dispatch, conv_wgrad.hip:544
_listed(_WGRAD, TRING, [f"WGRAD_TRING_CASES/{r}" for r in ("t1_like", "cin230_cout128", "ragged_both", "many_clips")])      # (switched off: the LDS-DMA kernel, DMA)
_listed(_WGRAD, WINO, [f"WGRAD_WINO_CASES/{r}" for r in ("w_10_odd_chunks", "r3d_layer1_like_64_rows", "m56_ragged_columns", "partial_chunk_aligned_w",
                                                         "unaligned_w_whole_chunks", "two_144_row_tiles", "m200_ragged_second_tile")],
        unless=[f"WGRAD_WINO_CASES/{r} ZSV_NO_WGRAD_WINO=1" for r in ("w_10_odd_chunks", "partial_chunk_aligned_w", "unaligned_w_whole_chunks")])
_listed(_WGRAD, DMA, [f"WGRAD_DMA_CASES/{r}" for r in ("s1_like", "t1_like", "cout_230", "full_333", "wide_w", "many_slices")] + ["CONV_CASES/spatial_144"],
        unless=[f"WGRAD_DMA_CASES/{r} ZSV_NO_WGRAD_DMA=1" for r in ("s1_like", "t1_like", "cout_230", "full_333", "wide_w", "many_slices")])
_listed(_WGRAD, f"{WINO}, or {DMA}", ["VW_CASES/r3d_layer3_333"])
_listed(_WGRAD, STEM, [f"stem_rows/{r}" for r in ("n2_t4_56x56_c45", "n3_t2_112x112_c45", "n2_t3_24x40_c20", "n2_t2_30x128_c48")],
        unless=[f"stem_rows/{r} ZSV_NO_STEM_WGRAD=1" for r in ("n2_t4_56x56_c45", "n3_t2_112x112_c45", "n2_t3_24x40_c20", "n2_t2_30x128_c48")])
# every row whose forward runs the tap kernel with the statistics epilogue (the Winograd kernels' epilogue does not look at y)
_listed(("zsv_conv3d_fwd_full (statistics)",), STATS,
        ["CONV_CASES/temporal_s2", "CONV_CASES/pointwise_s2", "S2_DGRAD_CASES/temporal_ragged_16_byte_pieces", "two_frame_dense/n2_45_70", "two_frame_dense/n3_64_48",
         "VW_CASES/w30 ZSV_WINO_NO_VW=1"] +
        [f"WGRAD_DMA_CASES/{r}" for r in ("t1_like", "cin_45", "cout_230", "full_333", "one_chunk", "wide_w", "pointwise", "many_slices")] +
        [f"WGRAD_WINO_CASES/{r}" for r in ("w_10_odd_chunks", "m56_ragged_columns", "partial_chunk_aligned_w", "unaligned_w_whole_chunks", "two_144_row_tiles")] +
        [f"WGRAD_TRING_CASES/{r}" for r in ("t1_like", "ragged_both", "many_clips")])
_listed(("zsv_conv3d_fwd_pre",), STATS, [f"WGRAD_TRING_CASES/{r}" for r in ("t1_like", "ragged_both", "many_clips")])
_listed(("zsv_relu_bwd_bias",), BIAS, ["2x5x3x4x4", "2x64x4x8x8"])            # the shapes with S % 4 == 0

ROUTE_SEEN = collections.defaultdict(list)     # key of ROUTE_CHANGES -> per matching call: the element-aligned run's bytes equalled the first run's
ALIGN_RUNS = collections.Counter()             # entry point -> element-aligned runs (of the combinations COUNTS counts)
# entry points with no fp32 / uint8 tensor operand at all: nothing to move, no element-aligned run
NO_ELEMENT_OPERANDS = {"zsv_maxpool3d_bf16", "zsv_maxpool3d_bf16_bwd", "zsv_maxpool3d_fp8"}


def _route_key(entry, route):
    """The ROUTE_CHANGES key a call falls under: its own (with its switches) before its row's."""
    if route is None:
        return None
    for key in ((entry, route), (entry, route.split(" ")[0])):
        if key in ROUTE_CHANGES:
            return key
    return None


def contract(entry, launch, outs, works=None, shifted=False, defined=None, count=True, ins=None, aligned=(), route=None, reference=None):
    """guarded.run_contract on the device: (a) - (d), (f), (g), (h).  ``aligned``: fp32 / uint8 operands that keep their 16-byte
    alignment in the element-aligned run; ``route``: "table/row" + switches, what ROUTE_CHANGES is looked up with; ``reference``:
    the comparison (a function of the run's outputs) the element-aligned run gets where ROUTE_CHANGES lists the call.
    Returns name -> the first run's output (a copy)."""
    key = _route_key(entry, route)
    listed = key is not None and ROUTE_CHANGES[key] is not None
    assert not listed or reference is not None, f"{key}: listed in ROUTE_CHANGES, but the call site gives no reference"
    first, info = G.run_contract(entry, launch, outs, works, shifted, defined, ins, aligned, DEV, torch.cuda.synchronize,
                                 lambda s: lib().zsv_status_string(s).decode(), reference if listed else None)
    if key is not None:
        ROUTE_SEEN[key].append(bool(info["element_equal"]))
    if count:
        COUNTS[entry] += 1
        ALIGN_RUNS[entry] += 1 if info["element_operands"] else 0
    return first


def pick(o, *names, **renamed):
    """The operands of one call out of a test's operand dict: ``pick(o, "x", "w", y="x")`` = {x: o[x], w: o[w], y: o[x]}."""
    d = {k: o[k] for k in names}
    d.update({k: o[v] for k, v in renamed.items()})
    return d


def same_bytes(got, want, what):
    """(e): equal as raw bytes."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    if not torch.equal(got.contiguous().view(U8), want.contiguous().view(U8)):
        bad = int((got != want).sum())
        raise AssertionError(f"{what}: {bad} of {got.numel()} elements differ from the wrapper's result")


def params_of(test_function):
    return [m for m in test_function.pytestmark if m.name == "parametrize"][0].args[1]


# =========================================================================================================================
# fp32 convolution
# =========================================================================================================================
ConvRow = collections.namedtuple("ConvRow", "table name xs ws stride pad knobs base")


def _conv_rows():
    rows = []

    def add(table, name, xs, ws, stride, pad, knobs, base=()):
        stride = ops._triple(stride)
        d = ops.conv_desc(xs, ws, stride, pad)
        if xs[0] == 22:
            return
        if d.N * d.Cout * d.To * d.Ho * d.Wo > GPU_ROW_LIMIT and name not in KEPT_LARGE_ROWS:
            return
        rows.append(ConvRow(table, str(name), tuple(xs), tuple(ws), stride, tuple(pad), [()] + list(knobs), tuple(base)))

    for name, n, cin, t, h, w, cout, k, s, p, _bias in T.CONV_CASES:
        add("CONV_CASES", name, (n, cin, t, h, w), (cout, cin) + k, s, p, [])
    for name, n, cin, thw, cout, k, p in T.WGRAD_DMA_CASES:
        add("WGRAD_DMA_CASES", name, (n, cin) + thw, (cout, cin) + k, 1, p, [(("ZSV_NO_WGRAD_DMA", "1"),)])
    for name, n, cin, thw, cout, kt in T.WGRAD_WINO_CASES:
        add("WGRAD_WINO_CASES", name, (n, cin) + thw, (cout, cin, kt, 3, 3), 1, (kt // 2, 1, 1),
            [(("ZSV_NO_WGRAD_WINO4", "1"),), (("ZSV_NO_WGRAD_WINO", "1"),)])
    for name, n, cin, thw, cout in T.WGRAD_TRING_CASES:
        add("WGRAD_TRING_CASES", name, (n, cin) + thw, (cout, cin, 3, 1, 1), 1, (1, 0, 0),
            [(("ZSV_NO_WGRAD_TRING", "1"),), (("ZSV_WGRAD_TRING_SLICES", "7"),)])
    for name, n, cin, cout, thw, kind in T.S2_DGRAD_CASES:
        k, s, p = ((1, 3, 3), (1, 2, 2), (0, 1, 1)) if kind == "hw" else ((3, 1, 1), (2, 1, 1), (1, 0, 0))
        add("S2_DGRAD_CASES", name, (n, cin) + thw, (cout, cin) + k, s, p,
            [(("ZSV_NO_DGRAD_S2", "1"),), (("ZSV_DGRAD_S2_NO_X4", "1"),)] +
            [(("ZSV_DGRAD_S2_BN", bn), ("ZSV_DGRAD_S2_KS", ks)) for bn in ("64", "128") for ks in ("1", "2", "3")])   # tile width x K parts
    for name, n, cin, cout, kt, thw in T.VW_CASES:
        add("VW_CASES", name, (n, cin) + thw, (cout, cin, kt, 3, 3), 1, (kt // 2, 1, 1), [(("ZSV_WINO_NO_VW", "1"),)],
            base=(("ZSV_WINO_VW_MIN_WGS", "1"),))
    for n, t, h, w, cout in params_of(T.test_stem_weight_gradient_row_kernel):
        add("stem_rows", f"n{n}_t{t}_{h}x{w}_c{cout}", (n, 3, t, h, w), (cout, 3, 1, 7, 7), (1, 2, 2), (0, 3, 3), [(("ZSV_NO_STEM_WGRAD", "1"),)])
    for n, cin, cout, hw in params_of(T.test_two_frame_temporal_conv_in_dense_form):
        add("two_frame_dense", f"n{n}_{cin}_{cout}", (n, cin, 2) + tuple(hw), (cout, cin, 3, 1, 1), 1, (1, 0, 0), [(("ZSV_NO_T2_DENSE", "1"),)])
    # the geometries of test_conv3d_split_k_small_grid (K parts: partial slabs in the workspace + an ordered reduce)
    for cin, cout, k, s, p, t, h, w in [(256, 320, (1, 3, 3), (1, 1, 1), (0, 1, 1), 2, 7, 7), (320, 128, (3, 1, 1), (1, 1, 1), (1, 0, 0), 2, 7, 7),
                                        (128, 200, (1, 3, 3), (1, 2, 2), (0, 1, 1), 2, 14, 14)]:
        add("split_k", f"{cin}_{cout}_k{k[0]}{k[1]}{k[2]}", (2, cin, t, h, w), (cout, cin) + k, s, p,
            [(("ZSV_SPLITK_REDUCE_SCALAR", "1"),), (("ZSV_NO_SPLITK", "1"),)])
    # test_weight_gradient_slab_sum_rows_equals_the_generic_sum, test_tiled_weight_pack_equals_the_elementwise_pack
    add("slab_sum_rows", "6x96_200", (6, 96, 2, 7, 7), (200, 96, 1, 3, 3), 1, (0, 1, 1), [(("ZSV_NO_SLAB_SUM_ROWS", "1"),)])
    for xs, ws, stride, pad in [((4, 128, 4, 14, 14), (300, 128, 1, 3, 3), (1, 2, 2), (0, 1, 1)), ((3, 200, 4, 7, 7), (120, 200, 3, 1, 1), (2, 1, 1), (1, 0, 0)),
                                ((3, 96, 2, 7, 7), (130, 96, 1, 3, 3), 1, (0, 1, 1)), ((2, 40, 3, 6, 6), (50, 40, 3, 3, 3), (2, 2, 2), (1, 1, 1))]:
        add("pack_tiled", f"{ws[1]}_{ws[0]}", xs, ws, stride, pad, [(("ZSV_NO_PACK_TILED", "1"),), (("ZSV_NO_WINO", "1"),)])
    return rows


CONV_ROWS = _conv_rows()
CONV_TABLES = ["CONV_CASES", "WGRAD_DMA_CASES", "WGRAD_WINO_CASES", "WGRAD_TRING_CASES", "S2_DGRAD_CASES", "VW_CASES", "stem_rows",
               "two_frame_dense", "split_k", "slab_sum_rows", "pack_tiled"]


def _conv_operands(row):
    g = torch.Generator().manual_seed(zlib.crc32((row.table + row.name).encode()))
    d = ops.conv_desc(row.xs, row.ws, row.stride, row.pad)
    ys = (d.N, d.Cout, d.To, d.Ho, d.Wo)
    k = numel(row.ws[1:])
    o = dict(x=torch.randn(row.xs, generator=g), w=torch.randn(row.ws, generator=g) / np.sqrt(k), bias=torch.randn(row.ws[0], generator=g),
             res=torch.randn(ys, generator=g), dy=torch.randn(ys, generator=g), add=torch.randn(row.xs, generator=g))
    pitch = (d.Cin + 15) // 16 * 16
    coef = torch.zeros(2, pitch)
    coef[0, :d.Cin] = torch.rand(d.Cin, generator=g) + 0.5
    coef[1, :d.Cin] = torch.randn(d.Cin, generator=g) * 0.2
    o["coef"] = coef
    return d, ys, {k_: v.to(DEV) for k_, v in o.items()}, g


_REFERENCE = {}


def _conv_reference(row, o, want):
    """The fp64 references of the row's own test in test_ops_gpu.py (F.conv3d and its weight gradient on the CPU), computed when a
    ROUTE_CHANGES row asks and kept for the row's other calls and switches: "y", "dw", and "y_pre" / "dw_pre" with x read through
    relu(x * scale[c] + shift[c])."""
    key = (row.table, row.name)
    if _REFERENCE.get("key") != key:
        _REFERENCE.clear()
        _REFERENCE["key"] = key
    if want not in _REFERENCE:
        x, w, dy = (o[k].double().cpu() for k in ("x", "w", "dy"))
        if want.endswith("_pre"):
            cin = row.xs[1]
            a, b = (o["coef"][i, :cin].double().cpu().view(1, cin, 1, 1, 1) for i in (0, 1))
            x = F.relu(x * a + b)
        if want.startswith("y"):
            _REFERENCE[want] = F.conv3d(x, w, None, row.stride, row.pad)
        else:
            _REFERENCE[want] = torch.nn.grad.conv3d_weight(x, row.ws, dy, stride=row.stride, padding=row.pad)
    return _REFERENCE[want]


def _conv_entry_points(row, tag):
    """Every fp32 convolution entry point on one row under the switches in force."""
    L = lib()
    d, ys, o, g = _conv_operands(row)
    dp = byref(d)
    nf, nd, nw = int(L.zsv_conv3d_fwd_workspace_bytes(dp)), int(L.zsv_conv3d_dgrad_workspace_bytes(dp)), int(L.zsv_conv3d_wgrad_workspace_bytes(dp))
    what = f"{row.table}/{row.name}{tag}"

    # ---- the wrapper's results (e) ----
    xg, wg = o["x"].clone().requires_grad_(), o["w"].clone().requires_grad_()
    yw = ops.conv3d(xg, wg, None, row.stride, row.pad)
    yw.backward(o["dy"])
    ops.join_wgrad_streams()
    with torch.no_grad():
        yw_relu = ops.conv3d(o["x"], o["w"], o["bias"], row.stride, row.pad, relu=True)
        yw_stats, stats_w = ops.conv3d(o["x"], o["w"], None, row.stride, row.pad, want_stats=True)
    torch.cuda.synchronize()

    # ---- forward ----
    def fwd(b, r, relu, stats, tiles):
        return lambda p: L.zsv_conv3d_fwd_full(dp, p["x"], p["w"], p.get(b), p.get(r), p["y"], relu, p.get(stats), tiles, p["ws"], nf, None)

    # zsv_conv3d_fwd_stat_tiles(d, y) answers for the y it is given: every run asks for its own y, and where the answer is 0 it
    # calls the plain form and gets no statistics, as the wrapper does
    asked = {}

    def tiles_for(p):
        asked["tiles"] = int(L.zsv_conv3d_fwd_stat_tiles(dp, p["y"]))
        assert asked["tiles"] in (0, tiles), f"{what}: zsv_conv3d_fwd_stat_tiles says {asked['tiles']} for this y and {tiles} for an aligned one"
        return asked["tiles"]

    def partials_written(name, v):
        return v if name != "bn_partials" or asked["tiles"] else v[:, :, :0]

    def y_reference(want):
        return lambda got: T.close(got["y"], _conv_reference(row, o, want), what=f"{what}: forward on element-aligned operands, against fp64")

    y = contract("zsv_conv3d_fwd_full", fwd(None, None, 0, None, 0), {"y": (F32, ys)}, {"ws": nf}, shifted=True, ins=pick(o, "x", "w"), route=what)["y"]
    same_bytes(y, yw.detach(), f"{what}: forward")
    ROWS_RUN[(row.table, "fwd")].add(row.name)
    yb = contract("zsv_conv3d_fwd_full (bias + ReLU)", fwd("bias", None, 1, None, 0), {"y": (F32, ys)}, {"ws": nf}, shifted=True,
                  ins=pick(o, "x", "w", "bias"), route=what)["y"]
    same_bytes(yb, yw_relu, f"{what}: forward + bias + ReLU")
    if L.zsv_conv3d_fwd_add_supported(dp):
        yr = contract("zsv_conv3d_fwd_full (residual)", fwd("bias", "res", 1, None, 0), {"y": (F32, ys)}, {"ws": nf}, shifted=True,
                      ins=pick(o, "x", "w", "bias", "res"), route=what)["y"]
        conv = torch.nn.Conv3d(d.Cin, d.Cout, row.ws[2:], row.stride, row.pad, bias=True).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(o["w"])
            conv.bias.copy_(o["bias"])
            same_bytes(yr, inference._ConvOpF32(conv, None, True)(o["x"], o["res"]), f"{what}: forward + bias + residual + ReLU")
    probe = G.guarded_like(F32, ys, DEV, 0)
    tiles = int(L.zsv_conv3d_fwd_stat_tiles(dp, probe.ptr))
    assert (tiles > 0) == (stats_w is not None), f"{what}: the statistics query disagrees with the wrapper's"
    if tiles > 0:
        out = contract("zsv_conv3d_fwd_full (statistics)",
                       lambda p: fwd(None, None, 0, "bn_partials", tiles)(p) if tiles_for(p) else fwd(None, None, 0, None, 0)(p),
                       {"y": (F32, ys), "bn_partials": (F32, (2, d.Cout, tiles))}, {"ws": nf}, shifted=True, ins=pick(o, "x", "w"),
                       defined=partials_written, route=what, reference=y_reference("y"))
        same_bytes(out["y"], yw_stats, f"{what}: forward with the statistics epilogue")
        same_bytes(out["bn_partials"], stats_w, f"{what}: statistics")

    # ---- input gradient ----
    dx = contract("zsv_conv3d_dgrad", lambda p: L.zsv_conv3d_dgrad(dp, p["dy"], p["w"], p["dx"], p["ws"], nd, None),
                  {"dx": (F32, row.xs)}, {"ws": nd}, shifted=True, ins=pick(o, "dy", "w"), route=what)["dx"]
    same_bytes(dx, xg.grad, f"{what}: dgrad")
    ROWS_RUN[(row.table, "dgrad")].add(row.name)
    if L.zsv_conv3d_dgrad_add_supported(dp):
        dxa = contract("zsv_conv3d_dgrad_add", lambda p: L.zsv_conv3d_dgrad_add(dp, p["dy"], p["w"], p["add"], p["dx"], p["ws"], nd, None),
                       {"dx": (F32, row.xs)}, {"ws": nd}, shifted=True, ins=pick(o, "dy", "w", "add"), route=what)["dx"]
        T.close(dxa, dx.double() + o["add"].double(), rtol=1e-6, what=f"{what}: dgrad + shortcut gradient")
    for st in (1, 2):
        if L.zsv_conv3d_dgrad_add_strided_supported(dp, st, 2, 2):
            sub = torch.randn((d.N, d.Cin, -(-d.Ti // st), d.Hi // 2, d.Wi // 2), generator=g).to(DEV)
            dxs = contract("zsv_conv3d_dgrad_add_strided",
                           lambda p: L.zsv_conv3d_dgrad_add_strided(dp, p["dy"], p["w"], p["sub"], st, 2, 2, p["dx"], p["ws"], nd, None),
                           {"dx": (F32, row.xs)}, {"ws": nd}, shifted=True, ins=dict(pick(o, "dy", "w"), sub=sub), route=what)["dx"]
            ref = dx.double()
            ref[:, :, ::st, :2 * (d.Hi // 2):2, :2 * (d.Wi // 2):2] += sub.double()
            T.close(dxs, ref, rtol=1e-6, what=f"{what}: dgrad + strided shortcut gradient (st = {st})")

    # ---- weight gradient ----
    def dw_reference(want, rtol):
        return lambda got: T.close(got["dw"], _conv_reference(row, o, want), rtol=rtol, what=f"{what}: wgrad on element-aligned operands, against fp64")

    rtol = 5e-5 if row.table == "stem_rows" else 2e-5              # (test_stem_weight_gradient_row_kernel; the other tables' tests)
    dw = contract("zsv_conv3d_wgrad", lambda p: L.zsv_conv3d_wgrad(dp, p["x"], p["dy"], p["dw"], p["ws"], nw, None),
                  {"dw": (F32, row.ws)}, {"ws": nw}, shifted=True, ins=pick(o, "x", "dy"), route=what, reference=dw_reference("dw", rtol))["dw"]
    same_bytes(dw, wg.grad, f"{what}: wgrad")
    ROWS_RUN[(row.table, "wgrad")].add(row.name)
    nm = int(L.zsv_conv3d_wgrad_mask_bytes(dp))
    dwm = contract("zsv_conv3d_wgrad_masked",
                   lambda p: [L.zsv_conv3d_wgrad_mask(dp, p["mask"], None) if nm else 0,
                              L.zsv_conv3d_wgrad_masked(dp, p["x"], p["dy"], p["dw"], p["ws"], nw, p["mask"] if nm else None, None)],
                   {"dw": (F32, row.ws)}, {"ws": nw, "mask": nm}, shifted={"ws"}, ins=pick(o, "x", "dy"), route=what,
                   reference=dw_reference("dw", rtol))["dw"]
    same_bytes(dwm, dw, f"{what}: wgrad with a kept tap-validity table")

    # ---- the BatchNorm + ReLU folded into the convolution ----
    if L.zsv_conv3d_pre_supported(dp):
        pitch = int(o["coef"].shape[1])
        wp = o["w"].clone().requires_grad_()
        yp, sp = ops.conv3d_pre(o["x"], o["coef"], wp, row.stride, row.pad, want_stats=True)
        yp.backward(o["dy"])
        ops.join_wgrad_streams()
        torch.cuda.synchronize()
        outs = {"y": (F32, ys)}
        if tiles > 0:
            outs["bn_partials"] = (F32, (2, d.Cout, tiles))
        out = contract("zsv_conv3d_fwd_pre",
                       lambda p: L.zsv_conv3d_fwd_pre(dp, p["x"], p["coef"], pitch, p["w"], p["y"], *((p["bn_partials"], tiles) if tiles and tiles_for(p)
                                                                                                   else (None, 0)), p["ws"], nf, None),
                       outs, {"ws": nf}, shifted=True, ins=pick(o, "x", "coef", "w"), aligned={"coef"}, defined=partials_written, route=what,
                       reference=y_reference("y_pre"))
        same_bytes(out["y"], yp.detach(), f"{what}: forward through BatchNorm + ReLU")
        if tiles > 0:
            same_bytes(out["bn_partials"], sp, f"{what}: statistics of the forward through BatchNorm + ReLU")
        dwp = contract("zsv_conv3d_wgrad_pre", lambda p: L.zsv_conv3d_wgrad_pre(dp, p["x"], p["coef"], pitch, p["dy"], p["dw"], p["ws"], nw, None),
                       {"dw": (F32, row.ws)}, {"ws": nw}, shifted=True, ins=pick(o, "x", "coef", "dy"), aligned={"coef"}, route=what,
                       reference=dw_reference("dw_pre", 5e-5))["dw"]       # (test_batchnorm_relu_folded_into_the_temporal_convolution)
        same_bytes(dwp, wp.grad, f"{what}: wgrad through BatchNorm + ReLU")


@pytest.mark.parametrize("row", CONV_ROWS, ids=[f"{r.table}-{r.name}" for r in CONV_ROWS])
def test_fp32_convolution_entry_points(row, monkeypatch):
    for k, v in row.base:
        monkeypatch.setenv(k, v)
    for knobs in row.knobs:
        for k, v in knobs:
            monkeypatch.setenv(k, v)                      # (tests/conftest.py: the library re-reads its switches; sizes are re-queried)
        _conv_entry_points(row, "".join(f" {k}={v}" for k, v in knobs))
        for k, _ in knobs:
            monkeypatch.delenv(k)


# =========================================================================================================================
# weight panels packed ahead of the call
# =========================================================================================================================
# PANEL_CASES, and one row more: none of them has the forward that reads its input through BatchNorm + ReLU
# (zsv_conv3d_fwd_pre_panel); the first row of WGRAD_TRING_CASES does
_name, _n, _cin, _thw, _cout = T.WGRAD_TRING_CASES[0]
PANEL_ROWS = list(T.PANEL_CASES) + [("bn_folded_" + _name, (_n, _cin) + _thw, (_cout, _cin, 3, 1, 1), 1, (1, 0, 0))]


@pytest.mark.parametrize("case", PANEL_ROWS, ids=[c[0] for c in PANEL_ROWS])
def test_weight_panels(case):
    name, xs, ws, stride, pad = case
    L = lib()
    row = ConvRow("PANEL_CASES", name, xs, ws, ops._triple(stride), pad, [()], ())
    d, ys, o, g = _conv_operands(row)
    dp = byref(d)
    nf, nd = int(L.zsv_conv3d_fwd_workspace_bytes(dp)), int(L.zsv_conv3d_dgrad_workspace_bytes(dp))

    def panel_bytes(direction, extras):
        nb = ctypes.c_size_t(0)
        _lib.check(L.zsv_conv3d_panel_query(dp, direction, extras, byref(nb)), "zsv_conv3d_panel_query")
        assert nb.value > 0, (name, direction, extras)
        return int(nb.value)

    def pack(p, direction, extras, nb):
        job = _lib.PackJob()
        s = L.zsv_conv3d_panel_job(dp, direction, extras, p["w"], p["panel"], nb, byref(job))
        if s:
            return s
        job.first_block = 0
        return L.zsv_pack_multi(p["table"](torch.frombuffer(bytearray(bytes(job)), dtype=U8), "jobs"), 1, (int(job.total) + 1023) // 1024, None)

    for extras in (0, 1):
        nb = panel_bytes(0, extras)
        y = contract("zsv_pack_multi + zsv_conv3d_fwd_full_panel",
                     lambda p: [pack(p, 0, extras, nb),
                                L.zsv_conv3d_fwd_full_panel(dp, p["x"], p["w"], p["bias"], None, p["y"], extras, None, 0, p["ws"], nf, None, p["panel"], nb)],
                     {"y": (F32, ys)}, {"ws": nf, "panel": nb}, shifted={"ws"}, ins=dict(pick(o, "x", "w"), bias=o["bias"] if extras else None))["y"]
        with torch.no_grad():
            same_bytes(y, ops.conv3d(o["x"], o["w"], o["bias"] if extras else None, stride, pad, relu=bool(extras)), f"{name}: forward, extras {extras}")
    nb = panel_bytes(1, 0)
    dx = contract("zsv_pack_multi + zsv_conv3d_dgrad_add_panel",
                  lambda p: [pack(p, 1, 0, nb), L.zsv_conv3d_dgrad_add_panel(dp, p["dy"], p["w"], None, p["dx"], p["ws"], nd, None, p["panel"], nb)],
                  {"dx": (F32, xs)}, {"ws": nd, "panel": nb}, shifted={"ws"}, ins=pick(o, "dy", "w"))["dx"]
    xg = o["x"].clone().requires_grad_()
    ops.conv3d(xg, o["w"], None, stride, pad).backward(o["dy"])
    same_bytes(dx, xg.grad, f"{name}: dgrad")
    if L.zsv_conv3d_pre_supported(dp):
        pitch = int(o["coef"].shape[1])
        y = contract("zsv_pack_multi + zsv_conv3d_fwd_pre_panel",
                     lambda p: [pack(p, 0, 0, panel_bytes(0, 0)),
                                L.zsv_conv3d_fwd_pre_panel(dp, p["x"], p["coef"], pitch, p["w"], p["y"], None, 0, p["ws"], nf, None, p["panel"],
                                                           panel_bytes(0, 0))],
                     {"y": (F32, ys)}, {"ws": nf, "panel": panel_bytes(0, 0)}, shifted={"ws"}, ins=pick(o, "x", "coef", "w"), aligned={"coef"})["y"]
        with torch.no_grad():
            same_bytes(y, ops.conv3d_pre(o["x"], o["coef"], o["w"], stride, pad), f"{name}: forward through BatchNorm + ReLU")
    for st in (1, 2):
        if L.zsv_conv3d_dgrad_add_strided_supported(dp, st, 2, 2):
            sub = torch.randn((d.N, d.Cin, -(-d.Ti // st), d.Hi // 2, d.Wi // 2), generator=g).to(DEV)
            dxs = contract("zsv_pack_multi + zsv_conv3d_dgrad_add_strided_panel",
                           lambda p: [pack(p, 1, 0, nb), L.zsv_conv3d_dgrad_add_strided_panel(dp, p["dy"], p["w"], p["sub"], st, 2, 2, p["dx"], p["ws"], nd,
                                                                                              None, p["panel"], nb)],
                           {"dx": (F32, xs)}, {"ws": nd, "panel": nb}, shifted={"ws"}, ins=dict(pick(o, "dy", "w"), sub=sub))["dx"]
            ref = dx.double()
            ref[:, :, ::st, :2 * (d.Hi // 2):2, :2 * (d.Wi // 2):2] += sub.double()
            T.close(dxs, ref, rtol=1e-6, what=f"{name}: dgrad + strided shortcut gradient (panel)")
    ROWS_RUN[("PANEL_CASES", "panel")].add(name)


# =========================================================================================================================
# reductions and BatchNorm
# =========================================================================================================================
BN_SHAPES = [(n, c) + tuple(s) for n, c, s in T.BN_CASES] + [(1, 1, 1, 1, 2), (2, 3, 1, 1, 1), (1, 260, 1, 3, 3), (5, 2, 3, 5, 7)]   # + the edge shapes


def _bn_operands(shape):
    n, c = shape[:2]
    g = torch.Generator().manual_seed(n * 1000 + c)
    o = dict(x=torch.randn(shape, generator=g) * 2 + 0.5, res=torch.randn(shape, generator=g), gamma=torch.rand(c, generator=g) + 0.5,
             beta=torch.randn(c, generator=g) * 0.1, rm=torch.randn(c, generator=g) * 0.1, rv=torch.rand(c, generator=g) + 0.5,
             dy=torch.randn(shape, generator=g))
    return {k: v.to(DEV) for k, v in o.items()}


@pytest.mark.parametrize("shape", BN_SHAPES, ids=["x".join(map(str, s)) for s in BN_SHAPES])
def test_channel_sum_and_relu_bwd_bias(shape):
    L = lib()
    o = _bn_operands(shape)
    n, c = shape[:2]
    s = numel(shape[2:])
    nb = int(L.zsv_channel_sum_workspace_bytes(n, c, s))
    db = contract("zsv_channel_sum", lambda p: L.zsv_channel_sum(p["dy"], n, c, s, p["db"], p["ws"], nb, None), {"db": (F32, (c,))}, {"ws": nb},
                  ins=pick(o, "dy"))["db"]
    same_bytes(db, ops.channel_sum(o["dy"]), "channel_sum")
    ref = torch.where(o["x"] > 0, o["dy"], torch.zeros_like(o["dy"]))

    def masked_and_summed(got, what="bias gradient"):                                     # (test_relu_bwd_bias_on_misaligned_views)
        assert torch.equal(got["dx"], ref)
        T.close(got["db"], ref.double().sum(dim=(0, 2, 3, 4)), what=what)

    out = contract("zsv_relu_bwd_bias", lambda p: L.zsv_relu_bwd_bias(p["dy"], p["y"], p["dx"], n, c, s, p["db"], p["ws"], nb, None),
                   {"dx": (F32, shape), "db": (F32, (c,))}, {"ws": nb}, ins=pick(o, "dy", y="x"), route="x".join(map(str, shape)),
                   reference=lambda got: masked_and_summed(got, "bias gradient on element-aligned operands"))
    masked_and_summed(out)
    ROWS_RUN[("BN_CASES", "channel_sum")].add(shape)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("use_res", [False, True], ids=["no_res", "res"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=["x".join(map(str, s)) for s in BN_SHAPES])
def test_batchnorm_entry_points(shape, use_res, relu):
    L = lib()
    o = _bn_operands(shape)
    n, c = shape[:2]
    s = numel(shape[2:])
    nb = int(L.zsv_bn_workspace_bytes(n, c, s))
    fwd_ins = dict(pick(o, "x", "gamma", "beta"), res=o["res"] if use_res else None)
    r = 1 if relu else 0
    stat_outs = {"save_mean": (F32, (c,)), "save_invstd": (F32, (c,)), "running_mean": (F32, (c,), o["rm"]), "running_var": (F32, (c,), o["rv"])}

    # ---- the wrapper (e): forward and backward, training and frozen ----
    def wrapper(training, stats=None):
        t = {k: o[k].clone().requires_grad_() for k in ("x", "gamma", "beta")}
        rg = o["res"].clone().requires_grad_() if use_res else None
        rm, rv = o["rm"].clone(), o["rv"].clone()
        y = ops.batch_norm_act(t["x"], t["gamma"], t["beta"], rm, rv, rg, training, 0.1, 1e-5, relu, stats=stats)
        y.backward(o["dy"])
        torch.cuda.synchronize()
        return dict(y=y.detach(), rm=rm, rv=rv, dx=t["x"].grad, dgamma=t["gamma"].grad, dbeta=t["beta"].grad, dres=rg.grad if use_res else None)

    # ---- training forward ----
    wt = wrapper(True)
    out = contract("zsv_bn_fwd_train",
                   lambda p: L.zsv_bn_fwd_train(p["x"], n, c, s, p["gamma"], p["beta"], p["res"], r, p["y"], p["save_mean"], p["save_invstd"],
                                                p["running_mean"], p["running_var"], 0.1, 1e-5, p["ws"], nb, None),
                   dict(stat_outs, y=(F32, shape)), {"ws": nb}, ins=fwd_ins)
    same_bytes(out["y"], wt["y"], "bn_fwd_train: y")
    same_bytes(out["running_mean"], wt["rm"], "bn_fwd_train: running_mean")
    same_bytes(out["running_var"], wt["rv"], "bn_fwd_train: running_var")
    xd = o["x"].double()
    mean, var = xd.mean(dim=(0, 2, 3, 4)), xd.var(dim=(0, 2, 3, 4), unbiased=False)
    T.close(out["save_mean"], mean, rtol=1e-4, what="save_mean")
    T.close(out["save_invstd"], torch.rsqrt(var + 1e-5), rtol=1e-4, what="save_invstd")
    save_mean, save_invstd, y_fwd = out["save_mean"], out["save_invstd"], out["y"]
    # the same from epilogue partials: three column tiles over the voxel axis (as many as the voxels allow)
    tiles = min(3, s)
    cuts = [s * i // tiles for i in range(tiles + 1)]
    xs_ = o["x"].reshape(n, c, s)
    partials = torch.stack([torch.stack([xs_[:, :, a:b].sum(dim=(0, 2)) for a, b in zip(cuts, cuts[1:])], 1),
                            torch.stack([(xs_[:, :, a:b] ** 2).sum(dim=(0, 2)) for a, b in zip(cuts, cuts[1:])], 1)]).contiguous()
    ws_ = wrapper(True, partials)
    out = contract("zsv_bn_fwd_train_stats",
                   lambda p: L.zsv_bn_fwd_train_stats(p["x"], n, c, s, p["gamma"], p["beta"], p["res"], r, p["y"], p["save_mean"], p["save_invstd"],
                                                      p["running_mean"], p["running_var"], 0.1, 1e-5, p["conv_partials"], tiles, p["ws"], nb, None),
                   dict(stat_outs, y=(F32, shape)), {"ws": nb}, ins=dict(fwd_ins, conv_partials=partials))
    same_bytes(out["y"], ws_["y"], "bn_fwd_train_stats: y")
    same_bytes(out["running_mean"], ws_["rm"], "bn_fwd_train_stats: running_mean")
    same_bytes(out["running_var"], ws_["rv"], "bn_fwd_train_stats: running_var")
    if not use_res and not relu:
        pitch = (c + 15) // 16 * 16
        out = contract("zsv_bn_fwd_train_coeffs",
                       lambda p: L.zsv_bn_fwd_train_coeffs(p["x"], n, c, s, p["gamma"], p["beta"], p["save_mean"], p["save_invstd"], p["running_mean"],
                                                           p["running_var"], 0.1, 1e-5, None, 0, p["coef"], pitch, p["ws"], nb, None),
                       dict(stat_outs, coef=(F32, (2, pitch))), {"ws": nb}, ins=pick(o, "x", "gamma", "beta"), aligned={"coef"})
        assert int(torch.count_nonzero(out["coef"][:, c:])) == 0, "coef entries C .. coef_pitch-1 must be zero"
        rm, rv = o["rm"].clone(), o["rv"].clone()
        _, coef_w = ops._BatchNormDeferred.apply(o["x"], o["gamma"], o["beta"], rm, rv, 0.1, 1e-5, None)
        same_bytes(out["coef"], coef_w, "bn_fwd_train_coeffs: coef")
        same_bytes(out["running_var"], rv, "bn_fwd_train_coeffs: running_var")
        same_bytes(out["save_mean"], save_mean, "bn_fwd_train_coeffs: save_mean")

    # ---- training backward: every ReLU mode this forward allows, with and without the residual gradient ----
    # (e): the combination the wrapper itself calls is held to the wrapper's bytes, the others to the fp64 reference with the
    # tolerance of test_batchnorm_train_fwd_bwd
    modes = [0] if not relu else ([1] if use_res else [1, 2])
    wrapper_calls = (0, False) if not relu else ((1, True) if use_res else (2, False))

    def reference(training):
        t = {k: o[k].double().cpu().requires_grad_() for k in ("x", "gamma", "beta")}
        y = F.batch_norm(t["x"], o["rm"].double().cpu(), o["rv"].double().cpu(), t["gamma"], t["beta"], training=training, momentum=0.1, eps=1e-5)
        if use_res:
            y = y + o["res"].double().cpu()
        if relu:
            y = F.relu(y)
        y.backward(o["dy"].double().cpu())
        return dict(dx=t["x"].grad, dgamma=t["gamma"].grad, dbeta=t["beta"].grad)

    def check_grads(got, mode, with_dres, wrap, ref, y_saved, name):
        for k in ("dx", "dgamma", "dbeta"):
            if (mode, with_dres) == wrapper_calls:
                same_bytes(got[k], wrap[k], f"{name} mode {mode}: {k}")
            elif k == "dx" and name == "bn_bwd" and n * s <= 2:
                # one or two samples per channel (the edge shapes): dx = a * (g - mean(g) - xhat * mean(g * xhat)) cancels to (almost)
                # nothing, so the fp32 error is relative to the terms of that sum, a * max |dy|, not to the result
                terms = float((o["gamma"].abs() * save_invstd.abs()).max() * o["dy"].abs().max())
                err = float((got[k].double().cpu() - ref[k]).abs().max())
                assert err <= 1e-4 * terms, f"{name} mode {mode}: dx: max err {err:.3e} vs the terms' scale {terms:.3e}"
            else:
                T.close(got[k], ref[k], rtol=1e-4, what=f"{name} mode {mode}{', d_residual' if with_dres else ''}: {k}")
        if with_dres:
            masked = o["dy"] if not relu else torch.where(y_saved > 0, o["dy"], torch.zeros_like(o["dy"]))
            assert torch.equal(got["d_residual"], masked), f"{name}: d_residual is the masked dy"
            if use_res and relu:
                same_bytes(got["d_residual"], wrap["dres"], f"{name}: d_residual")

    ref_t = reference(True)
    for mode in modes:
        for with_dres in (False, True):
            outs = {"dx": (F32, shape), "dgamma": (F32, (c,)), "dbeta": (F32, (c,))}
            if with_dres:
                outs["d_residual"] = (F32, shape)
            got = contract(f"zsv_bn_bwd (relu mode {mode}{', d_residual' if with_dres else ''})",
                           lambda p: L.zsv_bn_bwd(p["dy"], p["x"], p["y"], n, c, s, p["gamma"], p["beta"], p["save_mean"], p["save_invstd"], mode,
                                                  p["dx"], p.get("d_residual"), p["dgamma"], p["dbeta"], p["ws"], nb, None), outs, {"ws": nb},
                           ins=dict(pick(o, "dy", "x", "gamma", "beta"), y=y_fwd if mode == 1 else None, save_mean=save_mean, save_invstd=save_invstd))
            check_grads(got, mode, with_dres, wt, ref_t, y_fwd, "bn_bwd")

    # ---- frozen statistics: forward and backward ----
    we = wrapper(False)
    ye = contract("zsv_bn_fwd_eval", lambda p: L.zsv_bn_fwd_eval(p["x"], n, c, s, p["gamma"], p["beta"], p["rm"], p["rv"], p["res"], r, 1e-5, p["y"],
                                                                 p["ws"], nb, None),
                  {"y": (F32, shape)}, {"ws": nb}, ins=dict(fwd_ins, **pick(o, "rm", "rv")))["y"]
    same_bytes(ye, we["y"], "bn_fwd_eval: y")
    ref_e = reference(False)
    for mode in modes:
        for with_dres in (False, True):
            outs = {"dx": (F32, shape), "dgamma": (F32, (c,)), "dbeta": (F32, (c,))}
            if with_dres:
                outs["d_residual"] = (F32, shape)
            got = contract(f"zsv_bn_bwd_eval (relu mode {mode}{', d_residual' if with_dres else ''})",
                           lambda p: L.zsv_bn_bwd_eval(p["dy"], p["x"], p["y"], n, c, s, p["gamma"], p["beta"], p["rm"], p["rv"], 1e-5, mode,
                                                       p["dx"], p.get("d_residual"), p["dgamma"], p["dbeta"], p["ws"], nb, None), outs, {"ws": nb},
                           ins=dict(pick(o, "dy", "x", "gamma", "beta", "rm", "rv"), y=ye if mode == 1 else None))
            check_grads(got, mode, with_dres, we, ref_e, ye, "bn_bwd_eval")
    ROWS_RUN[("BN_CASES", "bn")].add(shape)


# =========================================================================================================================
# dense head and nearest class
# =========================================================================================================================
@pytest.mark.parametrize("rows,fin,fout,relu", params_of(T.test_linear))
def test_linear_entry_points(rows, fin, fout, relu):
    L = lib()
    g = torch.Generator().manual_seed(rows + fin)
    x, w, b, dy = (t.to(DEV) for t in (torch.randn(rows, fin, generator=g), torch.randn(fout, fin, generator=g) / np.sqrt(fin),
                                       torch.randn(fout, generator=g), torch.randn(rows, fout, generator=g)))
    with torch.no_grad():
        yw = ops.linear(x, w, b, relu=relu)
    xg2, wg2 = x.clone().requires_grad_(), w.clone().requires_grad_()
    ops.linear(xg2, wg2, None).backward(dy)                               # plain: dy reaches dgrad / wgrad unmasked
    torch.cuda.synchronize()
    nf, nd, nw = (int(f(rows, fin, fout)) for f in (L.zsv_linear_fwd_workspace_bytes, L.zsv_linear_dgrad_workspace_bytes, L.zsv_linear_wgrad_workspace_bytes))
    y = contract("zsv_linear_fwd", lambda p: L.zsv_linear_fwd(p["x"], p["w"], p["bias"], p["y"], rows, fin, fout, 1 if relu else 0,
                                                              p["ws"], nf, None), {"y": (F32, (rows, fout))}, {"ws": nf}, shifted=True,
                 ins=dict(x=x, w=w, bias=b))["y"]
    same_bytes(y, yw.detach(), "linear_fwd")
    dx = contract("zsv_linear_dgrad", lambda p: L.zsv_linear_dgrad(p["dy"], p["w"], p["dx"], rows, fin, fout, p["ws"], nd, None),
                  {"dx": (F32, (rows, fin))}, {"ws": nd}, shifted=True, ins=dict(dy=dy, w=w))["dx"]
    same_bytes(dx, xg2.grad, "linear_dgrad")
    dw = contract("zsv_linear_wgrad", lambda p: L.zsv_linear_wgrad(p["x"], p["dy"], p["dw"], rows, fin, fout, p["ws"], nw, None),
                  {"dw": (F32, (fout, fin))}, {"ws": nw}, shifted=True, ins=dict(x=x, dy=dy))["dw"]
    same_bytes(dw, wg2.grad, "linear_wgrad")
    ROWS_RUN[("test_linear", "linear")].add((rows, fin, fout))


@pytest.mark.parametrize("rows,n_classes,dim,k", params_of(TA.test_cosine_topk_c_abi_against_scipy))
def test_cosine_topk(rows, n_classes, dim, k):
    """The workspace is the (rows, n_classes rounded up to 16) double distance matrix: the top-k must not look at its pad columns."""
    L = lib()
    g = torch.Generator().manual_seed(rows * 1000 + n_classes)
    e, c = torch.randn(rows, dim, generator=g) * 3.0, torch.randn(n_classes, dim, generator=g)
    if n_classes > 8:
        c[7] = c[2]
    e, c = e.to(DEV), c.to(DEV)
    nb = int(L.zsv_cosine_topk_workspace_bytes(rows, n_classes))
    out = contract("zsv_cosine_topk", lambda p: L.zsv_cosine_topk(p["embed"], p["class_embed"], rows, dim, n_classes, k, p["out_index"], p["out_dist"],
                                                                  p["ws"], nb, None),
                   {"out_index": (I32, (rows, k)), "out_dist": (F64, (rows, k))}, {"ws": nb}, ins=dict(embed=e, class_embed=c))
    assert torch.equal(out["out_index"].long(), train.nearest_classes(e, c, k))
    out2 = contract("zsv_cosine_topk (no distances)", lambda p: L.zsv_cosine_topk(p["embed"], p["class_embed"], rows, dim, n_classes, k, p["out_index"], None,
                                                                                 p["ws"], nb, None), {"out_index": (I32, (rows, k))}, {"ws": nb},
                    ins=dict(embed=e, class_embed=c))
    same_bytes(out2["out_index"], out["out_index"], "cosine_topk without distances")
    ec, cc = e.double().cpu(), c.double().cpu()
    full = 1 - (ec @ cc.t()) / (ec.norm(dim=1, keepdim=True) * cc.norm(dim=1).view(1, -1))
    assert float((out["out_dist"].cpu() - full.gather(1, out["out_index"].long().cpu())).abs().max()) < 1e-13
    ROWS_RUN[("test_cosine_topk", "topk")].add((rows, n_classes, dim, k))


# =========================================================================================================================
# bf16 / fp8 path
# =========================================================================================================================
def _cl_random(shape5, channels, g, scale=1.0):
    """[N][T][H][W][Cp] fp32 values on the host, pad channels zero."""
    t = torch.randn(shape5, generator=g) * scale
    t[..., channels:] = 0
    return t


def _bf16_forward_operands(case):
    g = torch.Generator().manual_seed(zlib.crc32(("contract" + case.name).encode()))
    geo = BX._geometry(case.cin, case.cout, case.kernel, case.stride, case.padding)
    t, h, w = case.thw
    if geo.folded:
        xb, wo = geo.clip_input(torch.randn((case.n, case.cin) + case.thw, generator=g).to(DEV))
        d = geo.desc(case.n, t, xb.shape[2], xb.shape[3], wo)
    else:
        d = geo.desc(case.n, t, h, w)
        cp = inference.channel_pitch(case.cin)
        xb = _cl_random((case.n, t, h, w, cp), case.cin, g).to(DEV).to(BF16)
    k = case.cin * numel(case.kernel)
    wgt = (torch.randn((case.cout, case.cin) + case.kernel, generator=g) / np.sqrt(k)).to(DEV)
    scale, shift = (torch.rand(case.cout, generator=g) + 0.5).to(DEV), torch.randn(case.cout, generator=g).to(DEV)
    ys = (d.N, d.To, d.Ho, d.Wo, inference.channel_pitch(case.cout))
    return d, xb, wgt, scale, shift, ys, g


@pytest.mark.parametrize("case", X.FORWARD_CASES, ids=[c.name for c in X.FORWARD_CASES])
def test_bf16_blob_and_forward(case, monkeypatch):
    L = lib()
    d, xb, wgt, scale, shift, ys, g = _bf16_forward_operands(case)
    rb = _cl_random(ys, case.cout, g).to(DEV).to(BF16) if case.residual else None
    nb = int(L.zsv_conv3d_bf16_blob_bytes(byref(d)))
    assert nb > 0
    for knob in BX._routes(case):
        if knob:
            monkeypatch.setenv(knob, "1")
        y = contract("zsv_conv3d_bf16_pack + zsv_conv3d_bf16_fwd",
                     lambda p: [L.zsv_conv3d_bf16_pack(byref(d), p["w"], p["scale"], p["shift"], p["blob"], None),
                                L.zsv_conv3d_bf16_fwd(byref(d), p["x"], p["blob"], p["residual"], 1 if case.relu else 0, p["y"], None)],
                     {"y": (BF16, ys)}, {"blob": nb}, ins=dict(w=wgt, scale=scale, shift=shift, x=xb, residual=rb))["y"]
        same_bytes(y, inference.conv_bf16(d, xb, inference.pack_conv(d, wgt, scale, shift), rb, case.relu), f"{case.name} {knob or ''}: y")
        assert int(torch.count_nonzero(y[..., case.cout:].float())) == 0, "pad channels must be written as zero"
        if knob:
            monkeypatch.delenv(knob)
    ROWS_RUN[("FORWARD_CASES", "bf16_fwd")].add(case.name)


@pytest.mark.parametrize("case", X.STATS_CASES, ids=[c.name for c in X.STATS_CASES])
def test_bf16_statistics_epilogue(case):
    L = lib()
    fc = X.FwdCase(case.name, case.n, case.cin, case.cout, case.thw, case.kernel, case.stride, case.padding, False, False)
    d, xb, wgt, _, _, ys, g = _bf16_forward_operands(fc)
    nb = int(L.zsv_conv3d_bf16_blob_bytes(byref(d)))
    cap = int(L.zsv_conv3d_bf16_stat_rows(byref(d)))
    assert nb > 0 and cap > 0
    cp = ys[-1]
    rows = ctypes.c_int32(0)

    def launch(p):
        rows.value = 0
        return [L.zsv_conv3d_bf16_pack(byref(d), p["w"], None, None, p["blob"], None),
                L.zsv_conv3d_bf16_fwd_stats(byref(d), p["x"], p["blob"], p["y"], p["bn_partials"], cap, byref(rows), None)]

    out = contract("zsv_conv3d_bf16_fwd_stats", launch, {"y": (BF16, ys), "bn_partials": (F32, (cap, 2, cp))}, {"blob": nb}, ins=dict(w=wgt, x=xb),
                   defined=lambda name, v: v[:rows.value] if name == "bn_partials" else v)
    assert 0 < rows.value <= cap
    z, partials, rows_w = amp.conv_bf16_stats(d, xb, amp.pack_conv(d, wgt, None, None))
    assert rows_w == rows.value
    same_bytes(out["y"], z, f"{case.name}: z")
    same_bytes(out["bn_partials"], partials[:rows_w], f"{case.name}: partials")
    ROWS_RUN[("STATS_CASES", "bf16_fwd_stats")].add(case.name)


@pytest.mark.parametrize("case", X.DGRAD_CASES, ids=[c.name for c in X.DGRAD_CASES])
def test_bf16_dgrad_blob_and_forward(case):
    """The input-gradient problems of a convolution exactly as amp.Bf16TrainPath._dgrad forms them (one per residue class of a
    strided convolution), each packed into a guarded blob of exactly its size."""
    L = lib()
    g = torch.Generator().manual_seed(zlib.crc32(("contract" + case.name).encode()))
    n, cin, t, h, w_ = case.xs
    _, u = BX._unit(case)
    d = u.desc(n, t, h, w_)
    cp = inference.channel_pitch(case.cout)
    dz = _cl_random((n, d.To, d.Ho, d.Wo, cp), case.cout, g).to(DEV).to(BF16)
    w = u.conv.weight.detach()
    axes = [amp.Bf16TrainPath._axis_classes(k, p, s, n_in, n_out) for k, p, s, n_in, n_out in
            zip(u.kernel, u.padding, u.stride, (d.Ti, d.Hi, d.Wi), (d.To, d.Ho, d.Wo))]
    st, sh, sw = u.stride
    problems = 0
    for ct in axes[0]:
        for ch in axes[1]:
            for cw in axes[2]:
                if ct[2] == 0 or ch[2] == 0 or cw[2] == 0:
                    continue
                sub = w[:, :, ct[1]::st, ch[1]::sh, cw[1]::sw].contiguous()
                kernel, pads = (ct[2], ch[2], cw[2]), (ct[3], ch[3], cw[3])
                if all(len(a) == 1 for a in axes):
                    dims = (d.Ti, d.Hi, d.Wi)
                else:
                    dims = tuple(n_out + 2 * c[3] - c[2] + 1 for c, n_out in zip((ct, ch, cw), (d.To, d.Ho, d.Wo)))
                d2 = _lib.ConvDesc(n, u.cout, d.To, d.Ho, d.Wo, u.cin, dims[0], dims[1], dims[2], kernel[0], kernel[1], kernel[2], 1, 1, 1, *pads)
                nb = int(L.zsv_conv3d_bf16_blob_bytes(byref(d2)))
                assert nb > 0
                ys = (n,) + dims + (inference.channel_pitch(u.cin),)
                y = contract("zsv_conv3d_bf16_pack_dgrad + zsv_conv3d_bf16_fwd",
                             lambda p: [L.zsv_conv3d_bf16_pack_dgrad(byref(d2), p["w_fwd"], p["blob"], None),
                                        L.zsv_conv3d_bf16_fwd(byref(d2), p["dz"], p["blob"], None, 0, p["y"], None)],
                             {"y": (BF16, ys)}, {"blob": nb}, count=problems == 0, ins=dict(w_fwd=sub, dz=dz))["y"]
                same_bytes(y, amp.Bf16TrainPath._dgrad_problem(u, dz, sub, kernel, pads, dims), f"{case.name}: class problem {kernel}")
                problems += 1
    assert problems > 0
    ROWS_RUN[("DGRAD_CASES", "bf16_pack_dgrad")].add(case.name)


@pytest.mark.parametrize("case", X.WGRAD_CASES, ids=[c.name for c in X.WGRAD_CASES])
def test_bf16_weight_gradient(case):
    L = lib()
    g = torch.Generator().manual_seed(zlib.crc32(("contract" + case.name).encode()))
    n, cin, t, h, w_ = case.xs
    _, u = BX._unit(case)
    d = u.desc(n, t, h, w_)
    x = _cl_random((n, t, h, w_, inference.channel_pitch(cin)), cin, g).to(DEV).to(BF16)
    dz = _cl_random((n, d.To, d.Ho, d.Wo, inference.channel_pitch(case.cout)), case.cout, g).to(DEV).to(BF16)
    nb = int(L.zsv_conv3d_bf16_wgrad_workspace_bytes(byref(d)))
    assert nb > 0, "the native kernel must take this geometry"
    ws = (case.cout, cin) + tuple(case.kernel)
    dw = contract("zsv_conv3d_bf16_wgrad", lambda p: L.zsv_conv3d_bf16_wgrad(byref(d), p["x"], p["dz"], p["dw"], p["ws"], nb, None),
                  {"dw": (F32, ws)}, {"ws": nb}, shifted=True, ins=dict(x=x, dz=dz))["dw"]
    rec = amp._Record()
    rec.unit, rec.desc, rec.x, rec.clips = u, d, x, None
    want = amp.Bf16TrainPath._wgrad(rec, dz)
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    same_bytes(dw, want, f"{case.name}: dW")
    ROWS_RUN[("WGRAD_CASES", "bf16_wgrad")].add(case.name)


BN_CL_CASES = params_of(BX.test_batchnorm_forward_is_the_arithmetic_its_header_states)


@pytest.mark.parametrize("shape,relu,res", BN_CL_CASES, ids=[f"{'x'.join(map(str, s))}{'_relu' if r else ''}{'_res' if q else ''}" for s, r, q in BN_CL_CASES])
def test_channels_last_batchnorm_entry_points(shape, relu, res):
    L = lib()
    n, c = shape[:2]
    g = torch.Generator().manual_seed(c * 11 + shape[2])
    cp = inference.channel_pitch(c)
    cl = (n,) + tuple(shape[2:]) + (cp,)
    z = (_cl_random(cl, c, g, 1.5) + 0.3 * (torch.arange(cp) < c)).to(DEV).to(BF16)
    rb = _cl_random(cl, c, g).to(DEV).to(BF16) if res else None
    dy = _cl_random(cl, c, g).to(DEV).to(BF16)
    bn = BX._bn(c, g)
    rows = numel(cl[:-1])
    nb = int(L.zsv_bn_cl_workspace_bytes(rows, c))
    assert nb > 0
    r = 1 if relu else 0
    fwd_ins = dict(z=z, residual=rb, gamma=bn.weight.detach(), beta=bn.bias.detach())
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()

    def fresh_bn():
        with torch.no_grad():
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
        return bn

    outs = {"y": (BF16, cl), "save_mean": (F32, (c,)), "save_invstd": (F32, (c,)), "save_coef": (F32, (2, cp)),
            "running_mean": (F32, (c,), rm0), "running_var": (F32, (c,), rv0)}
    out = contract("zsv_bn_cl_fwd_train",
                   lambda p: L.zsv_bn_cl_fwd_train(p["z"], p["residual"], rows, c, p["gamma"], p["beta"], p["running_mean"], p["running_var"], 0.1, bn.eps,
                                                   r, p["y"], p["save_mean"], p["save_invstd"], p["save_coef"], p["ws"], nb, None), outs, {"ws": nb},
                   ins=fwd_ins)
    yw, mean, invstd, coef = amp.bn_cl_fwd_train(z, fresh_bn(), rb, relu, want_coef=True)
    torch.cuda.synchronize()
    for name, want in (("y", yw), ("save_mean", mean), ("save_invstd", invstd), ("save_coef", coef), ("running_mean", bn.running_mean),
                       ("running_var", bn.running_var)):
        same_bytes(out[name], want.detach(), f"bn_cl_fwd_train: {name}")
    # the same from a convolution's epilogue partials: [rows][2][Cp], three row blocks over the voxels
    blocks = min(3, rows)
    cuts = [rows * i // blocks for i in range(blocks + 1)]
    zf = z.reshape(rows, cp).float()
    partials = torch.stack([torch.stack([zf[a:b].sum(0), (zf[a:b] ** 2).sum(0)]) for a, b in zip(cuts, cuts[1:])]).contiguous()
    out2 = contract("zsv_bn_cl_fwd_train_stats",
                    lambda p: L.zsv_bn_cl_fwd_train_stats(p["z"], p["residual"], rows, c, p["gamma"], p["beta"], p["running_mean"], p["running_var"], 0.1,
                                                          bn.eps, r, p["y"], p["save_mean"], p["save_invstd"], p["save_coef"], p["conv_partials"], blocks,
                                                          p["ws"], nb, None), outs, {"ws": nb}, ins=dict(fwd_ins, conv_partials=partials))
    yw2, mean2, invstd2, coef2 = amp.bn_cl_fwd_train(z, fresh_bn(), rb, relu, want_coef=True, conv_stats=(partials, blocks))
    torch.cuda.synchronize()
    for name, want in (("y", yw2), ("save_mean", mean2), ("save_invstd", invstd2), ("save_coef", coef2), ("running_var", bn.running_var)):
        same_bytes(out2[name], want.detach(), f"bn_cl_fwd_train_stats: {name}")

    # ---- backward: the mask from the saved output, and (no residual) recomputed from z ----
    grads = {"dz": (BF16, cl), "g_out": (BF16, cl), "dgamma": (F32, (c,)), "dbeta": (F32, (c,))}
    y_saved = out["y"]
    forms = [False] + ([True] if (relu and not res) else [])
    for recompute in forms:
        o = contract("zsv_bn_cl_bwd" + (" (mask recomputed from z)" if recompute else ""),
                     lambda p: L.zsv_bn_cl_bwd(p["dy"], p["y"], p["z"], rows, c, p["gamma"], p["save_mean"], p["save_invstd"], p["fwd_coef"], r, p["dz"],
                                               p["g_out"], p["dgamma"], p["dbeta"], p["ws"], nb, None), grads, {"ws": nb},
                     ins=dict(dy=dy, y=y_saved if (relu and not recompute) else None, z=z, gamma=bn.weight.detach(), save_mean=mean, save_invstd=invstd,
                              fwd_coef=coef if recompute else None))
        dzw, gw, dgw, dbw = amp.bn_cl_bwd(dy, yw, z, bn, mean, invstd, relu, want_g=True, fwd_coef=coef if recompute else None)
        torch.cuda.synchronize()
        for name, want in (("dz", dzw), ("g_out", gw), ("dgamma", dgw), ("dbeta", dbw)):
            same_bytes(o[name], want, f"bn_cl_bwd: {name}")
    # ---- frozen statistics ----
    ye, coef4 = amp.bn_cl_fwd_eval(z, bn.eval(), rb, relu)
    for use_y in ([True, False] if relu else [False]):
        if relu and not use_y and res:
            continue                                       # (the recomputed mask is the forward's only without a residual)
        o = contract("zsv_bn_cl_bwd_eval" + ("" if use_y or not relu else " (mask recomputed from z)"),
                     lambda p: L.zsv_bn_cl_bwd_eval(p["dy"], p["y"], p["z"], rows, c, p["coef"], r, p["dz"], p["g_out"], p["dgamma"], p["dbeta"],
                                                    p["ws"], nb, None), grads, {"ws": nb}, ins=dict(dy=dy, y=ye if use_y else None, z=z, coef=coef4))
        dzw, gw, dgw, dbw = amp.bn_cl_bwd_eval(dy, ye if use_y else None, z, bn, coef4, relu, want_g=True)
        torch.cuda.synchronize()
        for name, want in (("dz", dzw), ("g_out", gw), ("dgamma", dgw), ("dbeta", dbw)):
            same_bytes(o[name], want, f"bn_cl_bwd_eval: {name}")
    bn.train()
    # ---- C3D's relu(conv + bias) backward on the same tensors ----
    o = contract("zsv_relu_bias_bwd_cl", lambda p: L.zsv_relu_bias_bwd_cl(p["dy"], p["y"], rows, c, p["g_out"], p["dbias"], p["ws"], nb, None),
                 {"g_out": (BF16, cl), "dbias": (F32, (c,))}, {"ws": nb}, ins=dict(dy=dy, y=y_saved))
    gw, dbw = amp.relu_bias_bwd_cl(dy, y_saved, c)
    torch.cuda.synchronize()
    same_bytes(o["g_out"], gw, "relu_bias_bwd_cl: g")
    same_bytes(o["dbias"], dbw, "relu_bias_bwd_cl: dbias")
    ROWS_RUN[("bn_cl", "bn_cl")].add((tuple(shape), relu, res))


@pytest.mark.parametrize("case", F8.CASES, ids=[f"c{i}" for i in range(len(F8.CASES))])
def test_fp8_blob_and_forward(case):
    L = lib()
    n, cin, cout, thw, k, s, p, use_res, relu = case
    t, h, w = thw
    g = torch.Generator().manual_seed(zlib.crc32(str(case).encode()))
    wgt = (torch.randn((cout, cin) + k, generator=g) / np.sqrt(cin * numel(k))).to(DEV)
    shift = (torch.randn(cout, generator=g) * 8.0).to(DEV)
    d = ops.conv_desc((n, cin, t, h, w), wgt.shape, s, p)
    ys = (d.N, d.To, d.Ho, d.Wo, inference.fp8_channel_pitch(cout))

    def e4m3_cl(shape5, channels, scale):
        v = _cl_random(shape5, channels, g, scale).clamp(-448.0, 448.0).to(F8.FP8)
        return v.view(U8).to(DEV).view(F8.FP8)

    xb = e4m3_cl((n, t, h, w, inference.fp8_channel_pitch(cin)), cin, 4.0)
    rb = e4m3_cl(ys, cout, 8.0) if use_res else None
    nb = int(L.zsv_conv3d_fp8_blob_bytes(byref(d)))
    assert nb > 0
    y = contract("zsv_conv3d_fp8_pack + zsv_conv3d_fp8_fwd",
                 lambda q: [L.zsv_conv3d_fp8_pack(byref(d), q["w"], None, q["shift"], q["blob"], None),
                            L.zsv_conv3d_fp8_fwd(byref(d), q["x"], q["blob"], q["residual"], 1 if relu else 0, q["y"], None)],
                 {"y": (U8, ys)}, {"blob": nb}, ins=dict(w=wgt, shift=shift, x=xb, residual=rb), aligned={"y"})["y"]
    want = inference.conv_fp8(d, xb, inference.pack_conv_fp8(d, wgt, None, shift), rb, relu)
    same_bytes(y, want.view(U8), "conv_fp8: y")
    assert int(torch.count_nonzero(y[..., cout:])) == 0, "pad channels must be written as zero"
    ROWS_RUN[("fp8 CASES", "fp8_fwd")].add(case)


# =========================================================================================================================
# entry points without a workspace: element-wise passes, pools, layout converters, the optimiser, clip pre-processing
# =========================================================================================================================
ELEMENTWISE_SHAPES = [(3, 5, 2, 7, 7), (1, 1, 1, 1, 3), (2, 4, 4, 8, 8)]            # test_relu_add_relu_meanpool


@pytest.mark.parametrize("shape", ELEMENTWISE_SHAPES, ids=["x".join(map(str, s)) for s in ELEMENTWISE_SHAPES])
def test_elementwise_and_mean_pool(shape):
    L = lib()
    g = torch.Generator().manual_seed(2 + sum(shape))
    a, b, dy = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
    n, c = shape[:2]
    s = numel(shape[2:])
    count = numel(shape)
    ag = a.clone().requires_grad_()
    yw = ops.relu(ag)
    yw.backward(dy)
    y = contract("zsv_relu_fwd", lambda p: L.zsv_relu_fwd(p["x"], p["y"], count, None), {"y": (F32, shape)}, ins=dict(x=a))["y"]
    same_bytes(y, yw.detach(), "relu_fwd")
    dx = contract("zsv_relu_bwd", lambda p: L.zsv_relu_bwd(p["dy"], p["y"], p["dx"], count, None), {"dx": (F32, shape)}, ins=dict(dy=dy, y=y))["dx"]
    same_bytes(dx, ag.grad, "relu_bwd")
    with torch.no_grad():
        sw = ops.add_relu(a, b)
    out = contract("zsv_add_relu_fwd", lambda p: L.zsv_add_relu_fwd(p["a"], p["b"], p["y"], count, None), {"y": (F32, shape)}, ins=dict(a=a, b=b))["y"]
    same_bytes(out, sw, "add_relu_fwd")
    dm = torch.randn((n, c), generator=g).to(DEV)
    ag = a.clone().requires_grad_()
    mw = ops.mean_pool(ag)
    mw.backward(dm)
    m = contract("zsv_meanpool_fwd", lambda p: L.zsv_meanpool_fwd(p["x"], n, c, s, p["y"], None), {"y": (F32, (n, c))}, ins=dict(x=a))["y"]
    same_bytes(m, mw.detach(), "meanpool_fwd")
    dxm = contract("zsv_meanpool_bwd", lambda p: L.zsv_meanpool_bwd(p["dy"], n, c, s, p["dx"], None), {"dx": (F32, shape)}, ins=dict(dy=dm))["dx"]
    same_bytes(dxm, ag.grad, "meanpool_bwd")
    ROWS_RUN[("elementwise", "elementwise")].add(shape)


def _pool_geometry(shape, k, p):
    n, c, ti, hi, wi = shape
    to, ho, wo = ((v + 2 * q - w) // w + 1 for v, q, w in zip((ti, hi, wi), p, k))
    return (n, c, ti, hi, wi) + tuple(k) + tuple(p) + (to, ho, wo), (to, ho, wo)


@pytest.mark.parametrize("k,p,shape", T.POOL_CASES, ids=[f"k{k[0]}{k[1]}{k[2]}_p{p[0]}{p[1]}{p[2]}_{'x'.join(map(str, s))}" for k, p, s in T.POOL_CASES])
def test_max_pool_fp32(k, p, shape):
    L = lib()
    g = torch.Generator().manual_seed(sum(shape))
    x = F.relu(torch.randn(*shape, generator=g)).to(DEV)            # ties at 0 like post-ReLU activations
    geom, (to, ho, wo) = _pool_geometry(shape, k, p)
    ys = shape[:2] + (to, ho, wo)
    dy = torch.randn(ys, generator=g).to(DEV)
    xg = x.clone().requires_grad_()
    yw = ops.max_pool3d(xg, k, k, p)
    yw.backward(dy)
    out = contract("zsv_maxpool3d_fwd", lambda q: L.zsv_maxpool3d_fwd(q["x"], *geom, q["y"], q["argmax"], None),
                   {"y": (F32, ys), "argmax": (I32, ys)}, ins=dict(x=x))
    same_bytes(out["y"], yw.detach(), "maxpool3d_fwd")
    arg = out["argmax"].long()
    assert int(arg.min()) >= 0 and int(arg.max()) < numel(shape[2:])
    assert torch.equal(x.flatten(2).gather(2, arg.flatten(2)).view(ys), out["y"]), "argmax names the element the maximum was taken from"
    dx = contract("zsv_maxpool3d_bwd", lambda q: L.zsv_maxpool3d_bwd(q["dy"], q["argmax"], *geom, q["dx"], None), {"dx": (F32, shape)},
                  ins=dict(dy=dy, argmax=out["argmax"]))["dx"]
    same_bytes(dx, xg.grad, "maxpool3d_bwd")
    ROWS_RUN[("POOL_CASES", "maxpool")].add((k, p, shape))


CL_POOL_CASES = params_of(TB.test_maxpool3d_channels_last_bf16)


@pytest.mark.parametrize("shape,kernel,pad", CL_POOL_CASES, ids=["x".join(map(str, s)) for s, _, _ in CL_POOL_CASES])
def test_channels_last_pools(shape, kernel, pad):
    L = lib()
    g = torch.Generator().manual_seed(sum(shape))
    n, c, t, h, w = shape
    geom, (to, ho, wo) = _pool_geometry(shape, kernel, pad)
    s = t * h * w
    # ---- bf16 ----
    cp = inference.channel_pitch(c)
    x = _cl_random((n, t, h, w, cp), c, g).to(DEV).to(BF16)
    dy = _cl_random((n, to, ho, wo, cp), c, g).to(DEV).to(BF16)
    y = contract("zsv_maxpool3d_bf16", lambda q: L.zsv_maxpool3d_bf16(q["x"], *geom, q["y"], None), {"y": (BF16, (n, to, ho, wo, cp))}, ins=dict(x=x))["y"]
    same_bytes(y, inference.maxpool3d_bf16(x, c, kernel, pad), "maxpool3d_bf16")
    dx = contract("zsv_maxpool3d_bf16_bwd", lambda q: L.zsv_maxpool3d_bf16_bwd(q["dy"], q["x"], *geom, q["dx"], None), {"dx": (BF16, tuple(x.shape))},
                  ins=dict(dy=dy, x=x))["dx"]
    same_bytes(dx, amp.maxpool3d_bf16_bwd(dy, x, c, kernel, pad), "maxpool3d_bf16_bwd")
    m = contract("zsv_meanpool_bf16", lambda q: L.zsv_meanpool_bf16(q["x"], n, s, c, q["out"], None), {"out": (F32, (n, c))}, ins=dict(x=x))["out"]
    same_bytes(m, inference.meanpool_bf16(x, c), "meanpool_bf16")
    dp = torch.randn((n, c), generator=g).to(DEV)
    dxm = contract("zsv_meanpool_bf16_bwd", lambda q: L.zsv_meanpool_bf16_bwd(q["dpooled"], n, s, c, q["dx"], None), {"dx": (BF16, tuple(x.shape))},
                   ins=dict(dpooled=dp))["dx"]
    same_bytes(dxm, amp.meanpool_bf16_bwd(dp, x, c), "meanpool_bf16_bwd")
    # ---- e4m3: finite codes of both signs; the input's pad channels hold a non-zero code (test_maxpool3d_channels_last_fp8) ----
    cp8 = inference.fp8_channel_pitch(c)
    codes = torch.full((n, t, h, w, cp8), 0x55, dtype=U8)
    codes[..., :c] = (torch.randn((n, t, h, w, c), generator=g) * 40.0).clamp(-448.0, 448.0).to(F8.FP8).view(U8)
    x8 = codes.to(DEV).view(F8.FP8)
    y8 = contract("zsv_maxpool3d_fp8", lambda q: L.zsv_maxpool3d_fp8(q["x"], *geom, q["y"], None), {"y": (U8, (n, to, ho, wo, cp8))}, ins=dict(x=x8), aligned={"y"})["y"]
    same_bytes(y8, inference.maxpool3d_fp8(x8, c, kernel, pad).view(U8), "maxpool3d_fp8")
    m8 = contract("zsv_meanpool_fp8", lambda q: L.zsv_meanpool_fp8(q["x"], n, s, c, q["out"], None), {"out": (F32, (n, c))}, ins=dict(x=x8))["out"]
    same_bytes(m8, inference.meanpool_fp8(x8, c), "meanpool_fp8")
    ROWS_RUN[("CL_POOL_CASES", "cl_pools")].add(shape)


CONVERTER_SHAPES = list(params_of(TAMP.test_layout_converters_round_trip))


@pytest.mark.parametrize("shape", CONVERTER_SHAPES, ids=["x".join(map(str, s)) for s in CONVERTER_SHAPES])
def test_layout_converters(shape):
    L = lib()
    g = torch.Generator().manual_seed(sum(shape))
    n, c, t, h, w = shape
    s, cp = t * h * w, inference.channel_pitch(c)
    x = torch.randn(shape, generator=g).to(DEV)
    cl = contract("zsv_ncs_f32_to_cl_bf16", lambda q: L.zsv_ncs_f32_to_cl_bf16(q["x"], n, s, c, q["out"], None), {"out": (BF16, (n, t, h, w, cp))},
                  ins=dict(x=x))["out"]
    same_bytes(cl, amp.ncdhw_to_cl_bf16(x), "ncs_f32_to_cl_bf16")
    back = contract("zsv_cl_bf16_to_ncs_f32", lambda q: L.zsv_cl_bf16_to_ncs_f32(q["x"], n, s, c, q["out"], None), {"out": (F32, shape)}, ins=dict(x=cl))["out"]
    same_bytes(back, amp.cl_to_ncdhw_f32(cl, c), "cl_bf16_to_ncs_f32")
    assert torch.equal(back, x.to(BF16).float())
    ROWS_RUN[("converters", "converters")].add(shape)


# (N, C, T, H, W), (padH, padW), (Hp, Wp): C = 3 and fewer, a border on every side, Hp / Wp beyond the frame + its offset
CLIP_CASES = [((2, 3, 2, 9, 11), (3, 3), (15, 24)), ((1, 3, 1, 5, 7), (1, 2), (6, 9)), ((1, 1, 3, 4, 5), (0, 0), (4, 8)), ((3, 2, 1, 1, 1), (2, 0), (5, 1))]


@pytest.mark.parametrize("shape,pads,padded", CLIP_CASES, ids=["x".join(map(str, c[0])) for c in CLIP_CASES])
def test_clip_to_bf16(shape, pads, padded):
    L = lib()
    g = torch.Generator().manual_seed(sum(shape))
    n, c, t, h, w = shape
    x = torch.randn(shape, generator=g).to(DEV)
    out = contract("zsv_clip_to_bf16", lambda q: L.zsv_clip_to_bf16(q["x"], n, c, t, h, w, pads[0], pads[1], padded[0], padded[1], q["out"], None),
                   {"out": (BF16, (n, t) + padded + (4,))}, ins=dict(x=x))["out"]
    same_bytes(out, inference.clip_to_bf16(x, pads[0], pads[1], padded[0], padded[1]), "clip_to_bf16")
    want = torch.zeros((n, t) + padded + (4,), device=DEV)
    want[:, :, pads[0]:pads[0] + h, pads[1]:pads[1] + w, :c] = x.permute(0, 2, 3, 4, 1)
    assert torch.equal(out, want.to(BF16)), "the frame at (padH, padW) inside a zero border"
    ROWS_RUN[("CLIP_CASES", "clip_to_bf16")].add(shape)


@pytest.mark.parametrize("shift", [0, 2, 14])
@pytest.mark.parametrize("count", [1, 255, 4 * 256 + 3])
def test_absmax_bf16(count, shift):
    """The head / 16-byte-aligned body / tail split starts at the input's address: the input begins 0, 2 and 14 bytes past a
    16-byte boundary.  The result is a maximum, so the 0x7F band is the run that matters (|NaN| wins the integer maximum too)."""
    L = lib()
    g = torch.Generator().manual_seed(count)
    x = torch.randn(count, generator=g).to(BF16).to(DEV)
    want = x.float().abs().max().reshape(1)
    for start in (0.0, 1e4):                            # folds into what *amax holds
        out = contract("zsv_absmax_bf16", lambda q: L.zsv_absmax_bf16(q["x"], count, q["amax"], None),
                       {"amax": (F32, (1,), torch.full((1,), start, device=DEV))}, ins=dict(x=(x, shift)), count=start == 0.0)["amax"]
        same_bytes(out, torch.maximum(want, torch.full((1,), start, device=DEV)), f"absmax_bf16 from {start}")
    amax = torch.zeros(1, device=DEV)
    inference.absmax_bf16(x, amax)
    assert torch.equal(amax, want)
    ROWS_RUN[("absmax", "absmax")].add((count, shift))


@pytest.mark.parametrize("c", [1, 3, 64, 260])
def test_bn_eval_coeffs(c):
    L = lib()
    o = _bn_operands((2, c, 1, 1, 1))
    pitch = (c + 15) // 16 * 16
    coef = contract("zsv_bn_eval_coeffs", lambda p: L.zsv_bn_eval_coeffs(c, p["gamma"], p["beta"], p["rm"], p["rv"], 1e-5, p["coef"], pitch, None),
                    {"coef": (F32, (2, pitch))}, ins=pick(o, "gamma", "beta", "rm", "rv"), aligned={"coef"})["coef"]
    _, coef_w = ops._BatchNormFrozenDeferred.apply(o["x"], o["gamma"], o["beta"], o["rm"], o["rv"], 1e-5)
    same_bytes(coef, coef_w, "bn_eval_coeffs")
    assert int(torch.count_nonzero(coef[:, c:])) == 0, "coef entries C .. coef_pitch-1 must be zero"
    a = o["gamma"].double() / torch.sqrt(o["rv"].double() + 1e-5)
    T.close(coef[0, :c], a, rtol=1e-6, what="scale")
    T.close(coef[1, :c], o["beta"].double() - o["rm"].double() * a, rtol=1e-6, what="shift")
    ROWS_RUN[("bn_eval_coeffs", "bn_eval_coeffs")].add(c)


@pytest.mark.parametrize("n", [1, 1000, 4099])         # (1000: test_adam_step_matches_torch)
def test_adam_step(n):
    L = lib()
    g = torch.Generator().manual_seed(4 + n)
    p0, grad, m0 = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    v0 = torch.rand(n, generator=g).to(DEV)
    out = contract("zsv_adam_step", lambda q: L.zsv_adam_step(q["p"], q["g"], q["exp_avg"], q["exp_avg_sq"], n, 1e-3, 0.9, 0.999, 1e-8, 3, None),
                   {"p": (F32, (n,), p0), "exp_avg": (F32, (n,), m0), "exp_avg_sq": (F32, (n,), v0)}, ins=dict(g=grad))
    pw, mw, vw = p0.clone(), m0.clone(), v0.clone()
    ops.adam_step_(pw, grad, mw, vw, 3, 1e-3)
    for name, want in (("p", pw), ("exp_avg", mw), ("exp_avg_sq", vw)):
        same_bytes(out[name], want, f"adam_step: {name}")
    ROWS_RUN[("adam_step", "adam_step")].add(n)


# ---- clip pre-processing: every video / image is a guarded uint8 buffer of its own, the device tables point into them ----
# crop 16 (short side resized to 256): the smallest frames of test_clip_batch_gpu.py / test_still_image_gpu.py.  (top, left, flip)
# per video: the four corners of the resized frame -- every frame edge, both flips, the bottom-right corner -- and the centre.
VIDEO_SIZES = [(40, 50), (41, 53), (50, 40)]


def _corner_params(sizes, crop, size):
    res = [preprocess.resized_hw(h, w, size)[:2] for h, w in sizes]
    corners = [lambda r: (0, 0, 0), lambda r: (r[0] - crop, r[1] - crop, 1), lambda r: (0, r[1] - crop, 1), lambda r: (r[0] - crop, 0, 0),
               lambda r: ((r[0] - crop) // 2, (r[1] - crop) // 2, 1)]
    return res, [[f(r) for r in res] for f in corners]


def test_clip_transform_one_size():
    L = lib()
    crop, n, t = 16, 5, 2
    clips = preprocess.ClipTransform(False, crop)
    for h, w in VIDEO_SIZES[:2]:
        frames = torch.randint(0, 256, (n, t, h, w, 3), dtype=U8, generator=torch.Generator().manual_seed(h * w)).to(DEV)
        hres, wres, inv_scale = preprocess.resized_hw(h, w, clips.size)
        _, rounds = _corner_params([(h, w)], crop, clips.size)
        params = [r[0] for r in rounds]                             # one corner per clip
        out = contract("zsv_clip_transform",
                       lambda p: L.zsv_clip_transform(p["frames"], n, t, h, w, hres, wres, float(inv_scale), crop, p["params"], p["out"], None),
                       {"out": (F32, (n, 3, t, crop, crop))}, ins=dict(frames=frames, params=torch.tensor(params, dtype=I32).to(DEV)))["out"]
        same_bytes(out, clips(frames, params), f"clip_transform {h}x{w}")
        ROWS_RUN[("clip_transform", "clip_transform")].add((h, w))


def test_clip_transform_batch():
    L = lib()
    crop, nc, t = 16, 2, 2
    clips = preprocess.VideoClips(False, n_clips=nc, clip_len=t, crop_size=crop)
    g = torch.Generator().manual_seed(11)
    videos = [torch.randint(0, 256, (nc * t, h, w, 3), dtype=U8, generator=g).to(DEV) for h, w in VIDEO_SIZES]
    _, rounds = _corner_params(VIDEO_SIZES, crop, clips.size)
    names = [f"video{b}" for b in range(len(videos))]
    for i, params in enumerate(rounds):
        out = contract("zsv_clip_transform_batch",
                       lambda p: L.zsv_clip_transform_batch(p["table"](torch.from_numpy(preprocess.video_table([p[k] for k in names], VIDEO_SIZES, params,
                                                                                                                 clips.size)), "video table"),
                                                            len(videos), nc, t, crop, p["out"], None),
                       {"out": (F32, (len(videos), nc, 3, t, crop, crop))}, ins=dict(zip(names, videos)), count=i == 0)["out"]
        same_bytes(out, clips(videos, params), f"clip_transform_batch, windows {params}")
    ROWS_RUN[("clip_transform", "clip_transform_batch")].update(VIDEO_SIZES)


def test_still_image_clips():
    L = lib()
    crop, nc, t = 16, 1, 4
    sizes = [(40, 50), (41, 53), (130, 141)]
    clips = preprocess.StillImageClips(clip_len=t, n_clips=nc, crop_size=crop)
    images = [torch.randint(0, 256, (h, w, 3), dtype=U8, generator=torch.Generator().manual_seed(h + w)).to(DEV) for h, w in sizes]
    # (top, left, side) per frame: flush with the top-left and the bottom-right corner at the smallest and the largest side the
    # image and the kernel allow (crop <= side <= 8 * crop), the other two corners in between
    trajectories = []
    for h, w in sizes:
        big = min(h, w, 8 * crop)
        mid = (crop + big) // 2
        trajectories.append(np.array([[0, 0, big], [h - crop, w - crop, crop], [0, w - mid, mid], [h - big, w - big, big]]))
    names = [f"image{b}" for b in range(len(images))]
    ftab = torch.from_numpy(np.stack(trajectories).astype(np.int32)).to(DEV)
    max_side = int(max(tr[:, 2].max() for tr in trajectories))
    out = contract("zsv_still_image_clips",
                   lambda p: L.zsv_still_image_clips(p["table"](torch.tensor([[p[k], im.shape[0], im.shape[1]] for k, im in zip(names, images)],
                                                                             dtype=torch.int64), "image table"),
                                                     p["frames"], len(images), nc, t, crop, max_side, p["out"], None),
                   {"out": (F32, (len(images), nc, 3, t, crop, crop))}, ins=dict(zip(names, images), frames=ftab))["out"]
    same_bytes(out, clips(images, trajectories), "still_image_clips")
    ROWS_RUN[("still_image", "still_image_clips")].update(sizes)



# =========================================================================================================================
# nothing was skipped
# =========================================================================================================================
ENTRY_POINTS = [
    "zsv_conv3d_fwd_full", "zsv_conv3d_fwd_full (bias + ReLU)", "zsv_conv3d_fwd_full (residual)", "zsv_conv3d_fwd_full (statistics)",
    "zsv_conv3d_fwd_pre", "zsv_conv3d_dgrad", "zsv_conv3d_dgrad_add", "zsv_conv3d_dgrad_add_strided", "zsv_conv3d_wgrad", "zsv_conv3d_wgrad_masked",
    "zsv_conv3d_wgrad_pre", "zsv_pack_multi + zsv_conv3d_fwd_full_panel", "zsv_pack_multi + zsv_conv3d_dgrad_add_panel",
    "zsv_pack_multi + zsv_conv3d_fwd_pre_panel", "zsv_pack_multi + zsv_conv3d_dgrad_add_strided_panel",
    "zsv_channel_sum", "zsv_relu_bwd_bias", "zsv_bn_fwd_train", "zsv_bn_fwd_train_stats", "zsv_bn_fwd_train_coeffs", "zsv_bn_fwd_eval",
    "zsv_bn_bwd (relu mode 0)", "zsv_bn_bwd (relu mode 0, d_residual)", "zsv_bn_bwd (relu mode 1)", "zsv_bn_bwd (relu mode 1, d_residual)",
    "zsv_bn_bwd (relu mode 2)", "zsv_bn_bwd (relu mode 2, d_residual)", "zsv_bn_bwd_eval (relu mode 0)", "zsv_bn_bwd_eval (relu mode 0, d_residual)",
    "zsv_bn_bwd_eval (relu mode 1)", "zsv_bn_bwd_eval (relu mode 1, d_residual)", "zsv_bn_bwd_eval (relu mode 2)",
    "zsv_bn_bwd_eval (relu mode 2, d_residual)", "zsv_linear_fwd", "zsv_linear_dgrad", "zsv_linear_wgrad", "zsv_cosine_topk", "zsv_cosine_topk (no distances)",
    "zsv_conv3d_bf16_pack + zsv_conv3d_bf16_fwd", "zsv_conv3d_bf16_pack_dgrad + zsv_conv3d_bf16_fwd", "zsv_conv3d_fp8_pack + zsv_conv3d_fp8_fwd",
    "zsv_conv3d_bf16_fwd_stats", "zsv_bn_cl_fwd_train", "zsv_bn_cl_fwd_train_stats", "zsv_bn_cl_bwd", "zsv_bn_cl_bwd (mask recomputed from z)",
    "zsv_bn_cl_bwd_eval", "zsv_bn_cl_bwd_eval (mask recomputed from z)", "zsv_relu_bias_bwd_cl", "zsv_conv3d_bf16_wgrad",
    # the entry points that take no workspace: their inputs and outputs are pinned all the same
    "zsv_relu_fwd", "zsv_relu_bwd", "zsv_add_relu_fwd", "zsv_meanpool_fwd", "zsv_meanpool_bwd", "zsv_maxpool3d_fwd", "zsv_maxpool3d_bwd",
    "zsv_maxpool3d_bf16", "zsv_maxpool3d_bf16_bwd", "zsv_maxpool3d_fp8", "zsv_meanpool_bf16", "zsv_meanpool_bf16_bwd", "zsv_meanpool_fp8",
    "zsv_cl_bf16_to_ncs_f32", "zsv_ncs_f32_to_cl_bf16", "zsv_clip_to_bf16", "zsv_absmax_bf16", "zsv_bn_eval_coeffs", "zsv_adam_step",
    "zsv_clip_transform", "zsv_clip_transform_batch", "zsv_still_image_clips",
]


def test_every_entry_point_ran_and_on_every_row(capsys):
    """Run the file as a whole: this test reads what the tests above recorded."""
    with capsys.disabled():
        print("\nworkspace / output contract: (entry point, case x switch combinations run)")
        for name in sorted(COUNTS):
            print(f"  {name:68s} {COUNTS[name]:5d}")
        print("element-aligned runs (fp32 / uint8 tensors 4, 8, 12 / 1, 2, 3 bytes past a 256-byte boundary) per entry point")
        for name in sorted(COUNTS):
            print(f"  {name:68s} {ALIGN_RUNS[name]:5d}")
        changed = sum(len(v) for k, v in ROUTE_SEEN.items() if ROUTE_CHANGES[k] is not None)
        print(f"ROUTE_CHANGES: {sum(1 for v in ROUTE_CHANGES.values() if v is not None)} rows whose kernel family follows the alignment, {changed} calls under them")
    assert COUNTS, "nothing was recorded: this test reads what the other tests of the file record -- run the file as a whole, in order"
    missing = [e for e in ENTRY_POINTS if COUNTS[e] == 0]
    assert not missing, f"entry points that ran on no case (was the whole file run?): {missing}"
    # (h): an element-aligned run for every entry point on every combination the other runs cover
    short = {e: (ALIGN_RUNS[e], COUNTS[e]) for e in ENTRY_POINTS if ALIGN_RUNS[e] != (0 if e in NO_ELEMENT_OPERANDS else COUNTS[e])}
    assert not short, f"element-aligned runs vs combinations run: {short}"
    never = sorted(k for k in ROUTE_CHANGES if k not in ROUTE_SEEN)
    assert not never, f"ROUTE_CHANGES lists calls that never ran: {never}"
    slack = sorted(k for k, equal in ROUTE_SEEN.items() if ROUTE_CHANGES[k] is not None and any(equal))
    assert not slack, f"ROUTE_CHANGES lists calls whose element-aligned run gave the first run's bits (take them out): {slack}"
    for table in CONV_TABLES:
        names = {r.name for r in CONV_ROWS if r.table == table}
        assert len(names) >= (1 if table == "slab_sum_rows" else 2), f"{table}: GPU_ROW_LIMIT left {len(names)} row(s)"
        for call in ("fwd", "dgrad", "wgrad"):
            assert ROWS_RUN[(table, call)] == names, f"{table}: the plain {call} call missed {sorted(names - ROWS_RUN[(table, call)])}"
    expected = {("PANEL_CASES", "panel"): len(PANEL_ROWS), ("BN_CASES", "bn"): len(BN_SHAPES), ("BN_CASES", "channel_sum"): len(BN_SHAPES),
                ("test_linear", "linear"): len(params_of(T.test_linear)),
                ("test_cosine_topk", "topk"): len(params_of(TA.test_cosine_topk_c_abi_against_scipy)),
                ("FORWARD_CASES", "bf16_fwd"): len(X.FORWARD_CASES), ("STATS_CASES", "bf16_fwd_stats"): len(X.STATS_CASES),
                ("DGRAD_CASES", "bf16_pack_dgrad"): len(X.DGRAD_CASES), ("WGRAD_CASES", "bf16_wgrad"): len(X.WGRAD_CASES),
                ("bn_cl", "bn_cl"): len(BN_CL_CASES), ("fp8 CASES", "fp8_fwd"): len(F8.CASES),
                ("elementwise", "elementwise"): len(ELEMENTWISE_SHAPES), ("POOL_CASES", "maxpool"): len(T.POOL_CASES),
                ("CL_POOL_CASES", "cl_pools"): len(CL_POOL_CASES), ("converters", "converters"): len(CONVERTER_SHAPES),
                ("CLIP_CASES", "clip_to_bf16"): len(CLIP_CASES), ("absmax", "absmax"): 9, ("bn_eval_coeffs", "bn_eval_coeffs"): 4,
                ("adam_step", "adam_step"): 3, ("clip_transform", "clip_transform"): 2, ("clip_transform", "clip_transform_batch"): len(VIDEO_SIZES),
                ("still_image", "still_image_clips"): 3}
    for key, count in expected.items():
        assert len(ROWS_RUN[key]) == count, f"{key}: {len(ROWS_RUN[key])} of {count} rows ran"
