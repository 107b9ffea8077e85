"""The tile-configuration matrix of the fp32 convolution kernels (TEST INFRASTRUCTURE; never imported by the package, no GPU import).

Four kernel families pick a tile configuration per shape with a host-side cost model; a ``ZSV_*`` switch forces it.  Which
configuration an ordinary test reaches is whatever the cost model picks for its shape, so a retune silently moves the suite's
coverage.  The matrix forces EVERY configuration on the smallest shapes that still cross every tile edge.

Restated tables (one line each; ``tests/test_conv_configs_host.py`` checks them against the library's own answers):
``TAP_TILES`` (csrc/conv_tap.hip kTapCfgs), ``GENERIC_TILES`` (csrc/conv_igemm.hip dispatch), ``STAGED_ROWS`` x ``STAGED_COLS``
(csrc/conv_wgrad.hip wgrad_plan) and ``DMA_PAIRS`` (csrc/conv_wgrad_dma.hip wgrad_dma_plan).

Operands of two kinds, as in ``dwconv_cases.py``:

* ``exact``: integers in [-4, 4] ([-2, 2] for the statistics epilogue), the voxels on the six faces of every clip non-zero so a
  lost border voxel cannot hide behind a zero product.  The kernels multiply on v_mfma_f32_16x16x4_f32 and add their partial
  slabs in a fixed order: every partial sum is an integer below 2^24, so the result does not depend on the order of addition
  and must equal the fp64 reference bit for bit (``torch.equal``).
* ``normal``: standard normal operands.  A length-L fp32 dot product summed in ANY order, with or without fused multiply-adds,
  is within (L + 2) * 2^-24 * sum |a_i b_i| of the exact value (gamma_L = L u / (1 - L u), u = 2^-24; a bias or a residual is
  one more term of the sum and joins it with its absolute value).  The right-hand side is the same fp64 reference on absolute
  values, so the bound is per element; where it is 0 the result must be exactly 0.  L = Cin * taps (forward), Cout * taps
  (input gradient), N * To * Ho * Wo (weight gradient).

  - BatchNorm + ReLU prologue (``zsv_conv3d_fwd_pre``): an operand is relu(fma(x, scale, shift)), one more rounding, relative to
    |x| |scale| + |shift| (ReLU is 1-Lipschitz): the bound becomes (L + 3) u * conv(|x| |scale| + |shift|, |w|).
  - statistics epilogue: a tile's sums are a butterfly over <= 256 fp32 outputs (depth 8), so the per-channel sum of y is within
    ((L + 2) + 9) u * sum y_abs of the reference's and the sum of y^2 within (2 (L + 2) + 10) u * sum y_abs^2; for the shape
    used (L = 96, P = 288) both are below the (P + 2) u the matrix asserts.
  - fused ReLU: the forward bound holds as it is (ReLU is 1-Lipschitz), but the gradient mask y > 0 must be the reference's.
    Precondition: no pre-activation of the reference lies within 4 x its bound of 0.  The bias of a ReLU case is standard normal
    too, redrawn per output channel until that channel satisfies the condition (a change of seed, one channel at a time).

Preconditions are asserted on the CPU (``assert_preconditions``); none is a measurement and no tolerance is fitted anywhere.
"""
import functools
import os
import re
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
LIMIT = float(2 ** 24)
KINDS = ("exact", "normal")

# ---- restated tables ----------------------------------------------------------------------------------------------------
TAP_TILES = [(144, 128), (128, 128), (80, 128), (64, 128), (48, 256), (64, 256)]      # ZSV_CONV_CFG=0..5 (bm, bn)
GENERIC_TILES = [(144, 128), (128, 128), (80, 128), (64, 128), (48, 256)]             # ZSV_CONV_CFG=0..4
STAGED_ROWS, STAGED_COLS = (144, 128, 64, 80), (128, 64)                              # ZSV_WGRAD_CFG=0..3, ZSV_WGRAD_BN
DMA_TMS, DMA_TNS = (9, 8, 4, 5), (1, 2, 3, 7)                                         # ZSV_WGRAD_DMA_TM, ZSV_WGRAD_DMA_TN


def dma_pair_valid(tm, tn):
    """The parser of wgrad_dma_plan: tm in {9, 8, 4, 5}; tn in {1, 2, 3} with tn * tm <= 27, or the pair (4, 7)."""
    return tm in DMA_TMS and ((1 <= tn <= 3 and tn * tm <= 27) or (tn == 7 and tm == 4))


DMA_PAIRS = [(tm, tn) for tm in DMA_TMS for tn in DMA_TNS if dma_pair_valid(tm, tn)]
STAGED_PAIRS = [(i, bn) for i in range(4) for bn in STAGED_COLS]                      # (ZSV_WGRAD_CFG, ZSV_WGRAD_BN)


def staged_pair_parsed(cfg_text, bn_text):
    """The parser of wgrad_plan: rows = table[atoi(cfg) & 3]; columns = 64 if atoi(bn) == 64 else 128."""
    return STAGED_ROWS[int(cfg_text) & 3], 64 if int(bn_text) == 64 else 128


def wgrad_two_taps(taps, nblk, bn):
    """csrc/conv_wgrad.hip wgrad_two_taps: every column tile of ``bn`` columns spans at most two taps?"""
    nb, total = bn // 16, taps * nblk
    for b0 in range(0, total, nb):
        last = min(b0 + nb - 1, total - 1)
        if last // nblk - b0 // nblk > 1:
            return False
    return True


# ---- cases --------------------------------------------------------------------------------------------------------------
# cout: an int, or (what, delta): "bm" -> rows of the forced tile + delta, "2bm" -> twice the rows + delta, "16tm" -> 16 * tm + delta
# variants: (name, extra switches) -- every variant runs for every configuration and kind
Case = namedtuple("Case", "name family xs kernel stride padding cout bias relu env variants only")
Geom = namedtuple("Geom", "xs cout kernel stride padding")


def _case(name, family, xs, kernel, stride, padding, cout, bias=False, relu=False, env=None, variants=None, only=None):
    return Case(name, family, xs, kernel, stride, padding, cout, bias, relu, dict(env or {}), list(variants or [("default", {})]), only)


ONE = (1, 1, 1)
CASES = [
    # ---- tap kernel (csrc/conv_tap.hip), configurations 0..5
    # two row tiles, the second with one live row; two channel blocks, the second with one live channel; oS = 130 (plain epilogue);
    # P = 260: 4 columns in the last tile, the clip boundary inside a column tile; its input gradient has M = 17
    _case("tap_ragged", "tap", (2, 17, 2, 5, 13), (1, 3, 3), ONE, (0, 1, 1), ("bm", 1)),
    # oS = 144, P = 288: the LDS-transposed epilogue (and the plain one on the same shape); modes in test_conv_configs_gpu.py
    _case("tap_aligned", "tap", (2, 32, 3, 8, 6), (3, 1, 1), ONE, (1, 0, 0), ("bm", -1), env={"ZSV_NO_SPLITK": "1"},
          variants=[("lds", {}), ("plain", {"ZSV_NO_LDS_EPILOGUE": "1"})]),
    # P = 36 (less than one 64-voxel segment), 27 chunks: uneven parts, one chunk per part, a clamp; the scalar slab reduce
    _case("tap_splitk", "tap", (1, 48, 1, 6, 6), (1, 3, 3), ONE, (0, 1, 1), ("2bm", -8), bias=True, relu=True,
          variants=[("ks2", {"ZSV_TAP_KS": "2"}), ("ks4", {"ZSV_TAP_KS": "4"}), ("ks27", {"ZSV_TAP_KS": "27"}),
                    ("ks99", {"ZSV_TAP_KS": "99"}), ("ks4_scalar_reduce", {"ZSV_TAP_KS": "4", "ZSV_SPLITK_REDUCE_SCALAR": "1"})]),
    # 27 taps, strided: the input gradient runs class by class on the tap kernel, residue classes of 12, 8, 6 and 4 taps... (3x3x3
    # has no merged stride-2 kernel, so ZSV_NO_DGRAD_S2 changes nothing here; tap_strided9 is the shape where it does)
    _case("tap_strided27", "tap", (2, 16, 3, 9, 11), (3, 3, 3), (1, 2, 2), (1, 1, 1), ("bm", 1),
          variants=[("default", {}), ("no_dgrad_s2", {"ZSV_NO_DGRAD_S2": "1"})]),
    # 1x3x3 stride (1,2,2) on even extents: by default the merged stride-2 kernel; with ZSV_NO_DGRAD_S2 four classes of 4, 2, 2, 1 taps
    _case("tap_strided9", "tap", (2, 16, 2, 8, 10), (1, 3, 3), (1, 2, 2), (0, 1, 1), ("bm", 1),
          variants=[("default", {}), ("no_dgrad_s2", {"ZSV_NO_DGRAD_S2": "1"})]),
    # 30 taps: the highest count the tap kernel takes with extents <= 7 (the upper tap-validity bits)
    _case("tap_30_taps", "tap", (2, 16, 3, 7, 9), (2, 3, 5), ONE, (0, 1, 2), 40),
    # conv_tap_dma_kernel<9,2,1,4,1,4,9>: configuration 0, forward, 9 taps, 4 channel blocks; Cin 49: 15 padded channels in the fourth
    _case("tap_9x4_cin64", "tap", (2, 64, 1, 6, 10), (1, 3, 3), ONE, (0, 1, 1), 144, env={"ZSV_NO_SPLITK": "1"}, only=(0,)),
    _case("tap_9x4_cin49", "tap", (2, 49, 1, 6, 10), (1, 3, 3), ONE, (0, 1, 1), 144, env={"ZSV_NO_SPLITK": "1"}, only=(0,)),
    # ---- generic kernel (csrc/conv_igemm.hip), tilings 0..4: wide (> 31 taps), vectorised A (K % 4 == 0), scalar A
    _case("generic_wide", "generic", (2, 3, 2, 9, 11), (1, 7, 7), (1, 2, 2), (0, 3, 3), ("bm", 1)),
    _case("generic_vector_a", "generic", (2, 8, 2, 5, 7), (1, 3, 3), ONE, (0, 1, 1), ("bm", 1)),
    _case("generic_scalar_a", "generic", (2, 5, 2, 5, 7), (3, 3, 3), ONE, (1, 1, 1), ("bm", 1)),
    # the 30-tap case's neighbour: 32 taps land on the wide generic kernel, forward and input gradient
    _case("generic_32_taps", "generic", (2, 16, 3, 7, 9), (2, 4, 4), ONE, (0, 1, 2), 40),
    # ---- register-staged weight gradient (csrc/conv_wgrad.hip), 4 x 2 pairs: strided shapes, which no specialised route takes
    _case("staged_av4", "staged", (2, 17, 2, 9, 11), (1, 3, 3), (1, 2, 2), (0, 1, 1), ("bm", 1)),            # oS = 60
    _case("staged_scalar", "staged", (3, 40, 5, 3, 7), (3, 1, 1), (2, 1, 1), (1, 0, 0), ("bm", -1)),         # oS = 63
    _case("staged_7_blocks", "staged", (1, 112, 1, 5, 8), (1, 3, 3), (1, 2, 2), (0, 1, 1), 20),             # oS = 12: two-tap at 128 columns
    _case("staged_7_blocks_scalar", "staged", (1, 112, 1, 5, 6), (1, 3, 3), (1, 2, 2), (0, 1, 1), 20),      # oS = 9: the scalar two-tap form at 128 columns
    # ---- LDS-DMA weight gradient (csrc/conv_wgrad_dma.hip), 13 pairs
    _case("dma_one_chunk", "dma", (3, 32, 1, 4, 4), (1, 3, 3), ONE, (0, 1, 1), ("16tm", 1)),                 # one chunk per clip
    _case("dma_864_columns", "dma", (2, 17, 2, 4, 10), (3, 3, 3), ONE, (1, 1, 1), ("16tm", -1)),             # W % 4 != 0
    _case("dma_frame_minor", "dma", (2, 16, 4, 4, 4), (3, 3, 3), ONE, (1, 1, 1), ("16tm", 1),
          variants=[("frame_minor", {}), ("linear", {"ZSV_WGRAD_LINEAR_WALK": "1"})]),
]
DMA_ROUTE_ENV = {"ZSV_NO_WGRAD_WINO": "1", "ZSV_NO_WGRAD_TRING": "1"}       # the DMA route is then the first the shape admits
NO_TWOTAP_ENV = {"ZSV_WGRAD_NO_TWOTAP": "1"}

# the BatchNorm + ReLU prologue: the smallest temporal shape zsv_conv3d_pre_supported admits on the direct kernel (N * S >= 16384,
# T % 4 == 0, Cin >= 99, ceil64(Cout) <= 1.3 Cout): Cout = 100 leaves a ragged last row tile in every configuration, Cin = 100 a
# seventh channel block with 4 live channels
PRE_GEOM = Geom((1, 100, 4, 64, 64), 100, (3, 1, 1), ONE, (1, 0, 0))
PRE_ENV = {"ZSV_NO_SPLITK": "1", "ZSV_NO_WINOT": "1"}


def by_name(name):
    return next(c for c in CASES if c.name == name)


def family_cases(family):
    return [c for c in CASES if c.family == family]


def configs(family):
    """The configurations of a family: tap 0..5, generic 0..4, staged (cfg, bn), dma (tm, tn)."""
    return {"tap": list(range(6)), "generic": list(range(5)), "staged": STAGED_PAIRS, "dma": DMA_PAIRS}[family]


def config_id(cfg):
    return "x".join(str(v) for v in cfg) if isinstance(cfg, tuple) else f"cfg{cfg}"


def force_env(family, cfg):
    """The switches that force configuration ``cfg`` of ``family``."""
    if family in ("tap", "generic"):
        return {"ZSV_CONV_CFG": str(cfg)}
    if family == "staged":
        return {"ZSV_WGRAD_CFG": str(cfg[0]), "ZSV_WGRAD_BN": str(cfg[1])}
    return dict(DMA_ROUTE_ENV, ZSV_WGRAD_DMA_TM=str(cfg[0]), ZSV_WGRAD_DMA_TN=str(cfg[1]))


def tile_rows(family, cfg):
    if family == "tap":
        return TAP_TILES[cfg][0]
    if family == "generic":
        return GENERIC_TILES[cfg][0]
    if family == "staged":
        return STAGED_ROWS[cfg[0]]
    return 16 * cfg[0]


def geometry(case, cfg):
    cout = case.cout
    if not isinstance(cout, int):
        what, delta = cout
        rows = tile_rows(case.family, cfg)
        cout = {"bm": rows, "2bm": 2 * rows, "16tm": rows}[what] + delta
    return Geom(case.xs, cout, case.kernel, case.stride, case.padding)


def staged_forms(case, cfg):
    """(av4, twotap) of a staged case at a pair, as wgrad_staged decides them (operands at 16-byte aligned addresses)."""
    g = geometry(case, cfg)
    o = out_shape(g)
    os_, p = o[2] * o[3] * o[4], o[0] * o[2] * o[3] * o[4]
    taps = g.kernel[0] * g.kernel[1] * g.kernel[2]
    return os_ % 4 == 0 and p >= 4, wgrad_two_taps(taps, (g.xs[1] + 15) // 16, cfg[1])


def runs(family):
    """Every (case, cfg, variant name, switches) of a family: the forcing switches, the case's own and the variant's; a staged case
    whose tile is two-tap runs again with ZSV_WGRAD_NO_TWOTAP."""
    out = []
    for case in family_cases(family):
        for cfg in configs(family):
            if case.only is not None and cfg not in case.only:
                continue
            for vname, venv in case.variants:
                env = dict(force_env(family, cfg))
                env.update(case.env)
                env.update(venv)
                out.append((case, cfg, vname, env))
                if family == "staged" and staged_forms(case, cfg)[1]:
                    out.append((case, cfg, vname + "_no_twotap", dict(env, **NO_TWOTAP_ENV)))
    return out


def all_runs():
    return [r for f in ("tap", "generic", "staged", "dma") for r in runs(f)]


def switch_names():
    """Every ZSV_* name the matrix sets."""
    names = set(PRE_ENV)
    for _, _, _, env in all_runs():
        names.update(env)
    return names


def knob_list():
    """The names in ZSV_KNOB_LIST of csrc/knobs.h, with their ZSV_ prefix (parsed from the header text)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zeroshotvideoclassification_amd", "csrc", "knobs.h")
    text = open(path).read()
    body = text[text.index("#define ZSV_KNOB_LIST(X)"):text.index("namespace zsv")]
    return {"ZSV_" + n for n in re.findall(r"\bX\((\w+)\)", body)}


# ---- operands and references ----------------------------------------------------------------------------------------------
def out_shape(g):
    return (g.xs[0], g.cout) + tuple((e + 2 * pp - kk) // ss + 1 for e, kk, ss, pp in zip(g.xs[2:], g.kernel, g.stride, g.padding))


def fill_faces(gen, x, amp):
    """(N, C, T, H, W): every zero on one of the six faces of a clip's (T, H, W) box is redrawn from +-{1 .. amp}."""
    t, h, w = x.shape[2:]
    face = torch.zeros((t, h, w), dtype=torch.bool)
    face[[0, -1]] = True
    face[:, [0, -1]] = True
    face[:, :, [0, -1]] = True
    sub = torch.randint(1, amp + 1, tuple(x.shape), generator=gen).double() * (torch.randint(0, 2, tuple(x.shape), generator=gen).double() * 2 - 1)
    return torch.where(face & (x == 0), sub, x)


def faces_nonzero(x):
    return all(bool((f != 0).all()) for f in (x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1], x[..., 0], x[..., -1]))


def _seed(g, kind, salt):
    return zlib.crc32(f"{tuple(g)} {kind} {salt}".encode())        # (not hash(): randomised per process)


def _pre_activation(g, x, w, b, res):
    z = F.conv3d(x, w, b, g.stride, g.padding)
    z_abs = F.conv3d(x.abs(), w.abs(), None if b is None else b.abs(), g.stride, g.padding)
    if res is not None:
        z, z_abs = z + res, z_abs + res.abs()
    return z, z_abs


@functools.lru_cache(maxsize=None)
def operands(g, kind, bias=False, relu=False, residual=False, amp=4):
    """x, w, b (or None), res (or None), dy of geometry ``g`` as fp64 CPU tensors; the same for every caller."""
    gen = torch.Generator().manual_seed(_seed(g, kind, f"{bias}{residual}{amp}"))
    wshape, oshape = (g.cout, g.xs[1]) + g.kernel, out_shape(g)
    if kind == "exact":
        draw = lambda s: torch.randint(-amp, amp + 1, tuple(s), generator=gen).double()
        x, dy = fill_faces(gen, draw(g.xs), amp), fill_faces(gen, draw(oshape), amp)
    else:
        draw = lambda s: torch.randn(tuple(s), generator=gen, dtype=torch.float64).float().double()     # (fp32 values)
        x, dy = draw(g.xs), draw(oshape)
    w = draw(wshape)
    b = draw((g.cout,)) if bias else None
    res = draw(oshape) if residual else None
    if relu and bias and kind == "normal":
        # redraw a channel's bias until none of its pre-activations lies within 4 x its bound of 0 (module docstring)
        taps = g.kernel[0] * g.kernel[1] * g.kernel[2]
        for _ in range(200):
            z, z_abs = _pre_activation(g, x, w, b, res)
            near = (z.abs() <= 4 * (g.xs[1] * taps + 2) * U * z_abs).permute(1, 0, 2, 3, 4).reshape(g.cout, -1).any(1)
            if not bool(near.any()):
                break
            b = torch.where(near, draw((g.cout,)), b)
    return x, w, b, res, dy


@functools.lru_cache(maxsize=None)
def reference(g, kind, bias=False, relu=False, residual=False, amp=4):
    """fp64 results and per-element bounds: x, w, b, res, dy, z (pre-activation), y, dx, dw, y_abs, y_bound, dx_bound, dw_bound."""
    x, w, b, res, dy = operands(g, kind, bias, relu, residual, amp)
    taps = g.kernel[0] * g.kernel[1] * g.kernel[2]
    o = out_shape(g)
    z, z_abs = _pre_activation(g, x, w, b, res)
    y = torch.relu(z) if relu else z
    gr = dy * (z > 0) if relu else dy                     # the gradient that reaches the convolution
    dx = torch.nn.grad.conv3d_input(x.shape, w, gr, g.stride, g.padding)
    dw = torch.nn.grad.conv3d_weight(x, w.shape, gr, g.stride, g.padding)
    dx_abs = torch.nn.grad.conv3d_input(x.shape, w.abs(), gr.abs(), g.stride, g.padding)
    dw_abs = torch.nn.grad.conv3d_weight(x.abs(), w.shape, gr.abs(), g.stride, g.padding)
    n_pos = o[0] * o[2] * o[3] * o[4]
    return {"x": x, "w": w, "b": b, "res": res, "dy": dy, "z": z, "y": y, "dx": dx, "dw": dw, "y_abs": z_abs,
            "y_bound": (g.xs[1] * taps + 2) * U * z_abs, "dx_bound": (g.cout * taps + 2) * U * dx_abs,
            "dw_bound": (n_pos + 2) * U * dw_abs, "dx_abs": dx_abs, "dw_abs": dw_abs}


@functools.lru_cache(maxsize=None)
def pre_reference(g, kind):
    """The BatchNorm + ReLU prologue on ``g``: coef ([2][pitch]: scale row, shift row, zero padding; pitch = Cin rounded up to 16),
    y = conv(relu(x * scale + shift)) in fp64 and its bound (module docstring).  ``exact``: scale and shift are integers in [-2, 2]."""
    x, w, _, _, _ = operands(g, kind)
    gen = torch.Generator().manual_seed(_seed(g, kind, "pre"))
    cin = g.xs[1]
    if kind == "exact":
        scale, shift = (torch.randint(-2, 3, (cin,), generator=gen).double() for _ in range(2))
    else:
        scale, shift = (torch.randn(cin, generator=gen).float().double() for _ in range(2))
    coef = torch.zeros(2, (cin + 15) // 16 * 16, dtype=torch.float64)
    coef[0, :cin], coef[1, :cin] = scale, shift
    v = lambda t: t.view(1, -1, 1, 1, 1)
    a = torch.relu(x * v(scale) + v(shift))
    a_abs = x.abs() * v(scale).abs() + v(shift).abs()
    y = F.conv3d(a, w, None, g.stride, g.padding)
    y_abs = F.conv3d(a_abs, w.abs(), None, g.stride, g.padding)
    taps = g.kernel[0] * g.kernel[1] * g.kernel[2]
    return {"x": x, "w": w, "coef": coef, "y": y, "y_abs": y_abs, "y_bound": (cin * taps + 3) * U * y_abs}


def assert_preconditions(g, kind, bias=False, relu=False, residual=False, amp=4, stats=False):
    """The conditions under which the comparison of this case is the one the module docstring derives."""
    r = reference(g, kind, bias, relu, residual, amp)
    what = f"{tuple(g)} {kind}"
    if kind == "exact":
        assert faces_nonzero(r["x"]) and faces_nonzero(r["dy"]), f"{what}: a border voxel is zero"
        for name in ("y_abs", "dx_abs", "dw_abs"):
            assert float(r[name].max()) < LIMIT, f"{what}: sum |terms| of {name[:-4]} reaches 2^24"
        if stats:
            sq = (r["y"] * r["y"]).sum(dim=(0, 2, 3, 4))
            assert float(sq.max()) < LIMIT, f"{what}: a channel's sum of y^2 reaches 2^24"
    if relu and kind == "normal":
        near = r["z"].abs() <= 4 * r["y_bound"]
        assert not bool(near.any()), f"{what}: {int(near.sum())} pre-activation(s) within 4 x the bound of 0"


def check(name, got, ref, bound, kind):
    """``exact``: bit for bit; ``normal``: |got - ref| <= bound per element (exactly 0 where the bound is 0).  Returns the worst
    error / bound ratio."""
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


# ---- the tap kernel's workspace, restated (csrc/conv_api.hip tap_fwd_workspace, dgrad_plan) ------------------------------------
def align256(n):
    return (n + 255) & ~255


def tap_workspace_bytes(m, c, taps, out_elems, cfg, ks):
    """[packed panel: (taps * Cpad + 16) rows of Mp floats][ks > 1: ks partial slabs of the output]; ``ks`` is clamped to the chunk
    count as ZSV_TAP_KS is."""
    bm = TAP_TILES[cfg][0]
    mp = (m + bm - 1) // bm * bm
    nblk = (c + 15) // 16
    ks = max(1, min(int(ks), taps * nblk))
    return align256((taps * nblk * 16 + 16) * mp * 4) + (ks * out_elems * 4 if ks > 1 else 0)
