"""The instantiation matrix of the Winograd-form forward / input-gradient kernels, csrc/conv_wino.hip (TEST INFRASTRUCTURE; never
imported by the package, no GPU import).  The companion of ``conv_config_cases.py``, whose helpers it reuses.

``wino_run`` / ``winot_run`` pick among 46 kernel instantiations (``ALL_INSTANTIATIONS``); which one a shape reaches is decided by
the host planners restated below, one short function each (``tests/test_wino_configs_host.py`` checks them against the library's own
answers under every set of switches the matrix uses).  The matrix forces every instantiation on the smallest shapes that cross its
edges; ``expected_instantiation`` says which (kernel, template arguments, K parts) a run reaches.

A case has M rows (Cout forward, Cin for the input gradient) and C reduction channels; both directions are the same operation
``conv3d(inp, G)`` with G the weights (forward) or the weights with flipped taps and swapped channel axes (input gradient).

Operands of two kinds:

* ``exact``: activations / incoming gradients are integers in [-2, 2] with non-zero voxels on the six faces of every clip, weights
  are 24 x integers in [-2, 2], bias / residual / shortcut gradient are integers in [-50, 50], prologue scale and shift integers
  in [-2, 2].  pack_wino_value<6> divides by 4, 6, 12 and 24 (in double, rounded once): with every weight a multiple of 24 all six
  U are integers; the F(2,3) pack 0.5 * ((g0 + g2) +- g1) is exact as well.  B has coefficients 1, 2, 4, 5, so V is an integer,
  every MFMA partial sum is an integer, and the output transform has coefficients 1, 2, 4, 8.  While the Winograd algorithm run
  on ABSOLUTE values, |A| . sum_K (|U| (.) |B| |d|) + |bias| + |add|, stays below 2^24 every intermediate is an exactly
  representable integer whatever the order of summation, the K split or the FMA contraction: the result must equal the fp64
  convolution bit for bit (``torch.equal``).  ``abs_wino`` is that restatement; it is NOT conv(|x|, |w|): the transforms amplify.

  Statistics (one entry per channel and column tile, compared tile by tile): every y is an exact integer, so sum y is exact
  while the tile's sum of |y| stays below 2^24.  sum y^2: every y is a multiple of 24, hence of 8, so y^2 and every partial sum of squares is a
  multiple of 64; the kernels form y*y + y*y (fused or not: one rounding of an exactly representable value) and add, so every
  partial is exact while the tile's sum of y^2 stays below 2^30 (= 64 * 2^24), which is asserted.

* ``normal``: standard-normal fp32 values, per element  |got - ref| <= (L + C_ROUND) * 2^-24 * abs_wino.
  L = padded reduction channels x row taps is the number of products an accumulator of one Winograd point takes (a length-L
  fp32 sum in any order, fused or not, carries at most L roundings per term).  C_ROUND = 12 is counted from the code, per term of
  the sum, along the deepest path:
    1  U rounded once (pack_bodies.h; the F(2,3) pack has two roundings, its V one: the same total),
    2  V: e.g. fma(4, d0, fma(-5, d2, d4)) or fma(-4, d1 + d2, d3 + d4),
    3  output transform: d34 = M3 - M4, fma(8, d34, d12), + M5,
    1  + add, 1 + bias, 1 the prologue's fma(x, scale, shift) (relative to |x| |scale| + |shift|; ReLU is 1-Lipschitz),
  = 9, plus 3 for the second-order terms of (1 + u)^(L + 9) <= 1 + (L + 12) u (L + 12 < 2^12 here).  K parts: a part accumulates
  L / ks >= 12 * 16 / 4 products less than L and the ordered slab sum adds ks - 1 <= 7 roundings, fewer than it saves.
  Where the bound is 0 the result must be exactly 0.  ReLU cases keep the precondition of the previous matrix: no
  pre-activation of the reference within 4 bounds of 0, the bias redrawn per channel until that holds (``relu_bias``).
  Statistics (per tile a butterfly over <= 256 values, depth 8): sum y within (L + C_ROUND + 9) u sum abs_wino, sum y^2 within
  (2 (L + C_ROUND) + 10) u sum abs_wino^2 (an error e of y moves y^2 by at most 2 |y| e, plus the rounding of the square), tile by tile.

Nothing is fitted; ``assert_preconditions`` asserts every condition on the CPU.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_config_cases as B
from conv_config_cases import Geom, LIMIT, U, KINDS, check, faces_nonzero, fill_faces, knob_list, out_shape  # noqa: F401

C_ROUND = 12
SQ_LIMIT = float(2 ** 30)
ONE = (1, 1, 1)

# ---- the 46 instantiations ------------------------------------------------------------------------------------------------
ALL_INSTANTIATIONS = (
    [("conv_wino_kernel", t) for t in ((3, 12, 1), (3, 0, 1), (3, 0, 0), (4, 0, 1), (4, 0, 0))] +
    [("conv_wino4_kernel", (tm, nch, vw, epi)) for tm, nch, vw in ((3, 0, 0), (3, 12, 0), (4, 0, 0), (3, 0, 1), (4, 0, 1)) for epi in (0, 1, 2, 4, 8)] +
    [("conv_winot_kernel", (tm, pre)) for tm in (3, 4) for pre in (0, 1)] +
    [("conv_winot4_kernel", (tm, pre, epi)) for tm in (3, 4) for pre in (0, 1) for epi in (0, 1, 2)])


# ---- restated planners (csrc/conv_wino.hip, host side) -----------------------------------------------------------------------
def _knob(env, name):
    return env.get("ZSV_" + name)


def rows_and_channels(g, direction):
    """(M, C): rows and reduction channels of a launch."""
    return (g.cout, g.xs[1]) if direction == "fwd" else (g.xs[1], g.cout)


def wino_tm(m):
    """16-row blocks per workgroup: 4, or 3 when 48-row tiles pad less."""
    return 3 if (m + 47) // 48 * 48 < (m + 63) // 64 * 64 else 4


def wino_vw_width(g, env):
    w = g.xs[4]
    if w % 4 == 0 or _knob(env, "WINO_NO_VW") or _knob(env, "WINO_NO_F43"):
        return 0
    for wv in (8, 16, 32, 64):
        if w < wv:
            return wv if w > wv - 4 and 8 * w >= 7 * wv else 0
    return 0


def wino_vw_plan(g, m, direction, env):
    """(K parts, tm) of a virtual-width launch: best rows x round fill over one or two rounds of 512 workgroups."""
    n, _, t, h, _ = g.xs
    tiles_n = (n * t * h * wino_vw_width(g, env) + 255) // 256
    c = rows_and_channels(g, direction)[1]
    nchunks = (c + 15) // 16 * 3 * g.kernel[0]
    e = _knob(env, "WINO_VW_MIN_WGS")
    min_wgs = int(e) if e else 256
    best, best_ks, tm = 0.0, 0, 4
    for tt in (4, 3):
        bm = 16 * tt
        tiles = (m + bm - 1) // bm * tiles_n
        rows = float(m) / float((m + bm - 1) // bm * bm)
        for ks in range(1, 9):
            if ks > 1 and (nchunks // ks < 12 or tiles >= 512):
                break
            wgs = tiles * ks
            if wgs < min_wgs or (ks > 1 and wgs > 1024):
                continue
            r, rc = float(wgs) / 512.0, float((wgs + 511) // 512)
            fill = r if wgs <= 512 else r / (r + 0.33 * (rc - r))
            eff = rows * fill * (1.0 - 0.03 * (ks - 1))
            if eff > best + 1e-9:
                best, best_ks, tm = eff, ks, tt
    return best_ks, tm


def winot_shape(g):
    return g.kernel == (3, 1, 1) and g.stride == ONE and g.padding == (1, 0, 0)


def winot_segs(g):
    pw = 256 // g.xs[2]
    return (g.xs[3] * g.xs[4] + pw - 1) // pw


def winot_geometry(g, m, env):
    if _knob(env, "NO_WINO") or _knob(env, "NO_WINOT") or not winot_shape(g):
        return False
    n, cin, t, h, w = g.xs
    t32 = t == 32 and not _knob(env, "WINOT_NO_F43") and not _knob(env, "WINOT_NO_T32")
    if (t not in (4, 8, 16) and not t32) or (h * w) % 4 != 0 or cin < 16 or g.cout < 16:
        return False
    p = n * t * h * w
    if g.cout * p >= 1 << 29 or cin * p >= 1 << 29:
        return False
    bm = 16 * wino_tm(m)
    tiles = (m + bm - 1) // bm * n * winot_segs(g)
    covered = winot_segs(g) * (256 // t)
    e1, e2 = _knob(env, "WINOT_MIN_TILES"), _knob(env, "WINOT_MAX_WASTE")
    return tiles >= (int(e1) if e1 else 256) and covered * 100 <= h * w * (100 + (int(e2) if e2 else 35))


def wino_ksplit(g, m, direction, env):
    """K parts: 1 (temporal, or enough tiles), 2..4 (2..8 virtual-width) parts of >= 12 chunks, 0 = not on these kernels."""
    if winot_geometry(g, m, env):
        return 1
    if wino_vw_width(g, env):
        return wino_vw_plan(g, m, direction, env)[0]
    n, _, t, h, w = g.xs
    bm, c = 16 * wino_tm(m), rows_and_channels(g, direction)[1]
    tiles = (m + bm - 1) // bm * ((n * t * h * w + 255) // 256)
    nchunks = (c + 15) // 16 * 3 * g.kernel[0]
    e = _knob(env, "WINO_MIN_TILES")
    min_tiles = int(e) if e else 512
    if tiles >= min_tiles:
        return 1
    if _knob(env, "WINO_NO_SPLITK"):
        return 0
    for ks in (2, 3, 4):
        if tiles * ks >= min_tiles and nchunks // ks >= 12:
            return ks
    return 0


def wino_geometry(g, m, direction, env):
    if winot_geometry(g, m, env):
        return True
    if _knob(env, "NO_WINO"):
        return False
    kt = g.kernel[0]
    if kt not in (1, 3) or g.kernel[1:] != (3, 3) or g.stride != ONE or g.padding != (kt // 2, 1, 1):
        return False
    n, cin, t, h, w = g.xs
    vw = wino_vw_width(g, env)
    if (w % 2 != 0 and not vw) or cin < 16 or g.cout < 16:
        return False
    p = n * t * h * w
    if (p % 2 != 0 and not vw) or g.cout * p >= 1 << 29 or cin * p >= 1 << 29:
        return False
    return wino_ksplit(g, m, direction, env) > 0


def wino_applicable(g, direction, env):
    m = rows_and_channels(g, direction)[0]
    return wino_geometry(g, m, direction, env) and not (direction == "fwd" and _knob(env, "NO_WINO_FWD"))


def wino_f43(g, env):
    return (g.xs[4] % 4 == 0 and not _knob(env, "WINO_NO_F43")) or wino_vw_width(g, env) != 0


def wino_tm_for(g, m, direction, env):
    if not winot_geometry(g, m, env) and wino_vw_width(g, env):
        return wino_vw_plan(g, m, direction, env)[1]
    return wino_tm(m)


def wino_bytes(g, direction, env):
    """The transformed-weight panel."""
    m, c = rows_and_channels(g, direction)
    bm = 16 * wino_tm_for(g, m, direction, env)
    mp, nblk = (m + bm - 1) // bm * bm, (c + 15) // 16
    if winot_shape(g):
        return B.align256(nblk * 6 * 16 * mp * 4)
    return B.align256(nblk * 3 * g.kernel[0] * (6 if wino_f43(g, env) else 4) * 16 * mp * 4)


def wino_workspace_bytes(g, direction, env):
    """wino_bytes + ks x out_bytes (the K parts' slabs)."""
    m = rows_and_channels(g, direction)[0]
    ks = wino_ksplit(g, m, direction, env)
    n, _, t, h, w = g.xs
    return wino_bytes(g, direction, env) + (ks * n * m * t * h * w * 4 if ks > 1 else 0)


def wino_fwd_stat_tiles(g, env):
    n, _, t, h, w = g.xs
    if winot_geometry(g, g.cout, env):
        return n * winot_segs(g)
    return (n * t * h * (wino_vw_width(g, env) or w) + 255) // 256


def fwd_stat_tiles_query(g, env):
    """zsv_conv3d_fwd_stat_tiles on a shape these kernels take: 0 with K parts."""
    return 0 if _knob(env, "NO_FUSED_STATS") or wino_ksplit(g, g.cout, "fwd", env) != 1 else wino_fwd_stat_tiles(g, env)


def fusable(g, direction, env):
    """zsv_conv3d_fwd_add_supported / zsv_conv3d_dgrad_add_supported: the epilogue extras need the whole K in one workgroup."""
    return wino_ksplit(g, rows_and_channels(g, direction)[0], direction, env) == 1


def wino4_epi(bias, relu, add, stats, generic):
    """The epilogue wino4_launch compiles in."""
    if bias and relu and not add and not stats and not generic:
        return 8
    if bias or relu or (add and stats) or generic:
        return 4
    if add:
        return 2
    return 1 if stats else 0


def winot4_epi(bias, relu, add, stats, generic):
    """The epilogue winot4_launch compiles in."""
    if add or bias or relu or generic:
        return 2
    return 1 if stats else 0


Mode = namedtuple("Mode", "name bias relu add stats pre")


def _mode(name, bias=False, relu=False, add=False, stats=False, pre=False):
    return Mode(name, bias, relu, add, stats, pre)


PLAIN = _mode("plain")
# forward: plain, + statistics, bias + ReLU, the other bias / ReLU / residual combinations.  ReLU without a bias has no bias to
# redraw for the ``normal`` precondition, so it runs in the ``exact`` kind only (EXACT_ONLY).  Residual + statistics is refused by
# zsv_conv3d_fwd_full whatever the kernel (REFUSED): the (add && statistics) branch of wino4_launch has no caller in the C ABI.
FWD_MODES = [PLAIN, _mode("stats", stats=True), _mode("bias_relu", bias=True, relu=True), _mode("bias", bias=True),
             _mode("residual", add=True), _mode("bias_residual", bias=True, add=True),
             _mode("bias_residual_relu", bias=True, relu=True, add=True), _mode("relu", relu=True)]
EXACT_ONLY = ("relu",)
REFUSED = _mode("residual_stats", add=True, stats=True)
DGRAD_MODES = [PLAIN, _mode("shortcut", add=True)]
PRE_MODES = [_mode("pre", pre=True), _mode("pre_stats", pre=True, stats=True)]
SPLITK_FWD_MODES = [PLAIN, _mode("bias_relu", bias=True, relu=True)]          # bias + ReLU move into splitk_reduce


def expected_instantiation(g, direction, mode, env):
    """(kernel name, template arguments, K parts) of the launch, or None when the shape is not on these kernels."""
    if not wino_applicable(g, direction, env):
        return None
    m, c = rows_and_channels(g, direction)
    if winot_geometry(g, m, env):
        tm, pre = wino_tm(m), int(mode.pre)
        if _knob(env, "WINOT_NO_F43"):
            return ("conv_winot_kernel", (tm, pre), 1)
        return ("conv_winot4_kernel", (tm, pre, winot4_epi(mode.bias, mode.relu, mode.add, mode.stats, bool(_knob(env, "WINOT_GENERIC_EPILOGUE")))), 1)
    tm, ks = wino_tm_for(g, m, direction, env), wino_ksplit(g, m, direction, env)
    nchunks = (c + 15) // 16 * 3 * g.kernel[0]
    twelve = 12 if (tm == 3 and nchunks == 12 and ks == 1) else 0
    if wino_f43(g, env):
        bias, relu = (mode.bias, mode.relu) if ks == 1 else (False, False)           # K parts: bias / ReLU move to the slab sum
        epi = wino4_epi(bias, relu, mode.add, mode.stats, bool(_knob(env, "WINO_GENERIC_EPILOGUE")))
        vw = 1 if wino_vw_width(g, env) else 0
        return ("conv_wino4_kernel", (tm, 0 if vw else twelve, vw, epi), ks)
    x4 = 1 if g.xs[4] % 4 == 0 and not _knob(env, "WINO_NO_X4") else 0
    return ("conv_wino_kernel", (tm, twelve if x4 else 0, x4), ks)


# ---- cases --------------------------------------------------------------------------------------------------------------
# shape: (N, T, H, W); m: rows; c: reduction channels; variants: (name, switches) -- every variant runs in both directions
Case = namedtuple("Case", "name shape kt m c variants modes directions")
BASE_ENV = {"ZSV_WINO_MIN_TILES": "1", "ZSV_WINO_VW_MIN_WGS": "1", "ZSV_WINOT_MIN_TILES": "1", "ZSV_WINOT_MAX_WASTE": "100000"}
F43, F23 = ("f43", {}), ("f23", {"ZSV_WINO_NO_F43": "1"})
F23_NO_X4 = ("f23_no_x4", {"ZSV_WINO_NO_F43": "1", "ZSV_WINO_NO_X4": "1"})
T43, T23 = ("f43", {}), ("f23", {"ZSV_WINOT_NO_F43": "1"})
BOTH = ("fwd", "dgrad")


def _spatial(name, shape, kt, m, c, variants, modes="all", directions=BOTH):
    return Case(name, shape, kt, m, c, list(variants), modes, directions)


def _tiles(shape, m):
    n, t, h, w = shape
    bm = 16 * wino_tm(m)
    return (m + bm - 1) // bm * ((n * t * h * w + 255) // 256)


def _ks_variants(shape, m, forms):
    """ZSV_WINO_MIN_TILES = tiles * (ks - 1) + 1 forces ks parts (fewer do not reach it; each part keeps >= 12 chunks)."""
    return [(f"{fname}_ks{ks}", dict(fenv, ZSV_WINO_MIN_TILES=str(_tiles(shape, m) * (ks - 1) + 1))) for fname, fenv in forms for ks in (2, 3, 4)]


S_ODD, S_PAIR = (3, 3, 5, 6), (5, 1, 1, 2)          # W % 4 == 2: F(2,3) without X4.  P = 270: a second tile of 14 voxels; one pair per row
S_504, S_ROW, S_QUAD = (3, 2, 7, 12), (3, 3, 5, 4), (5, 1, 1, 4)        # W % 4 == 0: P = 504; every quad a whole row (d0 and d5 padding); one quad
CASES = [
    # ---- F(2,3) along W without X4: conv_wino_kernel<3,0,0> and <4,0,0>; rows 47 / 65 (48-row tiles), 63 / 97 (64-row tiles)
    _spatial("odd_m47_c17", S_ODD, 1, 47, 17, [("f23", {})]),
    _spatial("odd_m65_c16_k3", S_ODD, 3, 65, 16, [("f23", {})]),
    _spatial("odd_m63_c16", S_ODD, 1, 63, 16, [("f23", {})]),
    _spatial("odd_m97_c17_k3", S_ODD, 3, 97, 17, [("f23", {})]),
    _spatial("pair_m47_c16", S_PAIR, 1, 47, 16, [("f23", {})]),
    _spatial("pair_m63_c17", S_PAIR, 1, 63, 17, [("f23", {})]),
    # ---- W % 4 == 0: F(4,3) (five epilogues each) and, under ZSV_WINO_NO_F43, F(2,3) with X4; C = 49 at kT = 1 is 12 chunks: with
    # M = 47 and one K part the NCHUNKS = 12 symbols.  (Two K parts of that shape do not exist: a part needs >= 12 chunks, so
    # wino_ksplit answers 0 and the shape leaves these kernels; the run-time-count symbols <3,0,..> are reached by C = 16 and 17.)
    _spatial("504_m47_c49", S_504, 1, 47, 49, [F43, F23, F23_NO_X4]),
    _spatial("504_m65_c16_k3", S_504, 3, 65, 16, [F43, F23]),
    _spatial("504_m63_c17", S_504, 1, 63, 17, [F43, F23, F23_NO_X4]),
    _spatial("504_m97_c16_k3", S_504, 3, 97, 16, [F43, F23]),
    _spatial("row_m47_c17_k3", S_ROW, 3, 47, 17, [F43, F23]),
    _spatial("row_m63_c16", S_ROW, 1, 63, 16, [F43, F23]),
    _spatial("quad_m47_c16", S_QUAD, 1, 47, 16, [F43, F23]),
    _spatial("quad_m97_c17", S_QUAD, 1, 97, 17, [F43, F23]),
    # ---- K parts: C = 90 at kT = 3 is 54 chunks: parts of 27/27, 18/18/18, 14/14/14/12
    _spatial("ks_m47_c90_k3", S_504, 3, 47, 90, _ks_variants(S_504, 47, [F43, F23]), modes="splitk"),
    _spatial("ks_m97_c90_k3", S_ODD, 3, 97, 90, _ks_variants(S_ODD, 97, [("f23", {})]), modes="splitk"),
    # ---- virtual width: the nine admitted widths on (2, 16, 2, 3, W): nvalid = 1, 2, 3 at every Wv (below 512 workgroups the plan
    # always prefers 48-row tiles: rows x fill favours them)
    *[_spatial(f"vw{w}_m{m}_c16", (2, 2, 3, w), 1, m, 16, [("vw", {})]) for w, m in
      ((7, 47), (14, 65), (15, 63), (29, 97), (30, 47), (31, 65), (61, 63), (62, 97), (63, 47))],
    _spatial("vw7_partial_m65_c17", (3, 2, 7, 7), 1, 65, 17, [("vw", {})]),                  # 336 virtual voxels: a partial last tile
    # the K parts the plan picks at kT = 3: C = 16 -> 1, C = 48 -> 2, C = 96 -> 4 (test_wino_configs_host.py asserts these)
    _spatial("vw14_m47_c16_k3", (2, 2, 3, 14), 3, 47, 16, [("vw", {})]),
    _spatial("vw14_m47_c48_k3", (2, 2, 3, 14), 3, 47, 48, [("vw", {})], modes="splitk"),
    _spatial("vw7_m63_c96_k3", (2, 2, 3, 7), 3, 63, 96, [("vw", {})], modes="splitk"),
    # 64-row virtual-width tiles: the plan picks them only when 48-row tiles would overflow one round of 512 workgroups by little.
    # M = 64 on 272 column tiles: 272 workgroups of 64 rows (fill 0.53 x rows 1) against 544 of 48 rows (fill 0.77 x rows 0.67);
    # the smallest comfortable margin (the tie is at 257 tiles), 15 MB of output -- half the (8, 16, 16, 64, 14) the issue names.
    # Forward only: the five epilogues are all forward modes but +add, which the forward's residual covers.
    _spatial("vw14_m64_c16_big", (8, 8, 68, 14), 1, 64, 16, [("vw", {})], directions=("fwd",)),
    # ---- temporal: T = 4, 8, 16, 32; H x W = PW + 4 (a second segment with four live positions) and 2 x 2 (one ragged segment)
    _spatial("t4_17_m47_c17", (2, 4, 4, 17), "t", 47, 17, [T43, T23]),
    _spatial("t4_2x2_m63_c16", (2, 4, 2, 2), "t", 63, 16, [T43, T23]),
    _spatial("t8_6x6_m65_c16", (2, 8, 6, 6), "t", 65, 16, [T43, T23]),
    _spatial("t8_2x2_m97_c17", (2, 8, 2, 2), "t", 97, 17, [T43, T23]),
    _spatial("t16_4x5_m63_c49", (2, 16, 4, 5), "t", 63, 49, [T43, T23]),
    _spatial("t16_2x2_m47_c16", (2, 16, 2, 2), "t", 47, 16, [T43, T23]),
    _spatial("t32_3x4_m97_c16", (2, 32, 3, 4), "t", 97, 16, [T43]),
    _spatial("t32_2x2_m65_c17", (2, 32, 2, 2), "t", 65, 17, [T43]),
    # ---- the BatchNorm + ReLU prologue (zsv_conv3d_fwd_pre).  zsv_conv3d_pre_supported also asks for the weight gradient's frame ring
    # (wgrad_tring_shape): N * S >= 16384, H * W % 16 == 0, ceil64(Cout) <= 1.3 Cout, pad(Cin) <= 1.3 Cin.  So Cout = 63 (one ragged
    # 64-row tile) and Cout = 270 (six 48-row tiles, 18 dead rows: the smallest band where 48 rows pad less AND 64 rows pad <= 30 %),
    # Cin = 113 (an eighth block with one live channel) and 100; 33 segments at T = 4 (the last with 16 live positions of 64).
    _spatial("pre_t4_m63_c113", (2, 4, 16, 129), "t", 63, 113, [T43, T23], modes="pre", directions=("fwd",)),
    _spatial("pre_t16_m270_c100", (2, 16, 16, 33), "t", 270, 100, [T43, T23], modes="pre", directions=("fwd",)),
    _spatial("pre_t32_m63_c100", (2, 32, 8, 34), "t", 63, 100, [T43], modes="pre", directions=("fwd",)),
]
GENERIC_ENV = {"ZSV_WINO_GENERIC_EPILOGUE": "1", "ZSV_WINOT_GENERIC_EPILOGUE": "1"}
OFF_ENV = {"ZSV_NO_WINO": "1"}                                  # the direct kernels: the Winograd-off result


def by_name(name):
    return next(c for c in CASES if c.name == name)


def geometry(case, direction):
    n, t, h, w = case.shape
    kernel, padding = ((3, 1, 1), (1, 0, 0)) if case.kt == "t" else ((case.kt, 3, 3), (case.kt // 2, 1, 1))
    if direction == "fwd":
        return Geom((n, case.c, t, h, w), case.m, kernel, ONE, padding)
    return Geom((n, case.m, t, h, w), case.c, kernel, ONE, padding)


# The prologue cases sum ~340 products of relu(x * scale + shift) <= 6 per output: with weights 24 x [-2, 2] a tile's sum of y^2
# passes 2^30 (1.1e9 - 1.5e9), so their weights are 24 x {-1, 0, 1} (a third of the squares)
WEIGHT_AMP = {geometry(c, "fwd"): 1 for c in CASES if c.modes == "pre"}


def modes_of(case, direction):
    if case.modes == "pre":
        return PRE_MODES
    if direction == "dgrad":
        return [PLAIN] if case.modes == "splitk" else DGRAD_MODES
    return SPLITK_FWD_MODES if case.modes == "splitk" else FWD_MODES


def runs():
    """Every (case, direction, variant name, switches)."""
    return [(case, direction, vname, dict(BASE_ENV, **venv)) for case in CASES for direction in case.directions for vname, venv in case.variants]


def run_id(run):
    case, direction, vname, _ = run
    return f"{case.name}-{direction}-{vname}"


def launches(run):
    """Every (mode, switches) the GPU half launches for a run, generic-epilogue repeats included."""
    case, direction, _, env = run
    return [(mode, e) for mode in modes_of(case, direction) for e in (env, dict(env, **GENERIC_ENV))]


def switch_names():
    names = set(GENERIC_ENV) | set(OFF_ENV)
    for _, _, _, env in runs():
        names.update(env)
    return names


def form_of(g, direction, env):
    """(axis, outputs per tile) of the Winograd form a run takes: ("w" | "t", 2 | 4)."""
    m = rows_and_channels(g, direction)[0]
    if winot_geometry(g, m, env):
        return ("t", 2 if _knob(env, "WINOT_NO_F43") else 4)
    return ("w", 4 if wino_f43(g, env) else 2)


# ---- the Winograd algorithm, restated in fp64 -------------------------------------------------------------------------------------
BT = {2: [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
      4: [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]}
GG = {2: [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
      4: [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]}
AT = {2: [[1, 1, 1, 0], [0, 1, -1, -1]],
      4: [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]}


def winograd(inp, geff, axis, m, absolute=False):
    """F(m,3) along W (``axis`` "w": geff [M][C][kT][3][3], "same" padding) or along T ("t": geff [M][C][3][1][1]) of inp [N][C][T][H][W]
    in fp64: y = A . sum_{c, row taps} (U (.) B d).  ``absolute``: |A| . sum (|U| (.) |B| |d|), the bound on every intermediate."""
    bt, gg, at = (torch.tensor(t, dtype=torch.float64) for t in (BT[m], GG[m], AT[m]))
    if axis == "t":
        inp, geff = inp.permute(0, 1, 3, 4, 2), geff.permute(0, 1, 3, 4, 2)
    length = inp.shape[-1]
    nt = (length + m - 1) // m
    u = torch.einsum("mcabk,pk->mcabp", geff, gg)
    d = F.pad(inp.abs() if absolute else inp, (1, nt * m + 1 - length)).unfold(-1, m + 2, m)         # [N][C][A][B][nt][m + 2]
    if absolute:
        bt, at, u = bt.abs(), at.abs(), u.abs()
    v = torch.einsum("ncabtk,pk->ncabtp", d, bt)
    pad = (geff.shape[2] // 2, geff.shape[3] // 2, 0)
    mm = torch.stack([F.conv3d(v[..., p].contiguous(), u[..., p].unsqueeze(-1).contiguous(), None, 1, pad) for p in range(m + 2)], dim=-1)
    y = torch.einsum("nmabtp,jp->nmabtj", mm, at).flatten(-2)[..., :length]
    return y.permute(0, 1, 4, 2, 3).contiguous() if axis == "t" else y.contiguous()


def effective_weights(w, direction):
    """G[m][c][taps]: the weights, or for the input gradient the weights with flipped taps and swapped channel axes."""
    return w if direction == "fwd" else w.flip(2, 3, 4).transpose(0, 1).contiguous()


def _seed(g, direction, kind, salt):
    return B._seed(g, kind, f"wino {direction} {salt}")


def acc_length(g, direction):
    """L: padded reduction channels x row taps."""
    c = rows_and_channels(g, direction)[1]
    return (c + 15) // 16 * 16 * (1 if winot_shape(g) else 3 * g.kernel[0])


@functools.lru_cache(maxsize=None)
def operands(g, direction, kind):
    """inp (x, or dy for the input gradient), w, bias, add (residual / shortcut gradient), coef ([2][pitch] prologue scale and
    shift, zero padded), scale, shift of a launch as fp64 CPU tensors; the same for every caller."""
    gen = torch.Generator().manual_seed(_seed(g, direction, kind, "operands"))
    m, c = rows_and_channels(g, direction)
    n, _, t, h, w_ = g.xs
    in_shape, res_shape, wshape = (n, c, t, h, w_), (n, m, t, h, w_), (g.cout, g.xs[1]) + g.kernel
    ints = lambda s, amp: torch.randint(-amp, amp + 1, tuple(s), generator=gen).double()
    normal = lambda s: torch.randn(tuple(s), generator=gen, dtype=torch.float64).float().double()
    if kind == "exact":
        inp, w = fill_faces(gen, ints(in_shape, 2), 2), 24.0 * ints(wshape, WEIGHT_AMP.get(g, 2))
        bias, add = ints((m,), 50), ints(res_shape, 50)
        scale, shift = ints((c,), 2), ints((c,), 2)
        shift[0], scale[0] = 2.0, -1.0                       # a used channel with a positive shift: relu(shift) != 0 where x == 0
    else:
        inp, w, bias, add, scale, shift = normal(in_shape), normal(wshape), normal((m,)), normal(res_shape), normal((c,)), normal((c,))
    coef = torch.zeros(2, (c + 15) // 16 * 16, dtype=torch.float64)
    coef[0, :c], coef[1, :c] = scale, shift
    return {"inp": inp, "w": w, "bias": bias, "add": add, "coef": coef, "scale": scale, "shift": shift}


@functools.lru_cache(maxsize=None)
def raw_reference(g, direction, kind, form, pre=False):
    """z = conv3d(inp, G) in fp64 (``pre``: of relu(inp * scale + shift), padded frames contributing 0) and abs = the Winograd
    restatement of ``form`` on absolute values."""
    o = operands(g, direction, kind)
    geff = effective_weights(o["w"], direction)
    a, a_abs = o["inp"], o["inp"].abs()
    if pre:
        v = lambda t: t.view(1, -1, 1, 1, 1)
        a, a_abs = torch.relu(o["inp"] * v(o["scale"]) + v(o["shift"])), o["inp"].abs() * v(o["scale"]).abs() + v(o["shift"]).abs()
    z = F.conv3d(a, geff, None, 1, g.padding)
    return z, winograd(a_abs, geff, form[0], form[1], absolute=True)


@functools.lru_cache(maxsize=None)
def relu_bias(g, direction, kind, form, add):
    """The bias of a ReLU mode: ``normal``: redrawn per channel until no pre-activation lies within 4 bounds of 0."""
    o = operands(g, direction, kind)
    bias = o["bias"].clone()
    if kind == "exact":
        return bias
    z, z_abs = raw_reference(g, direction, kind, form)
    if add:
        z, z_abs = z + o["add"], z_abs + o["add"].abs()
    factor = 4 * (acc_length(g, direction) + C_ROUND) * U
    gen = torch.Generator().manual_seed(_seed(g, direction, kind, f"bias {add}"))
    for attempt in range(400):
        b = bias.view(1, -1, 1, 1, 1)
        near = ((z + b).abs() <= factor * (z_abs + b.abs())).permute(1, 0, 2, 3, 4).reshape(bias.numel(), -1).any(1)
        if not bool(near.any()):
            break
        # (a channel of many voxels leaves no gap of 8 bounds among its pre-activations where they are dense: after every 25
        # failures the draw widens by 2, towards their tails)
        redraw = torch.randn(bias.numel(), generator=gen, dtype=torch.float64).float().double() * float(2 ** (attempt // 25))
        bias = torch.where(near, redraw.float().double(), bias)
    return bias


def reference(g, direction, kind, form, mode):
    """fp64 reference of a mode: bias (or None), y, bound, z (pre-activation), raw (the convolution alone, which the statistics
    describe), raw_abs."""
    o = operands(g, direction, kind)
    raw, raw_abs = raw_reference(g, direction, kind, form, mode.pre)
    z, z_abs, bias = raw, raw_abs, None
    if mode.add:
        z, z_abs = z + o["add"], z_abs + o["add"].abs()
    if mode.bias:
        bias = relu_bias(g, direction, kind, form, mode.add) if mode.relu else o["bias"]
        z, z_abs = z + bias.view(1, -1, 1, 1, 1), z_abs + bias.abs().view(1, -1, 1, 1, 1)
    y = torch.relu(z) if mode.relu else z
    return {"bias": bias, "y": y, "z": z, "y_abs": z_abs, "bound": (acc_length(g, direction) + C_ROUND) * U * z_abs, "raw": raw, "raw_abs": raw_abs}


def tile_sums(t, g, env):
    """[M][tiles] sums of t [N][M][T][H][W] over the kernels' column tiles, in the order of the statistics arrays: temporal
    (clip, segment of 256 / T positions, all frames); spatial 256 consecutive voxels of the (virtual-width) rows."""
    n, m, tt, h, w = t.shape
    if winot_geometry(g, g.cout, env):
        pw, segs = 256 // tt, winot_segs(g)
        s = F.pad(t.reshape(n, m, tt, h * w), (0, segs * pw - h * w)).reshape(n, m, tt, segs, pw).sum(dim=(2, 4))
        return s.permute(1, 0, 2).reshape(m, n * segs)
    wv = wino_vw_width(g, env) or w
    flat = F.pad(t, (0, wv - w)).permute(1, 0, 2, 3, 4).reshape(m, -1)
    tiles = (flat.shape[1] + 255) // 256
    return F.pad(flat, (0, tiles * 256 - flat.shape[1])).reshape(m, tiles, 256).sum(2)


def stat_reference(g, kind, form, env, pre=False):
    """Per (channel, column tile) sum of y and of y^2 of the raw forward convolution, with their bounds (module docstring)."""
    raw, raw_abs = raw_reference(g, "fwd", kind, form, pre)
    lc = acc_length(g, "fwd") + C_ROUND
    s_abs, q_abs = tile_sums(raw_abs, g, env), tile_sums(raw_abs * raw_abs, g, env)
    return {"sum": tile_sums(raw, g, env), "sq": tile_sums(raw * raw, g, env), "sum_mag": tile_sums(raw.abs(), g, env),
            "sum_bound": (lc + 9) * U * s_abs, "sq_bound": (2 * lc + 10) * U * q_abs}


def assert_preconditions(g, direction, kind, form, mode, env):
    """The conditions under which the comparison of this launch is the one the module docstring derives."""
    o = operands(g, direction, kind)
    r = reference(g, direction, kind, form, mode)
    what = f"{tuple(g)} {direction} {kind} F({form[1]},3) along {form[0]} {mode.name}"
    if kind == "exact":
        assert faces_nonzero(o["inp"]), f"{what}: a border voxel is zero"
        assert bool((o["w"] / 24 == (o["w"] / 24).round()).all()), f"{what}: a weight is not a multiple of 24"
        for name in ("inp", "bias", "add", "scale", "shift"):
            assert bool((o[name] == o[name].round()).all()), f"{what}: {name} is not an integer"
        assert float(r["y_abs"].max()) < LIMIT, f"{what}: the absolute-value restatement reaches 2^24 ({float(r['y_abs'].max()):.3g})"
        if mode.pre:
            used = o["shift"] > 0
            assert bool(used.any()) and bool((o["w"][:, used] != 0).any()), f"{what}: no used channel has a positive shift"
        if mode.stats:
            s = stat_reference(g, kind, form, env, mode.pre)
            assert float(s["sum_mag"].max()) < LIMIT, f"{what}: a tile's sum of |y| reaches 2^24 ({float(s['sum_mag'].max()):.3g})"
            assert bool((r["raw"] / 8 == (r["raw"] / 8).round()).all()), f"{what}: an output is not a multiple of 8"
            assert float(s["sq"].max()) < SQ_LIMIT, f"{what}: a tile's sum of y^2 reaches 2^30 ({float(s['sq'].max()):.3g})"
    if mode.relu and kind == "normal":
        near = r["z"].abs() <= 4 * r["bound"]
        assert not bool(near.any()), f"{what}: {int(near.sum())} pre-activation(s) within 4 x the bound of 0"
