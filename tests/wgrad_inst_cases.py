"""The instantiation matrix of the specialised fp32 weight-gradient kernels (TEST INFRASTRUCTURE; never imported by the package, no
GPU import).  The third companion of ``conv_config_cases.py`` (whose helpers it reuses) after ``wino_cases.py``.

``zsv_conv3d_wgrad`` / ``zsv_conv3d_wgrad_pre`` pick among 21 kernel instantiations besides the register-staged and the plain
LDS-DMA kernels (which ``conv_config_cases.py`` covers): ``ALL_INSTANTIATIONS``.  Which one a shape reaches is decided by the host
planners restated below, one short function each (``tests/test_wgrad_inst_host.py`` checks them against the library's own answers
under every set of switches the matrix uses).  The matrix forces every instantiation on the smallest shapes the routes admit
(N * T * H * W >= 16384 and row padding <= 30 % for the Winograd and ring routes) that cross its edges;
``expected_instantiation`` says which (kernel, template arguments) a run reaches.

``BASE_ENV`` sets ZSV_WGRAD_WGS=1 and ZSV_WGRAD_DMA_SLICES=1 in every run: the workspace query is the maximum over the
register-staged kernel and every route the shape admits, and with these two the staged and the LDS-DMA share is ONE slab, so the
queried size is the forced route's own plan (its slice count and tile choice) and the host test can pin both.  Neither switch is read
by a planner of the kernels under test.

Operands of two kinds:

* ``exact``: x and dy are integers in [-2, 2] with non-zero voxels on the six faces of every clip, the prologue's scale and shift
  integers in [-2, 2].
  - plain kernels (frame ring, generic, stem, the dense problem under the fold): every product and partial sum is an integer; while
    conv3d_weight(|x|, |dy|) < 2^24 they are exactly representable whatever the order of addition, the slice count or the FMA
    contraction, and the result must equal the fp64 reference bit for bit (``torch.equal``).
  - F(2,3) forms (``conv_wgrad_wino_kernel`` along W, ``conv_wgrad_twino_kernel`` along T): A = (y0, y0+y1, y0-y1, y1), V = (d0-d2,
    d1+d2, d2-d1, d1-d3) are integers; the precondition is the algorithm restated on ABSOLUTE values, |A| = (|y0|, |y0|+|y1|,
    |y0|+|y1|, |y1|), |V| = (|d0|+|d2|, |d1|+|d2|, |d1|+|d2|, |d1|+|d3|), every |M_i| = sum |A_i| |V_i| and |M1| + |M2| (``emit``
    adds the two before halving) below 2^24.  M1 + M2 = 2 sum (y0 d2 + y1 d1) and M1 - M2 = 2 sum (y0 d1 + y1 d2) are even, so the
    halves are integers: bit for bit again.  It is NOT conv3d_weight(|x|, |dy|): the transforms amplify.
  - the bits do not depend on the slice count: every Winograd / ring run repeats under ZSV_WGRAD_WINO_SLICES / ZSV_WGRAD_TRING_SLICES
    = 1 and 7 and must give identical tensors (on exact sums a difference is a chunk that a slice lost or doubled).
  - F(4,3) (``conv_wgrad_wino4_kernel``) is the exception to bit equality.  Its six point sums are exact integers (A has coefficients
    1, 2, 4, 8, V = B^T d 1, 2, 4, 5; |M_i|, |M1|+|M2| and |M3|+|M4| below 2^24), but ``emit(float (&)[6])`` of wgrad_sum.hip then
    multiplies by the fp32 constants 1/6, 1/12 and 1/24, which are not representable.  Per term of an output, e.g. the m1 of
    0.25f * m0 - s12 * (1.f / 6.f) + s34 * (1.f / 24.f): s12 = m1 + m2 is exact, then 1 rounding of the constant, 1 of the product
    (0 when it is fused into the add), 1 for each of the two adds = 4, and 1 more for the second-order terms of (1 + u)^4:
    ``C_EMIT`` = 5, so |got - ref| <= C_EMIT * 2^-24 * emit(|M|) with emit(|M|) the transform on absolute values
    (0.25 |m0| + (|m1| + |m2|) / 6 + (|m3| + |m4|) / 24 and so on).  The slice-count invariance stays ``torch.equal``: the sums going
    into ``emit`` are the same integers.

* ``normal``: standard-normal fp32 values, per element |got - ref| <= (L + c) * 2^-24 * abs, and exactly 0 where the bound is 0.
  L is the number of products one accumulator takes: N * S voxels (plain kernels; the two dense sums of a fold's middle tap
  together), N * S / 2 pairs (F(2,3)) or N * S / 4 quads (F(4,3)) per Winograd point; ``abs`` is the same restatement on absolute
  values.  c = c1 + c2, with c1 counted from the code per term along the deepest path (``C_FIRST``):
    plain    0
    fold     1   t2_fold_kernel's a[0] + b[1]
    f23      4   A: y0 + y1 (1); V: d1 + d2 (1); emit: m1 + m2 (1), m0 + h (1) -- the halvings are exact
    f43      9   A: e = y0 + y2, e + o, or fma(4, y2, y0), fma(2, q, e4) (2); V: d1 + d2, fma(-4, ., .) (2); emit: s12 (1) + the 4 above
    + 1 under the prologue: fma(x, scale, shift), relative to |x| |scale| + |shift| (ReLU is 1-Lipschitz)
  and c2 = ceil(1.01 (L + c1)^2 2^-24) for the second-order terms: (1 + u)^k - 1 <= k u / (1 - k u) <= (k + 1.01 k^2 u) u while
  k u <= 2^-9 (k <= 32768, asserted).  Slices: a slice's accumulator takes L / s products instead of L and the ordered slab sum
  (8 groups, then the 8 partials) adds ceil(s / 8) + 7 roundings per term; s <= 4096 and s >= 2 saves L / 2 >= 2048 of them on the
  Winograd and ring routes (L >= 4096), so L bounds every slice count.  The generic and stem rows have at most 12 slabs.

Nothing is fitted; ``assert_preconditions`` asserts every condition on the CPU.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F
from torch.nn.grad import conv3d_weight

import conv_config_cases as B
from conv_config_cases import Geom, KINDS, LIMIT, U, align256, check, faces_nonzero, fill_faces, knob_list, operands, out_shape  # noqa: F401

ONE = (1, 1, 1)
AMP = 2                                                      # exact operands: integers in [-AMP, AMP]
C_EMIT = 5
C_FIRST = {"plain": 0, "fold": 1, "f23w": 4, "f23t": 4, "f43w": 9}

# ---- the 21 instantiations (bool template arguments as 0 / 1) ----------------------------------------------------------------------
ALL_INSTANTIATIONS = (
    [("conv_wgrad_wino_kernel", (tm, tn, e)) for tm, tn in ((9, 1), (8, 1), (4, 2)) for e in (0, 1)] +
    [("conv_wgrad_wino4_kernel", t) for t in ((5, 4), (4, 4))] +
    [("conv_wgrad_tring_kernel", (tm, p)) for tm in (9, 8) for p in (0, 1)] +
    [("conv_wgrad_twino_kernel", (tm, p)) for tm in (9, 8) for p in (0, 1)] +
    [("conv_wgrad_generic_kernel", t) for t in ((4, 4, 2, 2), (4, 2, 1, 4), (9, 1, 1, 4))] +
    [("stem_wgrad_kernel", ()), ("t2_fold_kernel", ())])
FAMILIES = sorted({k for k, _ in ALL_INSTANTIATIONS})
FORM_OF_KERNEL = {"conv_wgrad_wino_kernel": "f23w", "conv_wgrad_wino4_kernel": "f43w", "conv_wgrad_tring_kernel": "plain",
                  "conv_wgrad_twino_kernel": "f23t", "conv_wgrad_generic_kernel": "plain", "stem_wgrad_kernel": "plain",
                  "t2_fold_kernel": "fold"}


# ---- restated planners (csrc/wgrad_plan.h, conv_wgrad*.hip, host side) ---------------------------------------------------------------
def _knob(env, name):
    return env.get("ZSV_" + name)


def _dims(g):
    n, cin, t, h, w = g.xs
    return n, cin, t, h, w, t * h * w


def rows_144_or_128(n):
    """The row tile, 144 or 128, that pads ``n`` rows less (144 on ties)."""
    return 144 if (n + 143) // 144 * 144 <= (n + 127) // 128 * 128 else 128


def pad_144_or_128(n):
    t = rows_144_or_128(n)
    return (n + t - 1) // t * t


def clamp1(v, cap):
    return 1 if v < 1 else min(v, cap)


def slices_by_cost(tiles, resident, t_mfma, t_slice, max_slices):
    """The count that minimises MFMA time / round fill + slab traffic per slice; fewer unless more gain 0.1 %."""
    sl, best = 1, 1e300
    for c in range(1, max_slices + 1):
        wgs = tiles * c
        rounds = (wgs + resident - 1) // resident
        cost = t_mfma * float(rounds * resident) / float(wgs) + t_slice * float(c)
        if cost < best * 0.999:
            best, sl = cost, c
    return sl


def split_chunks(chunks, slices):
    """(chunks per slice, slices that are not empty)."""
    per = (chunks + slices - 1) // slices
    return per, (chunks + per - 1) // per


def same_stride1(g, kernel):
    return g.kernel == kernel and g.stride == ONE and g.padding == tuple(k // 2 for k in kernel)


def wgrad_wino_shape(g, env):
    n, cin, t, h, w, s = _dims(g)
    if _knob(env, "NO_WINO") or _knob(env, "NO_WGRAD_WINO") or not (same_stride1(g, (1, 3, 3)) or same_stride1(g, (3, 3, 3))):
        return False
    if w % 2 != 0 or cin < 16 or s % 4 != 0 or n * cin * s >= 1 << 29 or n * g.cout * s >= 1 << 29:
        return False
    pm = 64 if g.cout <= 64 else pad_144_or_128(g.cout)
    return pm * 10 <= g.cout * 13 and n * s >= 16384


def wgrad_wino4_shape(g):
    return g.xs[4] % 4 == 0 and _dims(g)[5] % 32 == 0 and g.cout > 64


def wgrad_wino_edge(g):
    """EDGE: a partial last chunk or X pieces that are only dword aligned."""
    return _dims(g)[5] % 32 != 0 or g.xs[4] % 4 != 0


Plan = namedtuple("Plan", "tm tn tiles_m tiles_n slices per_slice")


def _wino_slices(g, env, tiles, resident, macs_factor, points, kp, chunks):
    t_mfma = macs_factor * float(chunks * 32) / 1.1e14
    t_slice = 2.0 * points * float(g.cout) * kp * 4 / 6.0e12
    sl = slices_by_cost(tiles, resident, t_mfma, t_slice, clamp1(chunks // 24, 4096))
    if _knob(env, "WGRAD_WINO_SLICES"):
        sl = int(_knob(env, "WGRAD_WINO_SLICES"))
    return split_chunks(chunks, clamp1(sl, chunks))


def wgrad_wino_plan(g, env):
    """F(2,3): 64 rows x 128 columns up to 64 output channels, else 144 or 128 rows x 64 columns; two workgroups per CU."""
    n, cin, t, h, w, s = _dims(g)
    kp = 3 * g.kernel[0] * ((cin + 15) // 16 * 16)
    tm = 4 if g.cout <= 64 else rows_144_or_128(g.cout) // 16
    tn = 2 if tm == 4 else 1
    bm, bn = 16 * tm, 64 * tn
    tiles_m, tiles_n = (g.cout + bm - 1) // bm, (kp + bn - 1) // bn
    chunks = n * ((s + 31) // 32)
    per, slices = _wino_slices(g, env, tiles_m * tiles_n, 512, 4.0 * float(tiles_m * bm) * float(tiles_n * bn), 4.0, kp, chunks)
    return Plan(tm, tn, tiles_m, tiles_n, slices, per)


def wgrad_wino4_plan(g, env):
    """F(4,3): 144 (5 + 4 blocks) or 128 (4 + 4) rows x 64 columns, one eight-wave workgroup per CU."""
    n, cin, t, h, w, s = _dims(g)
    kp = 3 * g.kernel[0] * ((cin + 15) // 16 * 16)
    tma = 5 if rows_144_or_128(g.cout) == 144 else 4
    bm = 16 * (tma + 4)
    tiles_m, tiles_n = (g.cout + bm - 1) // bm, (kp + 63) // 64
    chunks = n * (s // 32)
    per, slices = _wino_slices(g, env, tiles_m * tiles_n, 256, 3.0 * float(tiles_m * bm) * float(tiles_n * 64), 6.0, kp, chunks)
    return Plan(tma, 4, tiles_m, tiles_n, slices, per)


def wgrad_wino_workspace_bytes(g, env):
    """The larger of the two forms' slabs (the F(4,3) knob may change between the query and the call) + the tap-validity table."""
    n, cin, t, h, w, s = _dims(g)
    kp = 3 * g.kernel[0] * ((cin + 15) // 16 * 16)
    slabs = align256(wgrad_wino_plan(g, env).slices * 4 * g.cout * kp * 4)
    if wgrad_wino4_shape(g):
        slabs = max(slabs, align256(wgrad_wino4_plan(g, env).slices * 6 * g.cout * kp * 4))
    return slabs + s * 4


def wgrad_tring_shape(g, env):
    n, cin, t, h, w, s = _dims(g)
    if _knob(env, "NO_WGRAD_TRING") or not same_stride1(g, (3, 1, 1)):
        return False
    if t % 4 != 0 or (h * w) % 16 != 0 or g.cout < 32 or n * cin * s >= 1 << 29 or n * g.cout * s >= 1 << 29:
        return False
    return pad_144_or_128(cin) * 10 <= cin * 13 and (g.cout + 63) // 64 * 64 * 10 <= g.cout * 13 and n * s >= 16384


def wgrad_twino_shape(g, env):
    return g.xs[2] >= 8 and not _knob(env, "NO_WGRAD_TWINO")


def wgrad_tring_tiles(g):
    """(tm, row tiles of input channels, 64-column tiles of output channels)."""
    tm = rows_144_or_128(g.xs[1]) // 16
    return tm, (g.xs[1] + 16 * tm - 1) // (16 * tm), (g.cout + 63) // 64


def _tring_forced(env):
    e = _knob(env, "WGRAD_TRING_SLICES")
    return None if not e else (int(e) if int(e) > 0 else 1)


def wgrad_tring_plan(g, env):
    n, cin, t, h, w, s = _dims(g)
    tm, tiles_m, tiles_n = wgrad_tring_tiles(g)
    chunks = n * t * (h * w // 16)
    t_mfma = 2.0 * float(tiles_m * 16 * tm) * float(tiles_n * 192) * float(chunks) * 16.0 / 1.1e14
    t_slice = 2.0 * float(cin) * 3.0 * g.cout * 4 / 6.0e12
    sl = slices_by_cost(tiles_m * tiles_n, 512 if tm == 9 else 768, t_mfma, t_slice, clamp1(chunks // 32, 4096))
    if _tring_forced(env) is not None:
        sl = _tring_forced(env)
    per, slices = split_chunks(chunks, min(sl, chunks))
    return Plan(tm, 3, tiles_m, tiles_n, slices, per)


def wgrad_twino_plan(g, env):
    """Chunks are frame pairs; the slices take whole (clip, segment) jobs and the count is taken as it is."""
    n, cin, t, h, w, s = _dims(g)
    tm, tiles_m, tiles_n = wgrad_tring_tiles(g)
    chunks, jobs = n * (t // 2) * (h * w // 16), n * (h * w // 16)
    t_mfma = 2.0 * float(tiles_m * 16 * tm) * float(tiles_n * 256) * float(chunks) * 16.0 / 1.1e14
    t_slice = 2.0 * float(cin) * 4.0 * g.cout * 4 / 6.0e12
    sl = slices_by_cost(tiles_m * tiles_n, 512, t_mfma, t_slice, clamp1(chunks // 16, 4096))
    if _tring_forced(env) is not None:
        sl = _tring_forced(env)
    sl = min(sl, jobs)
    return Plan(tm, 4, tiles_m, tiles_n, sl, (jobs + sl - 1) // sl * (t // 2))


def wgrad_tring_workspace_bytes(g, env):
    need = wgrad_tring_plan(g, env).slices * g.xs[1] * 3 * g.cout * 4
    if g.xs[2] >= 8:                                       # (the Winograd form may be chosen at call time)
        need = max(need, wgrad_twino_plan(g, env).slices * g.xs[1] * 4 * g.cout * 4)
    return need


def wgrad_dma_shape(g, env):
    """The plain LDS-DMA route, third in the order (never reached by the matrix; its share of the workspace query is one slab)."""
    n, cin, t, h, w, s = _dims(g)
    taps = g.kernel[0] * g.kernel[1] * g.kernel[2]
    if _knob(env, "NO_WGRAD_DMA") or cin < 16 or g.cout < 16 or g.stride != ONE or tuple(out_shape(g)[2:]) != (t, h, w):
        return False
    return s % 16 == 0 and taps <= 32 and taps * ((cin + 15) // 16 * 16) >= 256 and n * cin * s < 1 << 31 and n * g.cout * s < 1 << 31


def wgrad_gen_plan(g):
    """(cfg, Plan) of the Cin < 16 kernel: 64 x 128 up to 64 output channels, 144 x 64 for 129..144 or a multiple of 144, else 128 x 128."""
    m, k = g.cout, g.xs[1] * g.kernel[0] * g.kernel[1] * g.kernel[2]
    o = out_shape(g)
    p = o[0] * o[2] * o[3] * o[4]
    if m <= 64:
        cfg, inst, bm, bn = 1, (4, 2, 1, 4), 64, 128
    elif m % 144 == 0 or 128 < m <= 144:
        cfg, inst, bm, bn = 2, (9, 1, 1, 4), 144, 64
    else:
        cfg, inst, bm, bn = 0, (4, 4, 2, 2), 128, 128
    tiles_m, tiles_n = (m + bm - 1) // bm, (k + bn - 1) // bn
    chunks = (p + 31) // 32
    tiles = tiles_m * tiles_n
    slices = min((1536 + tiles - 1) // tiles, max((chunks + 15) // 16, 1))       # ~6 workgroups per CU, >= 16 chunks per slice
    per, slices = split_chunks(chunks, min(max(slices, 1), 1024))
    return inst, Plan(inst[0], inst[1], tiles_m, tiles_n, slices, per)


def stem_wgrad_shape(g, env):
    n, cin, t, h, w, s = _dims(g)
    o = out_shape(g)
    if _knob(env, "NO_STEM_WGRAD") or cin != 3 or g.kernel != (1, 7, 7) or g.stride != (1, 2, 2) or g.padding != (0, 3, 3):
        return False
    if h % 2 != 0 or w % 4 != 0 or o[4] != w // 2 or o[3] != h // 2 or o[4] % 4 != 0 or o[4] > 64 or not 1 <= g.cout <= 48:
        return False
    return n * g.cout * o[2] * o[3] * o[4] < 1 << 29 and n * 3 * s < 1 << 29


def stem_wgrad_parts(g, env):
    """Workgroups per frame: ~1408 in all, at least 8 output rows each, an even split of the rows where one is near."""
    o = out_shape(g)
    frames, ho = o[0] * o[2], o[3]
    e = _knob(env, "STEM_WGRAD_WGS")
    target = int(e) if e and int(e) > 0 else 1408
    parts = max(min((target + frames - 1) // frames, (ho + 7) // 8), 1)
    q = parts
    while q * 2 > parts and q >= 1:
        if ho % q == 0:
            parts = q
            break
        q -= 1
    rows = (ho + parts - 1) // parts
    return (ho + rows - 1) // rows


def wgrad_generic_workspace_bytes(g, env):
    _, pl = wgrad_gen_plan(g)
    k = g.xs[1] * g.kernel[0] * g.kernel[1] * g.kernel[2]
    gen = pl.slices * g.cout * k * 4 if pl.slices > 1 else 0
    if not stem_wgrad_shape(g, env):
        return gen
    o = out_shape(g)
    return max(gen, (o[0] * o[2] * stem_wgrad_parts(g, env) + 32) * g.cout * 147 * 4)      # the workgroups' slabs + 32 partial sums


def t2_dense_shape(g, env):
    return not _knob(env, "NO_T2_DENSE") and same_stride1(g, (3, 1, 1)) and g.xs[2] == 2 and g.xs[1] >= 16 and g.cout >= 16


def t2_dense_geom(g):
    """The dense 1x1x1 problem over (channel, frame) pairs."""
    n, cin, _, h, w = g.xs
    return Geom((n, 2 * cin, 1, h, w), 2 * g.cout, ONE, ONE, (0, 0, 0))


def route(g, env):
    """The route order of zsv_conv3d_wgrad: the t2 fold first, generic / stem for Cin < 16, then wino -> tring -> dma -> staged."""
    if t2_dense_shape(g, env):
        return "t2"
    if g.xs[1] < 16:
        return "stem" if stem_wgrad_shape(g, env) else "generic"
    for name, shape in (("wino", wgrad_wino_shape), ("tring", wgrad_tring_shape), ("dma", wgrad_dma_shape)):
        if shape(g, env):
            return name
    return "staged"


def workspace_bytes(g, env):
    """zsv_conv3d_wgrad_workspace_bytes under BASE_ENV (one staged slab, one LDS-DMA slab: module docstring)."""
    assert _knob(env, "WGRAD_WGS") == "1" and _knob(env, "WGRAD_DMA_SLICES") == "1"
    n, cin, t, h, w, s = _dims(g)
    if t2_dense_shape(g, env):
        return align256(4 * g.cout * cin * 4) + workspace_bytes(t2_dense_geom(g), env)
    if cin < 16:
        return wgrad_generic_workspace_bytes(g, env)
    kp = g.kernel[0] * g.kernel[1] * g.kernel[2] * ((cin + 15) // 16 * 16)
    need = g.cout * kp * 4
    if wgrad_wino_shape(g, env):
        need = max(need, wgrad_wino_workspace_bytes(g, env))
    if wgrad_tring_shape(g, env):
        need = max(need, wgrad_tring_workspace_bytes(g, env))
    if wgrad_dma_shape(g, env):
        need = max(need, align256(g.cout * kp * 4) + s * 4)
    return need


def mask_bytes(g, env):
    """zsv_conv3d_wgrad_mask_bytes: the first admitted route reads the per-voxel tap-validity table."""
    return 4 * _dims(g)[5] if route(g, env) in ("wino", "dma") else 0


def pre_supported(g, env):
    """zsv_conv3d_pre_supported, the weight gradient's half: the frame ring admits the shape (the forward's half is the other two
    matrices' business; every temporal row of this matrix has it)."""
    return not _knob(env, "NO_BN_FUSION") and route(g, env) == "tring"


def expected_instantiation(g, env, pre=False):
    """(kernel name, template arguments) of the launch under test."""
    r = route(g, env)
    if r == "t2":
        return ("t2_fold_kernel", ())
    if r == "stem":
        return ("stem_wgrad_kernel", ())
    if r == "generic":
        return ("conv_wgrad_generic_kernel", wgrad_gen_plan(g)[0])
    if r == "wino":
        if wgrad_wino4_shape(g) and not _knob(env, "NO_WGRAD_WINO4"):
            return ("conv_wgrad_wino4_kernel", (wgrad_wino4_plan(g, env).tm, 4))
        pl = wgrad_wino_plan(g, env)
        return ("conv_wgrad_wino_kernel", (pl.tm, pl.tn, int(wgrad_wino_edge(g))))
    if r == "tring":
        name = "conv_wgrad_twino_kernel" if wgrad_twino_shape(g, env) else "conv_wgrad_tring_kernel"
        return (name, (wgrad_tring_tiles(g)[0], int(pre)))
    return None


def planned_slices(g, env):
    """Slices of the launch under test (Winograd and ring routes)."""
    inst = expected_instantiation(g, env)
    plan = {"conv_wgrad_wino_kernel": wgrad_wino_plan, "conv_wgrad_wino4_kernel": wgrad_wino4_plan,
            "conv_wgrad_tring_kernel": wgrad_tring_plan, "conv_wgrad_twino_kernel": wgrad_twino_plan}[inst[0]]
    return plan(g, env).slices


# ---- rows ------------------------------------------------------------------------------------------------------------------------
# variants: (name, switches); pre: the row also runs through zsv_conv3d_wgrad_pre; slices: the switch that forces the slice count
Row = namedtuple("Row", "name geom variants pre slices")
BASE_ENV = {"ZSV_WGRAD_WGS": "1", "ZSV_WGRAD_DMA_SLICES": "1"}
DEFAULT = ("default", {})
F23 = ("f23", {"ZSV_NO_WGRAD_WINO4": "1"})
RING = ("ring", {"ZSV_NO_WGRAD_TWINO": "1"})
FORCED_SLICES = (1, 7)


def _spatial(name, xs, cout, variants, kt=1):
    return Row(name, Geom(xs, cout, (kt, 3, 3), ONE, (kt // 2, 1, 1)), list(variants), False, "ZSV_WGRAD_WINO_SLICES")


def _temporal(name, xs, cout):
    variants = [("wino", {}), RING] if xs[2] >= 8 else [DEFAULT]
    return Row(name, Geom(xs, cout, (3, 1, 1), ONE, (1, 0, 0)), variants, True, "ZSV_WGRAD_TRING_SLICES")


def _other(name, geom, variants=(DEFAULT,)):
    return Row(name, geom, list(variants), False, None)


S32, E14 = (4, 17, 4, 32, 32), (21, 17, 4, 14, 14)          # Cin = 17: Cpad = 32, 15 dead channels, a half-empty second column tile
GEN_SMALL, GEN_SLICED = (2, 5, 2, 9, 11), (2, 5, 4, 16, 16)
STEM = lambda xs, cout: Geom(xs, cout, (1, 7, 7), (1, 2, 2), (0, 3, 3))      # noqa: E731
ROWS = [
    # ---- Winograd forms along W, 1x3x3 "same"
    _spatial("s32_m50", S32, 50, [DEFAULT]),                            # wino<4,2,false>: a ragged 64-row tile
    _spatial("s32_m100", S32, 100, [DEFAULT, F23]),                     # wino4<4,4>; wino<8,1,false>
    _spatial("s32_m130", S32, 130, [DEFAULT, F23]),                     # wino4<5,4>; wino<9,1,false>
    _spatial("s32_m197", S32, 197, [DEFAULT, F23]),                     # two 128-row tiles, 69 live rows in the second
    _spatial("s32_m257", S32, 257, [DEFAULT, F23]),                     # two 144-row tiles, 113 live rows in the second
    _spatial("e14_m130", E14, 130, [DEFAULT]),                          # wino<9,1,true>: W % 4 == 2, S = 784: a partial last chunk
    _spatial("e14_m50", E14, 50, [DEFAULT]),                            # wino<4,2,true>
    _spatial("e20x12_m100", (23, 16, 3, 20, 12), 100, [DEFAULT]),       # wino<8,1,true>: S = 720, W % 4 == 0: EDGE by the chunk alone
    _spatial("s32_k3_m130", S32, 130, [DEFAULT, F23], kt=3),            # nine row taps
    _spatial("t2_k3_m100", (8, 16, 2, 32, 32), 100, [DEFAULT, F23], kt=3),      # nine row taps, every voxel on a temporal border
    # ---- temporal 3x1x1: frame ring (T = 4, or ZSV_NO_WGRAD_TWINO) and its Winograd form (T >= 8), each with and without the prologue
    _temporal("t4_c100", (1, 100, 4, 64, 64), 100),                     # tring<8,.>
    _temporal("t4_c130", (1, 130, 4, 64, 64), 100),                     # tring<9,.>
    _temporal("t8_c100", (1, 100, 8, 32, 64), 100),                     # twino<8,.>
    _temporal("t8_c130", (1, 130, 8, 32, 64), 100),                     # twino<9,.>
    _temporal("t4_c197_m50", (1, 197, 4, 64, 64), 50),                  # two row tiles of 128, a ragged 64-column tile
    _temporal("t4_c257_m50", (1, 257, 4, 64, 64), 50),                  # two row tiles of 144
    _temporal("t4_clips256", (256, 100, 4, 4, 4), 50),                  # one 16-position segment per frame: every slice boundary a clip boundary
    _temporal("t4_clips16", (16, 100, 4, 16, 16), 50),
    # ---- Cin < 16: one slice written straight to dw without a workspace; several slices
    *[_other(f"gen_small_m{m}", Geom(GEN_SMALL, m, (3, 3, 3), ONE, (1, 1, 1))) for m in (45, 80, 144)],
    *[_other(f"gen_sliced_m{m}", Geom(GEN_SLICED, m, (3, 3, 3), ONE, (1, 1, 1))) for m in (45, 80, 144)],
    # ---- the stem's row kernel: one part per frame (all a four-row frame has); two parts and one part forced
    _other("stem_tiny", STEM((1, 3, 1, 8, 8), 45)),
    _other("stem_m20", STEM((2, 3, 3, 24, 40), 20), [("parts2", {"ZSV_STEM_WGRAD_WGS": "1408"}), ("parts1", {"ZSV_STEM_WGRAD_WGS": "1"})]),
    # ---- the two-frame fold over the dense 1x1x1 problem
    _other("t2_whole", Geom((3, 64, 2, 8, 8), 48, (3, 1, 1), ONE, (1, 0, 0))),
    _other("t2_ragged", Geom((2, 45, 2, 5, 6), 70, (3, 1, 1), ONE, (1, 0, 0))),
]
Run = namedtuple("Run", "row vname env pre")


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def runs():
    """Every (row, variant, switches, prologue?)."""
    return [Run(row, vname, dict(BASE_ENV, **venv), pre) for row in ROWS for vname, venv in row.variants
            for pre in ((False, True) if row.pre else (False,))]


def run_id(run):
    return f"{run.row.name}-{run.vname}-{'pre' if run.pre else 'plain'}"


def switch_names():
    names = set(BASE_ENV)
    for row in ROWS:
        if row.slices:
            names.add(row.slices)
        for _, venv in row.variants:
            names.update(venv)
    return names


# ---- the Winograd forms of the weight gradient, restated in fp64 ----------------------------------------------------------------------
# A = YA y (the kernels' own signs), V = BT d, M_p = sum A_p V_p, dW = GT M
YA = {2: [[1, 0], [1, 1], [1, -1], [0, 1]],
      4: [[1, 0, 0, 0], [1, 1, 1, 1], [1, -1, 1, -1], [1, 2, 4, 8], [1, -2, 4, -8], [0, 0, 0, 1]]}
BT = {2: [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
      4: [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]}
GT = {2: [[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, -1]],
      4: [[1 / 4, -1 / 6, -1 / 6, 1 / 24, 1 / 24, 0], [0, -1 / 6, 1 / 6, 1 / 12, -1 / 12, 0], [0, -1 / 6, -1 / 6, 1 / 6, 1 / 6, 1]]}


def winograd_wgrad(x, dy, g, axis, m, absolute=False):
    """The transpose of F(m,3) along W (``axis`` "w", 1x3x3 / 3x3x3 "same") or along T ("t", 3x1x1) in fp64: (dW [Cout][Cin][taps],
    peak).  ``absolute``: |GT| . sum (|YA| |y|) (|BT| |d|), the bound on every intermediate; ``peak`` is then the largest value an
    fp32 intermediate of the exact kind can reach: every |M_p| and the pair sums |M1| + |M2| (, |M3| + |M4|) that emit forms."""
    ya, bt, gt = (torch.tensor(t, dtype=torch.float64) for t in (YA[m], BT[m], GT[m]))
    if absolute:
        x, dy, ya, bt, gt = x.abs(), dy.abs(), ya.abs(), bt.abs(), gt.abs()
    if axis == "t":
        x, dy = x.permute(0, 1, 3, 4, 2), dy.permute(0, 1, 3, 4, 2)
        kernel, pad = (1, 1, 1), (0, 0, 0)
    else:
        kernel, pad = (g.kernel[0], 3, 1), (g.kernel[0] // 2, 1, 0)
    assert x.shape[-1] % m == 0
    d = F.pad(x, (1, 1)).unfold(-1, m + 2, m)                                  # [N][C][.][.][q][m + 2]
    y = dy.contiguous().unfold(-1, m, m)
    v, a = torch.einsum("ncabqk,pk->pncabq", d, bt).contiguous(), torch.einsum("ncabqk,pk->pncabq", y, ya).contiguous()
    mm = torch.stack([conv3d_weight(v[p], (g.cout, g.xs[1]) + kernel, a[p], 1, pad) for p in range(m + 2)])    # [P][Cout][Cin][.][.][1]
    dw = torch.einsum("pmcab,kp->mcabk", mm[..., 0], gt)
    peak = max(float(mm.max()), float((mm[1] + mm[2]).max()), float((mm[3] + mm[4]).max()) if m == 4 else 0.0)
    return (dw.permute(0, 1, 4, 2, 3) if axis == "t" else dw).contiguous(), peak


FORMS = {"f23w": ("w", 2, 2), "f43w": ("w", 4, 4), "f23t": ("t", 2, 2)}              # form -> (axis, m, voxels per product)


def form_of(g, env, pre=False):
    return FORM_OF_KERNEL[expected_instantiation(g, env, pre)[0]]


@functools.lru_cache(maxsize=None)
def pre_coef(g, kind):
    """scale, shift and coef ([2][pitch]: scale row, shift row, zero padded; pitch = Cin rounded up to 16) of the prologue."""
    gen = torch.Generator().manual_seed(B._seed(g, kind, "wgrad pre"))
    cin = g.xs[1]
    if kind == "exact":
        scale, shift = (torch.randint(-2, 3, (cin,), generator=gen).double() for _ in range(2))
        scale[0], shift[0] = -1.0, 2.0                       # a channel with a positive shift: relu(shift) != 0 where x == 0
    else:
        scale, shift = (torch.randn(cin, generator=gen).float().double() for _ in range(2))
    coef = torch.zeros(2, (cin + 15) // 16 * 16, dtype=torch.float64)
    coef[0, :cin], coef[1, :cin] = scale, shift
    return scale, shift, coef


def activation(g, kind):
    """relu(x * scale + shift) in fp64 and |x| |scale| + |shift|."""
    x = operands(g, kind, amp=AMP)[0]
    scale, shift, _ = pre_coef(g, kind)
    v = lambda t: t.view(1, -1, 1, 1, 1)                     # noqa: E731
    return torch.relu(x * v(scale) + v(shift)), x.abs() * v(scale).abs() + v(shift).abs()


def acc_length(g, form):
    """L: the products one accumulator takes."""
    o = out_shape(g)
    return o[0] * o[2] * o[3] * o[4] // (FORMS[form][2] if form in FORMS else 1)


def c_round(g, form, pre):
    k = acc_length(g, form) + C_FIRST[form] + int(pre)
    assert k <= 32768
    return C_FIRST[form] + int(pre) + math.ceil(1.01 * k * k * U)


@functools.lru_cache(maxsize=6)
def reference(g, kind, form, pre=False):
    """dw: conv3d_weight in fp64 (``pre``: of relu(x * scale + shift)); abs: the form's restatement on absolute values; peak: the
    largest intermediate of the exact kind; bound: None where the comparison is ``torch.equal``."""
    x, _, _, _, dy = operands(g, kind, amp=AMP)
    a, a_abs = activation(g, kind) if pre else (x, x.abs())
    dw = conv3d_weight(a, (g.cout, g.xs[1]) + g.kernel, dy, g.stride, g.padding)
    if form in FORMS:
        dw_abs, peak = winograd_wgrad(a_abs, dy, g, FORMS[form][0], FORMS[form][1], absolute=True)
    else:
        dw_abs = conv3d_weight(a_abs, (g.cout, g.xs[1]) + g.kernel, dy.abs(), g.stride, g.padding)
        peak = float(dw_abs.max())
    if kind == "exact":
        bound = C_EMIT * U * dw_abs if form == "f43w" else None
    else:
        bound = (acc_length(g, form) + c_round(g, form, pre)) * U * dw_abs
    return {"dw": dw, "abs": dw_abs, "peak": peak, "bound": bound}


def compare(name, got, ref, kind):
    """``check`` of conv_config_cases: bit for bit where the reference has no bound, else per element within it."""
    return check(name, got, ref["dw"], ref["bound"], "exact" if ref["bound"] is None else "normal")


def assert_preconditions(g, kind, form, pre=False):
    """The conditions under which the comparison of a launch is the one the module docstring derives."""
    x, _, _, _, dy = operands(g, kind, amp=AMP)
    what = f"{tuple(g)} {kind} {form}{' pre' if pre else ''}"
    if kind != "exact":
        return
    r = reference(g, kind, form, pre)
    assert faces_nonzero(x) and faces_nonzero(dy), f"{what}: a border voxel is zero"
    for t in (x, dy) + (pre_coef(g, kind)[:2] if pre else ()):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= AMP, f"{what}: an operand is not an integer in [-{AMP}, {AMP}]"
    assert r["peak"] < LIMIT, f"{what}: the absolute-value restatement reaches 2^24 ({r['peak']:.3g})"
    assert bool((r["dw"] == r["dw"].round()).all()), f"{what}: the reference is not an integer"
    if pre:
        scale, shift, _ = pre_coef(g, kind)
        assert bool((shift > 0).any()), f"{what}: no channel has a positive shift"
