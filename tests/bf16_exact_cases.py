"""Exactly representable operands for the bf16 kernels (TEST INFRASTRUCTURE; never imported by the package, no GPU import).

The bf16 kernels multiply bf16 operands and accumulate in fp32.  Take every operand as an integer multiple of ``2^-q`` and keep
the sum of the absolute values of all terms of an output, counted in units of ``2^-q``, below ``2^24``: then every partial sum,
in every order (MFMA blocks, split slices, fixed-order block sums), is an integer below ``2^24`` in that unit and therefore an
fp32 number.  fp32 accumulation is EXACT, the fp32 result is the one right answer, and a bf16 store of it has one correct
round-to-nearest-even code.  The comparison is ``torch.equal``: a lost product changes an integer, a wrong tie direction flips
a bit.  No tolerance is derived anywhere in this file.

What is here:
* seeded generators of such operands (``forward_operands``, ``stats_operands``, ``dgrad_operands``, ``wgrad_operands``):
  activations and upstream gradients are small integers, weights integers times a per-channel power of two, shifts multiples
  of 1/8, residuals multiples of 1/2 -- all exact in bf16.  The voxels on the six faces of every clip are drawn non-zero, so a
  lost border voxel cannot hide behind a zero product;
* the float64 reference of each op on the CPU (``F.conv3d`` / ``torch.nn.grad`` in double: exact on these grids) together with
  ``sum |terms|`` (the same op on absolute values);
* ``assert_exact_in_fp32`` (the precondition), ``rne_bf16`` (the expected bits), ``rounding_profile`` (what share of the outputs
  needs rounding at all, and how many exact ties there are in each direction) and ``assert_same_values`` (the comparison);
* the case tables: the geometries of ``test_bf16_gpu.py`` (CASES, NINE_TAP_CASES, the two folded clip forms) and of
  ``test_amp_gpu.py`` (input gradient, weight gradient, statistics epilogue), at their original sizes: the float64 references
  take about a second at most, and several cases reach their kernel only at their size (see the comments).

``tests/test_bf16_exact_host.py`` checks the preconditions and the checker without a GPU; ``tests/test_bf16_exact_gpu.py``
runs the kernels.
"""
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

# ---- case tables --------------------------------------------------------------------------------------------------------
FwdCase = namedtuple("FwdCase", "name n cin cout thw kernel stride padding residual relu")

FORWARD_CASES = [FwdCase(f"c{i}", *c) for i, c in enumerate([
    # n, cin, cout, (t,h,w), kernel, stride, padding, residual, relu -- CASES of test_bf16_gpu.py
    (2, 64, 144, (4, 14, 14), (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True),     # S1-like, row tile 144 + zero-filled pitch
    (2, 144, 64, (4, 14, 14), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, True),      # T1-like + residual, K pitch 160
    (1, 64, 230, (4, 16, 16), (1, 3, 3), (1, 2, 2), (0, 1, 1), False, True),     # strided spatial
    (1, 230, 128, (6, 8, 8), (3, 1, 1), (2, 1, 1), (1, 0, 0), False, False),     # strided temporal, no relu
    (3, 64, 128, (4, 12, 12), (1, 1, 1), (2, 2, 2), (0, 0, 0), False, False),    # shortcut 1x1x1
    (1, 45, 64, (5, 9, 11), (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),       # T0: 45 -> pitch 64
    (1, 128, 288, (3, 10, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True),     # r3d-style 3x3x3
    (1, 512, 1152, (2, 7, 7), (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True),     # layer4 width
    (1, 921, 512, (2, 4, 4), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, True),       # 921 -> pitch 928, ragged voxel tile
    (5, 32, 33, (1, 3, 3), (1, 3, 3), (1, 1, 1), (0, 1, 1), False, False),       # tiny, Cout just over one chunk
    (2, 144, 64, (8, 8, 8), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, True),        # temporal, frames-x-positions tiles (8 x 32)
    (1, 45, 64, (16, 8, 12), (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),      # same, two frame blocks per clip
    # 16 frames x 16 positions, 128-row tiles: that kernel needs >= 384 column tiles of 256 voxels, so N stays 8
    (8, 32, 128, (16, 28, 28), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, False),
])] + [FwdCase(f"n{i}", n, cin, cout, thw, k, (1, 1, 1), (k[0] // 2, 1, 1), False, False) for i, (n, cin, cout, thw, k) in enumerate([
    # NINE_TAP_CASES of test_bf16_gpu.py: geometries that reach conv_bf16_same9_kernel
    (3, 144, 64, (16, 56, 56), (1, 3, 3)),      # 64-row tile, W = 56: taken only from 131072 voxels up, so the size stays
    (8, 128, 128, (16, 28, 28), (1, 3, 3)),     # one 128-row tile, W = 28: needs >= 384 column tiles, so the size stays
    (2, 128, 144, (6, 20, 28), (3, 3, 3)),      # 3x3x3 taps, 144-row tile, ragged last voxel tile
    (1, 160, 288, (4, 9, 7), (3, 3, 3)),        # 3x3x3, two row tiles, W = 7: a 256-voxel tile spans 36 image rows
])] + [
    # the stems (clip convolution, folded form): 3 channels, border materialised, kw folded into K
    FwdCase("clip_1x7x7", 2, 3, 45, (4, 20, 24), (1, 7, 7), (1, 2, 2), (0, 3, 3), False, True),
    FwdCase("clip_3x7x7", 2, 3, 45, (4, 20, 24), (3, 7, 7), (1, 2, 2), (1, 3, 3), False, True),
]

StatsCase = namedtuple("StatsCase", "name n cin cout thw kernel stride padding")
STATS_CASES = [StatsCase(*c) for c in [
    # CONV_STATS_CASES of test_amp_gpu.py: one per bf16 forward kernel that carries the statistics epilogue
    ("per_tap_strided_230", 2, 64, 230, (4, 16, 16), (1, 3, 3), (1, 2, 2), (0, 1, 1)),        # conv_bf16_kernel, ragged last voxel tile
    ("shared_image_144_rows", 2, 64, 144, (4, 20, 28), (1, 3, 3), (1, 1, 1), (0, 1, 1)),      # conv_bf16_same_kernel<9>, odd row block
    ("nine_tap_image_128_rows", 8, 128, 128, (16, 28, 28), (1, 3, 3), (1, 1, 1), (0, 1, 1)),  # conv_bf16_same9_kernel<8>
    ("temporal_frames_x_positions", 2, 144, 64, (8, 8, 8), (3, 1, 1), (1, 1, 1), (1, 0, 0)),  # conv_bf16_tsame_kernel
    ("small_problem_128_voxel_tiles", 1, 230, 128, (4, 7, 7), (3, 1, 1), (1, 1, 1), (1, 0, 0)),  # conv_bf16_kernel<4,4,2,2>
    ("shortcut_1x1x1", 3, 64, 128, (4, 12, 12), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    ("two_row_tiles_288", 1, 128, 288, (2, 14, 14), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("clip_convolution_folded", 2, 3, 45, (4, 32, 32), (1, 7, 7), (1, 2, 2), (0, 3, 3)),
]]

GradCase = namedtuple("GradCase", "name xs cout kernel stride padding")


def _grad_cases(prefix, rows):
    out = []
    for i, g in enumerate(rows):
        xs, cout, k = g[:3]
        stride = g[3] if len(g) > 3 else (1, 1, 1)
        pad = g[4] if len(g) > 4 else tuple((v - 1) // 2 for v in k)
        out.append(GradCase(f"{prefix}{i}", xs, cout, k, stride, pad))
    return out


DGRAD_CASES = _grad_cases("d", [
    # (N, Cin, T, H, W), Cout, kernel, stride, padding -- test_input_gradient_through_the_forward_kernel
    ((2, 64, 4, 12, 12), 144, (1, 3, 3), (1, 1, 1), (0, 1, 1)),      # spatial half of a (2+1)D pair
    ((2, 144, 4, 12, 12), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),      # temporal half
    ((2, 64, 4, 12, 12), 230, (1, 3, 3), (1, 2, 2), (0, 1, 1)),      # strided spatial (layer2 entry): four residue classes
    ((2, 230, 4, 6, 6), 128, (3, 1, 1), (2, 1, 1), (1, 0, 0)),       # strided temporal: two classes
    ((2, 64, 4, 12, 12), 128, (1, 1, 1), (2, 2, 2), (0, 0, 0)),      # strided 1x1x1 shortcut: 7 of 8 classes receive nothing
    ((1, 64, 4, 10, 10), 64, (3, 3, 3), (1, 1, 1), (1, 1, 1)),       # R3D-18
    ((1, 64, 4, 10, 10), 128, (3, 3, 3), (2, 2, 2), (1, 1, 1)),      # R3D-18 strided: eight classes
    ((1, 64, 3, 7, 9), 96, (1, 3, 3), (1, 2, 2), (0, 1, 1)),         # odd extents: the remainder rows / columns get zero gradient
])

WGRAD_CASES = _grad_cases("w", [
    # (N, Cin, T, H, W), Cout, kernel -- stride 1, "same" padding: test_native_bf16_weight_gradient_kernel
    ((2, 64, 4, 12, 12), 144, (1, 3, 3)),
    ((3, 64, 8, 28, 28), 144, (1, 3, 3)),       # 18816 voxels: several slices
    ((2, 128, 4, 14, 14), 230, (1, 3, 3)),      # odd channel count on the dz side (pitch 256)
    ((2, 512, 2, 7, 7), 1152, (1, 3, 3)),       # layer4: W = 7 (two borders inside a lane's 8 voxels), 8 input panels
    ((1, 64, 2, 4, 4), 48, (1, 3, 3)),          # 32 voxels: one chunk, W = 4
    ((2, 144, 4, 12, 12), 64, (3, 1, 1)),
    ((3, 144, 8, 28, 28), 64, (3, 1, 1)),
    ((2, 45, 4, 12, 12), 64, (3, 1, 1)),        # the stem's temporal half: 45 input channels (pitch 64)
    ((2, 921, 2, 7, 7), 512, (3, 1, 1)),        # layer4: two frames, odd channel count on the x side
    ((1, 64, 4, 10, 10), 64, (3, 3, 3)),        # R3D-18
    ((2, 128, 2, 6, 6), 256, (3, 3, 3)),
    ((1, 64, 3, 5, 9), 64, (3, 1, 3)),          # odd extents, voxel count not a multiple of 32
    ((2, 32, 2, 6, 6), 45, (1, 3, 3)),          # half an input panel, an output channel count that is no multiple of 16
    ((2, 48, 3, 5, 5), 20, (3, 3, 3)),          # 75 voxels per clip: partial last chunk; 20 output channels (pitch 32)
    ((1, 200, 4, 6, 6), 72, (3, 1, 1)),         # temporal form: 72 output channels (one panel and a bit), 200 input channels
    ((5, 64, 1, 3, 3), 64, (1, 3, 3)),          # 45 voxels, W = 3: every voxel is on a border
    # the gather form (one image per tap, rows fetched at strided input coordinates): the strided convolutions and the 1x1x1 shortcuts
    ((2, 64, 4, 12, 12), 230, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ((2, 230, 4, 6, 6), 128, (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    ((2, 64, 4, 12, 12), 128, (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    ((1, 64, 4, 10, 10), 128, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    ((1, 128, 3, 7, 9), 96, (1, 3, 3), (1, 2, 2), (0, 1, 1)),      # odd extents
    ((3, 256, 4, 14, 14), 921, (1, 3, 3), (1, 2, 2), (0, 1, 1)),   # S8-like: 4 input panels, 20 output-channel groups
    ((2, 96, 2, 5, 5), 40, (1, 1, 1), (1, 1, 1), (0, 0, 0)),       # 1x1x1 stride 1
])

FORWARD_Q = 3       # shifts are multiples of 1/8; weight scales 1, 2, 4; residuals multiples of 1/2
DGRAD_Q = 6         # weight scales 2^0 ... 2^-6 per forward output channel (they mix inside an input gradient's sum)
WGRAD_Q = 0         # integers


# ---- generators ---------------------------------------------------------------------------------------------------------
def _generator(case, salt=""):
    return torch.Generator().manual_seed(zlib.crc32((salt + str(tuple(case))).encode()))   # (not hash(): randomised per process)


def _ints(g, shape, amp):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).double()


def fill_border(g, x, amp):
    """(N, C, T, H, W): every zero on one of the six faces of a clip's (T, H, W) box is redrawn from +-{1 .. amp}."""
    t, h, w = x.shape[2:]
    face = torch.zeros((t, h, w), dtype=torch.bool)
    face[[0, -1]] = True
    face[:, [0, -1]] = True
    face[:, :, [0, -1]] = True
    sub = torch.randint(1, amp + 1, tuple(x.shape), generator=g).double() * (torch.randint(0, 2, tuple(x.shape), generator=g).double() * 2 - 1)
    return torch.where(face & (x == 0), sub, x)


def assert_faces_nonzero(x, what):
    """(N, C, T, H, W): no zero on any of the six faces of a clip's box, in any channel."""
    for face in (x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1], x[..., 0], x[..., -1]):
        assert bool((face != 0).all()), f"{what}: a border voxel is zero"


def out_dims(thw, kernel, stride, padding):
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(thw, kernel, stride, padding))


def forward_operands(case):
    """x in {-3..3} (faces non-zero), w in {-2..2}, per-channel scale in {1, 2, 4}, shift in multiples of 1/8 within +-4,
    residual in multiples of 1/2 within +-4 (None when the case has none): float64 CPU tensors."""
    g = _generator(case)
    x = fill_border(g, _ints(g, (case.n, case.cin) + case.thw, 3), 3)
    w = _ints(g, (case.cout, case.cin) + case.kernel, 2)
    scale = 2.0 ** torch.randint(0, 3, (case.cout,), generator=g).double()
    shift = _ints(g, (case.cout,), 32) / 8
    res = None
    if case.residual:
        res = _ints(g, (case.n, case.cout) + out_dims(case.thw, case.kernel, case.stride, case.padding), 8) / 2
    return x, w, scale, shift, res


def forward_reference(case, x, w, scale, shift, res):
    """(y, sum |terms|) in float64: relu?(conv3d(x, w * scale) + shift (+ res))."""
    ws = w * scale.view(-1, 1, 1, 1, 1)
    y = F.conv3d(x, ws, None, case.stride, case.padding) + shift.view(1, -1, 1, 1, 1)
    total = F.conv3d(x.abs(), ws.abs(), None, case.stride, case.padding) + shift.abs().view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + res
        total = total + res.abs()
    return (y.clamp_min(0) if case.relu else y), total


def stats_operands(case):
    """The statistics epilogue sums z and z^2 in fp32, so per channel sum |z| and sum z^2 (in the channel's unit) must stay below
    2^24 as well: x in {-2..2} (faces non-zero), w in {-1, 0, 1} times a per-channel scale in {1/2, 1, 2}, thinned so that the
    expected sum of z^2 is about 0.3 * 2^24."""
    g = _generator(case, "stats")
    x = fill_border(g, _ints(g, (case.n, case.cin) + case.thw, 2), 2)
    voxels = case.n * int(torch.tensor(out_dims(case.thw, case.kernel, case.stride, case.padding)).prod())
    k = case.cin * case.kernel[0] * case.kernel[1] * case.kernel[2]
    density = min(1.0, 0.3 * 2.0 ** 24 / (voxels * k * 2.0))        # E x^2 = 2
    w = _ints(g, (case.cout, case.cin) + case.kernel, 1) * (torch.rand((case.cout, case.cin) + case.kernel, generator=g) < density * 1.5).double()
    scale = 2.0 ** torch.randint(-1, 2, (case.cout,), generator=g).double()
    return x, w, scale


def stats_reference(case, x, w, scale):
    ws = w * scale.view(-1, 1, 1, 1, 1)
    return (F.conv3d(x, ws, None, case.stride, case.padding), F.conv3d(x.abs(), ws.abs(), None, case.stride, case.padding))


def dgrad_operands(case):
    """w in {-2..2} * 2^-e, e in {0..DGRAD_Q} per forward output channel; dz in {-3..3} (faces non-zero).  (The spread of scales
    makes the sums long in the grid's unit: on the 1x1x1 stride-2 shortcut only one input position in eight receives anything,
    and 5 % of ALL outputs must need rounding.)"""
    g = _generator(case, "dgrad")
    n, cin, t, h, w_ = case.xs
    scale = 2.0 ** -torch.randint(0, DGRAD_Q + 1, (case.cout,), generator=g).double()
    w = _ints(g, (case.cout, cin) + case.kernel, 2) * scale.view(-1, 1, 1, 1, 1)
    dz = fill_border(g, _ints(g, (n, case.cout) + out_dims((t, h, w_), case.kernel, case.stride, case.padding), 3), 3)
    return w, dz


def dgrad_reference(case, w, dz):
    """(dx, sum |terms|, reached): ``reached`` is False where no tap of any output touches the input position."""
    dx = torch.nn.grad.conv3d_input(case.xs, w, dz, case.stride, case.padding)
    total = torch.nn.grad.conv3d_input(case.xs, w.abs(), dz.abs(), case.stride, case.padding)
    reached = torch.nn.grad.conv3d_input(case.xs, torch.ones_like(w), torch.ones_like(dz), case.stride, case.padding) > 0
    return dx, total, reached


def wgrad_operands(case):
    """x and dz in {-3..3}, faces non-zero."""
    g = _generator(case, "wgrad")
    n, cin, t, h, w_ = case.xs
    x = fill_border(g, _ints(g, case.xs, 3), 3)
    dz = fill_border(g, _ints(g, (n, case.cout) + out_dims((t, h, w_), case.kernel, case.stride, case.padding), 3), 3)
    return x, dz


def wgrad_reference(case, x, dz):
    shape = (case.cout, case.xs[1]) + case.kernel
    return (torch.nn.grad.conv3d_weight(x, shape, dz, case.stride, case.padding),
            torch.nn.grad.conv3d_weight(x.abs(), shape, dz.abs(), case.stride, case.padding))


# ---- the precondition, the expected bits, the comparison ---------------------------------------------------------------
def assert_exact_in_fp32(q, total, *operands):
    """Every operand is an integer multiple of 2^-q and is a bf16 value; ``total`` (sum |terms| per output, every addend the
    kernel adds included) stays below 2^(24 - q): every partial sum in every order is then an fp32 number."""
    unit = 2.0 ** q
    for t in operands:
        if t is None:
            continue
        assert torch.equal((t * unit).round(), t * unit), f"an operand is not on the 2^-{q} grid"
        assert torch.equal(t.to(torch.bfloat16).double(), t), "an operand is not a bf16 value"
    assert float(total.max()) * unit < 2.0 ** 24, f"sum |terms| = {float(total.max())} reaches 2^(24 - {q})"


def rne_bf16(y64):
    """The one correct bf16 code of an exact result: the value is an fp32 number (asserted), so the conversion rounds once."""
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "the reference value is not an fp32 number: the precondition does not hold"
    return y32.to(torch.bfloat16)


def rounding_profile(y64):
    """(share of the outputs that are not bf16 values, exact ties whose even neighbour is the larger magnitude, ... the smaller)."""
    y32 = y64.float()
    assert torch.equal(y32.double(), y64)
    bits = y32.view(torch.int32)
    low = bits & 0xFFFF
    tie = low == 0x8000
    up = tie & (((bits >> 16) & 1) == 1)
    return float((low != 0).double().mean()), int(up.sum()), int((tie & ~up).sum())


def ties_away_bf16(y64):
    """What a kernel that rounds ties away from zero would store (a planted error for the host test)."""
    bits = y64.float().view(torch.int32)
    return (((bits + 0x8000) >> 16) << 16).view(torch.float32).to(torch.bfloat16)


def assert_same_values(got, want, exact=None, what=""):
    """``torch.equal`` on the values (+0 and -0 are one zero).  On failure: the count, the first coordinates, got / want / exact."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    if torch.equal(g, w):
        return
    bad = g != w
    lines = []
    for idx in bad.nonzero()[:6]:
        i = tuple(int(v) for v in idx)
        lines.append(f"  {i}: got {float(g[i])!r} want {float(w[i])!r}" + (f" exact {float(exact[i])!r}" if exact is not None else ""))
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ\n" + "\n".join(lines))


def channels_first(y_cl, channels):
    """[N][T][H][W][Cp] -> (N, channels, T, H, W) on the host, dtype kept (a test-side layout change, no kernel)."""
    return y_cl[..., :channels].permute(0, 4, 1, 2, 3).contiguous().cpu()


# ---- element-wise references ----------------------------------------------------------------------------------------------
def _exact_sum(p, q, what):
    """p + q in float64, asserted free of rounding (Knuth's two-sum: the error term of a float64 addition is itself a float64
    number and is zero exactly when the sum was exact)."""
    s = p + q
    qq = s - p
    err = (p - (s - qq)) + (q - qq)
    assert int(torch.count_nonzero(err)) == 0, f"{what} is not exact in float64: the reference would round twice"
    return s


def bn_apply_reference(z, a, b, residual, relu):
    """``bn_cl_apply_kernel`` as its file header states it: y = relu?(fma(z, a, b) (+ res)), one rounding to bf16.  z (bf16 values,
    8 bits) times a (fp32, 24 bits) is exact in float64; the sum with b is exact in float64 unless the exponents lie far apart,
    and that is asserted, not hoped: then one rounding to fp32 = the fma.  The residual is added in fp32 (exact in float64,
    asserted, rounded once); ReLU last; then round-to-nearest-even to bf16.
    z, residual: (..., C) bf16 values as float64; a, b: (C,) fp32 as float64."""
    p = z * a
    s = _exact_sum(p, b.expand_as(p), "z * a + b")
    v = s.float()
    if residual is not None:
        v = _exact_sum(v.double(), residual, "fma + residual").float()
    if relu:
        v = v.clamp_min(0)
    return v.to(torch.bfloat16)


def fp32_ulp(v64):
    """Spacing of the fp32 numbers at |v| (float64 tensor; normal range)."""
    return 2.0 ** (torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** -126))) - 23)
