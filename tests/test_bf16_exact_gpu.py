"""The bf16 kernels bit for bit on exactly representable operands (``bf16_exact_cases.py``: why fp32 accumulation is exact there,
the operand grids, the float64 references; ``test_bf16_exact_host.py``: every case meets the precondition and exercises
rounding and ties).  Every comparison here is ``torch.equal`` on the values (+0 and -0 are one zero); there is no tolerance,
except where a non-dyadic division is involved (the mean pools over a voxel count that is no power of two), and there the
allowance is one fp32 ulp of the quotient, stated at the test.

* conversion edges: the fp32 -> bf16 conversions of the tree (``to_bf16_bits`` of csrc/train_bf16.hip, the compiler's ``(__bf16)``
  cast of csrc/conv_bf16.hip) against torch's CPU ``.to(torch.bfloat16)`` bit patterns on midpoints, their fp32 neighbours, the
  ends of the format and the subnormal range;
* forward convolution (every route a geometry has), statistics epilogue, input gradient, weight gradient;
* ``bn_cl_fwd_train`` against the arithmetic the header of csrc/train_bf16.hip states, on the kernel's own (a, b) rows; the
  integer sums ``dbeta`` / ``dbias``; the mean pool and its backward.
"""
from ctypes import byref

import pytest
import torch

import bf16_exact_cases as X

pytestmark = pytest.mark.gpu

from zeroshotvideoclassification_amd import _lib, amp, inference, ops  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16


def _dev(t):
    return t.float().to(DEV)


def to_cl(t):
    return amp.ncdhw_to_cl_bf16(_dev(t))


def _geometry(cin, cout, kernel, stride, padding):
    return inference.ConvGeometry(torch.nn.Conv3d(cin, cout, kernel, stride, padding, bias=False, device="meta"))


def _forward_input(case, x):
    """(descriptor, x in the layout the forward reads): channels-last bf16, or the folded clip form inside its border."""
    geo = _geometry(case.cin, case.cout, case.kernel, case.stride, case.padding)
    t, h, w = case.thw
    if geo.folded:
        xb, wo = geo.clip_input(_dev(x))
        return geo.desc(case.n, t, xb.shape[2], xb.shape[3], wo), xb
    return geo.desc(case.n, t, h, w), to_cl(x)


def _routes(case):
    """The default route and every ``ZSV_BF16_NO_*`` switch whose kernel this geometry can reach (the eligibility rules of
    csrc/conv_bf16.hip: bf16_tsame_frames, bf16_same_applicable, bf16_same9_applicable, the 64-row same form).

    This restates those rules by hand, on the generous side: a switch is listed wherever its kernel MIGHT be chosen (the 64-row
    form also needs 131072 voxels, the nine-tap form a single K chunk), and a switch that changes nothing costs one more exact
    run of the default route.  Nothing here proves that a switch moved the launch to another kernel
    (``test_amp_full_size_gpu.py`` does that with a kernel trace at the benchmarked size): if the rules in the .hip file move,
    move this list with them, or a route stops being exercised without any test failing."""
    routes = [None]
    if case.cin <= 4 or case.stride != (1, 1, 1):
        return routes
    if case.kernel == (3, 1, 1) and case.padding == (1, 0, 0):
        routes.append("ZSV_BF16_NO_TSAME")
    if case.kernel[2] == 3 and case.padding[2] == 1 and X.out_dims(case.thw, case.kernel, case.stride, case.padding) == case.thw:
        routes.append("ZSV_BF16_NO_SAME")
        if case.kernel[1] == 3 and case.padding[1] == 1 and case.thw[2] <= 63:
            routes.append("ZSV_BF16_NO_SAME9")
        if case.cout <= 64:
            routes.append("ZSV_BF16_NO_SAME64")
    return routes


# ---- conversion edges ------------------------------------------------------------------------------------------------------
def _edge_values():
    """fp32 values around every pair of neighbouring bf16 codes of six code ranges: the code itself, the midpoint to the next code
    (both parities of the kept bit), and the fp32 numbers one ulp either side of the midpoint; both signs.  The ranges: the
    subnormals and the first normal binade (256 codes), then 2000 consecutive codes starting in five binades, the last range
    ending at the largest finite code -- its midpoint values are FLT_MAX's neighbourhood: 0x7F7F7FFF stays finite, the overflow
    midpoint 0x7F7F8000 and FLT_MAX round to infinity.  +-0 (sign kept), +-inf and FLT_MAX are in the list by construction."""
    codes = torch.cat([torch.arange(0x0000, 0x0100)] + [torch.arange(s, s + 2000) for s in (0x0780, 0x3F00, 0x4280, 0x6000, 0x7F80 - 2000)])
    base = codes.to(torch.int64) << 16
    bits = torch.cat([base, base | 0x7FFF, base | 0x8000, base | 0x8001, torch.tensor([0x7F7FFFFF, 0x7F800000])])
    bits = torch.cat([bits, bits | 0x80000000])
    vals = (bits & 0xFFFFFFFF).to(torch.int64)
    vals = torch.where(vals >= 2 ** 31, vals - 2 ** 32, vals).to(torch.int32).view(torch.float32)
    assert not torch.isnan(vals).any()
    return vals


def _pad_to(vals, multiple):
    n = -(-vals.numel() // multiple) * multiple
    return torch.cat([vals, torch.zeros(n - vals.numel())])


def _assert_same_bits(got, want, vals, what):
    g, w = got.cpu().contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    bad = g != w
    if bool(bad.any()):
        i = bad.nonzero().flatten()[:6]
        rows = [f"  fp32 {int(vals.view(torch.int32)[j]) & 0xFFFFFFFF:#010x}: got {int(g[j]) & 0xFFFF:#06x} want {int(w[j]) & 0xFFFF:#06x}" for j in i]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} codes differ\n" + "\n".join(rows))


def test_layout_converters_round_to_nearest_even_at_the_edges():
    """``amp.ncdhw_to_cl_bf16`` (``to_bf16_bits``) and ``inference.clip_to_bf16`` (the compiler's cast): torch's bit patterns, the
    sign of zero and the subnormals included; NaN stays NaN."""
    vals = _edge_values()
    v = _pad_to(vals, 64)
    got = amp.ncdhw_to_cl_bf16(v.view(1, 64, 1, 1, -1).to(DEV))                   # [1][1][1][S][64]
    _assert_same_bits(got[0, 0, 0].t().reshape(-1), v.to(BF16), v, "ncdhw_to_cl_bf16")
    v = _pad_to(vals, 3)
    got = inference.clip_to_bf16(v.view(1, 3, 1, 1, -1).to(DEV), 0, 0, 1, v.numel() // 3)     # [1][1][1][S][4]
    _assert_same_bits(got[0, 0, 0, :, :3].t().reshape(-1), v.to(BF16), v, "clip_to_bf16")
    assert int(torch.count_nonzero(got[..., 3].float())) == 0
    nan = torch.tensor([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000, 0x7F80FFFF, 0x7FBF0000], dtype=torch.int64)
    nan = torch.cat([nan, nan | 0x80000000])
    nan = torch.where(nan >= 2 ** 31, nan - 2 ** 32, nan).to(torch.int32).view(torch.float32)
    assert bool(torch.isnan(nan).all())
    got = amp.ncdhw_to_cl_bf16(_pad_to(nan, 64).view(1, 64, 1, 1, -1).to(DEV))
    assert bool(torch.isnan(got[0, 0, 0].t().reshape(-1)[:nan.numel()].float()).all()), "ncdhw_to_cl_bf16 lost a NaN"
    got = inference.clip_to_bf16(nan.view(1, 3, 1, 1, -1).to(DEV), 0, 0, 1, nan.numel() // 3)
    assert bool(torch.isnan(got[0, 0, 0, :, :3].float()).all()), "clip_to_bf16 lost a NaN"


def test_convolution_epilogue_rounds_to_nearest_even_at_the_edges():
    """The forward epilogue's store: a 1x1x1 convolution with all-zero weights whose shift carries the values (0 + shift is the
    shift; a shift of -0 gives +0, which is the same value), with and without a zero residual, 1024 channels a launch."""
    vals = _pad_to(_edge_values(), 1024).view(-1, 1024)
    cout, cin = 1024, 32
    d = _geometry(cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0)).desc(1, 1, 1, 2)
    x = torch.ones((1, 1, 1, 2, cin), dtype=BF16, device=DEV)
    w = torch.zeros((cout, cin, 1, 1, 1), device=DEV)
    zero_res = torch.zeros((1, 1, 1, 2, cout), dtype=BF16, device=DEV)
    for res in (None, zero_res):
        out = []
        for row in vals:
            blob = inference.pack_conv(d, w, None, row.to(DEV))
            out.append(inference.conv_bf16(d, x, blob, res, False))
        got = torch.stack(out).cpu()                                                # (launch, 1, 1, 1, 2, 1024)
        for voxel in range(2):
            X.assert_same_values(got[:, 0, 0, 0, voxel], vals.to(BF16), vals.double(),
                                 f"conv epilogue {'with' if res is not None else 'without'} residual, voxel {voxel}")


def test_batchnorm_apply_rounds_to_nearest_even_at_the_edges():
    """``bn_cl_fwd_eval`` with identity coefficients (gamma = 1, running variance 1, eps = 0, running mean 0: a = 1 exactly):
    every non-NaN bf16 code through z comes back as itself, subnormals included; and the fp32 edge values through the shift
    row (z = 0, b = beta) are rounded to nearest even."""
    c = 1024
    bn = torch.nn.BatchNorm3d(c).to(DEV).eval()
    bn.eps = 0.0
    codes = torch.arange(0, 65536, dtype=torch.int32)
    codes = torch.where((codes & 0x7FFF) > 0x7F80, torch.zeros_like(codes), codes)
    z = torch.where(codes >= 32768, codes - 65536, codes).to(torch.int16).view(BF16).view(1, 1, 1, 64, c).to(DEV)
    y, coef = amp.bn_cl_fwd_eval(z, bn, None, False)
    assert torch.equal(coef[0], torch.ones(c, device=DEV)) and int(torch.count_nonzero(coef[1])) == 0
    X.assert_same_values(y, z, z.double(), "bn_cl_fwd_eval identity")
    vals = _pad_to(_edge_values(), c).view(-1, c)
    zero = torch.zeros((1, 1, 1, 2, c), dtype=BF16, device=DEV)
    out = []
    for row in vals:
        with torch.no_grad():
            bn.bias.copy_(row)
        out.append(amp.bn_cl_fwd_eval(zero, bn, None, False)[0])
    got = torch.stack(out).cpu()
    for voxel in range(2):
        X.assert_same_values(got[:, 0, 0, 0, voxel], vals.to(BF16), vals.double(), f"bn_cl_fwd_eval shift row, voxel {voxel}")


# ---- convolutions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.FORWARD_CASES, ids=[c.name for c in X.FORWARD_CASES])
def test_forward_stores_the_one_correct_code_on_every_route(case, monkeypatch):
    x, w, scale, shift, res = X.forward_operands(case)
    y64, _ = X.forward_reference(case, x, w, scale, shift, res)
    want = X.rne_bf16(y64)
    d, xb = _forward_input(case, x)
    rb = to_cl(res) if res is not None else None
    for knob in _routes(case):
        if knob:
            monkeypatch.setenv(knob, "1")
        blob = inference.pack_conv(d, _dev(w), _dev(scale), _dev(shift))
        y = inference.conv_bf16(d, xb, blob, rb, case.relu)
        torch.cuda.synchronize()
        if knob:
            monkeypatch.delenv(knob)
        what = f"{case.name} on {'the default route' if knob is None else knob}"
        assert y.shape[-1] == inference.channel_pitch(case.cout)
        assert int(torch.count_nonzero(y[..., case.cout:].float())) == 0, f"{what}: pad channels must be written as zero"
        X.assert_same_values(X.channels_first(y, case.cout), want, y64, what)


@pytest.mark.parametrize("case", X.STATS_CASES, ids=[c.name for c in X.STATS_CASES])
def test_statistics_epilogue_sums_the_stored_values_exactly(case):
    x, w, scale = X.stats_operands(case)
    z64, _ = X.stats_reference(case, x, w, scale)
    want = X.rne_bf16(z64)
    d, xb = _forward_input(case, x)
    blob = amp.pack_conv(d, _dev(w * scale.view(-1, 1, 1, 1, 1)), None, None)
    z0 = amp.conv_bf16(d, xb, blob, None, False)
    z, partials, rows = amp.conv_bf16_stats(d, xb, blob)
    torch.cuda.synchronize()
    assert torch.equal(z, z0), "the statistics epilogue must not change the stored values"
    X.assert_same_values(X.channels_first(z, case.cout), want, z64, f"{case.name}: z")
    assert 0 < rows <= partials.shape[0]
    stored = want.double()
    s1, s2 = partials[:rows, 0, :case.cout].double().sum(0), partials[:rows, 1, :case.cout].double().sum(0)
    X.assert_same_values(s1, stored.sum(dim=(0, 2, 3, 4)), what=f"{case.name}: sum z")
    X.assert_same_values(s2, (stored * stored).sum(dim=(0, 2, 3, 4)), what=f"{case.name}: sum z^2")


def _unit(case):
    cin = case.xs[1]
    conv = torch.nn.Conv3d(cin, case.cout, case.kernel, stride=case.stride, padding=case.padding, bias=False)
    return conv, amp._Unit(conv.to(DEV), torch.nn.BatchNorm3d(case.cout).to(DEV), False)


@pytest.mark.parametrize("case", X.DGRAD_CASES, ids=[c.name for c in X.DGRAD_CASES])
def test_input_gradient_stores_the_one_correct_code(case):
    w, dz = X.dgrad_operands(case)
    dx64, _, reached = X.dgrad_reference(case, w, dz)
    n, cin, t, h, w_ = case.xs
    conv, u = _unit(case)
    with torch.no_grad():
        u.conv.weight.copy_(_dev(w))
    rec = amp._Record()
    rec.unit, rec.desc = u, u.desc(n, t, h, w_)
    dx_cl = amp.Bf16TrainPath._dgrad(rec, to_cl(dz))
    torch.cuda.synchronize()
    got = X.channels_first(dx_cl, cin)
    assert tuple(got.shape) == tuple(case.xs)
    X.assert_same_values(got, X.rne_bf16(dx64), dx64, f"{case.name}: dx")          # strided residue classes included
    assert int(torch.count_nonzero(got.float()[~reached])) == 0, "a position no tap reaches must be exactly zero"
    assert int(torch.count_nonzero(dx_cl[..., cin:].float())) == 0, "pad channels must be zero"


@pytest.mark.parametrize("case", X.WGRAD_CASES, ids=[c.name for c in X.WGRAD_CASES])
def test_weight_gradient_is_the_exact_integer(case):
    """``zsv_conv3d_bf16_wgrad``, native (w0 .. w15) and gather form (w16 .. w22): every fp32 output is the integer sum."""
    x, dz = X.wgrad_operands(case)
    dw64, _ = X.wgrad_reference(case, x, dz)
    n, cin, t, h, w_ = case.xs
    _, u = _unit(case)
    rec = amp._Record()
    rec.unit, rec.desc, rec.x, rec.clips = u, u.desc(n, t, h, w_), to_cl(x), None
    assert _lib.load().zsv_conv3d_bf16_wgrad_workspace_bytes(byref(rec.desc)) > 0, "the native kernel must take this geometry"
    dw = amp.Bf16TrainPath._wgrad(rec, to_cl(dz))
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32
    X.assert_same_values(dw, dw64, what=f"{case.name}: dW")


# ---- element-wise and reductions ----------------------------------------------------------------------------------------
def _bf16_randn(shape, g, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(BF16).double()


def _bn(c, g):
    bn = torch.nn.BatchNorm3d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
    return bn.to(DEV).train()


@pytest.mark.parametrize("shape,relu,res", [((2, 45, 4, 9, 7), True, False), ((3, 64, 2, 8, 8), True, True),
                                            ((1, 144, 3, 5, 6), False, False), ((2, 230, 2, 4, 4), False, True),
                                            ((2, 1152, 1, 3, 3), True, True), ((4, 64, 8, 28, 28), True, True)])
def test_batchnorm_forward_is_the_arithmetic_its_header_states(shape, relu, res):
    """y = relu?(fma(z, a, b) (+ res)), one rounding to bf16, with the kernel's OWN (a, b) rows: bit for bit.  (The rows follow from
    the returned statistics, which ``test_amp_gpu.py`` holds to 1e-5 of fp64.)"""
    c = shape[1]
    g = torch.Generator().manual_seed(c * 11 + shape[2])
    z = _bf16_randn(shape, g, 1.5, 0.3)
    r = _bf16_randn(shape, g) if res else None
    bn = _bn(c, g)
    z_cl, r_cl = to_cl(z), (to_cl(r) if res else None)
    y_cl, mean, invstd, coef = amp.bn_cl_fwd_train(z_cl, bn, r_cl, relu, want_coef=True)
    torch.cuda.synchronize()
    a, b = coef[0, :c].double().cpu(), coef[1, :c].double().cpu()
    want = X.bn_apply_reference(z_cl[..., :c].double().cpu(), a, b, r_cl[..., :c].double().cpu() if res else None, relu)
    X.assert_same_values(y_cl[..., :c], want, what=f"bn_cl_fwd_train {shape} relu={relu} res={res}")
    assert int(torch.count_nonzero(y_cl[..., c:].float())) == 0 and int(torch.count_nonzero(coef[:, c:])) == 0


@pytest.mark.parametrize("relu", [False, True], ids=["no_mask", "relu_mask"])
@pytest.mark.parametrize("shape", [(2, 45, 4, 9, 7), (2, 1152, 1, 3, 3), (4, 64, 8, 28, 28)])      # 504, 18 and 25088 rows
def test_dbeta_is_the_exact_integer_sum(shape, relu):
    """``bn_cl_bwd`` on integer dy: dbeta = sum of dy (where the forward's stored y is positive, with the mask), exactly; the
    recomputed-mask form (``fwd_coef``) gives the same integer."""
    c = shape[1]
    g = torch.Generator().manual_seed(c * 13 + shape[2])
    z_cl = to_cl(_bf16_randn(shape, g, 1.5, 0.3))
    dy_cl = to_cl(torch.randint(-3, 4, shape, generator=g).double())
    bn = _bn(c, g)
    y_cl, mean, invstd, coef = amp.bn_cl_fwd_train(z_cl, bn, None, relu, want_coef=True)
    _, _, _, dbeta = amp.bn_cl_bwd(dy_cl, y_cl, z_cl, bn, mean, invstd, relu, want_g=False)
    torch.cuda.synchronize()
    dy = dy_cl[..., :c].double()
    want = (dy * (y_cl[..., :c] > 0) if relu else dy).reshape(-1, c).sum(0)
    assert float(dy.abs().reshape(-1, c).sum(0).max()) < 2.0 ** 24
    X.assert_same_values(dbeta, want, what="dbeta")
    if relu:
        _, _, _, dbeta2 = amp.bn_cl_bwd(dy_cl, None, z_cl, bn, mean, invstd, True, want_g=False, fwd_coef=coef)
        X.assert_same_values(dbeta2, want, what="dbeta (mask recomputed from z)")


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "relu_mask"])
@pytest.mark.parametrize("shape", [(2, 64, 4, 9, 7), (3, 512, 1, 4, 4), (4, 64, 8, 28, 28)])
def test_dbias_is_the_exact_integer_sum(shape, masked):
    """``relu_bias_bwd_cl`` on integer dy: with an output that is positive everywhere the mask keeps everything."""
    c = shape[1]
    g = torch.Generator().manual_seed(c * 17 + shape[2])
    y = _bf16_randn(shape, g)
    y = y.clamp_min(0) if masked else y.abs() + 1
    dy = torch.randint(-3, 4, shape, generator=g).double()
    gg, db = amp.relu_bias_bwd_cl(to_cl(dy), to_cl(y), c)
    torch.cuda.synchronize()
    expect = dy * (y > 0)
    X.assert_same_values(X.channels_first(gg, c), expect.to(BF16), what="masked gradient")
    X.assert_same_values(db, expect.sum(dim=(0, 2, 3, 4)), what="dbias")


@pytest.mark.parametrize("thw", [(4, 4, 4), (2, 5, 7)], ids=["S64", "S70"])
def test_meanpool_and_its_backward(thw):
    """Integer inputs: the fp32 sum is exact.  S = 64: the quotient is exact too -- equality.  S = 70: the kernel divides in fp32, so
    the result is within one fp32 ulp of the exact quotient; the backward's stored bf16 code is the code of some value within one
    fp32 ulp of the exact quotient (it may be the neighbour only where a bf16 midpoint lies that close)."""
    n, c, cp = 3, 70, 96
    s = thw[0] * thw[1] * thw[2]
    g = torch.Generator().manual_seed(s)
    x = torch.randint(-3, 4, (n,) + thw + (cp,), generator=g).to(BF16).to(DEV)
    got = inference.meanpool_bf16(x, c).double().cpu()
    q = x[..., :c].double().cpu().sum(dim=(1, 2, 3)) / s
    dp = torch.randn((n, c), generator=g)
    dx = amp.meanpool_bf16_bwd(dp.to(DEV), x, c)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(dx[..., c:].float())) == 0
    dxc = dx[..., :c].double().cpu().reshape(n, s, c)
    assert bool((dxc == dxc[:, :1]).all()), "every voxel of a clip gets the same gradient"
    qb = dp.double() / s
    if s & (s - 1) == 0:
        X.assert_same_values(got, q, what="meanpool_bf16")
        X.assert_same_values(dxc[:, 0], X.rne_bf16(qb), qb, "meanpool_bf16_bwd")
    else:
        assert bool(((got - q).abs() <= X.fp32_ulp(q)).all())
        u = X.fp32_ulp(qb)
        codes = [(qb + k * u).float().to(BF16).double() for k in (-1, 0, 1)]
        ok = (dxc[:, 0] == codes[0]) | (dxc[:, 0] == codes[1]) | (dxc[:, 0] == codes[2])
        assert bool(ok.all()), f"{int((~ok).sum())} codes are not the code of any value within one fp32 ulp of the quotient"
