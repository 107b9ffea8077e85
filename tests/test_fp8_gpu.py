"""e4m3 inference path: zsv_conv3d_fp8_fwd per layer against a float64 convolution of the SAME e4m3 operands,
the e4m3 encode / decode against torch's float8_e4m3fn bit patterns, the mean pool, and the whole Fp8Engine against the fp32
fixtures and the bf16 engine.

Per layer the only freedom is the fp32 accumulation: an output code must equal the code of the float64 result rounded
(to nearest even) to e4m3 after the clamp to +-448, except where that float64 value lies within fp32 summation noise
(n * 2^-23 * sum of |products|) of a rounding midpoint -- there the neighbouring code is as right.  Zeros are compared as values (+0 and -0 are one zero).
End to end the bars are statistical: per-clip cosine to the fp32 embedding >= 0.995 (measured minimum and margin).
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden, make_opt
from zeroshotvideoclassification_amd import _lib, inference, network, ops, synthetic, train

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
COS_BAR = 0.995


def e4m3(t):
    """Saturating float -> e4m3 (torch's own cast turns values beyond the range into NaN: clamp first)."""
    return t.float().clamp(-448.0, 448.0).to(FP8)


def to_ndhwc8(x, pitch):
    """(N,C,T,H,W) values already on the e4m3 grid -> [N][T][H][W][pitch] e4m3 on the device, pad channels zero."""
    n, c, t, h, w = x.shape
    codes = torch.zeros((n, t, h, w, pitch), dtype=torch.uint8)
    codes[..., :c] = e4m3(x.permute(0, 2, 3, 4, 1)).view(torch.uint8)
    return codes.to(DEV).view(FP8)


def codes_of(y):
    return y.view(torch.uint8).cpu()


def values_of(codes):
    return codes.view(FP8).double()


def grid_weights(g, cout, cin, k):
    """Weights whose per-channel e4m3 quantisation is exact: codes q on the e4m3 grid with max |q| = 448 per row, times a
    power of two per row.  Returns (fp32 weights, q as float64, row factors as float64)."""
    q = e4m3(torch.randn((cout, cin) + k, generator=g) * 60.0).double()
    flat = q.view(cout, -1)
    pos = torch.randint(0, flat.shape[1], (cout,), generator=g)
    sign = torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0).double()
    flat[torch.arange(cout), pos] = 448.0 * sign
    e = torch.randint(-14, -7, (cout,), generator=g).double()
    s = torch.pow(2.0, e)
    return (q * s.view(-1, 1, 1, 1, 1)).float(), q, s


def check_codes(got_codes, y, tol, what):
    """got_codes (uint8, NCTHW) against the exact float64 result y (before saturation) with accumulation noise tol."""
    ys = y.clamp(-448.0, 448.0)
    ref = values_of(e4m3(ys).view(torch.uint8))
    got = values_of(got_codes)
    assert not torch.isnan(got).any(), f"{what}: NaN code"
    bad = got != ref
    if bad.any():
        mid = (got + ref) / 2
        near = (ys - mid).abs() <= tol
        worst = bad & ~near
        assert not worst.any(), (f"{what}: {int(worst.sum())} of {got.numel()} codes differ away from a rounding midpoint; e.g. "
                                 f"got {got[worst][:4].tolist()} want {ref[worst][:4].tolist()} (exact {ys[worst][:4].tolist()})")
    return int(bad.sum())


def run_case(n, cin, cout, thw, k, s, p, use_res, relu, seed):
    t, h, w = thw
    g = torch.Generator().manual_seed(seed)
    x = e4m3(torch.randn((n, cin, t, h, w), generator=g) * 4.0).double()
    wgt, q, rs = grid_weights(g, cout, cin, k)
    shift = torch.randn(cout, generator=g) * 8.0
    acc = F.conv3d(x, q, stride=s, padding=p)
    mag = F.conv3d(x.abs(), q.abs(), stride=s, padding=p) * rs.view(1, -1, 1, 1, 1)
    y = acc * rs.view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    res = None
    if use_res:
        res = e4m3(torch.randn(y.shape, generator=g) * 8.0).double()
        y = y + res
    if relu:
        y = y.clamp_min(0)
    # fp32 summation noise: the bound n * u * sum|terms| of any summation order over the n = Cin x taps products, with u = 2^-23
    # (one ulp per addition: the matrix core's internal adds need not round to nearest), plus the epilogue's fma / residual add
    tol = mag * (cin * int(np.prod(k))) * 2.0 ** -23 + y.abs() * 2.0 ** -22 + 1e-30

    d = ops.conv_desc(x.shape, wgt.shape, s, p)
    blob = inference.pack_conv_fp8(d, wgt.to(DEV), None, shift.to(DEV))
    xb = to_ndhwc8(x, inference.fp8_channel_pitch(cin))
    rb = to_ndhwc8(res, inference.fp8_channel_pitch(cout)) if use_res else None
    yk = inference.conv_fp8(d, xb, blob, rb, relu)
    assert yk.dtype == FP8 and yk.shape[-1] == inference.fp8_channel_pitch(cout)
    codes = codes_of(yk)
    assert torch.count_nonzero(codes[..., cout:]) == 0, "pad channels must be written as zero"
    return check_codes(codes[..., :cout].permute(0, 4, 1, 2, 3), y, tol, f"{n}x{cin}->{cout} thw={thw} k={k} s={s}")


CASES = [
    # n, cin, cout, (t,h,w), kernel, stride, padding, residual, relu
    (2, 64, 144, (4, 14, 14), (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True),     # S1: 144-row tile, pitch 192 zero-filled; shared image
    (2, 144, 64, (8, 8, 8), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, True),        # T1 + residual: frames-x-positions tiles, K pitch 192
    (2, 144, 64, (4, 14, 14), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, True),      # T1 shape the frame tiles do not divide: per-tap
    (1, 64, 230, (4, 16, 16), (1, 3, 3), (1, 2, 2), (0, 1, 1), False, True),     # strided spatial, 230 -> pitch 256
    (1, 230, 128, (6, 8, 8), (3, 1, 1), (2, 1, 1), (1, 0, 0), False, False),     # strided temporal, no relu
    (3, 64, 128, (4, 12, 12), (1, 1, 1), (2, 2, 2), (0, 0, 0), False, False),    # the 1x1x1 stride-2 shortcut
    (1, 45, 64, (5, 9, 11), (3, 1, 1), (1, 1, 1), (1, 0, 0), False, True),       # the stem's temporal half: 45 -> pitch 64
    (1, 128, 288, (3, 10, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True),     # 3x3x3 stride 1 (R3D / MC3)
    (1, 64, 128, (4, 10, 10), (3, 3, 3), (2, 2, 2), (1, 1, 1), False, True),     # 3x3x3 stride 2
    (2, 128, 128, (8, 28, 28), (1, 3, 3), (1, 1, 1), (0, 1, 1), True, True),     # one image for the nine (kh, kw) taps
    (1, 256, 144, (4, 9, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), False, True),      # nine-tap image, 3x3x3, 144-row tile
    (1, 921, 512, (2, 4, 4), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, True),       # 921 -> pitch 960, ragged voxel tile
    (1, 512, 921, (2, 7, 7), (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True),      # 921 produced channels (row tile 144)
    (8, 64, 128, (16, 28, 28), (3, 1, 1), (1, 1, 1), (1, 0, 0), True, False),    # 16 frames x 16 positions, 128-row tiles
    (2, 64, 64, (8, 56, 56), (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True),       # R3D layer1: 64-row shared image
]


@pytest.mark.parametrize("case", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_conv_fp8_matches_fp64_of_e4m3_operands(case):
    run_case(*case, seed=zlib.crc32(str(case).encode()))


def test_conv_fp8_random_geometries():
    """Seeded sweep over the four kernels' domains (per-tap, shared image over kw, nine-tap image, frames-x-positions tiles),
    strides, channel pitches and ragged tiles."""
    rng = np.random.RandomState(78)
    kernels = [((1, 3, 3), (0, 1, 1)), ((3, 1, 1), (1, 0, 0)), ((3, 3, 3), (1, 1, 1)), ((1, 1, 1), (0, 0, 0))]
    for it in range(20):
        k, p = kernels[rng.randint(len(kernels))]
        s = tuple(int(v) for v in (rng.choice([1, 1, 2]) if k[0] > 1 or k == (1, 1, 1) else 1,
                                   rng.choice([1, 1, 2]) if k[1] > 1 or k == (1, 1, 1) else 1,
                                   rng.choice([1, 1, 2]) if k[2] > 1 or k == (1, 1, 1) else 1))
        cin = int(rng.choice([32, 45, 64, 100, 144, 230]))
        cout = int(rng.choice([33, 64, 128, 144, 230]))
        t, h, w = int(rng.choice([2, 4, 8, 16])), int(rng.choice([4, 7, 8, 12])), int(rng.choice([4, 8, 9, 16]))
        n = int(rng.randint(1, 4))
        use_res, relu = bool(rng.randint(2)), bool(rng.randint(2))
        run_case(n, cin, cout, (t, h, w), k, s, p, use_res, relu, seed=600 + it)


def _shift_only(values, relu=False, residual=None):
    """A 1x1x1 convolution with all-zero weights: the output is sat_e4m3(shift (+ residual)), exactly."""
    cout = values.numel()
    d = ops.conv_desc((1, 64, 1, 1, 16), (cout, 64, 1, 1, 1), (1, 1, 1), (0, 0, 0))
    blob = inference.pack_conv_fp8(d, torch.zeros((cout, 64, 1, 1, 1), device=DEV), None, values.float().to(DEV))
    x = torch.zeros((1, 1, 1, 16, 64), dtype=torch.uint8, device=DEV).view(FP8)
    y = inference.conv_fp8(d, x, blob, residual, relu)
    return codes_of(y)[0, 0, 0, :, :cout]


def test_e4m3_encode_matches_torch_bit_patterns_and_saturates():
    """Every finite e4m3 value, the midpoints between neighbours (ties to even), values beyond the range and tiny values
    through the epilogue's conversion, against torch's float8_e4m3fn codes of the clamped value."""
    grid = torch.arange(0, 127, dtype=torch.uint8).view(FP8).float()            # 0 ... 448, all finite non-negative codes
    mids = (grid[:-1] + grid[1:]) / 2
    beyond = torch.tensor([448.5, 449.0, 463.9, 464.0, 470.0, 479.9, 480.0, 500.0, 1e4, 3e38])
    tiny = torch.tensor([1e-6, 2.0 ** -10, 2.0 ** -10 * 1.5, 2.0 ** -9 * 0.75, 2.0 ** -7 * 0.9])
    pos = torch.cat([grid, mids, beyond, tiny])
    vals = torch.cat([pos, -pos])
    got = _shift_only(vals)
    assert got.shape[1] == vals.numel()
    want = e4m3(vals).view(torch.uint8)
    for r in range(got.shape[0]):
        diff = (got[r] != want) & ~((values_of(got[r]) == 0) & (values_of(want) == 0))
        assert not diff.any(), f"codes differ at {vals[diff][:6].tolist()}: got {got[r][diff][:6].tolist()} want {want[diff][:6].tolist()}"
    assert (got[:, :pos.numel()][:, -len(tiny) - len(beyond):-len(tiny)] == 0x7E).all(), "beyond +448 must give the +448 code"
    assert (got[:, pos.numel():][:, -len(tiny) - len(beyond):-len(tiny)] == 0xFE).all(), "beyond -448 must give the -448 code"
    nan = (got & 0x7F) == 0x7F
    assert not nan.any(), "a conversion produced the NaN code"
    # ReLU clamps below at zero
    relu = values_of(_shift_only(vals, relu=True))
    assert (relu >= 0).all() and torch.equal(relu[0], values_of(e4m3(vals.clamp_min(0)).view(torch.uint8)))


def test_e4m3_decode_of_the_residual_round_trips():
    """Residual codes (every finite e4m3 value, both signs) decoded in the epilogue and encoded again: the same values;
    a residual at +-448 plus a positive / negative shift saturates to +-448, never NaN."""
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    cout = 256
    res = torch.zeros((1, 1, 1, 16, cout), dtype=torch.uint8)
    res[..., :codes.numel()] = codes
    got = _shift_only(torch.zeros(cout), residual=res.to(DEV).view(FP8))
    assert torch.equal(values_of(got[:, :codes.numel()]), values_of(codes).expand(16, -1))
    full = torch.full((1, 1, 1, 16, 64), 0x7E, dtype=torch.uint8)                        # +448 everywhere
    full[..., 32:] = 0xFE                                                               # -448
    shift = torch.cat([torch.full((32,), 100.0), torch.full((32,), -100.0)])
    sat = _shift_only(shift, residual=full.to(DEV).view(FP8))
    assert (sat[:, :32] == 0x7E).all() and (sat[:, 32:] == 0xFE).all()


def test_meanpool_fp8():
    g = torch.Generator().manual_seed(5)
    n, s, c = 3, 98, 921
    pitch = inference.fp8_channel_pitch(c)
    x = torch.zeros((n, 2, 7, 7, pitch), dtype=torch.uint8)
    x[..., :c] = e4m3(torch.randn((n, 2, 7, 7, c), generator=g) * 20).view(torch.uint8)
    got = inference.meanpool_fp8(x.to(DEV).view(FP8), c).cpu().double()
    ref = x[..., :c].view(FP8).double().reshape(n, s, c).mean(dim=1)
    assert got.shape == (n, c)
    assert torch.allclose(got, ref, rtol=1e-6, atol=1e-6), (got - ref).abs().max()


def test_rejects():
    d = ops.conv_desc((1, 64, 2, 4, 4), (64, 64, 1, 1, 1), (1, 1, 1), (0, 0, 0))
    blob = inference.pack_conv_fp8(d, torch.randn((64, 64, 1, 1, 1), device=DEV), None, None)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        inference.conv_fp8(d, torch.zeros((1, 2, 4, 4, 64), dtype=torch.bfloat16, device=DEV), blob)
    with pytest.raises(RuntimeError, match="does not match"):
        inference.conv_fp8(d, torch.zeros((1, 2, 4, 4, 32), dtype=torch.uint8, device=DEV).view(FP8), blob)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.meanpool_fp8(torch.zeros((1, 2, 4, 4, 64), dtype=torch.uint8).view(FP8), 64)


# ---- the engine -------------------------------------------------------------------------------------

def _model(name, seed, jitter=True):
    if name == "mc3_18":            # not reachable through get_network's dispatch (network.py:24-44)
        from zeroshotvideoclassification_amd import resnet
        model = network.Model(resnet.mc3_18)
    else:
        model = network.get_network(make_opt(name))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=seed, bn_jitter=jitter))
    return model.to(DEV).eval()


def _cos(a, b):
    return F.cosine_similarity(a.double(), b.double(), dim=1)


@pytest.mark.parametrize("name", ["r2plus1d_18", "r3d_18", "mc3_18"])
def test_engine_matches_fp32_eval_forward(name):
    """Same weights, eval mode: the e4m3 engine against the module's own fp32 eval forward and against the bf16 engine."""
    model = _model(name, seed=7)
    x = synthetic.synthetic_clips(3, 8, 64).to(DEV)
    with torch.no_grad():
        ref, _ = model(x)
    emb, second = inference.Fp8Engine(model)(x)
    assert second is None and emb.shape == ref.shape and emb.dtype == torch.float32
    assert torch.allclose(emb.norm(dim=1), torch.ones(3, device=DEV), atol=1e-5)
    cos = _cos(emb, ref)
    assert cos.min().item() >= COS_BAR, cos
    bf, _ = inference.Bf16Engine(model)(x)
    assert _cos(emb, bf).min().item() >= COS_BAR


def test_engine_against_the_reference_fixture_t32_batch_of_4():
    """The reference's own eval-mode embeddings of four 32-frame clips (tests/golden/r2plus1d_t32_batch.npz): cosine per clip
    >= 0.995 for the e4m3 engine, and the same bar against the bf16 engine on the same clips."""
    g = load_golden("r2plus1d_t32_batch")
    model = network.get_network(make_opt(str(g["meta_network"])))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=bool(g["meta_bn_jitter"])))
    model.to(DEV).eval()
    x = synthetic.synthetic_clips(int(g["meta_n"]), int(g["meta_frames"]), int(g["meta_size"]), seed=int(g["meta_seed"])).to(DEV)
    ref = torch.from_numpy(g["emb_eval_t32_f32"]).to(DEV)
    emb, _ = inference.Fp8Engine(model)(x)
    cos = _cos(emb, ref)
    print(f"[fp8] per-clip cosine to the reference fixture: {cos.tolist()}")
    assert cos.min().item() >= COS_BAR, cos
    bf, _ = inference.Bf16Engine(model)(x)
    cb = _cos(emb, bf)
    print(f"[fp8] per-clip cosine to the bf16 engine: {cb.tolist()}")
    assert cb.min().item() >= COS_BAR, cb


def test_batch_invariance():
    """No activation scale and a kernel choice that depends on the per-clip geometry only: a clip's pooled feature is
    bit-identical in a batch of 1 and a batch of 8, its embedding within 1e-6."""
    model = _model("r2plus1d_18", seed=4)
    eng = inference.Fp8Engine(model)
    x = synthetic.synthetic_clips(8, 16, 64, seed=41).to(DEV)
    clips = x.reshape(8, *x.shape[2:])
    pooled8 = eng.trunk(clips)
    emb8, _ = eng(x)
    for i in (0, 5):
        assert torch.equal(eng.trunk(clips[i:i + 1])[0], pooled8[i])
        emb1, _ = eng(x[i:i + 1])
        assert (emb1[0] - emb8[i]).abs().max().item() <= 1e-6


def test_evaluate_protocol_in_fp8():
    """train.evaluate(dtype=float8_e4m3fn) against dtype=bfloat16 on the setup of test_evaluate_protocol_in_bf16: top-5 may
    differ by at most one of the 8 clips, top-1 by at most one."""
    model = _model("r2plus1d_18", seed=5)
    table = synthetic.class_table(51)
    batches = []
    for i in range(2):
        x = synthetic.synthetic_clips(4, 8, 64, seed=300 + i)
        labels, z = synthetic.synthetic_targets(4, 51, rank=i)
        batches.append((x, labels, z))
    b = train.evaluate(model, batches, table, device=torch.device(DEV), splits=2, dtype=torch.bfloat16)
    f = train.evaluate(model, batches, table, device=torch.device(DEV), splits=2, dtype=FP8)
    print(f"[fp8] evaluate: bf16 {b}, fp8 {f}")
    assert b["n"] == f["n"] == 8
    assert abs(b["accuracy_top5"] - f["accuracy_top5"]) <= 12.5 + 1e-6
    assert abs(b["accuracy"] - f["accuracy"]) <= 12.5 + 1e-6
    with pytest.raises(RuntimeError, match="not supported"):
        train.evaluate(model, batches, table, device=torch.device(DEV), dtype=torch.float16)


def test_engine_cache_and_surface():
    model = _model("r2plus1d_18", seed=6)
    eng = inference.engine_for(model, FP8)
    assert isinstance(eng, inference.Fp8Engine)
    assert inference.engine_for(model, FP8) is eng, "cached while the weights are unchanged"
    assert type(inference.engine_for(model, torch.bfloat16)) is inference.Bf16Engine
    assert type(inference.engine_for(model, torch.float32)) is inference.Fp32Engine
    with torch.no_grad():
        model.model.layer2[0].conv1[0][0].weight.mul_(1.0)
    assert inference.engine_for(model, FP8) is not eng, "a write to a trunk weight rebuilds it"
    eng = inference.engine_for(model, FP8)
    _lib.note_raw_write()
    assert inference.engine_for(model, FP8) is not eng, "a raw write (HIP BatchNorm, FusedAdam, load_weights) rebuilds it"
    c3d = network.get_network(make_opt("c3d")).to(DEV).eval()
    with pytest.raises(RuntimeError, match="C3D has no fp8"):
        inference.engine_for(c3d, FP8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.engine_for(_model("r3d_18", seed=1).cpu(), FP8)
