"""The calibrated e4m3 engine of network.C3D: the channels-last e4m3 max-pool and the bf16 abs-max exactly, the
scale folding at the operator against a float64 convolution of the same operands, and the whole engine against an fp32 forward
and a fake-quantised simulation of the format, both written with plain torch ops on the CPU in this file.

The default test model proves nothing at the embedding (the biases decide it: two different noise clips give fp32 embeddings
with cosine 0.9999998), so the end-to-end tests use structured clips and two models: the keyed initialiser as it is ("quiet":
activations shrink from 0.7 to 0.01 over the eight layers) and with the convolution weights x 6.12 ("loud": they grow to 2e3).
The engine and the simulation differ in summation order only, i.e. by rounding flips: the engine's error against fp32 may be
1.5 x the simulation's own, and an engine without scales must be at least 2 x worse than the calibrated one.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import make_opt
from test_fp8_gpu import check_codes, codes_of, e4m3, grid_weights, to_ndhwc8
from zeroshotvideoclassification_amd import _lib, inference, network, ops, synthetic, train

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
LOUD = 6.12
# network.py:147-163: the eight relu(conv + bias) layers and the max-pool (kernel, padding) behind five of them
LAYERS = [("conv1", ((1, 2, 2), (0, 0, 0))), ("conv2", ((2, 2, 2), (0, 0, 0))), ("conv3a", None), ("conv3b", ((2, 2, 2), (0, 0, 0))),
          ("conv4a", None), ("conv4b", ((2, 2, 2), (0, 0, 0))), ("conv5a", None), ("conv5b", ((2, 2, 2), (0, 1, 1)))]


# ---- 1. the max-pool ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kernel,pad", [((2, 64, 4, 12, 12), (1, 2, 2), (0, 0, 0)), ((1, 128, 4, 6, 6), (2, 2, 2), (0, 0, 0)),
                                              ((3, 512, 2, 7, 7), (2, 2, 2), (0, 1, 1)), ((2, 45, 3, 5, 9), (1, 2, 2), (0, 1, 0))])
def test_maxpool3d_channels_last_fp8(shape, kernel, pad):
    """zsv_maxpool3d_fp8 against torch's MaxPool3d on the decoded values: exact.  Negative values, both zeros, subnormals and
    +-448 are among the inputs, one channel is negative throughout, and the input's pad channels hold a non-zero code."""
    g = torch.Generator().manual_seed(sum(shape))
    n, c, t, h, w = shape
    x = torch.randn(shape, generator=g) * 40.0
    special = torch.tensor([0.0, -0.0, 2.0 ** -9, -2.0 ** -9, 3 * 2.0 ** -9, -7 * 2.0 ** -9, 448.0, -448.0, 1000.0, -1000.0])
    where = torch.randint(0, x.numel(), (x.numel() // 8,), generator=g)
    x.view(-1)[where] = special[torch.randint(0, len(special), where.shape, generator=g)]
    x[:, 1] = -x[:, 1].abs() - 2.0 ** -9                     # a channel without a non-negative value
    codes = e4m3(x).view(torch.uint8)
    values = codes.view(FP8).float()
    assert (codes == 0x7E).any() and (codes == 0xFE).any() and (codes == 0x80).any() and (codes == 0x00).any()
    assert (((codes & 0x78) == 0) & ((codes & 0x07) != 0)).any(), "subnormals"
    pitch = inference.fp8_channel_pitch(c)
    cl = torch.full((n, t, h, w, pitch), 0x55, dtype=torch.uint8)
    cl[..., :c] = codes.permute(0, 2, 3, 4, 1)
    y = inference.maxpool3d_fp8(cl.to(DEV).view(FP8), c, kernel, pad)
    ref = F.max_pool3d(values, kernel, kernel, pad)
    got = codes_of(y)
    assert y.dtype == FP8 and tuple(got.shape) == (n,) + tuple(ref.shape[2:]) + (pitch,)
    assert torch.equal(got[..., :c].permute(0, 4, 1, 2, 3).contiguous().view(FP8).float(), ref)
    assert torch.count_nonzero(got[..., c:]) == 0, "pad channels must be written as zero"


# ---- 2. the abs-max ----------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 255, 4 * 256 + 3, 2 ** 20 + 7])
def test_absmax_bf16(count):
    g = torch.Generator().manual_seed(count)
    base = torch.randn(count + 1, generator=g).to(torch.bfloat16)
    for name, pos, value in (("first", 0, 7.5), ("last", count - 1, 9.25), ("negative", count // 2, -11.0)):
        x = base[:count].clone()
        x[pos] = value
        want = x.float().abs().max().item()
        assert want == abs(value)
        amax = torch.zeros(3, device=DEV)
        inference.absmax_bf16(x.to(DEV), amax[1:2])
        assert amax.tolist() == [0.0, want, 0.0], name
    x = base[:count].to(DEV)
    want = x.float().abs().max().item()
    amax = torch.tensor([1e4], device=DEV)
    inference.absmax_bf16(x, amax)
    assert amax.item() == 1e4, "a larger value already in *amax survives"
    # two calls fold; the second starts 2 bytes behind a 16-byte boundary (the elements in front of the aligned middle)
    amax = torch.zeros(1, device=DEV)
    both = base.to(DEV)
    half = (count + 1) // 2
    inference.absmax_bf16(both[:half].contiguous(), amax)
    first = amax.item()
    inference.absmax_bf16(both[1:], amax)
    assert first == both[:half].float().abs().max().item()
    assert amax.item() == max(first, both[1:].float().abs().max().item())


def test_absmax_bf16_non_finite():
    x = torch.randn(1000).to(torch.bfloat16)
    x[17] = float("-inf")
    amax = torch.zeros(1, device=DEV)
    inference.absmax_bf16(x.to(DEV), amax)
    assert amax.item() == float("inf")
    x[500] = float("nan")
    inference.absmax_bf16(x.to(DEV), amax)
    assert np.isnan(amax.item())
    with pytest.raises(RuntimeError, match="bf16"):
        inference.absmax_bf16(torch.zeros(8, device=DEV), amax)


# ---- 3. scale folding at the operator ------------------------------------------------------------------

@pytest.mark.parametrize("n,cin,cout,thw", [(2, 64, 128, (4, 10, 10)), (1, 128, 256, (4, 6, 6)), (1, 256, 512, (2, 7, 7)),
                                             (1, 512, 512, (2, 4, 4))])
def test_conv_fp8_folds_the_activation_scales(n, cin, cout, thw):
    """C3D's channel pairs, 3x3x3 / stride 1 / padding 1, packed with scale = a_{l-1} / a_l = 2^-3 and shift = bias / a_l
    (a_l = 4): sat(relu(acc * wscale + shift)) against the float64 convolution of the same e4m3 operands, by the rule of
    test_fp8_gpu.py (codes equal except within fp32 summation noise of a rounding midpoint)."""
    k, s, p = (3, 3, 3), (1, 1, 1), (1, 1, 1)
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x = e4m3(torch.randn((n, cin) + thw, generator=g) * 4.0).double()
    wgt, q, rs = grid_weights(g, cout, cin, k)               # w = q * rs per row: w * 2^-3 quantises to q exactly
    bias = torch.randn(cout, generator=g) * 8.0
    scale, shift = torch.full((cout,), 2.0 ** -3), bias / 4
    rows = (rs * 2.0 ** -3).view(1, -1, 1, 1, 1)
    y = (F.conv3d(x, q, stride=s, padding=p) * rows + shift.double().view(1, -1, 1, 1, 1)).clamp_min(0)
    mag = F.conv3d(x.abs(), q.abs(), stride=s, padding=p) * rows
    tol = mag * (cin * 27) * 2.0 ** -23 + y.abs() * 2.0 ** -22 + 1e-30
    d = ops.conv_desc(x.shape, wgt.shape, s, p)
    blob = inference.pack_conv_fp8(d, wgt.to(DEV), scale.to(DEV), shift.to(DEV))
    yk = inference.conv_fp8(d, to_ndhwc8(x, inference.fp8_channel_pitch(cin)), blob, None, True)
    codes = codes_of(yk)
    assert torch.count_nonzero(codes[..., cout:]) == 0
    flips = check_codes(codes[..., :cout].permute(0, 4, 1, 2, 3), y, tol, f"{cin}->{cout} on {thw}")
    assert (y > 1.0).float().mean().item() > 0.1, "the case must exercise non-zero outputs"
    print(f"[fp8 c3d] {cin}->{cout} on {thw}: {flips} of {y.numel()} codes on the other side of a midpoint")


def test_clip_conv_fp8_folds_the_first_scale():
    """The clip convolution 3 -> 64 (bf16 operands, e4m3 output) packed with scale = 1 / a_1 = 2^-2 and shift = bias / a_1."""
    n, thw, cout = 2, (4, 12, 12), 64
    g = torch.Generator().manual_seed(364)
    u8 = torch.randint(0, 256, (n, 3) + thw, generator=g)
    x = ((u8.float() / 255 - 1) / 2).to(torch.bfloat16).float()                  # bf16-exact clips
    wgt = e4m3(torch.randn((cout, 3, 3, 3, 3), generator=g) * 60.0).float() * 2.0 ** -3         # 4 significant bits: bf16-exact
    bias = torch.randn(cout, generator=g) * 8.0
    scale, shift = torch.full((cout,), 2.0 ** -2), bias / 4
    w4 = wgt.double() * 2.0 ** -2
    y = (F.conv3d(x.double(), w4, padding=1) + shift.double().view(1, -1, 1, 1, 1)).clamp_min(0)
    mag = F.conv3d(x.double().abs(), w4.abs(), padding=1)
    tol = mag * 81 * 2.0 ** -23 + y.abs() * 2.0 ** -22 + 1e-30
    geo = inference.ConvGeometry(torch.nn.Conv3d(3, cout, 3, padding=1))
    xb, wo = geo.clip_input(x.to(DEV))
    d = geo.desc(n, thw[0], xb.shape[2], xb.shape[3], wo)
    blob = inference.pack_conv_fp8(d, wgt.to(DEV), scale.to(DEV), shift.to(DEV))
    codes = codes_of(inference.conv_fp8(d, xb, blob, None, True))
    assert tuple(codes.shape) == (n,) + thw + (64,)
    check_codes(codes.permute(0, 4, 1, 2, 3), y, tol, "clip 3->64")
    assert (y > 1.0).float().mean().item() > 0.1


# ---- the end-to-end inputs, the fp32 forward and the simulation (CPU, plain torch) -----------------------------------

def structured_clips(seed, n):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, 4, 7, 7, generator=g)
    up = F.interpolate(low, size=(16, 112, 112), mode="trilinear", align_corners=False)
    u8 = (up * 255 + 8 * torch.randn(up.shape, generator=g)).clamp(0, 255).round()
    return (u8 / 255 - 1) / 2


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def clips_of(name):
    return cached(("clips", name), lambda: structured_clips(*{"calibration": (99, 2), "evaluation": (1234, 3), "four": (1234, 4)}[name]))


def weights_of(mult):
    def make():
        model = network.get_network(make_opt("c3d"))
        sd = synthetic.keyed_state_dict(model.state_dict(), seed=0)
        for name, _ in LAYERS:
            sd[name + ".weight"] = sd[name + ".weight"] * mult
        return sd
    return cached(("weights", mult), make)


def device_model(mult):
    model = network.get_network(make_opt("c3d"))
    model.load_state_dict(weights_of(mult))
    return model.to(DEV).eval()


def sat(t):
    return t.clamp(-448.0, 448.0).to(FP8).float()


def fp32_forward(mult, name):
    """(features (N, 8192), [amax of each layer's output]) of the fp32 eval forward."""
    def make():
        sd, x, amax = weights_of(mult), clips_of(name), []
        with torch.no_grad():
            for conv, pool in LAYERS:
                x = F.relu(F.conv3d(x, sd[conv + ".weight"], sd[conv + ".bias"], padding=1))
                amax.append(x.max().item())
                if pool is not None:
                    x = F.max_pool3d(x, pool[0], pool[0], pool[1])
        return x.reshape(x.shape[0], -1), amax
    return cached(("fp32", mult, name), make)


def simulated(mult, name, scales):
    """The format, fake-quantised: e4m3 weights per produced channel as zsv_conv3d_fp8_pack forms them, saturating e4m3
    activations stored as true / a_l, bf16 operands for the clip convolution.  -> features (N, 8192) times a_8."""
    def make():
        sd, q, before = weights_of(mult), clips_of(name), 1.0
        with torch.no_grad():
            for l, (conv, pool) in enumerate(LAYERS):
                w, b, a = sd[conv + ".weight"], sd[conv + ".bias"], scales[l]
                if l == 0:
                    y = F.conv3d(q.to(torch.bfloat16).float(), (w / a).to(torch.bfloat16).float(), padding=1)
                else:
                    ws = w * (before / a)
                    rows = ws.abs().amax(dim=(1, 2, 3, 4)) / 448.0
                    wq = sat(ws / rows.view(-1, 1, 1, 1, 1))
                    y = F.conv3d(q, wq, padding=1) * rows.view(1, -1, 1, 1, 1)
                q = sat(F.relu(y + (b / a).view(1, -1, 1, 1, 1)))
                if pool is not None:
                    q = F.max_pool3d(q, pool[0], pool[0], pool[1])
                before = a
        return q.reshape(q.shape[0], -1) * scales[-1]
    return cached(("sim", mult, name, tuple(scales)), make)


def head(mult, feats, bs, nc):
    """network.py:166-179 in fp32: fc6 + ReLU, the clip mean, the regressor, L2 normalisation."""
    sd = weights_of(mult)
    with torch.no_grad():
        a = F.relu(F.linear(feats, sd["fc6.weight"], sd["fc6.bias"]))
        a = a.reshape(bs, nc, -1).mean(1)
        return F.normalize(F.linear(a, sd["regressor.weight"], sd["regressor.bias"]), dim=-1)


def rel_err(f, ref):
    return ((f.double() - ref.double()).norm(dim=1) / ref.double().norm(dim=1)).tolist()


def is_power_of_two(v):
    return v > 0 and np.frexp(v)[0] == 0.5


# ---- 4. engine features ------------------------------------------------------------------------------

@pytest.mark.parametrize("mult", [1.0, LOUD], ids=["quiet", "loud"])
def test_engine_features_against_fp32_and_the_simulation(mult):
    """(a) per clip the engine's relative L2 error against fp32 is at most 1.5 x the simulation's own (summation order is the
    only difference: rounding flips); (b) an engine with scales 1 is at least 2 x worse per clip (quiet: the late layers fall into
    the subnormals, loud: conv5b saturates); (c) no stored code is +-448 and the scales are powers of two that follow from the
    fp32 maxima of the calibration clips (bf16 rounds each layer by <= 2^-9 relative: 2 % over the eight layers)."""
    model = device_model(mult)
    scales = inference.calibrate_fp8(model, clips_of("calibration").to(DEV))
    assert scales == inference.fp8_scales(model) and len(scales) == 8 and all(is_power_of_two(s) for s in scales)
    for s, amax in zip(scales, fp32_forward(mult, "calibration")[1]):
        assert inference.fp8_scale(amax * 0.98) <= s <= inference.fp8_scale(amax * 1.02), (scales, amax)
    ref, amax32 = fp32_forward(mult, "evaluation")
    sim = simulated(mult, "evaluation", scales)
    taps = []
    engine = inference.Fp8EngineC3D(model)
    feats = engine.features(clips_of("evaluation").to(DEV), taps=taps)
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (3, 8192) and len(taps) == 8
    err, err_sim = rel_err(feats.cpu(), ref), rel_err(sim, ref)
    unscaled = inference.Fp8EngineC3D(model, scales=[1.0] * 8)
    assert unscaled.scales == (1.0,) * 8 and inference.fp8_scales(model) == scales
    err_unscaled = rel_err(unscaled.features(clips_of("evaluation").to(DEV)).cpu(), ref)
    stored = [float(codes_of(t).view(FP8).float().max()) for t in taps]
    print(f"[fp8 c3d] x{mult}: fp32 amax per layer {['%.3g' % v for v in amax32]}")
    print(f"[fp8 c3d] x{mult}: scales {scales}; largest stored value per layer {stored}")
    print(f"[fp8 c3d] x{mult}: error per clip: engine {err}, simulation {err_sim}, unscaled engine {err_unscaled}")
    for t in taps:
        assert t.dtype == FP8
        magnitude = codes_of(t) & 0x7F
        assert not (magnitude == 0x7E).any(), "a stored activation saturated"
        assert not (magnitude == 0x7F).any(), "a NaN code"
    for e, es, eu in zip(err, err_sim, err_unscaled):
        assert e <= 1.5 * es, (err, err_sim)
        assert eu >= 2.0 * e, (err_unscaled, err)


# ---- 5. embedding and protocol -----------------------------------------------------------------------

def test_embedding_and_protocol_on_the_loud_model():
    model = device_model(LOUD)
    with pytest.raises(RuntimeError, match="C3D has no fp8"):
        inference.engine_for(model, FP8)
    with pytest.raises(RuntimeError, match="C3D has no fp8"):
        inference.Fp8EngineC3D(model)
    scales = inference.calibrate_fp8(model, clips_of("calibration").to(DEV))
    x = clips_of("four").reshape(2, 2, 3, 16, 112, 112)
    ref = head(LOUD, fp32_forward(LOUD, "four")[0], 2, 2)
    between = F.cosine_similarity(ref[0:1].double(), ref[1:2].double()).item()
    assert between <= 0.995, f"the inputs do not discriminate: the two rows' fp32 embeddings have cosine {between}"
    sim = head(LOUD, simulated(LOUD, "four", scales), 2, 2)
    engine = inference.engine_for(model, FP8)
    assert type(engine) is inference.Fp8EngineC3D and engine.scales == scales
    emb = engine(x.to(DEV))
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (2, 300)
    assert torch.allclose(emb.norm(dim=1), torch.ones(2, device=DEV), atol=1e-5)
    cos = F.cosine_similarity(emb.cpu().double(), ref.double(), dim=1)
    cos_sim = F.cosine_similarity(sim.double(), ref.double(), dim=1)
    print(f"[fp8 c3d] embedding: cosine between the rows {between}; to fp32: engine {cos.tolist()}, simulation {cos_sim.tolist()}")
    for c, cs in zip(cos.tolist(), cos_sim.tolist()):
        assert 1.0 - c <= 1.5 * (1.0 - cs) + 1e-6, (cos, cos_sim)
    assert inference.engine_for(model, FP8) is engine, "cached while the weights and the scales are unchanged"
    _lib.note_raw_write()
    again = inference.engine_for(model, FP8)
    assert again is not engine and again.scales == scales, "a raw write rebuilds it with the same scales"
    inference.set_fp8_scales(model, [2 * s for s in scales])
    other = inference.engine_for(model, FP8)
    assert other is not again and other.scales == tuple(2 * s for s in scales), "the scales are part of the cache key"
    inference.set_fp8_scales(model, scales)
    table = synthetic.class_table(51, seed=5)
    labels, z = synthetic.synthetic_targets(2, 51, seed=5)
    out = train.evaluate(model, [(x, labels, z)], table, device=torch.device(DEV), dtype=FP8, splits=0)
    assert out["n"] == 2


# ---- 6. batch invariance, 7. calibration folds ---------------------------------------------------------

def test_batch_invariance():
    """Static scales and a kernel choice per clip geometry: a clip's features are bit-identical alone and in a batch of 3."""
    model = device_model(LOUD)
    inference.calibrate_fp8(model, clips_of("calibration").to(DEV))
    engine = inference.Fp8EngineC3D(model)
    x = clips_of("evaluation").to(DEV)
    assert torch.equal(engine.features(x[0:1])[0], engine.features(x)[0])


def test_calibration_folds_over_batches():
    model = device_model(LOUD)
    a, b = clips_of("calibration")[0:1].to(DEV), (clips_of("calibration")[1:2] * 0.05).to(DEV)
    sa = inference.calibrate_fp8(model, a)
    assert inference.fp8_scales(model) == sa
    sb = inference.calibrate_fp8(model, b)
    assert inference.fp8_scales(model) == sb and sa != sb, "the two batches must calibrate differently for this test to say something"
    both = inference.calibrate_fp8(model, [a, b])
    assert both == tuple(max(p, q) for p, q in zip(sa, sb))
    assert inference.fp8_scales(model) == both
    assert inference.calibrate_fp8(model, iter([b, a])) == both
    assert inference.calibrate_fp8(model, torch.cat([a, b]).unsqueeze(0)) == both          # (bs, nc, 3, T, H, W)
    assert inference.calibrate_fp8(model, a, headroom=8.0) == tuple(2 * s for s in sa)
