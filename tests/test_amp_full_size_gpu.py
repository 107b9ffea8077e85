"""The bf16 training path at the size the benchmark runs it (``extra.train_bf16``: 22 clips of 3x16x112x112).

The per-op tests of ``test_amp_gpu.py`` stop at about 3x8x28x28 and the model-level ones at 2-4 clips of 8x56x56; the kernel
choice depends on the size (``bf16_fwd_impl``'s "small" test, ``wgrad_cl_plan``'s slice count, the BatchNorm reductions over
1.1 M rows, the per-clip offsets of the last clip, the ragged last voxel tile).  Pinned here at size:

1. Every convolution geometry of the benchmarked step (25 of R(2+1)D-18, 7 of C3D) at N = 22, each op the step calls, against a
   float64 reference of the SAME bf16-rounded operands.  A whole-tensor fp64 convolution is out of reach on the host, so the
   convolutions are checked on a sample: clips {0, 11, 21} x at most 24 channels for the forward and the input gradient (each
   output (n, c) depends only on clip n and channel c's weights; the sample holds channel 0, the last channel and one channel of
   every row tile, the ragged last one included), all 22 clips x at most 16 x 16 channels for the weight gradient (the last input
   panel and the last output group included).  Element-wise and reduction kernels are checked on the whole tensor.  Bars (those of
   ``test_amp_gpu.py`` / ``test_bf16_gpu.py``):
   * forward (``conv_bf16_stats``; C3D: ``conv_bf16`` with bias + ReLU): 2^-8 relative + 1e-3 absolute per element; pad channels
     zero; the statistics partials add up to the fp64 sums of the stored z within 1e-5;
   * input gradient (``Bf16TrainPath._dgrad``): 2^-7 of the range; the positions no tap reaches are exactly zero;
   * weight gradient (``Bf16TrainPath._wgrad``): 1e-3 of the range; and, one geometry per kernel mode, EXACT on integer operands
     (a lost border voxel is four times under that bar at this size);
   * BatchNorm (``bn_cl_fwd_train`` with and without ``conv_stats``, ``bn_cl_bwd`` with and without residual / ReLU / ``fwd_coef``):
     y 2^-7 of the range, mean 1e-5, invstd / running statistics 1e-5 relative, dz 2^-6 of the range, dgamma / dbeta 2e-3 of the range;
   * C3D's max-pools and ``relu_bias_bwd_cl``: exact, bias gradient 1e-5.
   The other route of S1, S3, T0, T1, S2 and T3 (``ZSV_BF16_NO_*`` switches) is held to the same sample and bars, with a kernel
   trace showing the switch changed the kernel.
2. The whole step against the imported reference under ``torch.autocast("cpu", bfloat16)`` and the fp32 HIP path: R(2+1)D-18
   train mode at 22 clips (the bars of ``test_autocast_training_step_against_the_reference_under_cpu_autocast``), C3D eval mode
   at 4 clips (those of ``test_c3d_autocast_training_step_against_the_reference_under_cpu_autocast``).
3. Two eager full-size steps of R(2+1)D-18 agree bit for bit, and so does one ``amp.autocast(graph=True)`` step.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import make_opt  # noqa: E402
from zeroshotvideoclassification_amd import amp, inference, network, ops, synthetic, train  # noqa: E402

DEV = "cuda"
N = 22                                  # clips of the benchmarked step
CLIPS = (0, N // 2, N - 1)              # the forward / input-gradient sample: first, middle and last clip

# name, Cin, Cout, (T, H, W) of the input, kernel, stride, padding -- the distinct convolutions of a 16x112x112 forward.
# Comments: the kernel instantiation each op reaches at N = 22 (conv_bf16.hip bf16_fwd_impl, wgrad_bf16.hip wgrad_cl_plan);
# "fwd" is the forward with statistics, "dgrad" the stride-1 problems of the input gradient, "wgrad" the weight-gradient mode.
R2P1D = [
    # fwd conv_bf16_kernel<4,4,1,4> (folded clip form) | dgrad none (first layer) | wgrad fp32 zsv_conv3d_wgrad on the clip
    ("S0", 3, 45, (16, 112, 112), (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    # fwd conv_bf16_tsame_kernel<4,4,1,4,8> | dgrad conv_bf16_tsame_kernel<4,4,1,4,8> | wgrad mode 1, 384 slices x 90 chunks
    ("T0", 45, 64, (16, 56, 56), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_same_kernel<9,4,1,4> | dgrad conv_bf16_same9_kernel<4,4,1,4,24> | wgrad mode 0, 128 slices x 270 chunks
    ("S1", 64, 144, (16, 56, 56), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_tsame_kernel<4,4,1,4,8> | dgrad conv_bf16_kernel<9,4,1,4> | wgrad mode 1, 384 x 90
    ("T1", 144, 64, (16, 56, 56), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_kernel<8,4,1,4> (539 tiles) | dgrad conv_bf16_kernel<4,4,1,4>, 7 of 8 classes empty | wgrad mode 4, 360 x 12
    ("P1", 64, 128, (16, 56, 56), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    # fwd conv_bf16_kernel<8,4,1,4> (2156 tiles) | dgrad 4 x conv_bf16_kernel<4,4,1,4> | wgrad mode 2, 77 x 112
    ("S2", 64, 230, (16, 56, 56), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    # fwd conv_bf16_kernel<8,4,1,4> (539 tiles) | dgrad 2 x conv_bf16_kernel<8,4,1,4> | wgrad mode 3, 96 x 45
    ("T2", 230, 128, (16, 28, 28), (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_same_kernel<8,4,1,4> (1078 tiles) | dgrad conv_bf16_same9_kernel<8,4,1,4,20> | wgrad mode 0, 39 x 111
    ("S3", 128, 230, (8, 28, 28), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_kernel<8,4,1,4> (539 tiles) | dgrad conv_bf16_kernel<8,4,1,4> | wgrad mode 1, 96 x 45
    ("T3", 230, 128, (8, 28, 28), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_same_kernel<9,4,1,4> | dgrad conv_bf16_same9_kernel<8,4,1,4,20> | wgrad mode 0, 32 x 135
    ("S4", 128, 288, (8, 28, 28), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_kernel<8,4,1,4> (539 tiles) | dgrad conv_bf16_kernel<9,4,1,4> | wgrad mode 1, 96 x 45
    ("T4", 288, 128, (8, 28, 28), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_kernel<4,4,2,2> (136 tiles) | dgrad conv_bf16_kernel<4,4,2,2>, 7 classes empty | wgrad mode 4, 90 x 6
    ("P2", 128, 256, (8, 28, 28), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    # fwd conv_bf16_kernel<8,4,1,4> (540 tiles) | dgrad 4 x conv_bf16_kernel<4,4,2,2> | wgrad mode 2, 20 x 54
    ("S5", 128, 460, (8, 28, 28), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad 2 x conv_bf16_kernel<4,4,2,2> | wgrad mode 3, 24 x 23
    ("T5", 460, 256, (8, 14, 14), (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 10 x 54
    ("S6", 256, 460, (4, 14, 14), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 1, 24 x 23
    ("T6", 460, 256, (4, 14, 14), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_same_kernel<9,4,1,4> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 8 x 68
    ("S7", 256, 576, (4, 14, 14), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<9,4,1,4> | wgrad mode 1, 24 x 23
    ("T7", 576, 256, (4, 14, 14), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<4,4,2,2>, 7 classes empty | wgrad mode 4, 23 x 3
    ("P3", 256, 512, (4, 14, 14), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    # fwd conv_bf16_kernel<9,4,1,4> (1008 rows: ragged 921) | dgrad 4 x conv_bf16_kernel<4,4,2,2> | wgrad mode 2, 5 x 27
    ("S8", 256, 921, (4, 14, 14), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad 2 x conv_bf16_kernel<9,4,1,4> | wgrad mode 3, 7 x 10
    ("T8", 921, 512, (4, 7, 7), (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_same_kernel<9,4,1,4> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 3 x 23
    ("S9", 512, 921, (2, 7, 7), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<9,4,1,4> | wgrad mode 1, 7 x 10
    ("T9", 921, 512, (2, 7, 7), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    # fwd conv_bf16_kernel<4,4,2,2> (81 tiles) | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 2 x 34
    ("S10", 512, 1152, (2, 7, 7), (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 1, 6 x 12
    ("T10", 1152, 512, (2, 7, 7), (3, 1, 1), (1, 1, 1), (1, 0, 0)),
]
C3D = [
    # fwd conv_bf16_kernel<4,4,1,4> (folded clip form) | dgrad none | wgrad fp32 zsv_conv3d_wgrad on the clip
    ("C1", 3, 64, (16, 112, 112), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    # fwd conv_bf16_same_kernel<8,4,1,4> | dgrad conv_bf16_same9_kernel<4,4,1,4,24> | wgrad mode 0, 43 x 803
    ("C2", 64, 128, (16, 56, 56), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    # fwd conv_bf16_same9_kernel<8,4,1,4,20> | dgrad conv_bf16_same9_kernel<8,4,1,4,20> | wgrad mode 0, 11 x 392
    ("C3a", 128, 256, (8, 28, 28), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    # fwd conv_bf16_same9_kernel<8,4,1,4,20> | dgrad conv_bf16_same9_kernel<8,4,1,4,20> | wgrad mode 0, 6 x 719
    ("C3b", 256, 256, (8, 28, 28), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 3 x 180
    ("C4a", 256, 512, (4, 14, 14), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 2 x 270
    ("C4b", 512, 512, (4, 14, 14), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    # fwd conv_bf16_kernel<4,4,2,2> (36 tiles) | dgrad conv_bf16_kernel<4,4,2,2> | wgrad mode 0, 2 x 34
    ("C5", 512, 512, (2, 7, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
]
GEOMS = {g[0]: g for g in R2P1D + C3D}

# the other route of a geometry, held to the same sample and bars: the switch, the kernel it reaches instead and the default
# route's kernel (both checked in a kernel trace of the case)
ALT_FWD = [("S1", "ZSV_BF16_NO_SAME", "conv_bf16_kernel<9,4,1,4,", "conv_bf16_same_kernel<9,4,1,4,"),
           ("S3", "ZSV_BF16_NO_SAME", "conv_bf16_kernel<8,4,1,4,", "conv_bf16_same_kernel<8,4,1,4,"),
           ("T1", "ZSV_BF16_NO_TSAME", "conv_bf16_kernel<4,4,1,4,", "conv_bf16_tsame_kernel<4,4,1,4,8,"),
           ("T0", "ZSV_BF16_NO_TSAME", "conv_bf16_kernel<4,4,1,4,", "conv_bf16_tsame_kernel<4,4,1,4,8,")]
ALT_DGRAD = [("S1", "ZSV_BF16_NO_SAME9", "conv_bf16_same_kernel<4,4,1,4,", "conv_bf16_same9_kernel<4,4,1,4,24,"),
             ("S1", "ZSV_BF16_NO_SAME", "conv_bf16_kernel<4,4,1,4,", "conv_bf16_same9_kernel<4,4,1,4,24,"),
             ("S3", "ZSV_BF16_NO_SAME9", "conv_bf16_same_kernel<8,4,1,4,", "conv_bf16_same9_kernel<8,4,1,4,20,")]
ALT_WGRAD = [("S1", "ZSV_BF16_NO_WGRAD"),       # the converted-operand fp32 path (zsv_conv3d_wgrad)
             ("T1", "ZSV_BF16_NO_WGRAD"),
             ("S2", "ZSV_BF16_NO_WGRAD_GATHER"),
             ("T3", "ZSV_BF16_NO_WGRAD")]


@pytest.fixture(autouse=True, scope="module")
def _host_threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    yield


def _randn(shape, seed, scale=1.0, shift=0.0):
    """bf16-rounded normal values, drawn on the device (fp32 NCDHW)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(torch.bfloat16).float()


def _channels(c, k, seed):
    """At most ``k`` of ``c`` channels: 0, c - 1 and one seeded random pick in each of the k - 2 equal stretches of c / (k - 2)
    channels between them (so one in every row tile / input panel / output group at least that wide)."""
    if c <= k:
        return list(range(c))
    rng = np.random.default_rng(seed)
    edges = np.linspace(0, c, k - 1)
    picks = {0, c - 1}
    for lo, hi in zip(edges[:-1], edges[1:]):
        lo, hi = int(np.ceil(lo)), max(int(np.ceil(lo)) + 1, int(np.floor(hi)))
        picks.add(int(rng.integers(lo, hi)))
    picks = sorted(picks)
    while len(picks) > k:                  # (rounding at the stretch ends can add one): drop an interior pick
        picks.pop(len(picks) // 2)
    return picks


def _out_dims(t, h, w, k, s, p):
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((t, h, w), k, s, p))


class _Problem:
    """One full-size convolution: bf16-rounded x (fp32 NCDHW on the device), weights, the unit and descriptor of the training
    path, and x in the layout the forward reads (channels-last bf16, or the folded clip form with its materialised border)."""

    def __init__(self, name, bias=False):
        _, cin, cout, (t, h, w), k, s, p = GEOMS[name]
        seed = sum(map(ord, name))
        self.name, self.cin, self.cout, self.k, self.s, self.p = name, cin, cout, k, s, p
        self.x = _randn((N, cin, t, h, w), seed)
        fan = cin * k[0] * k[1] * k[2]
        self.w = _randn((cout, cin) + k, seed + 1, fan ** -0.5)
        self.b = _randn((cout,), seed + 2, 0.1) if bias else None
        conv = torch.nn.Conv3d(cin, cout, k, stride=s, padding=p, bias=bias).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(self.w)
            if bias:
                conv.bias.copy_(self.b)
        self.unit = amp._Unit(conv, None, True, plain=True) if bias else amp._Unit(conv, torch.nn.BatchNorm3d(cout).to(DEV), False)
        self.out = _out_dims(t, h, w, k, s, p)
        if self.unit.folded:
            hp, wp = h + 2 * p[1], max(w + 2 * p[2], (self.out[2] - 1) * s[2] + 8)
            self.xb = amp.clip_to_bf16(self.x, p[1], p[2], hp, wp)
            self.desc = self.unit.desc(N, t, hp, wp, self.out[2])
        else:
            self.xb = amp.ncdhw_to_cl_bf16(self.x)
            self.desc = self.unit.desc(N, t, h, w)
        assert (self.desc.To, self.desc.Ho, self.desc.Wo) == self.out

    def record(self):
        r = amp._Record()
        r.unit, r.desc, r.x, r.clips = self.unit, self.desc, self.xb, (self.x if self.unit.folded else None)
        return r

    def dz(self):
        return _randn((N, self.cout) + self.out, sum(map(ord, self.name)) + 3)


def _cl_sample(t_cl, clips, chans):
    """[N][T][H][W][Cp] -> (len(clips), len(chans), T, H, W) float64 on the host."""
    return t_cl[list(clips)][..., chans].permute(0, 4, 1, 2, 3).double().cpu()


# ---- 1. per-op kernels at every geometry -------------------------------------------------------------------------------
def _check_forward(pb, z):
    chans = _channels(pb.cout, 24, len(pb.name))
    x64 = pb.x[list(CLIPS)].double().cpu()
    ref = F.conv3d(x64, pb.w[chans].double().cpu(), None if pb.b is None else pb.b[chans].double().cpu(), pb.s, pb.p)
    if pb.b is not None:
        ref = torch.relu(ref)
    got = _cl_sample(z, CLIPS, chans)
    assert got.shape == ref.shape
    err = (got - ref).abs()
    bad = err > ref.abs() * 2.0 ** -8 + 1e-3
    assert not bool(bad.any()), (pb.name, int(bad.sum()), float(err.max()))
    assert float(z[..., pb.cout:].float().abs().sum()) == 0.0, "pad channels must be zero"


def _check_partials(z, partials, rows, c):
    assert 0 < rows <= partials.shape[0]
    zf = z[..., :c].double().reshape(-1, c)
    s1, s2 = partials[:rows, 0, :c].double().sum(0), partials[:rows, 1, :c].double().sum(0)
    assert float((s1 - zf.sum(0)).abs().max()) <= 1e-5 * float(zf.abs().sum(0).max())
    assert float((s2 / (zf * zf).sum(0) - 1).abs().max()) <= 1e-5


def _bn(c, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm3d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn.to(DEV).train()


def _check_bn_forward(z, c, bn0, bn, y, mean, invstd, residual=None, relu=True):
    """The train-mode BatchNorm forward (+ residual) (+ ReLU) against fp64 on the whole tensor; ``bn0``: the module's state before."""
    zf = z[..., :c].double().reshape(-1, c)
    m64 = zf.mean(0)
    v64 = zf.var(0, unbiased=False)
    assert float((mean.double() - m64).abs().max()) < 1e-5
    assert float((invstd.double() * torch.sqrt(v64 + bn.eps) - 1).abs().max()) < 1e-5
    mom = bn.momentum
    rm = (1 - mom) * bn0["running_mean"].double() + mom * m64
    rv = (1 - mom) * bn0["running_var"].double() + mom * zf.var(0, unbiased=True)
    assert float((bn.running_mean.double() - rm).abs().max()) < 1e-5
    assert float((bn.running_var.double() / rv - 1).abs().max()) < 1e-5
    assert int(bn.num_batches_tracked) == int(bn0["num_batches_tracked"]) + 1
    a = bn.weight.double() / torch.sqrt(v64 + bn.eps)
    pre = (zf - m64) * a + bn.bias.double()
    if residual is not None:
        pre = pre + residual[..., :c].double().reshape(-1, c)
    y64 = torch.relu(pre) if relu else pre
    got = y[..., :c].double().reshape(-1, c)
    assert float((got - y64).abs().max()) <= float(y64.abs().max()) * 2.0 ** -7
    assert float(y[..., c:].float().abs().sum()) == 0.0


def _run_forward(pb):
    blob = amp.pack_conv(pb.desc, pb.w, None, pb.b)
    if pb.b is not None:                            # C3D: relu(conv(x) + bias), no statistics
        z = amp.conv_bf16(pb.desc, pb.xb, blob, None, True)
        torch.cuda.synchronize()
        _check_forward(pb, z)
        return
    z0 = amp.conv_bf16(pb.desc, pb.xb, blob, None, False)
    z, partials, rows = amp.conv_bf16_stats(pb.desc, pb.xb, blob)
    torch.cuda.synchronize()
    assert torch.equal(z, z0), "the statistics epilogue must not change the stored values"
    _check_forward(pb, z)
    _check_partials(z, partials, rows, pb.cout)
    # the BatchNorm on top: with the epilogue's statistics and with its own pass (ZSV_AMP_NO_CONV_STATS), both against fp64
    for stats in (None, (partials, rows)):
        bn = _bn(pb.cout, pb.cout)
        bn0 = {k: v.clone() for k, v in bn.state_dict().items()}
        y, mean, invstd = amp.bn_cl_fwd_train(z, bn, None, True, conv_stats=stats)
        torch.cuda.synchronize()
        _check_bn_forward(z, pb.cout, bn0, bn, y, mean, invstd)


def _run_dgrad(pb):
    dz = pb.dz()
    dx_cl = amp.Bf16TrainPath._dgrad(pb.record(), amp.ncdhw_to_cl_bf16(dz))
    torch.cuda.synchronize()
    t, h, w = pb.x.shape[2:]
    assert tuple(dx_cl.shape[:4]) == (N, t, h, w)
    chans = _channels(pb.cin, 24, len(pb.name) + 1)
    ref = torch.nn.grad.conv3d_input((len(CLIPS), len(chans), t, h, w), pb.w[:, chans].double().cpu(),
                                     dz[list(CLIPS)].double().cpu(), pb.s, pb.p)
    got = _cl_sample(dx_cl, CLIPS, chans)
    assert float((got - ref).abs().max()) <= float(ref.abs().max()) * 2.0 ** -7, pb.name
    assert float(dx_cl[..., pb.cin:].float().abs().sum()) == 0.0, "pad channels must be zero"
    if pb.k == (1, 1, 1) and pb.s == (2, 2, 2):
        # the 1x1x1 stride-2 shortcut: 7 of 8 residue classes receive no tap -- exactly zero on every clip
        hit = torch.zeros((t, h, w), dtype=torch.bool, device=DEV)
        hit[::2, ::2, ::2] = True
        assert float(dx_cl[:, ~hit].float().abs().sum()) == 0.0


def _run_wgrad(pb):
    dz = pb.dz()
    dw = amp.Bf16TrainPath._wgrad(pb.record(), amp.ncdhw_to_cl_bf16(dz))
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    assert tuple(dw.shape) == tuple(pb.w.shape) and dw.dtype == torch.float32
    ci = _channels(pb.cin, 16, len(pb.name) + 2)
    co = _channels(pb.cout, 16, len(pb.name) + 3)
    ref = torch.nn.grad.conv3d_weight(pb.x[:, ci].double().cpu(), (len(co), len(ci)) + pb.k, dz[:, co].double().cpu(), pb.s, pb.p)
    got = dw[co][:, ci].double().cpu()
    assert float((got - ref).abs().max()) <= 1e-3 * float(ref.abs().max()), pb.name
    return dw


@pytest.mark.parametrize("name", list(GEOMS))
def test_forward_at_size(name):
    """``conv_bf16_stats`` (C3D: ``conv_bf16`` with bias + ReLU) on the whole 22-clip problem: the sampled outputs against fp64,
    the partials against the fp64 sums of the stored z, and the BatchNorm forward on top with and without them."""
    _run_forward(_Problem(name, bias=name.startswith("C")))


@pytest.mark.parametrize("name", [g[0] for g in R2P1D + C3D if g[1] > 4])
def test_input_gradient_at_size(name):
    _run_dgrad(_Problem(name, bias=name.startswith("C")))


@pytest.mark.parametrize("name", list(GEOMS))
def test_weight_gradient_at_size(name):
    """All five ``wgrad_cl_kernel`` modes at their slice counts of the benchmarked step, and the fp32 path of the folded stems;
    two runs agree bit for bit (the slices are summed in a fixed order)."""
    pb = _Problem(name, bias=name.startswith("C"))
    dw = _run_wgrad(pb)
    dw2 = amp.Bf16TrainPath._wgrad(pb.record(), amp.ncdhw_to_cl_bf16(pb.dz()))
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2)


# one geometry per ``wgrad_cl_kernel`` mode (0: S1, 1: T1, 2: S2, 3: T2, 4: P1) on exactly representable operands
GRID_WGRAD = ("S1", "T1", "S2", "T2", "P1")


def _grid(shape, seed):
    """Integers in {-2..2} drawn on the device (fp32 NCDHW); a zero on one of the six faces of a clip's (T, H, W) box becomes +-1,
    so a lost border voxel cannot hide behind a zero product."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randint(-2, 3, shape, generator=g, device=DEV).float()
    sign = torch.randint(0, 2, shape, generator=g, device=DEV).float() * 2 - 1
    face = torch.zeros(tuple(shape[2:]), dtype=torch.bool, device=DEV)
    face[[0, -1]] = True
    face[:, [0, -1]] = True
    face[:, :, [0, -1]] = True
    return torch.where(face & (x == 0), sign, x)


@pytest.mark.parametrize("name", GRID_WGRAD)
def test_weight_gradient_at_size_is_exact_on_grid_operands(name):
    """The lost voxel at size.  With N(0,1) operands one dropped or doubled voxel of the 1.1 M moves a weight gradient by 2.4e-4 of
    its range, under the 1e-3 bar of ``test_weight_gradient_at_size``.  With x, dz in {-2..2} the sum of |terms| of an output is at
    most 4 x 1 103 872 < 2^24: every partial sum of every slice, in every order, is an fp32 integer, so the fp32 result must EQUAL the
    float64 one (``tests/bf16_exact_cases.py`` has the argument) -- same channel sample, all 22 clips."""
    pb = _Problem(name)
    seed = sum(map(ord, name))
    pb.x = _grid(tuple(pb.x.shape), seed + 10)
    pb.xb = amp.ncdhw_to_cl_bf16(pb.x)
    dz = _grid((N, pb.cout) + pb.out, seed + 11)
    assert 4 * N * pb.out[0] * pb.out[1] * pb.out[2] < 2 ** 24
    dw = amp.Bf16TrainPath._wgrad(pb.record(), amp.ncdhw_to_cl_bf16(dz))
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    ci = _channels(pb.cin, 16, len(pb.name) + 2)
    co = _channels(pb.cout, 16, len(pb.name) + 3)
    ref = torch.nn.grad.conv3d_weight(pb.x[:, ci].double().cpu(), (len(co), len(ci)) + pb.k, dz[:, co].double().cpu(), pb.s, pb.p)
    got = dw[co][:, ci].double().cpu()
    bad = got != ref
    assert not bool(bad.any()), (name, int(bad.sum()), bad.nonzero()[:4].tolist(), got[bad][:4].tolist(), ref[bad][:4].tolist())


def _kernels_run(fn):
    """The device kernels ``fn`` launches (names without spaces), from a kernel trace."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key.replace(" ", "") for e in prof.key_averages()}


def _check_route(names, alt, default):
    assert any(alt in k for k in names), (alt, sorted(k[:60] for k in names if "conv_bf16" in k))
    assert not any(default in k for k in names), (default, "the switch did not change the route")


@pytest.mark.parametrize("name,knob,alt,default", ALT_FWD, ids=[f"{a}-{b}" for a, b, _, _ in ALT_FWD])
def test_forward_other_route_at_size(name, knob, alt, default, monkeypatch):
    monkeypatch.setenv(knob, "1")
    pb = _Problem(name)
    _check_route(_kernels_run(lambda: _run_forward(pb)), alt, default)


@pytest.mark.parametrize("name,knob,alt,default", ALT_DGRAD, ids=[f"{a}-{b}" for a, b, _, _ in ALT_DGRAD])
def test_input_gradient_other_route_at_size(name, knob, alt, default, monkeypatch):
    monkeypatch.setenv(knob, "1")
    pb = _Problem(name)
    _check_route(_kernels_run(lambda: _run_dgrad(pb)), alt, default)


def test_default_routes_of_the_switched_cases():
    """Without the switches the cases above reach the default kernels named in ALT_FWD / ALT_DGRAD (so the two routes differ)."""
    for name, _, _, default in ALT_FWD:
        pb = _Problem(name)
        blob = amp.pack_conv(pb.desc, pb.w, None, None)
        assert any(default in k for k in _kernels_run(lambda: amp.conv_bf16_stats(pb.desc, pb.xb, blob))), (name, default)
    for name, _, _, default in ALT_DGRAD:
        pb = _Problem(name)
        dz = amp.ncdhw_to_cl_bf16(pb.dz())
        assert any(default in k for k in _kernels_run(lambda: amp.Bf16TrainPath._dgrad(pb.record(), dz))), (name, default)


@pytest.mark.parametrize("name,knob", ALT_WGRAD, ids=[f"{a}-{b}" for a, b in ALT_WGRAD])
def test_weight_gradient_other_route_at_size(name, knob, monkeypatch):
    from ctypes import byref
    from zeroshotvideoclassification_amd import _lib
    pb = _Problem(name)
    monkeypatch.setenv(knob, "1")
    assert _lib.load().zsv_conv3d_bf16_wgrad_workspace_bytes(byref(pb.desc)) == 0       # the switch really takes the other route
    _run_wgrad(pb)


# channels, (T, H, W), relu, residual: the unit forms of the benchmarked step, the block tail (residual + ReLU) once per layer
BN_CASES = [
    ("stem_S0", 45, (16, 56, 56), True, False),
    ("layer1_S1", 144, (16, 56, 56), True, False),
    ("layer1_tail", 64, (16, 56, 56), True, True),
    ("layer2_P1", 128, (8, 28, 28), False, False),         # the shortcut's BatchNorm: no ReLU
    ("layer2_S3", 230, (8, 28, 28), True, False),
    ("layer2_tail", 128, (8, 28, 28), True, True),
    ("layer3_S6", 460, (4, 14, 14), True, False),
    ("layer3_tail", 256, (4, 14, 14), True, True),
    ("layer4_S9", 921, (2, 7, 7), True, False),
    ("layer4_tail", 512, (2, 7, 7), True, True),
]


@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batchnorm_at_size(case):
    """``bn_cl_fwd_train`` / ``bn_cl_bwd`` on the whole 22-clip tensor (up to 1.1 M rows) against fp64: the unit forms the step
    runs -- ReLU without a residual (the backward also with the forward's scale / shift rows, same bits), no ReLU (shortcut),
    and the block tail (residual + ReLU, the masked gradient ``g``)."""
    name, c, (t, h, w), relu, res = case
    seed = sum(map(ord, name))
    shape = (N, c, t, h, w)
    z = amp.ncdhw_to_cl_bf16(_randn(shape, seed, 1.5, 0.3))
    r = amp.ncdhw_to_cl_bf16(_randn(shape, seed + 1)) if res else None
    dy = amp.ncdhw_to_cl_bf16(_randn(shape, seed + 2))
    bn = _bn(c, seed)
    bn0 = {k: v.clone() for k, v in bn.state_dict().items()}
    y, mean, invstd, coef = amp.bn_cl_fwd_train(z, bn, r, relu, want_coef=True)
    torch.cuda.synchronize()
    _check_bn_forward(z, c, bn0, bn, y, mean, invstd, r, relu)
    zf = z[..., :c].double().reshape(-1, c)
    if relu:
        # the ReLU mask against the forward's scale / shift rows (checked above through y): z * a + b is exact in fp64 (a bf16 times
        # an fp32 value), so without a residual its sign is fma(z, a, b)'s -- the same mask bit for bit; with one, the fp32 sum may
        # differ in sign only within a few roundings of zero
        lin = zf * coef[0, :c].double() + coef[1, :c].double()
        mask = y[..., :c].reshape(-1, c) > 0
        if res:
            rf = r[..., :c].double().reshape(-1, c)
            pre = lin + rf
            clear = pre.abs() > 1e-6 * (lin.abs() + rf.abs())
            assert torch.equal(mask[clear], (pre > 0)[clear])
            del rf, pre, clear
        else:
            assert torch.equal(mask, lin > 0)
        del lin, mask
    dz, g, dgamma, dbeta = amp.bn_cl_bwd(dy, y, z, bn, mean, invstd, relu, want_g=res)
    torch.cuda.synchronize()
    # fp64 backward on the kernel's own mask (y > 0 on the ROUNDED output, pinned to the coefficients above: an fp64 mask of the
    # reference's own statistics flips within an ulp of zero)
    m64, v64 = zf.mean(0), zf.var(0, unbiased=False)
    inv64 = 1.0 / torch.sqrt(v64 + bn.eps)
    xhat = (zf - m64) * inv64
    gy = dy[..., :c].double().reshape(-1, c)
    if relu:
        gy = gy * (y[..., :c].reshape(-1, c) > 0).double()
    dbeta64, dgamma64 = gy.sum(0), (gy * xhat).sum(0)
    dz64 = (bn.weight.double() * inv64) * (gy - dbeta64 / zf.shape[0] - xhat * (dgamma64 / zf.shape[0]))
    del xhat, zf
    got = dz[..., :c].double().reshape(-1, c)
    assert float((got - dz64).abs().max()) <= float(dz64.abs().max()) * 2.0 ** -6
    assert float(dz[..., c:].float().abs().sum()) == 0.0
    assert float((dgamma.double() - dgamma64).abs().max()) <= 2e-3 * float(dgamma64.abs().max()) + 1e-6
    assert float((dbeta.double() - dbeta64).abs().max()) <= 2e-3 * float(dbeta64.abs().max()) + 1e-6
    if res:
        expect = dy.float() * (y.float() > 0) if relu else dy.float()
        assert torch.equal(g.float(), expect)
    if relu and not res:
        # the step's form of this unit: the mask recomputed from z with the forward's scale / shift rows -- the same bits
        dz2, _, dgamma2, dbeta2 = amp.bn_cl_bwd(dy, None, z, bn, mean, invstd, True, want_g=False, fwd_coef=coef)
        torch.cuda.synchronize()
        assert torch.equal(dz2, dz) and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)


# C3D's pools at full size: (channels, (T, H, W) of the pool's input, kernel, padding)  (network.py:138-149)
POOLS = [("pool1", 64, (16, 112, 112), (1, 2, 2), (0, 0, 0)), ("pool2", 128, (16, 56, 56), (2, 2, 2), (0, 0, 0)),
         ("pool3", 256, (8, 28, 28), (2, 2, 2), (0, 0, 0)), ("pool4", 512, (4, 14, 14), (2, 2, 2), (0, 0, 0)),
         ("pool5", 512, (2, 7, 7), (2, 2, 2), (0, 1, 1))]


@pytest.mark.parametrize("case", POOLS, ids=[c[0] for c in POOLS])
def test_c3d_pool_and_relu_bias_backward_at_size(case):
    """``maxpool3d_bf16`` / ``maxpool3d_bf16_bwd`` and ``relu_bias_bwd_cl`` on each pool's full-size input (the output of a
    relu(conv + bias): many exact zeros and repeated values): exact against torch on the same values (the gradient to the FIRST
    maximum of a window), the bias gradient against fp64 sums."""
    name, c, (t, h, w), k, p = case
    seed = sum(map(ord, name))
    y = torch.relu(_randn((N, c, t, h, w), seed))
    y_cl = amp.ncdhw_to_cl_bf16(y)
    pooled = inference.maxpool3d_bf16(y_cl, c, k, p)
    yr = y.clone().requires_grad_(True)
    ref = F.max_pool3d(yr, k, k, p)
    assert torch.equal(amp.cl_to_ncdhw_f32(pooled, c), ref.detach())
    assert float(pooled[..., c:].float().abs().sum()) == 0.0
    dp = _randn(tuple(ref.shape), seed + 1)
    ref.backward(dp)
    dy_cl = amp.maxpool3d_bf16_bwd(amp.ncdhw_to_cl_bf16(dp), y_cl, c, k, p)
    torch.cuda.synchronize()
    assert torch.equal(amp.cl_to_ncdhw_f32(dy_cl, c), yr.grad)
    assert float(dy_cl[..., c:].float().abs().sum()) == 0.0
    gg, db = amp.relu_bias_bwd_cl(dy_cl, y_cl, c)
    torch.cuda.synchronize()
    expect = yr.grad * (y > 0)
    assert torch.equal(amp.cl_to_ncdhw_f32(gg, c), expect)
    db64 = expect.double().sum(dim=(0, 2, 3, 4))
    assert float((db.double() - db64).abs().max()) <= 1e-5 * float(db64.abs().max()) + 1e-6


# ---- 2. the whole step at size against the CPU-autocast oracle and the fp32 path --------------------------------------------
# The oracle's draw is taken on the host in child processes that do not open the device (see _oracle_autocast).
_ORACLE_CHILD = r"""
import os, sys
root, net, n, train_mode, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1", sys.argv[5]
sys.path[:0] = [root, os.path.join(root, "tests")]
import torch
import torch.nn.functional as F
from helpers import make_opt
from zeroshotvideoclassification_amd import synthetic
from oracle import restatement as R
torch.set_num_threads(min(16, torch.get_num_threads()))
oracle = R.oracle_network(make_opt(net))
oracle.load_state_dict(synthetic.keyed_state_dict(oracle.state_dict(), seed=0, bn_jitter=net != "c3d"))
oracle.train(train_mode)
x = synthetic.synthetic_clips(n, 16, 112)
_, z = synthetic.synthetic_targets(n)
with torch.autocast("cpu", dtype=torch.bfloat16):
    y = R.embed(oracle, x)
    loss = F.mse_loss(y.float(), z)
loss.backward()
torch.save({"y": y.detach().float(), "loss": float(loss.item()),
            "grads": {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None},
            "buffers": {k: v for k, v in oracle.state_dict().items() if "running" in k or "num_batches" in k}}, out)
"""


def _oracle_autocast(net, n, train_mode, tmp_path):
    """The imported reference under torch.autocast("cpu", bfloat16) on the same weights and clips, each run in a child process.
    The host's bf16 weight gradient of the deepest convolutions (the 2-frame ones: R(2+1)D-18's layer4 temporal convolutions,
    C3D's conv5) has come back non-finite in some runs, and differs between two runs of the same inputs when finite, while
    everything else the reference computes is the same bits run to run.  So it runs twice: embeddings, loss and buffers must
    agree bit for bit, and a gradient that is not finite or not the same bits in both runs is no draw of the reference's
    rounding -- its name goes to ``ref["unsure"]`` (the callers bound how many there may be and check those parameters against
    the fp32 path only)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    draws = []
    for i in range(2):
        out = str(tmp_path / f"oracle_{net}_{n}_{i}.pt")
        subprocess.run([sys.executable, "-c", _ORACLE_CHILD, root, net, str(n), "1" if train_mode else "0", out], env=env,
                       check=True, timeout=600)
        draws.append(torch.load(out))
    ref, other = draws
    assert bool(torch.isfinite(ref["y"]).all())
    assert torch.equal(other["y"], ref["y"]) and other["loss"] == ref["loss"] and sorted(other["grads"]) == sorted(ref["grads"])
    for k in ref["buffers"]:
        assert torch.equal(other["buffers"][k], ref["buffers"][k]), k
    ref["unsure"] = {k for k, v in ref["grads"].items() if not (bool(torch.isfinite(v).all()) and torch.equal(v, other["grads"][k]))}
    return ref


def _model(net, jitter):
    model = network.get_network(make_opt(net))
    weights = synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=jitter)
    model.load_state_dict(weights)
    return model.to(DEV), weights


def _cos(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


def _step(model, weights, x, z, bf16):
    model.load_state_dict(weights)
    model.zero_grad(set_to_none=True)
    with amp.autocast(enabled=bf16):
        y = train.embed(model, x)
        loss = F.mse_loss(y, z)
    loss.backward()
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    bufs = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    return y.detach(), loss.detach(), grads, bufs


def test_r2plus1d_bf16_step_at_size_against_the_autocast_oracle_and_the_fp32_path(tmp_path):
    """R(2+1)D-18, train mode, 22 clips of 3x16x112x112 (extra.train_bf16's step): the amp.autocast() step against the imported
    reference under CPU autocast and the fp32 HIP step at the same size (which test_full_size_gradients_match_the_oracle_per_parameter
    pins to the fp32 oracle).  The bars of test_autocast_training_step_against_the_reference_under_cpu_autocast: embedding cosine
    >= 0.99 per row and 4e-2 absolute against both, loss within 3 % of both, the same live set, finite gradients; per parameter
    the shortfall of the cosine to the fp32 gradients against the oracle's own draw -- none more than 0.3, at most two more than
    0.2, the median within 0.08; norms within [0.7, 1.4] of fp32; BatchNorm running statistics after the step within 2e-2 / 5e-2
    of the oracle's."""
    model, weights = _model("r2plus1d_18", True)
    x = synthetic.synthetic_clips(N, 16, 112)
    _, z = synthetic.synthetic_targets(N)
    model.train()
    y32, loss32, g32, _ = _step(model, weights, x.to(DEV), z.to(DEV), False)
    y, loss, grads, bufs = _step(model, weights, x.to(DEV), z.to(DEV), True)
    assert y.dtype == torch.float32
    ref = _oracle_autocast("r2plus1d_18", N, True, tmp_path)
    for row in range(N):
        assert _cos(y[row], ref["y"][row]) >= 0.99, ("autocast oracle", row)
        assert _cos(y[row], y32[row]) >= 0.99, ("fp32 path", row)
    assert float((y.cpu() - ref["y"]).abs().max()) <= 4e-2
    assert float((y - y32).abs().max()) <= 4e-2
    assert abs(loss.item() / ref["loss"] - 1) <= 0.03
    assert abs(loss.item() / loss32.item() - 1) <= 0.03
    assert sorted(grads) == sorted(g32) == sorted(ref["grads"]) and len(grads) == 115
    for k, v in grads.items():
        assert v.dtype == torch.float32 and torch.isfinite(v).all(), k
    # (the oracle's unreproducible gradients: at most the four 2-frame temporal convolutions of layer4; norms below still apply)
    assert len(ref["unsure"]) <= 4 and all(k.startswith("model.layer4.") for k in ref["unsure"]), sorted(ref["unsure"])
    drawn = [k for k in grads if k not in ref["unsure"]]
    mine_cos = {k: _cos(grads[k], g32[k]) for k in drawn}
    oracle_cos = {k: _cos(ref["grads"][k], g32[k]) for k in drawn}
    short = sorted(((oracle_cos[k] - mine_cos[k], k) for k in drawn), reverse=True)
    assert short[0][0] <= 0.3, short[:3]
    assert sum(1 for v, _ in short if v > 0.2) <= 2, short[:5]
    assert np.median(list(mine_cos.values())) >= np.median(list(oracle_cos.values())) - 0.08
    for k in grads:
        ratio = float(grads[k].double().norm()) / float(g32[k].double().norm())
        assert 0.7 <= ratio <= 1.4, (k, ratio)
    rb = ref["buffers"]
    assert sorted(bufs) == sorted(rb)
    rm = torch.cat([bufs[k].flatten().cpu() for k in sorted(bufs) if k.endswith("running_mean")])
    rv = torch.cat([bufs[k].flatten().cpu() for k in sorted(bufs) if k.endswith("running_var")])
    rm_ref = torch.cat([rb[k].flatten() for k in sorted(rb) if k.endswith("running_mean")])
    rv_ref = torch.cat([rb[k].flatten() for k in sorted(rb) if k.endswith("running_var")])
    assert float((rm - rm_ref).abs().max()) <= 2e-2 * max(1.0, float(rm_ref.abs().max()))
    assert float((rv / rv_ref - 1).abs().max()) <= 5e-2
    for k in bufs:
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(rb[k]), k


def test_c3d_bf16_step_at_size_against_the_autocast_oracle_and_the_fp32_path(tmp_path):
    """C3D, eval mode (dropout off), 4 clips of 3x16x112x112: the bars of the one-clip test -- cosine >= 0.999 and 1e-2 absolute
    against the oracle under CPU autocast and the fp32 path, loss within 2 %, the same live set, finite gradients, each gradient's
    cosine to fp32 at most 0.05 below the oracle's own, norms within [0.85, 1.15] of fp32."""
    n = 4
    model, weights = _model("c3d", False)
    model.eval()
    x = synthetic.synthetic_clips(n, 16, 112)
    _, z = synthetic.synthetic_targets(n)
    y32, _, g32, _ = _step(model, weights, x.to(DEV), z.to(DEV), False)
    y, loss, grads, _ = _step(model, weights, x.to(DEV), z.to(DEV), True)
    ref = _oracle_autocast("c3d", n, False, tmp_path)
    for name, other in (("autocast oracle", ref["y"]), ("fp32 path", y32.cpu())):
        for row in range(n):
            assert _cos(y[row], other[row]) >= 0.999, (name, row)
        assert float((y.cpu() - other).abs().max()) <= 1e-2, name
    assert abs(loss.item() / ref["loss"] - 1) <= 0.02
    assert sorted(grads) == sorted(g32) == sorted(ref["grads"]) and len(grads) == 20
    # (the oracle's unreproducible gradients: at most conv5a / conv5b's weights, held to the fp32 path's cosine and norm only)
    assert ref["unsure"] <= {"conv5a.weight", "conv5b.weight"}, sorted(ref["unsure"])
    for k in grads:
        assert grads[k].dtype == torch.float32 and torch.isfinite(grads[k]).all(), k
        mine = _cos(grads[k], g32[k])
        theirs = 1.0 if k in ref["unsure"] else _cos(ref["grads"][k], g32[k])
        assert mine >= theirs - 0.05, (k, mine, theirs)
        ratio = float(grads[k].double().norm()) / float(g32[k].double().norm())
        assert 0.85 <= ratio <= 1.15, (k, ratio)


# ---- 3. reproducibility at size ------------------------------------------------------------------------------------------
def test_bf16_step_at_size_is_reproducible_eager_and_graphed():
    """Two eager amp.autocast() steps of R(2+1)D-18 at 22 clips from the same state give the same bits -- loss, every gradient,
    every BatchNorm buffer (the weight-gradient slices and the statistics partials are summed in a fixed order) -- and one
    amp.autocast(graph=True) step (the capture at the benchmarked allocation sizes) gives the same bits again."""
    model, weights = _model("r2plus1d_18", True)
    x = synthetic.synthetic_clips(N, 16, 112).to(DEV)
    _, z = synthetic.synthetic_targets(N)
    z = z.to(DEV)
    model.train()
    crit = torch.nn.MSELoss()

    def run(graph):
        model.load_state_dict(weights)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        _, loss = train.train_step(model, opt, crit, x, z, autocast=True, graph=graph)
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        bufs = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
        return loss.clone(), grads, bufs

    runs = [run(False), run(False), run(True)]
    la, ga, ba = runs[0]
    assert len(ga) == 115 and len(ba) > 0
    assert bool(torch.isfinite(la)) and all(bool(torch.isfinite(v).all()) for v in ga.values())
    for lb, gb, bb in runs[1:]:
        assert torch.equal(la, lb)
        assert sorted(ga) == sorted(gb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
        for k in ba:
            assert torch.equal(ba[k], bb[k]), k
    assert "_graphs" in amp.train_path_for(model.model).__dict__
