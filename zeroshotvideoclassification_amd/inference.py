"""bf16 evaluation engine: the reference's eval loop body (main.py:224-252, BASELINE config 5)
with the VideoResNet trunk run in bf16 on ``zsv_conv3d_bf16_fwd``; ``Fp8Engine`` is the same walk in
OCP e4m3 (``float8_e4m3fn``) on ``zsv_conv3d_fp8_fwd``.  ``Bf16EngineC3D`` / ``Fp8EngineC3D`` are the
same pair for ``network.C3D``, the e4m3 one with calibrated activation scales (``calibrate_fp8``).

``Bf16Engine(model)`` walks a ``network.Model`` whose trunk is a ``resnet.VideoResNet``
(R(2+1)D-18 / R3D-18 / MC3-18), folds every eval-mode ``BatchNorm3d`` into the convolution in
front of it (scale into the weights, shift into the epilogue -- resnet.py:40-52,94-98), fuses
ReLU and the block's ``out += residual; relu`` (resnet.py:110-111) into the same epilogue, and
packs the weights once.  Calling it has ``Model.forward``'s contract (network.py:533-600):
``(bs, nc, 3, T, H, W) fp32 -> (emb (bs*nc, 300) fp32 unit-norm, None)``.  Activations are
channels-last bf16 between layers; the 512-d pooled feature, the MLP head and the normalisation
stay fp32 on the training path's kernels.

The engine holds a snapshot of the weights: build it after loading / training, rebuild after the
weights change.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from ctypes import byref
from functools import lru_cache, partial
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from ._lib import ConvDesc


class _Format:
    """One element format of the channels-last engines: the tensor dtype, the C entry points and the public functions' names in
    messages (all formed here, once), and the format a clip convolution (Cin <= 4) reads -- an e4m3 clip convolution takes the
    bf16 output of ``clip_to_bf16``."""

    def __init__(self, name: str, dtype: torch.dtype, label: str, clip: Optional["_Format"] = None):
        self.name, self.dtype, self.label, self.clip = name, dtype, label, clip or self
        self.conv_name, self.meanpool_name = f"conv_{name}", f"meanpool_{name}"
        self.pitch, self.meanpool = f"zsv_{name}_channel_pitch", f"zsv_meanpool_{name}"
        self.maxpool_name, self.maxpool = f"maxpool3d_{name}", f"zsv_maxpool3d_{name}"
        self.blob_bytes, self.pack, self.fwd = (f"zsv_conv3d_{name}_{f}" for f in ("blob_bytes", "pack", "fwd"))


FP8 = torch.float8_e4m3fn
BF16 = _Format("bf16", torch.bfloat16, "bf16")
E4M3 = _Format("fp8", FP8, "float8_e4m3fn", clip=BF16)


def _check(t: torch.Tensor, fmt: _Format, op: str, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{op} {what}: MI355X HIP tensor expected, got {t.device} (there is no CPU fallback)")
    if t.dtype != fmt.dtype or not t.is_contiguous():
        raise RuntimeError(f"{op} {what}: contiguous {fmt.label} tensor expected")


@lru_cache(maxsize=None)                   # (a pure function of its arguments, asked twice per convolution launch)
def _pitch(fmt: _Format, channels: int) -> int:
    return int(getattr(_lib.load(), fmt.pitch)(int(channels)))


def clip_to_bf16(x: torch.Tensor, pad_h: int, pad_w: int, hp: int, wp: int) -> torch.Tensor:
    """(N, 3, T, H, W) fp32 -> [N][T][hp][wp][4] bf16 with the frame at (pad_h, pad_w) in a zero border."""
    ops._require(x)
    x = x.contiguous()
    n, c, t, h, w = x.shape
    out = torch.empty((n, t, hp, wp, 4), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().zsv_clip_to_bf16(x.data_ptr(), n, c, t, h, w, pad_h, pad_w, hp, wp, out.data_ptr(),
                                            ops._stream()), "zsv_clip_to_bf16")
    return out


def _pack(fmt: _Format, d: ConvDesc, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor]) -> torch.Tensor:
    """Packed weights (x scale per produced channel) + fp32 shifts for ``_conv``; e4m3: quantised per produced channel (bf16 for
    a clip convolution), with the fp32 dequantisation factors behind the shifts."""
    ops._require(weight, scale, shift)
    lib = _lib.load()
    nbytes = getattr(lib, fmt.blob_bytes)(byref(d))
    if nbytes == 0:
        raise RuntimeError(f"{fmt.blob_bytes}: unsupported convolution geometry")
    blob = torch.empty(int(nbytes), dtype=torch.uint8, device=weight.device)
    _lib.check(getattr(lib, fmt.pack)(byref(d), weight.contiguous().data_ptr(), ops._ptr(scale), ops._ptr(shift), blob.data_ptr(),
                                      ops._stream()), fmt.pack)
    return blob


def _conv(fmt: _Format, d: ConvDesc, x: torch.Tensor, blob: torch.Tensor, residual: Optional[torch.Tensor] = None,
          relu: bool = False) -> torch.Tensor:
    """y[N][To][Ho][Wo][Cp] = relu?(conv(x) * scale + shift (+ residual)) in ``fmt`` (e4m3: saturating)."""
    what = fmt.conv_name
    if fmt.clip is not fmt and d.Cin <= 4:
        _check(x, fmt.clip, what, "clip input")
    else:
        _check(x, fmt, what, "input")
    expect = (d.N, d.Ti, d.Hi, d.Wi, _pitch(fmt, d.Cin))
    if tuple(x.shape) != expect:
        raise RuntimeError(f"{what}: input {tuple(x.shape)} does not match the descriptor {expect}")
    y = torch.empty((d.N, d.To, d.Ho, d.Wo, _pitch(fmt, d.Cout)), dtype=fmt.dtype, device=x.device)
    if residual is not None:
        _check(residual, fmt, what, "residual")
        if residual.shape != y.shape:
            raise RuntimeError(f"{what}: residual {tuple(residual.shape)} != output {tuple(y.shape)}")
    _lib.check(getattr(_lib.load(), fmt.fwd)(byref(d), x.data_ptr(), blob.data_ptr(), ops._ptr(residual), 1 if relu else 0,
                                             y.data_ptr(), ops._stream()), fmt.fwd)
    return y


def _meanpool(fmt: _Format, x: torch.Tensor, channels: int) -> torch.Tensor:
    """[N][T][H][W][Cp] -> (N, channels) fp32 mean over the voxels."""
    _check(x, fmt, fmt.meanpool_name, "input")
    n = x.shape[0]
    s = x.shape[1] * x.shape[2] * x.shape[3]
    out = torch.empty((n, channels), dtype=torch.float32, device=x.device)
    _lib.check(getattr(_lib.load(), fmt.meanpool)(x.data_ptr(), n, s, channels, out.data_ptr(), ops._stream()), fmt.meanpool)
    return out


# the public per-format names: (d, weight, scale, shift) / (d, x, blob, residual=None, relu=False) / (x, channels) / (channels)
pack_conv, conv_bf16, meanpool_bf16, channel_pitch = (partial(f, BF16) for f in (_pack, _conv, _meanpool, _pitch))
pack_conv_fp8, conv_fp8, meanpool_fp8, fp8_channel_pitch = (partial(f, E4M3) for f in (_pack, _conv, _meanpool, _pitch))


def _maxpool3d(fmt: _Format, x: torch.Tensor, channels: int, kernel, padding) -> torch.Tensor:
    """nn.MaxPool3d(kernel, stride = kernel, padding) on [N][T][H][W][Cp] in ``fmt`` (network.py:148-163)."""
    _check(x, fmt, fmt.maxpool_name, "input")
    n, t, h, w, cp = x.shape
    kt, kh, kw = (int(v) for v in kernel)
    pt, ph, pw = (int(v) for v in padding)
    to, ho, wo = (t + 2 * pt - kt) // kt + 1, (h + 2 * ph - kh) // kh + 1, (w + 2 * pw - kw) // kw + 1
    y = torch.empty((n, to, ho, wo, cp), dtype=fmt.dtype, device=x.device)
    _lib.check(getattr(_lib.load(), fmt.maxpool)(x.data_ptr(), n, channels, t, h, w, kt, kh, kw, pt, ph, pw, to, ho, wo, y.data_ptr(),
                                                 ops._stream()), fmt.maxpool)
    return y


maxpool3d_bf16, maxpool3d_fp8 = partial(_maxpool3d, BF16), partial(_maxpool3d, E4M3)      # (x, channels, kernel, padding)


def absmax_bf16(x: torch.Tensor, amax: torch.Tensor) -> None:
    """``amax[0] = max(amax[0], max |x|)`` over a contiguous bf16 tensor, on the device: one read, no host synchronisation.
    ``amax`` is one fp32 element >= 0 on the same device (a slot of a larger tensor will do); calls fold."""
    _check(x, BF16, "absmax_bf16", "input")
    if not amax.is_cuda or amax.dtype != torch.float32 or amax.numel() != 1:
        raise RuntimeError("absmax_bf16 amax: one fp32 element on the MI355X HIP device expected")
    _lib.check(_lib.load().zsv_absmax_bf16(x.data_ptr(), x.numel(), amax.data_ptr(), ops._stream()), "zsv_absmax_bf16")


def fold_bn(bn: Optional[nn.BatchNorm3d], conv: nn.Conv3d) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(scale, shift) of ``bn.eval()(conv(x))``: gamma/sqrt(var+eps), beta - mean*scale (+ conv bias)."""
    bias = conv.bias.detach().float() if conv.bias is not None else None
    if bn is None:
        return None, bias
    inv = torch.rsqrt(bn.running_var.detach().double() + bn.eps)
    gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(inv)
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(inv)
    scale = gamma * inv
    shift = beta - bn.running_mean.detach().double() * scale
    if bias is not None:
        shift = shift + bias.double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


class ConvGeometry:
    """The extents of one ``nn.Conv3d`` and what follows from them: the kernel descriptor for a stored input, and for the clip
    convolution (``folded``) the materialised border."""

    who = "inference"                          # the prefix of this class's error messages

    def __init__(self, conv: nn.Conv3d):
        if tuple(conv.dilation) != (1, 1, 1) or conv.groups != 1:
            raise RuntimeError(f"{self.who}: dilation / groups are not used by the reference and not supported")
        self.cout, self.cin = conv.weight.shape[0], conv.weight.shape[1]
        self.kernel = tuple(conv.weight.shape[2:])
        self.stride, self.padding = tuple(conv.stride), tuple(conv.padding)
        self.folded = self.cin <= 4            # the clip itself: border materialised, kw folded into K (conv_bf16.hip)

    def desc(self, n: int, t: int, h: int, w: int, folded_wo: Optional[int] = None) -> ConvDesc:
        """``h, w``: stored extents of the input (with the materialised border for the clip convolution, whose output width
        ``folded_wo`` then comes from ``clip_input``)."""
        kt, kh, kw = self.kernel
        pt, ph, pw = self.padding
        if self.folded:
            ph = pw = 0
        st, sh, sw = self.stride
        to = (t + 2 * pt - kt) // st + 1
        ho = (h + 2 * ph - kh) // sh + 1
        wo = (w + 2 * pw - kw) // sw + 1 if folded_wo is None else folded_wo
        return ConvDesc(n, self.cin, t, h, w, self.cout, to, ho, wo, kt, kh, kw, st, sh, sw, pt, ph, pw)

    def _clip_wo(self, w: int) -> int:
        return (w + 2 * self.padding[2] - self.kernel[2]) // self.stride[2] + 1

    def input_border(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """(pad_h, pad_w, Hp, Wp) of the materialised border for the clip convolution."""
        ph, pw = self.padding[1], self.padding[2]
        return ph, pw, h + 2 * ph, max(w + 2 * pw, (self._clip_wo(w) - 1) * self.stride[2] + 8)

    def clip_input(self, clips: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """(N, 3, T, H, W) fp32 -> (the clip in bf16 inside its border, the ``folded_wo`` of this convolution on it)."""
        h, w = clips.shape[3:]
        return clip_to_bf16(clips, *self.input_border(h, w)), self._clip_wo(w)


class _ConvOp(ConvGeometry):
    """One folded convolution: geometry is resolved per input shape, the packed blob per layer."""

    def __init__(self, conv: nn.Conv3d, bn: Optional[nn.BatchNorm3d], relu: bool, fmt: _Format = BF16):
        super().__init__(conv)
        self.weight = conv.weight.detach().float().contiguous()
        self.scale, self.shift = fold_bn(bn, conv)
        self.relu, self.fmt = relu, fmt
        self._blob = None

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, wo: Optional[int] = None) -> torch.Tensor:
        n, t, h, w, _ = x.shape
        d = self.desc(n, t, h, w, wo)
        if self._blob is None:
            self._blob = _pack(self.fmt, d, self.weight, self.scale, self.shift)
        return _conv(self.fmt, d, x, self._blob, residual, self.relu)


def conv_bn_relu_chain(mods, who: str) -> List[Tuple[nn.Conv3d, Optional[nn.BatchNorm3d], bool]]:
    """[Conv3d, BN?, ReLU?, Conv3d, ...] (nested Sequentials flattened) -> (conv, bn or None, relu) triples."""
    flat: List[nn.Module] = []

    def walk(m):
        if isinstance(m, nn.Conv3d) or not isinstance(m, nn.Sequential):
            flat.append(m)
        else:
            for c in m:
                walk(c)
    for m in mods:
        walk(m)
    out = []
    i = 0
    while i < len(flat):
        conv = flat[i]
        if not isinstance(conv, nn.Conv3d):
            raise RuntimeError(f"{who}: expected a Conv3d, found {type(conv).__name__}")
        i += 1
        bn = None
        if i < len(flat) and isinstance(flat[i], nn.BatchNorm3d):
            bn = flat[i]
            i += 1
        relu = False
        if i < len(flat) and isinstance(flat[i], nn.ReLU):
            relu = True
            i += 1
        out.append((conv, bn, relu))
    return out


def video_resnet_ops(trunk: nn.Module, make, who: str):
    """``stem, [(conv1, conv2, down or None)]``: a ``resnet.VideoResNet`` of BasicBlocks as lists of ``make(conv, bn, relu)``
    objects (which carry a writable ``.relu``), in the order ``run_blocks`` executes them."""
    from . import resnet

    def chain(mods):
        return [make(*triple) for triple in conv_bn_relu_chain(mods, who)]
    if conv_bn_relu_chain(trunk.stem, who)[0][0].weight.shape[1] > 4:
        raise RuntimeError(f"{who}: the stem's first convolution must take the clip (<= 4 channels)")
    stem, blocks = chain(trunk.stem), []
    for layer in (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4):
        for block in layer:
            if not isinstance(block, resnet.BasicBlock):
                raise RuntimeError(f"{who}: only BasicBlock trunks (the reference's *_18 models) are supported")
            conv1, conv2 = chain(block.conv1), chain(block.conv2)
            conv2[-1].relu = True                   # out += residual; relu (resnet.py:110-111)
            blocks.append((conv1, conv2, chain(block.downsample) if block.downsample is not None else None))
    return stem, blocks


def run_blocks(x, blocks, call):
    """The residual blocks of ``video_resnet_ops`` on ``x``; ``call(op, x, residual or None)`` runs one of their objects."""
    for conv1, conv2, down in blocks:
        residual = x
        for op in down or ():
            residual = call(op, residual, None)
        y = x
        for op in conv1:
            y = call(op, y, None)
        for op in conv2[:-1]:
            y = call(op, y, None)
        x = call(conv2[-1], y, residual)
    return x


def c3d_layers(model: nn.Module, who: str):
    """``network.C3D``'s eight ``relu(conv(x) + bias)`` layers in order (network.py:147-163): (conv, (kernel, padding) of the
    max-pool behind it or None)."""
    if model.conv1.weight.shape[1] > 4:
        raise RuntimeError(f"{who}: conv1 must take the clip (<= 4 channels)")
    for conv, pool in (("conv1", "pool1"), ("conv2", "pool2"), ("conv3a", None), ("conv3b", "pool3"), ("conv4a", None),
                       ("conv4b", "pool4"), ("conv5a", None), ("conv5b", "pool5")):
        if pool is not None:
            pool = getattr(model, pool)
            k, pd = ops._triple(pool.kernel_size), ops._triple(pool.padding)
            if pool.stride is not None and ops._triple(pool.stride) != k:
                raise RuntimeError(f"{who}: max-pools with stride != kernel are not used by the reference")
            pool = (k, pd)
        yield getattr(model, conv), pool


def _device_model(model: nn.Module, who: str, c3d: bool = False) -> nn.Module:
    """The unwrapped model of an engine, after the two refusals that need no trunk walk (in this order)."""
    from . import network, resnet
    model = getattr(model, "module", model)
    if c3d and not isinstance(model, network.C3D):
        raise RuntimeError(f"{who} supports network.C3D")
    if not c3d and not (isinstance(model, network.Model) and isinstance(model.model, resnet.VideoResNet)):
        raise RuntimeError(f"{who} supports network.Model over a resnet.VideoResNet trunk")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError(f"{who}: the model must live on the MI355X HIP device (there is no CPU fallback)")
    return model


def _call_op(op, x, residual):
    return op(x, residual=residual)


class Bf16Engine:
    """Eval-mode ``Model.forward`` (network.py:533-600) in bf16.  See the module docstring."""

    _fmt = BF16

    def __init__(self, model: nn.Module):
        who = type(self).__name__
        self.model = _device_model(model, who)
        self.stem, self.blocks = video_resnet_ops(self.model.model, partial(_ConvOp, fmt=self._fmt), who)
        self.features = self.blocks[-1][1][-1].cout

    @torch.no_grad()
    def trunk(self, clips: torch.Tensor) -> torch.Tensor:
        """(N, 3, T, H, W) fp32 -> pooled (N, 512) fp32 (VideoResNet.forward's first output)."""
        x, wo = self.stem[0].clip_input(clips)
        x = self.stem[0](x, wo=wo)
        for op in self.stem[1:]:
            x = op(x)
        return _meanpool(self._fmt, run_blocks(x, self.blocks, _call_op), self.features)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor):
        bs, nc = x.shape[:2]
        clips = x.reshape(bs * nc, *x.shape[2:])                    # network.py:534-535
        pooled = self.trunk(clips)
        emb = self.model.output2emb_proj(pooled)                       # network.py:595 (mean already taken)
        return F.normalize(emb, dim=-1), None                          # network.py:596,600


class Fp8Engine(Bf16Engine):
    """Eval-mode ``Model.forward`` (network.py:533-600) in OCP e4m3: ``Bf16Engine``'s walk, structure checks and
    contract, with every convolution after the clip's on ``zsv_conv3d_fp8_fwd`` (e4m3 x e4m3, fp32 accumulation, weights
    quantised per produced channel, activations unscaled and saturating at +-448).  The clip convolution keeps bf16 operands
    (``zsv_clip_to_bf16``, the folded clip form) and writes e4m3; the mean pool reads e4m3 and writes the fp32 (N, 512) feature;
    the head and the normalisation stay fp32.  A clip's embedding does not depend on the other clips of its batch."""

    _fmt = E4M3


class Bf16EngineC3D:
    """Eval-mode ``network.C3D.forward`` (network.py:147-179) with the eight convolutions and five max-pools in bf16 on the
    channels-last layout: ``relu(conv(x) + bias)`` is one ``zsv_conv3d_bf16_fwd`` launch per layer (bias as the epilogue's
    shift), the pools are ``zsv_maxpool3d_bf16``; fc6 (+ ReLU), the clip mean, the regressor and the normalisation stay fp32
    (dropout is the identity in eval mode).  Same contract as the module: ``(bs, nc, 3, T, H, W) fp32 -> (bs, 300)``."""

    _fmt = BF16

    def __init__(self, model: nn.Module):
        who = type(self).__name__
        self.model = _device_model(model, who, c3d=True)
        # network.py:147-162: relu(conv(x)), bias in the epilogue
        self.ops = [(_ConvOp(conv, None, True, self._fmt), pool) for conv, pool in c3d_layers(self.model, who)]

    def _walk(self, clips: torch.Tensor, visit=None) -> torch.Tensor:
        """The eight layers and five pools on (N, 3, T, H, W) fp32 clips; ``visit(l, y)`` sees layer l's output before its pool."""
        x, wo = self.ops[0][0].clip_input(clips)
        for l, (op, pool) in enumerate(self.ops):
            x = op(x, wo=wo)
            wo = None
            if visit is not None:
                visit(l, x)
            if pool is not None:
                x = _maxpool3d(self._fmt, x, op.cout, pool[0], pool[1])
        return x

    def _values(self, x: torch.Tensor) -> torch.Tensor:
        return x.float()

    @torch.no_grad()
    def features(self, clips: torch.Tensor, taps: Optional[list] = None) -> torch.Tensor:
        """(N, 3, T, H, W) fp32 -> (N, 8192) fp32 in the (C, T, H, W) order of ``view(-1, 8192)`` (network.py:165).  With a list
        as ``taps`` every layer's output before its pool (channels-last, in the engine's format) is appended to it."""
        x = self._walk(clips, None if taps is None else (lambda l, y: taps.append(y)))
        c = self.ops[-1][0].cout
        if x.dtype == FP8:
            x = x.view(torch.uint8)                 # the codes as bytes: decoded by ``_values`` behind the strided copy
        return self._values(x[..., :c].permute(0, 4, 1, 2, 3).reshape(clips.shape[0], -1))

    @torch.no_grad()
    def __call__(self, x: torch.Tensor):
        m = self.model
        bs, nc = x.shape[:2]
        a = self.features(x.reshape(bs * nc, *x.shape[2:]))
        if a.shape[1] != m.fc6.in_features:
            raise RuntimeError(f"C3D: {a.shape[1]} features reach fc6, {m.fc6.in_features} expected (16x112x112 clips)")
        a = m.fc6(a.contiguous(), relu=True)                           # network.py:166 (dropout: identity in eval mode)
        a = a.reshape(bs, nc, -1).mean(1).reshape(bs, -1)              # network.py:174-176
        return F.normalize(m.regressor(a), dim=-1)                     # network.py:178-179


# ---- network.C3D in e4m3: one static power-of-two activation scale per layer -------------------------------
_NO_FP8_SCALES = ("C3D has no fp8 (float8_e4m3fn) engine until its eight activation scales are known (it has no BatchNorm to bound "
                  "its activations): call inference.calibrate_fp8(model, clips) first, or inference.set_fp8_scales(model, scales) "
                  "with scales kept from an earlier calibration")
_SCALES_ATTR = "_zsv_fp8_scales"


def fp8_scale(amax: float, headroom: float = 4.0) -> float:
    """The power-of-two scale a layer whose largest calibrated |activation| is ``amax`` is stored with:
    ``2 ** ceil(log2(amax * headroom / 448))``, so the stored ``amax / scale`` is at most ``448 / headroom`` (112 by default:
    two binades below saturation, thirteen normal binades below that).  ``amax == 0`` gives 1."""
    amax, headroom = float(amax), float(headroom)
    if not math.isfinite(amax) or amax < 0.0:
        raise ValueError(f"fp8_scale: amax must be finite and >= 0, got {amax}")
    if not math.isfinite(headroom) or headroom <= 0.0:
        raise ValueError(f"fp8_scale: headroom must be finite and > 0, got {headroom}")
    v = amax * headroom / 448.0
    if v == 0.0:
        return 1.0
    m, e = math.frexp(v)                        # v = m * 2**e with 0.5 <= m < 1: ceil(log2(v)) without a rounded logarithm
    return math.ldexp(1.0, e - 1 if m == 0.5 else e)


def _c3d(model: nn.Module, who: str) -> nn.Module:
    from . import network
    model = getattr(model, "module", model)
    if not isinstance(model, network.C3D):
        raise RuntimeError(f"{who} supports network.C3D")
    return model


def _checked_scales(scales) -> Tuple[float, ...]:
    try:
        out = tuple(float(v) for v in scales)
    except TypeError:
        raise ValueError(f"fp8 scales: eight finite positive numbers expected, got {scales!r}") from None
    if len(out) != 8 or not all(math.isfinite(v) and v > 0.0 for v in out):
        raise ValueError(f"fp8 scales: eight finite positive numbers expected, got {out}")
    return out


def set_fp8_scales(model: nn.Module, scales) -> None:
    """Keep the eight activation scales of ``calibrate_fp8`` on the (unwrapped) ``network.C3D``: in its ``__dict__``, not in its
    ``state_dict`` -- the reference's checkpoint format stays as it is; carry them next to a checkpoint (INTEGRATION)."""
    _c3d(model, "set_fp8_scales").__dict__[_SCALES_ATTR] = _checked_scales(scales)


def fp8_scales(model: nn.Module) -> Optional[Tuple[float, ...]]:
    """The stored activation scales of a ``network.C3D``, or None before ``calibrate_fp8`` / ``set_fp8_scales``."""
    return _c3d(model, "fp8_scales").__dict__.get(_SCALES_ATTR)


@torch.no_grad()
def calibrate_fp8(model: nn.Module, clips, headroom: float = 4.0) -> Tuple[float, ...]:
    """Take the eight activation scales of ``Fp8EngineC3D`` from calibration clips -- ``(N, 3, T, H, W)``,
    ``(bs, nc, 3, T, H, W)`` or an iterable of such -- store them on the model (``set_fp8_scales``) and return them.  The clips
    run through the bf16 engine's operators; each ``relu(conv + bias)`` output is read once more by ``zsv_absmax_bf16`` into its
    slot of one 8-float device tensor, which the host reads once at the end.  Several batches give the element-wise maximum
    of their separate calibrations."""
    own = _device_model(model, "calibrate_fp8", c3d=True)
    if own.training:
        raise RuntimeError("calibrate_fp8: the model must be in eval mode")
    engine = engine_for(own, torch.bfloat16)
    device = next(own.parameters()).device
    amax = torch.zeros(8, dtype=torch.float32, device=device)
    for batch in ([clips] if isinstance(clips, torch.Tensor) else clips):
        if batch.dim() == 6:
            batch = batch.reshape(-1, *batch.shape[2:])
        engine._walk(batch.to(device, torch.float32), lambda l, y: absmax_bf16(y, amax[l:l + 1]))
    scales = tuple(fp8_scale(v, headroom) for v in amax.tolist())          # (the one host read)
    set_fp8_scales(own, scales)
    return scales


@lru_cache(maxsize=None)
def _e4m3_values(device: torch.device) -> torch.Tensor:
    return torch.arange(256, dtype=torch.uint8).view(FP8).float().to(device)


class Fp8EngineC3D(Bf16EngineC3D):
    """Eval-mode ``network.C3D.forward`` (network.py:147-179) in OCP e4m3: ``Bf16EngineC3D``'s walk and contract with
    layer l's activation stored as ``true / scales[l]``, one static power of two per layer (``calibrate_fp8``; default: the scales
    stored on the model).  The convolution kernels are ``Fp8Engine``'s, unchanged: layer l is packed with
    ``scale = scales[l-1] / scales[l]`` (1 in front of the clip) and ``shift = bias / scales[l]``, and ReLU and the max-pool
    (``zsv_maxpool3d_fp8``) commute with a positive factor.  The clip convolution keeps bf16 operands and writes e4m3; the
    (N, 8192) feature is dequantised by ``scales[-1]``; fc6 and everything behind it stay fp32.  Static scales: a clip's
    embedding does not depend on the other clips of its batch."""

    _fmt = E4M3

    def __init__(self, model: nn.Module, scales=None):
        scales = fp8_scales(model) if scales is None else _checked_scales(scales)
        if scales is None:
            raise RuntimeError(_NO_FP8_SCALES)
        super().__init__(model)
        self.scales = scales
        before = 1.0
        for (op, _), a in zip(self.ops, scales):
            op.scale = torch.full((op.cout,), before / a, dtype=torch.float32, device=op.weight.device)
            if op.shift is not None:
                op.shift = (op.shift / a).contiguous()
            before = a

    def _values(self, x: torch.Tensor) -> torch.Tensor:
        return _e4m3_values(x.device)[x.long()] * self.scales[-1]


class _ConvOpF32:
    """One folded fp32 convolution: w * scale and shift are formed once; ReLU and the block's residual add
    run in the convolution's epilogue (``zsv_conv3d_fwd_add``)."""

    def __init__(self, conv: nn.Conv3d, bn: Optional[nn.BatchNorm3d], relu: bool):
        scale, shift = fold_bn(bn, conv)
        w = conv.weight.detach().float()
        self.weight = (w * scale.view(-1, 1, 1, 1, 1)).contiguous() if scale is not None else w.contiguous()
        self.bias = shift
        self.stride, self.padding, self.relu = tuple(conv.stride), tuple(conv.padding), relu
        self.cout = self.weight.shape[0]

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        d = ops.conv_desc(x.shape, self.weight.shape, self.stride, self.padding)
        lib = _lib.load()
        y = torch.empty((d.N, d.Cout, d.To, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
        nbytes = lib.zsv_conv3d_fwd_workspace_bytes(byref(d))
        ws = ops._workspace(nbytes, x.device)
        fused = residual is None or bool(lib.zsv_conv3d_fwd_add_supported(byref(d)))
        _lib.check(lib.zsv_conv3d_fwd_add(byref(d), x.data_ptr(), self.weight.data_ptr(), ops._ptr(self.bias),
                                          ops._ptr(residual if fused else None), y.data_ptr(),
                                          1 if (self.relu and fused) else 0, ops._ptr(ws), nbytes, ops._stream()),
                   "zsv_conv3d_fwd_add")
        if not fused:                                   # split-K geometry: separate add (+ ReLU)
            y = ops.add_relu(y, residual) if self.relu else y + residual
        return y


class Fp32Engine:
    """Eval-mode ``Model.forward`` in fp32 with every BatchNorm folded into its convolution:
    same contract and structure as ``Bf16Engine``, fp32 NCDHW activations, no BatchNorm kernels."""

    def __init__(self, model: nn.Module):
        self.model = _device_model(model, "Fp32Engine")
        self.stem, self.blocks = video_resnet_ops(self.model.model, _ConvOpF32, "Fp32Engine")

    @torch.no_grad()
    def trunk(self, clips: torch.Tensor) -> torch.Tensor:
        ops._require(clips)
        x = clips.contiguous()
        for op in self.stem:
            x = op(x)
        return ops.mean_pool(run_blocks(x, self.blocks, _call_op))

    @torch.no_grad()
    def __call__(self, x: torch.Tensor):
        bs, nc = x.shape[:2]
        pooled = self.trunk(x.reshape(bs * nc, *x.shape[2:]))
        return F.normalize(self.model.output2emb_proj(pooled), dim=-1), None


def engine_for(model: nn.Module, dtype: torch.dtype = torch.bfloat16, rebuild: bool = False):
    """The model's inference engine for ``dtype`` (bf16: ``Bf16Engine``, fp32: ``Fp32Engine``, ``torch.float8_e4m3fn``:
    ``Fp8Engine``, or ``Fp8EngineC3D`` for a ``network.C3D`` with stored activation scales -- ``calibrate_fp8``; the scales are
    part of what the cached engine is keyed on), rebuilt only when a
    trunk parameter or BatchNorm buffer may have been written since it was built, e.g. once per epoch for the
    three test sets of main.py:352-358.  "Written" = the tensors' identity / version counters (torch-side
    writes) AND ``_lib.raw_write_generation()``: the HIP BatchNorm running-statistics update, ``FusedAdam``,
    ``load_weights`` and ``GradientSync.broadcast_state`` write through raw pointers or ``.data`` and announce
    it there.  ``rebuild=True`` forces a rebuild (for writers this package does not know about)."""
    own = getattr(model, "module", model)
    from . import network
    is_c3d = isinstance(own, network.C3D)
    trunk = own if is_c3d else own.model
    tensors = list(trunk.parameters()) + list(trunk.buffers())
    key = (_lib.raw_write_generation(),) + tuple((id(t), t.data_ptr(), t._version) for t in tensors)
    if dtype == FP8 and is_c3d:
        scales = fp8_scales(own)
        if scales is None:
            raise RuntimeError(_NO_FP8_SCALES)
        key += (scales,)
    cache = own.__dict__.setdefault("_zsv_engines", {})
    cached = None if rebuild else cache.get(dtype)
    if cached is None or cached[0] != key:
        if dtype == torch.bfloat16:
            engine = Bf16EngineC3D(own) if is_c3d else Bf16Engine(own)
        elif dtype == torch.float32 and is_c3d:
            raise RuntimeError("no folded fp32 engine for C3D (it has no BatchNorm to fold): use the module's own forward")
        elif dtype == torch.float32:
            engine = Fp32Engine(own)
        elif dtype == FP8:
            engine = Fp8EngineC3D(own) if is_c3d else Fp8Engine(own)
        else:
            raise RuntimeError(f"no inference engine for {dtype} (fp32 or bf16)")
        cached = (key, engine)
        cache[dtype] = cached
    return cached[1]
