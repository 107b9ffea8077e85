"""bf16 evaluation engine: the reference's eval loop body (main.py:224-252, BASELINE config 5)
with the VideoResNet trunk run in bf16 on ``zsv_conv3d_bf16_fwd``; ``Fp8Engine`` is the same walk in
OCP e4m3 (``float8_e4m3fn``) on ``zsv_conv3d_fp8_fwd``.

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

from ctypes import byref
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from ._lib import ConvDesc


def _check_bf16(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: MI355X HIP tensor expected, got {t.device} (there is no CPU fallback)")
    if t.dtype != torch.bfloat16 or not t.is_contiguous():
        raise RuntimeError(f"{what}: contiguous bf16 tensor expected")


def channel_pitch(channels: int) -> int:
    return int(_lib.load().zsv_bf16_channel_pitch(int(channels)))


def clip_to_bf16(x: torch.Tensor, pad_h: int, pad_w: int, hp: int, wp: int) -> torch.Tensor:
    """(N, 3, T, H, W) fp32 -> [N][T][hp][wp][4] bf16 with the frame at (pad_h, pad_w) in a zero border."""
    ops._require(x)
    x = x.contiguous()
    n, c, t, h, w = x.shape
    out = torch.empty((n, t, hp, wp, 4), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().zsv_clip_to_bf16(x.data_ptr(), n, c, t, h, w, pad_h, pad_w, hp, wp, out.data_ptr(),
                                            ops._stream()), "zsv_clip_to_bf16")
    return out


def pack_conv(d: ConvDesc, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor]) -> torch.Tensor:
    """Packed bf16 weights (x scale per produced channel) + fp32 shifts for ``conv_bf16``."""
    ops._require(weight, scale, shift)
    lib = _lib.load()
    nbytes = lib.zsv_conv3d_bf16_blob_bytes(byref(d))
    if nbytes == 0:
        raise RuntimeError("zsv_conv3d_bf16_blob_bytes: unsupported convolution geometry")
    blob = torch.empty(int(nbytes), dtype=torch.uint8, device=weight.device)
    _lib.check(lib.zsv_conv3d_bf16_pack(byref(d), weight.contiguous().data_ptr(), ops._ptr(scale), ops._ptr(shift),
                                        blob.data_ptr(), ops._stream()), "zsv_conv3d_bf16_pack")
    return blob


def conv_bf16(d: ConvDesc, x: torch.Tensor, blob: torch.Tensor, residual: Optional[torch.Tensor] = None,
              relu: bool = False) -> torch.Tensor:
    """y[N][To][Ho][Wo][Cp] = relu?(conv(x) * scale + shift (+ residual)) in bf16."""
    _check_bf16(x, "conv_bf16 input")
    expect = (d.N, d.Ti, d.Hi, d.Wi, channel_pitch(d.Cin))
    if tuple(x.shape) != expect:
        raise RuntimeError(f"conv_bf16: input {tuple(x.shape)} does not match the descriptor {expect}")
    y = torch.empty((d.N, d.To, d.Ho, d.Wo, channel_pitch(d.Cout)), dtype=torch.bfloat16, device=x.device)
    if residual is not None:
        _check_bf16(residual, "conv_bf16 residual")
        if residual.shape != y.shape:
            raise RuntimeError(f"conv_bf16: residual {tuple(residual.shape)} != output {tuple(y.shape)}")
    _lib.check(_lib.load().zsv_conv3d_bf16_fwd(byref(d), x.data_ptr(), blob.data_ptr(), ops._ptr(residual),
                                               1 if relu else 0, y.data_ptr(), ops._stream()), "zsv_conv3d_bf16_fwd")
    return y


def meanpool_bf16(x: torch.Tensor, channels: int) -> torch.Tensor:
    """[N][T][H][W][Cp] bf16 -> (N, channels) fp32 mean over the voxels."""
    _check_bf16(x, "meanpool_bf16 input")
    n = x.shape[0]
    s = x.shape[1] * x.shape[2] * x.shape[3]
    out = torch.empty((n, channels), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().zsv_meanpool_bf16(x.data_ptr(), n, s, channels, out.data_ptr(), ops._stream()),
               "zsv_meanpool_bf16")
    return out


def maxpool3d_bf16(x: torch.Tensor, channels: int, kernel, padding) -> torch.Tensor:
    """nn.MaxPool3d(kernel, stride = kernel, padding) on [N][T][H][W][Cp] bf16 (network.py:148-163)."""
    _check_bf16(x, "maxpool3d_bf16 input")
    n, t, h, w, cp = x.shape
    kt, kh, kw = (int(v) for v in kernel)
    pt, ph, pw = (int(v) for v in padding)
    to, ho, wo = (t + 2 * pt - kt) // kt + 1, (h + 2 * ph - kh) // kh + 1, (w + 2 * pw - kw) // kw + 1
    y = torch.empty((n, to, ho, wo, cp), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().zsv_maxpool3d_bf16(x.data_ptr(), n, channels, t, h, w, kt, kh, kw, pt, ph, pw, to, ho, wo, y.data_ptr(),
                                              ops._stream()), "zsv_maxpool3d_bf16")
    return y


FP8 = torch.float8_e4m3fn


def _check_fp8(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: MI355X HIP tensor expected, got {t.device} (there is no CPU fallback)")
    if t.dtype != FP8 or not t.is_contiguous():
        raise RuntimeError(f"{what}: contiguous float8_e4m3fn tensor expected")


def fp8_channel_pitch(channels: int) -> int:
    return int(_lib.load().zsv_fp8_channel_pitch(int(channels)))


def pack_conv_fp8(d: ConvDesc, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor]) -> torch.Tensor:
    """Packed e4m3 weights (w x scale, quantised per produced channel; bf16 for a clip convolution) + fp32 shifts + fp32
    dequantisation factors for ``conv_fp8``."""
    ops._require(weight, scale, shift)
    lib = _lib.load()
    nbytes = lib.zsv_conv3d_fp8_blob_bytes(byref(d))
    if nbytes == 0:
        raise RuntimeError("zsv_conv3d_fp8_blob_bytes: unsupported convolution geometry")
    blob = torch.empty(int(nbytes), dtype=torch.uint8, device=weight.device)
    _lib.check(lib.zsv_conv3d_fp8_pack(byref(d), weight.contiguous().data_ptr(), ops._ptr(scale), ops._ptr(shift),
                                       blob.data_ptr(), ops._stream()), "zsv_conv3d_fp8_pack")
    return blob


def conv_fp8(d: ConvDesc, x: torch.Tensor, blob: torch.Tensor, residual: Optional[torch.Tensor] = None,
             relu: bool = False) -> torch.Tensor:
    """y[N][To][Ho][Wo][Cp] = sat_e4m3(relu?(conv(x) * wscale + shift (+ residual))); x is e4m3, or for a clip convolution
    (Cin <= 4) the bf16 output of ``clip_to_bf16``."""
    if d.Cin <= 4:
        _check_bf16(x, "conv_fp8 clip input")
    else:
        _check_fp8(x, "conv_fp8 input")
    expect = (d.N, d.Ti, d.Hi, d.Wi, fp8_channel_pitch(d.Cin))
    if tuple(x.shape) != expect:
        raise RuntimeError(f"conv_fp8: input {tuple(x.shape)} does not match the descriptor {expect}")
    y = torch.empty((d.N, d.To, d.Ho, d.Wo, fp8_channel_pitch(d.Cout)), dtype=FP8, device=x.device)
    if residual is not None:
        _check_fp8(residual, "conv_fp8 residual")
        if residual.shape != y.shape:
            raise RuntimeError(f"conv_fp8: residual {tuple(residual.shape)} != output {tuple(y.shape)}")
    _lib.check(_lib.load().zsv_conv3d_fp8_fwd(byref(d), x.data_ptr(), blob.data_ptr(), ops._ptr(residual),
                                              1 if relu else 0, y.data_ptr(), ops._stream()), "zsv_conv3d_fp8_fwd")
    return y


def meanpool_fp8(x: torch.Tensor, channels: int) -> torch.Tensor:
    """[N][T][H][W][Cp] e4m3 -> (N, channels) fp32 mean over the voxels."""
    _check_fp8(x, "meanpool_fp8 input")
    n = x.shape[0]
    s = x.shape[1] * x.shape[2] * x.shape[3]
    out = torch.empty((n, channels), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().zsv_meanpool_fp8(x.data_ptr(), n, s, channels, out.data_ptr(), ops._stream()), "zsv_meanpool_fp8")
    return out


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


class _ConvOp:
    """One folded convolution: geometry is resolved per input shape, the packed blob per layer."""

    def __init__(self, conv: nn.Conv3d, bn: Optional[nn.BatchNorm3d], relu: bool):
        self.weight = conv.weight.detach().float().contiguous()
        self.scale, self.shift = fold_bn(bn, conv)
        self.stride = tuple(conv.stride)
        self.padding = tuple(conv.padding)
        self.relu = relu
        self.cout, self.cin = self.weight.shape[0], self.weight.shape[1]
        self.kernel = tuple(self.weight.shape[2:])
        if tuple(conv.dilation) != (1, 1, 1) or conv.groups != 1:
            raise RuntimeError("Bf16Engine: dilation / groups are not used by the reference and not supported")
        self.folded = self.cin <= 4            # the clip itself: border materialised, kw folded into K
        self._blob = None

    def input_border(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """(pad_h, pad_w, Hp, Wp) of the materialised border for the clip convolution."""
        kt, kh, kw = self.kernel
        ph, pw = self.padding[1], self.padding[2]
        wo = (w + 2 * pw - kw) // self.stride[2] + 1
        return ph, pw, h + 2 * ph, max(w + 2 * pw, (wo - 1) * self.stride[2] + 8)

    def desc(self, n: int, t: int, h: int, w: int) -> ConvDesc:
        """``h, w`` are the stored extents (border included for the clip convolution)."""
        kt, kh, kw = self.kernel
        pt, ph, pw = self.padding
        if self.folded:
            ph = pw = 0
        st, sh, sw = self.stride
        to = (t + 2 * pt - kt) // st + 1
        ho = (h + 2 * ph - kh) // sh + 1
        wo = (w + 2 * pw - kw) // sw + 1
        return ConvDesc(n, self.cin, t, h, w, self.cout, to, ho, wo, kt, kh, kw, st, sh, sw, pt, ph, pw)

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, wo: Optional[int] = None) -> torch.Tensor:
        n, t, h, w, _ = x.shape
        d = self.desc(n, t, h, w)
        if wo is not None:
            d.Wo = wo
        if self._blob is None:
            self._blob = pack_conv(d, self.weight, self.scale, self.shift)
        return conv_bf16(d, x, self._blob, residual, self.relu)


class _ConvOpFp8(_ConvOp):
    """One folded convolution of ``Fp8Engine``: e4m3 weights with per-channel factors, e4m3 output."""

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, wo: Optional[int] = None) -> torch.Tensor:
        n, t, h, w, _ = x.shape
        d = self.desc(n, t, h, w)
        if wo is not None:
            d.Wo = wo
        if self._blob is None:
            self._blob = pack_conv_fp8(d, self.weight, self.scale, self.shift)
        return conv_fp8(d, x, self._blob, residual, self.relu)


def _conv_bn_relu_chain(mods: List[nn.Module], keep_modules: bool = False, op_cls=_ConvOp) -> List[_ConvOp]:
    """[Conv3d, BN?, ReLU?, Conv3d, ...] (nested Sequentials flattened) -> folded ops."""
    flat: List[nn.Module] = []

    def walk(m):
        if isinstance(m, nn.Conv3d) or not isinstance(m, nn.Sequential):
            flat.append(m)
        else:
            for c in m:
                walk(c)
    for m in mods:
        walk(m)
    out: List[_ConvOp] = []
    i = 0
    while i < len(flat):
        conv = flat[i]
        if not isinstance(conv, nn.Conv3d):
            raise RuntimeError(f"Bf16Engine: expected a Conv3d, found {type(conv).__name__}")
        i += 1
        bn = None
        if i < len(flat) and isinstance(flat[i], nn.BatchNorm3d):
            bn = flat[i]
            i += 1
        relu = False
        if i < len(flat) and isinstance(flat[i], nn.ReLU):
            relu = True
            i += 1
        op = op_cls(conv, bn, relu)
        if keep_modules:
            op._conv, op._bn = conv, bn
        out.append(op)
    return out


class Bf16Engine:
    """Eval-mode ``Model.forward`` (network.py:533-600) in bf16.  See the module docstring."""

    _name, _op = "Bf16Engine", _ConvOp

    def __init__(self, model: nn.Module):
        from . import network, resnet
        name, chain = self._name, (lambda mods: _conv_bn_relu_chain(mods, op_cls=self._op))
        model = getattr(model, "module", model)
        if not isinstance(model, network.Model) or not isinstance(model.model, resnet.VideoResNet):
            raise RuntimeError(f"{name} supports network.Model over a resnet.VideoResNet trunk")
        if next(model.parameters()).device.type != "cuda":
            raise RuntimeError(f"{name}: the model must live on the MI355X HIP device (there is no CPU fallback)")
        self.model = model
        trunk = model.model
        self.stem = chain(list(trunk.stem))
        if not self.stem[0].folded:
            raise RuntimeError(f"{name}: the stem's first convolution must take the clip (<= 4 channels)")
        self.blocks = []
        for layer in (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4):
            for block in layer:
                if not isinstance(block, resnet.BasicBlock):
                    raise RuntimeError(f"{name}: only BasicBlock trunks (the reference's *_18 models) are supported")
                conv1 = chain(list(block.conv1))
                conv2 = chain(list(block.conv2))
                conv2[-1].relu = True                   # out += residual; relu (resnet.py:110-111)
                down = chain(list(block.downsample)) if block.downsample is not None else None
                self.blocks.append((conv1, conv2, down))
        self.features = self.blocks[-1][1][-1].cout

    def _pool(self, x: torch.Tensor) -> torch.Tensor:
        return meanpool_bf16(x, self.features)

    @torch.no_grad()
    def trunk(self, clips: torch.Tensor) -> torch.Tensor:
        """(N, 3, T, H, W) fp32 -> pooled (N, 512) fp32 (VideoResNet.forward's first output)."""
        first = self.stem[0]
        n, _, t, h, w = clips.shape
        pad_h, pad_w, hp, wp = first.input_border(h, w)
        wo = (w + 2 * pad_w - first.kernel[2]) // first.stride[2] + 1
        x = clip_to_bf16(clips, pad_h, pad_w, hp, wp)
        x = first(x, wo=wo)
        for op in self.stem[1:]:
            x = op(x)
        for conv1, conv2, down in self.blocks:
            residual = x
            if down is not None:
                for op in down:
                    residual = op(residual)
            y = x
            for op in conv1:
                y = op(y)
            for op in conv2[:-1]:
                y = op(y)
            x = conv2[-1](y, residual=residual)
        return self._pool(x)

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

    _name, _op = "Fp8Engine", _ConvOpFp8

    def _pool(self, x: torch.Tensor) -> torch.Tensor:
        return meanpool_fp8(x, self.features)


class Bf16EngineC3D:
    """Eval-mode ``network.C3D.forward`` (network.py:147-179) with the eight convolutions and five max-pools in bf16 on the
    channels-last layout: ``relu(conv(x) + bias)`` is one ``zsv_conv3d_bf16_fwd`` launch per layer (bias as the epilogue's
    shift), the pools are ``zsv_maxpool3d_bf16``; fc6 (+ ReLU), the clip mean, the regressor and the normalisation stay fp32
    (dropout is the identity in eval mode).  Same contract as the module: ``(bs, nc, 3, T, H, W) fp32 -> (bs, 300)``."""

    LAYERS = (("conv1", "pool1"), ("conv2", "pool2"), ("conv3a", None), ("conv3b", "pool3"), ("conv4a", None), ("conv4b", "pool4"),
              ("conv5a", None), ("conv5b", "pool5"))

    def __init__(self, model: nn.Module):
        from . import network
        model = getattr(model, "module", model)
        if not isinstance(model, network.C3D):
            raise RuntimeError("Bf16EngineC3D supports network.C3D")
        if next(model.parameters()).device.type != "cuda":
            raise RuntimeError("Bf16EngineC3D: the model must live on the MI355X HIP device (there is no CPU fallback)")
        self.model = model
        self.ops = []
        for conv_name, pool_name in self.LAYERS:
            op = _ConvOp(getattr(model, conv_name), None, True)           # network.py:147-162: relu(conv(x)), bias in the epilogue
            pool = getattr(model, pool_name) if pool_name else None
            if pool is not None:
                k, st, pd = pool.kernel_size, pool.stride, pool.padding
                k = (k,) * 3 if isinstance(k, int) else tuple(k)
                st = k if st is None else ((st,) * 3 if isinstance(st, int) else tuple(st))
                pd = (pd,) * 3 if isinstance(pd, int) else tuple(pd)
                if st != k:
                    raise RuntimeError("Bf16EngineC3D: max-pools with stride != kernel are not used by the reference")
                pool = (k, pd)
            self.ops.append((op, pool))
        if not self.ops[0][0].folded:
            raise RuntimeError("Bf16EngineC3D: conv1 must take the clip (<= 4 channels)")

    @torch.no_grad()
    def features(self, clips: torch.Tensor) -> torch.Tensor:
        """(N, 3, T, H, W) fp32 -> (N, 8192) fp32 in the (C, T, H, W) order of ``view(-1, 8192)`` (network.py:165)."""
        first = self.ops[0][0]
        n, _, t, h, w = clips.shape
        pad_h, pad_w, hp, wp = first.input_border(h, w)
        wo = (w + 2 * pad_w - first.kernel[2]) // first.stride[2] + 1
        x = clip_to_bf16(clips, pad_h, pad_w, hp, wp)
        for i, (op, pool) in enumerate(self.ops):
            x = op(x, wo=wo) if i == 0 else op(x)
            if pool is not None:
                x = maxpool3d_bf16(x, op.cout, pool[0], pool[1])
        c = self.ops[-1][0].cout
        return x[..., :c].permute(0, 4, 1, 2, 3).reshape(n, -1).float()

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
        from . import network, resnet
        model = getattr(model, "module", model)
        if not isinstance(model, network.Model) or not isinstance(model.model, resnet.VideoResNet):
            raise RuntimeError("Fp32Engine supports network.Model over a resnet.VideoResNet trunk")
        if next(model.parameters()).device.type != "cuda":
            raise RuntimeError("Fp32Engine: the model must live on the MI355X HIP device (there is no CPU fallback)")
        self.model = model
        chain = lambda mods: [_ConvOpF32(o._conv, o._bn, o.relu) for o in _conv_bn_relu_chain(mods, keep_modules=True)]
        trunk = model.model
        self.stem = chain(list(trunk.stem))
        self.blocks = []
        for layer in (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4):
            for block in layer:
                if not isinstance(block, resnet.BasicBlock):
                    raise RuntimeError("Fp32Engine: only BasicBlock trunks (the reference's *_18 models) are supported")
                conv1, conv2 = chain(list(block.conv1)), chain(list(block.conv2))
                conv2[-1].relu = True                   # out += residual; relu (resnet.py:110-111)
                down = chain(list(block.downsample)) if block.downsample is not None else None
                self.blocks.append((conv1, conv2, down))

    @torch.no_grad()
    def trunk(self, clips: torch.Tensor) -> torch.Tensor:
        ops._require(clips)
        x = clips.contiguous()
        for op in self.stem:
            x = op(x)
        for conv1, conv2, down in self.blocks:
            residual = x
            if down is not None:
                for op in down:
                    residual = op(residual)
            y = x
            for op in conv1:
                y = op(y)
            for op in conv2[:-1]:
                y = op(y)
            x = conv2[-1](y, residual=residual)
        return ops.mean_pool(x)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor):
        bs, nc = x.shape[:2]
        pooled = self.trunk(x.reshape(bs * nc, *x.shape[2:]))
        return F.normalize(self.model.output2emb_proj(pooled), dim=-1), None


def engine_for(model: nn.Module, dtype: torch.dtype = torch.bfloat16, rebuild: bool = False):
    """The model's inference engine for ``dtype`` (bf16: ``Bf16Engine``, fp32: ``Fp32Engine``, ``torch.float8_e4m3fn``:
    ``Fp8Engine``, VideoResNet trunks only), rebuilt only when a
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
    cache = own.__dict__.setdefault("_zsv_engines", {})
    cached = None if rebuild else cache.get(dtype)
    if cached is None or cached[0] != key:
        if dtype == torch.bfloat16:
            engine = Bf16EngineC3D(own) if is_c3d else Bf16Engine(own)
        elif dtype == torch.float32 and is_c3d:
            raise RuntimeError("no folded fp32 engine for C3D (it has no BatchNorm to fold): use the module's own forward")
        elif dtype == torch.float32:
            engine = Fp32Engine(own)
        elif dtype == FP8 and is_c3d:
            raise RuntimeError("C3D has no fp8 (float8_e4m3fn) engine: use bf16 or the module's own forward")
        elif dtype == FP8:
            engine = Fp8Engine(own)
        else:
            raise RuntimeError(f"no inference engine for {dtype} (fp32 or bf16)")
        cached = (key, engine)
        cache[dtype] = cached
    return cached[1]
