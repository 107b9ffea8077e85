"""``torch.nn`` layer classes whose ``forward`` runs the gfx950 kernels.

Each class subclasses the torch layer the reference instantiates, so constructor
signatures, parameter / buffer names (``state_dict`` keys), initialisation and ``repr`` are
inherited unchanged; only ``forward`` differs: it calls ``ops`` (HIP kernels through the C
ABI) and raises on CPU tensors -- there is no fallback path.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops


class Conv3d(nn.Conv3d):
    """nn.Conv3d with dilation 1, zero padding and groups 1 (all the reference uses) or groups == in_channels == out_channels
    (depthwise: the middle convolution of the channel-separated residual unit)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        depthwise = self.groups == self.in_channels == self.out_channels
        if self.dilation != (1, 1, 1) or not (self.groups == 1 or depthwise) or self.padding_mode != "zeros" \
                or isinstance(self.padding, str):
            raise NotImplementedError("only dilation=1, groups=1 or depthwise (groups == in_channels == out_channels), zero padding "
                                      "are on the hot path")

    def forward(self, x, relu: bool = False, want_stats: bool = False):
        """``want_stats=True`` returns ``(y, stats)``: BatchNorm partial statistics of ``y`` gathered in
        the kernel epilogue (None when the geometry does not provide them; always None for a depthwise layer)."""
        return ops.conv3d(x, self.weight, self.bias, self.stride, self.padding, relu=relu, want_stats=want_stats, groups=self.groups)

    def pre_supported(self, x_shape) -> bool:
        """Can this convolution take a training-mode ``BatchNorm3d -> ReLU`` in front of it inside its own kernels?"""
        if self.groups != 1:
            return False
        return self.bias is None and ops.conv_pre_supported(x_shape, self.weight.shape, self.stride, self.padding)

    def forward_pre(self, x, coef, want_stats: bool = False):
        """``self(relu(x * scale + shift))`` with ``coef`` from ``BatchNorm3d.deferred``: the normalised tensor is never
        written (resnet.py:46-52, the mid tensor of ``Conv2Plus1D``)."""
        return ops.conv3d_pre(x, coef, self.weight, self.stride, self.padding, want_stats=want_stats)


class BatchNorm3d(nn.BatchNorm3d):
    def forward(self, x, residual=None, relu: bool = False, stats=None, skip_link=None, defer: bool = False):
        """``defer=True`` (training mode, followed by ReLU and a convolution that ``pre_supported`` it): statistics, running
        statistics and the affine coefficients WITHOUT the normalise pass -- returns ``(x_handle, coef)`` for
        ``Conv3d.forward_pre``."""
        if x.dim() != 5:
            raise ValueError(f"expected 5D input (got {x.dim()}D input)")
        if defer:
            return ops.bn_module_deferred(x, self, stats=stats)
        return ops.bn_module_act(x, self, residual=residual, relu=relu, stats=stats, skip_link=skip_link)

    def deferred(self, x, stats=None):
        return self(x, stats=stats, defer=True)


class SyncBatchNorm3d(BatchNorm3d):
    """``BatchNorm3d`` whose training-mode batch statistics are taken over every rank of ``process_group`` (default: the world):
    ``torch.nn.SyncBatchNorm`` for this package's fused passes.  Same parameters, buffers and ``state_dict`` keys as
    ``BatchNorm3d`` (``ddp.convert_sync_batchnorm`` swaps the class and keeps the tensors).  It synchronises only in training
    mode with ``torch.distributed`` initialised and a world size above 1 -- torch's rule; in every other case (eval mode, a
    frozen backward, no process group, one rank) ``forward`` IS the parent's, bit for bit and with all its fusions.  fp32 only:
    ``amp.autocast()`` refuses a trunk with a layer that would synchronise."""

    def __init__(self, num_features, eps: float = 1e-5, momentum=0.1, affine: bool = True, track_running_stats: bool = True,
                 process_group=None, device=None, dtype=None):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        self.process_group = process_group

    def synchronizes(self) -> bool:
        """Would a forward in the current mode exchange statistics?"""
        if not self.training:
            return False
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1

    def forward(self, x, residual=None, relu: bool = False, stats=None, skip_link=None, defer: bool = False):
        """The parent's signature.  When synchronising: BatchNorm + residual + ReLU stay one apply pass and ``skip_link`` is
        honoured; ``stats`` (the producing convolution's epilogue sums) are not used -- the moments pass shifts by a pivot,
        the epilogue does not -- and ``defer=True`` is refused: the fold's backward is ``zsv_bn_bwd`` with this rank's sums
        alone (``resnet._run_chain`` asks a synchronising layer for neither)."""
        if not self.synchronizes():
            return super().forward(x, residual=residual, relu=relu, stats=stats, skip_link=skip_link, defer=defer)
        if x.dim() != 5:
            raise ValueError(f"expected 5D input (got {x.dim()}D input)")
        if defer:
            raise RuntimeError("SyncBatchNorm3d: a synchronising layer has no deferred fold into the next convolution")
        return ops.sync_bn_module_act(x, self, residual=residual, relu=relu, skip_link=skip_link)


def synchronizes(m: nn.Module) -> bool:
    """True for a ``SyncBatchNorm3d`` that would exchange statistics in its current mode (False for every other module)."""
    return isinstance(m, SyncBatchNorm3d) and m.synchronizes()


class ReLU(nn.ReLU):
    """``inplace`` is accepted for signature compatibility; the kernel writes a fresh tensor and
    keeps only the output for backward, which is what inplace ReLU keeps too."""

    def forward(self, x):
        return ops.relu(x)


class Linear(nn.Linear):
    def forward(self, x, relu: bool = False):
        lead = x.shape[:-1]
        y = ops.linear(x.reshape(-1, x.shape[-1]), self.weight, self.bias, relu=relu)
        return y.reshape(*lead, y.shape[-1])


class MaxPool3d(nn.MaxPool3d):
    def forward(self, x):
        if self.dilation not in (1, (1, 1, 1)) or self.ceil_mode or self.return_indices:
            raise NotImplementedError("MaxPool3d: dilation/ceil_mode/return_indices are not on the hot path")
        return ops.max_pool3d(x, self.kernel_size, self.stride, self.padding)


class AdaptiveAvgPool3d(nn.AdaptiveAvgPool3d):
    """Only the global (1,1,1) form the reference builds (resnet.py:222)."""

    def forward(self, x):
        if tuple(self.output_size) != (1, 1, 1):
            raise NotImplementedError("only AdaptiveAvgPool3d((1,1,1)) is on the hot path")
        return ops.mean_pool(x).reshape(x.shape[0], x.shape[1], 1, 1, 1)
