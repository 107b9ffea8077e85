"""Fused multi-tensor Adam and SGD and an on-device loss scaler (main.py:131-137,195-203).

The reference steps ``torch.optim.Adam(model.parameters(), lr)`` (betas (0.9, 0.999), eps 1e-8, no weight
decay, no amsgrad) under ``torch.cuda.amp.GradScaler``: ``scaler.scale(loss).backward();
scaler.step(optimizer); scaler.update()``.

``FusedAdam`` keeps that update rule and the same ``state_dict`` layout (``step`` / ``exp_avg`` /
``exp_avg_sq`` per parameter) but applies it to every parameter that has a gradient with ONE launch of
``zsv_adam_multi`` driven by a descriptor table {p, g, m, v, n, first_chunk}:

* default: the table is rebuilt on the host every step (autograd re-allocates the gradients, so their addresses
  change), uploaded through a small pinned ring, and a grid of 4096-element chunks walks all tensors;
* ``grad_buckets=<ddp.GradientSync>``: the gradients live in the flat all-reduce buckets of the data-parallel
  exchange (``.grad`` are views of them), ``exp_avg`` / ``exp_avg_sq`` are allocated as matching flat buffers
  (the per-parameter state entries are views), and the table is built and uploaded ONCE per bucket layout --
  Adam reads the all-reduce buffers directly, no pack / unpack copies and no per-step host work.

Parameters without a gradient (the reference's dead Transformer encoder etc.) are skipped exactly
like torch does.

``LossScaler`` is ``GradScaler`` with its state (scale, growth tracker, found-inf flag, count of steps
actually taken) in device memory: the non-finite check (``zsv_grad_check_multi``), the skip-on-inf Adam step
with the 1/scale folded into the gradient read (``zsv_adam_multi_scaled``) and the scale update
(``zsv_scaler_update``) are three launches and no host synchronisation.

Fine-tuning options (csrc/optim.hip), all off by default -- with ``weight_decay == 0`` in every group and
``max_grad_norm is None`` the step calls ``zsv_adam_multi`` / ``zsv_adam_multi_scaled`` exactly as before:

* ``weight_decay`` / ``decoupled_weight_decay`` per parameter group: ``torch.optim.Adam(weight_decay=)`` (L2, the decay joins
  the gradient) or ``torch.optim.AdamW`` (decoupled, ``p *= 1 - lr * wd``), inside the same single launch
  (``zsv_adamw_multi`` / ``zsv_adamw_multi_scaled``);
* ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_`` over every parameter of every group.  One extra read of the
  gradients (``zsv_grad_norm_multi``: sum of squares per chunk, which also serves as the scaler's non-finite check), one
  small launch that sums the partials in a fixed order in double and leaves ``{total_norm, clip_coef}`` on the device
  (``zsv_grad_norm_finalize``), and the update multiplies each gradient by ``clip_coef`` as it reads it.  ``.grad`` is NOT
  rewritten (torch's ``clip_grad_norm_`` rewrites it).  ``FusedAdam.grad_norm`` is the device-resident total norm;
* ``LossScaler.unscale_(optimizer)``: ``GradScaler.unscale_`` (``zsv_grad_unscale_multi``) for loops that keep torch's literal
  ``unscale_`` + ``clip_grad_norm_`` + ``step`` recipe.

No floating-point atomics: the same gradients give the same norm bits and the same parameter bits on every run.

``WeightAverage(optimizer, decay=)`` keeps an exponential moving average (``decay=None``: an equal-weight running mean, SWA) of
every parameter of a ``FusedAdam`` or ``FusedSGD`` -- ``torch.optim.swa_utils.AveragedModel`` folded into the optimizer's own
launch: the ``*_avg`` entry points (the same kernel with the average compiled in, csrc/optim.hip) apply it with the new parameter
value still in a register, the count of averaged steps is device state (a step the scaler skips averages nothing, and the host
never learns which it was), and ``applied()`` swaps the averaged values INTO the live tensors for evaluation.  Without a
``WeightAverage`` the step launches what it always did.

``FusedSGD`` is ``torch.optim.SGD`` -- momentum, dampening, Nesterov, L2 weight decay, ``maximize``, the recipe torchvision trained
these trunks with -- on the same machinery, which lives in ``_FusedOptimizer``, the base class of both: descriptor tables (per step
or once per bucket layout, the momentum buffers then flat like the buckets), ``max_grad_norm``, ``LossScaler``, ``WeightAverage`` and
``step()`` itself (tables, the norm pass or the check for every group, then one update launch per group, the average's own
launches, the host's bookkeeping); a subclass supplies the launch of one group (``_update``) and that bookkeeping.  One
``zsv_sgd_multi`` launch per parameter group (csrc/sgd.hip: 16 bytes per lane where a tensor's pointers allow it); clip record, scaler
state and shadows are NULL-able arguments of that ONE entry point.  The state is torch's (``momentum_buffer``).  torch's first step
copies the gradient into the new buffer; here the launch is told -- by the host, or under a scaler by the device-resident count of
steps taken, so that a skipped first step leaves the next one the first -- whether it is that step.

``FusedLARS`` and ``FusedLAMB`` are ``FusedSGD`` and ``FusedAdam`` with the update of every parameter tensor scaled by a trust ratio of
two 2-norms over that tensor -- the large-batch forms of the two recipes.  Three launches per parameter group (csrc/layerwise.hip;
the LARS update is ``zsv_sgd_multi``'s kernel with the ratio compiled in, csrc/sgd.hip):
partial sums per chunk (LAMB's also updates the moments), one workgroup per tensor that leaves ``{|p|, |g| or |u|, ratio}`` on the
device, the update.  No host synchronisation, no atomics; everything the base class gives works with both.  ``layer_norms`` is the
per-layer norm monitor, ``layerwise_groups(model, weight_decay)`` the usual split into adapting weights and non-adapting affines / biases.
"""
from __future__ import annotations

import contextlib
import math
import struct
from ctypes import c_void_p
from typing import Optional

import torch

from . import _lib
from ._tables import PinnedRing, pack_rows


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class LossScaler:
    """``torch.cuda.amp.GradScaler`` (main.py:137) with device-resident state; same defaults."""

    def __init__(self, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("LossScaler keeps its state on an MI355X HIP device (no CPU fallback)")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # zsv_scaler_state {float scale; int32 growth_tracker; int32 found_inf; int32 steps_done}
        host = torch.zeros(4, dtype=torch.int32)
        host.view(torch.float32)[0] = float(init_scale)
        self._state = host.to(self.device)
        self._scale = self._state.view(torch.float32)[0:1]
        self._unscaled = set()                            # id() of the optimizers unscale_() has run on since update()

    @property
    def state_ptr(self) -> int:
        return self._state.data_ptr()

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """``scaler.scale(loss)`` (main.py:195): multiplied on the device, differentiable."""
        return loss * self._scale.detach().reshape(())

    def step(self, optimizer) -> None:
        """``scaler.step(optimizer)`` (main.py:200): unscale + non-finite check + (skipped-if-inf) optimizer step."""
        if not isinstance(optimizer, _FusedOptimizer):
            raise RuntimeError("LossScaler.step drives optim.FusedAdam, optim.FusedSGD, optim.FusedLARS or optim.FusedLAMB "
                               "(the check, unscale and skip run inside their kernels)")
        optimizer.step(scaler=self)

    def unscale_(self, optimizer) -> None:
        """``GradScaler.unscale_(optimizer)``: the gradients of ``optimizer`` are multiplied by 1/scale in place and
        ``found_inf`` is set if any is non-finite (``zsv_grad_unscale_multi``, no host synchronisation).  The following
        ``step(optimizer)`` does not unscale again; a second call before ``update()`` raises, as torch's does.  For
        ``scaler.unscale_(opt); torch.nn.utils.clip_grad_norm_(...); scaler.step(opt)``; ``FusedAdam(max_grad_norm=)``
        is the fused route, which needs no ``unscale_``."""
        if not isinstance(optimizer, _FusedOptimizer):
            raise RuntimeError("LossScaler.unscale_ drives optim.FusedAdam, optim.FusedSGD, optim.FusedLARS or optim.FusedLAMB")
        if id(optimizer) in self._unscaled:
            raise RuntimeError("unscale_() has already been called on this optimizer since the last update().")
        optimizer._unscale(self)
        self._unscaled.add(id(optimizer))

    def update(self) -> None:
        """``scaler.update()`` (main.py:203)."""
        self._unscaled.clear()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().zsv_scaler_update(self.state_ptr, self.growth_factor, self.backoff_factor,
                                                     self.growth_interval, _stream()), "zsv_scaler_update")

    def state(self) -> dict:
        """Host copy of the device state (synchronises): scale, growth_tracker, found_inf, steps_done."""
        host = self._state.cpu()
        return {"scale": float(host.view(torch.float32)[0]), "growth_tracker": int(host[1]), "found_inf": int(host[2]),
                "steps_done": int(host[3])}

    def get_scale(self) -> float:
        return self.state()["scale"]

    def state_dict(self) -> dict:
        """``GradScaler.state_dict()`` keys (``scale``, ``growth_factor``, ``backoff_factor``, ``growth_interval``,
        ``_growth_tracker``) plus ``steps_done`` -- the count of optimizer steps actually taken, which the Adam bias
        correction reads on the device.  One host sync."""
        st = self.state()
        return {"scale": st["scale"], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": st["growth_tracker"], "steps_done": st["steps_done"]}

    def load_state_dict(self, state: dict) -> None:
        """Resume: uploads the 4-word device state.  A ``torch.amp.GradScaler`` state dict is accepted too (no
        ``steps_done``: the count is then taken from the optimizer when it adopts this scaler)."""
        self.growth_factor = float(state.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(state.get("backoff_factor", self.backoff_factor))
        self.growth_interval = int(state.get("growth_interval", self.growth_interval))
        host = torch.zeros(4, dtype=torch.int32)
        host.view(torch.float32)[0] = float(state["scale"])
        host[1] = int(state.get("_growth_tracker", 0))
        host[3] = int(state.get("steps_done", 0))
        self._state.copy_(host)

    def _seed_steps_done(self, steps: int) -> None:
        host = self._state.cpu()
        host[3] = int(steps)
        self._state.copy_(host)


class _FusedOptimizer(torch.optim.Optimizer):
    """What ``FusedAdam`` and ``FusedSGD`` share: the descriptor tables {p, g, state, state, n, first_chunk} -- rebuilt per step and
    uploaded through a pinned ring, or built once per layout over the flat gradient buckets -- the ``LossScaler`` they are driven
    by, ``LossScaler.unscale_``, the norm pass of ``max_grad_norm``, the ``WeightAverage`` that rides in their launches, and
    ``step()``.  A subclass validates its defaults and calls ``_setup``; it checks one group (``_check_group``), creates its own
    host-side fields (``_reset_rule_state``), names its per-parameter state tensors (``_state_keys``), creates them
    (``_entry_state``), launches the update of one group (``_update``) and keeps its own count of steps (``_after_step``)."""

    def _setup(self, params, defaults, max_grad_norm, grad_buckets):
        """What every constructor does once it has validated its defaults: torch's own set-up, the check of every group, the
        fields of this class and those of the update rule."""
        torch.optim.Optimizer.__init__(self, params, defaults)
        for group in self.param_groups:
            self._check_group(group)
        self._init_fused(max_grad_norm, grad_buckets)
        self._reset_rule_state()

    def _check_group(self, group):
        """Raise ``ValueError`` on a group option the update rule cannot take."""
        raise NotImplementedError

    def _reset_rule_state(self):
        """Create the host-side fields of the update rule as they are before the first step (each rule names its own once)."""
        raise NotImplementedError

    def _init_fused(self, max_grad_norm, grad_buckets):
        self.max_grad_norm = max_grad_norm
        self._clip = None                                 # zsv_clip_record {total_norm, clip_coef} on the device
        self._partials = None                             # one float per gradient chunk (zsv_grad_norm_multi)
        self._ring = PinnedRing(4)                        # staging for the per-step descriptor tables
        self.grad_buckets = grad_buckets                  # ddp.GradientSync (or None)
        self._static = None                               # (layout_version, table, count, chunks, [(p, grad ptr)], flats)
        self._scaler: Optional[LossScaler] = None
        self._average: Optional["WeightAverage"] = None   # set by WeightAverage(optimizer): the update launches average too

    @staticmethod
    def _check_max_grad_norm(max_grad_norm):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
                raise ValueError(f"max_grad_norm must be a finite positive number or None, not {max_grad_norm}")
        return max_grad_norm

    @staticmethod
    def _check_decay(weight_decay):
        if not (isinstance(weight_decay, (int, float)) and math.isfinite(weight_decay) and weight_decay >= 0):
            raise ValueError(f"weight_decay must be a finite number >= 0, not {weight_decay}")

    @property
    def grad_norm(self) -> torch.Tensor:
        """2-norm of all gradients of the last ``step()`` (unscaled, before clipping) as a 0-d device tensor; reading it
        does not synchronise.  Valid after a step when ``max_grad_norm`` is set.  On a step the scaler skipped it holds
        what the non-finite gradients gave (inf or NaN)."""
        if self._clip is None:
            raise RuntimeError(f"{type(self).__name__}.grad_norm is available after step() of an optimizer built with max_grad_norm=")
        return self._clip[0]

    # -- descriptor tables ------------------------------------------------------------------------
    @classmethod
    def _check_param(cls, p):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError(f"{cls.__name__} needs contiguous fp32 parameters on a HIP device (no CPU fallback)")

    def _upload(self, raw: bytearray, dev) -> torch.Tensor:
        return self._ring.upload(raw, dev)                # pinned ring guarded by events (_tables.PinnedRing)

    def _state_keys(self, group):
        """Names of the per-parameter state tensors behind the `exp_avg` / `exp_avg_sq` fields of the descriptor (at most two)."""
        raise NotImplementedError

    def _entry_state(self, p, group):
        """The state dict of a parameter about to enter a table, created (and checked) as the update rule needs it."""
        raise NotImplementedError

    def _rehome(self, st, keys, views):
        """Move the state tensors of one parameter into their views of the flat buffers of the bucket path."""
        raise NotImplementedError

    def _dynamic_table(self, group):
        keys = self._state_keys(group)
        rows, keep, live = [], [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            self._check_param(p)
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            st = self._entry_state(p, group)
            ptrs = [st[k].data_ptr() for k in keys] + [0] * (2 - len(keys))
            rows.append((p.data_ptr(), g.data_ptr(), ptrs[0], ptrs[1], p.numel()))
            keep.append(g)
            live.append(p)
        if not rows:
            return None
        raw, chunks = pack_rows(rows)
        if self._average is not None:
            raw += self._average._shadow_pointers(live)   # the shadow-pointer array rides behind the table (_avg_args)
        table = self._upload(raw, keep[0].device)
        return table, len(rows), chunks, keep

    def _static_table(self, group):
        """Table over the flat gradient buckets, built once per bucket layout; None when it does not apply this
        step (buckets not built yet, several parameter groups, or a ``.grad`` that is not its bucket view)."""
        sync = self.grad_buckets
        if sync is None or not sync.ready or len(self.param_groups) != 1:
            return None
        if self._static is None or self._static[0] != sync.layout_version:
            keys = self._state_keys(group)
            mine = {id(p) for p in group["params"]}
            rows, expect, flats = [], [], []
            for flat, slices in sync.bucket_layout():
                if not flat.is_cuda:
                    return None
                state_flats = tuple(torch.zeros_like(flat) for _ in keys)
                flats.append(state_flats)
                for p, off in slices:
                    if id(p) not in mine:
                        raise RuntimeError(f"{type(self).__name__}: a bucketed parameter is not in this optimizer")
                    self._check_param(p)
                    n = p.numel()
                    views = [f[off:off + n].view_as(p) for f in state_flats]
                    self._rehome(self.state[p], keys, views)      # state from the discovery step(s) moves into the flat buffers
                    ptrs = [v.data_ptr() for v in views] + [0] * (2 - len(keys))
                    gptr = flat.data_ptr() + 4 * off
                    rows.append((p.data_ptr(), gptr, ptrs[0], ptrs[1], n))
                    expect.append((p, gptr))
            raw, chunks = pack_rows(rows)
            if self._average is not None:
                raw += self._average._shadow_pointers([p for p, _ in expect])       # once per layout, like the table
            dev = expect[0][0].device
            table = torch.frombuffer(raw, dtype=torch.uint8).to(dev)          # once per layout: a blocking copy is fine
            self._static = (sync.layout_version, table, len(rows), chunks, expect, flats)
        _, table, count, chunks, expect, _ = self._static
        bucketed = {id(p) for p, _ in expect}
        for p, gptr in expect:
            if p.grad is None or p.grad.data_ptr() != gptr:
                return None
        for p in group["params"]:
            if p.grad is not None and id(p) not in bucketed:
                return None
        return table, count, chunks, []

    def _on_adopt(self, scaler: "LossScaler") -> None:
        """A scaler drives this optimizer from now on: what the update rule needs to know at that moment."""

    def _adopt(self, scaler: Optional[LossScaler]) -> None:
        if scaler is not None and self._scaler is None:
            self._on_adopt(scaler)
            self._scaler = scaler
        if self._scaler is not None and scaler is not self._scaler:
            raise RuntimeError(f"{type(self).__name__}: this optimizer is driven by a LossScaler; step through scaler.step(optimizer)")

    def _avg_args(self, table, count):
        """(shadow-pointer array, averaging state, EMA weight) of a launch: the pointers sit behind the ``count`` descriptors.
        Without a ``WeightAverage``: the NULLs that tell the launch so."""
        if self._average is None:
            return None, None, 0.0
        return table.data_ptr() + 48 * count, self._average._state_ptr(table.device), self._average._ema_weight

    def _tables(self):
        work = []
        for group in self.param_groups:
            built = self._static_table(group) or self._dynamic_table(group)
            if built is not None:
                work.append((group, built))
        return work

    def _unscale(self, scaler: LossScaler) -> None:
        """``LossScaler.unscale_``: g *= 1/scale in place + the non-finite check, one launch per parameter group."""
        self._adopt(scaler)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None and not p.grad.is_contiguous():
                    raise RuntimeError("LossScaler.unscale_ rewrites the gradients in place and needs them contiguous")
        lib = _lib.load()
        for _, (table, count, chunks, keep) in self._tables():
            with torch.cuda.device(table.device):
                _lib.check(lib.zsv_grad_unscale_multi(table.data_ptr(), count, chunks, scaler.state_ptr, _stream()),
                           "zsv_grad_unscale_multi")
            table.record_stream(torch.cuda.current_stream())
            del keep
        _lib.note_raw_write()                      # gradients rewritten through raw pointers

    def _norm_pass(self, lib, work, scaler: Optional[LossScaler], unscaled: bool):
        """What comes before the update launches of a step: with ``max_grad_norm`` the norm pass per group (which is the scaler's
        non-finite check as well) and the finalize, otherwise the check alone under a scaler whose gradients are still scaled in
        memory -- every group before any is updated.  Returns the device address of the clip record, or None."""
        state_ptr = scaler.state_ptr if scaler is not None else None
        scaled_in_memory = scaler is not None and not unscaled
        clip_ptr = None
        if self.max_grad_norm is not None:
            dev = work[0][1][0].device
            total = sum(chunks for _, (_, _, chunks, _) in work)
            nbytes = int(lib.zsv_grad_norm_workspace_bytes(total))
            if self._clip is None or self._clip.device != dev:
                self._clip = torch.zeros(2, dtype=torch.float32, device=dev)
            if self._partials is None or self._partials.device != dev or self._partials.numel() * 4 < nbytes:
                self._partials = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
            offset = 0
            with torch.cuda.device(dev):
                for _, (table, count, chunks, _keep) in work:
                    # with a scaler this read of the gradients is the non-finite check as well (all groups before any update)
                    _lib.check(lib.zsv_grad_norm_multi(table.data_ptr(), count, chunks, offset, self._partials.data_ptr(),
                                                       self._partials.numel() * 4, state_ptr if scaled_in_memory else None,
                                                       _stream()), "zsv_grad_norm_multi")
                    offset += chunks
                _lib.check(lib.zsv_grad_norm_finalize(self._partials.data_ptr(), total, self.max_grad_norm,
                                                      state_ptr if scaled_in_memory else None, self._clip.data_ptr(),
                                                      _stream()), "zsv_grad_norm_finalize")
            clip_ptr = self._clip.data_ptr()
        elif scaled_in_memory:
            for _, (table, count, chunks, _keep) in work:
                with torch.cuda.device(table.device):
                    _lib.check(lib.zsv_grad_check_multi(table.data_ptr(), count, chunks, state_ptr, _stream()),
                               "zsv_grad_check_multi")
        return clip_ptr

    # -- step -------------------------------------------------------------------------------------
    def _check_groups(self) -> None:
        """Raise on a group option the update rule cannot take (the groups are editable between steps)."""

    def _update(self, lib, scaler: Optional[LossScaler], unscaled: bool, clip_ptr):
        """Decide once what this step's launches share and return ``launch(group, table, count, chunks)``, which launches the
        update of one parameter group on the current stream."""
        raise NotImplementedError

    def _after_step(self, scaler: Optional[LossScaler]) -> None:
        """Host bookkeeping after the launches of a step (under a scaler the host does not know whether it was taken)."""

    @torch.no_grad()
    def step(self, closure=None, scaler: Optional[LossScaler] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._adopt(scaler)
        lib = _lib.load()
        avg = self._average
        if avg is not None:
            avg._check_live()
        self._check_groups()
        work = self._tables()
        if not work:
            return loss
        unscaled = scaler is not None and id(self) in scaler._unscaled      # LossScaler.unscale_ has run on these gradients
        # GradScaler.step checks EVERY gradient before the optimizer touches anything (an inf in the last group must skip the first
        # group's update too): the norm pass or the check, all groups first
        clip_ptr = self._norm_pass(lib, work, scaler, unscaled)
        launch = self._update(lib, scaler, unscaled, clip_ptr)
        for group, (table, count, chunks, keep) in work:
            with torch.cuda.device(table.device):
                launch(group, table, count, chunks)
            # keep the uploaded table and any contiguous gradient copies alive until the stream is past the launch
            table.record_stream(torch.cuda.current_stream())
            del keep
        del work
        if avg is not None:
            avg._after_update(lib, scaler)         # BatchNorm statistics, then n_averaged += !found_inf (before scaler.update())
        self._after_step(scaler)
        _lib.note_raw_write()                      # parameters updated through raw pointers
        return loss


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` / ``torch.optim.AdamW`` in one launch per parameter group (module docstring).

    ``weight_decay`` and ``decoupled_weight_decay`` are per parameter group, like ``lr``: ``decoupled_weight_decay=False``
    is ``Adam(weight_decay=)`` (L2: ``g += wd * p``), ``True`` is ``AdamW`` (``p *= 1 - lr * wd``).  Parameters without a
    gradient are skipped, decay included, as torch does; a step the ``LossScaler`` skips applies no decay either.

    ``max_grad_norm`` belongs to the optimizer and spans all groups: the gradients are scaled by
    ``min(1, max_grad_norm / (total_norm + 1e-6))`` -- ``clip_grad_norm_`` with ``norm_type=2`` over all parameters -- on
    their way into the update.  ``.grad`` itself is not rewritten (torch's ``clip_grad_norm_`` rewrites it).  With
    ``grad_buckets=`` the norm is that of the averaged gradients, identical on every rank."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False,
                 max_grad_norm=None, grad_buckets=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        self._check_decay(weight_decay)
        max_grad_norm = self._check_max_grad_norm(max_grad_norm)
        self._setup(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                 decoupled_weight_decay=bool(decoupled_weight_decay)), max_grad_norm, grad_buckets)

    @classmethod
    def _check_group(cls, group):
        cls._check_decay(group["weight_decay"])
        if not (math.isfinite(group["lr"]) and group["lr"] >= 0):
            raise ValueError(f"invalid learning rate {group['lr']}")

    def _reset_rule_state(self):
        self._host_steps = 0                              # steps taken without a scaler
        self._resumed = False                             # state came from load_state_dict (a scaler may then join late)

    # -- descriptor tables ------------------------------------------------------------------------
    def _ensure_state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _state_keys(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _entry_state(self, p, group):
        st = self._ensure_state(p)
        if self._scaler is None and int(st["step"].item()) != self._host_steps:
            raise RuntimeError("FusedAdam: every parameter that receives gradients must do so from the first step "
                               "(one bias correction per launch)")
        return st

    def _rehome(self, st, keys, views):
        if st:                                   # state from the discovery step(s): move it into the flat buffers
            for k, v in zip(keys, views):
                v.copy_(st[k])
        else:
            st["step"] = torch.tensor(0.0)
        for k, v in zip(keys, views):
            st[k] = v

    # -- step -------------------------------------------------------------------------------------
    def _update(self, lib, scaler, unscaled, clip_ptr):
        """One of the eight ``zsv_adam[w]_multi[_scaled][_avg]`` entry points, picked once per step.  The ``adamw`` forms run when
        anything needs them -- clipping, gradients ``unscale_`` has already rewritten, decay in any group -- and then for every
        group, one with ``weight_decay == 0`` included."""
        decay_clip = self.max_grad_norm is not None or unscaled or any(g["weight_decay"] != 0 for g in self.param_groups)
        scaled, averaged = scaler is not None, self._average is not None
        name = "zsv_adam" + ("w" if decay_clip else "") + "_multi" + ("_scaled" if scaled else "") + ("_avg" if averaged else "")
        entry = getattr(lib, name)

        def launch(group, table, count, chunks):
            b1, b2 = group["betas"]
            args = [table.data_ptr(), count, chunks, float(group["lr"]), float(b1), float(b2), float(group["eps"])]
            if decay_clip:
                wd = float(group["weight_decay"])
                self._check_decay(wd)
                args += [wd, int(bool(group["decoupled_weight_decay"])), clip_ptr]
            if scaled:                                 # the step number is the scaler's device-resident count
                args += [scaler.state_ptr, int(unscaled)] if decay_clip else [scaler.state_ptr]
            else:
                args += [self._host_steps + 1]
            if averaged:
                args += self._avg_args(table, count)
            _lib.check(entry(*args, _stream()), name)
        return launch

    def _after_step(self, scaler):
        if scaler is None:
            self._host_steps += 1
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None:
                        self.state[p]["step"] += 1

    def _on_adopt(self, scaler: LossScaler) -> None:
        if self._host_steps:
            if not self._resumed:
                raise RuntimeError("FusedAdam: a LossScaler must drive the optimizer from its first step "
                                   "(the count of steps taken lives in the scaler's device state)")
            # resumed from a checkpoint (load_state_dict): the scaler takes over the loaded step count unless its own
            # loaded state already carries one
            if scaler.state()["steps_done"] == 0:
                scaler._seed_steps_done(self._host_steps)
            elif scaler.state()["steps_done"] != self._host_steps:
                raise RuntimeError("FusedAdam: the loaded optimizer and scaler states disagree on the steps taken")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:            # a state dict saved before these options existed: the defaults
            group.setdefault("weight_decay", 0.0)
            group.setdefault("decoupled_weight_decay", False)
            self._check_decay(group["weight_decay"])
        steps = [int(st["step"].item()) for st in self.state.values() if "step" in st]
        if steps and min(steps) != max(steps):
            raise RuntimeError("FusedAdam: the loaded per-parameter step counts differ")
        self._host_steps = steps[0] if steps else 0
        self._resumed = True
        self._scaler = None
        for st in self.state.values():
            if "step" in st:
                st["step"] = st["step"].detach().to("cpu", torch.float32)
        self._static = None                        # the moments are re-homed into the flat buffers on the next step

    def state_dict(self):
        """With a ``LossScaler`` the number of steps actually taken is device state: fetched here (one sync)."""
        if self._scaler is not None:
            done = float(self._scaler.state()["steps_done"])
            for st in self.state.values():
                if "step" in st:
                    st["step"].fill_(done)
        return super().state_dict()


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD`` -- momentum, dampening, Nesterov, L2 weight decay, ``maximize`` -- in one ``zsv_sgd_multi`` launch per
    parameter group (csrc/sgd.hip), with everything ``FusedAdam`` carries: ``max_grad_norm``, ``grad_buckets=``, ``LossScaler`` and
    ``WeightAverage``.  Every option is per parameter group except ``max_grad_norm`` and ``grad_buckets``.

    The state is torch's: ``state[p]["momentum_buffer"]`` (none with ``momentum == 0``), so ``state_dict()`` /
    ``load_state_dict()`` interchange with ``torch.optim.SGD``.  torch creates the buffer on the first step as a copy of the
    gradient; here it is allocated as zeros and the launch is told whether it is the first one, which matters only with
    ``dampening != 0`` (``momentum * 0 + g`` is ``g``).  Without a scaler the host knows; under a ``LossScaler`` the device
    decides from the scaler's count of steps taken, so a first step that is skipped leaves the next one the first.  One flag per
    launch: a parameter that first receives a gradient after the first step is fine with ``dampening == 0`` and raises
    otherwise."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 max_grad_norm=None, grad_buckets=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        max_grad_norm = self._check_max_grad_norm(max_grad_norm)
        self._setup(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                                 maximize=bool(maximize)), max_grad_norm, grad_buckets)

    def _reset_rule_state(self):
        self._started = False                             # an update has been launched, or buffers were loaded: no host-side "first"
        self._first_at = -1                               # under a scaler: the launch is the first iff steps_done == this (-1: never)

    @staticmethod
    def _check_group(group):
        lr, momentum, dampening, wd = group["lr"], group["momentum"], group["dampening"], group["weight_decay"]
        if not (math.isfinite(lr) and lr >= 0):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not (math.isfinite(momentum) and momentum >= 0):
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not (math.isfinite(wd) and wd >= 0):
            raise ValueError(f"Invalid weight_decay value: {wd}")
        if not math.isfinite(dampening):
            raise ValueError(f"Invalid dampening value: {dampening}")
        if group["nesterov"] and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    @staticmethod
    def _needs_first(group) -> bool:
        return group["momentum"] != 0 and group["dampening"] != 0

    # -- descriptor tables ------------------------------------------------------------------------
    def _state_keys(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _entry_state(self, p, group):
        st = self.state[p]
        if group["momentum"] != 0 and st.get("momentum_buffer") is None:
            if self._started and self._needs_first(group):
                raise RuntimeError("FusedSGD: with dampening != 0 every parameter that receives gradients must do so from the first "
                                   "step (one 'the momentum buffer does not exist yet' flag per launch)")
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _rehome(self, st, keys, views):
        for k, v in zip(keys, views):
            if st.get(k) is not None:            # a buffer from the discovery step(s) or a checkpoint: move it into the flat one
                v.copy_(st[k])
            elif self._started and self._needs_first(self.param_groups[0]):
                raise RuntimeError("FusedSGD: with dampening != 0 every parameter that receives gradients must do so from the first "
                                   "step (one 'the momentum buffer does not exist yet' flag per launch)")
            st[k] = v

    def _on_adopt(self, scaler: LossScaler) -> None:
        # the device decides "first" from the scaler's count of steps taken: remember what it reads now, while no buffer exists
        # (one sync, and only for an update rule that can tell a first step from a zero buffer)
        if not self._started and any(self._needs_first(g) for g in self.param_groups):
            self._first_at = scaler.state()["steps_done"]
        else:
            self._first_at = -1

    # -- step -------------------------------------------------------------------------------------
    def _check_groups(self):
        for group in self.param_groups:
            self._check_group(group)

    def _step_flags(self, scaler):
        """``(state_ptr, first_step)`` of this step's launches: the scaler's device state, or None, and the count of steps taken
        at which a launch is the first (class docstring) -- the host's own answer, 0 or -1, without a scaler."""
        if scaler is not None:
            return scaler.state_ptr, self._first_at
        return None, -1 if self._started else 0

    def _update(self, lib, scaler, unscaled, clip_ptr):
        state_ptr, first_step = self._step_flags(scaler)

        def launch(group, table, count, chunks):
            shadows, avg_state, ema_weight = self._avg_args(table, count)
            _lib.check(lib.zsv_sgd_multi(table.data_ptr(), count, chunks, float(group["lr"]), float(group["momentum"]),
                                         float(group["dampening"]), int(bool(group["nesterov"])), float(group["weight_decay"]),
                                         int(bool(group["maximize"])), clip_ptr, state_ptr, int(unscaled), first_step,
                                         shadows, avg_state, ema_weight, _stream()), "zsv_sgd_multi")
        return launch

    def _after_step(self, scaler):
        self._started = True

    # -- state ------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:            # torch.optim.SGD's groups carry more keys (foreach, fused, ...): they are kept
            group.setdefault("nesterov", False)
            group.setdefault("maximize", False)
            self._check_group(group)
        for st in self.state.values():
            if st.get("momentum_buffer", 0) is None:       # torch stores None with momentum == 0
                del st["momentum_buffer"]
        # a loaded state that has buffers is past its first step
        self._started = any(st.get("momentum_buffer") is not None for st in self.state.values())
        self._first_at = -1
        self._scaler = None
        self._static = None                        # the buffers are re-homed into the flat ones on the next step

    def state_dict(self):
        """torch.optim.SGD's layout.  Under a ``LossScaler`` whether the first step has been taken is device state: fetched here
        (one sync) when it matters, and buffers that no taken step has written are left out, as torch has none then."""
        out = super().state_dict()
        if self._scaler is not None and self._first_at >= 0 and self._scaler.state()["steps_done"] == self._first_at:
            out["state"] = {k: {n: v for n, v in st.items() if n != "momentum_buffer"} for k, st in out["state"].items()}
        return out


class _Layerwise:
    """What ``FusedLARS`` and ``FusedLAMB`` add to the rule they inherit: one workspace for all parameter groups of a step -- a
    record ``{p_norm, q_norm, ratio}`` per tensor, then two partial sums per 4096-element chunk (``zsv_layerwise_workspace_bytes``)
    -- each table's place in it, and ``layer_norms`` / ``layer_params``.  Listed before the inherited optimizer in the bases."""

    _layer_keys = ()                                      # the group options a state dict of the inherited optimizer lacks

    def _reset_rule_state(self):
        super()._reset_rule_state()                       # the fields of the inherited rule
        self._layer_ws = None                             # fp32 view of the workspace (records first)
        self._layout = ({}, 0, 0)                         # {id(group): (tensor offset, chunk offset)}, tensors, chunks of this step
        self.layer_params = []                            # the parameters behind the rows of layer_norms, in order

    @property
    def layer_norms(self) -> torch.Tensor:
        """``(len(layer_params), 3)`` device tensor of the last step's records: the 2-norm of each parameter before the update, the
        2-norm of its gradient (LARS: unscaled and clipped) or of its update direction ``u`` (LAMB), and the trust ratio applied.
        A view of the workspace: reading it does not synchronise, and a step the scaler skips leaves it as it was."""
        if self._layer_ws is None or not self.layer_params:
            raise RuntimeError(f"{type(self).__name__}.layer_norms is available after step()")
        n = len(self.layer_params)
        return self._layer_ws[:3 * n].view(n, 3)

    def _tables(self):
        work = super()._tables()
        offsets, params, tensors, chunks_before = {}, [], 0, 0
        for group, (table, count, chunks, _keep) in work:
            offsets[id(group)] = (tensors, chunks_before)
            if self._static is not None and table is self._static[1]:
                params += [p for p, _ in self._static[4]]                     # the bucket layout's order
            else:
                params += [p for p in group["params"] if p.grad is not None]  # _dynamic_table's order
            tensors += count
            chunks_before += chunks
        assert len(params) == tensors
        self._layout, self.layer_params = (offsets, tensors, chunks_before), params
        return work

    def _place(self, lib, group, table, count, chunks):
        """The leading arguments of the three workspace launches of one table, and the address of its first record."""
        offsets, tensors, all_chunks = self._layout
        nbytes = int(lib.zsv_layerwise_workspace_bytes(all_chunks, tensors))
        ws = self._layer_ws
        if ws is None or ws.device != table.device or ws.numel() * 4 < nbytes:
            ws = self._layer_ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=table.device)
        first, chunk_offset = offsets[id(group)]
        return (table.data_ptr(), count, chunks, chunk_offset, first, tensors, ws.data_ptr(), ws.numel() * 4), ws.data_ptr() + 12 * first

    def load_state_dict(self, state_dict):
        mine = [dict(g) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, own in zip(self.param_groups, mine):   # a state dict of the inherited optimizer: these options stay as built
            for k in self._layer_keys:
                group.setdefault(k, own[k])
        self._check_groups()


class FusedLARS(_Layerwise, FusedSGD):
    """LARS (You, Gitman, Ginsburg 2017): ``FusedSGD``'s rule with the update of every parameter TENSOR scaled by a trust ratio,

        r   = trust_coefficient * |p| / (|g| + weight_decay * |p| + eps)     if adapt and |p| > 0 and |g| > 0, else 1
        d   = r * (g + weight_decay * p)
        buf = d on the first step taken, else momentum * buf + (1 - dampening) * d
        p  <- p - lr * (d + momentum * buf if nesterov else buf)

    the norms 2-norms over one tensor, ``g`` unscaled and clipped as in ``FusedSGD``.  Three launches per parameter group and no
    host synchronisation (csrc/layerwise.hip): partial sums per chunk, one workgroup per tensor that leaves ``{|p|, |g|, r}``
    on the device, the update.  ``adapt`` is a group option (default True): a group with ``adapt=False`` -- BatchNorm affines and
    biases, ``layerwise_groups`` -- takes ``r = 1``, which is ``torch.optim.SGD`` and ``FusedSGD`` bit for bit.  State, the
    first-step rule, ``max_grad_norm``, ``grad_buckets=``, ``LossScaler`` and ``WeightAverage`` are ``FusedSGD``'s;
    ``layer_norms`` is the per-layer monitor."""

    _layer_keys = ("adapt", "trust_coefficient", "eps")

    def __init__(self, params, lr, momentum=0.9, dampening=0, nesterov=False, weight_decay=1e-4, trust_coefficient=1e-3, eps=1e-8,
                 maximize=False, max_grad_norm=None, grad_buckets=None):
        max_grad_norm = self._check_max_grad_norm(max_grad_norm)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                        maximize=bool(maximize), trust_coefficient=trust_coefficient, eps=eps, adapt=True)
        self._check_group(defaults)
        self._setup(params, defaults, max_grad_norm, grad_buckets)

    @staticmethod
    def _check_group(group):
        FusedSGD._check_group(group)
        tc, eps = group.get("trust_coefficient", 1e-3), group.get("eps", 1e-8)
        if not (math.isfinite(tc) and tc > 0):
            raise ValueError(f"Invalid trust_coefficient value: {tc}")
        if not (math.isfinite(eps) and eps >= 0):
            raise ValueError(f"Invalid eps value: {eps}")

    def _update(self, lib, scaler, unscaled, clip_ptr):
        state_ptr, first_step = self._step_flags(scaler)

        def launch(group, table, count, chunks):
            place, records = self._place(lib, group, table, count, chunks)
            wd = float(group["weight_decay"])
            _lib.check(lib.zsv_lars_norms(*place, state_ptr, _stream()), "zsv_lars_norms")
            _lib.check(lib.zsv_layerwise_finalize(*place, 0, int(bool(group["adapt"])), float(group["trust_coefficient"]), wd,
                                                  float(group["eps"]), 0.0, clip_ptr, state_ptr, int(unscaled), _stream()),
                       "zsv_layerwise_finalize")
            shadows, avg_state, ema_weight = self._avg_args(table, count)
            _lib.check(lib.zsv_lars_multi(table.data_ptr(), count, chunks, records, float(group["lr"]), float(group["momentum"]),
                                          float(group["dampening"]), int(bool(group["nesterov"])), wd, int(bool(group["maximize"])),
                                          clip_ptr, state_ptr, int(unscaled), first_step, shadows, avg_state, ema_weight, _stream()),
                       "zsv_lars_multi")
        return launch


class FusedLAMB(_Layerwise, FusedAdam):
    """LAMB (You et al. 2020): Adam's moments, decoupled weight decay inside the update direction, and a trust ratio per TENSOR,

        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  t = steps taken + 1 (the scaler's device-resident count under one)
        u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay * p
        r = |p| / |u|   if adapt and |p| > 0 and |u| > 0, else 1;   r = min(r, trust_clip) when trust_clip is set
        p <- p - lr * r * u

    Three launches per parameter group and no host synchronisation (csrc/layerwise.hip): the first updates ``m`` and ``v`` and
    sums ``p^2`` and ``u^2`` per chunk, the second leaves ``{|p|, |u|, r}`` per tensor on the device, the third recomputes ``u``
    from the new moments and the old parameter -- ``u`` is never stored, ``.grad`` never rewritten.  ``adapt`` and ``trust_clip``
    are group options.  The state is ``FusedAdam``'s (``step`` / ``exp_avg`` / ``exp_avg_sq``; a ``FusedAdam`` state dict loads),
    and so are ``max_grad_norm``, ``grad_buckets=``, ``LossScaler`` and ``WeightAverage``; ``layer_norms`` is the per-layer
    monitor."""

    _layer_keys = ("adapt", "trust_clip")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, trust_clip=None, max_grad_norm=None,
                 grad_buckets=None):
        max_grad_norm = self._check_max_grad_norm(max_grad_norm)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, trust_clip=trust_clip, adapt=True)
        self._check_group(defaults)
        self._setup(params, defaults, max_grad_norm, grad_buckets)

    @classmethod
    def _check_group(cls, group):
        lr, eps, (b1, b2), clip = group["lr"], group["eps"], group["betas"], group.get("trust_clip")
        if not (math.isfinite(lr) and lr >= 0):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not (math.isfinite(eps) and eps >= 0):
            raise ValueError(f"Invalid eps value: {eps}")
        if not (0 <= b1 < 1) or not (0 <= b2 < 1):
            raise ValueError(f"Invalid betas: {(b1, b2)}")
        cls._check_decay(group["weight_decay"])
        if clip is not None and not (isinstance(clip, (int, float)) and math.isfinite(clip) and clip > 0):
            raise ValueError(f"trust_clip must be a finite positive number or None, not {clip}")

    def _check_groups(self):
        for group in self.param_groups:
            self._check_group(group)

    def _update(self, lib, scaler, unscaled, clip_ptr):
        state_ptr = scaler.state_ptr if scaler is not None else None
        step = 0 if scaler is not None else self._host_steps + 1      # under a scaler the device counts

        def launch(group, table, count, chunks):
            place, records = self._place(lib, group, table, count, chunks)
            b1, b2 = group["betas"]
            eps, wd = float(group["eps"]), float(group["weight_decay"])
            _lib.check(lib.zsv_lamb_moments(*place, float(b1), float(b2), eps, wd, clip_ptr, state_ptr, int(unscaled), step, _stream()),
                       "zsv_lamb_moments")
            _lib.check(lib.zsv_layerwise_finalize(*place, 1, int(bool(group["adapt"])), 0.0, 0.0, 0.0,
                                                  float(group["trust_clip"] or 0.0), None, state_ptr, int(unscaled), _stream()),
                       "zsv_layerwise_finalize")
            shadows, avg_state, ema_weight = self._avg_args(table, count)
            _lib.check(lib.zsv_lamb_multi(table.data_ptr(), count, chunks, records, float(group["lr"]), float(b1), float(b2), eps, wd,
                                          state_ptr, step, shadows, avg_state, ema_weight, _stream()), "zsv_lamb_multi")
        return launch


def layerwise_groups(model, weight_decay):
    """The two parameter groups LARS and LAMB are usually run with: every trainable parameter with ``dim() >= 2`` (convolution
    and linear weights) adapts and decays; the rest (BatchNorm affines, biases) takes ``adapt=False`` and no decay."""
    own = getattr(model, "module", model)
    params = [p for p in own.parameters() if p.requires_grad]
    return [dict(params=[p for p in params if p.dim() >= 2], adapt=True, weight_decay=weight_decay),
            dict(params=[p for p in params if p.dim() < 2], adapt=False, weight_decay=0.0)]


class WeightAverage:
    """A running average of the weights for evaluation, kept by the optimizer's own launches.

    ``decay`` in ``[0, 1)`` is an exponential moving average (``torch.optim.swa_utils.AveragedModel`` with
    ``get_ema_multi_avg_fn(decay)``); ``decay=None`` the equal-weight running mean of SWA (``AveragedModel``'s default).  Every
    parameter of the optimizer's groups gets a shadow, a view of ONE flat fp32 buffer per device initialised to the parameters;
    from then on each ``optimizer.step()`` -- directly, through ``LossScaler.step`` or inside ``train.train_step`` -- averages
    once: the first averaged step copies, later ones lerp, a step the scaler skips changes nothing (all decided on the device:
    ``n_averaged`` is a device counter, and reading it is the only thing here that synchronises).  A parameter that never
    receives a gradient keeps ``avg == p``.

    With ``model=`` the shadows are named like ``model.state_dict()``, and with ``buffers=True`` the model's floating-point
    buffers (BatchNorm ``running_mean`` / ``running_var``) are averaged as well, in one more launch per step
    (``zsv_avg_multi``).  Integer buffers (``num_batches_tracked``) are NOT shadowed and keep their live value under
    ``applied()`` -- ``AveragedModel(use_buffers=True)`` lerps them with truncation.

    ``applied()`` exchanges live and averaged values in place (``zsv_swap_multi``): no address changes, so cached weight panels,
    inference engines and captured graphs stay valid and only rebuild their contents.  Data parallel: every rank applies the
    same update to equal parameters, so the shadows are equal without a collective."""

    def __init__(self, optimizer, decay: Optional[float] = 0.999, model: Optional[torch.nn.Module] = None, buffers: bool = True):
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("WeightAverage averages inside optim.FusedAdam's update launch; got " + type(optimizer).__name__
                            + " (it takes an optim.FusedAdam, FusedSGD, FusedLARS or FusedLAMB)")
        if decay is not None:
            if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= decay < 1.0):
                raise ValueError(f"decay must be None (equal-weight) or a number in [0, 1), not {decay!r}")
        if optimizer._average is not None:
            raise RuntimeError(f"this {type(optimizer).__name__} already has a WeightAverage (one per optimizer)")
        self._set_decay(decay)
        self._applied = False
        own = getattr(model, "module", model) if model is not None else None
        params = [p for group in optimizer.param_groups for p in group["params"]]
        if own is not None:
            names = {id(p): k for k, p in own.named_parameters()}
            missing = [i for i, p in enumerate(params) if id(p) not in names]
            if missing:
                raise ValueError(f"WeightAverage: optimizer parameters {missing} are not parameters of `model`")
            keys = [names[id(p)] for p in params]
        else:
            keys = list(range(len(params)))
        for p in params:
            optimizer._check_param(p)
        live = list(zip(keys, params))
        self._n_params = len(live)
        if own is not None and buffers:
            for k, b in own.named_buffers():
                if not b.is_floating_point():
                    continue                                # num_batches_tracked: stays live (class docstring)
                if not b.is_cuda or b.dtype != torch.float32 or not b.is_contiguous():
                    raise RuntimeError(f"WeightAverage: buffer {k} must be a contiguous fp32 tensor on a HIP device")
                live.append((k, b))
        # one flat buffer and one zsv_avg_state {int32 n_averaged} per device; entries: (key, live tensor, shadow view)
        totals = {}
        for _, t in live:
            totals[t.device] = totals.get(t.device, 0) + t.numel()
        self._flat = {dev: torch.empty(n, dtype=torch.float32, device=dev) for dev, n in totals.items()}
        self._state = {dev: torch.zeros(1, dtype=torch.int32, device=dev) for dev in totals}
        self._entries, offsets = [], {dev: 0 for dev in totals}
        with torch.no_grad():
            for k, t in live:
                off, n = offsets[t.device], t.numel()
                shadow = self._flat[t.device][off:off + n].view_as(t)
                shadow.copy_(t.detach())
                offsets[t.device] = off + n
                self._entries.append((k, t, shadow))
        self._shadow_of = {id(t): shadow for _, t, shadow in self._entries}
        self._pair_tables = {}                              # (device, buffers only?) -> (live pointers, table, count, chunks)
        self.optimizer = optimizer
        optimizer._average = self
        optimizer._static = None                            # the bucket table is rebuilt with the shadow pointers behind it

    def _set_decay(self, decay) -> None:
        self.decay = None if decay is None else float(decay)
        # zsv_* ema_weight: (float)(1 - decay) -- the double is rounded once, by the call -- or negative for equal-weight
        self._ema_weight = -1.0 if decay is None else 1.0 - self.decay

    @property
    def n_averaged(self) -> torch.Tensor:
        """Optimizer steps averaged so far, a 0-d int32 device tensor (skipped steps do not count)."""
        return next(iter(self._state.values()))[0]

    def shadows(self) -> dict:
        """``{key: averaged tensor}``: views of the flat buffer(s), keyed like ``state_dict()['shadows']``."""
        return {k: shadow for k, _, shadow in self._entries}

    # -- what the optimizer's step calls ----------------------------------------------------------------
    def _state_ptr(self, dev) -> int:
        return self._state[dev].data_ptr()

    def _shadow_pointers(self, params) -> bytes:
        try:
            return b"".join(struct.pack("<Q", self._shadow_of[id(p)].data_ptr()) for p in params)
        except KeyError:
            raise RuntimeError("WeightAverage: a parameter joined the optimizer after the average was built") from None

    def _check_live(self) -> None:
        if self._applied:
            raise RuntimeError("optimizer.step() inside WeightAverage.applied(): the live tensors hold the averaged values")

    def _pair_table(self, dev, buffers_only: bool):
        """Device table of zsv_pair_tensor {live, shadow, n, first_chunk}; rebuilt only when a live tensor has moved."""
        rows = [(t, shadow) for _, t, shadow in (self._entries[self._n_params:] if buffers_only else self._entries)
                if t.device == dev and t.numel()]
        if not rows:
            return None
        ptrs = tuple(t.data_ptr() for t, _ in rows)
        cached = self._pair_tables.get((dev, buffers_only))
        if cached is None or cached[0] != ptrs:
            for t, shadow in rows:
                if t.device != shadow.device or t.numel() != shadow.numel() or not t.is_contiguous():
                    raise RuntimeError("WeightAverage: a shadowed tensor changed its device, size or layout")
            raw, chunks = pack_rows([(t.data_ptr(), shadow.data_ptr(), t.numel()) for t, shadow in rows])
            cached = (ptrs, torch.frombuffer(raw, dtype=torch.uint8).to(dev), len(rows), chunks)
            self._pair_tables[(dev, buffers_only)] = cached
        return cached[1:]

    def _after_update(self, lib, scaler: Optional[LossScaler]) -> None:
        state_ptr = scaler.state_ptr if scaler is not None else None
        for dev, state in self._state.items():
            with torch.cuda.device(dev):
                built = self._pair_table(dev, True)
                if built is not None:
                    table, count, chunks = built
                    _lib.check(lib.zsv_avg_multi(table.data_ptr(), count, chunks, state.data_ptr(), self._ema_weight, state_ptr,
                                                 _stream()), "zsv_avg_multi")
                _lib.check(lib.zsv_avg_advance(state.data_ptr(), state_ptr, _stream()), "zsv_avg_advance")

    # -- evaluation on the averaged weights ---------------------------------------------------------
    def _swap(self) -> None:
        lib = _lib.load()
        for dev in self._state:
            built = self._pair_table(dev, False)
            if built is None:
                continue
            table, count, chunks = built
            with torch.cuda.device(dev):
                _lib.check(lib.zsv_swap_multi(table.data_ptr(), count, chunks, _stream()), "zsv_swap_multi")
        _lib.note_raw_write()                               # parameters and buffers rewritten through raw pointers

    @contextlib.contextmanager
    def applied(self):
        """Inside the context the live tensors hold the averaged values (and the shadows the live ones); exit restores
        both bit for bit.  Not re-entrant, and ``optimizer.step()`` inside it raises.  Meant for evaluation: a training-mode
        forward inside the context would update the AVERAGED BatchNorm statistics."""
        if self._applied:
            raise RuntimeError("WeightAverage.applied() is already active (it cannot be nested)")
        self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._swap()
            self._applied = False

    # -- state ------------------------------------------------------------------------------------------
    def averaged_state_dict(self, model: torch.nn.Module) -> dict:
        """``model.state_dict()`` (no prefix) with every shadowed tensor replaced by its average; the rest is live."""
        if self._applied:
            raise RuntimeError("WeightAverage.averaged_state_dict() inside applied(): live and averaged values are exchanged")
        own = getattr(model, "module", model)
        return {k: self._shadow_of.get(id(v), v).detach() for k, v in own.state_dict(keep_vars=True).items()}

    def state_dict(self) -> dict:
        """``{"n_averaged", "decay", "shadows"}``; the shadows (host copies) are keyed by ``state_dict`` name when the
        average was built with ``model=``, by position in the optimizer otherwise.  One host sync."""
        if self._applied:
            raise RuntimeError("WeightAverage.state_dict() inside applied(): live and averaged values are exchanged")
        return {"n_averaged": int(self.n_averaged.item()), "decay": self.decay,
                "shadows": {k: shadow.detach().cpu().clone() for k, _, shadow in self._entries}}

    def load_state_dict(self, state: dict) -> None:
        """Resume: the shadows are copied back into the flat buffer(s), the counter is uploaded, ``decay`` is the saved one."""
        if self._applied:
            raise RuntimeError("WeightAverage.load_state_dict() inside applied()")
        decay = state["decay"]
        if decay is not None and not (0.0 <= float(decay) < 1.0):
            raise ValueError(f"decay must be None or a number in [0, 1), not {decay!r}")
        saved = state["shadows"]
        own = [k for k, _, _ in self._entries]
        if set(saved) != set(own):
            raise KeyError(f"WeightAverage.load_state_dict: missing {sorted(set(own) - set(saved), key=str)}, "
                           f"unexpected {sorted(set(saved) - set(own), key=str)}")
        with torch.no_grad():
            for k, _, shadow in self._entries:
                if tuple(saved[k].shape) != tuple(shadow.shape):
                    raise ValueError(f"WeightAverage.load_state_dict: shape of {k!r} is {tuple(saved[k].shape)}, "
                                     f"expected {tuple(shadow.shape)}")
                shadow.copy_(saved[k])
            for st in self._state.values():
                st.fill_(int(state["n_averaged"]))
        self._set_decay(decay)
