"""Data-parallel gradient exchange: one process per GPU, RCCL all-reduce over xGMI.

Replaces the reference's single-process ``nn.DataParallel`` (main.py:61-63,126): instead of
replicating 147 MB of parameters from GPU 0 every forward and reduce-adding gradients back
onto GPU 0, every rank owns a replica, runs its own 22-clip shard (``opt.bs`` is per GPU,
main.py:38,61-63) and the only exchange per step is one averaged all-reduce of the live
gradients (126.9 MB fp32), issued bucket by bucket while backward is still running:

* buckets are filled in the order gradients are actually produced (recorded during the first
  step): MLP head -> layer4 -> ... -> stem, so 74 % of the bytes (layer4) are on the wire
  after ~6 % of the backward FLOPs;
* each bucket is a flat fp32 buffer; when its last gradient lands, an event recorded on the
  autograd stream gates a side HIP stream that packs the bucket, runs ``all_reduce(SUM)``
  (backend "nccl" == RCCL on ROCm), scales by 1/world and unpacks -- backward never waits;
* ``finish_step()`` makes the compute stream wait for the side stream before
  ``optimizer.step()``;
* parameters that never receive a gradient (the reference's unused Transformer encoder,
  ``model.fc``, ... -- SURVEY F5) are discovered in the first step and excluded, so nothing
  waits for them;
* BatchNorm statistics stay per replica by default, as under DataParallel -- right for the reference's 22 clips
  per GPU.  ``convert_sync_batchnorm(model)`` is the opt-in for a few clips per rank (``ir_csn_50``, long clips, large crops)
  and for LARS / LAMB batches, whose statistics are meant to be the global batch's: it swaps every ``layers.BatchNorm3d`` for a
  ``layers.SyncBatchNorm3d`` (same tensors), which in training mode takes mean and variance over all ranks -- the same passes
  over the activations, plus one all_gather of 2C+1 doubles per forward and one all_reduce of 2C doubles per backward and layer.
  fp32 path only (``amp.autocast()`` refuses such a trunk); with ``train_step(micro_batches=k)`` each micro-batch synchronises
  across ranks on its own.  Measured on one device without the collectives (profiles/sync_bn.json); RCCL at world > 1 has
  not run here, so the cost of the collectives is not measured.

After ``finish_step()`` every live parameter's ``.grad`` IS a view of its bucket (the averaged values are not
copied back), so ``optim.FusedAdam(..., grad_buckets=sync)`` walks the all-reduce buffers themselves with a
descriptor table built once, and ``torch.optim.Adam`` sees ordinary ``.grad`` tensors.
``GradientSync(model, local=True)`` keeps the bucketing without any collective (one process, one GPU).

Gradient accumulation: ``begin_step(passes=k)`` declares k backward passes (micro-batches) per optimizer step; ``end_pass()``
closes each but the last, ``finish_step()`` the last (``train.train_step(micro_batches=k)`` drives all of it).  The bucket is the
accumulator: when a bucket completes in pass j the side stream folds the fresh gradients into it with ONE
``zsv_grad_accum_multi`` launch (csrc/optim.hip; ``acc = scale * g`` in the first pass, so the bucket is never zero-filled,
``acc += scale * g`` after it; scale = 1/world), ``end_pass()`` drops ``.grad`` of the live parameters so the next backward
hands over fresh tensors, the all-reduce runs once per optimizer step (in pass k), ``.grad`` become the bucket views in
``finish_step()`` as always and ``FusedAdam``'s table stays static.  k micro-batches of 22 followed by one step is what
DataParallel computes over k replicas (each with its own BatchNorm batch statistics); the running statistics are updated k
times, as torch does under accumulation.  If the very first step has k > 1, the live set and the bucket layout are fixed at the
end of its first pass.  CPU tensors (gloo) accumulate with ``_foreach_copy_`` / ``_foreach_add_``.  ``passes=1`` is the path
described above, unchanged.

With equal shards, the mean over ranks of per-rank mean-MSE gradients equals the full-batch
mean-MSE gradient DataParallel computes.  Works on CPU tensors with the gloo backend (tests).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import weakref
from ctypes import c_void_p

import torch
import torch.distributed as dist

from . import _lib
from ._tables import PinnedRing, chunks as _chunks, pack_rows

DEFAULT_BUCKET_BYTES = 25 * 1024 * 1024


@torch.no_grad()
def broadcast_tensors(tensors, src: int = 0, group=None) -> int:
    """Every rank takes rank ``src``'s values of ``tensors`` (parameters, buffers): ONE collective per dtype over a flat
    staging buffer instead of one per tensor (R(2+1)D-18: 304 tensors -> 2 broadcasts).  Returns the number of collectives.
    The source rank's tensors are not written."""
    by_dtype: Dict[torch.dtype, List[torch.Tensor]] = {}
    for t in tensors:
        by_dtype.setdefault(t.dtype, []).append(t.data)
    rank = dist.get_rank()
    calls = 0
    for dtype, group_tensors in by_dtype.items():
        flat = torch.cat([t.reshape(-1) for t in group_tensors])
        dist.broadcast(flat, src=src, group=group)
        calls += 1
        if rank != src:
            off = 0
            for t in group_tensors:
                n = t.numel()
                t.copy_(flat[off:off + n].view_as(t))
                off += n
    return calls


def convert_sync_batchnorm(model: torch.nn.Module, process_group=None) -> torch.nn.Module:
    """``torch.nn.SyncBatchNorm.convert_sync_batchnorm`` for this package: every ``layers.BatchNorm3d`` in ``model`` becomes a
    ``layers.SyncBatchNorm3d`` over ``process_group`` (default: the world), in place, holding the SAME Parameter and buffer
    objects -- an optimizer or a ``GradientSync`` built earlier stays valid and ``state_dict`` keys do not change; the train /
    eval mode of each layer is kept (hooks are not, as with torch's converter).  Layers that already are ``SyncBatchNorm3d``
    are left alone: a second call is a no-op.  Returns ``model`` (a lone ``BatchNorm3d`` comes back as its replacement).
    torch's own converter would hand the layers to ATen and lose the one-pass BN + residual + ReLU kernels."""
    from .layers import BatchNorm3d, SyncBatchNorm3d

    def converted(bn):
        new = SyncBatchNorm3d(bn.num_features, bn.eps, bn.momentum, bn.affine, bn.track_running_stats, process_group,
                              device="meta")
        new._parameters, new._buffers = bn._parameters, bn._buffers      # the same Parameter / buffer objects, not copies
        new.training = bn.training
        return new

    def plain(m):
        return isinstance(m, BatchNorm3d) and not isinstance(m, SyncBatchNorm3d)

    if plain(model):
        return converted(model)
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if plain(child):
                setattr(parent, name, converted(child))
    return model


class _Bucket:
    def __init__(self, params: List[torch.nn.Parameter]):
        self.params = params
        self.numel = sum(p.numel() for p in params)
        p0 = params[0]
        self.flat = torch.empty(self.numel, dtype=p0.dtype, device=p0.device)
        self.views = []
        off = 0
        for p in params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.pending = len(params)
        self.work = None
        # static half of the zsv_grad_accum_multi table: (index, accumulator slice address, n) per non-empty parameter
        self.slices = [(i, v.data_ptr(), v.numel()) for i, v in enumerate(self.views) if v.numel()] if self.flat.is_cuda else []
        self.chunks = sum(_chunks(n) for _, _, n in self.slices)


class GradientSync:
    """Bucketed, backward-overlapped gradient averaging for one model replica."""

    def __init__(self, model: torch.nn.Module, process_group=None, bucket_bytes: int = DEFAULT_BUCKET_BYTES,
                 broadcast_initial_state: bool = True, local: bool = False):
        self.local = bool(local)
        if not self.local and not dist.is_initialized():
            raise RuntimeError("torch.distributed is not initialised (one process per GPU; init_process_group first)")
        self.group = process_group
        self.world = 1 if self.local else dist.get_world_size(process_group)
        self.layout_version = 0                  # bumped whenever the buckets are (re)built
        self.model = model
        self.bucket_bytes = int(bucket_bytes)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self._index: Dict[int, int] = {id(p): i for i, p in enumerate(self.params)}
        self._arrival: List[int] = []          # parameter indices in the order their grads landed
        self._buckets: Optional[List[_Bucket]] = None
        self._bucket_of: Dict[int, _Bucket] = {}
        self._in_step = False
        self._passes = 1                         # backward passes of the current step (begin_step(passes=))
        self._pass = 0                           # index of the pass in flight
        self._cuda = any(p.is_cuda for p in self.params)
        self._side = torch.cuda.Stream() if self._cuda else None
        self._ring = PinnedRing(8)               # accumulate tables: one upload per bucket and pass
        # (ops._dw_read_early: a post-accumulate hook normally reads `.grad` on the backward stream, so the weight-gradient side
        # stream is joined before it runs; THIS hook joins that stream itself in `_launch`, and says so to keep the overlap)
        owner = weakref.ref(self)

        def on_grad(p):
            me = owner()
            if me is not None:
                me._on_grad(p)
        on_grad._zsv_joins_wgrad = True
        self._hooks = [p.register_post_accumulate_grad_hook(on_grad) for p in self.params]
        self.bytes_reduced_last_step = 0
        if broadcast_initial_state and self.world > 1:
            self.broadcast_state()

    # -- setup ---------------------------------------------------------------------------
    @torch.no_grad()
    def broadcast_state(self, src: int = 0) -> None:
        """Every replica starts from rank ``src``'s parameters and buffers (``src``: a global rank)."""
        broadcast_tensors(list(self.model.parameters()) + list(self.model.buffers()), src, self.group)
        if dist.get_rank() != src:
            _lib.note_raw_write()                  # `.data` writes do not bump the version counters

    def _build_buckets(self, order: List[int]) -> None:
        buckets, cur, cur_bytes = [], [], 0
        for idx in order:
            p = self.params[idx]
            nbytes = p.numel() * p.element_size()
            if cur and cur_bytes + nbytes > self.bucket_bytes:
                buckets.append(_Bucket(cur))
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += nbytes
        if cur:
            buckets.append(_Bucket(cur))
        self._buckets = buckets
        self._bucket_of = {id(p): b for b in buckets for p in b.params}
        self.layout_version += 1

    @property
    def ready(self) -> bool:
        """True once the discovery step has fixed the live set and the bucket layout."""
        return self._buckets is not None

    def bucket_layout(self):
        """``[(flat buffer, [(parameter, element offset), ...]), ...]`` in production order."""
        out = []
        for b in self._buckets or []:
            off, rows = 0, []
            for p in b.params:
                rows.append((p, off))
                off += p.numel()
            out.append((b.flat, rows))
        return out

    @property
    def live_parameter_count(self) -> int:
        return 0 if self._buckets is None else sum(len(b.params) for b in self._buckets)

    @property
    def bucket_sizes(self) -> List[int]:
        return [] if self._buckets is None else [b.numel for b in self._buckets]

    # -- per step ------------------------------------------------------------------------
    def begin_step(self, passes: int = 1) -> None:
        """``passes``: the number of backward passes (micro-batches) whose gradients this optimizer step sums; each but the
        last is closed with ``end_pass()``, the last with ``finish_step()``."""
        if isinstance(passes, bool) or not isinstance(passes, int) or passes < 1:
            raise ValueError(f"begin_step: passes must be an integer >= 1, not {passes!r}")
        self._passes, self._pass = passes, 0
        self._in_step = True
        self._arrival = []
        self.bytes_reduced_last_step = 0
        if self._buckets is not None:
            for b in self._buckets:
                b.pending = len(b.params)
                b.work = None

    def _on_grad(self, p: torch.nn.Parameter) -> None:
        if not self._in_step:
            return
        if self._buckets is None:                  # discovery step: just record the order
            self._arrival.append(self._index[id(p)])
            return
        b = self._bucket_of.get(id(p))
        if b is None:
            raise RuntimeError("a parameter that produced no gradient in the first step produced one now; "
                               "rebuild GradientSync (the live set is fixed after discovery)")
        if b.pending <= 0:
            raise RuntimeError("a gradient arrived for a bucket that was already complete in this pass: a second backward "
                               "pass must be declared (begin_step(passes=k) with end_pass() between the passes; "
                               "train_step(micro_batches=k))")
        b.pending -= 1
        if b.pending == 0:
            self._launch(b)

    @torch.no_grad()
    def _launch(self, b: _Bucket) -> None:
        """Pack the bucket's gradients into its flat buffer, sum over ranks, scale by 1/world -- on the side
        stream.  Nothing is copied back: ``finish_step`` points each ``.grad`` at its slice of the buffer.
        In a step of several passes the bucket is the accumulator (``_accumulate``) and only the last pass exchanges it."""
        grads = [p.grad for p in b.params]
        scale = 1.0 / self.world
        if self._passes > 1:
            self._launch_pass(b, grads, scale)
            return
        if self._cuda:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            self._side.wait_event(ready)
            from . import ops
            ops.join_wgrad_streams(self._side)        # weight gradients may come from their own side stream
            with torch.cuda.stream(self._side):
                torch._foreach_copy_(b.views, grads)
                if self.world > 1:
                    b.work = dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                    b.work.wait()                 # orders the side stream after RCCL; host does not block
                    b.flat.mul_(scale)
                for g in grads:                   # the side stream reads memory owned by the autograd stream
                    g.record_stream(self._side)
        else:
            torch._foreach_copy_(b.views, grads)
            if self.world > 1:
                dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group)
                b.flat.mul_(scale)
        self.bytes_reduced_last_step += b.numel * b.flat.element_size()

    def _launch_pass(self, b: _Bucket, grads, scale: float) -> None:
        """Pass j of k > 1: bucket (+)= this pass's gradients; the collective runs in pass k only.  On HIP tensors 1/world
        goes into every pass as the kernel's ``scale`` (no ``mul_`` pass over the bucket after the all-reduce); CPU tensors
        (gloo) keep ``mul_``."""
        first, last = self._pass == 0, self._pass == self._passes - 1
        if self._cuda:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            self._side.wait_event(ready)
            from . import ops
            ops.join_wgrad_streams(self._side)
            with torch.cuda.stream(self._side):
                self._accumulate(b, grads, scale, first)
                if last and self.world > 1:
                    b.work = dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                    b.work.wait()
                for g in grads:
                    g.record_stream(self._side)
        else:
            if first:
                torch._foreach_copy_(b.views, grads)
            else:
                torch._foreach_add_(b.views, grads)
            if last and self.world > 1:
                dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group)
                b.flat.mul_(scale)
        if last:
            self.bytes_reduced_last_step += b.numel * b.flat.element_size()

    def _accumulate(self, b: _Bucket, grads, scale: float, assign: bool) -> None:
        """One ``zsv_grad_accum_multi`` launch on the current (side) stream: every slice of the bucket = [itself +] scale * its
        gradient.  The gradients are fresh allocations every pass, so the table is built and uploaded per launch."""
        dev = b.flat.device
        rows, keep = [], []
        for i, acc, n in b.slices:
            g = grads[i]
            if g is None or not g.is_cuda or g.dtype != torch.float32 or b.flat.dtype != torch.float32 or g.numel() != n:
                raise RuntimeError("GradientSync: gradient accumulation needs dense fp32 gradients on the HIP device "
                                   "(no fallback)")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            rows.append((acc, g.data_ptr(), n))
        if not rows:
            return
        raw, chunks = pack_rows(rows)
        with torch.cuda.device(dev):
            table = self._ring.upload(raw, dev)
            _lib.check(_lib.load().zsv_grad_accum_multi(table.data_ptr(), len(rows), chunks, float(scale), int(bool(assign)),
                                                        c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "zsv_grad_accum_multi")
        del keep, table                            # allocated on this stream: reused only behind the launch

    def end_pass(self) -> None:
        """Call after every backward pass of a ``begin_step(passes=k)`` step except the last (after
        ``ops.join_wgrad_streams()``).  Checks that the pass produced every live gradient, drops ``.grad`` of the live
        parameters (the next backward hands over fresh gradients instead of adding into the old ones) and re-arms the
        buckets.  If this is the very first pass, it fixes the live set and the bucket layout."""
        if not self._in_step:
            raise RuntimeError("end_pass() without begin_step()")
        if self._pass >= self._passes - 1:
            raise RuntimeError(f"end_pass() after the last of the {self._passes} declared passes: call finish_step() "
                               "(or declare more with begin_step(passes=k) / train_step(micro_batches=k))")
        self._close_pass()
        for b in self._buckets:
            for p in b.params:
                p.grad = None
            b.pending = len(b.params)
        self._pass += 1

    def finish_step(self) -> None:
        """Call after ``loss.backward()`` and before ``optimizer.step()``."""
        if not self._in_step:
            raise RuntimeError("finish_step() without begin_step()")
        if self._pass != self._passes - 1:
            raise RuntimeError(f"finish_step() after {self._pass + 1} of the {self._passes} backward passes declared with "
                               "begin_step(passes=k) / train_step(micro_batches=k)")
        self._in_step = False
        self._close_pass()
        self._adopt_bucket_views()

    def _close_pass(self) -> None:
        if self._buckets is None:
            # first pass ever: the live set and the production order are now known.  Ranks must agree
            # on them (same model, same graph) -- checked cheaply through the count.
            order = list(self._arrival)
            if self.local:
                self._build_buckets(order)
                for b in self._buckets:
                    self._launch(b)
                return
            count = torch.tensor([len(order)], dtype=torch.int64, device=self.params[0].device)
            lo, hi = count.clone(), count.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
            if lo.item() != hi.item():
                raise RuntimeError("ranks disagree on which parameters receive gradients")
            # every rank lays its buckets out in RANK 0's production order: a flat all-reduce of buckets built
            # from different local orders would silently add unrelated gradients.  The live SET must agree.
            mine = torch.tensor(order, dtype=torch.int64, device=count.device)
            ref = mine.clone()
            src = 0 if self.group is None else dist.get_global_rank(self.group, 0)
            dist.broadcast(ref, src=src, group=self.group)
            differs = torch.tensor([0 if torch.equal(torch.sort(ref)[0], torch.sort(mine)[0]) else 1],
                                   dtype=torch.int64, device=count.device)
            dist.all_reduce(differs, op=dist.ReduceOp.MAX, group=self.group)
            if differs.item():
                raise RuntimeError("ranks disagree on which parameters receive gradients (same count, different set)")
            order = [int(i) for i in ref.tolist()]
            self._build_buckets(order)
            for b in self._buckets:                # no overlap in the discovery pass
                self._launch(b)
        else:
            late = [b for b in self._buckets if b.pending != 0]
            if late:
                missing = sum(b.pending for b in late)
                raise RuntimeError(f"{missing} live parameters produced no gradient this step")

    def _adopt_bucket_views(self) -> None:
        if self._cuda:
            torch.cuda.current_stream().wait_stream(self._side)
        for b in self._buckets:
            for p, v in zip(b.params, b.views):
                if p.grad is not v:
                    p.grad = v                    # the averaged gradient lives in the bucket; no copy back

    def remove(self) -> None:
        for h in self._hooks:
            h.remove()
        self._hooks = []
