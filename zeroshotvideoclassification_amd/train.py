"""Training / evaluation step of the reference's driver, on the HIP path.

``train_step`` reproduces the order of ``train_one_epoch`` (main.py:170-203): zero_grad ->
forward -> MSE -> backward -> optimizer step, with ``main_02.py:256``'s handling of the
``(emb, None)`` tuple.  The reference wraps forward in CUDA fp16 autocast +
GradScaler (main.py:137,172,195-203); the fp32 configuration benchmarked here (BASELINE
configs 1-3) runs without them, which is what the reference's CPU path does too (autocast is a
no-op there).  The per-step train accuracy (main.py:182-185) is computed on the device so it
does not stall the queue.

``evaluate`` / ``compute_accuracy`` restate main.py:224-325: eval-mode forward under
``no_grad``, cosine nearest class in the 300-d embedding space, top-1 / top-5, and the ten
seeded half-class splits.  The scoring is one device pass (``score_splits`` -> ``zsv_split_accuracy``)
and one device -> host copy of its integers.

``load_weights`` / ``save_checkpoint`` keep the reference's checkpoint format (main.py:114-124,
361-365): ``{'state_dict' ('module.'-prefixed keys), 'opt', 'accuracy'}``, loaded by key
intersection, so checkpoints move between the two implementations unchanged.

``classification_accuracy`` / ``evaluate_classification`` are the same two things for a ``network.Classifier`` -- a trunk
trained on class labels before the zero-shot stage takes it over (not in the reference, which downloads such trunks): top-1 /
top-5 of the logits from the counts the loss kernel leaves on the device.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Tuple

from ctypes import c_void_p

import numpy as np
import torch

from . import _lib, ops


_PREFIX = "module."       # nn.DataParallel's prefix in saved checkpoints (main.py:116,126,363)


_CLASS_LAYER = "model.fc."    # the trunk's classification layer: its class count belongs to the task the checkpoint was trained on


def load_weights(model: torch.nn.Module, path: str, key: str = "state_dict") -> int:
    """main.py:114-124: strip the ``module.`` prefix, keep the keys the model has, load the rest
    from the model itself.  Returns the number of tensors taken from the checkpoint.  ``key="state_dict_avg"`` loads the
    averaged weights ``save_checkpoint(average=)`` stored next to the live ones.

    The trunk's classification layer (``model.fc.*``) is left out, and not counted, when its shape differs from the model's:
    a ``network.Classifier`` pre-trained on any number of classes hands its trunk to a ``network.Model`` (which builds that
    layer with 400 and never applies it) or to a classifier for another label set.  Every other shape mismatch raises, as
    ``load_state_dict`` does."""
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    if key not in checkpoint:
        raise KeyError(f"{path} has no {key!r}: it holds {sorted(checkpoint, key=str)}")
    weights = checkpoint[key]
    own = getattr(model, "module", model)
    model_dict = own.state_dict()
    j = len(_PREFIX)
    weights = {k[j:]: v for k, v in weights.items() if k[j:] in model_dict}
    weights = {k: v for k, v in weights.items()
               if not (k.startswith(_CLASS_LAYER) and tuple(v.shape) != tuple(model_dict[k].shape))}
    model_dict.update(weights)
    own.load_state_dict(model_dict)
    _lib.note_raw_write()
    return len(weights)


def save_checkpoint(model: torch.nn.Module, path: str, opt=None, accuracy: float = 0.0, average=None) -> None:
    """main.py:361-365: the saved keys carry the ``module.`` prefix whether or not the model is wrapped.  ``average``
    (``optim.WeightAverage``) adds ``"state_dict_avg"``: a complete state dict of the same format with the averaged tensors
    substituted and everything else live.  The reference's loader reads only ``['state_dict']`` and is unaffected."""
    own = getattr(model, "module", model)
    state = {_PREFIX + k: v.detach().cpu() for k, v in own.state_dict().items()}
    checkpoint = {"state_dict": state, "opt": opt, "accuracy": accuracy}
    if average is not None:
        checkpoint["state_dict_avg"] = {_PREFIX + k: v.cpu() for k, v in average.averaged_state_dict(own).items()}
    torch.save(checkpoint, path)


def embed(model: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    out = model(x)
    return out[0] if isinstance(out, tuple) else out


class StepPacer:
    """Bounds how far the host may run ahead of the device: ``wait()`` at the head of a step blocks until the step
    ``depth`` steps back has finished on the device.

    The reference's loop reads ``loss.item()`` every iteration (main.py:203), i.e. it never runs ahead at all.  This path
    has no host sync in a step, and a host that queues step k+1 while step k still runs cannot reuse the activation blocks
    the weight-gradient stream still holds (``Tensor.record_stream``): every step of lead costs one more set of saved
    activations (8-11 GB at 22 clips) taken from the driver by hipMalloc inside the loop.  With few launches per step
    (C3D: ~130) the host would be many steps ahead within milliseconds.  ``depth = 2`` keeps one whole step queued behind
    the running one (the device never idles) and the pool at three sets, reached after three steps."""

    def __init__(self, depth: int = 2):
        from collections import deque
        self.depth = max(1, int(depth))
        self.marks = deque()
        self.waits = 0                 # steps whose head really had to wait (diagnostics)

    def wait(self) -> None:
        while len(self.marks) >= self.depth:
            ev = self.marks.popleft()
            if not ev.query():
                self.waits += 1
                ev.synchronize()

    def mark(self) -> None:
        ev = torch.cuda.Event()
        ev.record()
        self.marks.append(ev)

    def drain(self) -> None:
        self.marks.clear()


def train_step(model: torch.nn.Module, optimizer: torch.optim.Optimizer, criterion, x: torch.Tensor,
               z: torch.Tensor, grad_sync=None, scaler=None, pacer: Optional[StepPacer] = None,
               autocast: bool = False, graph: Optional[bool] = None,
               micro_batches: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """One iteration of main.py:170-203.  ``grad_sync`` (a ``ddp.GradientSync``) all-reduces the
    gradients across ranks, overlapped with backward, before the optimizer step.  ``scaler`` (an
    ``optim.LossScaler`` or a ``torch.cuda.amp.GradScaler``) reproduces main.py:195-203:
    ``scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()`` -- a non-finite gradient skips
    the update and halves the scale.  ``autocast=True`` runs forward and loss inside ``amp.autocast()`` -- main.py:172's
    ``with autocast():`` -- i.e. the VideoResNet trunks in bf16 (``amp``: bf16 activations and products, fp32 accumulation,
    statistics, parameters, gradients and loss); the default is the fp32 step of BASELINE configs 1-3, which is what the
    reference's CPU path runs (autocast is a no-op there).  ``pacer`` (a ``StepPacer``) bounds the host's lead over the device.
    Weight decay and gradient clipping need no argument here: the optimizer carries them (``optim.FusedAdam(weight_decay=,
    decoupled_weight_decay=, max_grad_norm=)``; the norm of the step is ``optimizer.grad_norm``, a device tensor).

    ``micro_batches=k`` accumulates the gradient over k consecutive parts of ``x`` / ``z`` (sizes as equal as possible, larger
    first) before ONE optimizer step: each part has its own forward, BatchNorm batch statistics and backward of
    ``(n_j / N) * loss_j`` -- what ``nn.DataParallel`` over k replicas computes (main.py:61-63,126), and torch's literal
    accumulation recipe.  The running statistics are updated k times and ``num_batches_tracked`` advances by k, as under
    torch accumulation (DataParallel keeps replica 0's update only).  One loss scale and one non-finite check per step: a
    non-finite gradient in any part skips the whole step.  Clipping and weight decay act on the accumulated gradient.
    Returns the concatenated embeddings and ``sum_j (n_j / N) * loss_j`` (the loss of the whole batch for a mean-reduced
    criterion).  With a ``grad_sync`` the flat buckets are the accumulators (one ``zsv_grad_accum_multi`` launch per bucket
    and part, one exchange per step); ``GradientSync(model, local=True)`` is the intended single-GPU path.  Without one the
    loop relies on autograd's own accumulation into ``.grad`` (torch add kernels)."""
    if micro_batches != 1:
        return _train_step_accumulated(model, optimizer, criterion, x, z, grad_sync, scaler, pacer, autocast, graph,
                                       micro_batches)
    if pacer is not None:
        pacer.wait()
    optimizer.zero_grad(set_to_none=True)
    if grad_sync is not None:
        grad_sync.begin_step()
    if autocast:
        from . import amp
        with amp.autocast(graph=graph):           # graph=True: the bf16 trunk as two hipGraphs (amp._GraphedTrunk)
            y = embed(model, x)
            loss = criterion(y, z)
    else:
        y = embed(model, x)
        loss = criterion(y, z)
    (scaler.scale(loss) if scaler is not None else loss).backward()
    ops.join_wgrad_streams()          # (the autograd end-of-pass callback has done this already; a no-op wait then)
    if grad_sync is not None:
        grad_sync.finish_step()
    if scaler is not None:
        scaler.step(optimizer)
        scaler.update()
    else:
        optimizer.step()
    if pacer is not None:
        pacer.mark()
    return y.detach(), loss.detach()


def micro_batch_sizes(n: int, k: int) -> list:
    """``n`` samples in ``k`` consecutive parts, as equal as possible, the larger ones first."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"micro_batches must be an integer >= 1, not {k!r}")
    if k > n:
        raise ValueError(f"micro_batches={k} exceeds the {n} samples of the batch")
    base, extra = divmod(n, k)
    return [base + 1] * extra + [base] * (k - extra)


def _train_step_accumulated(model, optimizer, criterion, x, z, grad_sync, scaler, pacer, autocast, graph, micro_batches):
    """``train_step(micro_batches=k)`` for k > 1 (see there)."""
    total = int(x.shape[0])
    sizes = micro_batch_sizes(total, micro_batches)
    if int(z.shape[0]) != total:
        raise ValueError(f"train_step: {total} clips but {int(z.shape[0])} targets")
    if pacer is not None:
        pacer.wait()
    optimizer.zero_grad(set_to_none=True)
    if grad_sync is not None:
        grad_sync.begin_step(passes=micro_batches)
    ys, loss_sum = [], None
    parts = zip(torch.split(x, sizes), torch.split(z, sizes))
    for j, (xj, zj) in enumerate(parts):
        if autocast:
            from . import amp
            with amp.autocast(graph=graph):
                yj = embed(model, xj)
                loss = criterion(yj, zj)
        else:
            yj = embed(model, xj)
            loss = criterion(yj, zj)
        loss = loss * (sizes[j] / total)
        (scaler.scale(loss) if scaler is not None else loss).backward()
        ops.join_wgrad_streams()
        if grad_sync is not None:
            if j + 1 < micro_batches:
                grad_sync.end_pass()
            else:
                grad_sync.finish_step()
        ys.append(yj.detach())
        loss_sum = loss.detach() if loss_sum is None else loss_sum + loss.detach()
    if scaler is not None:
        scaler.step(optimizer)
        scaler.update()
    else:
        optimizer.step()
    if pacer is not None:
        pacer.mark()
    return torch.cat(ys), loss_sum


def nearest_classes(embed_: torch.Tensor, class_embed: torch.Tensor, k: int = 5) -> torch.Tensor:
    """``cdist(embed, class_embed, 'cosine').argsort(1)[:, :k]`` (main.py:321) on the device: double-precision
    cosine distances on the matrix core + per-row top-k with ties by lower index (``zsv_cosine_topk``,
    csrc/nearest_class.hip).  ``(rows, k)`` int64 class indices; HIP tensors only."""
    if not (embed_.is_cuda and class_embed.is_cuda):
        raise RuntimeError("nearest_classes runs on an MI355X HIP device only (no CPU fallback)")
    c = class_embed.detach().float().contiguous()
    e = embed_.detach().float().reshape(len(embed_), c.shape[-1] if c.dim() == 2 else -1).contiguous()
    if e.dim() != 2 or c.dim() != 2 or e.shape[1] != c.shape[1]:
        raise RuntimeError(f"nearest_classes: embeddings {tuple(e.shape)} vs class table {tuple(c.shape)}")
    rows, n_classes = int(e.shape[0]), int(c.shape[0])
    k = min(int(k), n_classes)
    out = torch.empty((rows, k), dtype=torch.int32, device=e.device)
    if rows == 0:
        return out.long()
    lib = _lib.load()
    nbytes = lib.zsv_cosine_topk_workspace_bytes(rows, n_classes)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    with torch.cuda.device(e.device):
        _lib.check(lib.zsv_cosine_topk(e.data_ptr(), c.data_ptr(), rows, int(e.shape[1]), n_classes, k, out.data_ptr(),
                                       None, ws.data_ptr(), nbytes, c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "zsv_cosine_topk")
    return out.long()


def cosine_ranking(pred: torch.Tensor, class_embed: torch.Tensor, k: int = 5) -> torch.Tensor:
    """The first ``k`` columns of the reference's ``cdist(...).argsort(1)`` (main.py:321)."""
    return nearest_classes(pred, class_embed, k)


def train_accuracy(y: torch.Tensor, class_embed: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """main.py:182-185 without leaving the device: percent of samples whose nearest class embedding is
    their label's (``cdist(Y, class_embed, 'cosine').argmin(1) == l``).  A 0-d device tensor, no host sync."""
    pred = nearest_classes(y, class_embed.to(y.device), 1)[:, 0]
    return (pred == labels.to(pred.device).reshape(-1)).float().mean() * 100.0


_split_table_cache: dict = {}      # (n_classes, splits, device) -> (host table, its device copy)


def split_tables(n_classes: int, splits: int) -> np.ndarray:
    """The class tables ``evaluate`` scores, as ``(splits + 1, n_classes)`` int32 positions for ``zsv_split_accuracy``: row 0 is
    the whole table (``pos[0][c] = c``); row ``s + 1`` is split ``s`` of main.py:281-288 -- ``np.random.seed(s)``, ``chosen =
    np.random.permutation(C)[:C // 2]`` -- with ``pos[s + 1][chosen[j]] = j`` (the class's row in
    ``class_embedding[sel_classes]``: permutation order, not sorted) and -1 everywhere else.  The draws are made on numpy's
    GLOBAL generator on every call, like the reference does: it leaves that generator seeded and later draws
    (``camera_motion_trajectory``) come from it, so the host table is never cached."""
    n_classes, splits = int(n_classes), int(splits)
    pos = np.full((splits + 1, n_classes), -1, dtype=np.int32)
    pos[0] = np.arange(n_classes, dtype=np.int32)
    for split in range(splits):
        np.random.seed(split)                                             # main.py:284
        chosen = np.random.permutation(n_classes)[:n_classes // 2]
        pos[split + 1][chosen] = np.arange(len(chosen), dtype=np.int32)
    return pos


def _device_split_tables(n_classes: int, splits: int, device: torch.device) -> torch.Tensor:
    pos = split_tables(n_classes, splits)                                 # replayed every call; only the upload is cached
    key = (int(n_classes), int(splits), str(device))
    hit = _split_table_cache.get(key)
    if hit is None or not np.array_equal(hit[0], pos):
        hit = (pos, torch.from_numpy(pos).to(device))
        _split_table_cache[key] = hit
    return hit[1]


def _score_splits(pred, true, labels, class_embed, splits, per_class) -> Tuple[torch.Tensor, int]:
    """One int32 device buffer ``(splits + 1 [+ C], 3)``: ``counts`` and, below it, ``class_counts``; and the number of tables."""
    tensors = [pred, true, class_embed] + ([labels] if labels is not None else [])
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("score_splits runs on an MI355X HIP device only (no CPU fallback)")
    assert len(pred) == len(true), "True and predicted labels must have the same number of samples"
    c = class_embed.detach().float().contiguous()
    if c.dim() != 2:
        raise RuntimeError(f"score_splits: class table {tuple(c.shape)}")
    n_classes, dim = int(c.shape[0]), int(c.shape[1])
    p = pred.detach().float().reshape(len(pred), dim).contiguous()
    t = true.detach().float().reshape(len(true), dim).contiguous()
    rows, tables = int(p.shape[0]), int(splits) + 1
    if tables > 1:
        if labels is None or labels.numel() != rows:
            raise RuntimeError("score_splits: the class splits need one label per row")
        labels = labels.detach().reshape(-1).long().contiguous()
    pos = _device_split_tables(n_classes, int(splits), p.device)
    if rows == 0 or n_classes == 0:
        return torch.zeros((tables + (n_classes if per_class else 0), 3), dtype=torch.int32, device=p.device), tables
    out = torch.empty((tables + (n_classes if per_class else 0), 3), dtype=torch.int32, device=p.device)
    lib = _lib.load()
    nbytes = lib.zsv_split_accuracy_workspace_bytes(rows, n_classes)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(lib.zsv_split_accuracy(p.data_ptr(), t.data_ptr(), labels.data_ptr() if tables > 1 else None, c.data_ptr(),
                                          rows, dim, n_classes, pos.data_ptr(), tables, out.data_ptr(),
                                          out[tables:].data_ptr() if per_class else None, ws.data_ptr(), nbytes,
                                          c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_split_accuracy")
    return out, tables


def score_splits(pred: torch.Tensor, true: torch.Tensor, labels: Optional[torch.Tensor], class_embed: torch.Tensor,
                 splits: int = 10, per_class: bool = False):
    """The integers behind ``evaluate``'s accuracies, left on the device (``zsv_split_accuracy``, csrc/nearest_class.hip; no host
    synchronisation): ``counts (splits + 1, 3)`` int32 = rows scored, top-1 hits, top-5 hits over the whole class table (row 0,
    main.py:264-266) and over each ``np.random.seed(split)`` half-class split (row ``split + 1``, main.py:281-304; the tables are
    ``split_tables(C, splits)``).  Inside a split ties are ordered as the stable argsort of the gathered sub-table orders them:
    by the class's position in ``sel_classes``.  ``per_class=True`` also returns ``class_counts (C, 3)``: the same three numbers of
    the whole table per true class (main.py:322: the class nearest to the true embedding, not the label).  ``labels`` may be None
    when ``splits == 0``.  HIP tensors only; no rows: zeros, without a launch."""
    out, tables = _score_splits(pred, true, labels, class_embed, splits, per_class)
    return (out[:tables], out[tables:]) if per_class else out


def compute_accuracy(predicted_embed: torch.Tensor, class_embed: torch.Tensor,
                     true_embed: torch.Tensor) -> Tuple[float, float]:
    """Top-1 / top-5 accuracy (percent) to the closest class embedding (main.py:316-325): one ``score_splits`` and one read."""
    assert len(predicted_embed) == len(true_embed), "True and predicted labels must have the same number of samples"
    rows, hit1, hit5 = score_splits(predicted_embed, true_embed, None, class_embed, splits=0)[0].tolist()
    n = max(rows, 1)
    # counts are exact integers; the reference's np.mean of booleans is the same count / n in double
    return float(hit1) / n * 100, float(hit5) / n * 100


def _gather_rows(t: torch.Tensor, group) -> torch.Tensor:
    """All ranks' rows of ``t`` (different counts per rank), concatenated in rank order."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    count = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count, group=group)
    counts = [int(c.item()) for c in counts]
    width = max(counts)
    padded = torch.zeros((width,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    padded[:t.shape[0]] = t
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded, group=group)
    return torch.cat([p[:c] for p, c in zip(parts, counts)])


@torch.no_grad()
def evaluate(model: torch.nn.Module, batches: Iterable[Sequence[torch.Tensor]], class_embed: torch.Tensor,
             device: Optional[torch.device] = None, splits: int = 10, dtype: Optional[torch.dtype] = None,
             group=None, sharded: Optional[bool] = None, local_batches: bool = False,
             sync_state: bool = True, average=None, per_class: bool = False) -> dict:
    """main.py:224-313 for one test set.  ``batches`` yields ``(X, labels, Z, ...)``; samples with
    label -1 (failed loads, auxiliary_dataset.py:502-505) are dropped like main.py:246-248.
    ``dtype=torch.bfloat16`` runs the forward on the bf16 engine (``inference.Bf16Engine``, the
    reduced-precision eval of BASELINE config 5 / the reference's autocast, main.py:172), ``torch.float32``
    on the folded fp32 engine (``inference.Fp32Engine``), ``torch.float8_e4m3fn`` on the e4m3 engine
    (``inference.Fp8Engine``; for a ``network.C3D`` ``inference.Fp8EngineC3D``, which needs the activation scales of
    ``inference.calibrate_fp8(model, clips)`` stored on the model first); default (None): the module's own fp32 forward.

    With ``torch.distributed`` initialised (one process per GPU; ``sharded`` defaults to that) every rank
    iterates the SAME ``batches`` and runs the forward for every ``world``-th one (batch ``i`` belongs to
    rank ``i % world``); with ``local_batches=True`` the iterable is this rank's OWN shard (a per-rank loader:
    nothing is skipped, no rank decodes another rank's clips).  The ``(pred, true, label)`` rows are
    all-gathered over ``group`` (RCCL) and every rank computes the same accuracies.  The reference evaluates
    under one-process ``nn.DataParallel`` (main.py:126,250), which scatters each batch and runs every replica
    with DEVICE 0's parameters and BatchNorm running statistics.  Data-parallel training keeps those statistics
    per replica (``ddp.GradientSync``), so before a sharded evaluation every rank takes rank 0's parameters and
    buffers (``sync_state``; one flat broadcast per dtype): all samples are scored by ONE model -- the one rank 0
    would checkpoint (main.py:361-365).  NOTE: this overwrites the other ranks' BatchNorm running statistics, mid-training
    too -- what ``nn.DataParallel`` does implicitly every forward.  ``sync_state=False`` skips the broadcast when the caller knows the
    replicas are identical (e.g. right after ``load_weights`` on every rank).

    ``average`` (``optim.WeightAverage``): the evaluation runs on the averaged weights, swapped into the live tensors for
    its duration (``with average.applied():``).

    The scoring is one ``score_splits`` call and one device -> host copy of its integers; the percentages and the mean / std
    over the splits are formed from them on the host.  ``per_class=True`` adds ``"class_counts"`` (``(C, 3)`` int64: rows,
    top-1 hits, top-5 hits per true class over the whole table) and ``"mean_class_accuracy"`` (the mean of the per-class top-1
    over the classes that have rows); the other keys do not change."""
    if average is not None:
        with average.applied():
            return evaluate(model, batches, class_embed, device=device, splits=splits, dtype=dtype, group=group, sharded=sharded,
                            local_batches=local_batches, sync_state=sync_state, per_class=per_class)
    import torch.distributed as dist
    if sharded is None:
        sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if sharded else (0, 1)
    modes = [(m, m.training) for m in model.modules()]     # per module: a frozen BatchNorm in a training model stays frozen
    model.eval()
    if sharded and sync_state:
        src = 0 if group is None else dist.get_global_rank(group, 0)
        from .ddp import broadcast_tensors
        broadcast_tensors(list(model.parameters()) + list(model.buffers()), src, group)      # one collective per dtype
        if dist.get_rank() != src:                         # (the source's values did not change: its panels / engines stay)
            _lib.note_raw_write()                          # `.data` writes: cached folded-BatchNorm engines must rebuild
    device = device or next(model.parameters()).device
    forward = model
    if dtype in (torch.bfloat16, torch.float32, torch.float8_e4m3fn):
        from .inference import engine_for
        forward = engine_for(model, dtype)                 # BatchNorm folded; fp32, bf16 or e4m3 activations
    elif dtype is not None:
        raise RuntimeError(f"evaluate: dtype {dtype} is not supported (fp32 or bf16)")
    preds, trues, labels = [], [], []
    for index, batch in enumerate(batches):
        if not local_batches and index % world != rank:
            continue
        x, l, z = batch[0], batch[1], batch[2]
        keep = l != -1
        if keep.sum() == 0:
            continue
        x, l, z = x[keep], l[keep], z[keep]
        preds.append(embed(forward, x.to(device, non_blocking=True)).float())
        # targets / labels join the device once, after the loop: a per-batch blocking copy would drain the
        # queue every batch (and an idle-then-busy GPU showed sporadic 30-80 ms stalls on the test pool)
        trues.append(z.float().reshape(len(l), -1))
        labels.append(l.reshape(-1))
    for m, training in modes:
        m.training = training
    class_embed = class_embed.to(device)
    width = int(class_embed.shape[1])
    pred = torch.cat(preds) if preds else torch.zeros((0, width), device=device)
    true = torch.cat(trues).to(device) if trues else torch.zeros((0, width), device=device)
    label_dev = torch.cat(labels).to(device).long() if labels else torch.zeros((0,), dtype=torch.int64, device=device)
    if sharded:
        pred, true, label_dev = (_gather_rows(t, group) for t in (pred, true, label_dev))
    if not splits and not per_class:                      # the whole table alone: compute_accuracy is that one call and one read
        acc, acc5 = compute_accuracy(pred, class_embed, true)
        return {"accuracy": acc, "accuracy_top5": acc5, "n": int(len(pred))}
    # the whole table and every split in one launch chain, then ONE device -> host copy of the integers
    buf, tables = _score_splits(pred, true, label_dev, class_embed, int(splits), per_class)
    host = buf.cpu().numpy()
    n = max(int(len(pred)), 1)
    out = {"accuracy": float(host[0, 1]) / n * 100, "accuracy_top5": float(host[0, 2]) / n * 100, "n": int(len(pred))}
    if splits:
        scored = [row for row in host[1:tables] if row[0]]                   # a split none of whose classes occurs is left out
        a1 = [float(row[1]) / int(row[0]) * 100 for row in scored]
        a5 = [float(row[2]) / int(row[0]) * 100 for row in scored]
        if a1:
            out.update(split_accuracy=float(np.mean(a1)), split_accuracy_std=float(np.std(a1)),
                       split_accuracy_top5=float(np.mean(a5)), split_accuracy_top5_std=float(np.std(a5)))
    if per_class:
        per = host[tables:].astype(np.int64)
        seen = per[:, 0] > 0
        out["class_counts"] = per
        out["mean_class_accuracy"] = float(np.mean(per[seen, 1] / per[seen, 0] * 100)) if seen.any() else 0.0
    return out


def classification_accuracy(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-1 and top-5 accuracy in percent from the ``counts`` of ``ops.softmax_cross_entropy`` /
    ``network.SoftmaxCrossEntropy.counts`` (rows not ignored, top-1 hits, top-5 hits).  Two 0-d tensors on ``counts``' device,
    no host synchronisation; 0 when no row was scored."""
    scored = counts[0].clamp(min=1).to(torch.float32)
    return counts[1].to(torch.float32) * 100.0 / scored, counts[2].to(torch.float32) * 100.0 / scored


@torch.no_grad()
def evaluate_classification(model: torch.nn.Module, batches: Iterable[Sequence[torch.Tensor]],
                            device: Optional[torch.device] = None, label_smoothing: float = 0.0) -> dict:
    """``evaluate``'s loop for a ``network.Classifier``: eval-mode forward under ``no_grad``, cross-entropy and top-1 / top-5
    per clip.  ``batches`` yields ``(X (bs, nc, 3, T, H, W), labels (bs) or (bs, nc), ...)``; a clip labelled -1 (a failed load,
    auxiliary_dataset.py:502-505) is dropped by the loss kernel's ``ignore_index`` on the device, not by indexing on the host.
    The loss sum and the counts accumulate on the device and come back in ONE device -> host copy at the end.  Returns
    ``{"loss": mean loss of the scored clips, "top1": percent, "top5": percent, "samples": clips scored}``.  One process;
    clips are scored one by one (no averaging over the clips of a video)."""
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    device = device or next(model.parameters()).device
    totals = torch.zeros(4, dtype=torch.float64, device=device)          # loss sum, rows scored, top-1 hits, top-5 hits
    for batch in batches:
        x, l = batch[0], batch[1]
        clips_per_sample = int(x.shape[1])
        if l.dim() == 1 and clips_per_sample > 1:
            l = l.repeat_interleave(clips_per_sample)
        logits = model(x.to(device, non_blocking=True))
        loss, counts = ops.softmax_cross_entropy(logits.float(), l.reshape(-1).to(device, non_blocking=True).long(),
                                                 label_smoothing=label_smoothing, ignore_index=-1, reduction="sum")
        totals[0] += loss
        totals[1:] += counts
    for m, training in modes:
        m.training = training
    loss_sum, samples, top1, top5 = totals.cpu().tolist()
    n = max(samples, 1.0)
    return {"loss": loss_sum / n, "top1": top1 / n * 100, "top5": top5 / n * 100, "samples": int(samples)}
