"""Host side of the table-driven multi-tensor launches (``zsv_adam_multi``, ``zsv_grad_accum_multi``, ...).

A launch walks a device array of descriptors in chunks of ``CHUNK`` elements: ``first_chunk`` of a descriptor is the running
sum of ``ceil(n / CHUNK)`` over the descriptors before it.  Tables whose addresses change every step are built on the host
and uploaded through ``PinnedRing``.
"""
from __future__ import annotations

import struct

import torch

CHUNK = 4096                  # CHUNK of csrc/multi_tensor.h


def chunks(n: int) -> int:
    return (n + CHUNK - 1) // CHUNK


_ROW = {3: struct.Struct("<QQqq"), 5: struct.Struct("<QQQQqq")}       # zsv_pair_tensor / zsv_accum_tensor, zsv_adam_tensor


def pack_rows(rows):
    """The bytes of a descriptor table and its total chunk count.  A row is ``(*addresses, n)`` -- four addresses for a
    ``zsv_adam_tensor``, two for a ``zsv_pair_tensor`` or ``zsv_accum_tensor`` -- and gets its ``first_chunk`` here.  (On the
    host path of every optimizer step: one precompiled ``Struct`` per row shape, one join.)"""
    if not rows:
        return bytearray(), 0
    pack = _ROW[len(rows[0])].pack
    packed, first = [], 0
    for row in rows:
        packed.append(pack(*row, first))
        first += (row[-1] + CHUNK - 1) // CHUNK
    return bytearray(b"".join(packed)), first


class PinnedRing:
    """Uploads small descriptor tables without stalling the host.

    The host runs ahead of the GPU, so a pinned staging buffer may not be rewritten until the copy queued from it has
    executed: rotate over a small ring guarded by events (a pageable copy would be safe too, but torch synchronises the
    stream for it and the run-ahead is lost).  The copy is queued on the CURRENT stream of ``dev``; the returned device
    tensor belongs to that stream."""

    def __init__(self, slots: int = 4):
        self._ring = [[None, None] for _ in range(slots)]     # (pinned staging buffer, copy-done event)
        self._next = 0

    def upload(self, raw: bytearray, dev) -> torch.Tensor:
        nbytes = len(raw)
        slot = self._ring[self._next % len(self._ring)]
        self._next += 1
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 48 * 512), dtype=torch.uint8).pin_memory()
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0][:nbytes].copy_(torch.frombuffer(raw, dtype=torch.uint8))
        table = slot[0][:nbytes].to(dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(dev))
        return table
