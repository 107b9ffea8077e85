"""Host side of the table-driven multi-tensor launches (``zsv_adam_multi``, ``zsv_grad_accum_multi``, ...).

A launch walks a device array of descriptors in chunks of ``CHUNK`` elements: ``first_chunk`` of a descriptor is the running
sum of ``ceil(n / CHUNK)`` over the descriptors before it.  Tables whose addresses change every step are built on the host
and uploaded through ``PinnedRing``.
"""
from __future__ import annotations

import torch

CHUNK = 4096


def chunks(n: int) -> int:
    return (n + CHUNK - 1) // CHUNK


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
