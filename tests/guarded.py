"""Guard-band buffers for testing the C ABI's memory contract ("kernels never allocate: workspaces are passed in", the
caller owns every output): a workspace of exactly the queried size, or an output of exactly its shape, sits between two
1 MiB bands of a known byte inside ONE allocation.  A kernel that writes past either end of what it was given changes a
band -- inside the test's own allocation, so the overrun is an assertion and never a fault -- and a kernel that reads
bytes nobody wrote sees the payload's prefill, which the caller varies (0x00 / 0xFF) between two otherwise equal runs.

Plain module: no fixtures, works on CPU tensors as well (tests/test_guarded_host.py).
"""
import torch

GUARD_BYTES = 1 << 20
GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF)      # 0xFF..: a NaN in fp32 / fp64 / bf16, the NaN code of e4m3, -1 in int32


class Guarded:
    """[front guard | payload | back guard] in one uint8 allocation; see ``guarded``."""

    def __init__(self, nbytes, device, fill, align=256, shift=0):
        nbytes, align, shift = int(nbytes), int(align), int(shift)
        if nbytes < 0 or align <= 0 or not 0 <= shift < align:
            raise ValueError(f"guarded({nbytes}, align={align}, shift={shift})")
        self.nbytes, self.fill, self.align, self.shift = nbytes, int(fill), align, shift
        self.buf = torch.full((2 * GUARD_BYTES + nbytes + align,), GUARD_BYTE, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = GUARD_BYTES + (shift - (base + GUARD_BYTES)) % align      # first payload byte, within buf
        self.end = self.start + nbytes
        self.ptr = base + self.start
        self.payload.fill_(self.fill)

    @property
    def payload(self):
        """The payload as a uint8 view (empty for nbytes == 0)."""
        return self.buf[self.start:self.end]

    def view(self, dtype, shape):
        """The payload as a typed tensor (an output the kernel under test writes)."""
        return self.payload.view(dtype).view(shape)

    def bytes(self):
        """A copy of the payload's raw bytes."""
        return self.payload.clone()

    def check(self, what=""):
        """Both guards untouched; otherwise AssertionError naming the first and last changed byte of each guard relative to
        the payload's ends (front: negative offsets from the payload's first byte, -1 = the byte just before it; back:
        offsets from the byte just after the payload, +0)."""
        front = self.buf[self.start - GUARD_BYTES:self.start]
        back = self.buf[self.end:self.end + GUARD_BYTES]
        if not bool(((front != GUARD_BYTE).any() | (back != GUARD_BYTE).any()).item()):
            return
        msgs = []
        bad = torch.nonzero(front != GUARD_BYTE).flatten()
        if bad.numel():
            msgs.append(f"{bad.numel()} byte(s) written BEFORE the payload: first at payload_start{int(bad[0]) - GUARD_BYTES:+d}, "
                        f"last at payload_start{int(bad[-1]) - GUARD_BYTES:+d}")
        bad = torch.nonzero(back != GUARD_BYTE).flatten()
        if bad.numel():
            msgs.append(f"{bad.numel()} byte(s) written PAST the payload: first at payload_end{int(bad[0]):+d}, "
                        f"last at payload_end{int(bad[-1]):+d}")
        raise AssertionError(f"{what or 'buffer'} ({self.nbytes} bytes, prefill 0x{self.fill:02X}): " + "; ".join(msgs))


def guarded(nbytes, device, fill, align=256, shift=0):
    """One allocation laid out as [1 MiB guard | nbytes payload | 1 MiB guard]; the payload starts ``shift`` bytes after an
    ``align``-byte boundary; guards hold 0xA5, the payload ``fill``.  Returns an object with ``.ptr``, ``.view(dtype, shape)``
    and ``.check()``."""
    return Guarded(nbytes, device, fill, align, shift)


def guarded_like(dtype, shape, device, fill, align=256, shift=0):
    """A guarded buffer of exactly ``shape`` elements of ``dtype`` (an output tensor)."""
    n = 1
    for v in shape:
        n *= int(v)
    return Guarded(n * torch.empty((), dtype=dtype).element_size(), device, fill, align, shift)


def unwritten(t):
    """Number of elements of a 0xFF-prefilled output that still hold the prefill: NaN for the floating types (fp32, fp64,
    bf16: the inputs are finite, so a NaN is an element nobody wrote or a read of poison), 0xFF for uint8 (the e4m3 NaN code,
    which the saturating epilogues never produce), -1 for the signed integer types."""
    if t.dtype.is_floating_point:
        return int(torch.isnan(t).sum().item())
    if t.dtype == torch.uint8:
        return int((t == 0xFF).sum().item())
    return int((t == -1).sum().item())


def assert_all_written(t, what=""):
    """The "every element written" check on an output of a 0xFF-prefilled run."""
    n = unwritten(t)
    if n:
        flat = t.reshape(-1)
        bad = torch.isnan(flat) if t.dtype.is_floating_point else (flat == (0xFF if t.dtype == torch.uint8 else -1))
        first = int(torch.nonzero(bad).flatten()[0])
        raise AssertionError(f"{what or 'output'}: {n} of {t.numel()} element(s) still hold the 0xFF prefill (unwritten, or computed "
                             f"from unwritten workspace bytes); first at flat index {first}")
