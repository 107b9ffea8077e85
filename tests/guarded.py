"""Guard-band buffers for testing the C ABI's memory contract ("kernels never allocate: workspaces are passed in", the
caller owns every output): a workspace of exactly the queried size, or an output of exactly its shape, sits between two
1 MiB bands of a known byte inside ONE allocation.  A kernel that writes past either end of what it was given changes a
band -- inside the test's own allocation, so the overrun is an assertion and never a fault -- and a kernel that reads
bytes nobody wrote sees the payload's prefill, which the caller varies (0x00 / 0xFF) between two otherwise equal runs.

The same layout pins what a kernel READS: an input's bytes are the payload of a buffer of exactly the input's extent
(``guarded_copy``) and the bands hold a byte chosen per instance.  A kernel that fetches past either end of an input and lets
the value reach its result computes something else when the band byte changes (``BAND_BYTES``); the fetch itself stays inside
the test's own allocation.

Plain module: no fixtures, works on CPU tensors as well (tests/test_guarded_host.py).
"""
import torch

GUARD_BYTES = 1 << 20
GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF)      # 0xFF..: a NaN in fp32 / fp64 / bf16, the NaN code of e4m3, -1 in int32
# The two poison bytes for the bands around INPUTS.  Neither alone catches every over-read that reaches a result:
#   0xFF..  is a NaN in fp32 / fp64 / bf16, the NaN code of e4m3, -1 in int32 and 255 in uint8: it survives every sum, every
#           product (times zero included) and every fma -- but fmaxf and `>` silently drop a NaN, so a max or a `y > 0` mask
#           that over-reads computes the right answer next to it;
#   0x7F..  is 3.39e38 in fp32 and bf16 and the largest positive sign-magnitude e4m3 pattern: it wins every max and passes
#           every `> 0` mask (tests/test_guarded_host.py records both halves on three small numpy "kernels").
BAND_BYTES = (0xFF, 0x7F)


class Guarded:
    """[front guard | payload | back guard] in one uint8 allocation; see ``guarded``."""

    def __init__(self, nbytes, device, fill, align=256, shift=0, guard_byte=GUARD_BYTE):
        nbytes, align, shift, guard_byte = int(nbytes), int(align), int(shift), int(guard_byte)
        if nbytes < 0 or align <= 0 or not 0 <= shift < align or not 0 <= guard_byte <= 0xFF:
            raise ValueError(f"guarded({nbytes}, align={align}, shift={shift}, guard_byte={guard_byte})")
        self.nbytes, self.fill, self.align, self.shift, self.guard_byte = nbytes, int(fill), align, shift, guard_byte
        self.buf = torch.full((2 * GUARD_BYTES + nbytes + align,), guard_byte, dtype=torch.uint8, device=device)
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
        """Both guards still hold the instance's guard byte; otherwise AssertionError naming the first and last changed byte of each guard relative to
        the payload's ends (front: negative offsets from the payload's first byte, -1 = the byte just before it; back:
        offsets from the byte just after the payload, +0)."""
        front = self.buf[self.start - GUARD_BYTES:self.start]
        back = self.buf[self.end:self.end + GUARD_BYTES]
        gb = self.guard_byte
        if not bool(((front != gb).any() | (back != gb).any()).item()):
            return
        msgs = []
        bad = torch.nonzero(front != gb).flatten()
        if bad.numel():
            msgs.append(f"{bad.numel()} byte(s) written BEFORE the payload: first at payload_start{int(bad[0]) - GUARD_BYTES:+d}, "
                        f"last at payload_start{int(bad[-1]) - GUARD_BYTES:+d}")
        bad = torch.nonzero(back != gb).flatten()
        if bad.numel():
            msgs.append(f"{bad.numel()} byte(s) written PAST the payload: first at payload_end{int(bad[0]):+d}, "
                        f"last at payload_end{int(bad[-1]):+d}")
        band = "" if gb == GUARD_BYTE else f", guard byte 0x{gb:02X}"
        raise AssertionError(f"{what or 'buffer'} ({self.nbytes} bytes, prefill 0x{self.fill:02X}{band}): " + "; ".join(msgs))


def guarded(nbytes, device, fill, align=256, shift=0, guard_byte=GUARD_BYTE):
    """One allocation laid out as [1 MiB guard | nbytes payload | 1 MiB guard]; the payload starts ``shift`` bytes after an
    ``align``-byte boundary; guards hold ``guard_byte`` (0xA5), the payload ``fill``.  Returns an object with ``.ptr``,
    ``.view(dtype, shape)`` and ``.check()``."""
    return Guarded(nbytes, device, fill, align, shift, guard_byte)


def guarded_like(dtype, shape, device, fill, align=256, shift=0, guard_byte=GUARD_BYTE):
    """A guarded buffer of exactly ``shape`` elements of ``dtype`` (an output tensor)."""
    n = 1
    for v in shape:
        n *= int(v)
    return Guarded(n * torch.empty((), dtype=dtype).element_size(), device, fill, align, shift, guard_byte)


def guarded_copy(tensor, device, guard_byte=GUARD_BYTE, align=256, shift=0):
    """An INPUT: ``tensor``'s bytes (in contiguous order) as the payload of a guarded buffer of exactly
    ``tensor.numel() * tensor.element_size()`` bytes, the bands holding ``guard_byte``.  With ``align=256`` the payload has the
    alignment of a fresh allocation, so an entry point that dispatches on ``ptr & 15`` takes the route it takes elsewhere;
    ``shift`` moves it off that boundary on purpose."""
    src = tensor.detach().contiguous()
    b = Guarded(src.numel() * src.element_size(), device, 0x00, align, shift, guard_byte)
    if b.nbytes:
        b.payload.copy_(src.reshape(-1).view(torch.uint8))
    return b


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
