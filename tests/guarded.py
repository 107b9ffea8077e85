"""Guard-band buffers for testing the C ABI's memory contract ("kernels never allocate: workspaces are passed in", the
caller owns every output): a workspace of exactly the queried size, or an output of exactly its shape, sits between two
1 MiB bands of a known byte inside ONE allocation.  A kernel that writes past either end of what it was given changes a
band -- inside the test's own allocation, so the overrun is an assertion and never a fault -- and a kernel that reads
bytes nobody wrote sees the payload's prefill, which the caller varies (0x00 / 0xFF) between two otherwise equal runs.

The same layout pins what a kernel READS: an input's bytes are the payload of a buffer of exactly the input's extent
(``guarded_copy``) and the bands hold a byte chosen per instance.  A kernel that fetches past either end of an input and lets
the value reach its result computes something else when the band byte changes (``BAND_BYTES``); the fetch itself stays inside
the test's own allocation.

``run_contract`` is the sequence of runs built on this -- two prefills, a shifted workspace, two poisoned bands and the
element-aligned run, in which every fp32 / uint8 operand sits 4, 8 or 12 (1, 2 or 3) bytes past its boundary.

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


# ---- the element-aligned run ----------------------------------------------------------------------------------------------
# include/zsv_hip.h: fp32 tensors and vectors need only 4-byte alignment, each on its own, uint8 frames none at all.  Every such
# operand of a call, inputs and outputs alike, starts e * (1 + i mod 3) bytes past a 256-byte boundary -- e its element size,
# i its position among them -- so fp32 operands sit at +4, +8, +12 and neighbours differ from each other: a kernel that rounds
# a base down to 16 bytes, or takes "x and y are misaligned alike" for granted, writes a band, leaves an element unwritten or
# computes other bytes.  Everything else (workspaces, panels, blobs, mask tables, coefficient rows, channels-last bf16 / e4m3
# tensors, integer tables) keeps its alignment.
ELEMENT_ALIGNED_DTYPES = (torch.float32, torch.uint8)


def element_shift(dtype, position):
    """Bytes past the 256-byte boundary of the ``position``-th element-aligned operand of a call."""
    return torch.empty((), dtype=dtype).element_size() * (1 + int(position) % 3)


def contract_runs(shifted, element_aligned=True):
    """(payload prefill, workspace shift, band byte, element-aligned?) of every run of ``run_contract``."""
    return [(0x00, 0, GUARD_BYTE, False), (0xFF, 0, GUARD_BYTE, False)] + ([(0xFF, 16, GUARD_BYTE, False)] if shifted else []) + \
        [(0x00, 0, band, False) for band in BAND_BYTES] + ([(0xFF, 0, GUARD_BYTE, True)] if element_aligned else [])


def _raw(t):
    return t.contiguous().view(-1).view(torch.uint8)


def run_contract(entry, launch, outs, works=None, shifted=False, defined=None, ins=None, aligned=(), device="cpu", synchronize=None,
                 status_string=str, other_route=None, element_aligned=True):
    """Run ``launch`` once per entry of ``contract_runs`` on fresh guarded buffers and assert, after ``synchronize()``: status 0,
    every band intact, every input unchanged, no output element of a 0xFF run left at the prefill, and the outputs of every run
    equal to the first run's as raw bytes.

    outs:  name -> (dtype, shape) or (dtype, shape, initial tensor) -- the latter for in / out arguments;
    works: name -> bytes: workspaces, blobs, panels, mask tables (prefilled, guarded, not compared); ``shifted`` (True, or a set
           of their names): one more run has them 16 bytes past a 256-byte boundary;
    ins:   name -> tensor of EXACTLY the extent the callee may read (None: an operand left out, the launch gets None), or
           (tensor, shift): the copy starts ``shift`` bytes past a 256-byte boundary in every run;
    aligned: names of fp32 / uint8 operands that keep their 16-byte alignment in the element-aligned run (coefficient rows,
           e4m3 tensors held as uint8);
    launch(p): p[name] = address, p["table"](tensor) = the address of a guarded copy of a table the launch itself builds;
           returns the status, or a list of them;
    defined(name, tensor) -> the part of an output the operation defines (default: all of it);
    other_route: None, or -- for a call whose kernel family depends on the operands' alignment -- a function of the
           element-aligned run's outputs that makes the comparison (against a reference of its own) in place of the byte
           comparison with the first run.
    Returns (the first run's outputs (copies), {"element_operands": how many operands the element-aligned run moved (0: that run
    was left out, nothing to move), "element_equal": whether its outputs equalled the first run's bytes (None without it)})."""
    works, ins = works or {}, ins or {}
    for name in ins:
        assert name not in outs and name not in works, f"{entry}: {name} is named twice"
    moved = [name for name, t in ins.items() if t is not None and not isinstance(t, tuple) and t.dtype in ELEMENT_ALIGNED_DTYPES] + \
        [name for name, spec in outs.items() if spec[0] in ELEMENT_ALIGNED_DTYPES]
    moved = [name for name in moved if name not in aligned]
    runs = contract_runs(shifted, element_aligned and bool(moved))
    results = []
    for fill, shift, band, elem in runs:
        bufs, views, sources = {}, {}, {}
        at = {name: element_shift(ins[name].dtype if name in ins else outs[name][0], i) for i, name in enumerate(moved)} if elem else {}
        for name, t in ins.items():
            if t is None:
                continue
            t, in_shift = t if isinstance(t, tuple) else (t, at.get(name, 0))
            bufs[name] = sources[name] = guarded_copy(t, device, band, 256, in_shift)
        for name, spec in outs.items():
            b = guarded_like(spec[0], spec[1], device, fill, 256, at.get(name, 0), guard_byte=band)
            views[name] = b.view(spec[0], spec[1])
            if len(spec) > 2:
                views[name].copy_(spec[2])
            bufs[name] = b
        for name, nbytes in works.items():
            bufs[name] = guarded(nbytes, device, fill, 256, shift if (shifted is True or (shifted and name in shifted)) else 0, guard_byte=band)
        before = {name: b.bytes() for name, b in sources.items()}
        p = {name: b.ptr for name, b in bufs.items()}
        p.update({name: None for name, t in ins.items() if t is None})

        def table(tensor, name="table"):
            """For a launch that builds a table of addresses of this run's buffers: the table as one more guarded input."""
            name = f"{name} #{len(bufs)}"
            bufs[name] = sources[name] = guarded_copy(tensor, device, band)
            before[name] = sources[name].bytes()
            return sources[name].ptr

        p["table"] = table
        status = launch(p)
        if synchronize:
            synchronize()
        what = f"{entry}, prefill 0x{fill:02X}" + (", workspace at 256 k + 16" if shift else "") + \
            (f", bands 0x{band:02X}" if band != GUARD_BYTE else "") + \
            (", element-aligned operands (" + ", ".join(f"{n} +{s}" for n, s in at.items()) + ")" if elem else "")
        for s in (status if isinstance(status, (list, tuple)) else [status]):
            assert s == 0, f"{what}: {status_string(int(s))} (status {s})"
        for name, b in bufs.items():
            b.check(f"{what}: {name}")
        for name, b in sources.items():
            assert torch.equal(b.payload, before[name]), f"{what}: the input {name} was written (inputs are const)"
        got = {}
        for name, v in views.items():
            part = defined(name, v) if defined else v
            if fill == 0xFF:
                assert_all_written(part, f"{what}: {name}")
            got[name] = part.clone()
        results.append(got)
    info = {"element_operands": len(moved) if runs[-1][3] else 0, "element_equal": None}
    for (fill, shift, band, elem), got in zip(runs[1:], results[1:]):
        same = all(v.shape == results[0][name].shape and torch.equal(_raw(v), _raw(results[0][name])) for name, v in got.items())
        if elem:
            info["element_equal"] = same
            if other_route is not None:
                other_route(got)
                continue
        for name, v in got.items():
            first = results[0][name]
            if elem and v.shape != first.shape:
                raise AssertionError(f"{entry}: what the call defines of {name} depends on the ALIGNMENT of the operands: {tuple(v.shape)} with the "
                                     f"fp32 / uint8 tensors off their 16-byte boundaries, {tuple(first.shape)} on them")
            assert v.shape == first.shape, f"{entry}: {name}: {tuple(v.shape)} vs {tuple(first.shape)}"
            a, b = _raw(v), _raw(first)
            if torch.equal(a, b):
                continue
            index = int(torch.nonzero(a != b).flatten()[0]) // v.element_size()
            where = f"{int((a != b).sum())} byte(s) differ from the ordinary run, first at flat index {index} of {v.numel()}"
            if elem:
                raise AssertionError(f"{entry}: {name} depends on the ALIGNMENT of the operands: with the fp32 / uint8 tensors 4, 8 and 12 (1, 2, 3) "
                                     f"bytes past a 16-byte boundary {where}")
            if band == GUARD_BYTE:
                raise AssertionError(f"{entry}: {name} depends on what the buffers held before the call (prefill 0x00 vs 0x{fill:02X}, "
                                     f"shift {shift})")
            raise AssertionError(f"{entry}: {name} depends on bytes OUTSIDE the inputs or the workspace: with bands of 0x{band:02X} "
                                 f"around every buffer {where}")
    return results[0], info


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
