"""A stalled HIP stream as a test adversary: the tools of tests/test_stream_order_gpu.py.

The ordering between streams (weight-gradient side stream, panel cache, gradient buckets) and between host and device
(pinned rings, staged uploads) is hand-written Python around the kernels.  At fixture sizes a kernel finishes long before
Python reaches its reader, so a missing ``wait_stream`` / ``wait_event`` / ``record_stream`` loses no race and no test sees it.
Here one stream is held back by a bounded spin, so everything queued behind it really is late, and the blocks a racing reader
would see are poisoned, so "late" reads NaN instead of the previous test's (often correct) bits:

``stall(stream, ms)``       one finite spin of about ``ms`` milliseconds on ``stream`` (``torch.cuda._sleep``, calibrated once per
                            process between two timing events; without that attribute a chain of matrix products of calibrated
                            length) and an event recorded right behind it.  Never inside a captured graph, never above
                            ``MAX_STALL_MS``.
``held(event)``             the stall is still in force (``not event.query()``).  A scenario asserts it right after its last
                            consumer launch: a stall that is already over proved nothing, which is a failure, not a skip.
``independent_stream(others)``
                            a stream that shares no hardware queue with ``others``, found by probing: streams that share a queue
                            are serialised, and a stall of one would hold the other's reader back by accident.
``poison_pool(stream, shapes, dtype)``
                            allocates tensors of those shapes under ``stream``, fills every byte with 0xFF (a NaN in fp32, bf16
                            and fp64, 255 in uint8), frees them and synchronises: a fresh ``torch.empty`` of such a size on that
                            stream is served from these blocks and holds NaN until a kernel writes it.

``STALL_MS`` is the one stall length of the suite.  The rule: at least 4x the largest host time any scenario needs from queuing
its stall to its last enqueue and at least 50 ms.  ``MEASURED_ENQUEUE_MS`` holds those times, measured on an MI355X with the stall
replaced by a bare event (every race prints its own, ``pytest -s``): the model-level scenarios dominate at 33 ms, so the constant
is 150 ms.  ``held()`` is what makes a wrong choice a failure instead of a silent pass.

Plain module: no fixtures, importable without a device (tests/test_stalled_host.py).
"""
import math

import torch

MAX_STALL_MS = 2000
POISON_BYTE = 0xFF
MEASURED_ENQUEUE_MS = {           # scenario -> host milliseconds from the stall to the last enqueue, stall off
    "A1 backward": 5.8, "A1 autograd.grad": 0.4, "A2": 0.5, "A3 (five reasons, largest)": 0.6, "A5": 0.4, "A6 (three cases, largest)": 0.4,
    "A7": 0.6, "A4 wgrad held, 1 pass": 9.3, "A4 wgrad held, 3 passes": 32.3, "A4 bucket held, 1 pass": 8.4,
    "A4 bucket held, 3 passes": 28.6, "A8 join": 8.3, "A8 lifetime": 7.3, "C1 (four cases, largest)": 0.4, "C2": 0.3, "C3": 0.3,
    "C4": 33.2,
}
STALL_MS = 150
CALIBRATION_CYCLES = 2_000_000    # the probe spin: ~20 ms at the 100 MHz constant clock the spin kernel reads
_MM_SIDE = 2048                   # fallback: one fp32 product of this side per link of the chain

_rate = {}                        # "cycles": spin cycles per millisecond; "mm": milliseconds per matrix product


def check_ms(ms):
    """The stall length as a float; TypeError / ValueError for anything that is not a finite 0 < ms <= MAX_STALL_MS."""
    if isinstance(ms, bool) or not isinstance(ms, (int, float)):
        raise TypeError(f"stall: ms must be a number, not {type(ms).__name__}")
    ms = float(ms)
    if not math.isfinite(ms) or ms <= 0:
        raise ValueError(f"stall: ms must be finite and positive, not {ms}")
    if ms > MAX_STALL_MS:
        raise ValueError(f"stall: {ms} ms exceeds the {MAX_STALL_MS} ms cap (a stall is a bounded spin, never a wait)")
    return ms


def rate_from(units, elapsed_ms):
    """Calibration arithmetic: ``units`` (spin cycles, or matrix products) took ``elapsed_ms`` between two timing events."""
    if units <= 0:
        raise ValueError(f"calibration: {units} units of work")
    if not math.isfinite(elapsed_ms) or elapsed_ms <= 0:
        raise ValueError(f"calibration: {units} units of work measured as {elapsed_ms} ms")
    return units / elapsed_ms


def units_for(ms, per_ms):
    """Whole units of work (at least one) for a stall of ``ms`` at ``per_ms`` units per millisecond."""
    return max(1, int(math.ceil(check_ms(ms) * per_ms)))


def _timed(work, stream):
    """Milliseconds ``work()`` takes on ``stream``, between two timing events (after one untimed run: code-object load)."""
    with torch.cuda.stream(stream):
        work()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        work()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def cycles_per_ms(stream, measure=None):
    """Spin cycles per millisecond, measured once per process (``measure(cycles) -> ms`` replaces the device in the host test)."""
    if "cycles" not in _rate:
        measure = measure or (lambda cycles: _timed(lambda: torch.cuda._sleep(cycles), stream))
        _rate["cycles"] = rate_from(CALIBRATION_CYCLES, measure(CALIBRATION_CYCLES))
    return _rate["cycles"]


def _mm_operands(device):
    if "mm_ops" not in _rate:
        a = torch.full((_MM_SIDE, _MM_SIDE), 1.0 / _MM_SIDE, dtype=torch.float32, device=device)
        _rate["mm_ops"] = (a, torch.empty_like(a))
    return _rate["mm_ops"]


def mms_per_ms(stream, measure=None):
    """Matrix products per millisecond for the fallback chain, measured once per process."""
    if "mm" not in _rate:
        probe = 8

        def chain():
            a, out = _mm_operands(stream.device)
            for _ in range(probe):
                torch.mm(a, a, out=out)
        measure = measure or (lambda count: _timed(chain, stream))
        _rate["mm"] = rate_from(probe, measure(probe))
    return _rate["mm"]


def stall(stream, ms):
    """Queue one spin of about ``ms`` milliseconds on ``stream``; returns an event recorded right behind it."""
    ms = check_ms(ms)
    if not isinstance(stream, torch.cuda.Stream):
        raise TypeError(f"stall: a torch.cuda.Stream is expected, not {type(stream).__name__}")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("stall: not inside a captured graph")
    if hasattr(torch.cuda, "_sleep"):
        cycles = units_for(ms, cycles_per_ms(stream))
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
    else:
        links = units_for(ms, mms_per_ms(stream))
        a, out = _mm_operands(stream.device)
        with torch.cuda.stream(stream):
            for _ in range(links):
                torch.mm(a, a, out=out)
    event = torch.cuda.Event()
    event.record(stream)
    return event


def held(event):
    """The stall behind which ``event`` was recorded is still in force."""
    return not event.query()


def independent_stream(others, tries=16, probe_ms=5.0):
    """A new stream on which a stall does not hold ``others`` back (all idle: synchronise first).  The runtime multiplexes its
    streams over a few hardware queues, and two streams that share one are serialised: a stall of one then delays the other, the
    "racing" reader waits behind the spin by accident and a missing edge between the two cannot show.  Each candidate is probed
    with a short stall: a marker event recorded on every other stream must complete while the stall is still in force."""
    others = list(others)
    if not others or not all(isinstance(o, torch.cuda.Stream) for o in others):
        raise TypeError("independent_stream: the streams to be independent of are expected")
    probe_ms = check_ms(probe_ms)
    for _ in range(int(tries)):
        candidate = torch.cuda.Stream()
        spin = stall(candidate, probe_ms)
        free = True
        for other in others:
            marker = torch.cuda.Event()
            marker.record(other)
            marker.synchronize()
            if not held(spin):
                free = False
                break
        spin.synchronize()
        if free:
            return candidate
    raise RuntimeError(f"independent_stream: none of {tries} streams ran independently of the {len(others)} given")


def poison_(t):
    """Every byte of ``t`` (contiguous) becomes 0xFF: NaN in fp32 / bf16 / fp64, 255 in uint8.  Works on CPU tensors too."""
    if not t.is_contiguous():
        raise ValueError("poison_: a contiguous tensor is expected")
    if t.numel():
        t.reshape(-1).view(torch.uint8).fill_(POISON_BYTE)
    return t


def poison_pool(stream, shapes, dtype, copies=3):
    """Leave ``copies`` poisoned free blocks per shape in ``stream``'s pool of the caching allocator."""
    if not isinstance(stream, torch.cuda.Stream):
        raise TypeError(f"poison_pool: a torch.cuda.Stream is expected, not {type(stream).__name__}")
    if isinstance(copies, bool) or not isinstance(copies, int) or copies < 1:
        raise ValueError(f"poison_pool: copies must be an integer >= 1, not {copies!r}")
    shapes = [tuple(int(v) for v in (s if isinstance(s, (tuple, list, torch.Size)) else (s,))) for s in shapes]
    if any(v < 0 for s in shapes for v in s):
        raise ValueError(f"poison_pool: negative extent in {shapes}")
    with torch.cuda.stream(stream):
        blocks = [poison_(torch.empty(s, dtype=dtype, device=stream.device)) for s in shapes for _ in range(copies)]
        del blocks
    stream.synchronize()
