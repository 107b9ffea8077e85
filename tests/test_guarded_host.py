"""Host-side self-test of tests/guarded.py on CPU tensors: the guard bands and the "every element written" check must be
able to fail, and must say where (tests/test_workspace_contract_gpu.py relies on both)."""
import re

import pytest
import torch

import guarded as G


@pytest.mark.parametrize("fill", G.FILLS)
@pytest.mark.parametrize("nbytes", [0, 1, 100, 4096])
def test_untouched_buffer_passes(nbytes, fill):
    b = G.guarded(nbytes, "cpu", fill)
    assert b.payload.numel() == nbytes and bool((b.payload == fill).all())
    b.check()
    b.payload.fill_(0x3C)                 # writing all of the payload is what a kernel is allowed to do
    b.check()
    assert b.buf.numel() >= nbytes + 2 * G.GUARD_BYTES
    assert b.start >= G.GUARD_BYTES and b.end + G.GUARD_BYTES <= b.buf.numel()


@pytest.mark.parametrize("where,expect", [
    ("payload_end", r"PAST the payload: first at payload_end\+0, last at payload_end\+0"),
    ("payload_start-1", r"BEFORE the payload: first at payload_start-1, last at payload_start-1"),
    ("far_back", rf"PAST the payload: first at payload_end\+{G.GUARD_BYTES - 1}, last at payload_end\+{G.GUARD_BYTES - 1}"),
    ("far_front", rf"BEFORE the payload: first at payload_start-{G.GUARD_BYTES}, last at payload_start-{G.GUARD_BYTES}"),
])
@pytest.mark.parametrize("nbytes", [0, 52, 4096])
def test_one_flipped_guard_byte_fails_with_the_right_offset(nbytes, where, expect):
    b = G.guarded(nbytes, "cpu", 0xFF)
    index = {"payload_end": b.end, "payload_start-1": b.start - 1, "far_back": b.end + G.GUARD_BYTES - 1,
             "far_front": b.start - G.GUARD_BYTES}[where]
    b.buf[index] ^= 0x01
    with pytest.raises(AssertionError) as e:
        b.check("ws")
    assert re.search(expect, str(e.value)), str(e.value)
    assert "1 byte(s)" in str(e.value) and f"ws ({nbytes} bytes" in str(e.value)


def test_a_run_of_changed_bytes_reports_first_and_last():
    b = G.guarded(64, "cpu", 0x00)
    b.buf[b.end + 3:b.end + 20] = 0
    b.buf[b.start - 8:b.start - 2] = 0
    with pytest.raises(AssertionError) as e:
        b.check()
    assert "first at payload_end+3, last at payload_end+19" in str(e.value)
    assert "first at payload_start-8, last at payload_start-3" in str(e.value)


@pytest.mark.parametrize("align,shift", [(256, 0), (256, 16), (512, 0), (64, 4), (4096, 48)])
def test_alignment_and_shift_hold(align, shift):
    for nbytes in (0, 12, 1000):
        b = G.guarded(nbytes, "cpu", 0x00, align=align, shift=shift)
        assert b.ptr % align == shift
        assert b.ptr == b.buf.data_ptr() + b.start
        b.check()
    with pytest.raises(ValueError):
        G.guarded(16, "cpu", 0, align=256, shift=256)


def test_typed_views_alias_the_payload():
    b = G.guarded_like(torch.float32, (3, 5), "cpu", 0xFF)
    v = b.view(torch.float32, (3, 5))
    assert v.data_ptr() == b.ptr and b.nbytes == 60 and bool(torch.isnan(v).all())
    v.copy_(torch.arange(15.).view(3, 5))
    b.check()
    assert torch.equal(b.bytes().view(torch.float32), torch.arange(15.))
    assert bool((G.guarded_like(torch.int32, (4,), "cpu", 0xFF).view(torch.int32, (4,)) == -1).all())
    assert bool(torch.isnan(G.guarded_like(torch.bfloat16, (4,), "cpu", 0xFF).view(torch.bfloat16, (4,))).all())
    assert bool(torch.isnan(G.guarded_like(torch.float64, (4,), "cpu", 0xFF).view(torch.float64, (4,))).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.uint8])
def test_one_unwritten_element_fails_the_every_element_written_check(dtype):
    shape = (3, 7, 5)
    b = G.guarded_like(dtype, shape, "cpu", 0xFF)
    v = b.view(dtype, shape)
    assert G.unwritten(v) == v.numel()
    v.copy_(torch.arange(v.numel()).view(shape).to(dtype) if dtype != torch.uint8 else torch.ones(shape, dtype=dtype))
    G.assert_all_written(v)               # fully written: passes
    flat = b.payload.view(dtype)
    flat[52] = _prefill_scalar(dtype)     # exactly one element left alone
    assert G.unwritten(v) == 1
    with pytest.raises(AssertionError) as e:
        G.assert_all_written(v, "y")
    assert "y: 1 of 105 element(s)" in str(e.value) and "flat index 52" in str(e.value)


def _prefill_scalar(dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((size,), 0xFF, dtype=torch.uint8).view(dtype)[0]


# ---- the guard byte is the instance's own ---------------------------------------------------------------------------------
@pytest.mark.parametrize("guard_byte", [G.GUARD_BYTE] + list(G.BAND_BYTES))
def test_check_passes_and_fails_against_the_instance_s_own_guard_byte(guard_byte):
    b = G.guarded(52, "cpu", 0x00, guard_byte=guard_byte)
    assert b.guard_byte == guard_byte
    assert bool((b.buf[:b.start] == guard_byte).all()) and bool((b.buf[b.end:] == guard_byte).all())
    b.check()
    b.payload.fill_(0x3C)
    b.check()
    other = G.GUARD_BYTE if guard_byte != G.GUARD_BYTE else 0xFF     # the default byte is a change in a poisoned band, and the reverse
    b.buf[b.end + 5] = other
    b.buf[b.start - 3] = other
    with pytest.raises(AssertionError) as e:
        b.check("x")
    assert "first at payload_end+5, last at payload_end+5" in str(e.value)              # the offsets mean what they meant
    assert "first at payload_start-3, last at payload_start-3" in str(e.value)
    assert "x (52 bytes" in str(e.value)
    assert (f"guard byte 0x{guard_byte:02X}" in str(e.value)) == (guard_byte != G.GUARD_BYTE)
    with pytest.raises(ValueError):
        G.guarded(4, "cpu", 0, guard_byte=256)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.uint8, torch.float8_e4m3fn])
@pytest.mark.parametrize("guard_byte", G.BAND_BYTES)
def test_guarded_copy_round_trips_the_bytes_in_an_exact_extent(dtype, guard_byte):
    shape = (3, 5, 7)
    src = (torch.arange(105).view(shape) - 50).to(torch.float32).to(dtype)
    view = src.transpose(0, 2)                                       # a non-contiguous operand: placed in contiguous order
    for t in (src, view, src[:0], src[0, 0, 0]):
        b = G.guarded_copy(t, "cpu", guard_byte)
        assert b.nbytes == t.numel() * t.element_size() and b.end - b.start == b.nbytes
        assert b.ptr % 256 == 0 and b.guard_byte == guard_byte
        assert torch.equal(b.bytes(), t.contiguous().reshape(-1).view(torch.uint8))
        assert bool((b.buf[b.start - G.GUARD_BYTES:b.start] == guard_byte).all())
        assert bool((b.buf[b.end:b.end + G.GUARD_BYTES] == guard_byte).all())
        b.check()
    for shift in (2, 14):
        b = G.guarded_copy(src, "cpu", guard_byte, align=16, shift=shift)
        assert b.ptr % 16 == shift and torch.equal(b.bytes(), src.reshape(-1).view(torch.uint8))
    assert bool((G.guarded_copy(src, "cpu").buf[:G.GUARD_BYTES] == G.GUARD_BYTE).all())


def test_what_the_band_bytes_read_as():
    """The values the comment at guarded.BAND_BYTES promises."""
    ff, sf = (torch.full((8,), b, dtype=torch.uint8) for b in G.BAND_BYTES)
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        assert bool(torch.isnan(ff.view(dtype)).all())
    assert bool(torch.isnan(ff.view(torch.float8_e4m3fn).float()).all())
    assert bool((ff.view(torch.int32) == -1).all()) and bool((ff == 255).all())
    assert 3.38e38 < float(sf.view(torch.float32)[0]) < 3.4e38 and 3.38e38 < float(sf.view(torch.bfloat16)[0].float()) < 3.4e38
    assert bool(torch.isfinite(sf.view(torch.float32)).all())
    # e4m3: 0x7F is the positive NaN code, the largest positive pattern when the codes are compared as sign-magnitude integers
    assert int(sf[0]) == max(range(0x80))


# ---- the checker catches what it is for: three "kernels" that read one element past a guarded input ---------------------------
def _input_and_one_past(values, band):
    """The input as the kernel is given it (exactly its extent) and as a kernel with an off-by-one bound sees it."""
    import numpy as np
    b = G.guarded_copy(torch.from_numpy(values), "cpu", band)
    n = values.size
    return b, b.buf[b.start:b.end + 4].numpy().view(np.float32), n


def _k_sum(x, n, over):
    import numpy as np
    return np.asarray([x[:n + over].sum(dtype=np.float32)])


def _k_window_max(x, n, over):
    """fmaxf over windows of 4; the last window runs ``over`` elements long."""
    import numpy as np
    out = np.fmax.reduce(x[:n].reshape(-1, 4), axis=1)
    if over:
        out[-1] = np.fmax(out[-1], x[n])
    return out


def _k_relu_mask(y, n, over, dy):
    """dx[i] = y[i] > 0 ? dy[i] : 0, with the mask of the last element taken one element late."""
    import numpy as np
    idx = np.arange(n)
    if over:
        idx[-1] += 1
    with np.errstate(invalid="ignore"):
        return np.where(y[idx] > 0, dy, np.float32(0))


def _run_kernel(kind, band, over):
    import numpy as np
    rng = np.random.default_rng(7)
    x = rng.standard_normal(16).astype(np.float32)
    x[-1] = -abs(x[-1]) - 0.5                           # the mask kernel's last y is negative: the late read decides
    dy = rng.standard_normal(16).astype(np.float32) + 3.0
    b, seen, n = _input_and_one_past(x, band)
    with np.errstate(invalid="ignore", over="ignore"):
        out = {"sum": lambda: _k_sum(seen, n, over), "max": lambda: _k_window_max(seen, n, over),
               "mask": lambda: _k_relu_mask(seen, n, over, dy)}[kind]()
    b.check()                                           # an over-READ changes no band: only the results can tell
    assert torch.equal(b.bytes(), torch.from_numpy(x).view(torch.uint8))
    return out.tobytes()


@pytest.mark.parametrize("kind,caught_by", [("sum", {0xFF: True, 0x7F: True}), ("max", {0xFF: False, 0x7F: True}),
                                            ("mask", {0xFF: False, 0x7F: True})])
def test_two_band_bytes_because_a_nan_band_alone_misses_a_max_type_over_read(kind, caught_by):
    """The recorded reason for BAND_BYTES: the contract compares a poisoned run's outputs with the ordinary run's, byte for byte.
    A sum that reads one element too many differs under the NaN band; an fmax or a ``> 0`` mask that does so gives the RIGHT
    bytes next to a NaN and is only seen next to 3.39e38.  With correct bounds every kernel passes under both."""
    first = _run_kernel(kind, G.GUARD_BYTE, over=0)
    for band in G.BAND_BYTES:
        assert _run_kernel(kind, band, over=0) == first, f"{kind}: correct bounds, band 0x{band:02X}"
        differs = _run_kernel(kind, band, over=1) != first
        assert differs == caught_by[band], f"{kind} reading one element past its input, band 0x{band:02X}: caught = {differs}"
    assert any(caught_by.values())


# ---- the element-aligned run of guarded.run_contract ------------------------------------------------------------------------------
def test_element_shifts_differ_between_neighbouring_operands():
    assert [G.element_shift(torch.float32, i) for i in range(5)] == [4, 8, 12, 4, 8]
    assert [G.element_shift(torch.uint8, i) for i in range(4)] == [1, 2, 3, 1]
    runs = G.contract_runs(shifted=True)
    assert runs[-1] == (0xFF, 0, G.GUARD_BYTE, True) and [r[3] for r in runs[:-1]] == [False] * 5       # prefill 0xFF, ordinary bands
    assert G.contract_runs(shifted=False, element_aligned=False) == G.contract_runs(shifted=False)[:-1]


@pytest.mark.parametrize("shift", [4, 8, 12])
def test_a_shifted_output_buffer_is_placed_where_asked_and_guarded_from_its_first_byte(shift):
    b = G.guarded_like(torch.float32, (3, 5), "cpu", 0xFF, shift=shift)
    v = b.view(torch.float32, (3, 5))
    assert b.ptr % 256 == shift and v.data_ptr() == b.ptr and b.nbytes == 60
    v.fill_(1.0)
    b.check()                                              # all of the payload, nothing else
    b.buf[b.start - 4:b.start] = 0                         # one element in front of the shifted payload: where an aligned-down store lands
    with pytest.raises(AssertionError) as e:
        b.check("y")
    assert "4 byte(s) written BEFORE the payload: first at payload_start-4, last at payload_start-1" in str(e.value)


def _numpy_scale(base_of):
    """y = 2 * x on raw addresses, as a kernel sees them; ``base_of(x_address, y_address)`` = where it actually reads and writes."""
    import ctypes
    import numpy as np

    def launch(p, n=24):
        xa, ya = base_of(p["x"], p["y"])
        x = np.ctypeslib.as_array((ctypes.c_float * n).from_address(xa))
        y = np.ctypeslib.as_array((ctypes.c_float * n).from_address(ya))
        y[:] = 2 * x
        return 0
    return launch


@pytest.mark.parametrize("kind", ["honest", "rounds_its_bases_down", "takes_x_and_y_for_misaligned_alike"])
def test_a_kernel_that_assumes_16_byte_alignment_fails_the_element_aligned_run_only(kind):
    base_of = {"honest": lambda x, y: (x, y),
               "rounds_its_bases_down": lambda x, y: (x & ~15, y & ~15),             # "the first float4"
               "takes_x_and_y_for_misaligned_alike": lambda x, y: (x, (y & ~15) + (x & 15))}[kind]
    x = torch.arange(24.) - 7
    args = ("scale", _numpy_scale(base_of), {"y": (torch.float32, (24,))})
    first, info = G.run_contract(*args, ins={"x": x}, element_aligned=False)           # the runs there were before: every kernel passes
    assert torch.equal(first["y"], 2 * x) and info == {"element_operands": 0, "element_equal": None}
    if kind == "honest":
        first, info = G.run_contract(*args, ins={"x": x})
        assert torch.equal(first["y"], 2 * x) and info == {"element_operands": 2, "element_equal": True}
        return
    with pytest.raises(AssertionError) as e:
        G.run_contract(*args, ins={"x": x})
    assert "element-aligned operands (x +4, y +8)" in str(e.value) and "BEFORE the payload" in str(e.value), str(e.value)


def test_operands_that_keep_their_alignment_and_the_other_route_hook():
    """bf16 / integer operands and the names in ``aligned`` stay on their boundary; ``other_route`` replaces the byte comparison of
    the element-aligned run, and the caller learns whether the bytes were equal after all."""
    seen = []

    def launch(p):
        seen.append({k: v % 256 for k, v in p.items() if isinstance(v, int)})
        return 0

    outs = {"y": (torch.float32, (4,), torch.zeros(4)), "coef": (torch.float32, (4,), torch.zeros(4)), "z": (torch.bfloat16, (8,), torch.zeros(8)),
            "index": (torch.int32, (4,), torch.zeros(4, dtype=torch.int32))}
    ins = {"x": torch.ones(4), "frames": torch.ones(5, dtype=torch.uint8), "w": (torch.ones(4), 16)}
    hooked = []
    _, info = G.run_contract("placement", launch, outs, {"ws": 64}, shifted=True, ins=ins, aligned={"coef"}, other_route=hooked.append)
    assert info == {"element_operands": 3, "element_equal": True} and len(hooked) == 1 and set(hooked[0]) == set(outs)
    assert seen[-1] == {"x": 4, "frames": 2, "w": 16, "y": 12, "coef": 0, "z": 0, "index": 0, "ws": 0}
    assert seen[2]["ws"] == 16 and all(s["x"] == 0 and s["y"] == 0 for s in seen[:-1])
