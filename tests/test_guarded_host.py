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
