"""tests/stalled.py without a device: argument checks and the cap, the calibration arithmetic on injected timings, ``held`` on a
stub event, and the poison pattern as a NaN in every floating type the kernels use."""
import math

import pytest
import torch

import stalled


class _Event:
    def __init__(self, done):
        self.done = done
        self.queries = 0

    def query(self):
        self.queries += 1
        return self.done


def test_stall_length_checks_and_the_cap():
    assert stalled.MAX_STALL_MS == 2000
    assert stalled.check_ms(1) == 1.0 and stalled.check_ms(2000) == 2000.0 and stalled.check_ms(0.25) == 0.25
    for bad in (2000.001, 2001, 1e9, 0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            stalled.check_ms(bad)
    for bad in ("50", None, True, [50]):
        with pytest.raises(TypeError):
            stalled.check_ms(bad)
    # the suite's own constant obeys its rule: >= 50 ms, >= 4x every measured enqueue time, under the cap
    assert 50 <= stalled.STALL_MS <= stalled.MAX_STALL_MS
    assert stalled.STALL_MS >= 4 * max(stalled.MEASURED_ENQUEUE_MS.values(), default=0.0)


def test_stall_refuses_before_touching_a_device():
    with pytest.raises(ValueError):
        stalled.stall(None, 2001)                  # the cap comes first: nothing is queued for a refused length
    with pytest.raises(TypeError):
        stalled.stall(None, 50)
    with pytest.raises(TypeError):
        stalled.stall("cuda", 50)
    with pytest.raises(TypeError):
        stalled.poison_pool(None, [(4,)], torch.float32)
    with pytest.raises(TypeError):
        stalled.independent_stream([])
    with pytest.raises(TypeError):
        stalled.independent_stream(["cuda"])


def test_calibration_arithmetic_with_injected_timings(monkeypatch):
    assert stalled.rate_from(2_000_000, 20.0) == 100_000.0
    assert stalled.units_for(50, 100_000.0) == 5_000_000
    assert stalled.units_for(0.001, 3.0) == 1                     # never zero work
    assert stalled.units_for(2000, 0.75) == 1500
    assert stalled.units_for(10, 0.33) == 4                       # rounded up: a stall is never shorter than asked
    with pytest.raises(ValueError):
        stalled.units_for(2001, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            stalled.rate_from(1000, bad)
    with pytest.raises(ValueError):
        stalled.rate_from(0, 1.0)

    # once per process: the second call does not measure again
    monkeypatch.setattr(stalled, "_rate", {})
    calls = []

    def measure(cycles):
        calls.append(cycles)
        return cycles / 2_400_000.0                               # a 2.4 GHz clock

    assert stalled.cycles_per_ms(None, measure) == pytest.approx(2_400_000.0)
    assert stalled.cycles_per_ms(None, lambda c: 1 / 0) == pytest.approx(2_400_000.0)
    assert calls == [stalled.CALIBRATION_CYCLES]
    assert stalled.units_for(stalled.STALL_MS, stalled.cycles_per_ms(None)) == math.ceil(stalled.STALL_MS * 2_400_000.0)
    # the matrix-product fallback: 8 products in 4 ms -> 2 per ms -> a 50 ms chain has 100 links
    assert stalled.mms_per_ms(None, lambda count: 4.0) == 2.0
    assert stalled.mms_per_ms(None, lambda count: 1 / 0) == 2.0
    assert stalled.units_for(50, stalled.mms_per_ms(None)) == 100
    monkeypatch.setattr(stalled, "_rate", {})
    with pytest.raises(ValueError):
        stalled.cycles_per_ms(None, lambda c: 0.0)                # a probe that measured nothing is no calibration
    assert "cycles" not in stalled._rate


def test_held_is_not_query():
    running, done = _Event(False), _Event(True)
    assert stalled.held(running) is True
    assert stalled.held(done) is False
    assert running.queries == 1 and done.queries == 1             # one query, no waiting


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_poison_is_nan(dtype):
    t = stalled.poison_(torch.zeros(3, 5, dtype=dtype))
    assert bool(torch.isnan(t).all())
    assert bool((t.reshape(-1).view(torch.uint8) == 0xFF).all())
    assert stalled.poison_(torch.zeros(0, dtype=dtype)).numel() == 0


def test_poison_of_bytes_and_layout():
    assert stalled.POISON_BYTE == 0xFF
    b = stalled.poison_(torch.zeros(7, dtype=torch.uint8))
    assert b.tolist() == [255] * 7
    s = stalled.poison_(torch.zeros((), dtype=torch.float32))     # a 0-d tensor is poisoned too
    assert math.isnan(s.item())
    with pytest.raises(ValueError):
        stalled.poison_(torch.zeros(4, 4)[:, ::2])
