"""The eight multi-tensor Adam entry points (``zsv_adam[w]_multi[_scaled][_avg]``) against each other, raw through ctypes.

They are one update rule with three options -- decay / clipping, the loss scaler, the weight average -- so what one form computes
is pinned by another that must give the same bytes: an ``_avg`` form by its plain form, a clip record holding 1.0 by no record,
``grads_unscaled`` by a scale of 1.0, any scaled form with ``found_inf`` set by the untouched inputs.  Every comparison is of
bytes; the values themselves are held to torch's optimizers by test_optim_gpu.py and test_optim_decay_clip_gpu.py.

p, g, exp_avg, exp_avg_sq and the shadows are slices of five flat sentinel-filled buffers.  A slice starts 0-3 elements past a
16-byte boundary, differently in each buffer, and the lengths sit around the 4096-element chunk.  Each check runs on the table of
all slices and on a table of one 4097-element tensor (``count == 1``: the table search has nothing to search, two chunks)."""
import ctypes
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

from zeroshotvideoclassification_amd import _lib  # noqa: E402

DEV = "cuda"
LENGTHS, OFFSETS = (1, 255, 4095, 4096, 4097, 5000), (0, 1, 2, 3)
SENTINEL = -12345.0
ARRAYS = ("p", "g", "exp_avg", "exp_avg_sq", "shadow")
LR, B1, B2, EPS, WD, STEP, EMA = 1e-2, 0.9, 0.999, 1e-8, 0.05, 4, 0.25
FORMS = [(decay, scaled, avg) for decay in (False, True) for scaled in (False, True) for avg in (False, True)]


def _name(form):
    decay, scaled, avg = form
    return "zsv_adam" + ("w" if decay else "") + "_multi" + ("_scaled" if scaled else "") + ("_avg" if avg else "")


def _flat(seed, shift, square):
    """A flat buffer of sentinels with one slice per (offset, length): the slice starts (offset + shift) mod 4 elements past a
    16-byte boundary, and at least one sentinel separates neighbours.  Returns (buffer, [(start, n)], mask of the sentinels)."""
    spans, cursor = [], 0
    for off in OFFSETS:
        for n in LENGTHS:
            cursor += 1
            while cursor % 4 != (off + shift) % 4:
                cursor += 1
            spans.append((cursor, n))
            cursor += n
    flat = torch.full((cursor + 5,), SENTINEL, dtype=torch.float32)
    outside = torch.ones(flat.shape, dtype=torch.bool)
    gen = torch.Generator().manual_seed(seed)
    for start, n in spans:
        x = torch.randn(n, generator=gen)
        flat[start:start + n] = x * x if square else x
        outside[start:start + n] = False
    flat = flat.to(DEV)
    assert flat.data_ptr() % 16 == 0
    return flat, spans, outside.to(DEV)


@pytest.fixture(scope="module")
def world():
    """The five buffers, their pristine copies, and the two tables (with the shadow-pointer arrays that go with them)."""
    w = {"lib": _lib.load(), "flat": {}, "spans": {}, "outside": {}, "pristine": {}}
    for i, name in enumerate(ARRAYS):
        flat, spans, outside = _flat(10 + i, i, square=name == "exp_avg_sq")
        w["flat"][name], w["spans"][name], w["outside"][name], w["pristine"][name] = flat, spans, outside, flat.clone()
    every = list(range(len(LENGTHS) * len(OFFSETS)))
    single = [LENGTHS.index(4097) + len(LENGTHS)]                                    # the 4097-element slice at offset 1
    w["tables"] = {}
    for kind, picks in (("all_slices", every), ("one_tensor_two_chunks", single)):
        rows, pointers, first = b"", [], 0
        for j in picks:
            at = {name: w["flat"][name].data_ptr() + 4 * w["spans"][name][j][0] for name in ARRAYS}
            n = w["spans"]["p"][j][1]
            rows += struct.pack("<QQQQqq", at["p"], at["g"], at["exp_avg"], at["exp_avg_sq"], n, first)
            pointers.append(at["shadow"])
            first += (n + 4095) // 4096
        w["tables"][kind] = (torch.frombuffer(bytearray(rows), dtype=torch.uint8).to(DEV),
                             torch.tensor(pointers, dtype=torch.int64, device=DEV), len(picks), first, picks)
    assert w["tables"]["all_slices"][2:4] == (24, 4 * 8) and w["tables"]["one_tensor_two_chunks"][2:4] == (1, 2)
    w["scaler"] = torch.zeros(4, dtype=torch.int32, device=DEV)                      # zsv_scaler_state
    w["avg_state"] = torch.zeros(1, dtype=torch.int32, device=DEV)                   # zsv_avg_state
    w["clip"] = torch.zeros(2, dtype=torch.float32, device=DEV)                      # zsv_clip_record
    return w


def _run(w, kind, form, scale=1024.0, steps_done=3, found_inf=0, unscaled=0, clip=0.5, n_averaged=0, decoupled=1):
    """Restore the buffers, launch `form` on table `kind`, and return the five buffers as int32 bit patterns.  Checked on every
    launch: nothing outside a slice of the table changes, and g is not written at all."""
    decay, scaled, avg = form
    table, pointers, count, chunks, picks = w["tables"][kind]
    for name in ARRAYS:
        w["flat"][name].copy_(w["pristine"][name])
    host = torch.zeros(4, dtype=torch.int32)
    host.view(torch.float32)[0] = scale
    host[2], host[3] = found_inf, steps_done
    w["scaler"].copy_(host)
    w["avg_state"].fill_(n_averaged)
    if clip is not None:
        w["clip"].copy_(torch.tensor([7.0, clip]))
    args = [table.data_ptr(), count, chunks, LR, B1, B2, EPS]
    if decay:
        args += [WD, decoupled, w["clip"].data_ptr() if clip is not None else None]
    args += [w["scaler"].data_ptr(), unscaled] if decay and scaled else [w["scaler"].data_ptr()] if scaled else [STEP]
    if avg:
        args += [pointers.data_ptr(), w["avg_state"].data_ptr(), EMA]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(getattr(w["lib"], _name(form))(*args, stream), _name(form))
    out = {name: w["flat"][name].clone().view(torch.int32) for name in ARRAYS}
    for name in ARRAYS:
        before = w["pristine"][name].view(torch.int32)
        touched = torch.zeros_like(w["outside"][name])
        if name != "g" and (avg or name != "shadow"):
            for j in picks:
                start, n = w["spans"][name][j]
                touched[start:start + n] = True
        assert torch.equal(out[name][~touched], before[~touched]), (_name(form), kind, name)
    assert int(w["scaler"][2]) == found_inf and int(w["scaler"][3]) == steps_done and int(w["avg_state"]) == n_averaged
    return out


def _same(a, b, names, what):
    for name in names:
        assert torch.equal(a[name], b[name]), (what, name)


KINDS = ["all_slices", "one_tensor_two_chunks"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("decay,scaled", [(d, s) for d in (False, True) for s in (False, True)])
def test_avg_form_gives_the_bytes_of_its_plain_form(world, kind, decay, scaled):
    """1: p and both moments of an `_avg` launch are those of the plain launch, and with n_averaged == 0 the shadow is the new p.
    A later averaged step (n_averaged == 2) moves the shadow and still leaves the update alone."""
    plain = _run(world, kind, (decay, scaled, False))
    pristine = world["pristine"]["p"].view(torch.int32)
    assert not torch.equal(plain["p"], pristine)                                     # the launch did update something
    first = _run(world, kind, (decay, scaled, True), n_averaged=0)
    _same(first, plain, ("p", "exp_avg", "exp_avg_sq"), "first averaged step")
    for j in world["tables"][kind][4]:
        (sp, n), (ss, _) = world["spans"]["p"][j], world["spans"]["shadow"][j]
        assert torch.equal(first["shadow"][ss:ss + n], first["p"][sp:sp + n]), j
    later = _run(world, kind, (decay, scaled, True), n_averaged=2)
    _same(later, plain, ("p", "exp_avg", "exp_avg_sq"), "later averaged step")
    assert not torch.equal(later["shadow"], first["shadow"])
    assert not torch.equal(later["shadow"], world["pristine"]["shadow"].view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("decay,avg", [(d, a) for d in (False, True) for a in (False, True)])
def test_scaled_forms_write_nothing_on_found_inf(world, kind, decay, avg):
    """2: with found_inf set a scaled launch returns before it touches p, the moments or the shadows."""
    out = _run(world, kind, (decay, True, avg), found_inf=1)
    for name in ARRAYS:
        assert torch.equal(out[name], world["pristine"][name].view(torch.int32)), name


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("avg", [False, True])
def test_grads_unscaled_is_a_scale_of_one(world, kind, avg):
    """4: with scale == 1.0 the adamw scaled forms give the same bytes whether or not they are told the gradients are unscaled."""
    scaled = _run(world, kind, (True, True, avg), scale=1.0, unscaled=0, n_averaged=2)
    unscaled = _run(world, kind, (True, True, avg), scale=1.0, unscaled=1, n_averaged=2)
    _same(scaled, unscaled, ARRAYS, "grads_unscaled")
    assert not torch.equal(scaled["p"], world["pristine"]["p"].view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scaled,avg", [(s, a) for s in (False, True) for a in (False, True)])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["l2", "decoupled"])
def test_a_clip_coefficient_of_one_is_no_clip_record(world, kind, scaled, avg, decoupled):
    """5: a record whose clip_coef is 1.0 gives the bytes of a NULL record; one that holds 0.5 does not."""
    none = _run(world, kind, (True, scaled, avg), clip=None, n_averaged=2, decoupled=decoupled)
    one = _run(world, kind, (True, scaled, avg), clip=1.0, n_averaged=2, decoupled=decoupled)
    half = _run(world, kind, (True, scaled, avg), clip=0.5, n_averaged=2, decoupled=decoupled)
    _same(none, one, ARRAYS, "clip_coef 1.0")
    assert not torch.equal(half["p"], one["p"])
