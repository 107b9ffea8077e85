"""Host side of ``optim.FusedSGD``: the C ABI surface of ``zsv_sgd_multi``, constructor validation against ``torch.optim.SGD``'s,
the "no CPU fallback" error and the state-dict interchange with ``torch.optim.SGD``.  Nothing here touches a device."""
import inspect
import os
import re

import pytest
import torch

from zeroshotvideoclassification_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZSV_E_BAD_SHAPE, ZSV_E_NULL = 1, 2
KEYS = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize")


def _ps():
    return [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]


def test_sgd_multi_is_declared_bound_and_checks_its_arguments():
    """1: one entry point, declared in the header, bound with its prototype; NULL table and count <= 0 are refused before any
    launch."""
    P, i32, i64, f32, f64 = _lib._P, _lib.c_int32, _lib.c_int64, _lib.c_float, _lib.c_double
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    declared = set(re.findall(r"\b(zsv_[a-z0-9_]+)\s*\(", header))
    assert "zsv_sgd_multi" in declared
    assert [s for s in declared if s.startswith("zsv_sgd")] == ["zsv_sgd_multi"]          # optional features are NULL-able pointers
    res, args = _lib.SIGNATURES["zsv_sgd_multi"]
    assert res is _lib.c_int
    # table, count, total_chunks | lr, momentum, dampening, nesterov, weight_decay, maximize | clip | scaler state, grads_unscaled,
    # first_step | shadows, avg state, ema_weight | stream
    assert args == [P, i32, i64, f64, f32, f32, i32, f64, i32, P, P, i32, i32, P, P, f32, P]
    proto = re.search(r"int zsv_sgd_multi\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(args)
    for word in ("const zsv_adam_tensor* table_device", "double lr", "float momentum", "float dampening", "int32_t nesterov",
                 "double weight_decay", "int32_t maximize", "const zsv_clip_record* clip_device",
                 "const zsv_scaler_state* state_device", "int32_t grads_unscaled", "float* const* shadows_device",
                 "const zsv_avg_state* avg_state_device", "float ema_weight", "void* stream"):
        assert word in " ".join(proto.split()), word
    lib = _lib.load()
    tail = (None, None, 0, 0, None, None, 0.0, None)
    fake = 0x1000                                     # never dereferenced: every call below is refused on the host
    assert lib.zsv_sgd_multi(None, 1, 1, 1e-3, 0.9, 0.0, 0, 0.0, 0, *tail) == ZSV_E_NULL
    assert lib.zsv_sgd_multi(fake, 0, 1, 1e-3, 0.9, 0.0, 0, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE
    assert lib.zsv_sgd_multi(fake, -3, 1, 1e-3, 0.9, 0.0, 0, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE
    assert lib.zsv_sgd_multi(fake, 1, 0, 1e-3, 0.9, 0.0, 0, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE
    assert lib.zsv_sgd_multi(fake, 1, 1, -1e-3, 0.9, 0.0, 0, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, -0.9, 0.0, 0, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, 0.9, 0.0, 0, -0.1, 0, *tail) == ZSV_E_BAD_SHAPE
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, 0.0, 0.0, 1, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE       # nesterov without momentum
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, 0.9, 0.5, 1, 0.0, 0, *tail) == ZSV_E_BAD_SHAPE       # nesterov with dampening
    # shadows without an averaging state (and the reverse)
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, 0.9, 0.0, 0, 0.0, 0, None, None, 0, 0, fake, None, 0.5, None) == ZSV_E_NULL
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, 0.9, 0.0, 0, 0.0, 0, None, None, 0, 0, None, fake, 0.5, None) == ZSV_E_NULL
    assert lib.zsv_sgd_multi(fake, 1, 1, 1e-3, 0.9, 0.0, 0, 0.0, 0, None, None, 0, 0, fake, fake, 1.5, None) == ZSV_E_BAD_SHAPE


@pytest.mark.parametrize("kw", [
    {"lr": -1e-3}, {"momentum": -0.5}, {"weight_decay": -0.1},
    {"nesterov": True}, {"nesterov": True, "momentum": 0.9, "dampening": 0.1}, {"nesterov": True, "momentum": 0.0},
])
def test_constructor_validation_is_torchs(kw):
    """2: the same bad arguments, the same exception type and message."""
    with pytest.raises(ValueError) as want:
        torch.optim.SGD(_ps(), **kw)
    with pytest.raises(ValueError) as got:
        optim.FusedSGD(_ps(), **kw)
    assert str(got.value) == str(want.value)


def test_signature_groups_and_more_validation():
    sig = inspect.signature(optim.FusedSGD.__init__)
    assert list(sig.parameters)[1:] == ["params", "lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize",
                                        "max_grad_norm", "grad_buckets"]
    want = inspect.signature(torch.optim.SGD.__init__).parameters
    for name in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert sig.parameters[name].default == want[name].default, name
        assert sig.parameters[name].kind == want[name].kind, name
    assert issubclass(optim.FusedSGD, torch.optim.Optimizer)
    a, b = _ps()
    opt = optim.FusedSGD([{"params": [a], "momentum": 0.5, "dampening": 0.5}, {"params": [b], "lr": 0.3, "nesterov": True}], lr=0.1,
                         momentum=0.9, weight_decay=1e-4, max_grad_norm=2)
    assert [g["lr"] for g in opt.param_groups] == [0.1, 0.3]
    assert [g["momentum"] for g in opt.param_groups] == [0.5, 0.9]
    assert [g["dampening"] for g in opt.param_groups] == [0.5, 0]
    assert [g["nesterov"] for g in opt.param_groups] == [False, True]
    assert opt.max_grad_norm == 2.0
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        opt.grad_norm                                          # nothing stepped yet
    for bad in ({"max_grad_norm": 0.0}, {"max_grad_norm": float("nan")}, {"lr": float("inf")}, {"momentum": float("nan")}):
        with pytest.raises(ValueError):
            optim.FusedSGD(_ps(), **bad)
    with pytest.raises(ValueError, match="Nesterov"):          # per group as well
        optim.FusedSGD([{"params": [a]}, {"params": [b], "nesterov": True}], lr=0.1)


def test_cpu_parameters_are_refused_at_step():
    """3: no CPU fallback."""
    ps = _ps()
    opt = optim.FusedSGD(ps, lr=0.1, momentum=0.9)
    opt.step()                                                 # no gradients: nothing to do, nothing to refuse
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="FusedSGD needs contiguous fp32 parameters on a HIP device \\(no CPU fallback\\)"):
        opt.step()
    for p, q in zip(ps, before):
        assert torch.equal(p.detach(), q)


def _groups(opt):
    return [{k: g[k] for k in KEYS + ("params",)} for g in opt.state_dict()["param_groups"]]


def test_state_dict_interchanges_with_torch_sgd():
    """4: a fresh FusedSGD's state dict loads into torch.optim.SGD, and torch's loads back, with equal groups; a torch state with
    momentum buffers arrives as ``momentum_buffer`` entries and marks the optimizer as past its first step."""
    a, b = _ps()
    groups = [{"params": [a], "momentum": 0.5, "dampening": 0.5, "weight_decay": 0.25},
              {"params": [b], "lr": 0.3, "nesterov": True, "maximize": True}]
    fused = optim.FusedSGD(groups, lr=0.1, momentum=0.9)
    sd = fused.state_dict()
    assert sd["state"] == {}
    for g in sd["param_groups"]:
        assert set(KEYS) <= set(g)
    want = _groups(fused)
    ref = torch.optim.SGD([{"params": [q]} for q in _ps()], lr=7.0)
    ref.load_state_dict(sd)
    assert _groups(ref) == want
    back = optim.FusedSGD([{"params": [a]}, {"params": [b]}], lr=9.0)
    back.load_state_dict(ref.state_dict())
    assert _groups(back) == want
    assert back._started is False                              # no buffers: the next step is still the first

    # torch takes a step on the CPU; its buffers load into FusedSGD under torch's own key
    for p in (q for g in ref.param_groups for q in g["params"]):
        p.grad = torch.full_like(p, 0.5)
    ref.step()
    back.load_state_dict(ref.state_dict())
    bufs = [back.state[p]["momentum_buffer"] for p in (a, b)]
    for got, p in zip(bufs, (q for g in ref.param_groups for q in g["params"])):
        assert torch.equal(got, ref.state[p]["momentum_buffer"])
    assert back._started is True
    again = torch.optim.SGD([{"params": [a]}, {"params": [b]}], lr=0.1)
    again.load_state_dict(back.state_dict())
    assert torch.equal(again.state[a]["momentum_buffer"], bufs[0]) and _groups(again) == want
    # momentum == 0: torch stores `momentum_buffer: None`; nothing is kept for it here
    plain = torch.optim.SGD(_ps(), lr=0.1)
    for p in plain.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    plain.step()
    mine = optim.FusedSGD(_ps(), lr=0.2)
    mine.load_state_dict(plain.state_dict())
    assert all("momentum_buffer" not in st for st in mine.state.values()) and mine._started is False
    assert mine.param_groups[0]["lr"] == 0.1


def test_scaler_and_average_still_refuse_other_optimizers():
    """5: LossScaler.step / unscale_ and WeightAverage accept the fused optimizers only, with the messages they always had.  (The type
    check comes before anything that needs a device, so it runs on a bare LossScaler.)"""
    ref = torch.optim.SGD(_ps(), lr=0.1, momentum=0.9)
    scaler = object.__new__(optim.LossScaler)
    with pytest.raises(RuntimeError, match="LossScaler.step drives optim.FusedAdam"):
        scaler.step(ref)
    with pytest.raises(RuntimeError, match="LossScaler.unscale_ drives optim.FusedAdam"):
        scaler.unscale_(ref)
    with pytest.raises(TypeError, match="WeightAverage averages inside optim.FusedAdam's update launch; got SGD"):
        optim.WeightAverage(ref)
    # a FusedSGD passes the type check and is refused for its CPU parameters instead
    with pytest.raises(RuntimeError, match="FusedSGD needs contiguous fp32 parameters on a HIP device"):
        optim.WeightAverage(optim.FusedSGD(_ps(), lr=0.1))
    assert issubclass(optim.FusedSGD, optim._FusedOptimizer) and issubclass(optim.FusedAdam, optim._FusedOptimizer)
