"""Host side of ``optim.FusedLARS`` / ``optim.FusedLAMB``: the C ABI surface of csrc/layerwise.hip and its refusals, constructor
validation, ``optim.layerwise_groups`` and the fp64 restatement of the rules on its own exact cases.  Nothing here touches a device."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import layerwise_cases as C
from zeroshotvideoclassification_amd import _lib, network, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zsv_layerwise_workspace_bytes", "zsv_lars_norms", "zsv_lamb_moments", "zsv_layerwise_finalize", "zsv_lars_multi",
               "zsv_lamb_multi")
OK, BAD_SHAPE, NULL, WORKSPACE = 0, 1, 2, 3                   # include/zsv_hip.h


def _ps():
    return [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]


def test_new_symbols_are_declared_exported_and_have_prototypes():
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    declared = set(re.findall(r"\b(zsv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.SIGNATURES, sym
        assert getattr(lib, sym).argtypes == _lib.SIGNATURES[sym][1], sym
    assert "typedef struct zsv_layer_record" in header
    makefile = open(os.path.join(ROOT, "zeroshotvideoclassification_amd", "csrc", "Makefile")).read()
    assert "layerwise.hip" in makefile
    # what existed keeps its prototype
    assert len(_lib.SIGNATURES["zsv_sgd_multi"][1]) == 17 and len(_lib.SIGNATURES["zsv_adamw_multi_scaled"][1]) == 13


def test_workspace_query():
    lib = _lib.load()
    assert lib.zsv_layerwise_workspace_bytes(0, 1) == 0 and lib.zsv_layerwise_workspace_bytes(1, 0) == 0
    assert lib.zsv_layerwise_workspace_bytes(7, 3) == 48 + 56          # 3 records of 12 bytes rounded up to 16, 8 bytes per chunk
    assert lib.zsv_layerwise_workspace_bytes(1, 4) == 48 + 8


def _workspace_calls(lib, table, ws, nbytes, count=3, chunks=5, chunk_offset=0, tensor_offset=0, all_count=3):
    place = (table, count, chunks, chunk_offset, tensor_offset, all_count, ws, nbytes)
    return [lib.zsv_lars_norms(*place, None, None),
            lib.zsv_lamb_moments(*place, 0.9, 0.999, 1e-6, 0.01, None, None, 0, 1, None),
            lib.zsv_layerwise_finalize(*place, 0, 1, 1e-3, 1e-4, 1e-8, 0.0, None, None, 0, None),
            lib.zsv_layerwise_finalize(*place, 1, 1, 0.0, 0.0, 0.0, 0.0, None, None, 0, None)]


def test_refusals_are_decided_before_any_launch():
    """NULL first, then the shape, then the size of the workspace.  The pointers are host addresses: nothing reaches a launch."""
    lib = _lib.load()
    host = (ctypes.c_char * 256)()
    there = ctypes.addressof(host)
    need = lib.zsv_layerwise_workspace_bytes(5, 3)
    assert _workspace_calls(lib, None, there, need) == [NULL] * 4
    assert _workspace_calls(lib, there, None, need) == [NULL] * 4
    assert _workspace_calls(lib, None, None, 0) == [NULL] * 4
    assert _workspace_calls(lib, there, there, need - 1) == [WORKSPACE] * 4
    assert _workspace_calls(lib, there, there, 0) == [WORKSPACE] * 4
    # a table placed further into the workspace needs the chunks before it as well
    assert _workspace_calls(lib, there, there, need, chunk_offset=1) == [WORKSPACE] * 4
    assert _workspace_calls(lib, there, there, need, count=0) == [BAD_SHAPE] * 4
    assert _workspace_calls(lib, there, there, need, chunks=0) == [BAD_SHAPE] * 4
    assert _workspace_calls(lib, there, there, need, tensor_offset=1) == [BAD_SHAPE] * 4           # 1 + 3 records > all_count
    assert _workspace_calls(lib, there, there, need, chunk_offset=-1) == [BAD_SHAPE] * 4
    place = (there, 3, 5, 0, 0, 3, there, need)
    assert lib.zsv_layerwise_finalize(*place, 0, 1, 0.0, 1e-4, 1e-8, 0.0, None, None, 0, None) == BAD_SHAPE     # trust_coefficient 0
    assert lib.zsv_lamb_moments(*place, 1.0, 0.999, 1e-6, 0.01, None, None, 0, 1, None) == BAD_SHAPE            # beta1 == 1
    assert lib.zsv_lamb_moments(*place, 0.9, 0.999, 1e-6, 0.01, None, None, 0, 0, None) == BAD_SHAPE            # step 0 without a scaler
    # the apply launches: table and records, then shadows and averaging state together
    lars = lambda table, records, shadows=None, avg=None, lr=0.1, nesterov=0, momentum=0.9: lib.zsv_lars_multi(  # noqa: E731
        table, 3, 5, records, lr, momentum, 0.0, nesterov, 1e-4, 0, None, None, 0, 0, shadows, avg, 0.5, None)
    lamb = lambda table, records, shadows=None, avg=None, lr=1e-3, step=1: lib.zsv_lamb_multi(                  # noqa: E731
        table, 3, 5, records, lr, 0.9, 0.999, 1e-6, 0.01, None, step, shadows, avg, 0.5, None)
    for call in (lars, lamb):
        assert call(None, there) == NULL and call(there, None) == NULL
        assert call(there, there, shadows=there) == NULL and call(there, there, avg=there) == NULL
        assert call(there, there, lr=-1.0) == BAD_SHAPE and call(there, there, lr=float("nan")) == BAD_SHAPE
    assert lars(there, there, nesterov=1, momentum=0.0) == BAD_SHAPE
    assert lamb(there, there, step=0) == BAD_SHAPE


@pytest.mark.parametrize("kw", [
    {"lr": -0.1}, {"eps": -1e-8}, {"weight_decay": -1e-4}, {"trust_coefficient": 0.0}, {"trust_coefficient": -1.0},
    {"nesterov": True, "momentum": 0.0}, {"nesterov": True, "dampening": 0.5}, {"momentum": -0.5}, {"max_grad_norm": 0.0},
    {"lr": float("nan")}, {"trust_coefficient": float("inf")},
])
def test_lars_constructor_validation(kw):
    with pytest.raises(ValueError):
        optim.FusedLARS(_ps(), **dict({"lr": 0.1}, **kw))


@pytest.mark.parametrize("kw", [
    {"lr": -0.1}, {"eps": -1e-8}, {"weight_decay": -1e-4}, {"trust_clip": 0.0}, {"trust_clip": -1.0}, {"betas": (1.0, 0.999)},
    {"betas": (0.9, -0.1)}, {"max_grad_norm": -1.0}, {"trust_clip": float("nan")},
])
def test_lamb_constructor_validation(kw):
    with pytest.raises(ValueError):
        optim.FusedLAMB(_ps(), **kw)


def test_signatures_defaults_and_group_options():
    lars = inspect.signature(optim.FusedLARS.__init__)
    assert list(lars.parameters)[1:] == ["params", "lr", "momentum", "dampening", "nesterov", "weight_decay", "trust_coefficient", "eps",
                                         "maximize", "max_grad_norm", "grad_buckets"]
    assert lars.parameters["lr"].default is inspect.Parameter.empty
    assert [lars.parameters[k].default for k in ("momentum", "dampening", "nesterov", "weight_decay", "trust_coefficient", "eps",
                                                 "maximize", "max_grad_norm", "grad_buckets")] == [0.9, 0, False, 1e-4, 1e-3, 1e-8, False, None, None]
    lamb = inspect.signature(optim.FusedLAMB.__init__)
    assert list(lamb.parameters)[1:] == ["params", "lr", "betas", "eps", "weight_decay", "trust_clip", "max_grad_norm", "grad_buckets"]
    assert [lamb.parameters[k].default for k in ("lr", "betas", "eps", "weight_decay", "trust_clip")] == [1e-3, (0.9, 0.999), 1e-6, 0.01, None]
    for cls in (optim.FusedLARS, optim.FusedLAMB):
        assert issubclass(cls, optim._FusedOptimizer) and issubclass(cls, torch.optim.Optimizer)
    a, b = _ps()
    opt = optim.FusedLARS([{"params": [a]}, {"params": [b], "adapt": False, "weight_decay": 0.0}], lr=0.1)
    assert [g["adapt"] for g in opt.param_groups] == [True, False]
    with pytest.raises(ValueError):
        optim.FusedLARS([{"params": [a]}, {"params": [b], "trust_coefficient": 0.0}], lr=0.1)
    with pytest.raises(ValueError):
        optim.FusedLAMB([{"params": [a]}, {"params": [b], "trust_clip": -2.0}])
    with pytest.raises(RuntimeError, match="layer_norms is available after step"):
        opt.layer_norms
    opt.param_groups[0]["trust_coefficient"] = -1.0            # the groups are editable: checked again at step()
    a.grad = torch.ones(3)
    with pytest.raises(ValueError):
        opt.step()
    # CPU parameters are refused at step, as FusedSGD refuses them: there is no CPU fallback
    opt = optim.FusedLAMB(_ps())
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


@pytest.mark.parametrize("base,layerwise", [(optim.FusedSGD, optim.FusedLARS), (optim.FusedAdam, optim.FusedLAMB)],
                         ids=["sgd-lars", "adam-lamb"])
def test_a_layerwise_optimizer_has_every_attribute_of_the_one_it_inherits(base, layerwise):
    """The constructors share one set-up: a field the inherited optimizer creates exists in the layer-wise one."""
    missing = set(vars(base(_ps(), lr=0.1))) - set(vars(layerwise(_ps(), lr=0.1)))
    assert not missing, sorted(missing)


def test_state_dicts_round_trip_and_an_adam_state_loads_into_lamb():
    adam = optim.FusedAdam(_ps(), lr=3e-4, weight_decay=0.02)
    lamb = optim.FusedLAMB([{"params": _ps(), "adapt": False}], lr=1e-3, trust_clip=10.0)
    lamb.load_state_dict(adam.state_dict())
    g = lamb.param_groups[0]
    assert g["lr"] == 3e-4 and g["weight_decay"] == 0.02 and g["adapt"] is False and g["trust_clip"] == 10.0
    again = optim.FusedLAMB(_ps())
    again.load_state_dict(lamb.state_dict())
    assert again.param_groups[0]["adapt"] is False and again.param_groups[0]["trust_clip"] == 10.0
    sgd = torch.optim.SGD(_ps(), lr=0.3, momentum=0.8)
    lars = optim.FusedLARS(_ps(), lr=0.1, trust_coefficient=0.5)
    lars.load_state_dict(sgd.state_dict())
    g = lars.param_groups[0]
    assert g["lr"] == 0.3 and g["momentum"] == 0.8 and g["trust_coefficient"] == 0.5 and g["adapt"] is True and g["eps"] == 1e-8
    back = optim.FusedLARS(_ps(), lr=9.0)
    back.load_state_dict(lars.state_dict())
    assert back.param_groups[0]["trust_coefficient"] == 0.5 and back.param_groups[0]["lr"] == 0.3


def test_layerwise_groups_on_the_model():
    model = network.get_network(SimpleNamespace(network="r2plus1d_18", fixconvs=False, nopretrained=False))
    frozen = next(p for p in model.parameters() if p.dim() < 2)
    frozen.requires_grad_(False)
    groups = optim.layerwise_groups(model, 1e-4)
    assert len(groups) == 2
    assert groups[0]["adapt"] is True and groups[0]["weight_decay"] == 1e-4
    assert groups[1]["adapt"] is False and groups[1]["weight_decay"] == 0
    first, second = ({id(p) for p in g["params"]} for g in groups)
    assert len(first) == len(groups[0]["params"]) and len(second) == len(groups[1]["params"]) and not first & second   # nothing twice
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert first == {id(p) for p in trainable if p.dim() >= 2} and first
    assert second == {id(p) for p in trainable if p.dim() < 2} and second
    assert id(frozen) not in first | second
    optim.FusedLARS(groups, lr=0.1)                           # they are what the constructors take
    optim.FusedLAMB(optim.layerwise_groups(model, 0.01))


@pytest.mark.parametrize("n", C.EXACT_SIZES)
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_the_restatement_reproduces_the_exact_cases(kind, n):
    """fp64 and fp32 agree value for value: every intermediate is a power of two."""
    ps, grads = C.exact_case(n)
    (p64, rec64, _), = C.run(kind, ps, grads, C.exact_groups(kind))
    (p32, rec32, _), = C.run(kind, ps, grads, C.exact_groups(kind), dtype=torch.float32)
    want = C.EXACT_AFTER[kind]
    assert torch.equal(p64[0], torch.full((n,), want, dtype=torch.float64))
    assert torch.equal(p32[0].double(), p64[0]) and rec32 == rec64
    pn = 2.0 * n ** 0.5
    assert rec64 == [(pn, pn / 2, 2.0 ** -9 if kind == "lars" else 2.0)]


def test_the_restatement_on_the_shared_cases():
    """The edge cases are what the module says: a zero tensor and a zero gradient take ratio 1; adapt=False takes ratio 1; the
    i-th of the many tensors has norm i + 1."""
    for kind in ("lars", "lamb"):
        first = C.reference(kind, "sizes")[0][1]
        assert first[C.ZERO_PARAM][0] == 0.0 and first[C.ZERO_PARAM][2] == 1.0
        if kind == "lars":
            assert first[C.ZERO_GRAD][1] == 0.0 and first[C.ZERO_GRAD][2] == 1.0
        else:                                                  # u = wd * p: r = |p| / (wd |p|)
            assert abs(first[C.ZERO_GRAD][2] * C.LAMB_HP["weight_decay"] - 1.0) < 1e-12
        assert all(r != 1.0 for i, (_, _, r) in enumerate(first) if i not in (C.ZERO_PARAM, C.ZERO_GRAD))
        many = C.reference(kind, "many")
        assert len(many) == C.STEPS and len(many[0][1]) == C.MANY
        for i, (pn, _, r) in enumerate(many[0][1]):
            assert abs(pn - (i + 1)) < 1e-6 * (i + 1)
            assert (r == 1.0) == (i >= C.MANY_ADAPT)
