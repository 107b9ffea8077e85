"""Depthwise Conv3d (groups == channels) on the device: zsv_dwconv3d_fwd / _dgrad / _wgrad through ``ops.conv3d(groups=C)``,
``layers.Conv3d(groups=C)`` and ``torch.ops.zsv.depthwise_conv3d*`` against torch's own ``F.conv3d(groups=C)`` and autograd on the
CPU in fp64 (tests/dwconv_cases.py: the cases, the exact and the bounded check)."""
import pytest
import torch

import dwconv_cases as D
from zeroshotvideoclassification_amd import _lib, layers, ops, torch_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(index, kind, bias=False, relu=False):
    """y, dx, dw, db of case ``index`` through the ctypes path (forward + both gradients of one autograd pass)."""
    case = D.CASES[index]
    x, w, b, dy = (None if t is None else t.to(DEV) for t in D.operands(index, kind, bias))
    x.requires_grad_(True)
    w.requires_grad_(True)
    if b is not None:
        b.requires_grad_(True)
    y = ops.conv3d(x, w, b, case[2], case[3], relu=relu, groups=case[0][1])
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return y, x.grad, w.grad, None if b is None else b.grad


def _compare(index, kind, bias, relu, got):
    ref = D.reference(index, kind, bias, relu)
    y, dx, dw, db = got
    worst = {"y": D.check("y", y, ref["y"], ref["y_bound"], kind), "dx": D.check("dx", dx, ref["dx"], ref["dx_bound"], kind),
             "dw": D.check("dw", dw, ref["dw"], ref["dw_bound"], kind)}
    if kind == "normal":
        for name, g, bound in (("dx", dx, ref["dx_bound"]), ("dw", dw, ref["dw_bound"])):
            assert not bool((g.cpu()[bound == 0] != 0).any()), f"{name}: a voxel nothing touches must be exactly 0"
    if db is not None:
        # the bias gradient is a plain sum of the masked dY over N * To * Ho * Wo values (zsv_channel_sum / zsv_relu_bwd_bias)
        g = D.operands(index, kind, bias)[3].double() * ((ref["z"] > 0) if relu else 1.0)
        n_terms = g.numel() // g.shape[1]
        worst["db"] = D.check("db", db, ref["db"], (n_terms + 2) * D.U * g.abs().sum(dim=(0, 2, 3, 4)), kind)
    print(f"case {index + 1} {kind} bias={bias} relu={relu}: worst error / bound {worst}")


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("index", range(len(D.CASES)), ids=D.IDS)
def test_operator_parity(index, kind):
    """Forward, input gradient and weight gradient of the fourteen cases: bit for bit on small integers, inside the derived
    per-element bound on normal operands."""
    _compare(index, kind, False, False, _run(index, kind))


@pytest.mark.parametrize("kind", ["exact", "normal"])
@pytest.mark.parametrize("index", [0, 3], ids=["case1", "case4"])
def test_bias_and_fused_relu(index, kind):
    """Bias and ReLU in the forward's epilogue; the ReLU mask and the bias gradient in the backward."""
    ref = D.reference(index, kind, True, True)
    if kind == "normal":        # the mask is decided: no pre-activation of the reference lies within the bound of 0
        assert bool((ref["z"].abs() > 4 * ref["y_bound"]).all())
    _compare(index, kind, True, True, _run(index, kind, True, True))


def test_weight_gradient_is_reproducible():
    """Two calls of the weight gradient on case 6 return equal bits (fixed-order sums, no atomics)."""
    first, second = _run(5, "normal")[2], _run(5, "normal")[2]
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))


def _count(monkeypatch, names):
    lib = _lib.load()
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def counted(*a, _n=n, _real=real):
            calls[_n] += 1
            return _real(*a)

        monkeypatch.setattr(lib, n, counted, raising=False)
    return calls


def test_autograd_through_the_layer(monkeypatch):
    """``layers.Conv3d(groups=C)`` with a bias: .grad of input, weight and bias against the fp64 twin; a frozen weight launches
    no weight gradient and gets no .grad; an input that needs no gradient launches no input gradient."""
    torch.manual_seed(3)
    c = 6
    conv = layers.Conv3d(c, c, 3, stride=(1, 2, 2), padding=1, groups=c, bias=True)
    twin = torch.nn.Conv3d(c, c, 3, stride=(1, 2, 2), padding=1, groups=c, bias=True).double()
    twin.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    conv.to(DEV)
    x = torch.randn(2, c, 3, 9, 10)
    dy = torch.randn(2, c, 3, 5, 5)
    x64 = x.double().requires_grad_(True)
    twin(x64).backward(dy.double())
    calls = _count(monkeypatch, ["zsv_dwconv3d_fwd", "zsv_dwconv3d_dgrad", "zsv_dwconv3d_wgrad"])

    xd = x.to(DEV).requires_grad_(True)
    y = conv(xd)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert calls == {"zsv_dwconv3d_fwd": 1, "zsv_dwconv3d_dgrad": 1, "zsv_dwconv3d_wgrad": 1}
    # 27 taps (dx, y) / 150 positions (dw, db) in fp32 against fp64: 1e-5 of the largest value is two decades above either
    for name, got, ref in (("dx", xd.grad, x64.grad), ("dw", conv.weight.grad, twin.weight.grad), ("db", conv.bias.grad, twin.bias.grad)):
        err = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"layer {name}: {err:.2e}")
        assert err < 1e-5, name

    conv.zero_grad(set_to_none=True)
    conv.weight.requires_grad_(False)
    xd = x.to(DEV).requires_grad_(True)
    conv(xd).backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert conv.weight.grad is None and conv.bias.grad is not None and xd.grad is not None
    assert calls == {"zsv_dwconv3d_fwd": 2, "zsv_dwconv3d_dgrad": 2, "zsv_dwconv3d_wgrad": 1}

    conv.weight.requires_grad_(True)
    xd = x.to(DEV)
    conv(xd).backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert xd.grad is None and conv.weight.grad is not None
    assert calls == {"zsv_dwconv3d_fwd": 3, "zsv_dwconv3d_dgrad": 2, "zsv_dwconv3d_wgrad": 2}


def test_link_tags_are_dropped_unarmed():
    """A block input tagged for the fused shortcut gradients reaches a depthwise convolution: the tags are popped, no link is
    armed, and the convolution returns its own input gradient only."""
    x, w, _, dy = (None if t is None else t.to(DEV) for t in D.operands(0, "exact"))
    x.requires_grad_(True)
    link, down = ops.SkipLink(), ops.DownLink((1, 1, 1))
    x._zsv_skip_link, x._zsv_down_link, x._zsv_down_src = link, down, down
    y = ops.conv3d(x, w, None, 1, 1, groups=x.shape[1])
    assert not any(k.startswith("_zsv_") for k in x.__dict__)
    assert not link.armed and not down.armed
    y.backward(dy)
    D.check("dx", x.grad, D.reference(0, "exact")["dx"], None, "exact")


@pytest.mark.parametrize("index", [0, 3], ids=["case1", "case4"])
def test_torch_ops_match_the_ctypes_path(index):
    """``torch.ops.zsv.depthwise_conv3d`` (forward and all three gradients) and the three plain operators give the bits of the
    ctypes path."""
    ns = torch_ops.load()
    case = D.CASES[index]
    s, p = list(case[2]), list(case[3])
    want_y, want_dx, want_dw, want_db = _run(index, "normal", bias=True)
    x, w, b, dy = (t.to(DEV) for t in D.operands(index, "normal", True))
    x.requires_grad_(True)
    w.requires_grad_(True)
    b.requires_grad_(True)
    y = ns.depthwise_conv3d(x, w, b, s, p)
    y.backward(dy)
    torch.cuda.synchronize()
    bits = lambda t: t.detach().contiguous().view(torch.int32)
    for name, got, want in (("y", y, want_y), ("dx", x.grad, want_dx), ("dw", w.grad, want_dw)):
        assert torch.equal(bits(got), bits(want)), name
    # (the operator's bias gradient is aten's sum, the ctypes path's is zsv_channel_sum: close, not the same bits)
    assert float((b.grad - want_db).abs().max()) <= 1e-5 * float(want_db.abs().max())
    with torch.no_grad():
        assert torch.equal(bits(ns.depthwise_conv3d_fwd(x, w, b, s, p, False)), bits(want_y))
        assert torch.equal(bits(ns.depthwise_conv3d_dgrad(dy, w, list(x.shape), s, p)), bits(want_dx))
        assert torch.equal(bits(ns.depthwise_conv3d_wgrad(x, dy, list(w.shape), s, p)), bits(want_dw))
        relu = ns.depthwise_conv3d_fwd(x, w, b, s, p, True)
        assert torch.equal(bits(relu), bits(torch.relu(want_y)))
    with pytest.raises(RuntimeError):
        ns.depthwise_conv3d_fwd(x, w[:, :, :1].repeat(1, 1, 5, 1, 1).contiguous(), None, s, [2, 1, 1], False)     # kernel 5
