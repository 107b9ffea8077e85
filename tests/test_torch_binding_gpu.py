"""The torch-extension layer (csrc/torch_binding.cpp, `torch.ops.zsv.*`) against the ctypes binding of the same C ABI (bit for bit:
both call the same entry points) and against torch CPU fp64."""
import pytest
import torch

from zeroshotvideoclassification_amd import ops, torch_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [
    # name, N, Cin, (T, H, W), Cout, kernel, stride, padding
    ("spatial_s1", 2, 16, (4, 28, 28), 45, (1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ("temporal_s1", 2, 45, (4, 14, 14), 32, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ("spatial_s2", 2, 16, (2, 28, 28), 40, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("full_333", 1, 8, (4, 12, 12), 24, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ("pointwise_s2", 2, 16, (4, 8, 8), 32, (1, 1, 1), (2, 2, 2), (0, 0, 0)),
]


def close(a, ref, rtol=2e-5, what=""):
    a = a.detach().double().cpu()
    err = (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    assert err <= rtol, f"{what}: max err {err:.3e} of the range"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv3d_operator(case):
    name, n, cin, (t, h, w), cout, k, s, p = case
    ns = torch_ops.load()
    g = torch.Generator().manual_seed(len(name) + 7 * cin)
    x = torch.randn(n, cin, t, h, w, generator=g)
    wt = torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5
    b = torch.randn(cout, generator=g)
    xr, wr, br = (v.double().requires_grad_() for v in (x, wt, b))
    yr = torch.nn.functional.conv3d(xr, wr, br, s, p)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())

    xd, wd, bd = (v.to(DEV).requires_grad_() for v in (x, wt, b))
    y = ns.conv3d(xd, wd, bd, list(s), list(p))
    y.backward(gy.to(DEV))
    close(y, yr.detach(), what="torch.ops.zsv.conv3d forward")
    close(xd.grad, xr.grad, what="input gradient")
    close(wd.grad, wr.grad, what="weight gradient")
    close(bd.grad, br.grad, what="bias gradient")

    # the ctypes binding of the same entry points: identical bits
    xc, wc = x.to(DEV).requires_grad_(), wt.to(DEV).requires_grad_()
    yc = ops.conv3d(xc, wc, None, s, p)
    yc.backward(gy.to(DEV))
    y0 = ns.conv3d_fwd(x.to(DEV), wt.to(DEV), None, list(s), list(p), False)
    assert torch.equal(y0, yc.detach()), "forward differs between the two bindings"
    assert torch.equal(ns.conv3d_dgrad(gy.to(DEV), wt.to(DEV), list(x.shape), list(s), list(p)), xc.grad)
    assert torch.equal(ns.conv3d_wgrad(x.to(DEV), gy.to(DEV), list(wt.shape), list(s), list(p)), wc.grad)
    with torch.inference_mode():
        assert torch.equal(ns.conv3d(x.to(DEV), wt.to(DEV), None, list(s), list(p)), y0)


@pytest.mark.parametrize("relu", [False, True])
def test_batch_norm_relu_operator(relu):
    ns = torch_ops.load()
    g = torch.Generator().manual_seed(11 + relu)
    x = torch.randn(3, 24, 4, 10, 12, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g) * 0.1
    gy = torch.randn(x.shape, generator=g)
    bn = torch.nn.BatchNorm3d(24).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xr = x.double().requires_grad_()
    yr = bn(xr)
    if relu:
        yr = torch.relu(yr)
    yr.backward(gy.double())

    xd = x.to(DEV).requires_grad_()
    gd, bd = gamma.to(DEV).requires_grad_(), beta.to(DEV).requires_grad_()
    rm, rv = torch.zeros(24, device=DEV), torch.ones(24, device=DEV)
    y = ns.batch_norm_relu(xd, gd, bd, rm, rv, 0.1, 1e-5, relu)
    y.backward(gy.to(DEV))
    close(y, yr.detach(), what="batch_norm_relu forward")
    close(xd.grad, xr.grad, rtol=1e-4, what="dx")
    close(gd.grad, bn.weight.grad, rtol=1e-4, what="dgamma")
    close(bd.grad, bn.bias.grad, rtol=1e-4, what="dbeta")
    close(rm, bn.running_mean, what="running_mean")
    close(rv, bn.running_var, what="running_var")


def test_errors_name_the_status():
    ns = torch_ops.load()
    with pytest.raises(RuntimeError, match="channels"):
        ns.conv3d_fwd(torch.zeros(1, 3, 2, 4, 4, device=DEV), torch.zeros(4, 5, 1, 3, 3, device=DEV), None, [1, 1, 1], [0, 1, 1], False)
    with pytest.raises(RuntimeError, match="contiguous"):
        ns.conv3d_fwd(torch.zeros(1, 3, 2, 4, 8, device=DEV)[..., ::2], torch.zeros(4, 3, 1, 3, 3, device=DEV), None, [1, 1, 1], [0, 1, 1], False)


def test_relu_and_linear_operators():
    """`torch.ops.zsv.relu` / `linear` (network.MLP, network.py:603-617) against torch CPU fp64 and the ctypes binding."""
    ns = torch_ops.load()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(22, 512, generator=g)
    w = torch.randn(300, 512, generator=g) / 512 ** 0.5
    b = torch.randn(300, generator=g)
    gy = torch.randn(22, 300, generator=g)
    xr, wr, br = (v.double().requires_grad_() for v in (x, w, b))
    yr = torch.relu(torch.nn.functional.linear(xr, wr, br))
    yr.backward(gy.double())
    xd, wd, bd = (v.to(DEV).requires_grad_() for v in (x, w, b))
    y = ns.relu(ns.linear(xd, wd, bd))
    y.backward(gy.to(DEV))
    close(y, yr.detach(), what="relu(linear) forward")
    close(xd.grad, xr.grad, what="linear input gradient")
    close(wd.grad, wr.grad, what="linear weight gradient")
    close(bd.grad, br.grad, what="linear bias gradient")
    xc, wc, bc = (v.to(DEV).requires_grad_() for v in (x, w, b))
    yc = ops.linear(xc, wc, bc, relu=True)
    assert torch.equal(ns.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), True), yc.detach()), "fused linear + relu differs between the bindings"


# ---- what the layer refuses ---------------------------------------------------------------------------------------------------------
# Every wrong operand below is too LARGE, of the wrong dtype or a wrong list entry: were a check missing, the kernel would still read
# inside the tensors it was handed.

def _conv_operands():
    x, w = torch.zeros(1, 3, 2, 6, 6, device=DEV), torch.zeros(4, 3, 1, 3, 3, device=DEV)
    dy = torch.zeros(1, 4, 2, 6, 6, device=DEV)
    return x, w, dy


@pytest.mark.parametrize("stride,padding,word", [([1, 0, 1], [0, 1, 1], r"stride\[1\] = 0"), ([1, 1, 1], [0, -1, 1], r"padding\[1\] = -1")],
                         ids=["stride_0", "padding_-1"])
def test_convolution_operators_refuse_bad_strides_and_paddings(stride, padding, word):
    """A stride of 0 used to divide by zero in the descriptor (SIGFPE: the process dies), a negative padding went to the kernels."""
    ns = torch_ops.load()
    x, w, dy = _conv_operands()
    with pytest.raises(RuntimeError, match=word):
        ns.conv3d_fwd(x, w, None, stride, padding, False)
    with pytest.raises(RuntimeError, match=word):
        ns.conv3d_dgrad(dy, w, list(x.shape), stride, padding)
    with pytest.raises(RuntimeError, match=word):
        ns.conv3d_wgrad(x, dy, list(w.shape), stride, padding)
    with pytest.raises(RuntimeError, match=word):
        ns.conv3d(x, w, None, stride, padding)


def test_sizes_that_do_not_fit_int32_are_refused_by_name():
    """`w_sizes[0] = 2**32 + 4` used to be narrowed to Cout = 4 and accepted against a 4-channel dy."""
    ns = torch_ops.load()
    x, w, dy = _conv_operands()
    with pytest.raises(RuntimeError, match=r"w_sizes\[0\] = 4294967300"):
        ns.conv3d_wgrad(x, dy, [2 ** 32 + 4, 3, 1, 3, 3], [1, 1, 1], [0, 1, 1])
    with pytest.raises(RuntimeError, match=r"x_sizes\[0\] = 4294967297"):
        ns.conv3d_dgrad(dy, w, [2 ** 32 + 1, 3, 2, 6, 6], [1, 1, 1], [0, 1, 1])
    with pytest.raises(RuntimeError, match=r"padding\[0\] = 4294967296"):
        ns.conv3d_fwd(x, w, None, [1, 1, 1], [2 ** 32, 1, 1], False)


BN_BWD_OPERANDS = ["dy", "y", "weight", "bias", "save_mean", "save_invstd"]


@pytest.mark.parametrize("which", BN_BWD_OPERANDS)
def test_bn_train_bwd_checks_every_operand(which):
    """`bn_train_bwd` checked nothing about six of its seven operands.  Each in turn one channel (the per-channel ones) or one
    voxel (dy, y) too large, and once as float64; the refusal names it."""
    ns = torch_ops.load()
    c = 5
    shape = (2, c, 2, 3, 4)
    good = {"dy": torch.zeros(shape, device=DEV), "x": torch.zeros(shape, device=DEV), "y": torch.zeros(shape, device=DEV)}
    good.update({k: torch.ones(c, device=DEV) for k in BN_BWD_OPERANDS[2:]})
    order = ["dy", "x", "y"] + BN_BWD_OPERANDS[2:]
    big = torch.zeros(2, c, 2, 3, 5, device=DEV) if which in ("dy", "y") else torch.ones(c + 1, device=DEV)
    for bad, word in ((big, rf"(?<![a-z_]){which} has shape"), (good[which].double(), rf"(?<![a-z_]){which} must be float32")):
        args = dict(good)
        args[which] = bad
        with pytest.raises(RuntimeError, match=word):
            ns.bn_train_bwd(*(args[k] for k in order), True)


# ---- the plain backward operators, called directly ------------------------------------------------------------------------------------
def _lib_call(fn, *args):
    from zeroshotvideoclassification_amd import _lib
    _lib.check(getattr(_lib.load(), fn)(*args), fn)


def _same(got, want, what):
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, want):
        assert torch.equal(a, b), f"{what}: {name} differs between the two bindings"


BN_EDGE_CASES = [(4, 7, (1, 1, 1)), (2, 130, (2, 7, 7)), (2, 5, (3, 4, 4))]          # of tests/test_ops_gpu.py's BN_CASES


def _bn_case(n, c, sp, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, *sp, generator=g) * 2 + 0.5
    return (x, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.5,
            torch.rand(c, generator=g) * 2 + 0.5, torch.randn(x.shape, generator=g))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n,c,sp", BN_EDGE_CASES)
def test_bn_backward_operators_called_directly(n, c, sp, relu):
    """`bn_train_bwd` / `bn_eval_bwd` as plain operators: the ctypes call of the same entry point bit for bit, torch CPU fp64
    within 1e-4 of the range.  (The ReLU mask of the reference is the fp32 forward's: an fp64 one flips elements within an ulp of 0.)"""
    from zeroshotvideoclassification_amd import _lib
    ns = torch_ops.load()
    lib = _lib.load()
    x, gamma, beta, rm, rv, dy = _bn_case(n, c, sp, 1000 * n + c)
    xd, gd, bd, dyd = (v.to(DEV) for v in (x, gamma, beta, dy))
    s = sp[0] * sp[1] * sp[2]
    nbytes = lib.zsv_bn_workspace_bytes(n, c, s)
    ws = ops._workspace(nbytes, DEV)

    def empties():
        return torch.empty_like(xd), torch.empty(c, device=DEV), torch.empty(c, device=DEV)

    # training mode
    y, mean, invstd = ns.bn_train_fwd(xd, gd, bd, torch.zeros(c, device=DEV), torch.ones(c, device=DEV), 0.1, 1e-5, relu)
    got = ns.bn_train_bwd(dyd, xd, y, gd, bd, mean, invstd, relu)
    dx, dgamma, dbeta = empties()
    _lib_call("zsv_bn_bwd", dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), n, c, s, gd.data_ptr(), bd.data_ptr(), mean.data_ptr(),
              invstd.data_ptr(), 1 if relu else 0, dx.data_ptr(), None, dgamma.data_ptr(), dbeta.data_ptr(), ops._ptr(ws), nbytes,
              ops._stream())
    _same(got, (dx, dgamma, dbeta), "bn_train_bwd")
    xr, gr, br = (v.double().requires_grad_() for v in (x, gamma, beta))
    yr = torch.nn.functional.batch_norm(xr, None, None, gr, br, training=True, eps=1e-5)
    mask = (y > 0).cpu().double() if relu else 1.0
    (yr * mask * dy.double()).sum().backward()
    for a, r, what in zip(got, (xr.grad, gr.grad, br.grad), ("dx", "dgamma", "dbeta")):
        close(a, r, rtol=1e-4, what=f"bn_train_bwd {what}")

    # running statistics
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    y = ns.bn_eval_fwd(xd, gd, bd, rmd, rvd, 1e-5, relu)
    got = ns.bn_eval_bwd(dyd, xd, gd, bd, rmd, rvd, 1e-5, relu)
    dx, dgamma, dbeta = empties()
    _lib_call("zsv_bn_bwd_eval", dyd.data_ptr(), xd.data_ptr(), None, n, c, s, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(),
              rvd.data_ptr(), 1e-5, 2 if relu else 0, dx.data_ptr(), None, dgamma.data_ptr(), dbeta.data_ptr(), ops._ptr(ws), nbytes,
              ops._stream())
    _same(got, (dx, dgamma, dbeta), "bn_eval_bwd")
    xr, gr, br = (v.double().requires_grad_() for v in (x, gamma, beta))
    yr = torch.nn.functional.batch_norm(xr, rm.double(), rv.double(), gr, br, training=False, eps=1e-5)
    mask = (y > 0).cpu().double() if relu else 1.0
    (yr * mask * dy.double()).sum().backward()
    for a, r, what in zip(got, (xr.grad, gr.grad, br.grad), ("dx", "dgamma", "dbeta")):
        close(a, r, rtol=1e-4, what=f"bn_eval_bwd {what}")


@pytest.mark.parametrize("rows,fin,fout", [(3, 37, 11), (1, 8192, 64)], ids=["ragged", "one_row"])
def test_linear_and_relu_backward_operators_called_directly(rows, fin, fout):
    from zeroshotvideoclassification_amd import _lib
    ns = torch_ops.load()
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + fin)
    x, w, dy = torch.randn(rows, fin, generator=g), torch.randn(fout, fin, generator=g) / fin ** 0.5, torch.randn(rows, fout, generator=g)
    xd, wd, dyd = (v.to(DEV) for v in (x, w, dy))

    got = ns.linear_dgrad(dyd, wd)
    dx = torch.empty_like(xd)
    nbytes = lib.zsv_linear_dgrad_workspace_bytes(rows, fin, fout)
    ws = ops._workspace(nbytes, DEV)
    _lib_call("zsv_linear_dgrad", dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), rows, fin, fout, ops._ptr(ws), nbytes, ops._stream())
    assert torch.equal(got, dx), "linear_dgrad differs between the two bindings"
    close(got, dy.double() @ w.double(), what="linear_dgrad")

    got = ns.linear_wgrad(xd, dyd)
    dw = torch.empty_like(wd)
    nbytes = lib.zsv_linear_wgrad_workspace_bytes(rows, fin, fout)
    ws = ops._workspace(nbytes, DEV)
    _lib_call("zsv_linear_wgrad", xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), rows, fin, fout, ops._ptr(ws), nbytes, ops._stream())
    assert torch.equal(got, dw), "linear_wgrad differs between the two bindings"
    close(got, dy.double().t() @ x.double(), what="linear_wgrad")

    yd = torch.relu(dyd + 0.25)                                  # a saved ReLU output with exact zeros in it
    got = ns.relu_bwd(xd[:, :fout].contiguous(), yd)
    gd = xd[:, :fout].contiguous()
    dx = torch.empty_like(gd)
    _lib_call("zsv_relu_bwd", gd.data_ptr(), yd.data_ptr(), dx.data_ptr(), gd.numel(), ops._stream())
    assert torch.equal(got, dx), "relu_bwd differs between the two bindings"
    close(got, gd.cpu().double() * (yd.cpu() > 0), what="relu_bwd")


# ---- the differentiable operators: gradient subsets, upstream gradients that are not contiguous, grad modes ---------------------------
def _diff_cases():
    """name -> (call(ns, *tensors), the same in torch fp64, [operands], tolerance of the gradients)."""
    g = torch.Generator().manual_seed(5)
    F = torch.nn.functional
    c = 6
    rm, rv = torch.randn(c, generator=g) * 0.5, torch.rand(c, generator=g) * 2 + 0.5
    bn_x = torch.randn(2, c, 2, 4, 6, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    return {
        "conv3d": (lambda ns, x, w, b: ns.conv3d(x, w, b, [1, 1, 1], [0, 1, 1]),
                   lambda x, w, b: F.conv3d(x, w, b, (1, 1, 1), (0, 1, 1)),
                   [torch.randn(2, 5, 3, 8, 8, generator=g), torch.randn(7, 5, 1, 3, 3, generator=g) / 45 ** 0.5, torch.randn(7, generator=g)],
                   2e-5),
        "batch_norm_relu": (lambda ns, x, ga, be: ns.batch_norm_relu(x, ga, be, torch.zeros(c, device=x.device),
                                                                     torch.ones(c, device=x.device), 0.1, 1e-5, True),
                            lambda x, ga, be: torch.relu(F.batch_norm(x, None, None, ga, be, training=True, eps=1e-5)),
                            [bn_x, gamma, beta], 1e-4),
        "batch_norm_relu_eval": (lambda ns, x, ga, be: ns.batch_norm_relu_eval(x, ga, be, rm.to(x.device), rv.to(x.device), 1e-5, True),
                                 lambda x, ga, be: torch.relu(F.batch_norm(x, rm.double(), rv.double(), ga, be, training=False, eps=1e-5)),
                                 [bn_x, gamma, beta], 1e-4),
        "relu": (lambda ns, x: ns.relu(x), lambda x: torch.relu(x), [torch.randn(3, 5, 8, generator=g)], 2e-5),
        "linear": (lambda ns, x, w, b: ns.linear(x, w, b), lambda x, w, b: F.linear(x, w, b),
                   [torch.randn(3, 37, generator=g), torch.randn(11, 37, generator=g) / 37 ** 0.5, torch.randn(11, generator=g)], 2e-5),
    }


@pytest.mark.parametrize("name", ["conv3d", "linear", "batch_norm_relu"])
def test_each_operand_requiring_a_gradient_alone(name):
    """`needs_input_grad` subsets (batch_norm_relu_eval: tests/test_frozen_bn_gpu.py): with one operand requiring a gradient, that
    gradient has the bits of the all-operands run and the other operands get none."""
    ns = torch_ops.load()
    call, _, operands, _ = _diff_cases()[name]
    full = [v.to(DEV).requires_grad_() for v in operands]
    y = call(ns, *full)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    y.backward(gy)
    for i in range(len(operands)):
        part = [v.to(DEV).requires_grad_(j == i) for j, v in enumerate(operands)]
        yi = call(ns, *part)
        assert torch.equal(yi, y)
        yi.backward(gy)
        for j, (p, f) in enumerate(zip(part, full)):
            if j == i:
                assert torch.equal(p.grad, f.grad), f"{name}: operand {i} alone"
            else:
                assert p.grad is None, f"{name}: operand {j} got a gradient while only operand {i} requires one"


@pytest.mark.parametrize("upstream", ["expanded", "strided"])
@pytest.mark.parametrize("name", ["conv3d", "batch_norm_relu", "batch_norm_relu_eval", "relu", "linear"])
def test_upstream_gradients_that_are_not_contiguous(name, upstream):
    """`y.sum().backward()` hands the operator an expanded (stride-0) gradient, `y[..., ::2].sum().backward()` one built through
    a strided view; the kernels take dense pointers."""
    ns = torch_ops.load()
    call, ref, operands, tol = _diff_cases()[name]

    def reduce(y):
        return y.sum() if upstream == "expanded" else y[..., ::2].sum()
    rs = [v.double().requires_grad_() for v in operands]
    reduce(ref(*rs)).backward()
    ds = [v.to(DEV).requires_grad_() for v in operands]
    reduce(call(ns, *ds)).backward()
    for i, (d, r) in enumerate(zip(ds, rs)):
        close(d.grad, r.grad, rtol=tol, what=f"{name} ({upstream} upstream gradient): operand {i}")


@pytest.mark.parametrize("name", ["batch_norm_relu", "batch_norm_relu_eval", "relu", "linear"])
def test_no_grad_and_inference_mode_match_the_forward_under_autograd(name):
    ns = torch_ops.load()
    call, _, operands, _ = _diff_cases()[name]
    y = call(ns, *[v.to(DEV).requires_grad_() for v in operands])
    assert y.requires_grad
    with torch.no_grad():
        y_ng = call(ns, *[v.to(DEV).requires_grad_() for v in operands])
    plain = [v.to(DEV) for v in operands]
    with torch.inference_mode():
        y_im = call(ns, *plain)
    assert not y_ng.requires_grad and not y_im.requires_grad
    assert torch.equal(y_ng, y.detach()), f"{name} under no_grad"
    assert torch.equal(y_im, y.detach()), f"{name} under inference_mode"


def test_running_statistics_are_updated_exactly_once_in_every_grad_mode():
    ns = torch_ops.load()
    _, _, (x, gamma, beta), _ = _diff_cases()["batch_norm_relu"]
    c = x.shape[1]
    g = torch.Generator().manual_seed(9)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    xs = x.double().transpose(0, 1).reshape(c, -1)
    once = (0.9 * rm0.double() + 0.1 * xs.mean(1), 0.9 * rv0.double() + 0.1 * xs.var(1, unbiased=True))
    twice = 0.9 * once[0] + 0.1 * xs.mean(1)
    seen = []
    for mode in (torch.enable_grad, torch.no_grad, torch.inference_mode):
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        args = [v.to(DEV).requires_grad_(mode is not torch.inference_mode) for v in (x, gamma, beta)]
        with mode():
            ns.batch_norm_relu(*args, rm, rv, 0.1, 1e-5, True)
        close(rm, once[0], what=f"running_mean under {mode.__name__}")
        close(rv, once[1], what=f"running_var under {mode.__name__}")
        assert (rm.double().cpu() - twice).abs().max() > 1e-3                 # (the two are far enough apart to tell)
        seen.append((rm, rv))
    for rm, rv in seen[1:]:
        assert torch.equal(rm, seen[0][0]) and torch.equal(rv, seen[0][1])


# ---- torch.library.opcheck -----------------------------------------------------------------------------------------------------------
def _opcheck_samples(ns):
    """One small valid call per registered operator (a few hundred elements)."""
    g = torch.Generator().manual_seed(21)

    def t(*shape, grad=False):
        return torch.randn(*shape, generator=g).to(DEV).requires_grad_(grad)
    c = 6
    x, w, b = t(2, 4, 2, 5, 5), t(3, 4, 1, 3, 3), t(3)
    dy = t(2, 3, 2, 5, 5)
    s, p = [1, 1, 1], [0, 1, 1]
    bx, gamma, beta = t(2, c, 2, 3, 4), t(c).abs() + 0.5, t(c)
    stats = lambda: (torch.zeros(c, device=DEV), torch.ones(c, device=DEV))
    by, mean, invstd = ns.bn_train_fwd(bx, gamma, beta, *stats(), 0.1, 1e-5, True)
    lx, lw, lb, ldy = t(3, 37), t(11, 37), t(11), t(3, 11)
    plain = {
        "version": (),
        "conv3d_fwd": (x, w, b, s, p, True),
        "conv3d_dgrad": (dy, w, list(x.shape), s, p),
        "conv3d_wgrad": (x, dy, list(w.shape), s, p),
        "bn_train_fwd": (bx, gamma, beta, *stats(), 0.1, 1e-5, True),
        "bn_train_bwd": (t(*bx.shape), bx, by, gamma, beta, mean, invstd, True),
        "bn_eval_fwd": (bx, gamma, beta, *stats(), 1e-5, True),
        "bn_eval_bwd": (t(*bx.shape), bx, gamma, beta, *stats(), 1e-5, True),
        "relu_fwd": (lx,),
        "relu_bwd": (ldy, torch.relu(t(3, 11))),
        "linear_fwd": (lx, lw, lb, True),
        "linear_dgrad": (ldy, lw),
        "linear_wgrad": (lx, ldy),
    }
    diff = {
        "conv3d": (t(2, 4, 2, 5, 5, grad=True), t(3, 4, 1, 3, 3, grad=True), t(3, grad=True), s, p),
        "batch_norm_relu": (t(2, c, 2, 3, 4, grad=True), t(c, grad=True), t(c, grad=True), *stats(), 0.1, 1e-5, True),
        "batch_norm_relu_eval": (t(2, c, 2, 3, 4, grad=True), t(c, grad=True), t(c, grad=True), *stats(), 1e-5, True),
        "relu": (t(3, 37, grad=True),),
        "linear": (t(3, 37, grad=True), t(11, 37, grad=True), t(11, grad=True)),
    }
    return plain, diff


def test_opcheck_schema_and_autograd_registration():
    """`torch.library.opcheck`: every operator writes exactly the operands its schema marks `(a!)` / `(b!)` and aliases nothing
    (test_schema); the five differentiable ones have their autograd kernel where the dispatcher looks for it
    (test_autograd_registration).  No meta kernels exist, so the fake-tensor and AOT checks do not apply."""
    ns = torch_ops.load()
    plain, diff = _opcheck_samples(ns)
    assert sorted(list(plain) + list(diff)) == sorted(torch_ops.OPERATORS)
    for name, args in plain.items():
        assert torch.library.opcheck(getattr(ns, name).default, args, test_utils=("test_schema",)) == {"test_schema": "SUCCESS"}, name
    for name, args in diff.items():
        result = torch.library.opcheck(getattr(ns, name).default, args, test_utils=("test_schema", "test_autograd_registration"))
        assert result == {"test_schema": "SUCCESS", "test_autograd_registration": "SUCCESS"}, name


# ---- writes the version counters and the engine cache must see ------------------------------------------------------------------------
def test_running_statistics_written_by_the_operator_invalidate_the_cached_engine():
    """`bn_train_fwd` writes the running statistics through raw pointers; it moves their `_version` by hand, which is one of the
    things `inference.engine_for` keys a folded engine on."""
    from helpers import make_opt
    from zeroshotvideoclassification_amd import inference, network, synthetic, train
    ns = torch_ops.load()
    model = network.get_network(make_opt("r2plus1d_18"))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=2, bn_jitter=True))
    model.to(DEV).eval()
    clips = synthetic.synthetic_clips(2, 8, 64).to(DEV)
    engine = inference.engine_for(model)
    with torch.no_grad():
        stale = train.embed(engine, clips)
        assert inference.engine_for(model) is engine
        bn = model.model.stem[1]
        versions = bn.running_mean._version, bn.running_var._version
        x = torch.randn(2, bn.num_features, 2, 8, 8, generator=torch.Generator().manual_seed(4)).to(DEV) * 3 + 1
        ns.batch_norm_relu(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, 0.5, bn.eps, True)
        assert bn.running_mean._version > versions[0] and bn.running_var._version > versions[1]
        fresh = inference.engine_for(model)
        assert fresh is not engine, "a stale folded engine was served after the operator moved the running statistics"
        got = train.embed(fresh, clips)
        want = train.embed(inference.engine_for(model, rebuild=True), clips)
    assert torch.equal(got, want)
    assert not torch.equal(got, stale)                           # (the statistics moved far enough to matter)


# ---- two devices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_operators_run_on_their_operands_device_not_the_current_one():
    ns = torch_ops.load()
    other = torch.device("cuda:1")
    cases = _diff_cases()
    for name in ("conv3d", "batch_norm_relu", "linear"):
        call, _, operands, _ = cases[name]
        results = []
        for current in (0, 1):
            args = [v.to(other).requires_grad_() for v in operands]
            with torch.cuda.device(current):
                y = call(ns, *args)
                gy = torch.ones_like(y)
                y.backward(gy)
            assert y.device == other
            results.append([y.detach()] + [a.grad for a in args])
        torch.cuda.synchronize(other)
        for a, b in zip(*results):
            assert torch.equal(a, b), f"{name}: cuda:0 current vs cuda:1 current"
    x, w, b = (v.to(other) for v in cases["conv3d"][2])
    with pytest.raises(RuntimeError, match=r"(?<![a-z_])w is on cuda:0"):
        ns.conv3d_fwd(x, w.to(DEV), None, [1, 1, 1], [0, 1, 1], False)
    with pytest.raises(RuntimeError, match=r"running_var is on cuda:0"):
        bx, gamma, beta = (v.to(other) for v in cases["batch_norm_relu"][2])
        ns.bn_train_fwd(bx, gamma, beta, torch.zeros(6, device=other), torch.ones(6, device=DEV), 0.1, 1e-5, False)
