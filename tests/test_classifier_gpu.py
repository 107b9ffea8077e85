"""Supervised pre-training of the trunk on the device: the zsv_softmax_xent_* kernels against ``F.cross_entropy`` in fp64 on the
CPU (same fp32 logits), the label-rank rule as exact integers, ignored and out-of-range rows, scaling, run-to-run and alignment
bit-equality; then ``network.Classifier`` / ``network.SoftmaxCrossEntropy`` through ``train.train_step`` and
``train.evaluate_classification``.

The bars of the kernel tests are bounds on an fp32 evaluation, not measurements (eps32 = 2^-23):
    per-row loss            |err| <= eps32 * (32 + 4 * max|x|)            over the row
    unscaled gradient row   |err| <= eps32 * (16 + 2 * (max x - min x))   (the conditioning of exp at that logit range)
torch's own fp32 ``cross_entropy`` on the CPU sits at <= 0.25 and <= 0.08 of them on these inputs; the tests print the worst
ratio of every case (DESIGN 3.5l records them)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from guarded import BAND_BYTES, guarded_copy, guarded_like  # noqa: E402
from zeroshotvideoclassification_amd import _lib, amp, network, ops, optim, resnet, synthetic, train  # noqa: E402

DEV = "cuda"
EPS32 = 2.0 ** -23
NEVER = 0x7FFFFFFF
# (N, C, logit scale, label smoothing): one element; less than a wave; exactly one wave and one more; one workgroup pass of
# 256 groups of four and one more (1025), 256 + 1 elements; several passes and a row that is no multiple of four
CASES = [(1, 1, 1, 0.0), (1, 2, 1, 0.0), (3, 5, 1, 0.1), (7, 64, 1, 0.0), (7, 65, 3, 0.1), (5, 257, 30, 0.0), (22, 400, 3, 0.1),
         (9, 700, 3, 0.1), (4, 1025, 100, 0.1), (3, 4100, 10, 0.1)]


def close(a, ref, rtol=2e-5, what=""):
    """The bar tests/test_ops_gpu.py applies to zsv_linear_*."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-30
    err = (a - ref).abs().max().item()
    assert err <= rtol * scale + 1e-12, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


def ulps(a, b):
    """Largest distance in units in the last place between two finite fp32 tensors (+0 and -0 are the same number)."""
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())

    def key(t):                                  # the integer order of the floats
        i = t.view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max().item()) if a.numel() else 0


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def rank_rule(x, labels):
    """rank = #{j: x[j] > x[y] or (x[j] == x[y] and j < y)}, -1 for label -1; from the fp32 logits, on the CPU."""
    out = torch.full((len(labels),), -1, dtype=torch.int64)
    index = torch.arange(x.shape[1])
    for r, y in enumerate(labels.tolist()):
        if y != -1:
            out[r] = int(((x[r] > x[r, y]) | ((x[r] == x[r, y]) & (index < y))).sum())
    return out


@functools.lru_cache(maxsize=None)
def case(n, c, scale, eps):
    """Inputs and the fp64 CPU reference of one case; computed once, shared by the tests, never written."""
    g = torch.Generator().manual_seed(n * 1000 + c)
    x = torch.randn(n, c, generator=g) * scale
    labels = torch.randint(0, c, (n,), generator=g)
    if n > 2:
        labels[1] = -1                                                   # ignored
    if n > 4:
        x[2] = x[2].round()                                              # ties; the label is the LAST of a repeated value
        values, counts = torch.unique(x[2], return_counts=True)
        repeated = values[counts > 1]
        assert len(repeated), "no tie in the rounded row"
        labels[2] = int(torch.nonzero(x[2] == repeated[len(repeated) // 2]).flatten()[-1])
        x[3, 0], x[3, c - 1] = 1e4, -1e4                                 # NaN without the maximum subtracted
        labels[3] = 1 + int(labels[3]) % (c - 2)
    xr = x.double().requires_grad_()
    rows = F.cross_entropy(xr, labels, ignore_index=-1, label_smoothing=eps, reduction="none")
    rows.sum().backward()
    ranks = rank_rule(x, labels)
    valid = labels != -1
    counts = torch.tensor([int(valid.sum()), int((ranks == 0).sum()), int(((ranks >= 0) & (ranks < 5)).sum())])
    loss_bar = EPS32 * (32 + 4 * x.abs().amax(1).double())
    grad_bar = EPS32 * (16 + 2 * (x.amax(1) - x.amin(1)).double())
    return dict(x=x, labels=labels, row_loss=rows.detach(), grad=xr.grad, ranks=ranks, counts=counts, loss_bar=loss_bar,
                grad_bar=grad_bar)


def c_abi_forward(x, labels, eps, ignore_index=-1, want_grad=True):
    """zsv_softmax_xent_fwd + _reduce (sum) on device tensors -> row_loss, row_rank, dlogits, loss, counts."""
    n, c = x.shape
    row_loss = torch.full((n,), float("nan"), device=DEV)
    row_rank = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    dlogits = torch.full((n, c), float("nan"), device=DEV) if want_grad else None
    loss = torch.full((), float("nan"), device=DEV)
    counts = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    stream = ops._stream()
    _lib.check(lib.zsv_softmax_xent_fwd(x.data_ptr(), labels.data_ptr(), n, c, eps, ignore_index, row_loss.data_ptr(),
                                        row_rank.data_ptr(), ops._ptr(dlogits), stream), "zsv_softmax_xent_fwd")
    _lib.check(lib.zsv_softmax_xent_reduce(row_loss.data_ptr(), row_rank.data_ptr(), n, 0, loss.data_ptr(), counts.data_ptr(), stream),
               "zsv_softmax_xent_reduce")
    return row_loss, row_rank, dlogits, loss, counts


@pytest.mark.parametrize("n, c, scale, eps", CASES)
def test_rows_against_fp64_cross_entropy(n, c, scale, eps):
    ref = case(n, c, scale, eps)
    x, labels = ref["x"].to(DEV), ref["labels"].to(DEV)
    row_loss, row_rank, dlogits, loss, counts = c_abi_forward(x, labels, eps)
    torch.cuda.synchronize()
    loss_err = (row_loss.cpu().double() - ref["row_loss"]).abs()
    grad_err = (dlogits.cpu().double() - ref["grad"]).abs().amax(1)
    loss_ratio, grad_ratio = float((loss_err / ref["loss_bar"]).max()), float((grad_err / ref["grad_bar"]).max())
    print(f"\nsoftmax_xent (N={n}, C={c}, scale={scale}, eps={eps}): worst |err| / bar: loss {loss_ratio:.3f}, gradient {grad_ratio:.3f}")
    assert bool(torch.isfinite(row_loss).all()) and bool(torch.isfinite(dlogits).all())
    assert loss_ratio <= 1.0 and grad_ratio <= 1.0
    # exact: the rank rule, the counts, the ignored rows
    assert torch.equal(row_rank.cpu().long(), ref["ranks"])
    assert torch.equal(counts.cpu().long(), ref["counts"])
    ignored = (ref["labels"] == -1).to(DEV)
    assert bool((row_loss[ignored] == 0).all()) and bool((row_rank[ignored] == -1).all()) and bool((dlogits[ignored] == 0).all())
    # the summed loss: the valid rows' bars add up
    total_bar = float(ref["loss_bar"][ref["labels"] != -1].sum()) + EPS32 * abs(float(ref["row_loss"].sum()))
    assert abs(float(loss.cpu().double()) - float(ref["row_loss"].sum())) <= total_bar
    # two runs: the same bits; and without a gradient buffer the same loss and ranks
    again = c_abi_forward(x, labels, eps)
    assert all(same_bits(a, b) for a, b in zip(again, (row_loss, row_rank, dlogits, loss, counts)))
    bare = c_abi_forward(x, labels, eps, want_grad=False)
    assert same_bits(bare[0], row_loss) and same_bits(bare[1], row_rank) and same_bits(bare[3], loss)


def test_untied_rows_agree_with_topk():
    """On rows without a tie at the label the rank rule is torch.topk's membership (checked here on the CPU reference itself)."""
    ref = case(22, 400, 3, 0.1)
    top5 = ref["x"].topk(5, dim=1).indices
    for r, y in enumerate(ref["labels"].tolist()):
        if y != -1 and int((ref["x"][r] == ref["x"][r, y]).sum()) == 1:
            assert (y in top5[r].tolist()) == (int(ref["ranks"][r]) < 5) and (top5[r, 0] == y) == (int(ref["ranks"][r]) == 0)


def test_hits_are_counted():
    """Random labels hardly ever hit: here row r is labelled with its (r mod 7)-th largest logit, so its rank is r mod 7."""
    x = torch.randn(14, 65, generator=torch.Generator().manual_seed(7))
    labels = torch.stack([x[r].argsort(descending=True)[r % 7] for r in range(14)])
    assert rank_rule(x, labels).tolist() == [r % 7 for r in range(14)]
    criterion = network.SoftmaxCrossEntropy()
    criterion(x.to(DEV), labels.to(DEV))
    assert criterion.counts.tolist() == [14, 2, 10]
    top1, top5 = train.classification_accuracy(criterion.counts)
    assert top1.is_cuda and top1.item() == pytest.approx(100 * 2 / 14) and top5.item() == pytest.approx(100 * 10 / 14)
    # with fewer than five classes every scored row is a top-5 hit
    _, counts = ops.softmax_cross_entropy(x[:, :3].contiguous().to(DEV), torch.tensor([0, 1, 2, -1] * 3 + [0, 1], device=DEV))
    assert counts.tolist()[0] == 11 and counts.tolist()[2] == 11


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_every_row_ignored_is_zero_not_nan(reduction):
    x = torch.randn(6, 65, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_()
    labels = torch.full((6,), -1, dtype=torch.int64, device=DEV)
    loss, counts = ops.softmax_cross_entropy(x, labels, label_smoothing=0.1, reduction=reduction)
    loss.backward()
    assert loss.item() == 0.0 and counts.tolist() == [0, 0, 0]
    assert bool((x.grad == 0).all())


@pytest.mark.parametrize("band", BAND_BYTES)
def test_out_of_range_labels_poison_their_own_row_only(band):
    """Label C and label -7 (ignore_index is -1): those rows are NaN, count as valid, never hit; the others keep their bits; the
    bands around the logits and around every output are untouched, and poisoned bands around the logits change nothing."""
    ref = case(7, 65, 3, 0.1)
    n, c = ref["x"].shape
    good = c_abi_forward(ref["x"].to(DEV), ref["labels"].to(DEV), 0.1)
    labels = ref["labels"].clone()
    labels[0], labels[4] = c, -7
    bad_rows = torch.tensor([0, 4])
    logits = guarded_copy(ref["x"], DEV, guard_byte=band, shift=4)
    label_buf = guarded_copy(labels, DEV, guard_byte=band)
    outs = {"row_loss": guarded_like(torch.float32, (n,), DEV, 0xFF, shift=8), "row_rank": guarded_like(torch.int32, (n,), DEV, 0xFF),
            "dlogits": guarded_like(torch.float32, (n, c), DEV, 0xFF, shift=12), "loss": guarded_like(torch.float32, (1,), DEV, 0xFF),
            "counts": guarded_like(torch.int32, (3,), DEV, 0xFF)}
    lib = _lib.load()
    _lib.check(lib.zsv_softmax_xent_fwd(logits.ptr, label_buf.ptr, n, c, 0.1, -1, outs["row_loss"].ptr, outs["row_rank"].ptr,
                                        outs["dlogits"].ptr, ops._stream()), "zsv_softmax_xent_fwd")
    _lib.check(lib.zsv_softmax_xent_reduce(outs["row_loss"].ptr, outs["row_rank"].ptr, n, 1, outs["loss"].ptr, outs["counts"].ptr,
                                           ops._stream()), "zsv_softmax_xent_reduce")
    torch.cuda.synchronize()
    for name, b in list(outs.items()) + [("logits", logits), ("labels", label_buf)]:
        b.check(name)
    row_loss, row_rank = outs["row_loss"].view(torch.float32, (n,)), outs["row_rank"].view(torch.int32, (n,))
    dlogits = outs["dlogits"].view(torch.float32, (n, c))
    assert bool(torch.isnan(row_loss[bad_rows]).all()) and bool(torch.isnan(dlogits[bad_rows]).all())
    assert row_rank[bad_rows].tolist() == [NEVER, NEVER]
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad_rows] = False
    assert same_bits(row_loss[keep], good[0][keep]) and same_bits(row_rank[keep], good[1][keep])
    assert same_bits(dlogits[keep], good[2][keep])
    want = ref["counts"].clone()                   # rows 0 and 4 were valid rows and stay valid; whatever they hit is gone
    hits = ref["ranks"][bad_rows]
    assert want[0] == int((labels != -1).sum()) and bool((hits >= 0).all())
    want[1] -= int((hits == 0).sum())
    want[2] -= int(((hits >= 0) & (hits < 5)).sum())
    assert outs["counts"].view(torch.int32, (3,)).tolist() == want.tolist()
    assert bool(torch.isnan(outs["loss"].view(torch.float32, (1,))).all())


def test_scaling_mean_sum_and_the_incoming_gradient():
    ref = case(22, 400, 3, 0.1)
    labels = ref["labels"].to(DEV)
    valid = int(ref["counts"][0])

    def run(reduction, factor=None, scaler=None):
        x = ref["x"].to(DEV).requires_grad_()
        loss, counts = ops.softmax_cross_entropy(x, labels, label_smoothing=0.1, reduction=reduction)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and counts.dtype == torch.int32 and not counts.requires_grad
        out = loss if factor is None else loss * factor
        (scaler.scale(out) if scaler is not None else out).backward()
        return loss.detach(), x.grad, counts
    loss_sum, grad_sum, counts = run("sum")
    loss_mean, grad_mean, _ = run("mean")
    assert counts.tolist() == ref["counts"].tolist()
    assert ulps(loss_mean, loss_sum.cpu() / valid) <= 2
    # the gradient of the sum is the kernel's unscaled gradient; the mean's is that over `valid`
    assert float(((grad_sum.cpu().double() - ref["grad"]).abs().amax(1) / ref["grad_bar"]).max()) <= 1.0
    assert ulps(grad_mean, grad_sum.cpu() / valid) <= 1
    _, grad_4, _ = run("mean", factor=4.0)
    assert same_bits(grad_4, grad_mean * 4.0)
    scaler = optim.LossScaler()
    scale = scaler.get_scale()
    assert scale == 2.0 ** 16
    _, grad_scaled, _ = run("mean", scaler=scaler)
    assert ulps(grad_scaled / scale, grad_mean) <= 1
    # a graph is walked once: the backward scales the saved gradient in place
    x = ref["x"].to(DEV).requires_grad_()
    loss, _ = ops.softmax_cross_entropy(x, labels)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second"):
        loss.backward()


@pytest.mark.parametrize("n, c, scale, eps", [(7, 65, 3, 0.1), (22, 400, 3, 0.1)])
def test_a_view_four_bytes_past_a_boundary_gives_the_same_bits(n, c, scale, eps):
    ref = case(n, c, scale, eps)
    labels = ref["labels"].to(DEV)
    aligned = ref["x"].to(DEV)
    assert aligned.data_ptr() % 256 == 0
    big = torch.zeros(n * c + 128, device=DEV)
    assert big.data_ptr() % 256 == 0
    view = big[1:1 + n * c].view(n, c)
    view.copy_(aligned)
    assert view.data_ptr() % 256 == 4 and view.is_contiguous()
    # the C ABI with every fp32 operand off its boundary, each by another amount
    base = c_abi_forward(aligned, labels, eps)
    outs = {"row_loss": guarded_like(torch.float32, (n,), DEV, 0xFF, shift=8), "dlogits": guarded_like(torch.float32, (n, c), DEV, 0xFF, shift=12),
            "dx": guarded_like(torch.float32, (n, c), DEV, 0xFF, shift=4)}
    row_rank = torch.empty(n, dtype=torch.int32, device=DEV)
    grad_loss = torch.tensor(3.0, device=DEV)
    counts = base[4]
    lib = _lib.load()
    _lib.check(lib.zsv_softmax_xent_fwd(view.data_ptr(), labels.data_ptr(), n, c, eps, -1, outs["row_loss"].ptr, row_rank.data_ptr(),
                                        outs["dlogits"].ptr, ops._stream()), "zsv_softmax_xent_fwd")
    _lib.check(lib.zsv_softmax_xent_bwd(outs["dlogits"].ptr, grad_loss.data_ptr(), counts.data_ptr(), 1, n, c, outs["dx"].ptr,
                                        ops._stream()), "zsv_softmax_xent_bwd")
    dx = torch.empty_like(aligned)
    _lib.check(lib.zsv_softmax_xent_bwd(base[2].data_ptr(), grad_loss.data_ptr(), counts.data_ptr(), 1, n, c, dx.data_ptr(),
                                        ops._stream()), "zsv_softmax_xent_bwd")
    torch.cuda.synchronize()
    for name, b in outs.items():
        b.check(name)
    assert same_bits(outs["row_loss"].view(torch.float32, (n,)), base[0]) and same_bits(row_rank, base[1])
    assert same_bits(outs["dlogits"].view(torch.float32, (n, c)), base[2])
    assert same_bits(outs["dx"].view(torch.float32, (n, c)), dx)
    # and through the op
    results = []
    for logits in (aligned, view):
        leaf = logits.detach().requires_grad_()
        loss, got = ops.softmax_cross_entropy(leaf, labels, label_smoothing=eps)
        loss.backward()
        results.append((loss.detach(), got, leaf.grad))
    assert all(same_bits(a, b) for a, b in zip(*results))


def test_op_refusals_and_the_empty_batch():
    x = torch.randn(4, 7, device=DEV)
    labels = torch.tensor([0, 1, 2, 3], device=DEV)
    for bad_x, bad_l, kw in ((x.double(), labels, {}), (x, labels.int(), {}), (x, labels[:3], {}), (x.reshape(2, 2, 7), labels, {}),
                             (x, labels, {"reduction": "none"}), (x, labels, {"label_smoothing": 1.0}), (x, labels.cpu(), {})):
        with pytest.raises(RuntimeError):
            ops.softmax_cross_entropy(bad_x, bad_l, **kw)
    empty = torch.zeros(0, 7, device=DEV, requires_grad=True)
    loss, counts = ops.softmax_cross_entropy(empty, labels[:0])
    loss.backward()
    assert loss.item() == 0.0 and counts.tolist() == [0, 0, 0] and tuple(empty.grad.shape) == (0, 7)
    with torch.no_grad():
        loss, counts = ops.softmax_cross_entropy(x, labels, reduction="sum")
    assert not loss.requires_grad and counts[0].item() == 4


# ---- module level: r2plus1d_18, 2 clips of 3 x 8 x 56 x 56 ------------------------------------------------------------------
CLASSES = 7


def classifier(seed=0):
    clf = network.Classifier(resnet.r2plus1d_18, CLASSES)
    clf.load_state_dict(synthetic.keyed_state_dict(clf.state_dict(), seed=seed, bn_jitter=True))
    with torch.no_grad():
        clf.model.fc.weight.mul_(20.0)                                   # (0.01-sigma weights give seven nearly equal logits)
    return clf.to(DEV)


def clips(n=2, seed=0):
    return synthetic.synthetic_clips(n, 8, 56, seed=seed).to(DEV)


@pytest.mark.parametrize("training", [True, False])
def test_fp32_logits_are_the_trunk_feature_through_fc(training):
    clf = classifier().train(training)
    x = clips()
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    with torch.no_grad():
        logits = clf(x)
        clf.load_state_dict(before)                                      # (the running statistics moved in train mode)
        pooled = clf.model(x.reshape(2, 3, 8, 56, 56))[0]
        want = ops.linear(pooled, clf.model.fc.weight, clf.model.fc.bias)
    assert isinstance(logits, torch.Tensor) and tuple(logits.shape) == (2, CLASSES)
    assert same_bits(logits, want)


def test_autocast_logits_are_the_bf16_trunk_feature_through_fc():
    clf = classifier().train()
    x = clips()
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    with torch.no_grad():
        with amp.autocast():
            logits = clf(x)
        clf.load_state_dict(before)
        pooled = amp.trunk_features(clf.model, x.reshape(2, 3, 8, 56, 56))
        want = ops.linear(pooled, clf.model.fc.weight, clf.model.fc.bias)
        clf.load_state_dict(before)
        fp32 = clf(x)
    assert same_bits(logits, want)
    assert not same_bits(logits, fp32)                                   # it really took the other trunk
    # eval mode under autocast: the fp32 modules (there is no reduced-precision classifier engine)
    clf.load_state_dict(before)
    clf.eval()
    with torch.no_grad():
        plain = clf(x)
        with amp.autocast():
            inside = clf(x)
    assert same_bits(plain, inside)


def test_head_gradients_against_fp64():
    clf = classifier().train()
    x = clips()
    labels = torch.tensor([3, 5], device=DEV)
    seen = {}

    def watch(module, inputs):
        seen["pooled"] = inputs[0].detach().clone()
        inputs[0].register_hook(lambda g: seen.__setitem__("dpooled", g.detach().clone()))
    handle = clf.model.fc.register_forward_pre_hook(watch)
    criterion = network.SoftmaxCrossEntropy(0.1)
    loss = criterion(clf(x), labels)
    loss.backward()
    ops.join_wgrad_streams()
    torch.cuda.synchronize()
    handle.remove()
    pooled = seen["pooled"].cpu().double().requires_grad_()
    w, b = clf.model.fc.weight.detach().cpu().double().requires_grad_(), clf.model.fc.bias.detach().cpu().double().requires_grad_()
    want = F.cross_entropy(F.linear(pooled, w, b), labels.cpu(), label_smoothing=0.1)
    want.backward()
    close(loss, want, what="loss")
    close(clf.model.fc.weight.grad, w.grad, what="fc.weight.grad")
    close(clf.model.fc.bias.grad, b.grad, what="fc.bias.grad")
    close(seen["dpooled"], pooled.grad, what="the gradient arriving at the pooled feature")
    assert criterion.counts.tolist()[0] == 2
    assert clf.model.stem[0].weight.grad is not None and bool(torch.isfinite(clf.model.stem[0].weight.grad).all())


@pytest.mark.parametrize("mode", ["fp32", "autocast + LossScaler", "micro_batches=2"])
def test_train_step_trains_every_parameter(mode):
    clf = classifier().train()
    parts = 2 if mode == "micro_batches=2" else 1                        # every forward sees 2 clips: the criterion keeps its LAST call's counts
    x = clips(2 * parts)
    labels = torch.tensor([3, 5, 0, 6][:2 * parts], device=DEV)
    criterion = network.SoftmaxCrossEntropy(0.1)
    opt = optim.FusedSGD(clf.parameters(), lr=0.05, momentum=0.9)
    before = {k: p.detach().clone() for k, p in clf.named_parameters()}
    kwargs = {"fp32": {}, "autocast + LossScaler": {"autocast": True, "scaler": optim.LossScaler()},
              "micro_batches=2": {"micro_batches": 2}}[mode]
    logits, loss = train.train_step(clf, opt, criterion, x, labels, **kwargs)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (2 * parts, CLASSES) and loss.dim() == 0 and bool(torch.isfinite(loss))
    assert criterion.counts[0].item() == 2
    assert "model.fc.weight" in before and "model.fc.bias" in before
    for k, p in clf.named_parameters():
        assert p.grad is not None, k
        assert bool(torch.isfinite(p.grad).all()), k
        assert bool((p.grad != 0).any()), k
        assert not torch.equal(p.detach(), before[k]), k
    top1, top5 = train.classification_accuracy(criterion.counts)
    assert top1.is_cuda and 0.0 <= top1.item() <= top5.item() <= 100.0


def test_evaluate_classification_drops_label_minus_one_on_the_device():
    clf = classifier().train()
    batches = [(clips(2, seed=1).cpu(), torch.tensor([3, -1])), (clips(2, seed=2).cpu(), torch.tensor([-1, -1])),
               (clips(2, seed=3).cpu(), torch.tensor([5, 0]))]
    got = train.evaluate_classification(clf, batches, label_smoothing=0.1)
    assert clf.training and all(m.training for m in clf.modules())       # the modes come back
    clf.eval()
    with torch.no_grad():
        logits = torch.cat([clf(x.to(DEV)) for x, _ in batches]).cpu()
    labels = torch.cat([l for _, l in batches])
    keep = labels != -1
    kept, kept_labels = logits[keep], labels[keep]
    ranks = rank_rule(kept, kept_labels)
    want_loss = F.cross_entropy(kept.double(), kept_labels, label_smoothing=0.1, reduction="sum")
    assert got["samples"] == 3 and set(got) == {"loss", "top1", "top5", "samples"}
    assert got["top1"] == int((ranks == 0).sum()) / 3 * 100 and got["top5"] == int((ranks < 5).sum()) / 3 * 100
    bar = float((EPS32 * (32 + 4 * kept.abs().amax(1).double())).sum()) + EPS32 * abs(float(want_loss))
    assert abs(got["loss"] * 3 - float(want_loss)) <= bar
    # nothing scored: zeros, not NaN
    nothing = train.evaluate_classification(clf, batches[1:2])
    assert nothing == {"loss": 0.0, "top1": 0.0, "top5": 0.0, "samples": 0}
