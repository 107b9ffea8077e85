"""Gradient accumulation over micro-batches on the device: the zsv_grad_accum_multi kernel bit for bit against torch on the
CPU, train_step(micro_batches=k) through GradientSync's buckets against autograd's own accumulation (parent-commit code) and
against the CPU oracle, under autocast, under FusedAdam + LossScaler, and with two ranks on one device over gloo."""
import os
import socket
import struct
import sys
from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
CHUNK = 4096


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


# ---- 1. the kernel through the raw C ABI ---------------------------------------------------------------------------------
def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality, a NaN matching any NaN (IEEE leaves the payload open)."""
    nan = torch.isnan(b)
    if not torch.equal(torch.isnan(a), nan):
        return False
    return torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])


def test_accumulate_kernel_is_bit_exact_on_unaligned_slices():
    from zeroshotvideoclassification_amd import _lib
    lib = _lib.load()
    sizes = [1, 3, 4095, 4096, 4097, 6615]
    sentinel = 12345.0
    offs, off = [], 1                                       # sentinel | e0 | sentinel | e1 | ... | sentinel
    for n in sizes:
        offs.append(off)
        off += n + 1
    total = off
    assert sum((4 * o) % 16 != 0 for o in offs) >= 4 and any((4 * o) % 16 == 0 for o in offs)
    ref = torch.full((total,), sentinel)
    acc = ref.to(DEV)
    firsts, first = [], 0
    for n in sizes:
        firsts.append(first)
        first += (n + CHUNK - 1) // CHUNK
    gen = torch.Generator().manual_seed(5)
    inf, nan = float("inf"), float("nan")
    # launch -> {position in the 6615 entry: value}: inf and NaN arrive, stay, and +inf meets -inf
    special = [{0: inf, 5: -inf, 4096: nan, 6614: inf}, {5: 1.0, 6614: -inf, 4100: -inf}, {7: nan}]
    scales = [(1.0, 1), (0.5, 0), (float(torch.tensor(1.0 / 3.0, dtype=torch.float32)), 0)]
    for (scale, assign), marks in zip(scales, special):
        host = [torch.randn(n, generator=gen) for n in sizes]
        for pos, val in marks.items():
            host[-1][pos] = val
        dev = [h.to(DEV) for h in host[:-1]]
        padded = torch.zeros(sizes[-1] + 9, device=DEV)     # the last source: a view starting at element 1
        padded[1:1 + sizes[-1]] = host[-1].to(DEV)
        dev.append(padded[1:1 + sizes[-1]])
        assert dev[-1].data_ptr() % 16 == 4 and dev[0].data_ptr() % 16 == 0
        raw = b"".join(struct.pack("<QQqq", acc.data_ptr() + 4 * o, g.data_ptr(), n, f)
                       for o, g, n, f in zip(offs, dev, sizes, firsts))
        table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
        _lib.check(lib.zsv_grad_accum_multi(table.data_ptr(), len(sizes), first, scale, assign,
                                            c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_grad_accum_multi")
        torch.cuda.synchronize()
        s = torch.tensor(scale, dtype=torch.float32)
        for o, h, n in zip(offs, host, sizes):
            sg = h * s                                      # two correctly rounded fp32 operations, no fma
            ref[o:o + n] = sg if assign else ref[o:o + n] + sg
        got = acc.cpu()
        for o, n in zip(offs, sizes):
            assert got[o - 1].item() == sentinel and got[o + n].item() == sentinel, (scale, n)
            assert _same_bits(got[o:o + n], ref[o:o + n]), (scale, n)
        assert _same_bits(got, ref)
        assert padded[0].item() == 0.0 and float(padded[1 + sizes[-1]:].abs().max()) == 0.0
    last = ref[offs[-1]:offs[-1] + sizes[-1]]
    assert last[0] == inf and last[5] == -inf and torch.isnan(last[4096]) and torch.isnan(last[6614]) and last[4100] == -inf
    assert torch.isnan(last[7]) and int(torch.isfinite(last).logical_not().sum()) == 6


def test_accumulate_entry_point_rejects_bad_arguments():
    from zeroshotvideoclassification_amd import _lib
    lib = _lib.load()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.zsv_grad_accum_multi(None, 1, 1, 1.0, 1, stream) != 0
    table = torch.zeros(32, dtype=torch.uint8, device=DEV)
    assert lib.zsv_grad_accum_multi(table.data_ptr(), 1, 0, 1.0, 1, stream) != 0
    assert lib.zsv_grad_accum_multi(table.data_ptr(), 0, 0, 1.0, 1, stream) == 0


# ---- the model --------------------------------------------------------------------------------------------------------------
def _build_model():
    from zeroshotvideoclassification_amd import network, synthetic
    model = network.get_network(SimpleNamespace(network="r2plus1d_18", fixconvs=False, nopretrained=False))
    weights = synthetic.keyed_state_dict(model.state_dict(), seed=0)
    model.load_state_dict(weights)
    return model, weights


def _autograd_accumulated(model, state0, x, z, k, autocast=False, graph=None):
    """Yardstick A: k backward passes of (n_j / N) * loss_j summed by autograd into ``.grad``; no GradientSync anywhere."""
    from zeroshotvideoclassification_amd import amp, ops, train
    crit = torch.nn.MSELoss()
    sizes = train.micro_batch_sizes(int(x.shape[0]), k)
    model.load_state_dict(state0)
    model.zero_grad(set_to_none=True)
    for n, xj, zj in zip(sizes, torch.split(x, sizes), torch.split(z, sizes)):
        if autocast:
            with amp.autocast(graph=graph):
                loss = crit(train.embed(model, xj), zj)
        else:
            loss = crit(train.embed(model, xj), zj)
        (loss * (n / int(x.shape[0]))).backward()
        ops.join_wgrad_streams()
    torch.cuda.synchronize()
    grads = {name: p.grad.detach().clone() for name, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return grads


def _assert_grads_match(model, ref, tag):
    got = {name: p.grad for name, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(ref), (tag, set(got) ^ set(ref))
    for name, g in got.items():
        err = (g - ref[name]).abs().max().item()
        assert err <= 1e-6 * (ref[name].abs().max().item() + 1e-12), (tag, name, err)


@pytest.fixture(scope="module")
def case():
    from zeroshotvideoclassification_amd import synthetic
    model, weights = _build_model()
    model.to(DEV).train()
    x = synthetic.synthetic_clips(6, 8, 32).to(DEV)
    _, z = synthetic.synthetic_targets(6)
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return SimpleNamespace(model=model, weights=weights, x=x, z=z.to(DEV), state0=state0)


def test_accumulated_step_fp32_against_autograd_and_the_oracle(case):
    from helpers import rel_err
    from oracle import restatement as R
    from zeroshotvideoclassification_amd import ddp, train
    model, x, z = case.model, case.x, case.z
    ref = _autograd_accumulated(model, case.state0, x, z, 3)
    sync = ddp.GradientSync(model, local=True, bucket_bytes=8 << 20)
    try:
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        crit = torch.nn.MSELoss()
        for step in range(2):                               # discovery (at the end of the first pass), then the overlapped path
            model.load_state_dict(case.state0)
            y, loss = train.train_step(model, opt, crit, x, z, sync, micro_batches=3)
            torch.cuda.synchronize()
            _assert_grads_match(model, ref, step)
            for flat, rows in sync.bucket_layout():
                for p, off in rows:
                    assert p.grad.data_ptr() == flat.data_ptr() + 4 * off
        assert len(sync.bucket_sizes) >= 2 and sync.bytes_reduced_last_step == 4 * sum(sync.bucket_sizes)
    finally:
        sync.remove()

    # yardstick B: the CPU oracle over the same three micro-batches
    oracle = R.oracle_network(R.make_opt("r2plus1d_18"))
    oracle.load_state_dict(case.weights)
    oracle.train()
    xc, zc = x.cpu(), z.cpu()
    ys, loss_ref = [], 0.0
    with torch.no_grad():
        for xj, zj in zip(torch.split(xc, 2), torch.split(zc, 2)):
            yj = R.embed(oracle, xj)
            ys.append(yj)
            loss_ref = loss_ref + torch.nn.functional.mse_loss(yj, zj) * (2 / 6)
    y_ref = torch.cat(ys)
    assert rel_err(y.cpu().numpy(), y_ref.numpy()) < 1e-4
    assert abs(loss.item() / loss_ref.item() - 1) < 1e-4
    sd, osd = model.state_dict(), oracle.state_dict()
    rm = torch.cat([sd[k].flatten() for k in sd if k.endswith("running_mean")]).cpu().numpy()
    rv = torch.cat([sd[k].flatten() for k in sd if k.endswith("running_var")]).cpu().numpy()
    rm_ref = torch.cat([osd[k].flatten() for k in sd if k.endswith("running_mean")]).numpy()
    rv_ref = torch.cat([osd[k].flatten() for k in sd if k.endswith("running_var")]).numpy()
    assert np.abs(rm - rm_ref).max() < 1e-4 * (np.abs(rm_ref).max() + 1)
    assert rel_err(rv, rv_ref) < 1e-4
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert tracked and all(int(sd[k]) - int(case.state0[k]) == 3 for k in tracked)
    assert all(int(sd[k]) == int(osd[k]) for k in tracked)


@pytest.mark.parametrize("graph", [False, True])
def test_accumulated_step_under_autocast(case, graph):
    from zeroshotvideoclassification_amd import amp, ddp, train
    model, x, z = case.model, case.x, case.z
    ref = _autograd_accumulated(model, case.state0, x, z, 3, autocast=True, graph=graph)
    sync = ddp.GradientSync(model, local=True, bucket_bytes=8 << 20)
    try:
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        for step in range(2):
            model.load_state_dict(case.state0)
            y, loss = train.train_step(model, opt, torch.nn.MSELoss(), x, z, sync, autocast=True, graph=graph, micro_batches=3)
            torch.cuda.synchronize()
            assert y.shape[0] == 6 and torch.isfinite(loss).item() and not amp.is_autocast_enabled()
            _assert_grads_match(model, ref, (graph, step))
    finally:
        sync.remove()


def test_fused_adam_and_loss_scaler_over_accumulated_buckets(case):
    from zeroshotvideoclassification_amd import ddp, optim, train
    model, x, z = case.model, case.x[:4], case.z[:4]
    model.load_state_dict(case.state0)
    sync = ddp.GradientSync(model, local=True, bucket_bytes=8 << 20)
    try:
        fused = optim.FusedAdam(model.parameters(), lr=1e-3, grad_buckets=sync)
        scaler = optim.LossScaler(init_scale=128.0)
        crit = torch.nn.MSELoss()
        for step in range(2):
            train.train_step(model, fused, crit, x, z, sync, scaler, micro_batches=2)
        torch.cuda.synchronize()
        assert fused._static is not None
        for flat, rows in sync.bucket_layout():
            for p, off in rows:
                assert p.grad.data_ptr() == flat.data_ptr() + 4 * off
        assert scaler.state()["steps_done"] == 2 and scaler.state()["scale"] == 128.0
        moved = (model.output2emb_proj.layers[1].weight.detach() - case.state0["output2emb_proj.layers.1.weight"]).abs().max().item()
        assert 1e-4 < moved < 1e-2

        # a non-finite loss in the SECOND micro-batch only: the whole step is skipped
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        z_bad = z.clone()
        z_bad[2:, 0] = float("inf")
        train.train_step(model, fused, crit, x, z_bad, sync, scaler, micro_batches=2)
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            assert torch.equal(p.detach(), before[k]), k
        st = scaler.state()
        assert st["steps_done"] == 2 and st["scale"] == 64.0
    finally:
        sync.remove()


# ---- 5. two ranks on one device over gloo -----------------------------------------------------------------------------------
def _worker(rank, world, port):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from zeroshotvideoclassification_amd import ddp, synthetic, train
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        model, _ = _build_model()
        model.to(dev).train()
        x = synthetic.synthetic_clips(4, 8, 32, rank=rank).to(dev)         # 2 micro-batches of 2 clips, a shard per rank
        _, z = synthetic.synthetic_targets(4, rank=rank)
        z = z.to(dev)
        state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        ref = {}
        for k, g in _autograd_accumulated(model, state0, x, z, 2).items():  # plain collectives on yardstick A's result
            dist.all_reduce(g, op=dist.ReduceOp.SUM)
            ref[k] = g * (1.0 / world)
        sync = ddp.GradientSync(model, bucket_bytes=8 << 20, broadcast_initial_state=False)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        for step in range(2):
            model.load_state_dict(state0)
            train.train_step(model, opt, torch.nn.MSELoss(), x, z, sync, micro_batches=2)
            torch.cuda.synchronize()
            _assert_grads_match(model, ref, (rank, step))
            assert len(sync.bucket_sizes) >= 2 and sync.bytes_reduced_last_step == 4 * sum(sync.bucket_sizes)   # one exchange
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_accumulated_gradient_sync_two_ranks_on_hip_tensors():
    world = 2
    mp.spawn(_worker, args=(world, _free_port()), nprocs=world, join=True)
