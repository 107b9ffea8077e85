"""Gradient accumulation over micro-batches on CPU tensors: world-2 gloo exchange, the local bucket path, the errors."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class _Net(torch.nn.Module):
    """The stand-in of test_ddp_gloo.py: several parameter tensors of different sizes, a frozen one, and one that never
    receives a gradient.  No BatchNorm: micro-batching does not change what it computes."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(16, 32)
        self.b = torch.nn.Linear(32, 32)
        self.c = torch.nn.Linear(32, 8)
        self.dead = torch.nn.Linear(4, 4)          # never used in forward
        self.frozen = torch.nn.Linear(8, 8)
        for p in self.frozen.parameters():
            p.requires_grad = False
        self.register_buffer("running", torch.zeros(3))

    def forward(self, x):
        return self.frozen(self.c(torch.relu(self.b(torch.relu(self.a(x))))))


def _worker(rank, world, port, bucket_bytes, result_dir):
    sys.path.insert(0, ROOT)
    from zeroshotvideoclassification_amd import ddp, train
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)                      # replicas start DIFFERENT on purpose
        model = _Net()
        sync = ddp.GradientSync(model, bucket_bytes=bucket_bytes)

        g = torch.Generator().manual_seed(7)
        full_x = torch.randn(world * 6, 16, generator=g)
        full_z = torch.randn(world * 6, 8, generator=g)
        x, z = full_x[rank * 6:(rank + 1) * 6], full_z[rank * 6:(rank + 1) * 6]

        # single-process full batch of 12 (what DataParallel computes)
        torch.manual_seed(100)
        ref = _Net()
        ref_opt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad], lr=1e-2)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
        crit = torch.nn.MSELoss()
        for step in range(3):                              # step 0: discovery at the end of its first pass
            y, loss = train.train_step(model, opt, crit, x, z, sync, micro_batches=3)
            assert y.shape == (6, 8) and loss.dim() == 0
            assert sync.bytes_reduced_last_step == 4 * sum(sync.bucket_sizes), step      # one exchange, not three
            ref_opt.zero_grad()
            crit(ref(full_x), full_z).backward()
            if step == 0:
                for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
                    if q.grad is None:
                        assert p.grad is None, k
                    else:
                        assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-7), k
            ref_opt.step()
            for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
                assert torch.allclose(p, q, rtol=1e-4, atol=1e-6), (step, k)
        assert sync.live_parameter_count == 6
        for flat, rows in sync.bucket_layout():
            for p, off in rows:
                assert p.grad.data_ptr() == flat.data_ptr() + 4 * off
        open(os.path.join(result_dir, f"ok{rank}_{len(sync.bucket_sizes)}"), "w").close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("bucket_bytes,min_buckets", [(25 * 1024 * 1024, 1), (1024, 3)])
def test_accumulated_gradient_sync_equals_full_batch_training(tmp_path, bucket_bytes, min_buckets):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), bucket_bytes, str(tmp_path)), nprocs=world, join=True)
    done = sorted(os.listdir(tmp_path))
    assert [d.split("_")[0] for d in done] == ["ok0", "ok1"]
    assert all(int(d.split("_")[1]) >= min_buckets for d in done)


def _local_case():
    from zeroshotvideoclassification_amd import ddp
    torch.manual_seed(3)
    model = _Net()
    g = torch.Generator().manual_seed(11)
    x, z = torch.randn(7, 16, generator=g), torch.randn(7, 8, generator=g)
    sync = ddp.GradientSync(model, local=True, bucket_bytes=1024)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.0)
    return model, sync, opt, x, z


def test_micro_batch_sizes():
    from zeroshotvideoclassification_amd import train
    assert train.micro_batch_sizes(7, 3) == [3, 2, 2]
    assert train.micro_batch_sizes(6, 3) == [2, 2, 2]
    assert train.micro_batch_sizes(5, 5) == [1] * 5
    with pytest.raises(ValueError):
        train.micro_batch_sizes(2, 3)


def test_local_buckets_accumulate_unequal_parts():
    """N = 7, k = 3: parts of 3, 2, 2, so the weights n_j / N differ.  Two steps: discovery, then the armed buckets."""
    from zeroshotvideoclassification_amd import train
    model, sync, opt, x, z = _local_case()
    crit = torch.nn.MSELoss()
    crit(model(x), z).backward()
    ref = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    full_loss = crit(model(x), z).detach()
    for step in range(2):
        y, loss = train.train_step(model, opt, crit, x, z, sync, micro_batches=3)
        assert torch.allclose(y, model(x).detach(), rtol=1e-5, atol=1e-7)
        assert torch.allclose(loss, full_loss, rtol=1e-5, atol=1e-7)
        got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        assert set(got) == set(ref)
        for k in ref:
            assert torch.allclose(got[k], ref[k], rtol=1e-5, atol=1e-7), (step, k)
        assert len(sync.bucket_sizes) >= 3
        for flat, rows in sync.bucket_layout():
            for p, off in rows:
                assert p.grad.data_ptr() == flat.data_ptr() + 4 * off and p.grad.shape == p.shape
        assert sync.bytes_reduced_last_step == 4 * sum(sync.bucket_sizes)


def test_undeclared_second_backward_raises():
    from zeroshotvideoclassification_amd import train
    model, sync, opt, x, z = _local_case()
    crit = torch.nn.MSELoss()
    train.train_step(model, opt, crit, x, z, sync)                     # discovery
    sync.begin_step()
    crit(model(x), z).backward()
    with pytest.raises(RuntimeError, match=r"passes=.*micro_batches="):
        crit(model(x), z).backward()
    # declared passes that are not closed with end_pass() are caught the same way
    opt.zero_grad(set_to_none=True)
    sync.begin_step(passes=2)
    crit(model(x), z).backward()
    with pytest.raises(RuntimeError, match=r"passes=.*micro_batches="):
        crit(model(x), z).backward()


def test_finish_step_after_fewer_passes_than_declared_raises():
    model, sync, opt, x, z = _local_case()
    sync.begin_step(passes=3)
    torch.nn.MSELoss()(model(x), z).backward()
    sync.end_pass()
    torch.nn.MSELoss()(model(x), z).backward()
    with pytest.raises(RuntimeError, match="2 of the 3"):
        sync.finish_step()


def test_end_pass_outside_a_step_and_after_the_last_pass_raises():
    model, sync, opt, x, z = _local_case()
    with pytest.raises(RuntimeError, match=r"end_pass\(\) without begin_step"):
        sync.end_pass()
    sync.begin_step(passes=2)
    torch.nn.MSELoss()(model(x), z).backward()
    sync.end_pass()
    torch.nn.MSELoss()(model(x), z).backward()
    with pytest.raises(RuntimeError, match="finish_step"):
        sync.end_pass()
    sync.finish_step()
    with pytest.raises(RuntimeError, match=r"end_pass\(\) without begin_step"):
        sync.end_pass()
    with pytest.raises(ValueError):
        sync.begin_step(passes=0)


def test_a_pass_that_misses_a_live_gradient_raises():
    model, sync, opt, x, z = _local_case()
    crit = torch.nn.MSELoss()
    sync.begin_step(passes=2)
    crit(model(x), z).backward()
    sync.end_pass()                                                    # discovery: six live parameters
    assert sync.live_parameter_count == 6
    crit(model.a(x).sum(dim=1, keepdim=True).expand(-1, 8), z).backward()     # only a's two parameters
    with pytest.raises(RuntimeError, match="4 live parameters produced no gradient"):
        sync.finish_step()


def test_a_parameter_that_is_live_only_in_a_later_pass_raises():
    from zeroshotvideoclassification_amd import ddp
    model = _Net()
    sync = ddp.GradientSync(model, local=True)
    x = torch.randn(4, 16)
    sync.begin_step(passes=2)
    model(x).sum().backward()
    sync.end_pass()
    with pytest.raises(RuntimeError, match="live set is fixed"):
        (model(x).sum() + model.dead(torch.randn(2, 4)).sum()).backward()


def test_more_micro_batches_than_samples_raises():
    from zeroshotvideoclassification_amd import train
    model, sync, opt, x, z = _local_case()
    with pytest.raises(ValueError, match="micro_batches=8"):
        train.train_step(model, opt, torch.nn.MSELoss(), x, z, sync, micro_batches=8)
    with pytest.raises(ValueError):
        train.train_step(model, opt, torch.nn.MSELoss(), x, z, sync, micro_batches=0)


def test_accumulate_entry_point_is_declared_and_bound():
    import re
    from zeroshotvideoclassification_amd import _lib
    header = open(os.path.join(ROOT, "include", "zsv_hip.h")).read()
    declared = set(re.findall(r"\b(zsv_[a-z0-9_]+)\s*\(", header))
    assert "zsv_grad_accum_multi" in declared and "zsv_accum_tensor" in header
    assert _lib.SIGNATURES["zsv_grad_accum_multi"][1] == [_lib._P, _lib.c_int32, _lib.c_int64, _lib.c_float, _lib.c_int32, _lib._P]
    assert declared == set(_lib.SIGNATURES)
