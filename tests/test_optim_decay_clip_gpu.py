"""Weight decay (L2 and decoupled) and global-norm gradient clipping in ``optim.FusedAdam``, ``LossScaler.unscale_`` and the
``zsv_grad_norm_*`` entry points (csrc/optim.hip).  The yardstick is always torch's own optimizers on the same device:
``torch.optim.Adam(weight_decay=)`` / ``torch.optim.AdamW``, ``torch.nn.utils.clip_grad_norm_`` and ``torch.amp.GradScaler``.

Bars.  Parameters: ``2e-6 * max|p|`` after every step, the bar ``tests/test_optim_gpu.py`` holds ``FusedAdam`` to (decay and
clipping each add one rounding on the gradient's way in).  ``grad_norm``: ``2e-6`` relative of the float64 norm of the same
gradients -- a 4096-element chunk is summed as 16 serial adds per lane and an 8-level tree over 256 lanes, with the rounding of each
square at most 25 roundings of 2^-24 = 1.5e-6 on the sum of squares, half that on the norm; the cross-chunk sum is in double."""
import copy
import ctypes
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import make_opt  # noqa: E402
from test_optim_gpu import _Net, _loss, _params  # noqa: E402
from zeroshotvideoclassification_amd import _lib, amp, ddp, network, optim, synthetic, train  # noqa: E402

DEV = "cuda"
BAR = 2e-6
LR, WD, MAX_NORM = 1e-2, 0.05, 400.0


def _close(mine, ref, what):
    for i, (a, b) in enumerate(zip(mine, ref)):
        a, b = a.detach(), b.detach()
        err = (a - b).abs().max().item()
        bound = BAR * b.abs().max().item()
        print(f"{what} param {i}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, i, err, bound)


def _norm64(params):
    return torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)).item()


def _check_norm(opt, want, what):
    got = opt.grad_norm
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
    rel = abs(got.item() - want) / want
    print(f"{what}: grad_norm {got.item():.6f} float64 {want:.6f} rel {rel:.3e}")
    assert rel <= BAR, (what, got.item(), want)


def _factor(step):
    return 0.5 if step % 2 == 0 else 2.0


def _torch_opt(params, decoupled, **kw):
    return (torch.optim.AdamW if decoupled else torch.optim.Adam)(params, **kw)


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "l2"])
def test_weight_decay_matches_torch(decoupled):
    """Case 1: AdamW against torch.optim.AdamW, L2 against torch.optim.Adam(weight_decay=): 12 steps, lr 1e-2, decay 0.05."""
    ref_p, dev_p = _params(4, DEV), _params(4, DEV)
    ref_opt = _torch_opt(ref_p, decoupled, lr=LR, weight_decay=WD)
    dev_opt = optim.FusedAdam(dev_p, lr=LR, weight_decay=WD, decoupled_weight_decay=decoupled)
    for step in range(12):
        ref_opt.zero_grad(set_to_none=True)
        _loss(ref_p, step, None).backward()
        ref_opt.step()
        dev_opt.zero_grad(set_to_none=True)
        _loss(dev_p, step, None).backward()
        dev_opt.step()
        _close(dev_p, ref_p, f"decoupled={decoupled} step {step}")
    assert dev_opt.state_dict()["param_groups"][0]["weight_decay"] == WD
    assert dev_opt.state_dict()["param_groups"][0]["decoupled_weight_decay"] is decoupled


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "l2"])
def test_clipping_matches_clip_grad_norm(decoupled):
    """Case 2: the loss times 0.5 on even and 2.0 on odd steps, max_grad_norm 400: inactive on six steps, active on six."""
    ref_p, dev_p = _params(4, DEV), _params(4, DEV)
    ref_opt = _torch_opt(ref_p, decoupled, lr=LR, weight_decay=WD)
    dev_opt = optim.FusedAdam(dev_p, lr=LR, weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM)
    norms = []
    for step in range(12):
        ref_opt.zero_grad(set_to_none=True)
        (_loss(ref_p, step, None) * _factor(step)).backward()
        norms.append(torch.nn.utils.clip_grad_norm_(ref_p, MAX_NORM).item())
        ref_opt.step()
        dev_opt.zero_grad(set_to_none=True)
        (_loss(dev_p, step, None) * _factor(step)).backward()
        before = [p.grad.clone() for p in dev_p]
        dev_opt.step()
        _check_norm(dev_opt, _norm64(dev_p), f"step {step}")
        for p, g in zip(dev_p, before):
            assert torch.equal(p.grad, g)                                    # .grad is not rewritten
        _close(dev_p, ref_p, f"clip decoupled={decoupled} step {step}")
    print("torch norms", norms)
    assert sum(n > MAX_NORM for n in norms) == 6 and sum(n < MAX_NORM for n in norms) == 6


def _scaled_run(poison, steps=12, record=None):
    """Case 3's device side: LossScaler + AdamW decay + clipping.  Returns parameters, per-step grad_norm and the scaler."""
    dev_p = _params(4, DEV)
    dev_opt = optim.FusedAdam(dev_p, lr=LR, weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM)
    dev_scaler = optim.LossScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    norms = []
    for step in range(steps):
        dev_opt.zero_grad(set_to_none=True)
        dev_scaler.scale(_loss(dev_p, step, poison.get(step)) * _factor(step)).backward()
        held = [p.detach().clone() for p in dev_p]
        moments = [(dev_opt.state[p]["exp_avg"].clone(), dev_opt.state[p]["exp_avg_sq"].clone()) for p in dev_p if dev_opt.state[p]]
        dev_scaler.step(dev_opt)
        dev_scaler.update()
        norms.append(dev_opt.grad_norm.clone())
        if step in poison:
            # a skipped step leaves parameters, moments and decay untouched
            for p, q in zip(dev_p, held):
                assert torch.equal(p.detach(), q), step
            for p, (m, v) in zip(dev_p, moments):
                assert torch.equal(dev_opt.state[p]["exp_avg"], m) and torch.equal(dev_opt.state[p]["exp_avg_sq"], v), step
        if record is not None:
            record(step, dev_p, dev_scaler)
    return dev_p, norms, dev_scaler, dev_opt


POISON = {2: float("inf"), 5: float("nan"), 6: float("-inf")}


def test_scaler_decay_and_clipping_match_gradscaler():
    """Case 3: against GradScaler + unscale_ + clip_grad_norm_ + AdamW with inf / nan gradients at steps 2, 5 and 6."""
    ref_p = _params(4, DEV)
    ref_opt = torch.optim.AdamW(ref_p, lr=LR, weight_decay=WD)
    ref_scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    ref_state = {}

    def ref_step(step):
        ref_opt.zero_grad(set_to_none=True)
        ref_scaler.scale(_loss(ref_p, step, POISON.get(step)) * _factor(step)).backward()
        ref_scaler.unscale_(ref_opt)
        ref_state["norm"] = torch.nn.utils.clip_grad_norm_(ref_p, MAX_NORM).item()
        ref_scaler.step(ref_opt)
        ref_scaler.update()

    active = []

    def record(step, dev_p, dev_scaler):
        ref_step(step)
        st = dev_scaler.state()
        assert st["scale"] == ref_scaler.get_scale(), (step, st)
        assert st["growth_tracker"] == int(ref_scaler.state_dict()["_growth_tracker"]), (step, st)
        assert st["found_inf"] == 0
        _close(dev_p, ref_p, f"scaled step {step}")
        if step not in POISON:
            active.append(ref_state["norm"] > MAX_NORM)

    dev_p, norms, dev_scaler, dev_opt = _scaled_run(POISON, record=record)
    st = dev_scaler.state()
    assert st["steps_done"] == 12 - len(POISON)
    assert float(ref_opt.state[ref_p[0]]["step"]) == st["steps_done"]
    assert float(dev_opt.state_dict()["state"][0]["step"]) == st["steps_done"]
    assert any(active) and not all(active)


def test_unscale_recipe_matches_the_fused_route_and_torch():
    """Case 4: scaler.unscale_(opt); torch.nn.utils.clip_grad_norm_(...); scaler.step(opt) on a FusedAdam, against the fused
    route (max_grad_norm=) and against torch's GradScaler + AdamW."""
    scale = 1000.0
    inv = torch.tensor(scale, dtype=torch.float32).double().reciprocal().float().to(DEV)
    lit_p, fus_p, ref_p = _params(4, DEV), _params(4, DEV), _params(4, DEV)
    lit_opt = optim.FusedAdam(lit_p, lr=LR, weight_decay=WD, decoupled_weight_decay=True)
    fus_opt = optim.FusedAdam(fus_p, lr=LR, weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM)
    ref_opt = torch.optim.AdamW(ref_p, lr=LR, weight_decay=WD)
    lit_s, fus_s = optim.LossScaler(init_scale=scale), optim.LossScaler(init_scale=scale)
    ref_s = torch.amp.GradScaler("cuda", init_scale=scale)
    for step in range(6):
        lit_opt.zero_grad(set_to_none=True)
        lit_s.scale(_loss(lit_p, step, None) * _factor(step)).backward()
        scaled = [p.grad.clone() for p in lit_p]
        lit_s.unscale_(lit_opt)
        for p, g in zip(lit_p, scaled):
            assert torch.equal(p.grad, g * inv), step                       # exactly the scaled gradient times 1/scale
        with pytest.raises(RuntimeError, match="unscale_"):
            lit_s.unscale_(lit_opt)
        torch.nn.utils.clip_grad_norm_(lit_p, MAX_NORM)
        lit_s.step(lit_opt)
        lit_s.update()

        fus_opt.zero_grad(set_to_none=True)
        fus_s.scale(_loss(fus_p, step, None) * _factor(step)).backward()
        fus_s.step(fus_opt)
        fus_s.update()

        ref_opt.zero_grad(set_to_none=True)
        ref_s.scale(_loss(ref_p, step, None) * _factor(step)).backward()
        ref_s.unscale_(ref_opt)
        torch.nn.utils.clip_grad_norm_(ref_p, MAX_NORM)
        ref_s.step(ref_opt)
        ref_s.update()
        _close(lit_p, ref_p, f"literal vs torch step {step}")
        _close(fus_p, ref_p, f"fused vs torch step {step}")
        _close(lit_p, fus_p, f"literal vs fused step {step}")
    assert lit_s.state()["steps_done"] == fus_s.state()["steps_done"] == 6
    # a non-finite gradient seen by unscale_ skips the step, as GradScaler's does
    held = [p.detach().clone() for p in lit_p]
    lit_opt.zero_grad(set_to_none=True)
    lit_s.scale(_loss(lit_p, 6, float("inf"))).backward()
    lit_s.unscale_(lit_opt)
    lit_s.step(lit_opt)
    lit_s.update()
    for p, q in zip(lit_p, held):
        assert torch.equal(p.detach(), q)
    assert lit_s.state()["steps_done"] == 6 and lit_s.get_scale() == scale * 0.5


def test_two_groups_share_one_global_norm():
    """Case 5: two parameter groups (different lr and weight decay, one group without decay), one norm over both."""
    pa, pb = _params(11, DEV), _params(12, DEV)
    ra, rb = [p.detach().clone().requires_grad_() for p in pa], [p.detach().clone().requires_grad_() for p in pb]
    opt = optim.FusedAdam([{"params": pa, "weight_decay": WD}, {"params": pb, "lr": 3e-3}], lr=LR, weight_decay=0.0,
                          decoupled_weight_decay=True, max_grad_norm=MAX_NORM)
    ref_opt = torch.optim.AdamW([{"params": ra, "weight_decay": WD}, {"params": rb, "lr": 3e-3}], lr=LR, weight_decay=0.0)
    norms = []
    for step in range(8):
        ref_opt.zero_grad(set_to_none=True)
        ((_loss(ra, step, None) + _loss(rb, 50 + step, None)) * _factor(step)).backward()
        norms.append(torch.nn.utils.clip_grad_norm_(ra + rb, MAX_NORM).item())
        ref_opt.step()
        opt.zero_grad(set_to_none=True)
        ((_loss(pa, step, None) + _loss(pb, 50 + step, None)) * _factor(step)).backward()
        opt.step()
        _check_norm(opt, _norm64(pa + pb), f"two groups step {step}")
        _close(pa + pb, ra + rb, f"two groups step {step}")
    print("torch norms", norms)
    assert any(n > MAX_NORM for n in norms) and any(n < MAX_NORM for n in norms)


@pytest.mark.parametrize("use_scaler", [False, True])
def test_decay_and_clipping_on_the_bucket_table(use_scaler):
    """Case 6: GradientSync(local=True) + FusedAdam(grad_buckets=...): the norm pass and the update walk the table built once
    over the flat buckets.  The torch twin is fed clones of the same gradients, so only the optimizer differs."""
    torch.manual_seed(3)
    model = _Net().to(DEV)
    ref = copy.deepcopy(model)
    dead0 = [p.detach().clone() for p in model.dead.parameters()]
    sync = ddp.GradientSync(model, bucket_bytes=200 * 1024, local=True)
    max_norm = 2.0                                                           # between the small-target and large-target steps
    opt = optim.FusedAdam(model.parameters(), lr=LR, weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=max_norm,
                          grad_buckets=sync)
    ref_opt = torch.optim.AdamW(ref.parameters(), lr=LR, weight_decay=WD)
    scaler = optim.LossScaler(init_scale=256.0) if use_scaler else None
    g = torch.Generator().manual_seed(9)
    crit = torch.nn.MSELoss()
    norms = []
    for step in range(6):
        x, z = torch.randn(16, 40, generator=g).to(DEV), torch.randn(16, 20, generator=g).to(DEV)
        z = z * (1.0 if step % 2 == 0 else 8.0)                              # small and large gradients in turn
        train.train_step(model, opt, crit, x, z, sync, scaler)
        inv = 1.0 / 256.0 if use_scaler else 1.0
        ref_opt.zero_grad(set_to_none=True)
        for p, q in zip(model.parameters(), ref.parameters()):
            q.grad = None if p.grad is None else p.grad.detach().clone() * inv
        want = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in ref.parameters() if q.grad is not None)).item()
        norms.append(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm).item())
        ref_opt.step()
        _check_norm(opt, want, f"buckets step {step}")
        _close(list(model.parameters()), list(ref.parameters()), f"buckets step {step}")
        if step >= 1:
            assert opt._static is not None and opt._static[0] == sync.layout_version       # the bucket table was walked
    print("torch norms", norms)
    assert any(n > max_norm for n in norms) and any(n < max_norm for n in norms)
    # the dead layer: no gradient, not in the norm, no decay
    assert model.dead.weight.grad is None and not opt.state[model.dead.weight]
    for p, q in zip(model.dead.parameters(), dead0):
        assert torch.equal(p.detach(), q)


def test_two_runs_are_bit_identical():
    """Case 7: no floating-point atomics -- two runs of case 3 from the same seeds agree in every bit."""
    p1, n1, _, _ = _scaled_run(POISON)
    p2, n2, _, _ = _scaled_run(POISON)
    for a, b in zip(p1, p2):
        assert torch.equal(a.detach(), b.detach())
    for step, (a, b) in enumerate(zip(n1, n2)):
        if step not in POISON:                                               # only finite steps are specified
            assert torch.isfinite(a) and torch.equal(a, b), step


def test_defaults_launch_what_they_always_did():
    """Case 8: FusedAdam(ps, lr) and FusedAdam(ps, lr, weight_decay=0.0, max_grad_norm=None) are the same optimizer."""
    pa, pb = _params(4, DEV), _params(4, DEV)
    oa = optim.FusedAdam(pa, lr=LR)
    ob = optim.FusedAdam(pb, lr=LR, weight_decay=0.0, max_grad_norm=None)
    for step in range(5):
        for ps, o in ((pa, oa), (pb, ob)):
            o.zero_grad(set_to_none=True)
            _loss(ps, step, None).backward()
            o.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
        assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        oa.grad_norm


def test_in_the_model_under_autocast_with_the_scaler():
    """Case 9: network.Model over r2plus1d_18, 2 clips of 3x8x56x56, three LossScaler steps under amp.autocast(): decay in the
    trunk group, none in the head group, max_grad_norm = half the norm torch reports on step 1 (so the clip is active).  A torch
    AdamW + GradScaler twin is fed clones of the same (scaled) gradients each step, so only the optimizer differs."""
    model = network.get_network(make_opt("r2plus1d_18"))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
    model.to(DEV).train()
    for p in model.model.stem.parameters():
        p.requires_grad_(False)                                             # a frozen part of the trunk
    twin = copy.deepcopy(model)
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    trunk_ids = {id(p) for p in model.model.parameters()}

    def groups(m, ids):
        ps = list(m.parameters())
        return [{"params": [p for p in ps if id(p) in ids], "weight_decay": WD},
                {"params": [p for p in ps if id(p) not in ids], "weight_decay": 0.0}]

    lr, scale = 1e-4, 2.0 ** 10
    ref_opt = torch.optim.AdamW(groups(twin, {id(p) for p in twin.model.parameters()}), lr=lr)
    ref_scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    scaler = optim.LossScaler(init_scale=scale)
    x = synthetic.synthetic_clips(2, 8, 56).to(DEV)
    _, z = synthetic.synthetic_targets(2)
    z = z.to(DEV)
    opt, max_norm = None, None
    for step in range(3):
        model.zero_grad(set_to_none=True)
        with amp.autocast():
            loss = torch.nn.functional.mse_loss(train.embed(model, x), z)
        scaler.scale(loss).backward()
        ref_scaler.scale(torch.zeros((), device=DEV))                       # (GradScaler wants scale() before unscale_())
        ref_opt.zero_grad(set_to_none=True)
        for p, q in zip(model.parameters(), twin.parameters()):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        ref_scaler.unscale_(ref_opt)
        live = [q for q in twin.parameters() if q.grad is not None]
        if max_norm is None:
            max_norm = 0.5 * torch.nn.utils.clip_grad_norm_(live, float("inf")).item()
            assert max_norm > 0 and max_norm == max_norm and max_norm != float("inf")
            opt = optim.FusedAdam(groups(model, trunk_ids), lr=lr, decoupled_weight_decay=True, max_grad_norm=max_norm)
        want = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in live)).item()
        norm = torch.nn.utils.clip_grad_norm_(live, max_norm).item()
        ref_scaler.step(ref_opt)
        ref_scaler.update()
        scaler.step(opt)
        scaler.update()
        _check_norm(opt, want, f"model step {step}")
        print(f"model step {step}: torch norm {norm:.6f}, max_norm {max_norm:.6f}")
        if step == 0:
            assert norm > max_norm                                           # the clip is active
        moved = 0
        for (k, p), q in zip(model.named_parameters(), twin.parameters()):
            if p.grad is None:
                assert torch.equal(p.detach(), start[k]), k                 # frozen / dead: bit-unchanged (no decay either)
                continue
            moved += 1
            err = (p.detach() - q.detach()).abs().max().item()
            assert err <= BAR * q.detach().abs().max().item(), (step, k, err)
        assert moved > 50
    assert scaler.state()["steps_done"] == 3
    assert all(p.grad is None for p in model.model.stem.parameters()) and model.encoder.layers[0].linear1.weight.grad is None


def _table(rows):
    """Hand-built zsv_adam_tensor table {p, g, exp_avg, exp_avg_sq, n, first_chunk} over gradient tensors only."""
    raw, first = b"", 0
    for g in rows:
        raw += struct.pack("<QQQQqq", 0, g.data_ptr(), 0, 0, g.numel(), first)
        first += (g.numel() + 4095) // 4096
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV), len(rows), first


def test_raw_norm_entry_points_against_float64():
    """Case 10: zsv_grad_norm_workspace_bytes / zsv_grad_norm_multi / zsv_grad_norm_finalize through ctypes: two tables into one
    partials buffer, per-chunk sums and the total against float64, the clip record, the scaler's 1/scale and found_inf."""
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(77)
    a = [torch.randn(n, generator=gen).to(DEV) for n in (1, 4097, 5000, 10000)]
    b = [torch.randn(n, generator=gen).to(DEV) * 3 for n in (4096, 33)]
    ta, ca, ka = _table(a)
    tb, cb, kb = _table(b)
    assert (ka, kb) == (1 + 2 + 2 + 3, 1 + 1)
    total = ka + kb
    nbytes = lib.zsv_grad_norm_workspace_bytes(total)
    assert nbytes >= 4 * total and lib.zsv_grad_norm_workspace_bytes(0) == 0
    partials = torch.full((nbytes // 4,), -1.0, dtype=torch.float32, device=DEV)
    record = torch.zeros(2, dtype=torch.float32, device=DEV)
    # a buffer too small for chunk_offset + total_chunks is refused before anything is launched
    assert lib.zsv_grad_norm_multi(tb.data_ptr(), cb, kb, ka, partials.data_ptr(), 4 * total - 4, None, stream) != 0
    _lib.check(lib.zsv_grad_norm_multi(ta.data_ptr(), ca, ka, 0, partials.data_ptr(), nbytes, None, stream), "norm a")
    _lib.check(lib.zsv_grad_norm_multi(tb.data_ptr(), cb, kb, ka, partials.data_ptr(), nbytes, None, stream), "norm b")
    want = []
    for g in a + b:
        want += [(c.double() ** 2).sum().item() for c in g.split(4096)]
    got = partials[:total].cpu().double().tolist()
    assert len(want) == total
    for i, (u, v) in enumerate(zip(got, want)):
        assert abs(u - v) <= 2 * BAR * v, (i, u, v)                          # sum of squares: twice the norm's bar
    norm64 = sum(want) ** 0.5
    for max_norm in (0.5 * norm64, 2.0 * norm64):
        _lib.check(lib.zsv_grad_norm_finalize(partials.data_ptr(), total, max_norm, None, record.data_ptr(), stream), "finalize")
        n, c = record.cpu().tolist()
        assert abs(n - norm64) <= BAR * norm64
        assert abs(c - min(1.0, max_norm / (norm64 + 1e-6))) <= 1e-6
    assert lib.zsv_grad_norm_finalize(partials.data_ptr(), total, 0.0, None, record.data_ptr(), stream) != 0
    # with a scaler state: 1/scale on the norm, found_inf from the same pass
    state = torch.zeros(4, dtype=torch.int32)
    state.view(torch.float32)[0] = 128.0
    state = state.to(DEV)
    _lib.check(lib.zsv_grad_norm_multi(ta.data_ptr(), ca, ka, 0, partials.data_ptr(), nbytes, state.data_ptr(), stream), "norm a")
    _lib.check(lib.zsv_grad_norm_multi(tb.data_ptr(), cb, kb, ka, partials.data_ptr(), nbytes, state.data_ptr(), stream), "norm b")
    _lib.check(lib.zsv_grad_norm_finalize(partials.data_ptr(), total, 1.0, state.data_ptr(), record.data_ptr(), stream), "finalize")
    n, c = record.cpu().tolist()
    assert abs(n - norm64 / 128.0) <= BAR * norm64 / 128.0 and abs(c - 1.0 / (norm64 / 128.0 + 1e-6)) <= 1e-6 * c
    assert int(state.cpu()[2]) == 0
    b[1][7] = float("nan")
    _lib.check(lib.zsv_grad_norm_multi(tb.data_ptr(), cb, kb, ka, partials.data_ptr(), nbytes, state.data_ptr(), stream), "norm b")
    assert int(state.cpu()[2]) == 1
    # zsv_grad_unscale_multi: in place, exact
    state2 = torch.zeros(4, dtype=torch.int32)
    state2.view(torch.float32)[0] = 3.0
    state2 = state2.to(DEV)
    before = [g.clone() for g in a]
    _lib.check(lib.zsv_grad_unscale_multi(ta.data_ptr(), ca, ka, state2.data_ptr(), stream), "unscale")
    inv = torch.tensor(3.0).double().reciprocal().float().to(DEV)
    for g, g0 in zip(a, before):
        assert torch.equal(g, g0 * inv)
    assert int(state2.cpu()[2]) == 0
