"""``optim.WeightAverage``: EMA / equal-weight averaging of the weights inside ``FusedAdam``'s update launch, the device-resident
count of averaged steps, ``applied()`` and the raw ``zsv_avg_multi`` / ``zsv_swap_multi`` / ``zsv_avg_advance`` entry points.

The yardstick is torch: ``torch.optim.Adam`` / ``AdamW`` (+ ``clip_grad_norm_``, ``torch.amp.GradScaler``) stepping a copy of the
parameters, and ``torch.optim.swa_utils.AveragedModel`` over that copy, ``update_parameters`` after every step torch took.

Bar for a shadow, per tensor: ``(2e-6 + B) * max|ref|``.  ``2e-6`` is the bar ``tests/test_optim_gpu.py`` holds ``FusedAdam``'s
parameters to, and the shadow is a convex combination of those parameters.  ``B`` bounds the averaging's own rounding: a step
adds at most two fp32 roundings and the recurrence contracts by ``d``, so ``B = 2^-23 / (1 - d)`` for EMA; for the equal-weight
mean nothing contracts and ``B = steps * 2^-23``.  A single application of the rule on raw arrays (three roundings: the
difference, the product, the sum) is held to ``3 * 2^-23 * max(|avg|, |p|)`` of float64."""
import copy
import ctypes
import struct

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

pytestmark = pytest.mark.gpu

from helpers import make_opt  # noqa: E402
from test_optim_gpu import _Net, _loss, _params  # noqa: E402
from zeroshotvideoclassification_amd import _lib, ddp, inference, layers, network, optim, synthetic, train  # noqa: E402

DEV = "cuda"
EPS = 2.0 ** -23
LR, WD, MAX_NORM = 1e-2, 0.05, 400.0
MODES = {"adam": {}, "adamw_clip": dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM),
         "l2": dict(weight_decay=WD)}
POISON = {0: float("inf"), 2: float("inf"), 5: float("nan"), 6: float("-inf")}


def _factor(step):
    return 0.5 if step % 2 == 0 else 2.0        # max_grad_norm 400 is then active on the odd steps only


def _bar_ema(d):
    return 2e-6 + EPS / (1.0 - d)


def _close(shadows, refs, bar, what):
    for i, (a, b) in enumerate(zip(shadows, refs)):
        a, b = a.detach(), b.detach()
        err, bound = (a - b).abs().max().item(), bar * b.abs().max().item()
        print(f"{what} shadow {i}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, i, err, bound)


class _Holder(torch.nn.Module):
    """The oracle's parameters as a module, which is what AveragedModel wraps."""

    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.detach().clone()) for t in tensors])


def _averaged(holder, decay, **kw):
    return AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(decay), **kw) if decay is not None else AveragedModel(holder, **kw)


def _torch_run(mode, decay, steps=12, poison=None, use_scaler=False):
    """torch.optim + [clip_grad_norm_] + [GradScaler] + AveragedModel; update_parameters on the steps torch took."""
    kw = dict(MODES[mode])
    max_norm = kw.pop("max_grad_norm", None)
    decoupled = kw.pop("decoupled_weight_decay", False)
    holder = _Holder(_params(4, DEV))
    ps = list(holder.ps)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ps, lr=LR, **kw)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3) if use_scaler else None
    avg = _averaged(holder, decay)
    poison = poison or {}
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = _loss(ps, step, poison.get(step)) * _factor(step)
        if scaler is not None:
            scaler.scale(loss).backward()
            if max_norm is not None:
                scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_(ps, max_norm)
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
        if step not in poison:
            avg.update_parameters(holder)
    return list(avg.module.ps), ps


def _device_run(mode, decay, steps=12, poison=None, use_scaler=False, average=True, unscale_first=False, after_step=None):
    ps = _params(4, DEV)
    opt = optim.FusedAdam(ps, lr=LR, **MODES[mode])
    avg = optim.WeightAverage(opt, decay=decay) if average else None
    scaler = optim.LossScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3) if use_scaler else None
    poison = poison or {}
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = _loss(ps, step, poison.get(step)) * _factor(step)
        held = [s.clone() for s in avg.shadows().values()] if avg is not None and step in poison else None
        if scaler is not None:
            scaler.scale(loss).backward()
            if unscale_first:
                scaler.unscale_(opt)
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        if held is not None:
            for s, h in zip(avg.shadows().values(), held):
                assert torch.equal(s, h), step                               # a skipped step averages nothing
        if after_step is not None:
            after_step(step, ps, opt, avg)
    return ps, opt, avg, scaler


def _same_update(ps, opt, ps0, opt0):
    for a, b in zip(ps, ps0):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(opt.state[a]["exp_avg"], opt0.state[b]["exp_avg"])
        assert torch.equal(opt.state[a]["exp_avg_sq"], opt0.state[b]["exp_avg_sq"])


@pytest.mark.parametrize("mode", ["adam", "adamw_clip", "l2"])
def test_ema_matches_averaged_model(mode):
    """1: d = 0.9, 12 steps.  The shadows against AveragedModel; parameters and moments bit-equal to the run without averaging."""
    want, _ = _torch_run(mode, 0.9)
    ps, opt, avg, _ = _device_run(mode, 0.9)
    ps0, opt0, _, _ = _device_run(mode, 0.9, average=False)
    _close(avg.shadows().values(), want, _bar_ema(0.9), f"ema {mode}")
    _same_update(ps, opt, ps0, opt0)
    assert avg.n_averaged.is_cuda and avg.n_averaged.dim() == 0 and int(avg.n_averaged) == 12
    assert list(avg.shadows()) == list(range(6))                             # no model: keyed by position
    flat = next(iter(avg._flat.values()))
    offset = 0
    for p, s in zip(ps, avg.shadows().values()):                             # views of ONE flat buffer
        assert s.data_ptr() == flat.data_ptr() + 4 * offset and s.shape == p.shape
        offset += p.numel()


def test_equal_weight_matches_averaged_model():
    """2: decay=None against AveragedModel's default; the second averaged step has w = 0.5, the second branch of torch's lerp."""
    steps = 12
    seen = []
    want, _ = _torch_run("adam", None, steps)
    ps, opt, avg, _ = _device_run("adam", None, steps, after_step=lambda step, ps, opt, avg: seen.append(
        [s.clone() for s in avg.shadows().values()] + [p.detach().clone() for p in ps]))
    ps0, opt0, _, _ = _device_run("adam", None, steps, average=False)
    _close(avg.shadows().values(), want, 2e-6 + steps * EPS, "swa")
    _same_update(ps, opt, ps0, opt0)
    assert int(avg.n_averaged) == steps
    for s, p in zip(seen[0][:6], seen[0][6:]):
        assert torch.equal(s, p)                                             # the first averaged step copies
    for s0, s1, p1 in zip(seen[0][:6], seen[1][:6], seen[1][6:]):            # w = 0.5: p - (p - avg) * 0.5, one application
        ref = p1.double() - (p1.double() - s0.double()) * 0.5
        assert (s1.double() - ref).abs().max().item() <= 3 * EPS * max(p1.abs().max().item(), s0.abs().max().item())


@pytest.mark.parametrize("mode,unscale_first", [("adam", False), ("adamw_clip", False), ("adamw_clip", True)],
                         ids=["adam", "adamw_clip", "adamw_clip_unscaled"])
def test_under_the_loss_scaler(mode, unscale_first):
    """3: poisoned gradients at steps 0, 2, 5 and 6.  The first TAKEN step is step 1, so the copy rule is decided on the device;
    a skipped step leaves the shadows bit-equal (asserted in _device_run); n_averaged counts the steps taken."""
    counts = []
    want, _ = _torch_run(mode, 0.9, poison=POISON, use_scaler=True)
    ps, opt, avg, scaler = _device_run(mode, 0.9, poison=POISON, use_scaler=True, unscale_first=unscale_first,
                                       after_step=lambda step, ps, opt, avg: counts.append(int(avg.n_averaged)))
    ps0, opt0, _, _ = _device_run(mode, 0.9, poison=POISON, use_scaler=True, unscale_first=unscale_first, average=False)
    _close(avg.shadows().values(), want, _bar_ema(0.9), f"scaled {mode}")
    _same_update(ps, opt, ps0, opt0)
    taken = 0
    for step in range(12):
        taken += step not in POISON
        assert counts[step] == taken, (step, counts)
    assert int(avg.n_averaged) == 12 - len(POISON) == scaler.state()["steps_done"]


def _net_run(buckets, steps=5, micro_steps=2):
    torch.manual_seed(3)
    model = _Net().to(DEV)
    sync = ddp.GradientSync(model, bucket_bytes=200 * 1024, local=True)
    opt = optim.FusedAdam(model.parameters(), lr=LR, grad_buckets=sync if buckets else None)
    avg = optim.WeightAverage(opt, decay=0.9, model=model)
    g = torch.Generator().manual_seed(9)
    crit = torch.nn.MSELoss()
    counts = []
    for step in range(steps + micro_steps):
        x, z = torch.randn(16, 40, generator=g).to(DEV), torch.randn(16, 20, generator=g).to(DEV)
        train.train_step(model, opt, crit, x, z, sync, micro_batches=2 if step >= steps else 1)
        counts.append(int(avg.n_averaged))
    return model, opt, avg, counts


def test_bucket_route_matches_the_dynamic_route():
    """4: FusedAdam(grad_buckets=) -- the static table with the shadow pointers behind it -- against the per-step table."""
    model, opt, avg, counts = _net_run(True)
    model0, opt0, avg0, counts0 = _net_run(False)
    assert opt._static is not None and opt0._static is None                 # the two routes really were taken
    assert list(avg.shadows()) == [k for k, _ in model.named_parameters()]  # with a model: keyed by state_dict name
    _close(avg.shadows().values(), avg0.shadows().values(), _bar_ema(0.9), "buckets")
    for (k, p), (_, q) in zip(model.named_parameters(), model0.named_parameters()):
        assert (p - q).abs().max().item() <= 2e-6 * q.abs().max().item(), k
    for k in ("dead.weight", "dead.bias"):                                  # never a gradient: avg == p
        assert torch.equal(avg.shadows()[k], dict(model.named_parameters())[k].detach())
    assert model.dead.weight.grad is None
    # once per train_step, with micro_batches=2 (the last two) as well
    assert counts == list(range(1, 8)) and counts0 == counts


class _Norm(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bn = layers.BatchNorm3d(4)

    def forward(self, x):
        return self.bn(x)


def test_batchnorm_buffers_are_averaged():
    """5: running_mean / running_var against AveragedModel(use_buffers=True) fed the same live module after every step;
    num_batches_tracked is not shadowed and stays live under applied()."""
    torch.manual_seed(5)
    model = _Norm().to(DEV).train()
    opt = optim.FusedAdam(model.parameters(), lr=LR)
    avg = optim.WeightAverage(opt, decay=0.9, model=model, buffers=True)
    ref = _averaged(model, 0.9, use_buffers=True)
    assert set(avg.shadows()) == {"bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"}
    g = torch.Generator().manual_seed(6)
    for step in range(6):
        x = (torch.randn(2, 4, 2, 4, 4, generator=g) * (1 + step) + step).to(DEV)
        w = torch.randn(2, 4, 2, 4, 4, generator=g).to(DEV)
        opt.zero_grad(set_to_none=True)
        (model(x) * w).sum().backward()
        opt.step()
        ref.update_parameters(model)
    want = dict(ref.module.state_dict())
    live = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, s in avg.shadows().items():
        _close([s], [want[k]], _bar_ema(0.9), k)
        assert not torch.equal(s, live[k]), k                                # the average is not the live value
    assert int(live["bn.num_batches_tracked"]) == 6
    with avg.applied():
        assert int(model.bn.num_batches_tracked) == 6
        for k in ("bn.running_mean", "bn.running_var"):
            assert not torch.equal(model.state_dict()[k], live[k])
            _close([model.state_dict()[k]], [want[k]], _bar_ema(0.9), "applied " + k)
    for k, v in model.state_dict().items():
        assert torch.equal(v, live[k]), k
    # without buffers= only the parameters are shadowed
    opt2 = optim.FusedAdam(model.parameters(), lr=LR)
    assert set(optim.WeightAverage(opt2, model=model, buffers=False).shadows()) == {"bn.weight", "bn.bias"}
    with pytest.raises(RuntimeError, match="one per optimizer"):
        optim.WeightAverage(opt2)


def test_applied_on_the_model(tmp_path):
    """6: R(2+1)D-18, 2 clips of 3x8x56x56, three steps with d = 0.5."""
    model = network.get_network(make_opt("r2plus1d_18"))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
    model.to(DEV).train()
    opt = optim.FusedAdam(model.parameters(), lr=1e-4)
    avg = optim.WeightAverage(opt, decay=0.5, model=model)
    x = synthetic.synthetic_clips(2, 8, 56).to(DEV)
    _, z = synthetic.synthetic_targets(2)
    z = z.to(DEV)
    for _ in range(3):
        train.train_step(model, opt, torch.nn.MSELoss(), x, z)
    assert int(avg.n_averaged) == 3
    live = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pointers = {k: v.data_ptr() for k, v in model.state_dict().items()}
    shadows = {k: s.clone() for k, s in avg.shadows().items()}
    moved = sum(not torch.equal(shadows[k], live[k]) for k in shadows)
    assert moved > 50                                                        # the average differs from the live weights

    path = str(tmp_path / "ckpt.pth.tar")
    train.save_checkpoint(model, path, None, 0.25, average=avg)
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert set(saved) == {"state_dict", "opt", "accuracy", "state_dict_avg"}
    assert set(saved["state_dict_avg"]) == set(saved["state_dict"]) == {"module." + k for k in live}
    for k in live:
        assert torch.equal(saved["state_dict"]["module." + k], live[k].cpu()), k
        assert torch.equal(saved["state_dict_avg"]["module." + k], shadows.get(k, live[k]).cpu()), k
    fresh = network.get_network(make_opt("r2plus1d_18"))
    assert train.load_weights(fresh, path, key="state_dict_avg") == len(live)
    fresh.to(DEV).eval()
    with torch.no_grad():
        want = train.embed(fresh, x)
        want16 = train.embed(inference.engine_for(fresh, torch.bfloat16), x)

    with avg.applied():
        for k, v in model.state_dict().items():
            assert v.data_ptr() == pointers[k], k                            # in place: nothing moved
            assert torch.equal(v, shadows.get(k, live[k])), k
        for k, s in avg.shadows().items():
            assert torch.equal(s, live[k]), k                                # the live values wait in the shadows
        model.eval()
        with torch.no_grad():
            got = train.embed(model, x)
            got16 = train.embed(inference.engine_for(model, torch.bfloat16), x)
        model.train()
        assert torch.equal(got, want)
        assert torch.equal(got16, want16)
        with pytest.raises(RuntimeError, match="nested"):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            opt.step()
        with pytest.raises(RuntimeError, match="applied"):
            avg.state_dict()
    for k, v in model.state_dict().items():
        assert v.data_ptr() == pointers[k] and torch.equal(v, live[k]), k    # restored bit for bit
    for k, s in avg.shadows().items():
        assert torch.equal(s, shadows[k]), k
    with torch.no_grad():
        model.eval()
        back = train.embed(inference.engine_for(model, torch.bfloat16), x)   # the engine follows the swap back
        model.train()
    assert not torch.equal(back, got16)
    # evaluate(average=) is the same context as one argument
    table = torch.nn.functional.normalize(torch.randn(7, z.shape[-1], generator=torch.Generator().manual_seed(1)), dim=-1)
    batches = [(x, torch.tensor([0, 1]), table[:2])]
    with avg.applied():
        inside = train.evaluate(model, batches, table, splits=0, dtype=torch.bfloat16)
    assert train.evaluate(model, batches, table, splits=0, dtype=torch.bfloat16, average=avg) == inside
    for k, v in model.state_dict().items():
        assert torch.equal(v, live[k]), k
    train.train_step(model, opt, torch.nn.MSELoss(), x, z)                   # and training goes on
    assert int(avg.n_averaged) == 4


def test_resume_is_bit_equal_to_the_uninterrupted_run():
    """7: four steps, state_dict() of optimizer and average into fresh objects, four more steps.  Equal-weight, so the loaded
    count decides every weight."""
    ps, opt, avg, _ = _device_run("adamw_clip", None, steps=8)

    ps1, opt1, avg1, _ = _device_run("adamw_clip", None, steps=4)
    opt_state, avg_state = copy.deepcopy(opt1.state_dict()), avg1.state_dict()
    assert avg_state["n_averaged"] == 4 and avg_state["decay"] is None and list(avg_state["shadows"]) == list(range(6))
    ps2 = [p.detach().clone().requires_grad_() for p in ps1]
    opt2 = optim.FusedAdam(ps2, lr=LR, **MODES["adamw_clip"])
    opt2.load_state_dict(opt_state)
    avg2 = optim.WeightAverage(opt2)                                         # built as an EMA: the saved decay wins
    avg2.load_state_dict(avg_state)
    assert avg2.decay is None and int(avg2.n_averaged) == 4
    for step in range(4, 8):
        opt2.zero_grad(set_to_none=True)
        (_loss(ps2, step, None) * _factor(step)).backward()
        opt2.step()
    for a, b in zip(ps2, ps):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(avg2.shadows().values(), avg.shadows().values()):
        assert torch.equal(a, b)
    assert int(avg2.n_averaged) == 8
    with pytest.raises(KeyError):
        avg2.load_state_dict({"n_averaged": 1, "decay": 0.5, "shadows": {0: avg_state["shadows"][0]}})


OFFSETS, LENGTHS = (1, 2, 3), (1, 255, 4095, 4096, 4097, 5000)
SENTINEL = -12345.0


def _slices(seed, shift):
    """One flat buffer of sentinels with a slice per (offset, length): slice j starts at an element offset = (offset + shift)
    mod 4 past a 16-byte boundary, with at least one sentinel between neighbours."""
    spans, cursor = [], 0
    for off in OFFSETS:
        for n in LENGTHS:
            cursor += 1
            while cursor % 4 != (off + shift) % 4:
                cursor += 1
            spans.append((cursor, n))
            cursor += n
    flat = torch.full((cursor + 5,), SENTINEL, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    for start, n in spans:
        flat[start:start + n] = torch.randn(n, generator=g)
    mask = torch.ones_like(flat, dtype=torch.bool)
    for start, n in spans:
        mask[start:start + n] = False
    flat = flat.to(DEV)
    assert flat.data_ptr() % 16 == 0
    return flat, spans, mask.to(DEV)


def _pair_table(a, a_spans, b, b_spans):
    raw, first = b"", 0
    for (sa, n), (sb, m) in zip(a_spans, b_spans):
        assert n == m
        raw += struct.pack("<QQqq", a.data_ptr() + 4 * sa, b.data_ptr() + 4 * sb, n, first)
        first += (n + 4095) // 4096
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV), len(a_spans), first


@pytest.mark.parametrize("shift", [0, 1], ids=["same_alignment", "different_alignment"])
def test_raw_entry_points(shift):
    """8: zsv_avg_multi / zsv_swap_multi / zsv_avg_advance through ctypes on slices of flat buffers."""
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src, src_spans, src_mask = _slices(1, shift)                             # the live side `a`
    avg, avg_spans, avg_mask = _slices(2, 0)                                 # the shadows `b`
    table, count, chunks = _pair_table(src, src_spans, avg, avg_spans)
    assert count == 18 and chunks == 3 * (1 + 1 + 1 + 1 + 2 + 2)
    src0, avg0 = src.clone(), avg.clone()
    state = torch.zeros(1, dtype=torch.int32, device=DEV)
    scaler = torch.zeros(4, dtype=torch.int32, device=DEV)

    def run(n_averaged, weight, found_inf=0, with_scaler=True):
        avg.copy_(avg0)
        state.fill_(n_averaged)
        scaler[2] = found_inf
        _lib.check(lib.zsv_avg_multi(table.data_ptr(), count, chunks, state.data_ptr(), weight,
                                     scaler.data_ptr() if with_scaler else None, stream), "zsv_avg_multi")
        assert torch.equal(src, src0)                                        # the source is only read
        assert torch.equal(avg[avg_mask], avg0[avg_mask])                    # nothing outside [avg, avg + n)
        assert int(state) == n_averaged                                      # the launch does not advance the count
        return [(avg[sb:sb + n].double(), avg0[sb:sb + n].double(), src0[sa:sa + n].double())
                for (sa, n), (sb, _) in zip(src_spans, avg_spans)]

    for got, old, new in run(0, 0.1):                                        # first averaged step: an exact copy
        assert torch.equal(got, new)
    w32 = float(torch.tensor(0.1, dtype=torch.float32))
    cases = [(3, 0.1, lambda a, p: a + w32 * (p - a)),                      # EMA, first branch
             (3, 0.75, lambda a, p: p - (p - a) * 0.25),                     # EMA, second branch
             (1, -1.0, lambda a, p: p - (p - a) * 0.5),                      # equal-weight, w = 1/2
             (2, -1.0, lambda a, p: a + float(torch.tensor(1.0, dtype=torch.float32) / 3) * (p - a))]
    for n_averaged, weight, rule in cases:
        for with_scaler in (True, False):
            for got, old, new in run(n_averaged, weight, with_scaler=with_scaler):
                bound = 3 * EPS * max(old.abs().max().item(), new.abs().max().item())
                assert (got - rule(old, new)).abs().max().item() <= bound, (n_averaged, weight)
    run(3, 0.1, found_inf=1)                                                 # a skipped step: nothing is written
    assert torch.equal(avg, avg0)
    assert lib.zsv_avg_multi(table.data_ptr(), count, chunks, None, 0.1, None, stream) != 0
    assert lib.zsv_avg_multi(table.data_ptr(), count, chunks, state.data_ptr(), 1.5, None, stream) != 0

    # the count: += !found_inf, or += 1 without a scaler
    state.fill_(5)
    scaler[2] = 1
    _lib.check(lib.zsv_avg_advance(state.data_ptr(), scaler.data_ptr(), stream), "zsv_avg_advance")
    assert int(state) == 5 and int(scaler[2]) == 1
    scaler[2] = 0
    _lib.check(lib.zsv_avg_advance(state.data_ptr(), scaler.data_ptr(), stream), "zsv_avg_advance")
    _lib.check(lib.zsv_avg_advance(state.data_ptr(), None, stream), "zsv_avg_advance")
    assert int(state) == 7

    # the swap is exact, both ways, and stays inside the slices
    avg.copy_(avg0)
    _lib.check(lib.zsv_swap_multi(table.data_ptr(), count, chunks, stream), "zsv_swap_multi")
    assert torch.equal(src[src_mask], src0[src_mask]) and torch.equal(avg[avg_mask], avg0[avg_mask])
    for (sa, n), (sb, _) in zip(src_spans, avg_spans):
        assert torch.equal(src[sa:sa + n], avg0[sb:sb + n]) and torch.equal(avg[sb:sb + n], src0[sa:sa + n]), (sa, sb, n)
    _lib.check(lib.zsv_swap_multi(table.data_ptr(), count, chunks, stream), "zsv_swap_multi")
    assert torch.equal(src, src0) and torch.equal(avg, avg0)


def test_two_runs_are_bit_identical():
    """9: the same inputs give the same bits: no atomics anywhere on the way."""
    runs = [_device_run("adamw_clip", 0.9, poison=POISON, use_scaler=True) for _ in range(2)]
    (ps1, _, avg1, _), (ps2, _, avg2, _) = runs
    for a, b in zip(avg1.shadows().values(), avg2.shadows().values()):
        assert torch.equal(a, b)
    for a, b in zip(ps1, ps2):
        assert torch.equal(a.detach(), b.detach())
    assert int(avg1.n_averaged) == int(avg2.n_averaged) == 12 - len(POISON)
