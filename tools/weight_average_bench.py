"""Cost of weight averaging (optim.WeightAverage) in the fused Adam step, alternated in one process on one device.
    python tools/weight_average_bench.py [--rounds 7] [--steps 50] [--out profiles/weight_average_step.json]

The table is the live parameter set of R(2+1)D-18 inside network.Model (the parameters one training step gives gradients to,
31.7 M values); the gradients are synthetic and stay in place, so only the optimizer runs.  Every figure is from device events
around `--steps` calls after a synchronised warm-up, host work for the per-step table included, the variants alternated per
round (order reversed every other round):

* a_default            `FusedAdam.step()` without a WeightAverage: the launches of the parent commit
* a_default_again      the same, measured a second time in the same rounds: the run-to-run spread
* b_average            `FusedAdam.step()` with `WeightAverage(decay=0.999)`: zsv_adam_multi_avg + the one-thread count
* c_foreach_lerp       a_default followed by `torch._foreach_lerp_(shadows, params, 1 - 0.999)`: what a loop does today
* d_*                  the same three under `LossScaler` with decoupled decay and clipping on (`step()` + `update()`);
                       d_c lerps unconditionally, i.e. without the flag read-back a correct loop would also need

Bytes per value: the update reads p, g, m, v and writes p, m, v (28 B); the fused average adds one read and one write of the
shadow (36 B); the separate lerp reads p and reads and writes the shadow (28 + 12 B).

`ZSV_LIB_PATH` selects another build of the library (e.g. one compiled with -DZSV_AVG_NONTEMPORAL: non-temporal instead of plain
loads and stores on the shadows); the path is recorded."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from zeroshotvideoclassification_amd import _lib, network, optim, synthetic, train

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--network", default="r2plus1d_18")
ap.add_argument("--decay", type=float, default=0.999)
ap.add_argument("--hbm-peak-TBps", type=float, default=8.0, help="MI355X HBM3E peak, for the achieved fraction")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("weight_average_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
_lib.load()

# the live parameter set: one small training step tells which parameters receive gradients
model = network.get_network(SimpleNamespace(network=args.network, fixconvs=False, nopretrained=False))
model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
model.to(dev).train()
x = synthetic.synthetic_clips(2, 8, 56).to(dev)
_, z = synthetic.synthetic_targets(2)
torch.nn.functional.mse_loss(train.embed(model, x), z.to(dev)).backward()
torch.cuda.synchronize()
live = [p for p in model.parameters() if p.grad is not None]
gen = torch.Generator(device=dev).manual_seed(0)
for p in live:
    p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
values = sum(p.numel() for p in live)
bytes_per_value = {"update": 28, "update_with_average": 36, "update_then_lerp": 28 + 12}

FINE = dict(weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0)


def plain(**kw):
    opt = optim.FusedAdam(live, lr=1e-4, **kw)
    return opt, None


def averaged(**kw):
    opt = optim.FusedAdam(live, lr=1e-4, **kw)
    return opt, optim.WeightAverage(opt, decay=args.decay)


def lerped(**kw):
    opt = optim.FusedAdam(live, lr=1e-4, **kw)
    return opt, [p.detach().clone() for p in live]


def stepper(opt, extra, scaled):
    scaler = optim.LossScaler(init_scale=1.0) if scaled else None
    shadows = extra if isinstance(extra, list) else None
    detached = [p.detach() for p in live]

    def run():
        if scaler is None:
            opt.step()
        else:
            scaler.step(opt)
            scaler.update()
        if shadows is not None:
            torch._foreach_lerp_(shadows, detached, 1.0 - args.decay)
    return run


variants = {
    "a_default": stepper(*plain(), False),
    "a_default_again": stepper(*plain(), False),
    "b_average": stepper(*averaged(), False),
    "c_foreach_lerp": stepper(*lerped(), False),
    "d_a_scaler_decay_clip": stepper(*plain(**FINE), True),
    "d_a_scaler_decay_clip_again": stepper(*plain(**FINE), True),
    "d_b_scaler_decay_clip_average": stepper(*averaged(**FINE), True),
    "d_c_scaler_decay_clip_foreach_lerp": stepper(*lerped(**FINE), True),
}


def measure():
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for r in range(args.rounds):
        order = list(variants) if r % 2 == 0 else list(reversed(list(variants)))
        for name in order:
            fn = variants[name]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / args.steps)
    out = {}
    for name, t in times.items():
        out[name] = {"us_median": statistics.median(t), "us_min": min(t), "us_max": max(t), "rounds_us": t}
        print(f"{name:36s} median {statistics.median(t):8.1f} us  (min {min(t):.1f}, max {max(t):.1f})", flush=True)
    return out


result = {"network": args.network, "device": torch.cuda.get_device_name(dev), "library": os.path.relpath(_lib.LIB_PATH, ROOT),
          "tensors": len(live), "values": values, "decay": args.decay, "steps_per_round": args.steps, "rounds": args.rounds,
          "bytes_per_value": bytes_per_value, "hbm_peak_TBps": args.hbm_peak_TBps}
print(f"{len(live)} tensors, {values} values; bytes per value {bytes_per_value}")
result["step"] = step = measure()
if not all(torch.isfinite(p).all().item() for p in live):
    raise SystemExit("weight_average_bench: non-finite parameters")


def tbps(name, per_value):
    return per_value * values / step[name]["us_median"] / 1e6


a, again, b, c = (step[k] for k in ("a_default", "a_default_again", "b_average", "c_foreach_lerp"))
da, dagain, db, dc = (step[k] for k in ("d_a_scaler_decay_clip", "d_a_scaler_decay_clip_again", "d_b_scaler_decay_clip_average",
                                        "d_c_scaler_decay_clip_foreach_lerp"))
result["summary"] = {
    "default_spread_us": [min(a["us_min"], again["us_min"]), max(a["us_max"], again["us_max"])],
    "default_medians_us": [a["us_median"], again["us_median"]],
    "average_over_default": b["us_median"] / a["us_median"],
    "foreach_lerp_over_default": c["us_median"] / a["us_median"],
    "average_cheaper_than_foreach_lerp": b["us_median"] < c["us_median"],
    "expected_by_bytes": {"average_over_default": 36 / 28, "foreach_lerp_over_default": 40 / 28},
    "default_TBps": tbps("a_default", 28),
    "average_TBps": tbps("b_average", 36),
    "average_fraction_of_hbm_peak": tbps("b_average", 36) / args.hbm_peak_TBps,
    "foreach_lerp_TBps": tbps("c_foreach_lerp", 40),
    "scaler_default_spread_us": [min(da["us_min"], dagain["us_min"]), max(da["us_max"], dagain["us_max"])],
    "scaler_average_over_default": db["us_median"] / da["us_median"],
    "scaler_foreach_lerp_over_default": dc["us_median"] / da["us_median"],
    "scaler_average_cheaper_than_foreach_lerp": db["us_median"] < dc["us_median"],
}
print(json.dumps(result["summary"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
