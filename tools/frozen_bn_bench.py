"""Frozen-BatchNorm training step against the batch-statistics step, alternated in one process on one device.
    python tools/frozen_bn_bench.py [--rounds 5] [--steps 6] [--batch 22] [--out profiles/frozen_bn_step_ab.json]

Two models with the same weights: "batch" trains every BatchNorm with batch statistics (the default step); "frozen" has every
BatchNorm in eval mode inside a training-mode model (frozen-BatchNorm fine-tuning).  Each round times `--steps` steps of one
variant, then of the other (the order alternates per round), for fp32 and for amp.autocast().  Times are device events around
the timed window, after a synchronised warm-up.  Prints one line per (precision, variant) and writes the JSON record."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from zeroshotvideoclassification_amd import network, optim, synthetic, train

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=22)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--size", type=int, default=112)
ap.add_argument("--network", default="r2plus1d_18")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("frozen_bn_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
x = synthetic.synthetic_clips(args.batch, args.frames, args.size).to(dev)
_, z = synthetic.synthetic_targets(args.batch)
z = z.to(dev)
crit = torch.nn.MSELoss()


def make(frozen):
    model = network.get_network(SimpleNamespace(network=args.network, fixconvs=False, nopretrained=False))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
    model.to(dev).train()
    if frozen:
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.eval()
    return model, optim.FusedAdam(model.parameters(), lr=1e-4)


variants = {"batch": make(False), "frozen": make(True)}
pacer = train.StepPacer(2)


def run(name, amp, steps):
    model, opt = variants[name]
    loss = None
    for _ in range(steps):
        loss = train.train_step(model, opt, crit, x, z, pacer=pacer, autocast=amp)[1]
    return loss


result = {"network": args.network, "batch": args.batch, "frames": args.frames, "size": args.size, "steps_per_round": args.steps,
          "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "legs": {}}
for amp in (False, True):
    prec = "bf16" if amp else "fp32"
    for name in variants:
        run(name, amp, args.warmup)
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for r in range(args.rounds):
        order = list(variants) if r % 2 == 0 else list(reversed(list(variants)))
        for name in order:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = run(name, amp, args.steps)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
            if not torch.isfinite(loss).item():
                raise SystemExit(f"frozen_bn_bench: non-finite loss ({prec} {name})")
    for name in variants:
        t = times[name]
        result["legs"][f"{prec}_{name}"] = {"ms_per_step_median": statistics.median(t), "ms_per_step_min": min(t),
                                            "ms_per_step_max": max(t), "rounds_ms": t}
        print(f"{prec} {name:6s}: median {statistics.median(t):7.2f} ms/step  (min {min(t):.2f}, max {max(t):.2f}, "
              f"{args.rounds} rounds x {args.steps} steps)", flush=True)
for prec in ("fp32", "bf16"):
    a, b = result["legs"][f"{prec}_frozen"], result["legs"][f"{prec}_batch"]
    result[f"{prec}_frozen_over_batch"] = a["ms_per_step_median"] / b["ms_per_step_median"]
print(json.dumps({k: v for k, v in result.items() if k != "legs"}))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
