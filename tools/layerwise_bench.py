"""What the layer-wise trust ratio costs on the live parameter set of R(2+1)D-18: FusedLARS against FusedSGD and FusedLAMB against
FusedAdam(weight_decay=, decoupled_weight_decay=True), alternated in one process on one device.
    python tools/layerwise_bench.py [--rounds 7] [--steps 50] [--out profiles/layerwise_step.json] [--scalar-lib other/libzsv_hip.so]

The table is the live parameter set of R(2+1)D-18 inside network.Model (115 tensors, 31.7 M fp32 values); the gradients are
synthetic and stay in place, so only the optimizer runs.  Variants are alternated per round (order reversed every other round)
after a synchronised warm-up, as in tools/sgd_bench.py.

* "raw": the launches of one step back to back on one prebuilt descriptor table (every tensor 16-byte aligned), timed by device
  events -- the kernel time.  `lars` = zsv_lars_norms + zsv_layerwise_finalize + zsv_lars_multi against `sgd` = zsv_sgd_multi;
  `lamb` = zsv_lamb_moments + zsv_layerwise_finalize + zsv_lamb_multi against `adamw` = zsv_adamw_multi; each baseline a second
  time in the same rounds (the run-to-run spread).  With `--scalar-lib` (as in tools/sgd_bench.py: a second build of the library,
  with -DZSV_SGD_SCALAR or another commit's) `sgd` and `lars` of that library run in the same rounds, `sgd` twice: the A/B.
* "parts": the five launches of the two three-launch steps, each back to back on its own: where their time goes.
* "step": `optimizer.step()` as a training loop calls it, host work included, with per-step tables and over the flat buckets of
  ddp.GradientSync(local=True) (`*_buckets`: the table built once, the gradients bucket views at element offsets).  `device_us`
  from device events around the loop, `wall_us` from the host clock around the loop and the synchronisation that ends it,
  `enqueue_us` the host clock around the loop alone.

Expected kernel-time ratios from bytes per value: LARS reads p and g for the norms (8 B) and then moves SGD's 20 B: 28 / 20 = 1.4;
LAMB moves 24 B (read g, m, v, p, write m, v) and 16 B (read m, v, p, write p) against AdamW's 28 B: 40 / 28 = 1.43; the finalize
launch comes on top of both.  The summary records the measured ratios next to these."""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import time
from ctypes import c_void_p
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from zeroshotvideoclassification_amd import _lib, ddp, network, optim, synthetic, train

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--network", default="r2plus1d_18")
ap.add_argument("--scalar-lib", default="", help="a second build of libzsv_hip.so whose sgd and lars launches run in the same rounds (the A/B)")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("layerwise_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()
other = None
if args.scalar_lib:
    other = ctypes.CDLL(os.path.abspath(args.scalar_lib))
    for sym in ("zsv_sgd_multi", "zsv_lars_norms", "zsv_layerwise_finalize", "zsv_lars_multi"):
        getattr(other, sym).restype, getattr(other, sym).argtypes = _lib.SIGNATURES[sym]

# the live parameter set: one small training step tells which parameters receive gradients
model = network.get_network(SimpleNamespace(network=args.network, fixconvs=False, nopretrained=False))
model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
model.to(dev).train()
x = synthetic.synthetic_clips(2, 8, 56).to(dev)
_, z = synthetic.synthetic_targets(2)
SGD_HP = dict(lr=1e-6, momentum=0.9, weight_decay=1e-4)
ADAM_HP = dict(lr=1e-6, weight_decay=0.01)
sync = ddp.GradientSync(model, local=True)
sgd_buckets = optim.FusedSGD(model.parameters(), grad_buckets=sync, **SGD_HP)
for _ in range(2):                                       # the first step discovers the buckets, the second builds the static table
    train.train_step(model, sgd_buckets, torch.nn.MSELoss(), x, z.to(dev), sync)
torch.cuda.synchronize()
live = [p for p in model.parameters() if p.grad is not None]
gen = torch.Generator(device=dev).manual_seed(0)
with torch.no_grad():
    for p in live:                                       # in place: the gradients stay the views of the flat buckets
        p.grad.copy_(torch.randn(p.shape, generator=gen, device=dev) * 1e-3)
values = sum(p.numel() for p in live)
BYTES = {"sgd": 20, "lars": 28, "adamw": 28, "lamb": 40}  # per value


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- raw launches on one prebuilt table ---------------------------------------------------------------------------------
m_raw = [torch.zeros_like(p) for p in live]
v_raw = [torch.zeros_like(p) for p in live]
p_raw = [p.detach().clone() for p in live]
g_raw = [p.grad.detach().clone() for p in live]           # allocations of their own: every tensor of the raw table is 16-byte aligned
rows, first = [], 0
for p, mm, vv, q, gg in zip(live, m_raw, v_raw, p_raw, g_raw):
    rows.append(struct.pack("<QQQQqq", q.data_ptr(), gg.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.numel(), first))
    first += (p.numel() + 4095) // 4096
table = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev)
count, chunks = len(rows), first
ws_bytes = int(lib.zsv_layerwise_workspace_bytes(chunks, count))
ws = torch.zeros(ws_bytes // 4, dtype=torch.float32, device=dev)
T, W = table.data_ptr(), ws.data_ptr()
PLACE = (T, count, chunks, 0, 0, count, W, ws_bytes)


def raw_sgd_of(which):
    def run():
        _lib.check(which.zsv_sgd_multi(T, count, chunks, 1e-6, 0.9, 0.0, 0, 1e-4, 0, None, None, 0, -1, None, None, 0.0, stream()),
                   "zsv_sgd_multi")
    return run


def raw_lars_of(which):
    def run():
        _lib.check(which.zsv_lars_norms(*PLACE, None, stream()), "zsv_lars_norms")
        _lib.check(which.zsv_layerwise_finalize(*PLACE, 0, 1, 1e-3, 1e-4, 1e-8, 0.0, None, None, 0, stream()), "zsv_layerwise_finalize")
        _lib.check(which.zsv_lars_multi(T, count, chunks, W, 1e-6, 0.9, 0.0, 0, 1e-4, 0, None, None, 0, -1, None, None, 0.0, stream()),
                   "zsv_lars_multi")
    return run


raw_sgd, raw_lars = raw_sgd_of(lib), raw_lars_of(lib)


def raw_adamw():
    _lib.check(lib.zsv_adamw_multi(T, count, chunks, 1e-6, 0.9, 0.999, 1e-8, 0.01, 1, None, 100, stream()), "zsv_adamw_multi")


def raw_lamb():
    _lib.check(lib.zsv_lamb_moments(*PLACE, 0.9, 0.999, 1e-6, 0.01, None, None, 0, 100, stream()), "zsv_lamb_moments")
    _lib.check(lib.zsv_layerwise_finalize(*PLACE, 1, 1, 0.0, 0.0, 0.0, 0.0, None, None, 0, stream()), "zsv_layerwise_finalize")
    _lib.check(lib.zsv_lamb_multi(T, count, chunks, W, 1e-6, 0.9, 0.999, 1e-6, 0.01, None, 100, None, None, 0.0, stream()), "zsv_lamb_multi")


raw = {"sgd": raw_sgd, "lars": raw_lars, "sgd_again": raw_sgd, "adamw": raw_adamw, "lamb": raw_lamb, "adamw_again": raw_adamw}
if other is not None:
    raw.update({"sgd_other_build": raw_sgd_of(other), "lars_other_build": raw_lars_of(other), "sgd_other_build_again": raw_sgd_of(other),
                "lars_other_build_again": raw_lars_of(other)})

# the same launches one at a time: where the three-launch steps spend their time (bytes per value: what that launch moves)
parts = {
    "lars_norms": lambda: _lib.check(lib.zsv_lars_norms(*PLACE, None, stream()), "zsv_lars_norms"),
    "lars_finalize": lambda: _lib.check(lib.zsv_layerwise_finalize(*PLACE, 0, 1, 1e-3, 1e-4, 1e-8, 0.0, None, None, 0, stream()),
                                        "zsv_layerwise_finalize"),
    "lars_multi": lambda: _lib.check(lib.zsv_lars_multi(T, count, chunks, W, 1e-6, 0.9, 0.0, 0, 1e-4, 0, None, None, 0, -1, None, None,
                                                        0.0, stream()), "zsv_lars_multi"),
    "lamb_moments": lambda: _lib.check(lib.zsv_lamb_moments(*PLACE, 0.9, 0.999, 1e-6, 0.01, None, None, 0, 100, stream()),
                                       "zsv_lamb_moments"),
    "lamb_multi": lambda: _lib.check(lib.zsv_lamb_multi(T, count, chunks, W, 1e-6, 0.9, 0.999, 1e-6, 0.01, None, 100, None, None, 0.0,
                                                        stream()), "zsv_lamb_multi"),
}
PART_BYTES = {"lars_norms": 8, "lars_finalize": 0, "lars_multi": 20, "lamb_moments": 24, "lamb_multi": 16}

# ---- the optimizers as a loop calls them ------------------------------------------------------------------------------------
LARS_HP = dict(SGD_HP, trust_coefficient=1e-3)
steps = {
    "sgd": optim.FusedSGD(live, **SGD_HP), "lars": optim.FusedLARS(live, **LARS_HP), "sgd_again": optim.FusedSGD(live, **SGD_HP),
    "adamw": optim.FusedAdam(live, decoupled_weight_decay=True, **ADAM_HP), "lamb": optim.FusedLAMB(live, **ADAM_HP),
    "adamw_again": optim.FusedAdam(live, decoupled_weight_decay=True, **ADAM_HP),
    "sgd_buckets": sgd_buckets, "lars_buckets": optim.FusedLARS(model.parameters(), grad_buckets=sync, **LARS_HP),
    "adamw_buckets": optim.FusedAdam(model.parameters(), decoupled_weight_decay=True, grad_buckets=sync, **ADAM_HP),
    "lamb_buckets": optim.FusedLAMB(model.parameters(), grad_buckets=sync, **ADAM_HP),
}
bucketed = {k: o for k, o in steps.items() if k.endswith("_buckets")}


def measure(variants, bytes_of):
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: {"device_us": [], "wall_us": [], "enqueue_us": []} for name in variants}
    for r in range(args.rounds):
        order = list(variants) if r % 2 == 0 else list(reversed(list(variants)))
        for name in order:
            fn = variants[name]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            times[name]["device_us"].append(1e3 * e0.elapsed_time(e1) / args.steps)
            times[name]["wall_us"].append(1e6 * (t2 - t0) / args.steps)
            times[name]["enqueue_us"].append(1e6 * (t1 - t0) / args.steps)
    out = {}
    for name, t in times.items():
        d = t["device_us"]
        gbps = bytes_of(name) * values / statistics.median(d) / 1e3
        out[name] = {"device_us_median": statistics.median(d), "device_us_min": min(d), "device_us_max": max(d),
                     "wall_us_median": statistics.median(t["wall_us"]), "enqueue_us_median": statistics.median(t["enqueue_us"]),
                     "GBps_of_its_bytes": gbps, "rounds": t}
        print(f"{name:16s} device {statistics.median(d):8.1f} us (min {min(d):.1f}, max {max(d):.1f})  wall "
              f"{statistics.median(t['wall_us']):8.1f} us  enqueue {statistics.median(t['enqueue_us']):8.1f} us  {gbps:7.0f} GB/s of its bytes",
              flush=True)
    return out


def bytes_of(name):
    return BYTES[name.split("_")[0]]


result = {"network": args.network, "device": torch.cuda.get_device_name(dev), "tensors": count, "values": values, "chunks": chunks,
          "bytes_per_value": BYTES, "steps_per_round": args.steps, "rounds": args.rounds, "torch": torch.__version__}
print(f"{count} tensors, {values} values, {chunks} chunks")
print("-- raw launches on a prebuilt table")
result["raw"] = measure(raw, bytes_of)
print("-- the launches of the three-launch steps, each on its own")
result["parts"] = measure(parts, lambda name: PART_BYTES[name])
print("-- optimizer.step()")
result["step"] = measure({k: o.step for k, o in steps.items()}, bytes_of)
for name, o in bucketed.items():
    if o._static is None or o._static[0] != sync.layout_version:
        raise SystemExit(f"layerwise_bench: {name} fell back to the per-step table")
if not all(torch.isfinite(p).all().item() for p in live + p_raw):
    raise SystemExit("layerwise_bench: non-finite parameters")


def spread(a, b):
    """Run-to-run spread of a baseline measured twice in the same rounds, relative to its median."""
    lo, hi = min(a["device_us_min"], b["device_us_min"]), max(a["device_us_max"], b["device_us_max"])
    return (hi - lo) / a["device_us_median"]


R, S = result["raw"], result["step"]
result["summary"] = {
    "rows_us": {k: {"kernel": R[k]["device_us_median"], "step_wall": S[k]["wall_us_median"], "step_enqueue": S[k]["enqueue_us_median"],
                    "buckets_step_wall": S[k + "_buckets"]["wall_us_median"], "buckets_step_device": S[k + "_buckets"]["device_us_median"]}
                for k in ("sgd", "lars", "adamw", "lamb")},
    "lars_over_sgd_kernel": R["lars"]["device_us_median"] / R["sgd"]["device_us_median"],
    "lars_over_sgd_expected_from_bytes": BYTES["lars"] / BYTES["sgd"],
    "sgd_kernel_spread": spread(R["sgd"], R["sgd_again"]),
    "lamb_over_adamw_kernel": R["lamb"]["device_us_median"] / R["adamw"]["device_us_median"],
    "lamb_over_adamw_expected_from_bytes": BYTES["lamb"] / BYTES["adamw"],
    "adamw_kernel_spread": spread(R["adamw"], R["adamw_again"]),
    "parts_us": {k: v["device_us_median"] for k, v in result["parts"].items()},
    "lars_over_sgd_step_wall": S["lars"]["wall_us_median"] / S["sgd"]["wall_us_median"],
    "lamb_over_adamw_step_wall": S["lamb"]["wall_us_median"] / S["adamw"]["wall_us_median"],
    "lars_over_sgd_buckets_step_wall": S["lars_buckets"]["wall_us_median"] / S["sgd_buckets"]["wall_us_median"],
    "lamb_over_adamw_buckets_step_wall": S["lamb_buckets"]["wall_us_median"] / S["adamw_buckets"]["wall_us_median"],
}
print(json.dumps(result["summary"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
