"""What an SGD-with-momentum step costs on the live parameter set of R(2+1)D-18, alternated in one process on one device.
    python tools/sgd_bench.py [--rounds 7] [--steps 50] [--out profiles/sgd_step.json] [--scalar-lib libzsv_sgd_scalar.so]

The table is the live parameter set of R(2+1)D-18 inside network.Model (the parameters one training step gives gradients to:
115 tensors, 31.7 M fp32 values); the gradients are synthetic and stay in place, so only the optimizer runs.  Variants are
alternated per round (order reversed every other round) after a synchronised warm-up.

* "raw": `zsv_sgd_multi` (momentum 0.9, weight decay 1e-4, not the first step) launched back to back on one prebuilt descriptor
  table -- the device time of the kernel; the same launch a second time in the same rounds (the run-to-run spread); the launch
  with scaler state, clip record and shadows; `zsv_adam_multi` on the same table.  With `--scalar-lib` (sgd.hip built with
  -DZSV_SGD_SCALAR into a library of its own: `hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -DZSV_SGD_SCALAR
  -Iinclude -Izeroshotvideoclassification_amd/csrc zeroshotvideoclassification_amd/csrc/sgd.hip -o libzsv_sgd_scalar.so`) the 4-bytes-per-lane form of the same kernel runs in the same rounds: the A/B of
  the 16-byte accesses.  Any other build of `zsv_sgd_multi` -- another commit's library -- is compared the same way: the second
  library runs the plain launch twice (its own spread) and the launch with every option.
* "step": a training loop's calls, host work included: (1) FusedSGD(momentum=0.9, weight_decay=1e-4), (2) the same under
  LossScaler with max_grad_norm and a WeightAverage, and FusedSGD(grad_buckets=) on the local buckets of ddp.GradientSync (the table
  built once; the gradients of every "step" variant are the bucket views, which start at element offsets), (3)
  torch.optim.SGD(foreach=True) and, if this torch accepts it, fused=True, (4) FusedAdam.  Per variant: `device_us` from device events around the loop, `wall_us` from the host clock around
  the loop and the synchronisation that ends it, and `enqueue_us`, the host clock around the loop alone -- a variant whose
  enqueue time reaches its wall time is bound by the host, one whose wall time is its raw kernel time by HBM.

Bytes: an SGD-momentum step must read p, g, buf and write p, buf: 5 x 4 B per value; GB/s figures are against that."""
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
ap.add_argument("--scalar-lib", default="",
                help="a second library exporting zsv_sgd_multi, run in the same rounds: built with -DZSV_SGD_SCALAR, or another commit's (the A/B)")
ap.add_argument("--out", default="")
ap.add_argument("--ab-out", default="", help="where the vector / scalar A/B goes (with --scalar-lib)")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("sgd_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()
scalar = None
if args.scalar_lib:
    scalar = ctypes.CDLL(os.path.abspath(args.scalar_lib))
    scalar.zsv_sgd_multi.restype, scalar.zsv_sgd_multi.argtypes = _lib.SIGNATURES["zsv_sgd_multi"]

# the live parameter set: one small training step tells which parameters receive gradients
model = network.get_network(SimpleNamespace(network=args.network, fixconvs=False, nopretrained=False))
model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
model.to(dev).train()
x = synthetic.synthetic_clips(2, 8, 56).to(dev)
_, z = synthetic.synthetic_targets(2)
HP = dict(lr=1e-6, momentum=0.9, weight_decay=1e-4)
sync = ddp.GradientSync(model, local=True)
bucketed = optim.FusedSGD(model.parameters(), grad_buckets=sync, **HP)
for _ in range(2):                                       # the first step discovers the buckets, the second builds the static table
    train.train_step(model, bucketed, torch.nn.MSELoss(), x, z.to(dev), sync)
torch.cuda.synchronize()
if bucketed._static is None:
    raise SystemExit("sgd_bench: the bucket path did not engage")
live = [p for p in model.parameters() if p.grad is not None]
gen = torch.Generator(device=dev).manual_seed(0)
with torch.no_grad():
    for p in live:                                       # in place: the gradients stay the views of the flat buckets
        p.grad.copy_(torch.randn(p.shape, generator=gen, device=dev) * 1e-3)
values = sum(p.numel() for p in live)
sgd_bytes = 5 * 4 * values


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- raw launches on one prebuilt table ---------------------------------------------------------------------------------
m_raw = [torch.zeros_like(p) for p in live]
v_raw = [torch.zeros_like(p) for p in live]
p_raw = [p.detach().clone() for p in live]
g_raw = [p.grad.detach().clone() for p in live]           # allocations of their own: every tensor of the raw table is 16-byte aligned
s_flat = torch.cat([p.detach().reshape(-1) for p in live])
rows, shadow_ptrs, first, off = [], [], 0, 0
for p, mm, vv, q, gg in zip(live, m_raw, v_raw, p_raw, g_raw):
    rows.append(struct.pack("<QQQQqq", q.data_ptr(), gg.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.numel(), first))
    shadow_ptrs.append(s_flat.data_ptr() + 4 * off)
    first += (p.numel() + 4095) // 4096
    off += p.numel()
table = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).to(dev)
shadows = torch.tensor(shadow_ptrs, dtype=torch.int64, device=dev)
count, chunks = len(rows), first
record = torch.ones(2, dtype=torch.float32, device=dev)
state = torch.zeros(4, dtype=torch.int32)
state.view(torch.float32)[0] = 1.0
state = state.to(dev)
avg_state = torch.ones(1, dtype=torch.int32, device=dev)
T, R, S, SH, AS = table.data_ptr(), record.data_ptr(), state.data_ptr(), shadows.data_ptr(), avg_state.data_ptr()
aligned = sum(p.numel() for p, q, gg in zip(live, p_raw, g_raw) if (q.data_ptr() | gg.data_ptr()) % 16 == 0)
aligned_in_buckets = sum(p.numel() for p in live if p.grad.data_ptr() % 16 == 0)


def sgd_of(which):
    def run():
        _lib.check(which.zsv_sgd_multi(T, count, chunks, 1e-6, 0.9, 0.0, 0, 1e-4, 0, None, None, 0, -1, None, None, 0.0, stream()),
                   "zsv_sgd_multi")
    return run


def sgd_all_options_of(which):
    def run():
        _lib.check(which.zsv_sgd_multi(T, count, chunks, 1e-6, 0.9, 0.0, 0, 1e-4, 0, R, S, 0, -1, SH, AS, 1e-3, stream()), "zsv_sgd_multi")
    return run


def adam_multi():
    _lib.check(lib.zsv_adam_multi(T, count, chunks, 1e-6, 0.9, 0.999, 1e-8, 100, stream()), "zsv_adam_multi")


raw = {"sgd_multi": sgd_of(lib), "sgd_multi_again": sgd_of(lib), "sgd_multi_scaler_clip_avg": sgd_all_options_of(lib),
       "adam_multi": adam_multi}
if scalar is not None:
    raw.update({"sgd_multi_scalar_build": sgd_of(scalar), "sgd_multi_scalar_build_again": sgd_of(scalar),
                "sgd_multi_scaler_clip_avg_scalar_build": sgd_all_options_of(scalar)})

# ---- the optimizers as a loop calls them ------------------------------------------------------------------------------------
full = optim.FusedSGD(live, max_grad_norm=1.0, **HP)
optim.WeightAverage(full, decay=0.999)
full_scaler = optim.LossScaler(init_scale=1.0)


def full_step():
    full_scaler.step(full)
    full_scaler.update()


steps = {"fused_sgd": optim.FusedSGD(live, **HP).step, "fused_sgd_again": optim.FusedSGD(live, **HP).step,
         "fused_sgd_buckets": bucketed.step, "fused_sgd_scaler_clip_avg": full_step, "torch_sgd_foreach": torch.optim.SGD(live, foreach=True, **HP).step}
torch_fused_error = None
try:
    candidate = torch.optim.SGD(live, fused=True, **HP)
    candidate.step()
    torch.cuda.synchronize()
    steps["torch_sgd_fused"] = candidate.step
except Exception as e:                                   # this torch build does not take fused=True on HIP: recorded, not timed
    torch_fused_error = f"{type(e).__name__}: {e}"[:300]
steps["fused_adam"] = optim.FusedAdam(live, lr=1e-6).step


def measure(variants):
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
        out[name] = {"device_us_median": statistics.median(d), "device_us_min": min(d), "device_us_max": max(d),
                     "wall_us_median": statistics.median(t["wall_us"]), "enqueue_us_median": statistics.median(t["enqueue_us"]),
                     "GBps_of_sgd_bytes": sgd_bytes / statistics.median(d) / 1e3, "rounds": t}
        print(f"{name:28s} device {statistics.median(d):8.1f} us (min {min(d):.1f}, max {max(d):.1f})  wall "
              f"{statistics.median(t['wall_us']):8.1f} us  enqueue {statistics.median(t['enqueue_us']):8.1f} us  "
              f"{out[name]['GBps_of_sgd_bytes']:7.0f} GB/s of the SGD bytes", flush=True)
    return out


result = {"network": args.network, "device": torch.cuda.get_device_name(dev), "tensors": count, "values": values, "chunks": chunks,
          "values_in_16_byte_aligned_tensors": aligned, "values_in_16_byte_aligned_bucket_slices": aligned_in_buckets,
          "sgd_step_bytes": sgd_bytes, "steps_per_round": args.steps,
          "rounds": args.rounds, "torch": torch.__version__, "torch_sgd_fused_error": torch_fused_error}
print(f"{count} tensors, {values} values ({aligned} in 16-byte aligned tensors of the raw table, {aligned_in_buckets} in 16-byte aligned "
      f"bucket slices), {chunks} chunks; an SGD-momentum step moves "
      f"{sgd_bytes / 1e6:.0f} MB")
print("-- raw launches on a prebuilt table")
result["raw"] = measure(raw)
print("-- optimizer.step()")
result["step"] = measure(steps)
if bucketed._static is None or bucketed._static[0] != sync.layout_version:
    raise SystemExit("sgd_bench: the bucket path fell back to the per-step table")
if not all(torch.isfinite(p).all().item() for p in live + p_raw):
    raise SystemExit("sgd_bench: non-finite parameters")
kernel, again, step = result["raw"]["sgd_multi"], result["raw"]["sgd_multi_again"], result["step"]["fused_sgd"]
result["summary"] = {
    "sgd_multi_kernel_us": kernel["device_us_median"],
    "sgd_multi_kernel_GBps": kernel["GBps_of_sgd_bytes"],
    "sgd_multi_spread_us": [min(kernel["device_us_min"], again["device_us_min"]), max(kernel["device_us_max"], again["device_us_max"])],
    "fused_sgd_step_wall_us": step["wall_us_median"],
    "fused_sgd_step_enqueue_us": step["enqueue_us_median"],
    "fused_sgd_bound": "host" if step["enqueue_us_median"] > 0.9 * step["wall_us_median"] else "HBM",
    "fused_sgd_buckets_step_wall_us": result["step"]["fused_sgd_buckets"]["wall_us_median"],
    "fused_sgd_buckets_step_enqueue_us": result["step"]["fused_sgd_buckets"]["enqueue_us_median"],
    "torch_foreach_over_fused_sgd_wall": result["step"]["torch_sgd_foreach"]["wall_us_median"] / step["wall_us_median"],
    "adam_multi_over_sgd_multi_kernel": result["raw"]["adam_multi"]["device_us_median"] / kernel["device_us_median"],
}
if scalar is not None:
    result["summary"]["scalar_build_over_vector_kernel"] = result["raw"]["sgd_multi_scalar_build"]["device_us_median"] / kernel["device_us_median"]
print(json.dumps(result["summary"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
if args.ab_out and scalar is not None:
    ab = {k: result[k] for k in ("network", "device", "tensors", "values", "values_in_16_byte_aligned_tensors", "sgd_step_bytes",
                                 "steps_per_round", "rounds")}
    ab["raw"] = {k: v for k, v in result["raw"].items() if k != "adam_multi"}
    ab["scalar_build_over_vector_kernel"] = result["summary"]["scalar_build_over_vector_kernel"]
    with open(args.ab_out, "w") as f:
        json.dump(ab, f, indent=1)
