"""What the synchronised BatchNorm's kernels cost next to the plain ones, WITHOUT the collectives, on one device in one process.
    python tools/sync_bn_bench.py [--rounds 7] [--steps 20] [--out profiles/sync_bn.json]

Per shape -- layer 1 of the 22-clip step, (22, 64, 16*56*56) and (22, 144, 16*56*56), and layer 4's (22, 512, 2*7*7) -- and per
case ("relu": BatchNorm + ReLU, mask mode 2; "res_relu": BatchNorm + residual + ReLU with the residual gradient, mask mode 1) a
forward + backward runs in two forms on the same tensors, alternated per round (order reversed every other round) after a
synchronised warm-up, timed with device events:

* "plain": zsv_bn_fwd_train + zsv_bn_bwd;
* "sync":  zsv_bn_sync_moments, zsv_bn_sync_finalize, zsv_bn_sync_apply; zsv_bn_sync_bwd_reduce, zsv_bn_sync_bwd_apply, with
  world = 1: `gathered` IS the moments buffer and `sums_global` IS the local sums, i.e. the two collectives are left out.

The five synchronised entry points are also timed one by one.  Bytes: tensor passes of N*C*S*4 bytes -- "relu": 3 forward
(x for the statistics, x, y) + 5 backward (dy, x | dy, x, dx) in both forms; "res_relu": 4 forward + 7 backward plain (the
reduction writes the masked gradient and the apply pass reads it alone) or 8 backward synchronised (the reduction has no tensor
output).  GB/s figures are against each form's own bytes.

NOT measured here: the all_gather of 2C+1 doubles and the all_reduce of 2C doubles per layer over RCCL at world > 1 (one device;
a gloo timing on one device would say nothing about them)."""
import argparse
import json
import os
import statistics
import sys
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from zeroshotvideoclassification_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("sync_bn_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()
SHAPES = [(22, 64, 16 * 56 * 56), (22, 144, 16 * 56 * 56), (22, 512, 2 * 7 * 7)]
PASSES = {"relu": {"plain": 8, "sync": 8}, "res_relu": {"plain": 11, "sync": 12}}
F32, F64 = torch.float32, torch.float64


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def forms(n, c, s, case):
    gen = torch.Generator(device=dev).manual_seed(c)
    x = torch.randn((n, c, s), generator=gen, device=dev) * 2 + 0.5
    dy = torch.randn((n, c, s), generator=gen, device=dev)
    res = torch.randn((n, c, s), generator=gen, device=dev) if case == "res_relu" else None
    y, dx = torch.empty_like(x), torch.empty_like(x)
    dres = torch.empty_like(x) if res is not None else None
    gamma, beta = torch.rand(c, generator=gen, device=dev) + 0.5, torch.randn(c, generator=gen, device=dev) * 0.1
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    mean, invstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
    dgamma, dbeta = torch.empty(c, device=dev), torch.empty(c, device=dev)
    nb = lib.zsv_bn_workspace_bytes(n, c, s)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    nbs = lib.zsv_bn_sync_workspace_bytes(n, c, s)
    wss = torch.empty(nbs, dtype=torch.uint8, device=dev)
    moments = torch.empty(2 * c + 1, dtype=F64, device=dev)
    sums = torch.empty(2 * c, dtype=F64, device=dev)
    count = torch.empty(1, dtype=F64, device=dev)
    mode = 1 if res is not None else 2
    P = lambda t: None if t is None else t.data_ptr()
    ym = y if mode == 1 else None

    def plain():
        _lib.check(lib.zsv_bn_fwd_train(P(x), n, c, s, P(gamma), P(beta), P(res), 1, P(y), P(mean), P(invstd), P(rm), P(rv), 0.1, 1e-5,
                                        P(ws), nb, stream()), "zsv_bn_fwd_train")
        _lib.check(lib.zsv_bn_bwd(P(dy), P(x), P(ym), n, c, s, P(gamma), P(beta), P(mean), P(invstd), mode, P(dx), P(dres), P(dgamma),
                                  P(dbeta), P(ws), nb, stream()), "zsv_bn_bwd")

    def s_moments():
        _lib.check(lib.zsv_bn_sync_moments(P(x), n, c, s, P(moments), P(wss), nbs, stream()), "zsv_bn_sync_moments")

    def s_finalize():
        _lib.check(lib.zsv_bn_sync_finalize(P(moments), 1, c, P(gamma), P(beta), P(rm), P(rv), 0.1, 1e-5, P(mean), P(invstd), P(count),
                                            stream()), "zsv_bn_sync_finalize")

    def s_apply():
        _lib.check(lib.zsv_bn_sync_apply(P(x), n, c, s, P(mean), P(invstd), P(gamma), P(beta), P(res), 1, P(y), stream()), "zsv_bn_sync_apply")

    def s_reduce():
        _lib.check(lib.zsv_bn_sync_bwd_reduce(P(dy), P(x), P(ym), n, c, s, P(mean), P(invstd), P(gamma), P(beta), mode, P(sums), P(wss), nbs,
                                              stream()), "zsv_bn_sync_bwd_reduce")

    def s_bwd_apply():
        _lib.check(lib.zsv_bn_sync_bwd_apply(P(dy), P(x), P(ym), n, c, s, P(mean), P(invstd), P(gamma), P(beta), mode, P(sums), P(sums),
                                             P(count), P(dx), P(dres), P(dgamma), P(dbeta), stream()), "zsv_bn_sync_bwd_apply")

    def sync():
        s_moments()
        s_finalize()
        s_apply()
        s_reduce()
        s_bwd_apply()

    # the two forms agree (same statistics up to the merge's rounding): a bench of a wrong kernel is worth nothing
    plain()
    ref = (y.clone(), dx.clone())
    sync()
    torch.cuda.synchronize()
    for a, b, what in ((y, ref[0], "y"), (dx, ref[1], "dx")):
        err = (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)
        if not err < 1e-5:
            raise SystemExit(f"sync_bn_bench: {what} of the two forms differs by {err:.2e} of its range")
    keep = (x, dy, res, y, dx, dres, gamma, beta, rm, rv, mean, invstd, dgamma, dbeta, ws, wss, moments, sums, count)
    return {"plain": plain, "sync": sync}, {"moments": s_moments, "finalize": s_finalize, "apply": s_apply, "bwd_reduce": s_reduce,
                                            "bwd_apply": s_bwd_apply}, keep


def measure(variants):
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
    return {name: {"device_us_median": statistics.median(t), "device_us_min": min(t), "device_us_max": max(t), "rounds": t}
            for name, t in times.items()}


result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "rounds": args.rounds, "steps_per_round": args.steps,
          "collectives": "not run: world = 1, gathered = the local moments, sums_global = the local sums; RCCL at world > 1 is not measured",
          "shapes": []}
for n, c, s in SHAPES:
    row = {"N": n, "C": c, "S": s, "tensor_bytes": n * c * s * 4, "cases": {}}
    for case in ("relu", "res_relu"):
        both, parts, keep = forms(n, c, s, case)
        out = measure(both)
        for form in ("plain", "sync"):
            out[form]["tensor_passes"] = PASSES[case][form]
            out[form]["GBps"] = PASSES[case][form] * row["tensor_bytes"] / out[form]["device_us_median"] / 1e3
        out["sync_over_plain"] = out["sync"]["device_us_median"] / out["plain"]["device_us_median"]
        out["sync_over_plain_spread"] = [out["sync"]["device_us_min"] / out["plain"]["device_us_max"],
                                         out["sync"]["device_us_max"] / out["plain"]["device_us_min"]]
        out["sync_entry_points"] = measure(parts)
        row["cases"][case] = out
        print(f"({n}, {c}, {s}) {case:8s} plain {out['plain']['device_us_median']:8.1f} us ({out['plain']['GBps']:5.0f} GB/s)  sync "
              f"{out['sync']['device_us_median']:8.1f} us ({out['sync']['GBps']:5.0f} GB/s)  ratio {out['sync_over_plain']:.3f} "
              f"[{out['sync_over_plain_spread'][0]:.3f}, {out['sync_over_plain_spread'][1]:.3f}]  "
              + "  ".join(f"{k} {v['device_us_median']:.1f}" for k, v in out["sync_entry_points"].items()), flush=True)
        del both, parts, keep
        torch.cuda.empty_cache()
    result["shapes"].append(row)
print(json.dumps({f"{r['C']}x{r['S']}": {k: round(v["sync_over_plain"], 4) for k, v in r["cases"].items()} for r in result["shapes"]}))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
