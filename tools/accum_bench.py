"""Cost of gradient accumulation: train_step(micro_batches=k) against k plain steps, and the accumulate kernel on its own.

    python tools/accum_bench.py [--micro-batches 4] [--batch 22] [--autocast] [--steps 10] [--warmup 4]
        one JSON line: ms per optimizer step of R(2+1)D-18 on k x 22 clips, FusedAdam on the local buckets of
        GradientSync(local=True), timed like the bench legs (train.StepPacer(2), HIP events around every step, queued warm-up).
        --micro-batches 1 is the plain step; --root DIR imports the package from another checkout (the baseline of an A/B).
    python tools/accum_bench.py --kernel [--reps 20]
        zsv_grad_accum_multi over the full bucket layout of the model (one table upload and one launch per bucket, as in a
        step; and the launches alone over resident tables) next to torch._foreach_add_ on the same tensors and one flat add
        per bucket: ms and GB/s per pass.
    python tools/accum_bench.py --ab BASELINE_DIR [--rounds 3] [--out FILE.json]
        alternates fresh child processes: the plain step of the checkout at BASELINE_DIR, the accumulated step of this one,
        fp32 and autocast; reports the accumulated step next to k x the plain step and the plain step's run-to-run spread.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--micro-batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=22, help="clips per micro-batch")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--network", default="r2plus1d_18")
    ap.add_argument("--autocast", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--root", default=HERE, help="checkout to import the package from")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ab", metavar="BASELINE_DIR")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out")
    return ap.parse_args()


def setup(args, clips):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from types import SimpleNamespace
    from zeroshotvideoclassification_amd import ddp, network, optim, synthetic, train
    dev = torch.device("cuda")
    model = network.get_network(SimpleNamespace(network=args.network, fixconvs=False, nopretrained=False))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0))
    model.to(dev).train()
    x = synthetic.synthetic_clips(clips, args.frames, args.size).to(dev)
    _, z = synthetic.synthetic_targets(clips)
    sync = ddp.GradientSync(model, local=True)
    opt = optim.FusedAdam(model.parameters(), lr=1e-3, grad_buckets=sync)
    return torch, train, model, sync, opt, x, z.to(dev)


def run_step(args):
    k = args.micro_batches
    torch, train, model, sync, opt, x, z = setup(args, k * args.batch)
    crit = torch.nn.MSELoss()
    pacer = train.StepPacer(2)
    extra = {"micro_batches": k} if k != 1 else {}          # (a baseline checkout may not know the argument)

    def step():
        return train.train_step(model, opt, crit, x, z, sync, pacer=pacer, autocast=args.autocast, **extra)[1]

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        loss = step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps
    dev_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    print(json.dumps({"mode": "step", "root": os.path.abspath(args.root), "micro_batches": k, "clips": k * args.batch,
                      "autocast": bool(args.autocast), "steps": args.steps, "ms_per_step": round(1e3 * wall, 3),
                      "device_ms_min_median_max": [round(dev_ms[0], 3), round(dev_ms[len(dev_ms) // 2], 3), round(dev_ms[-1], 3)],
                      "pacer_waits": pacer.waits, "loss": float(loss)}))


def run_kernel(args):
    torch, train, model, sync, opt, x, z = setup(args, 2)
    train.train_step(model, opt, torch.nn.MSELoss(), x, z, sync)     # fixes the bucket layout
    torch.cuda.synchronize()
    buckets = sync._buckets
    grads = [[torch.randn_like(p) for p in b.params] for b in buckets]
    numel = sum(b.numel for b in buckets)
    tensors = sum(len(b.params) for b in buckets)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
        marks[0].record()
        for i in range(args.reps):
            fn()
            marks[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.reps))
        return ms[len(ms) // 2]

    def hip(assign):
        def fn():
            for b, g in zip(buckets, grads):
                sync._accumulate(b, g, 1.0, assign)
        return fn

    from ctypes import c_void_p
    from zeroshotvideoclassification_amd import _lib, _tables
    lib = _lib.load()
    tables = []                                              # uploaded once: the launches alone, without the per-pass table upload
    for b, g in zip(buckets, grads):
        raw, chunks = _tables.pack_rows([(acc, g[i].data_ptr(), n) for i, acc, n in b.slices])
        tables.append((torch.frombuffer(raw, dtype=torch.uint8).to(x.device), len(b.slices), chunks))

    def hip_launch_only():
        stream = c_void_p(torch.cuda.current_stream().cuda_stream)
        for table, count, chunks in tables:
            _lib.check(lib.zsv_grad_accum_multi(table.data_ptr(), count, chunks, 1.0, 0, stream), "zsv_grad_accum_multi")

    def foreach():
        for b, g in zip(buckets, grads):
            torch._foreach_add_(b.views, g)

    def flat_add():                                          # the roofline stand-in: one contiguous add of the same size
        for b, f in zip(buckets, flats):
            b.flat.add_(f)

    flats = [torch.randn_like(b.flat) for b in buckets]
    out = {"mode": "kernel", "tensors": tensors, "buckets": len(buckets), "elements": numel, "mbytes": round(4e-6 * numel, 1)}
    for name, fn, streams in (("zsv_grad_accum_multi_add", hip(False), 3), ("zsv_grad_accum_multi_assign", hip(True), 2),
                              ("zsv_grad_accum_multi_add_tables_resident", hip_launch_only, 3),
                              ("torch_foreach_add", foreach, 3), ("torch_flat_add", flat_add, 3)):
        ms = timed(fn)
        out[name] = {"ms": round(ms, 4), "gb_per_s": round(streams * 4e-9 * numel / (1e-3 * ms), 1)}
    print(json.dumps(out))


def run_ab(args):
    k = args.micro_batches
    me = os.path.abspath(__file__)
    common = ["--batch", str(args.batch), "--steps", str(args.steps), "--warmup", str(args.warmup), "--network", args.network]
    result = {"micro_batches": k, "clips_per_micro_batch": args.batch, "rounds": args.rounds, "order": "plain, accumulated, plain, ..."}
    for tag, flag in (("fp32", []), ("autocast", ["--autocast"])):
        plain, accum = [], []
        for _ in range(args.rounds):
            for runs, cmd in ((plain, ["--micro-batches", "1", "--root", args.ab]), (accum, ["--micro-batches", str(k)])):
                p = subprocess.run([sys.executable, me] + cmd + common + flag, capture_output=True, text=True,
                                   timeout=args.child_timeout)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit(f"a child run failed with status {p.returncode}: nothing more is started")
                runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(p.stdout.strip().splitlines()[-1], flush=True)
        pm = [r["ms_per_step"] for r in plain]
        am = [r["ms_per_step"] for r in accum]
        mean = sum(pm) / len(pm)
        result[tag] = {"plain_ms_per_step_runs": pm, "accumulated_ms_per_step_runs": am,
                       "plain_ms_per_step_mean": round(mean, 3), "plain_spread_ms": round(max(pm) - min(pm), 3),
                       "k_times_plain_ms": round(k * mean, 3), "accumulated_ms_per_step_mean": round(sum(am) / len(am), 3),
                       "accumulated_minus_k_times_plain_ms": round(sum(am) / len(am) - k * mean, 3),
                       "plain_device_ms_median_runs": [r["device_ms_min_median_max"][1] for r in plain],
                       "accumulated_device_ms_median_runs": [r["device_ms_min_median_max"][1] for r in accum]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    a = parse()
    if a.ab:
        run_ab(a)
    elif a.kernel:
        run_kernel(a)
    else:
        run_step(a)
