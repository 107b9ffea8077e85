"""What the softmax cross-entropy of a classifier step costs: the three zsv_softmax_xent_* launches against torch's
F.cross_entropy (forward + backward) + topk on the same device, alternated in one process.
    python tools/xent_bench.py [--rounds 7] [--steps 200] [--out profiles/softmax_xent.json]

Shapes (N, C): (22, 400) -- the benchmark's 22 clips on Kinetics-400 --, (176, 700) and (1408, 700): 8 and 64 times that batch
(the FusedLARS / FusedLAMB range) on Kinetics-700.  Logits are randn * 3, one label in 16 is -1 (ignored), label smoothing 0.1.

Per shape, alternated per round (order reversed every other round) after a synchronised warm-up:
* "zsv_launches": zsv_softmax_xent_fwd + _reduce + _bwd on prebuilt buffers -- the device time of the kernels;
* "zsv_launches_again": the same a second time in the same rounds (the run-to-run spread);
* "zsv_op": ops.softmax_cross_entropy(...) and loss.backward(), host work and autograd included;
* "torch": F.cross_entropy(ignore_index=-1, label_smoothing=0.1) and loss.backward(), then the top-1 / top-5 hit counts of the
  rows that are not ignored from logits.topk(5), all left on the device (no host filter, no synchronisation).
Per variant: `device_us` from device events around the loop, `wall_us` from the host clock around the loop and the
synchronisation that ends it, `enqueue_us` from the host clock around the loop alone."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from zeroshotvideoclassification_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("xent_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()
SHAPES = [(22, 400), (176, 700), (1408, 700)]
SMOOTHING = 0.1


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def variants_for(n, c):
    g = torch.Generator().manual_seed(n * 1000 + c)
    logits = (torch.randn(n, c, generator=g) * 3).to(dev)
    labels = torch.randint(0, c, (n,), generator=g)
    labels[::16] = -1
    labels = labels.to(dev)
    row_loss, row_rank = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    dlogits, dx = torch.empty(n, c, device=dev), torch.empty(n, c, device=dev)
    loss, counts = torch.empty((), device=dev), torch.empty(3, dtype=torch.int32, device=dev)
    one = torch.ones((), device=dev)
    leaf = logits.clone().requires_grad_()

    def launches():
        _lib.check(lib.zsv_softmax_xent_fwd(logits.data_ptr(), labels.data_ptr(), n, c, SMOOTHING, -1, row_loss.data_ptr(),
                                            row_rank.data_ptr(), dlogits.data_ptr(), stream()), "zsv_softmax_xent_fwd")
        _lib.check(lib.zsv_softmax_xent_reduce(row_loss.data_ptr(), row_rank.data_ptr(), n, 1, loss.data_ptr(), counts.data_ptr(),
                                               stream()), "zsv_softmax_xent_reduce")
        _lib.check(lib.zsv_softmax_xent_bwd(dlogits.data_ptr(), one.data_ptr(), counts.data_ptr(), 1, n, c, dx.data_ptr(), stream()),
                   "zsv_softmax_xent_bwd")

    def op():
        leaf.grad = None
        out, hits = ops.softmax_cross_entropy(leaf, labels, label_smoothing=SMOOTHING)
        out.backward()
        return out, hits

    def reference():
        leaf.grad = None
        out = F.cross_entropy(leaf, labels, ignore_index=-1, label_smoothing=SMOOTHING)
        out.backward()
        top = leaf.detach().topk(min(5, c), dim=1).indices
        valid = labels != -1
        hit = (top == labels[:, None]) & valid[:, None]
        return out, torch.stack([valid.sum(), hit[:, 0].sum(), hit.any(1).sum()])

    # the two sides compute the same thing (ties aside: randn logits have none at the label)
    a, b = op(), reference()
    torch.cuda.synchronize()
    if abs(a[0].item() - b[0].item()) > 1e-5 * abs(b[0].item()) or a[1].tolist() != b[1].tolist():
        raise SystemExit(f"xent_bench: ({n}, {c}): op {a[0].item()} {a[1].tolist()} vs torch {b[0].item()} {b[1].tolist()}")
    return {"zsv_launches": launches, "zsv_launches_again": launches, "zsv_op": op, "torch": reference}


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
                     "wall_us_median": statistics.median(t["wall_us"]), "enqueue_us_median": statistics.median(t["enqueue_us"]), "rounds": t}
        print(f"  {name:20s} device {statistics.median(d):8.1f} us (min {min(d):.1f}, max {max(d):.1f})  wall "
              f"{statistics.median(t['wall_us']):8.1f} us  enqueue {statistics.median(t['enqueue_us']):8.1f} us", flush=True)
    return out


result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "steps_per_round": args.steps, "rounds": args.rounds,
          "label_smoothing": SMOOTHING, "ignored_rows": "every 16th", "shapes": {}, "summary": {}}
for n, c in SHAPES:
    print(f"-- (N, C) = ({n}, {c})")
    got = measure(variants_for(n, c))
    key = f"{n}x{c}"
    result["shapes"][key] = got
    result["summary"][key] = {
        "zsv_launches_device_us": got["zsv_launches"]["device_us_median"],
        "zsv_launches_spread_us": [min(got["zsv_launches"]["device_us_min"], got["zsv_launches_again"]["device_us_min"]),
                                   max(got["zsv_launches"]["device_us_max"], got["zsv_launches_again"]["device_us_max"])],
        "zsv_op_wall_us": got["zsv_op"]["wall_us_median"], "zsv_op_enqueue_us": got["zsv_op"]["enqueue_us_median"],
        "torch_device_us": got["torch"]["device_us_median"], "torch_wall_us": got["torch"]["wall_us_median"],
        "torch_enqueue_us": got["torch"]["enqueue_us_median"],
        "torch_over_zsv_op_wall": got["torch"]["wall_us_median"] / got["zsv_op"]["wall_us_median"]}
print(json.dumps(result["summary"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
