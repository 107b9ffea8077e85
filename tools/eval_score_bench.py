"""What evaluate()'s scoring costs once the rows are on the device: the loop it ran before against one zsv_split_accuracy.
    python tools/eval_score_bench.py [--kernel-stats 132x101=STATS.csv] [--bench-parent A.json --bench-this B.json] --out profiles/eval_score.json

Two paths in one process, alternating, on the same device rows (synthetic.synthetic_eval_set), ten splits:

* loop       the scoring of evaluate() before train.score_splits existed, rebuilt from train.nearest_classes: one labels.cpu(),
             then per table a host np.isin, an upload of the mask, two boolean-index gathers, a class-table gather, two
             nearest_classes calls and two .item() reads
* one_pass   train.score_splits (zsv_split_accuracy: two distance launches + split_score_kernel) and its one device -> host copy

Both end in a device -> host read, so the host clock around a call is the time of the call; `--reps` timed calls each (at least
20) after `--warmup`, median / min / max / p10 / p90.  `spread` is p90 - p10 of a path's own calls.  The two paths must give the
same integers, or the tool stops.  `entry_us` is the device time of zsv_split_accuracy alone from HIP events around the call
(the table already uploaded).  The time of split_score_kernel by itself comes from a kernel trace taken in a run of its own
(`rocprofv3 --kernel-trace --stats -- python tools/eval_score_bench.py --only 132x101`), whose kernel statistics file is read
with --kernel-stats 132x101=FILE.  --bench-parent / --bench-this: files holding the JSON line of `python bench.py --full` on the parent commit and
on this one, same device; their extra.eval_t32_bf16 entries are copied into the result.

What must hold: one_pass is not slower than loop at any size, and at 132 x 101 faster by more than loop's own spread."""
import argparse
import csv
import json
import os
import statistics
import sys
import time
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zeroshotvideoclassification_amd import _lib, synthetic, train

SIZES = [(132, 101), (3783, 101), (6766, 51), (4926, 200)]      # the bench leg's row count; UCF101 / HMDB51 / ActivityNet test sets
SPLITS = 10

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", default="", help="ROWSxCLASSES: time this size alone (the run a kernel trace is taken of); no acceptance")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="ROWSxCLASSES=STATS.csv",
                help="kernel statistics CSV of a `rocprofv3 --kernel-trace --stats` run of this tool with --only ROWSxCLASSES")
ap.add_argument("--bench-parent", default="", help="file with the JSON line of `bench.py --full` on the parent commit")
ap.add_argument("--bench-this", default="", help="file with the JSON line of `bench.py --full` on this commit, same device")
ap.add_argument("--out", default="")
args = ap.parse_args()
if args.reps < 20:
    raise SystemExit("eval_score_bench: at least 20 timed calls")
if not torch.cuda.is_available():
    raise SystemExit("eval_score_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()


def loop_scoring(pred, true, label_dev, table):
    """evaluate()'s scoring before score_splits: (splits + 1, 3) integers through ~45 launches and ~70 host round trips."""
    def accuracy(p, e, t):
        order = train.nearest_classes(p, e, 5)
        y = train.nearest_classes(t, e, 1)[:, 0]
        return int((order[:, 0] == y).sum().item()), int((order == y[:, None]).any(dim=1).sum().item())
    label = label_dev.cpu().numpy()
    counts = np.zeros((SPLITS + 1, 3), dtype=np.int64)
    counts[0] = (len(pred),) + accuracy(pred, table, true)
    for split in range(SPLITS):
        np.random.seed(split)
        chosen = np.random.permutation(len(table))[:len(table) // 2]
        sel = torch.from_numpy(np.isin(label, chosen)).to(pred.device)
        n = int(sel.sum())
        if n == 0:
            continue
        counts[split + 1] = (n,) + accuracy(pred[sel], table[torch.from_numpy(chosen).to(pred.device)], true[sel])
    return counts


def one_pass_scoring(pred, true, label_dev, table):
    return train.score_splits(pred, true, label_dev, table, splits=SPLITS).cpu().numpy().astype(np.int64)


def summary(samples, unit_scale):
    s = sorted(unit_scale * v for v in samples)
    p10, p90 = s[int(0.1 * (len(s) - 1))], s[int(round(0.9 * (len(s) - 1)))]
    return {"median": round(statistics.median(s), 2), "min": round(s[0], 2), "max": round(s[-1], 2), "p10": round(p10, 2),
            "p90": round(p90, 2), "spread": round(p90 - p10, 2), "calls": len(s)}


result = {"device": torch.cuda.get_device_name(dev), "splits": SPLITS, "reps": args.reps, "warmup": args.warmup, "sizes": {}}
for rows, classes in SIZES:
    if args.only and args.only != f"{rows}x{classes}":
        continue
    table, labels, true, pred = (t.to(dev) for t in synthetic.synthetic_eval_set(rows, classes))
    labels = labels.long()
    paths = {"loop": loop_scoring, "one_pass": one_pass_scoring}
    outputs = {name: fn(pred, true, labels, table) for name, fn in paths.items()}
    if not np.array_equal(outputs["loop"], outputs["one_pass"]):
        raise SystemExit(f"eval_score_bench: the two paths disagree at {rows} x {classes}:\n{outputs['loop']}\n{outputs['one_pass']}")
    for _ in range(args.warmup):
        for fn in paths.values():
            fn(pred, true, labels, table)
    torch.cuda.synchronize()
    samples = {name: [] for name in paths}
    for _ in range(args.reps):                                   # alternating: both paths see the same machine
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn(pred, true, labels, table)
            samples[name].append(time.perf_counter() - t0)
    entry = {name + "_ms": summary(v, 1e3) for name, v in samples.items()}

    # the entry point alone, on the device: HIP events around one call
    pos = torch.from_numpy(train.split_tables(classes, SPLITS)).to(dev)
    counts = torch.empty((SPLITS + 1, 3), dtype=torch.int32, device=dev)
    nbytes = lib.zsv_split_accuracy_workspace_bytes(rows, classes)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    p, t, c = pred.contiguous(), true.contiguous(), table.contiguous()

    def launch():
        _lib.check(lib.zsv_split_accuracy(p.data_ptr(), t.data_ptr(), labels.data_ptr(), c.data_ptr(), rows, int(p.shape[1]), classes,
                                          pos.data_ptr(), SPLITS + 1, counts.data_ptr(), None, ws.data_ptr(), nbytes,
                                          c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_split_accuracy")
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    entry["entry_us"] = summary(us, 1.0)
    if not np.array_equal(counts.cpu().numpy(), outputs["loop"]):
        raise SystemExit(f"eval_score_bench: the raw call disagrees at {rows} x {classes}")
    entry["counts_full_table"] = [int(v) for v in outputs["loop"][0]]
    entry["one_pass_not_slower"] = entry["one_pass_ms"]["median"] <= entry["loop_ms"]["median"]
    entry["gain_ms"] = round(entry["loop_ms"]["median"] - entry["one_pass_ms"]["median"], 2)
    result["sizes"][f"{rows}x{classes}"] = entry
    print(f"{rows}x{classes}", json.dumps(entry), flush=True)

if args.only:
    raise SystemExit(0)
small = result["sizes"]["132x101"]
result["acceptance"] = {"one_pass_not_slower_at_every_size": all(e["one_pass_not_slower"] for e in result["sizes"].values()),
                        "gain_ms_at_132x101": small["gain_ms"], "loop_spread_ms_at_132x101": small["loop_ms"]["spread"],
                        "gain_exceeds_loop_spread_at_132x101": small["gain_ms"] > small["loop_ms"]["spread"]}
result["acceptance"]["met"] = bool(result["acceptance"]["one_pass_not_slower_at_every_size"]
                                   and result["acceptance"]["gain_exceeds_loop_spread_at_132x101"])
print(json.dumps(result["acceptance"]), flush=True)

if args.kernel_stats:
    result["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats around a run of this tool of its own per size (--only): warm-up "
                                        "and timed calls of both paths and of the raw entry point", "sizes": {}}
    for item in args.kernel_stats:
        size, path = item.split("=", 1)
        kernels = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                for key in ("split_score_kernel", "cosine_dist_kernel", "row_topk_kernel"):
                    if key in name:
                        kernels[key] = {k: row[k] for k in ("Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row}
        result["kernel_trace"]["sizes"][size] = kernels


def bench_leg(path):
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
    line = json.loads(lines[-1])
    return {"value": line.get("value"), "metric": line.get("metric"), "eval_t32_bf16": line.get("extra", {}).get("eval_t32_bf16")}


if args.bench_parent and args.bench_this:
    result["bench_full"] = {"source": "the JSON line of `python bench.py --full`, each a process of its own, one after the other on the "
                                      "same device", "parent": bench_leg(args.bench_parent), "this": bench_leg(args.bench_this)}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
if not result["acceptance"]["met"]:
    raise SystemExit("eval_score_bench: the acceptance does not hold (see the line above)")
