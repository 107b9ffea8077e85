"""A/B of the strided bf16 input gradients of R(2+1)D-18 at the benchmarked size (22 clips of 16 x 112 x 112): the per-class
composition (``Bf16TrainPath._dgrad_composed``: per class a strided weight copy, a pack, a convolution and a strided copy, plus
the fill of the shortcuts and the torch add of the fan-in) against the one-launch ``zsv_conv3d_bf16_dgrad`` (pack + convolution,
fan-in in the epilogue), alternating in one process on one device.

    python tools/dgrad_bf16_bench.py [--batch 22] [--repeats 7] [--iters 20] [--out profiles/bf16_dgrad_one_launch.json]

Per geometry and path: the median over ``repeats`` of the mean device time of ``iters`` back-to-back calls (device events), and the
spread (max - min over the repeats).  The two results are compared with ``torch.equal`` before anything is timed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from zeroshotvideoclassification_amd import amp

# name, Cin, Cout, (T, H, W) of the input, kernel, stride, padding: the strided convolutions of a 16 x 112 x 112 forward
GEOMS = [
    ("S2", 64, 230, (16, 56, 56), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("S5", 128, 460, (8, 28, 28), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("S8", 256, 921, (4, 14, 14), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ("T2", 230, 128, (16, 28, 28), (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    ("T5", 460, 256, (8, 14, 14), (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    ("T8", 921, 512, (4, 7, 7), (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    ("P1", 64, 128, (16, 56, 56), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    ("P2", 128, 256, (8, 28, 28), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
    ("P3", 256, 512, (4, 14, 14), (1, 1, 1), (2, 2, 2), (0, 0, 0)),
]


def problem(n, cin, cout, thw, k, s, p, seed):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    conv = torch.nn.Conv3d(cin, cout, k, stride=s, padding=p, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=g, device=dev) * (cin * k[0] * k[1] * k[2]) ** -0.5))
    u = amp._Unit(conv, torch.nn.BatchNorm3d(cout).to(dev), False)
    rec = amp._Record()
    rec.unit, rec.desc = u, u.desc(n, *thw)
    d = rec.desc
    dz = amp.ncdhw_to_cl_bf16(torch.randn((n, cout, d.To, d.Ho, d.Wo), generator=g, device=dev))
    fanin = amp.ncdhw_to_cl_bf16(torch.randn((n, cin) + tuple(thw), generator=g, device=dev))
    return rec, dz, fanin


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dgrad_bf16_bench: an MI355X is needed (there is no CPU fallback)")
    rows = []
    for i, (name, cin, cout, thw, k, s, p) in enumerate(GEOMS):
        rec, dz, fanin = problem(args.batch, cin, cout, thw, k, s, p, 100 + i)
        paths = {}
        for with_fanin in (False, True):
            f = fanin if with_fanin else None
            tag = "+fanin" if with_fanin else ""
            paths["composed" + tag] = (lambda f=f: amp.Bf16TrainPath._dgrad_composed(rec, dz) if f is None
                                       else amp.Bf16TrainPath._dgrad_composed(rec, dz) + f)
            paths["one_launch" + tag] = lambda f=f: amp.Bf16TrainPath._dgrad(rec, dz, fanin=f)
            assert torch.equal(paths["composed" + tag](), paths["one_launch" + tag]()), f"{name}{tag}: the two paths differ"
        for fn in paths.values():                                   # warm-up of every shape
            timed(fn, 3)
        samples = {k_: [] for k_ in paths}
        for _ in range(args.repeats):                               # alternate the paths inside every repeat
            for k_, fn in paths.items():
                samples[k_].append(timed(fn, args.iters))
        row = {"name": name, "cin": cin, "cout": cout, "thw": list(thw), "kernel": list(k), "stride": list(s), "clips": args.batch}
        for k_, v in samples.items():
            v = sorted(v)
            row[k_] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                       "spread_ms": round(v[-1] - v[0], 4)}
        rows.append(row)
        print(name, {k_: row[k_]["median_ms"] for k_ in samples}, flush=True)
    result = {"what": "strided bf16 input gradients of r2plus1d_18, per-class composition vs zsv_conv3d_bf16_dgrad, device ms per call",
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "iters": args.iters, "geometries": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
