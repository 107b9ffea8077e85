"""The depthwise 3x3x3 convolutions of an ``ir_csn_50`` training step at 22 clips of 3 x 16 x 112 x 112, three directions each:
zsv_dwconv3d_fwd / _dgrad / _wgrad against torch's own ``F.conv3d(groups=C)`` and the ``aten::convolution_backward`` its autograd
calls, alternating in one process on one device.

    python tools/dwconv_bench.py [--batch 22] [--repeats 5] [--window 0.5] [--out profiles/dwconv.json]

Every shape and path is warmed first.  A sample is the mean device time (device events) of as many back-to-back calls as fill a
window of ``--window`` seconds; per row and path the file holds the median of ``--repeats`` samples and their spread (max - min),
the compulsory bytes of the direction (fwd |x| + |y|, dgrad |dy| + |dx|, wgrad |x| + |dy|, times 4), the bytes/s that makes and
its share of the 6.29 TB/s a float4 copy reaches on this chip.  The two results are compared before anything is timed."""
import argparse
import json
import math
import os
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from zeroshotvideoclassification_amd import _lib, ops

COPY_RATE = 6.29e12         # bytes/s of a float4 copy, the practical HBM ceiling of the chip
# name, channels, (T, H, W) of the input, stride: the five geometries of conv2 that carry the step's depthwise traffic (the
# strided first blocks of layer3 / layer4 are smaller than their stride-1 successors)
GEOMS = [
    ("layer1", 64, (16, 56, 56), 1),
    ("layer2.0", 128, (16, 56, 56), 2),
    ("layer2", 128, (8, 28, 28), 1),
    ("layer3", 256, (4, 14, 14), 1),
    ("layer4", 512, (2, 7, 7), 1),
]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def paths_of(n, c, thw, stride, seed):
    """direction -> (ours, torch's, compulsory bytes); the operands live as long as the closures"""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    lib = _lib.load()
    s, p = (stride,) * 3, (1, 1, 1)
    x = torch.randn((n, c) + tuple(thw), generator=g, device=dev)
    w = torch.randn((c, 1, 3, 3, 3), generator=g, device=dev) * 27 ** -0.5
    d = ops.conv_desc(x.shape, (c, c, 3, 3, 3), s, p)
    y = torch.empty((n, c, d.To, d.Ho, d.Wo), device=dev)
    dy = torch.randn(y.shape, generator=g, device=dev)
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    nbytes = int(lib.zsv_dwconv3d_wgrad_workspace_bytes(byref(d)))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)

    def ours_fwd():
        _lib.check(lib.zsv_dwconv3d_fwd(byref(d), x.data_ptr(), w.data_ptr(), None, y.data_ptr(), 0, ops._stream()), "fwd")
        return y

    def ours_dgrad():
        _lib.check(lib.zsv_dwconv3d_dgrad(byref(d), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), ops._stream()), "dgrad")
        return dx

    def ours_wgrad():
        _lib.check(lib.zsv_dwconv3d_wgrad(byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), "wgrad")
        return dw

    def backward(mask):
        return torch.ops.aten.convolution_backward(dy, x, w, None, s, p, (1, 1, 1), False, (0, 0, 0), c, mask)

    return {"fwd": (ours_fwd, lambda: F.conv3d(x, w, None, s, p, 1, c), 4 * (x.numel() + y.numel())),
            "dgrad": (ours_dgrad, lambda: backward((True, False, False))[0], 4 * (dy.numel() + dx.numel())),
            "wgrad": (ours_wgrad, lambda: backward((False, True, False))[1], 4 * (x.numel() + dy.numel()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed sample (at least 0.5)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench: an MI355X is needed (there is no CPU fallback)")
    window = max(args.window, 0.5)
    rows = []
    for i, (name, c, thw, stride) in enumerate(GEOMS):
        for direction, (ours, theirs, nbytes) in paths_of(args.batch, c, thw, stride, 300 + i).items():
            a, b = ours().double(), theirs().double()
            torch.cuda.synchronize()
            err = float((a - b).abs().max() / b.abs().max())
            assert err < 1e-4, f"{name} {direction}: the two paths differ ({err:.2e})"
            fns = {"zsv": ours, "torch": theirs}
            iters = {}
            for k, fn in fns.items():                                  # warm-up, and the calls that fill one window
                timed(fn, 3)
                iters[k] = max(3, int(math.ceil(window * 1e3 / timed(fn, 10))))
            samples = {k: [] for k in fns}
            for _ in range(args.repeats):                              # alternate the paths inside every repeat
                for k, fn in fns.items():
                    samples[k].append(timed(fn, iters[k]))
            row = {"name": name, "direction": direction, "clips": args.batch, "channels": c, "thw": list(thw), "stride": stride,
                   "compulsory_bytes": nbytes, "max_rel_difference": err}
            for k, v in samples.items():
                v = sorted(v)
                med = v[len(v) // 2]
                rate = nbytes / (med * 1e-3)
                row[k] = {"median_ms": round(med, 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "spread_ms": round(v[-1] - v[0], 4),
                          "calls_per_sample": iters[k], "bytes_per_s": round(rate, 0), "share_of_copy_rate": round(rate / COPY_RATE, 4)}
            row["zsv_over_torch"] = round(row["zsv"]["median_ms"] / row["torch"]["median_ms"], 4)
            # slower than torch's by more than the run-to-run spread of the two?
            row["slower_than_torch"] = bool(row["zsv"]["median_ms"] - row["torch"]["median_ms"] > row["zsv"]["spread_ms"] + row["torch"]["spread_ms"])
            rows.append(row)
            print(name, direction, {k: (row[k]["median_ms"], row[k]["share_of_copy_rate"]) for k in fns}, flush=True)
    result = {"what": "depthwise 3x3x3 convolutions of ir_csn_50 (fp32), zsv_dwconv3d_* vs torch (F.conv3d groups=C / aten::convolution_backward), "
                      "device ms per call; outputs of the zsv calls are preallocated, torch's come from its caching allocator",
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "repeats": args.repeats, "window_s": window,
              "copy_rate_bytes_per_s": COPY_RATE, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({"rows": len(rows), "slower_than_torch": [f"{r['name']} {r['direction']}" for r in rows if r["slower_than_torch"]]}))


if __name__ == "__main__":
    main()
