"""The e4m3 evaluation engine next to the bf16 one, BASELINE config 5 geometry: 32-frame 112x112 clips.

python tools/eval_bench_fp8.py [--batch 22] [--frames 32] [--iters 10] [--rounds 3]
    forward-only clips/s of Fp8Engine and Bf16Engine in the same process, alternating rounds; the whole
    train.evaluate() protocol (forward + nearest class + the half-class splits) in both dtypes; per-layer times of
    S1 (layer1 64->144 1x3x3), T1 (144->64 3x1x1 + residual), S4 (layer4 512->1152 1x3x3) and T4 (1152->512 3x1x1 + residual).
python tools/eval_bench_fp8.py --layer S1 --dtype fp8 --iters 3
    only that layer's convolution (for a counter-only rocprofv3 --pmc run); one JSON line either way."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from types import SimpleNamespace

from zeroshotvideoclassification_amd import inference, network, synthetic, train

FP8 = torch.float8_e4m3fn
DTYPES = {"fp8": FP8, "bf16": torch.bfloat16}


def layer_calls(eng, clips):
    """{name: (op, input, residual)} for S1 / T1 (layer1 block 0) and S4 / T4 (layer4 block 1), captured by one trunk walk."""
    want = {id(eng.blocks[0][0][0]): "S1", id(eng.blocks[0][1][1]): "T1", id(eng.blocks[-1][0][0]): "S4",
            id(eng.blocks[-1][1][1]): "T4"}
    got = {}
    originals = {}
    for conv1, conv2, _ in eng.blocks:
        for op in conv1 + conv2:
            if id(op) in want:
                originals[id(op)] = op

    class Spy:
        def __init__(self, op):
            self.op = op

        def __call__(self, x, residual=None, wo=None):
            got[want[id(self.op)]] = (self.op, x, residual)
            return self.op(x, residual=residual)

    def swap(lst):
        return [Spy(o) if id(o) in want else o for o in lst]

    saved = eng.blocks
    eng.blocks = [(swap(c1), swap(c2), d) for c1, c2, d in saved]
    try:
        eng.trunk(clips)
    finally:
        eng.blocks = saved
    return got


def time_it(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=22)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layer", choices=["S1", "T1", "S4", "T4"])
    ap.add_argument("--dtype", choices=list(DTYPES), default="fp8")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = network.get_network(SimpleNamespace(network="r2plus1d_18", fixconvs=False, nopretrained=False))
    model.load_state_dict(synthetic.keyed_state_dict(model.state_dict(), seed=0, bn_jitter=True))
    model = model.to(dev).eval()
    x = synthetic.synthetic_clips(a.batch, a.frames, 112).to(dev)
    clips = x.reshape(a.batch, *x.shape[2:])
    engines = {k: inference.engine_for(model, v) for k, v in DTYPES.items() if not a.layer or k == a.dtype}
    shape = f"{a.batch} clips 3x{a.frames}x112x112"
    if a.layer:
        op, xin, res = layer_calls(engines[a.dtype], clips)[a.layer]
        dt = time_it(lambda: op(xin, residual=res), a.iters)
        print(json.dumps({"workload": f"{a.layer} {a.dtype}, {shape}", "ms": dt * 1e3}))
        return
    rounds = {k: [] for k in DTYPES}
    for _ in range(a.rounds):                                  # alternating: fp8, bf16, fp8, bf16, ...
        for k, eng in engines.items():
            rounds[k].append(time_it(lambda: eng(x), a.iters) * 1e3)
    out = {"workload": f"r2plus1d_18 eval forward, {shape}"}
    for k in DTYPES:
        best = min(rounds[k])
        out[f"{k}_forward_ms"] = rounds[k]
        out[f"{k}_clips_per_s"] = a.batch / best * 1e3
    out["fp8_speedup_forward"] = min(rounds["bf16"]) / min(rounds["fp8"])
    for k, eng in engines.items():
        for name, (op, xin, res) in layer_calls(eng, clips).items():
            out[f"{k}_{name}_ms"] = time_it(lambda: op(xin, residual=res), a.iters) * 1e3
    table = synthetic.class_table(101)
    batches = []
    for i in range(3):
        xb = synthetic.synthetic_clips(a.batch, a.frames, 112, seed=700 + i)
        labels, z = synthetic.synthetic_targets(a.batch, 101, rank=i)
        batches.append((xb, labels, z))
    for _ in range(a.rounds):
        for k, v in DTYPES.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = train.evaluate(model, batches, table, device=dev, splits=10, dtype=v)
            torch.cuda.synchronize()
            rate = r["n"] / (time.perf_counter() - t0)
            out[f"{k}_protocol_clips_per_s"] = max(out.get(f"{k}_protocol_clips_per_s", 0.0), rate)
            out[f"{k}_protocol_top1"], out[f"{k}_protocol_top5"] = r["accuracy"], r["accuracy_top5"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
