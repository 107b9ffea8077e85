"""Cost of transforming a batch of videos of different frame sizes on the device (preprocess.VideoClips).
    python bench.py --gpus 1 --steps 20 --warmup 5 --full > step.json      # --full adds extra.train_bf16, the bf16 step
    python tools/clip_batch_bench.py --bench-json step.json [--out profiles/clip_batch.json]

Two workloads, both 22 videos of 16 frames, n_clips = 1, crop 112 (one 22-clip training batch):

* mixed     a fixed mix of 256 x 340, 256 x 454, 340 x 256 and 240 x 320 frames (what one Kinetics batch holds)
  - launch_us            zsv_clip_transform_batch alone, table already on the device
  - call_us              VideoClips.__call__: checks, draws, the pinned table, its upload, the launch
  - per_video_calls_us   22 ClipTransform calls (one launch + one parameter upload each) + torch.stack: the only way to
                         do this batch without the batch entry point
  - stage_ms             VideoClips.stage of the whole batch: the host copies into the pinned buffer, one upload; host
                         clock from the call to the end of a device synchronise
* uniform   22 x 16 x 240 x 320: launch_us of the batch kernel and clip_transform_us of zsv_clip_transform for the same
            frames and parameters, timed alternately in this process; their outputs must be bit-identical

Every device time is from HIP events around one call, median and min - max of `--reps` calls after a warm-up.
fp32_step_ms / bf16_step_ms: ms_per_step of `bench.py --gpus 1` and of its extra.train_bf16, read from --bench-json: the JSON
line of a run of its own on the same device (the step is never timed next to this process); without --full the line has
no bf16 step and that share is null.

Bounds written into the JSON: the mixed launch takes no more than 5 % of the fp32 step; on the uniform workload the batch
kernel's median does not exceed zsv_clip_transform's by more than the larger of the two min - max spreads; call_us is below
per_video_calls_us."""
import argparse
import json
import os
import random
import statistics
import sys
import time
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zeroshotvideoclassification_amd import _lib, preprocess

MIX = [(256, 340), (256, 454), (340, 256), (240, 320)]

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=22)
ap.add_argument("--clip-len", type=int, default=16)
ap.add_argument("--crop", type=int, default=112)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--bench-json", required=True,
                help="file holding the JSON line of `python bench.py --gpus 1 --steps 20 --warmup 5 --full > FILE`, run on the same device before this tool")
ap.add_argument("--out", default="")
args = ap.parse_args()
if args.reps < 20:
    raise SystemExit("clip_batch_bench: at least 20 timed calls")
if not torch.cuda.is_available():
    raise SystemExit("clip_batch_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()
B, T, crop = args.videos, args.clip_len, args.crop
clips = preprocess.VideoClips(False, n_clips=1, clip_len=T, crop_size=crop)
single = preprocess.ClipTransform(False, crop)


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def summary(us, digits=2):
    return {"median": round(statistics.median(us), digits), "min": round(min(us), digits), "max": round(max(us), digits), "calls": len(us)}


def one_call_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def timed(*fns):
    """HIP events around one call; several functions are timed alternately (a, b, a, b, ...)."""
    for _ in range(args.warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(args.reps):
        for k, fn in enumerate(fns):
            us[k].append(one_call_us(fn))
    return [summary(u) for u in us]


def batch_launch(vtab, out):
    def launch():
        _lib.check(lib.zsv_clip_transform_batch(vtab.data_ptr(), B, 1, T, crop, out.data_ptr(), stream()), "zsv_clip_transform_batch")
    return launch


result = {"device": torch.cuda.get_device_name(dev), "videos": B, "clip_len": T, "n_clips": 1, "crop": crop,
          "output_bytes": B * 3 * T * crop * crop * 4, "reps": args.reps, "warmup": args.warmup}
rng = np.random.RandomState(0)
random.seed(0)

# ---- mixed -------------------------------------------------------------------------------------------------------------
sizes = [MIX[b % len(MIX)] for b in range(B)]
arrays = [rng.randint(0, 256, (T, h, w, 3)).astype(np.uint8) for h, w in sizes]
videos = [torch.from_numpy(a).to(dev) for a in arrays]
params = clips.draw_params(sizes)
vtab = torch.from_numpy(preprocess.video_table([v.data_ptr() for v in videos], sizes, params, clips.size)).to(dev)
out = torch.empty((B, 1, 3, T, crop, crop), dtype=torch.float32, device=dev)


def per_video_calls():
    return torch.stack([single(v.unsqueeze(0), params=[p]) for v, p in zip(videos, params)])


mixed = {"frame_sizes": {f"{h}x{w}": sizes.count((h, w)) for h, w in MIX}, "source_bytes": int(sum(a.nbytes for a in arrays))}
mixed["launch_us"], = timed(batch_launch(vtab, out))
mixed["call_us"], mixed["per_video_calls_us"] = timed(lambda: clips(videos), per_video_calls)
if not torch.equal(out, clips(videos, params=params)) or not torch.equal(out, per_video_calls()) or not torch.isfinite(out).all():
    raise SystemExit("clip_batch_bench: the direct launch, VideoClips and the per-video calls disagree")
for _ in range(args.warmup):
    clips.stage(arrays)
torch.cuda.synchronize()
stage_ms = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    staged = clips.stage(arrays)
    torch.cuda.synchronize()
    stage_ms.append(1e3 * (time.perf_counter() - t0))
if not torch.equal(out, clips(staged, params=params)):
    raise SystemExit("clip_batch_bench: staged videos give another result")
mixed["stage_ms"] = summary(stage_ms, 3)
mixed["stage_GBps"] = round(mixed["source_bytes"] / mixed["stage_ms"]["median"] / 1e6, 2)
mixed["launch_output_GBps"] = round(result["output_bytes"] / mixed["launch_us"]["median"] / 1e3, 1)
mixed["call_over_per_video_calls"] = round(mixed["call_us"]["median"] / mixed["per_video_calls_us"]["median"], 4)
result["mixed"] = mixed
print("mixed", json.dumps(mixed), flush=True)
del videos, staged, arrays

# ---- uniform -----------------------------------------------------------------------------------------------------------
h, w = 240, 320
frames = torch.from_numpy(rng.randint(0, 256, (B, T, h, w, 3)).astype(np.uint8)).to(dev)
hres, wres, inv_scale = preprocess.resized_hw(h, w, single.size)
params = clips.draw_params([(h, w)] * B)
ptab = torch.tensor(params, dtype=torch.int32).to(dev)
vtab_u = torch.from_numpy(preprocess.video_table([frames[b].data_ptr() for b in range(B)], [(h, w)] * B, params, clips.size)).to(dev)
dense = torch.empty((B, 3, T, crop, crop), dtype=torch.float32, device=dev)


def dense_launch():
    _lib.check(lib.zsv_clip_transform(frames.data_ptr(), B, T, h, w, hres, wres, float(inv_scale), crop, ptab.data_ptr(), dense.data_ptr(),
                                      stream()), "zsv_clip_transform")


uniform = {"frame_size": [h, w], "source_bytes": frames.numel()}
uniform["launch_us"], uniform["clip_transform_us"] = timed(batch_launch(vtab_u, out), dense_launch)
if not torch.equal(out, dense.unsqueeze(1)):
    raise SystemExit("clip_batch_bench: the batch kernel and zsv_clip_transform differ on one frame size")
uniform["bit_identical"] = True
result["uniform"] = uniform
print("uniform", json.dumps(uniform), flush=True)

# ---- the steps this has to feed ----------------------------------------------------------------------------------------
with open(args.bench_json) as f:
    lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
bench = json.loads(lines[-1])
source = ("the JSON line of `bench.py --gpus 1 --steps 20 --warmup 5 --full`, run as a process of its own on the same device just before "
          "this tool (never next to it: the step is timed with the device to itself)")
step_ms = float(bench["ms_per_step"])
result["fp32_step_ms"] = {"ms_per_step": step_ms, "clips_per_s": bench["value"], "metric": bench["metric"], "source": source}
bf16 = (bench.get("extra") or {}).get("train_bf16") or {}
bf16_ms = float(bf16["ms_per_step"]) if "ms_per_step" in bf16 else None
result["bf16_step_ms"] = {"ms_per_step": bf16_ms, "source": "extra.train_bf16 of the same line"}
launch_ms = mixed["launch_us"]["median"] / 1e3
spread = max(uniform[k]["max"] - uniform[k]["min"] for k in ("launch_us", "clip_transform_us"))
excess = uniform["launch_us"]["median"] - uniform["clip_transform_us"]["median"]
result["bounds"] = {
    "input_synthesis": {"mixed_launch_us": mixed["launch_us"]["median"], "launch_over_fp32_step": round(launch_ms / step_ms, 5), "bound": 0.05,
                        "launch_over_bf16_step": None if bf16_ms is None else round(launch_ms / bf16_ms, 5),
                        "met": launch_ms <= 0.05 * step_ms},
    "against_clip_transform": {"launch_us_median": uniform["launch_us"]["median"], "clip_transform_us_median": uniform["clip_transform_us"]["median"],
                               "excess_us": round(excess, 2), "larger_min_max_spread_us": round(spread, 2), "met": excess <= spread},
    "against_per_video_calls": {"call_us": mixed["call_us"]["median"], "per_video_calls_us": mixed["per_video_calls_us"]["median"],
                                "ratio": mixed["call_over_per_video_calls"],
                                "met": mixed["call_us"]["median"] < mixed["per_video_calls_us"]["median"]}}
print(json.dumps(result["bounds"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
