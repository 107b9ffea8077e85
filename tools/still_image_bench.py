"""Cost of synthesising camera-motion clips from still images on the device (preprocess.StillImageClips).
    python bench.py --gpus 1 --steps 20 --warmup 5 > step.json
    python tools/still_image_bench.py --bench-json step.json [--out profiles/still_image_clips.json]

Workload: 22 images of 512 x 512, clip_len = 16, n_clips = 1, crop = 112: the 352 frames of one 22-clip training batch
(main.py --dataset sun2both, auxiliary/auxiliary_stillimages.py:92-138).  Two trajectory sets: `drawn` (the reference's
random start / end windows under a fixed seed) and `all_512` (every window the whole image: the most taps and source rows
the workload can ask for).  Every device time is from HIP events around one call, median of `--reps` calls after a warm-up:

* launch_us                 zsv_still_image_clips alone, tables already on the device
* call_us                   StillImageClips.__call__: checks, the two pinned tables, their uploads, the launch
* clip_transform_us         zsv_clip_transform (the video source's kernel) for the same output shape, same process
* pil_352_frames_ms         the host's PIL resizes of the same 352 frames on up to 16 CPU threads (PIL drops the GIL), and
                            single-threaded per frame
* fp32_step_ms              ms_per_step of `bench.py --gpus 1` (the 22-clip fp32 training step), read from --bench-json: the JSON
                            line of a run of its own on the same device (the step is never timed next to this process)

Acceptance: the launch takes no more than 5 % of the step."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zeroshotvideoclassification_amd import _lib, preprocess

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=22)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--clip-len", type=int, default=16)
ap.add_argument("--crop", type=int, default=112)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--bench-json", required=True,
                help="file holding the JSON line of `python bench.py --gpus 1 --steps 20 --warmup 5 > FILE`, run on the same device before this tool")
ap.add_argument("--out", default="")
args = ap.parse_args()
if args.reps < 20:
    raise SystemExit("still_image_bench: at least 20 timed calls")
if not torch.cuda.is_available():
    raise SystemExit("still_image_bench: needs the GPU (no CPU timing is meaningful here)")
dev = torch.device("cuda")
lib = _lib.load()
B, T, crop, size = args.images, args.clip_len, args.crop, args.size

rng = np.random.RandomState(0)
images_np = [rng.randint(0, 256, (size, size, 3)).astype(np.uint8) for _ in range(B)]
images = [torch.from_numpy(im).to(dev) for im in images_np]
np.random.seed(0)
trajectories = {"drawn": [preprocess.camera_motion_trajectory(size, size, crop, T) for _ in range(B)],
                "all_512": [np.tile(np.array([[0, 0, size]]), (T, 1)) for _ in range(B)]}
clips = preprocess.StillImageClips(clip_len=T, n_clips=1, crop_size=crop)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2), "calls": len(us)}


result = {"device": torch.cuda.get_device_name(dev), "images": B, "image_size": [size, size], "clip_len": T, "n_clips": 1, "crop": crop,
          "frames": B * T, "output_bytes": B * 3 * T * crop * crop * 4, "source_bytes": B * size * size * 3, "sets": {}}
itab = torch.tensor([[im.data_ptr(), size, size] for im in images], dtype=torch.int64).to(dev)
out = torch.empty((B, 1, 3, T, crop, crop), dtype=torch.float32, device=dev)
for name, traj in trajectories.items():
    table = np.ascontiguousarray(np.stack(traj), dtype=np.int32)         # (trajectories are transposed views)
    ftab = torch.from_numpy(table).to(dev)
    max_side = int(table[:, :, 2].max())

    def launch():
        _lib.check(lib.zsv_still_image_clips(itab.data_ptr(), ftab.data_ptr(), B, 1, T, crop, max_side, out.data_ptr(),
                                             c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_still_image_clips")
    entry = {"sides": [int(table[:, :, 2].min()), int(table[:, :, 2].max())], "mean_side": round(float(table[:, :, 2].mean()), 1),
             "launch_us": timed(launch), "call_us": timed(lambda: clips(images, trajectories=traj))}
    if not torch.equal(out, clips(images, trajectories=traj)) or not torch.isfinite(out).all():
        raise SystemExit("still_image_bench: the direct launch and StillImageClips disagree")
    entry["launch_output_GBps"] = round(result["output_bytes"] / entry["launch_us"]["median"] / 1e3, 1)
    result["sets"][name] = entry
    print(name, json.dumps(entry), flush=True)

# the video source's kernel for the same output shape: (22, 16, 128, 171, 3) uint8 -> (22, 3, 16, 112, 112)
frames = torch.randint(0, 256, (B, T, 128, 171, 3), dtype=torch.uint8, device=dev)
video = preprocess.ClipTransform(is_validation=True, crop_size=crop)
hres, wres, inv_scale = preprocess.resized_hw(128, 171, video.size)
ptab = torch.tensor(video.draw_params(B, hres, wres), dtype=torch.int32).to(dev)
vout = torch.empty((B, 3, T, crop, crop), dtype=torch.float32, device=dev)


def video_launch():
    _lib.check(lib.zsv_clip_transform(frames.data_ptr(), B, T, 128, 171, hres, wres, float(inv_scale), crop, ptab.data_ptr(),
                                      vout.data_ptr(), c_void_p(torch.cuda.current_stream().cuda_stream)), "zsv_clip_transform")


result["clip_transform_us"] = timed(video_launch)
print("clip_transform_us", json.dumps(result["clip_transform_us"]), flush=True)

# the host's PIL time for the same frames (the reference does one PIL resize per frame on a CPU worker)
try:
    from PIL import Image
except ImportError:
    Image = None
    result["pil_352_frames_ms"] = None
if Image is not None:
    jobs = [(b, int(t), int(l), int(s)) for b, traj in enumerate(trajectories["drawn"]) for t, l, s in traj]

    def one(job):
        b, t, l, s = job
        return Image.fromarray(images_np[b][t:t + s, l:l + s]).resize((crop, crop), Image.BILINEAR).size

    threads = max(1, min(args.threads, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    for job in jobs:
        one(job)
    serial_ms = 1e3 * (time.perf_counter() - t0)
    pooled = []
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(5):
            t0 = time.perf_counter()
            list(pool.map(one, jobs))
            pooled.append(1e3 * (time.perf_counter() - t0))
    result["pil_352_frames_ms"] = {"trajectories": "drawn", "threads": threads, "pooled_median": round(statistics.median(pooled), 2),
                                   "pooled_min": round(min(pooled), 2), "single_thread": round(serial_ms, 2),
                                   "single_thread_per_frame": round(serial_ms / len(jobs), 3)}
    print("pil_352_frames_ms", json.dumps(result["pil_352_frames_ms"]), flush=True)

# the 22-clip fp32 training step this source has to feed
with open(args.bench_json) as f:
    lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
source = ("the JSON line of `bench.py --gpus 1 --steps 20 --warmup 5`, run as a process of its own on the same device just before "
          "this tool (never next to it: the step is timed with the device to itself)")
bench = json.loads(lines[-1])
step_ms = float(bench["ms_per_step"])
result["fp32_step_ms"] = {"ms_per_step": step_ms, "clips_per_s": bench["value"], "metric": bench["metric"], "source": source}
worst = max(e["launch_us"]["median"] for e in result["sets"].values())
result["acceptance"] = {"launch_us_worst_set": worst, "launch_over_step": round(worst / 1e3 / step_ms, 5), "bound": 0.05,
                        "met": worst / 1e3 <= 0.05 * step_ms}
print(json.dumps(result["acceptance"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
