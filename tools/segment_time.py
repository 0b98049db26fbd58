#!/usr/bin/env python3
"""What arvx_segment_views costs: kernel time from HIP events around the call on the context's stream,
the median of five rounds of twenty calls each after a warm-up, at 36 views of 640 x 480.

  device form   arvx_segment_views_device with (a) the rule only, (b) plus open 1 and close 2, (c) plus
                specks (min_area 20) and holes (any size); beside them arvx_set_views_device on the
                final masks of (c) -- re-deriving the views is part of every segment call
  host form     arvx_segment_views against arvx_set_views + arvx_set_images of the same frames, wall
                time, PCIe included

python tools/segment_time.py [views=36] [json path]
python tools/segment_time.py 36 trace      five calls of (c) after a warm-up, for a kernel trace"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ar_voxel_project_amd import capi, synthetic as syn  # noqa: E402

V = int(sys.argv[1]) if len(sys.argv) > 1 else 36
ROUNDS, WARMUP, REPS = 5, 2, 20
sc = syn.textured_sphere_scene(64, V)
W, H = sc.W, sc.H
# the frames: the sphere's photographs with salt and pepper (what the opening and the closing remove), four
# bright 4 x 4 specks in the background and two dark 6 x 6 holes in the silhouette per view (what
# survives them and is left to the components)
rng = np.random.default_rng(0)
frames = sc.images.copy()
salt = rng.random((V, H, W)) < 0.002
frames[salt] = np.where(frames[salt].max(axis=-1, keepdims=True) > 20, 0, 200).astype(np.uint8)
for k in range(4):
    frames[:, 20:24, 20 + 40 * k:24 + 40 * k] = 200
for dx in (-20, 20):
    frames[:, H // 2 - 3:H // 2 + 3, W // 2 + dx - 3:W // 2 + dx + 3] = 0
DARK = dict(lo=(0, 0, 0), hi=(20, 20, 20))
CASES = [("rule", dict(**DARK)),
         ("rule+open1+close2", dict(open_radius=1, close_radius=2, **DARK)),
         ("rule+open1+close2+specks+holes", dict(open_radius=1, close_radius=2, min_area=20, max_hole=-1, **DARK))]

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = capi.Context(64, 64, 64, sc.voxel_size)
ctx.set_stream(stream.cuda_stream)
d_frames = torch.from_numpy(frames).to(dev)


def timed(call):
    """median kernel time of call() in microseconds"""
    out = []
    for r in range(WARMUP + ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(REPS):
            call()
        b.record(stream)
        torch.cuda.synchronize()
        if r >= WARMUP:
            out.append(a.elapsed_time(b) * 1e3 / REPS)
    return statistics.median(out), min(out), max(out)


def wall(call):
    out = []
    for r in range(WARMUP + ROUNDS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if r >= WARMUP:
            out.append((time.perf_counter() - t) * 1e6)
    return statistics.median(out), min(out), max(out)


if len(sys.argv) > 2 and sys.argv[2] == "trace":
    for _ in range(WARMUP + 5):
        ctx.segment_views_device(sc.M, d_frames.data_ptr(), W, H, campos=sc.campos, **CASES[-1][1])
    torch.cuda.synchronize()
    sys.exit(0)

result = {"views": V, "W": W, "H": H, "rounds": ROUNDS, "calls_per_round": REPS, "device_form_us": {}, "host_form_us": {}}
for name, kw in CASES:
    med, lo, hi = timed(lambda: ctx.segment_views_device(sc.M, d_frames.data_ptr(), W, H, campos=sc.campos, **kw))
    result["device_form_us"][name] = {"median": med, "min": lo, "max": hi}
    print(f"segment_views_device {name}: {med:.1f} us (min {lo:.1f}, max {hi:.1f})", flush=True)
masks = np.stack([ctx.segment_mask(v) for v in range(V)])
counts = np.stack([ctx.segment_counts(v) for v in range(V)])
result["counts_sum"] = [int(c) for c in counts.sum(axis=0)]
d_masks = torch.from_numpy(masks).to(dev)
med, lo, hi = timed(lambda: ctx.set_views_device(sc.M, d_masks.data_ptr(), W, H, 1, campos=sc.campos))
result["device_form_us"]["set_views_device"] = {"median": med, "min": lo, "max": hi}
print(f"set_views_device on the final masks: {med:.1f} us (min {lo:.1f}, max {hi:.1f})", flush=True)

name, kw = CASES[-1]
med, lo, hi = wall(lambda: ctx.segment_views(sc.M, frames, sc.campos, **kw))
result["host_form_us"]["segment_views " + name] = {"median": med, "min": lo, "max": hi}
print(f"segment_views (host, {name}): {med:.1f} us wall (min {lo:.1f}, max {hi:.1f})", flush=True)


def two_calls():
    ctx.set_views(sc.M, masks, sc.campos)
    ctx.set_images(frames)


med, lo, hi = wall(two_calls)
result["host_form_us"]["set_views + set_images"] = {"median": med, "min": lo, "max": hi}
print(f"set_views + set_images (host): {med:.1f} us wall (min {lo:.1f}, max {hi:.1f})", flush=True)
print(json.dumps(result))
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
