#!/usr/bin/env python3
"""Device time of the connected components (arvx_components, arvx_components_keep) on the three-ball
scene -- the sphere scene with three small spheres OR-ed into its masks, which a carve leaves as
four components -- at 512^3 with 36 views of 640x480, after arvx_carve of a fresh model.  Five legs,
WARMUP + REPS calls each, one after the other, every call on a freshly carved model:

    1. arvx_components, connectivity 6
    2. arvx_components, connectivity 26
    3. arvx_components_keep, ARVX_COMPONENTS_LARGEST, connectivity 6
    4. arvx_components_keep, ARVX_COMPONENTS_LARGEST, connectivity 26
    5. arvx_fast_carve of a fresh model (the yardstick: its flood is the library's other walk over
       the grid's connectivity)

Run it under the profiler, then let it read the trace (GPU required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/components_time.py [N]
    python tools/components_time.py --summarize OUT

The first prints, per leg, the median host wall time around the call (the calls of legs 1 to 4
synchronise themselves; leg 5 is followed by a synchronisation) and writes host_times.json; the
second prints, per leg, the median over the calls of the summed kernel time and of each kernel, and
writes kernel_times.json.  Both write into --out DIR (default profiles/components)."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V = 36
WARMUP = 2
REPS = 9
LEGS = ("arvx_components 6", "arvx_components 26", "arvx_components_keep LARGEST 6",
        "arvx_components_keep LARGEST 26", "arvx_fast_carve")
BALLS = (((0.36, 0.0, 0.0), 0.06), ((0.0, 0.36, 0.1), 0.05), ((-0.3, -0.3, -0.05), 0.04))
# the kernels of a components call: its own, and the ones it borrows
OWN = ("comp_", "bitgrid_from_rec_kernel", "bit_compact_counted_kernel", "rec_andnot_bitgrid_kernel",
       "carve_fill_kernel", "fillBuffer")


def scene(N):
    from ar_voxel_project_amd import synthetic as syn
    sc = syn.sphere_scene(N, V, radius_factor=0.25)
    _, c = syn.ring_cameras(V)
    for off, r in BALLS:
        sc.masks |= syn.sphere_masks(sc.K, sc.Rt, c + np.array(off) * syn.EXTENT, r * syn.EXTENT, sc.W, sc.H)
    return sc


def run(N, out_dir):
    from ar_voxel_project_amd import capi
    capi.load_library()
    sc = scene(N)
    result = {"N": N, "views": V, "image": [int(sc.W), int(sc.H)], "warmup": WARMUP, "reps": REPS, "legs": {}}
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        answers = {}
        legs = (lambda: ctx.components(6), lambda: ctx.components(26),
                lambda: ctx.keep_components(largest=True, connectivity=6),
                lambda: ctx.keep_components(largest=True, connectivity=26), lambda: ctx.fast_carve())
        print(f"{N}^3, {V} views of {sc.W}x{sc.H}, three-ball scene, after arvx_carve of a fresh model; host wall "
              f"time around the call, median of {REPS}:")
        for name, leg in zip(LEGS, legs):
            t = []
            for i in range(WARMUP + REPS):
                ctx.reset()
                if leg is not legs[4]:
                    ctx.carve()
                ctx.synchronize()
                t0 = time.perf_counter()
                answers[name] = leg()
                ctx.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            occupied = int((ctx.download_state() & 1).sum())
            a = answers[name]
            what = "" if a is None else (f"sizes {sorted(map(int, a[1]), reverse=True)}" if isinstance(a[0], np.ndarray)
                                         else f"kept {a[0]}, removed {a[1]}")
            print(f"  {name:34s} {np.median(t[WARMUP:]):8.3f} ms   occupied after {occupied}   {what}")
            result["legs"][name] = {"host_ms_median": float(np.median(t[WARMUP:])), "host_ms_min": float(min(t[WARMUP:])),
                                    "host_ms_max": float(max(t[WARMUP:])), "occupied_after": occupied, "answer": what}
    XW = (N + 63) // 64
    result["plane_bytes"] = XW * N * N * 8
    result["label_bytes"] = N ** 3 * 4
    print(f"one bit plane: {result['plane_bytes'] / 2**20:.1f} MiB; the labels: {result['label_bytes'] / 2**20:.0f} MiB")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "host_times.json"), "w") as f:
        json.dump(result, f, indent=1)


def summarize(trace_dir, out_dir):
    traces = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for path in traces:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()

    def short(name):
        name = name.split("(")[0]
        return name.replace("arvx::", "").replace("void ", "").strip()

    # a components call: a run of OWN kernels that holds a comp_init_kernel
    calls, cur, cur_own = [], [], None
    for start, end, name in rows:
        own = any(k in name for k in OWN)
        if cur and own != cur_own:
            calls.append((cur_own, cur))
            cur = []
        cur_own = own
        cur.append((short(name), end - start))
    if cur:
        calls.append((cur_own, cur))
    comp = [c for own, c in calls if own and any(n.startswith("comp_init_kernel") for n, _ in c)]
    per = WARMUP + REPS
    if len(comp) != 4 * per:
        sys.exit(f"{len(comp)} components calls in the trace, expected {4 * per}")
    out = {"legs": {}}
    print(f"kernel time per call from {len(traces)} trace file(s), median of {REPS} (after {WARMUP} warm-up calls):")
    for li, name in enumerate(LEGS[:4]):
        cs = comp[li * per + WARMUP:(li + 1) * per]
        tot = [sum(d for _, d in c) for c in cs]
        names = []
        for n, _ in cs[0]:
            if n not in names:
                names.append(n)
        parts = {n: float(np.median([sum(d for m, d in c if m == n) for c in cs])) / 1e3 for n in names}
        out["legs"][name] = {"kernels_us_median": float(np.median(tot)) / 1e3, "kernels_us_min": min(tot) / 1e3,
                             "kernels_us_max": max(tot) / 1e3, "launches": len(cs[0]), "per_kernel_us": parts}
        print(f"  {name:34s} {np.median(tot) / 1e3:9.1f} us   (min {min(tot) / 1e3:.1f}, max {max(tot) / 1e3:.1f}; "
              f"{len(cs[0])} launches)")
        for n, v in parts.items():
            print(f"      {n:40s} {v:9.1f} us")
    # the greedy carve's flood: its calls follow each other without a kernel of the components between
    # them, so the mean over all of them (warm-up calls included) instead of a median
    fl = [(n, d) for _, c in calls for n, d in c if "flood" in n or "fill_row" in n]
    if fl:
        out["legs"][LEGS[4]] = {"flood_kernels_us_mean": sum(d for _, d in fl) / per / 1e3,
                                "flood_launches_mean": len(fl) / per}
        print(f"  {LEGS[4]:34s} flood kernels {sum(d for _, d in fl) / per / 1e3:9.1f} us per call "
              f"({len(fl) / per:.1f} launches; mean of {per} calls)")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernel_times.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "components")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    if args and args[0] == "--summarize":
        summarize(args[1], out_dir)
    else:
        run(int(args[0]) if args else 512, out_dir)
