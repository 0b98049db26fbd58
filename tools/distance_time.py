#!/usr/bin/env python3
"""Device time of the distance field and the ball morphology (arvx_distance, arvx_morph) on the sphere
scene's carved model at 512^3 with 36 views of 640x480, after arvx_carve of a fresh model.  Six legs,
WARMUP + REPS calls each, one after the other, every call on a freshly carved model:

    1. arvx_distance                                  4. arvx_morph DILATE, radius_sq 9
    2. arvx_distance, ARVX_DISTANCE_BORDER_OCCUPIED   5. arvx_morph OPEN, radius_sq 9
    3. arvx_morph ERODE, radius_sq 9                  6. arvx_morph CLOSE, radius_sq 9

Run it under the profiler, then let it read the trace (GPU required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/distance_time.py [N]
    python tools/distance_time.py --summarize OUT [N]

The first prints, per leg, the median host wall time around the call (arvx_distance is followed by a
synchronisation, arvx_morph synchronises itself) and writes host_times.json; the second prints, per
leg, the median over the calls of the summed kernel time and of each launch in order -- the row pass,
the column pass along y, the one along z, the thresholds, the record update -- beside the bytes the
launch has to move at least divided by the copy rate DESIGN.md quotes for the card (FLOOR_TBS), and
writes kernel_times.json and kernel_times.txt.  Both write into --out DIR (default profiles/distance)."""
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
RADIUS_SQ = 9
FLOOR_TBS = 6.3  # HBM copy rate measured on the card ("Peaks")
LEGS = ("arvx_distance", "arvx_distance BORDER_OCCUPIED", "arvx_morph ERODE", "arvx_morph DILATE",
        "arvx_morph OPEN", "arvx_morph CLOSE")
# the kernels of a call: its own, and the ones it borrows
OWN = ("dist_", "bitgrid_from_rec_kernel", "rec_andnot_bitgrid_kernel", "rec_or_bitgrid_kernel",
       "carve_fill_kernel", "fillBuffer")


def least_bytes(kernel, nvox):
    """What a launch has to read and write at least: the field once each way for a column pass, the plane
    in and the field out for the row pass, the field in and a plane out for a threshold."""
    if kernel.startswith("dist_column_kernel"):
        return 8 * nvox
    if kernel.startswith("dist_row_kernel") or kernel.startswith("dist_threshold_kernel"):
        return 4 * nvox + nvox // 8
    return None


def run(N, out_dir):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    capi.load_library()
    sc = syn.sphere_scene(N, V)
    result = {"N": N, "views": V, "image": [int(sc.W), int(sc.H)], "warmup": WARMUP, "reps": REPS,
              "radius_sq": RADIUS_SQ, "legs": {}}
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        lib, h = ctx._lib, ctx._h
        legs = (lambda: ctx._ck(lib.arvx_distance(h, 0)),
                lambda: ctx._ck(lib.arvx_distance(h, capi.DISTANCE_BORDER_OCCUPIED)),
                lambda: ctx.morph(capi.MORPH_ERODE, RADIUS_SQ), lambda: ctx.morph(capi.MORPH_DILATE, RADIUS_SQ),
                lambda: ctx.morph(capi.MORPH_OPEN, RADIUS_SQ), lambda: ctx.morph(capi.MORPH_CLOSE, RADIUS_SQ))
        print(f"{N}^3, {V} views of {sc.W}x{sc.H}, sphere scene, after arvx_carve of a fresh model; host wall time "
              f"around the call, median of {REPS}:")
        for name, leg in zip(LEGS, legs):
            t, answer = [], None
            for i in range(WARMUP + REPS):
                ctx.reset()
                ctx.carve()
                ctx.synchronize()
                t0 = time.perf_counter()
                answer = leg()
                ctx.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            occupied = int((ctx.download_state() & 1).sum())
            what = "" if answer is None else f"removed {answer[0]}, added {answer[1]}"
            print(f"  {name:32s} {np.median(t[WARMUP:]):8.3f} ms   occupied after {occupied}   {what}")
            result["legs"][name] = {"host_ms_median": float(np.median(t[WARMUP:])), "host_ms_min": float(min(t[WARMUP:])),
                                    "host_ms_max": float(max(t[WARMUP:])), "occupied_after": occupied, "answer": what}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "host_times.json"), "w") as f:
        json.dump(result, f, indent=1)


def summarize(trace_dir, out_dir, N):
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

    # a call: a run of OWN kernels that holds a dist_row_kernel; its launches are numbered in order
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
    mine = [c for own, c in calls if own and any(n.startswith("dist_row_kernel") for n, _ in c)]
    per = WARMUP + REPS
    if len(mine) != len(LEGS) * per:
        sys.exit(f"{len(mine)} distance calls in the trace, expected {len(LEGS) * per}")
    nvox = N ** 3
    out = {"N": N, "floor_tbs": FLOOR_TBS, "legs": {}}
    lines = [f"kernel time per call from {len(traces)} trace file(s), median of {REPS} (after {WARMUP} warm-up "
             f"calls); floor: the least bytes of the launch at {FLOOR_TBS} TB/s"]
    for li, name in enumerate(LEGS):
        cs = mine[li * per + WARMUP:(li + 1) * per]
        tot = [sum(d for _, d in c) for c in cs]
        n_launch = min(len(c) for c in cs)
        parts = []
        for k in range(n_launch):
            kernel = cs[0][k][0]
            us = float(np.median([c[k][1] for c in cs])) / 1e3
            b = least_bytes(kernel, nvox)
            floor_us = None if b is None else b / (FLOOR_TBS * 1e12) * 1e6
            parts.append({"launch": k, "kernel": kernel, "us_median": us, "floor_us": floor_us,
                          "times_floor": None if floor_us is None else us / floor_us})
        out["legs"][name] = {"kernels_us_median": float(np.median(tot)) / 1e3, "kernels_us_min": min(tot) / 1e3,
                             "kernels_us_max": max(tot) / 1e3, "launches": n_launch, "per_launch": parts}
        lines.append(f"  {name:32s} {np.median(tot) / 1e3:9.1f} us   (min {min(tot) / 1e3:.1f}, max {max(tot) / 1e3:.1f}; "
                     f"{n_launch} launches)")
        for p in parts:
            fl = "" if p["floor_us"] is None else f"   floor {p['floor_us']:7.1f} us, x{p['times_floor']:.1f}"
            lines.append(f"      {p['launch']:2d} {p['kernel']:36s} {p['us_median']:9.1f} us{fl}")
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernel_times.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, "kernel_times.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "distance")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    if args and args[0] == "--summarize":
        summarize(args[1], out_dir, int(args[2]) if len(args) > 2 else 512)
    else:
        run(int(args[0]) if args else 512, out_dir)
