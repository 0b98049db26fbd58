#!/usr/bin/env python3
"""Device time of the refined mesh (arvx_mc_mesh_refined) beside the welded mesh of the same state: the
sphere scene's carved model at 512^3 with 36 views of 640x480.  Four legs, WARMUP + REPS calls each, one
after the other on the one carved state:

    1. arvx_mc_mesh_welded          3. arvx_mc_mesh_refined, 4 bisections
    2. arvx_mc_mesh_refined, 0      4. arvx_mc_mesh_refined, 8 bisections

Run it under the profiler, then let it read the trace (GPU required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mesh_refine_time.py [N]
    python tools/mesh_refine_time.py --summarize OUT [N]

The first prints, per leg, the median host wall time of the call (each has its one synchronisation) and
the mesh's counts, and writes host_times.json; the second prints, per leg, the median over the calls of
the summed kernel time and of each kernel, and for the bisection kernel the projections it makes at most
-- Vr * (B + 2) * V -- per second beside the brute-force carve's (CARVE_PROJ_PER_S), and writes
kernel_times.json and kernel_times.txt.  Both write into --out DIR (default profiles/mesh_refine)."""
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
LEGS = (("arvx_mc_mesh_welded", None), ("arvx_mc_mesh_refined B=0", 0), ("arvx_mc_mesh_refined B=4", 4),
        ("arvx_mc_mesh_refined B=8", 8))
# the brute-force carve at 512^3 x 36 views: 512^3 * 36 projections in 1.73 ms (profiles/r5_kernel_v28)
CARVE_PROJ_PER_S = 512 ** 3 * 36 / 1.73e-3
FIRST_KERNEL = "bitgrid_from_rec_kernel"  # every mesh call starts with the occupancy plane


def run(N, out_dir):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    capi.load_library()
    sc = syn.sphere_scene(N, V)
    result = {"N": N, "views": V, "image": [int(sc.W), int(sc.H)], "warmup": WARMUP, "reps": REPS, "legs": {}}
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        ctx.carve()
        ctx.synchronize()
        print(f"{N}^3, {V} views of {sc.W}x{sc.H}, sphere scene, after arvx_carve of a fresh model; host wall time "
              f"of the call, median of {REPS}:")
        for name, B in LEGS:
            t, counts = [], None
            for i in range(WARMUP + REPS):
                t0 = time.perf_counter()
                counts = ctx.mc_mesh_welded_count() if B is None else ctx.mc_mesh_refined_count(B)
                t.append((time.perf_counter() - t0) * 1e3)
            print(f"  {name:28s} {np.median(t[WARMUP:]):8.3f} ms   vertices {counts[0]}   triangles {counts[1]}")
            result["legs"][name] = {"host_ms_median": float(np.median(t[WARMUP:])), "host_ms_min": float(min(t[WARMUP:])),
                                    "host_ms_max": float(max(t[WARMUP:])), "vertices": counts[0], "triangles": counts[1]}
        result["host_total_fallbacks"] = int(ctx.stats()["host_total_fallbacks"])
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
        return name.split("(")[0].split("<")[0].replace("arvx::", "").replace("void ", "").strip()

    calls = []
    for start, end, name in rows:
        if FIRST_KERNEL in name:
            calls.append([])
        if calls:
            calls[-1].append((short(name), end - start))
    per = WARMUP + REPS
    if len(calls) != len(LEGS) * per:
        sys.exit(f"{len(calls)} mesh calls in the trace, expected {len(LEGS) * per}")
    counts = {}
    host = os.path.join(out_dir, "host_times.json")
    if os.path.exists(host):
        counts = {k: v["vertices"] for k, v in json.load(open(host))["legs"].items()}
    out = {"N": N, "carve_proj_per_s": CARVE_PROJ_PER_S, "legs": {}}
    lines = [f"kernel time per call from {len(traces)} trace file(s), median of {REPS} (after {WARMUP} warm-up calls)"]
    for li, (name, B) in enumerate(LEGS):
        cs = calls[li * per + WARMUP:(li + 1) * per]
        tot = [sum(d for _, d in c) for c in cs]
        kernels = []
        for k, _ in cs[0]:
            if k not in kernels:
                kernels.append(k)
        parts = {k: float(np.median([sum(d for n, d in c if n == k) for c in cs])) / 1e3 for k in kernels}
        leg = {"kernels_us_median": float(np.median(tot)) / 1e3, "kernels_us_min": min(tot) / 1e3,
               "kernels_us_max": max(tot) / 1e3, "launches": len(cs[0]), "per_kernel_us": parts}
        lines.append(f"  {name:28s} {np.median(tot) / 1e3:9.1f} us   (min {min(tot) / 1e3:.1f}, max {max(tot) / 1e3:.1f}; "
                     f"{len(cs[0])} launches)")
        for k, us in parts.items():
            lines.append(f"      {k:36s} {us:9.1f} us")
        if B is not None and name in counts and "mc_refine_vertex_kernel" in parts:
            proj = counts[name] * (B + 2) * V
            rate = proj / (parts["mc_refine_vertex_kernel"] * 1e-6)
            leg.update(projections_at_most=proj, proj_per_s=rate, carve_rate_over_this=CARVE_PROJ_PER_S / rate)
            lines.append(f"      at most {proj / 1e6:.1f} M projections: {rate / 1e9:.1f} G/s; the brute-force carve makes "
                         f"{CARVE_PROJ_PER_S / 1e9:.0f} G/s, {CARVE_PROJ_PER_S / rate:.1f} times as many")
        out["legs"][name] = leg
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernel_times.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, "kernel_times.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "mesh_refine")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    if args and args[0] == "--summarize":
        summarize(args[1], out_dir, int(args[2]) if len(args) > 2 else 512)
    else:
        run(int(args[0]) if args else 512, out_dir)
