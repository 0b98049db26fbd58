#!/usr/bin/env python3
"""Kernel times of the triangle render (arvx_render_mesh_view) beside the voxel render
(arvx_render_view) of the same carved model, and both renders' agreement with the masks: the sphere
scene with 36 views of 640x480, carved, its welded mesh and its refined mesh (4 bisections).

Run it under the profiler, then let it read the trace (GPU required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_render_mesh.py [N]
    python tools/profile_render_mesh.py --summarize OUT [N]

The first renders every view WARMUP + REPS times with each of the two calls (the refined mesh's
triangles, then the welded mesh's vertex voxels), prints the median host wall time of a pass over the
views and the mesh's counts and class counts, and writes host_times.json.  The second prints, per
call, the median over the views and repetitions of the summed kernel time and of each kernel, and
writes kernel_times.json and kernel_times.txt.

    python tools/profile_render_mesh.py --agreement N [N ...]

prints and writes (agreement.json, agreement.txt), per grid size, the agreement counts summed over
the views of the voxel render and of the triangle renders of the welded and the refined mesh.
All write into --out DIR (default profiles/render_mesh)."""
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
B = 4
WARMUP = 1
REPS = 5
FIRST_KERNEL = "render_clear_kernel"  # every render starts with it
LEGS = ("arvx_render_mesh_view REFINED", "arvx_render_view")


def carved(N, with_meshes=True):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    capi.load_library()
    sc = syn.sphere_scene(N, V)
    ctx = capi.Context(N, N, N, sc.voxel_size)
    ctx.set_views(sc.M, sc.masks)
    ctx.carve()
    counts = {}
    if with_meshes:
        counts["welded"] = ctx.mc_mesh_welded_count(False)
        counts["refined"] = ctx.mc_mesh_refined_count(B)
    ctx.synchronize()
    return capi, sc, ctx, counts


def run(N, out_dir):
    capi, sc, ctx, counts = carved(N)
    result = {"N": N, "views": V, "image": [int(sc.W), int(sc.H)], "bisections": B, "warmup": WARMUP, "reps": REPS,
              "welded": counts["welded"], "refined": counts["refined"], "legs": {}}
    print(f"{N}^3, {V} views of {sc.W}x{sc.H}, sphere scene: welded mesh {counts['welded']}, refined mesh (B = {B}) "
          f"{counts['refined']} (vertices, triangles); host wall time of a pass over the views, median of {REPS}:")
    with ctx:
        legs = ((LEGS[0], lambda v: ctx.render_mesh_view(capi.MESH_REFINED, v, download=False)),
                (LEGS[1], lambda v: ctx.render_view(v, download=False)))
        for name, fn in legs:
            t = []
            for _ in range(WARMUP + REPS):
                ctx.synchronize()
                t0 = time.perf_counter()
                for v in range(V):
                    fn(v)
                ctx.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            ms = float(np.median(t[WARMUP:]))
            print(f"  {name:32s} {ms:8.3f} ms ({ms / V:.3f} ms per view)")
            result["legs"][name] = {"host_ms_per_pass_median": ms, "host_ms_per_view": ms / V}
        ctx.render_mesh_view(capi.MESH_REFINED, 0, download=False)
        result["classes_view0"] = dict(zip(("drawn", "empty", "flat", "refused"), ctx.render_mesh_stats()))
        print(f"  classes of view 0: {result['classes_view0']}")
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
    # (the last call of the run is the one whose class counts were read: not part of a leg)
    per = (WARMUP + REPS) * V
    if len(calls) < 2 * per:
        sys.exit(f"{len(calls)} renders in the trace, expected at least {2 * per}")
    out = {"N": N, "views": V, "legs": {}}
    lines = [f"kernel time per render from {len(traces)} trace file(s), {N}^3: median over {V} views x {REPS} passes "
             f"(after {WARMUP} warm-up pass(es))"]
    for li, name in enumerate(LEGS):
        cs = calls[li * per + WARMUP * V:(li + 1) * per]
        mesh = any(k.startswith("render_mesh") for k, _ in cs[0])
        if mesh != (li == 0):
            sys.exit(f"leg {name}: the trace's renders are not in the run's order")
        tot = [sum(d for _, d in c) for c in cs]
        kernels = []
        for k, _ in cs[0]:
            if k not in kernels:
                kernels.append(k)
        parts = {k: float(np.median([sum(d for n, d in c if n == k) for c in cs])) / 1e3 for k in kernels}
        out["legs"][name] = {"kernels_us_median": float(np.median(tot)) / 1e3, "kernels_us_min": min(tot) / 1e3,
                             "kernels_us_max": max(tot) / 1e3, "launches": len(cs[0]), "per_kernel_us": parts}
        lines.append(f"  {name:32s} {np.median(tot) / 1e3:9.1f} us   (min {min(tot) / 1e3:.1f}, max {max(tot) / 1e3:.1f}; "
                     f"{len(cs[0])} launches)")
        for k, us in parts.items():
            lines.append(f"      {k:36s} {us:9.1f} us")
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernel_times.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, "kernel_times.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def agreement(grids, out_dir):
    out, lines = {}, []
    for N in grids:
        capi, sc, ctx, counts = carved(N)
        with ctx:
            legs = {"voxel render (welded vertex voxels)": lambda v: ctx.render_agreement(v),
                    "triangles, welded mesh": lambda v: ctx.render_mesh_agreement(capi.MESH_WELDED, v),
                    f"triangles, refined mesh (B = {B})": lambda v: ctx.render_mesh_agreement(capi.MESH_REFINED, v)}
            fg = int(sum(np.count_nonzero(m) for m in sc.masks))
            lines.append(f"{N}^3, {V} views of {sc.W}x{sc.H}, sphere scene; {fg} foreground pixels over the views; "
                         f"welded {counts['welded']}, refined {counts['refined']} (vertices, triangles)")
            out[str(N)] = {"foreground": fg, "welded": counts["welded"], "refined": counts["refined"], "legs": {}}
            for name, fn in legs.items():
                c = np.sum([fn(v) for v in range(V)], axis=0)
                out[str(N)]["legs"][name] = {"both": int(c[0]), "model_only": int(c[1]), "mask_only": int(c[2])}
                lines.append(f"  {name:40s} both {c[0]:9d}   model only {c[1]:8d}   mask only {c[2]:8d}")
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "agreement.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, "agreement.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "render_mesh")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    if args and args[0] == "--summarize":
        summarize(args[1], out_dir, int(args[2]) if len(args) > 2 else 512)
    elif args and args[0] == "--agreement":
        agreement([int(a) for a in args[1:]] or [128, 512], out_dir)
    else:
        run(int(args[0]) if args else 512, out_dir)
