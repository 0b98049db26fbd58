#!/usr/bin/env python3
"""Kernel times of the triangle render with and without a near plane (arvx_ctx_set_render_near): the
sphere scene with 36 views of 640x480, carved, its refined mesh (4 bisections), drawn
  outside      from every view of the ring, no plane (the leg of tools/profile_render_mesh.py)
  inside off   from a camera inside the sphere, close under its surface, no plane
  inside on    from the same camera with the plane at 0.01

Run it under the profiler, then let it read the trace (GPU required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_render_mesh_clip.py [N]
    python tools/profile_render_mesh_clip.py --summarize OUT [N] [--label NAME]

The first renders each leg (WARMUP + REPS) * 36 times and writes host_times.json with the inside
view's class counts, clip counts and covered pixels.  The second prints, per leg, the median over the
renders of the summed kernel time and of each kernel, and writes kernel_times[_NAME].json / .txt.
With ARVX_LIB_PATH naming a build without the plane, the third leg is left out: the first two then
time that build.  All write into --out DIR (default profiles/render_mesh_clip)."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V = 36
B = 4
WARMUP = 1
REPS = 5
NEAR = 0.01
FIRST_KERNEL = "render_clear_kernel"  # every render starts with it
LEGS = ("outside", "inside off", "inside on")


def inside_camera(syn, W, H):
    """A camera 0.17 from the sphere's centre (its radius is 0.185), looking along the surface."""
    K = syn.K_DATASET.copy()
    K[0] *= W / syn.IMAGE_W
    K[1] *= H / syn.IMAGE_H
    K32 = K.astype(np.float32)
    centre = np.array([0.256, 0.256, -0.256])
    d = np.array([1, 0.3, 0.2], float)
    d /= np.linalg.norm(d)
    cam = centre + 0.17 * d
    side = np.cross(d, [0.1, 0.2, 1.0])
    side /= np.linalg.norm(side)
    Rt32 = syn.look_at_rt(cam, cam + side + 0.3 * d, d)[None].astype(np.float32)
    return syn.compose_m(K32, Rt32)[0]


def run(N, out_dir):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    lib = capi.load_library()
    has_plane = hasattr(lib, "arvx_ctx_set_render_near")
    sc = syn.sphere_scene(N, V)
    W, H = int(sc.W), int(sc.H)
    M = inside_camera(syn, W, H)
    result = {"N": N, "views": V, "image": [W, H], "bisections": B, "warmup": WARMUP, "reps": REPS, "near": NEAR,
              "plane": has_plane, "legs": [name for name in LEGS if has_plane or name != "inside on"]}
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        ctx.carve()
        result["refined"] = ctx.mc_mesh_refined_count(B)
        ctx.synchronize()
        for _ in range(WARMUP + REPS):
            for v in range(V):
                ctx.render_mesh_view(capi.MESH_REFINED, v, download=False)
        ctx.synchronize()
        for _ in range((WARMUP + REPS) * V):
            ctx.render_mesh(capi.MESH_REFINED, M, W, H, download=False)
        ctx.synchronize()
        _, _, ids = ctx.render_download()
        result["inside off"] = {"classes": ctx.render_mesh_stats(), "covered": int(np.count_nonzero(ids >= 0))}
        if has_plane:
            ctx.set_render_near(NEAR)
            for _ in range((WARMUP + REPS) * V):
                ctx.render_mesh(capi.MESH_REFINED, M, W, H, download=False)
            ctx.synchronize()
            _, _, ids = ctx.render_download()
            result["inside on"] = {"classes": ctx.render_mesh_stats(), "clip": ctx.render_mesh_clip_stats(),
                                   "covered": int(np.count_nonzero(ids >= 0))}
        result["host_total_fallbacks"] = int(ctx.stats()["host_total_fallbacks"])
    print(json.dumps(result))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "host_times.json"), "w") as f:
        json.dump(result, f, indent=1)


def summarize(trace_dir, out_dir, N, label):
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
    per = (WARMUP + REPS) * V
    legs = LEGS[:len(calls) // per]
    if len(legs) < 2:
        sys.exit(f"{len(calls)} renders in the trace, expected at least {2 * per}")
    out = {"N": N, "views": V, "label": label, "legs": {}}
    lines = [f"kernel time per render from {len(traces)} trace file(s), {N}^3{' (' + label + ')' if label else ''}: "
             f"median over {REPS * V} renders (after {WARMUP * V} warm-up renders)"]
    for li, name in enumerate(legs):
        cs = calls[li * per + WARMUP * V:(li + 1) * per]
        clipped = any("clip" in k for k, _ in cs[0])
        if clipped != (name == "inside on"):
            sys.exit(f"leg {name}: the trace's renders are not in the run's order")
        tot = [sum(d for _, d in c) for c in cs]
        kernels = []
        for k, _ in cs[0]:
            if k not in kernels:
                kernels.append(k)
        parts = {k: float(np.median([sum(d for n, d in c if n == k) for c in cs])) / 1e3 for k in kernels}
        out["legs"][name] = {"kernels_us_median": float(np.median(tot)) / 1e3, "kernels_us_min": min(tot) / 1e3,
                             "kernels_us_max": max(tot) / 1e3, "launches": len(cs[0]), "per_kernel_us": parts}
        lines.append(f"  {name:12s} {np.median(tot) / 1e3:9.1f} us   (min {min(tot) / 1e3:.1f}, max {max(tot) / 1e3:.1f}; "
                     f"{len(cs[0])} launches)")
        for k, us in parts.items():
            lines.append(f"      {k:36s} {us:9.1f} us")
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    stem = "kernel_times" + ("_" + label if label else "")
    with open(os.path.join(out_dir, stem + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, stem + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "render_mesh_clip")
    label = ""
    for flag in ("--out", "--label"):
        if flag in args:
            k = args.index(flag)
            if flag == "--out":
                out_dir = args[k + 1]
            else:
                label = args[k + 1]
            del args[k:k + 2]
    if args and args[0] == "--summarize":
        summarize(args[1], out_dir, int(args[2]) if len(args) > 2 else 512, label)
    else:
        run(int(args[0]) if args else 512, out_dir)
