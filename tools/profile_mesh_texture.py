#!/usr/bin/env python3
"""Kernel times of the mesh textures from the images (arvx_mesh_texture) beside arvx_mesh_color of the
same mesh, in one run on one device: the sphere scene with 36 views of 640x480 and their images, carved;
its refined mesh (4 bisections) textured at R = 2 and its decimated mesh (C = 4) textured at R = 14, each
into an atlas 4096 texels wide; tolerance 3 voxel edges.

Run it under the profiler -- one kernel trace, no counters --, then let it read the trace (GPU
required for the first command):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/profile_mesh_texture.py [N]
    python tools/profile_mesh_texture.py --summarize OUT [N]

The first runs WARMUP + REPS times each of: arvx_mesh_texture and arvx_mesh_color (AVERAGE) of the refined
mesh, then the same two of the decimated mesh.  After every one of them it downloads a depth buffer of
the mesh colours' product, whose kernel (mesh_color_depth_kernel) marks the end of the segment in the
trace.  It prints the host wall times and writes host_times.json.  The second prints, per leg, the median
over the repetitions of the summed kernel time and of each kernel, the texture calls split into depth
pass, selection and fill, and the fill kernel's bytes per second -- the atlas written plus the face
records, the faces' views, the positions and the colours read once -- against the 6.29 TB/s a float4 copy
reaches on this device (8.0 TB/s is the HBM's specification); it writes kernel_times.json and
kernel_times.txt.

    python tools/profile_mesh_texture.py --quality N [N ...]

prints and writes (quality.json, quality.txt), per grid size and for both meshes, the mean absolute
difference per channel between the photographs of synthetic.textured_sphere_scene -- which agree with
each other -- and the mesh drawn into their views with (a) the voxel colours of arvx_color_visible, (b)
the image vertex colours of arvx_mesh_color and (c) the texture, over the pixels that are foreground in
the mask and covered by the mesh.
All write into --out DIR (default profiles/mesh_texture)."""
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
CELL = 4
R_REFINED, R_DECIMATED = 2, 14
ATLAS_WIDTH = 4096
TOL_VOXELS = 3.0
PERIOD = 0.25
WARMUP = 1
REPS = 5
MARKER = "mesh_color_depth_kernel"
LEGS = (f"arvx_mesh_texture REFINED R={R_REFINED}", "arvx_mesh_color REFINED",
        f"arvx_mesh_texture DECIMATED R={R_DECIMATED}", "arvx_mesh_color DECIMATED")
DEPTH_PASS = ("mesh_color_project_kernel", "mesh_color_raster_kernel", "mesh_color_large_kernel")
SELECTION = ("mesh_texture_visible_kernel", "mesh_texture_select_kernel")
FILL = "mesh_texture_fill_kernel"
COPY_RATE = 6.29e12  # bytes per second of a float4 copy on an MI355X


def carved(N, textured=False):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    capi.load_library()
    sc = syn.textured_sphere_scene(N, V, period=PERIOD) if textured else syn.sphere_scene(N, V, with_images=True)
    ctx = capi.Context(N, N, N, sc.voxel_size)
    ctx.set_views(sc.M, sc.masks, campos=sc.campos)
    ctx.set_images(sc.images)
    ctx.carve()
    ctx.synchronize()
    return capi, sc, ctx


def meshes(capi, ctx):
    """The refined and the decimated mesh on the device: {name: (source, R, vertices, triangles)}."""
    rv, rt = ctx.mc_mesh_refined_count(B)
    ctx.mc_mesh_welded(False)
    dv, dt = ctx.mc_mesh_decimate(CELL, download=False)
    return {"REFINED": (capi.MESH_REFINED, R_REFINED, rv, rt), "DECIMATED": (capi.MESH_DECIMATED, R_DECIMATED, dv, dt)}


def fill_bytes(nv, nt, AW, AH):
    """What the fill kernel writes and reads once: the atlas; 24 bytes of record and 4 of view per face; 12
    bytes of position and 12 of colour per vertex."""
    return 3 * AW * AH + 28 * nt + 24 * nv


def run(N, out_dir):
    capi, sc, ctx = carved(N)
    tol = float(np.float32(TOL_VOXELS) * sc.voxel_size)
    with ctx:
        ms = meshes(capi, ctx)
        result = {"N": N, "views": V, "image": [int(sc.W), int(sc.H)], "bisections": B, "cell": CELL,
                  "atlas_width": ATLAS_WIDTH, "tolerance_voxels": TOL_VOXELS, "warmup": WARMUP, "reps": REPS,
                  "meshes": {}, "legs": {}}
        legs = []
        for name, (src, R, nv, nt) in ms.items():
            counts = ctx.mesh_texture(src, R, ATLAS_WIDTH, tol, download=False)
            result["meshes"][name] = {"vertices": nv, "triangles": nt, "resolution": R, "textured": counts[1],
                                      "atlas": [counts[2], counts[3]], "texels_per_face": (R + 2) * (R + 3) // 2,
                                      "fill_bytes": fill_bytes(nv, nt, counts[2], counts[3])}
            print(f"{N}^3, {V} views of {sc.W}x{sc.H}, sphere scene: {name} mesh {nv} vertices, {nt} triangles, R = {R}: "
                  f"atlas {counts[2]} x {counts[3]}, {counts[1]} faces textured")
            legs.append((f"arvx_mesh_texture {name} R={R}",
                         lambda src=src, R=R: ctx.mesh_texture(src, R, ATLAS_WIDTH, tol, download=False)))
            legs.append((f"arvx_mesh_color {name}",
                         lambda src=src: ctx.mesh_color(src, capi.COLOR_AVERAGE, tol, download=False)))
        assert tuple(n for n, _ in legs) == LEGS
        legs[1][1]()  # (the product whose depth download marks the segments)
        ctx.mesh_color_depth(0)
        for name, fn in legs:
            t = []
            for _ in range(WARMUP + REPS):
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
                ctx.mesh_color_depth(0)  # (the colours' product: a texture call keeps it)
            med = float(np.median(t[WARMUP:]))
            print(f"  {name:40s} {med:8.3f} ms host wall time, median of {REPS}")
            result["legs"][name] = {"host_ms_median": med}
        result["host_total_fallbacks"] = int(ctx.stats()["host_total_fallbacks"])
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "host_times.json"), "w") as f:
        json.dump(result, f, indent=1)


def summarize(trace_dir, out_dir, N):
    traces = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    host = {}
    if os.path.exists(os.path.join(out_dir, "host_times.json")):
        host = json.load(open(os.path.join(out_dir, "host_times.json"))).get("meshes", {})
    rows = []
    for path in traces:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()

    def short(name):
        return name.split("(")[0].split("<")[0].replace("arvx::", "").replace("void ", "").strip()

    segments, cur = [], []
    for start, end, name in rows:
        if MARKER in name:
            segments.append(cur)
            cur = []
        else:
            cur.append((short(name), end - start))
    per = WARMUP + REPS
    if len(segments) != 1 + len(LEGS) * per:
        sys.exit(f"{len(segments)} segments in the trace, expected {1 + len(LEGS) * per}")
    segments = segments[1:]  # (the first holds the set-up and the product the markers read)
    out = {"N": N, "views": V, "legs": {}}
    lines = [f"kernel time per call from {len(traces)} trace file(s), {N}^3: median over {REPS} repetitions "
             f"(after {WARMUP} warm-up)"]
    for li, name in enumerate(LEGS):
        cs = segments[li * per + WARMUP:(li + 1) * per]
        tot = [sum(d for _, d in c) for c in cs]
        kernels = []
        for k, _ in cs[0]:
            if k not in kernels:
                kernels.append(k)
        parts = {k: float(np.median([sum(d for n, d in c if n == k) for c in cs])) / 1e3 for k in kernels}
        leg = {"kernels_us_median": float(np.median(tot)) / 1e3, "kernels_us_min": min(tot) / 1e3,
               "kernels_us_max": max(tot) / 1e3, "launches": len(cs[0]), "per_kernel_us": parts}
        lines.append(f"  {name:40s} {np.median(tot) / 1e3:9.1f} us   (min {min(tot) / 1e3:.1f}, max {max(tot) / 1e3:.1f}; "
                     f"{len(cs[0])} launches)")
        for k, us in parts.items():
            lines.append(f"      {k:36s} {us:9.1f} us")
        leg["depth_pass_us"] = float(np.median([sum(d for n, d in c if n in DEPTH_PASS) for c in cs])) / 1e3
        if "texture" in name:
            leg["selection_us"] = float(np.median([sum(d for n, d in c if n in SELECTION) for c in cs])) / 1e3
            leg["fill_us"] = parts.get(FILL, 0.0)
            lines.append(f"      depth pass {leg['depth_pass_us']:9.1f} us; selection (visible, select) "
                         f"{leg['selection_us']:9.1f} us; fill {leg['fill_us']:9.1f} us")
            mesh = host.get(name.split()[1])
            if mesh and leg["fill_us"] > 0:
                rate = mesh["fill_bytes"] / (leg["fill_us"] * 1e-6)
                leg.update(fill_bytes=mesh["fill_bytes"], fill_bytes_per_s=rate, fill_share_of_copy_rate=rate / COPY_RATE)
                lines.append(f"      fill: {mesh['fill_bytes']} bytes, {rate / 1e12:.3f} TB/s, {100 * rate / COPY_RATE:.1f} % "
                             f"of a float4 copy's {COPY_RATE / 1e12:.2f} TB/s")
        else:
            leg["vote_us"] = parts.get("mesh_color_vote_kernel", 0.0)
            lines.append(f"      depth pass {leg['depth_pass_us']:9.1f} us; vote {leg['vote_us']:9.1f} us")
        out["legs"][name] = leg
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "kernel_times.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, "kernel_times.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def quality(grids, out_dir):
    out, lines = {}, []
    for N in grids:
        capi, sc, ctx = carved(N, textured=True)
        tol = float(np.float32(TOL_VOXELS) * sc.voxel_size)
        with ctx:
            ctx.color_visible(capi.COLOR_AVERAGE, tol)
            ms = meshes(capi, ctx)

            def mad(source):
                total, pixels = 0, 0
                for v in range(V):
                    bgr, _, ids = ctx.render_mesh_view(source, v)
                    pick = (sc.masks[v] != 0) & (ids >= 0)
                    total += int(np.abs(bgr[pick].astype(np.int64) - sc.images[v][pick].astype(np.int64)).sum())
                    pixels += int(np.count_nonzero(pick))
                return total / (3.0 * max(pixels, 1)), pixels

            out[str(N)] = {}
            for name, (src, R, nv, nt) in ms.items():
                legs = {"voxel colours (arvx_color_visible)": mad(src)}
                _, views, coloured = ctx.mesh_color(src, capi.COLOR_AVERAGE, tol)
                legs["image vertex colours (arvx_mesh_color)"] = mad(src | capi.MESH_IMAGE_COLORS) + (f"{coloured} vertices coloured",)
                counts = ctx.mesh_texture(src, R, ATLAS_WIDTH, tol, download=False)
                legs[f"texture, R = {R}"] = mad(src | capi.MESH_TEXTURED) + (f"{counts[1]} faces textured, atlas {counts[2]} x {counts[3]}",)
                lines.append(f"{N}^3, {V} views of {sc.W}x{sc.H}, textured sphere (period {PERIOD}), {name} mesh {nv} vertices, "
                             f"{nt} triangles; tolerance {TOL_VOXELS} voxel edges; mean absolute difference per channel to "
                             f"the photographs over {legs[f'texture, R = {R}'][1]} foreground pixels the mesh covers")
                out[str(N)][name] = {"vertices": nv, "triangles": nt, "legs": {}}
                for leg, r in legs.items():
                    out[str(N)][name]["legs"][leg] = {"mean_abs_diff": r[0], "pixels": r[1]}
                    lines.append(f"  {leg:44s} {r[0]:8.3f}" + (f"   ({r[2]})" if len(r) > 2 else ""))
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "quality.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(out_dir, "quality.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "mesh_texture")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    if args and args[0] == "--summarize":
        summarize(args[1], out_dir, int(args[2]) if len(args) > 2 else 512)
    elif args and args[0] == "--quality":
        quality([int(a) for a in args[1:]] or [128, 512], out_dir)
    else:
        run(int(args[0]) if args else 512, out_dir)
