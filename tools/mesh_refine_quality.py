#!/usr/bin/env python3
"""How far the vertices of the refined mesh (arvx_mc_mesh_refined) lie from the visual hull's surface,
by the number of bisections: the sphere scene with 16 views of 640x480 at N = 64 and N = 128.

    python tools/mesh_refine_quality.py [N ...]      (GPU required; default 64 128)

The truth is a device carve of the same views on a grid eight times finer and arvx_distance of it: a
fine voxel's signed distance to the boundary between occupied and empty fine voxels is
sign * (sqrt(|d|) - 1/2) fine voxels, sampled at a vertex by trilinear interpolation.  It is quantised
to a sixteenth of a voxel.  Prints, for the snapped vertices (the occupied ends: today's meshes), the
midpoints (0 bisections) and 1, 2, 4, 6 and 8 bisections, the rms and the largest distance in voxels, and
writes them to --out DIR/quality.txt and quality.json (default profiles/mesh_refine)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V = 16
FINE = 8
BISECTIONS = (0, 1, 2, 4, 6, 8)


def sample(field, p):
    """The truth at points p (n, 3) in fine voxel coordinates x y z: trilinear over the 8 fine voxels
    around each; field is the (Z, Y, X) int32 signed squared distance."""
    n = field.shape[0]
    p = np.clip(p.astype(np.float64), 0.0, n - 1.0)
    i0 = np.minimum(np.floor(p).astype(np.int64), n - 2)
    t = p - i0
    out = np.zeros(len(p))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                d = field[i0[:, 2] + dz, i0[:, 1] + dy, i0[:, 0] + dx].astype(np.float64)
                sd = np.sign(d) * (np.sqrt(np.abs(d)) - 0.5)
                w = ((t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) *
                     (t[:, 2] if dz else 1 - t[:, 2]))
                out += w * sd
    return out


def run(N, lines, result):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    sc = syn.sphere_scene(N, V)
    Nf = N * FINE
    with capi.Context(Nf, Nf, Nf, np.float32(sc.voxel_size / np.float32(FINE))) as ctx:
        ctx.set_views(sc.M, sc.masks)
        ctx.carve()
        field = ctx.distance().reshape(Nf, Nf, Nf)
    rows = {}
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        ctx.carve()
        for B in BISECTIONS:
            verts, _, _, edges, _ = ctx.mc_mesh_refined(B, details=True)
            if B == 0:
                d = sample(field, edges[:, :3].astype(np.float64) * FINE) / FINE
                rows["snapped"] = (float(np.sqrt((d * d).mean())), float(np.abs(d).max()))
                silhouette = float((edges[:, 3] < 8).mean())
            d = sample(field, verts.astype(np.float64) * FINE) / FINE
            rows[f"{B} bisections"] = (float(np.sqrt((d * d).mean())), float(np.abs(d).max()))
        fallbacks = int(ctx.stats()["host_total_fallbacks"])
    lines.append(f"{N}^3, {V} views of {sc.W}x{sc.H}, sphere scene; truth: carve at {Nf}^3 and arvx_distance; "
                 f"{len(verts)} cut edges, {100 * silhouette:.1f} % silhouette edges; host_total_fallbacks {fallbacks}")
    lines.append(f"  {'vertices':16s} {'rms (voxels)':>13s} {'max':>8s}")
    for k, (rms, mx) in rows.items():
        lines.append(f"  {k:16s} {rms:13.4f} {mx:8.4f}")
    result[str(N)] = {"cut_edges": int(len(verts)), "silhouette_share": silhouette,
                      "rows": {k: {"rms": r, "max": m} for k, (r, m) in rows.items()}}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "mesh_refine")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    lines, result = [], {"views": V, "fine": FINE}
    for N in [int(a) for a in args] or [64, 128]:
        run(N, lines, result)
    print("\n".join(lines))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "quality.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "quality.json"), "w") as f:
        json.dump(result, f, indent=1)
