#!/usr/bin/env python3
"""What an opening does to a carved model with spurs (arvx_morph ARVX_MORPH_OPEN, then
arvx_components_keep ARVX_COMPONENTS_LARGEST): the sphere scene, and the same scene with a rod sticking
out of the sphere and a thin bridge from the sphere to a small ball OR-ed into its masks.  The rod and
the bridge are chains of small spheres, ROD_RADIUS and BRIDGE_RADIUS voxel edges thick.

    python tools/morph_quality.py [N] [radius_voxels]      (GPU required; default 128, 2.5)

Prints, for the carve of the spurred masks as it is, after the opening, after the keep alone and after
the opening and the keep: the voxels of the clean model (the carve of the plain sphere scene) that are
still there, and the voxels outside the clean model -- the spurs -- that are left; and writes them to
--out DIR/morph_quality.json (default profiles/distance)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

V = 16
ROD_RADIUS = 1.0     # voxel edges
BRIDGE_RADIUS = 0.75
BALL_RADIUS = 5.0


def chain(K, Rt, a, b, radius, W, H, step):
    """Masks of the spheres of `radius` strung from a to b, `step` apart."""
    from ar_voxel_project_amd import synthetic as syn
    n = max(2, int(np.ceil(np.linalg.norm(b - a) / step)) + 1)
    out = np.zeros((Rt.shape[0], H, W), np.uint8)
    for t in np.linspace(0.0, 1.0, n):
        out |= syn.sphere_masks(K, Rt, a + t * (b - a), radius, W, H)
    return out


def run(N, radius_voxels, out_dir):
    from ar_voxel_project_amd import capi
    from ar_voxel_project_amd import synthetic as syn
    capi.load_library()
    sc = syn.sphere_scene(N, V)
    _, c = syn.ring_cameras(V)
    E, s = syn.EXTENT, float(sc.voxel_size)
    R = 0.35 * E  # the sphere's radius (synthetic.sphere_scene)
    ux, uy = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    spurs = chain(sc.K, sc.Rt, c + ux * R * 0.9, c + ux * (R + 0.1 * E), ROD_RADIUS * s, sc.W, sc.H, s)
    ball = c - uy * (R + 0.09 * E)
    spurs |= chain(sc.K, sc.Rt, c - uy * R * 0.9, ball, BRIDGE_RADIUS * s, sc.W, sc.H, s)
    spurs |= syn.sphere_masks(sc.K, sc.Rt, ball, BALL_RADIUS * s, sc.W, sc.H)
    radius_sq = int(np.floor(radius_voxels * radius_voxels))
    with capi.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks)
        ctx.carve()
        clean = (ctx.download_state().reshape(-1) & 1).astype(bool)
        ctx.set_views(sc.M, sc.masks | spurs)
        rows = {}

        def carve():
            ctx.reset()
            ctx.carve()

        def report(name):
            occ = (ctx.download_state().reshape(-1) & 1).astype(bool)
            rows[name] = {"clean_kept": int((occ & clean).sum()), "spur_left": int((occ & ~clean).sum()),
                          "components": int(len(ctx.components(6)[0]))}

        carve()
        report("carved")
        carve()
        ctx.keep_components(largest=True)
        report("largest alone")
        carve()
        removed, added = ctx.morph(capi.MORPH_OPEN, radius_sq)
        report("opened")
        ctx.keep_components(largest=True)
        report("opened, then largest")
    print(f"{N}^3, {V} views, sphere with a rod ({ROD_RADIUS} voxels thick), a bridge ({BRIDGE_RADIUS}) and a ball "
          f"({BALL_RADIUS}); opening by radius {radius_voxels} voxels (radius_sq {radius_sq}); clean model: "
          f"{int(clean.sum())} voxels")
    for name, r in rows.items():
        print(f"  {name:22s} clean kept {r['clean_kept']:9d} ({100.0 * r['clean_kept'] / clean.sum():6.2f} %)   "
              f"spur left {r['spur_left']:6d}   components {r['components']}")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "morph_quality.json"), "w") as f:
        json.dump({"N": N, "views": V, "radius_voxels": radius_voxels, "radius_sq": radius_sq,
                   "clean_voxels": int(clean.sum()), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "distance")
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    run(int(args[0]) if args else 128, float(args[1]) if len(args) > 1 else 2.5, out_dir)
