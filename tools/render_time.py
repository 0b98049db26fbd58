#!/usr/bin/env python3
"""The render of the welded mesh against the visible colour pass's depth-buffer splat on the sphere
scene (carve, visible colour, welded mesh; 36 views of 640x480, tolerance 3 voxel edges): the time
of the C-ABI calls arvx_render_view + arvx_render_download's synchronisation (no copy),
arvx_render_agreement and arvx_color_visible, each the median of 11 calls.

    python tools/render_time.py [N ...]      (default 512; GPU required)

Kernel times per launch (render_clear / _splat / _splat_large / _resolve / _agreement and the
vis_clear / vis_splat / vis_splat_large kernels of the 36 depth buffers): run it under
rocprofv3 --kernel-trace --stats."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ar_voxel_project_amd import capi, synthetic  # noqa: E402

V = 36
REPS = 11


def call_ms(ctx, fn):
    t = []
    for _ in range(REPS + 1):  # (the first sizes the buffers)
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[1:]))


def main():
    grids = [int(a) for a in sys.argv[1:]] or [512]
    capi.load_library()
    for N in grids:
        sc = synthetic.sphere_scene(N, V, with_images=True)
        tol = np.float32(3.0) * sc.voxel_size
        with capi.Context(N, N, N, sc.voxel_size) as ctx:
            ctx.set_views(sc.M, sc.masks, campos=sc.campos)
            ctx.set_images(sc.images)
            ctx.carve()
            vis = call_ms(ctx, lambda: ctx.color_visible(capi.COLOR_AVERAGE, tol))
            nv, nt = ctx.mc_mesh_welded_count(False)
            one = call_ms(ctx, lambda: ctx.render_view(0, download=False))
            allv = call_ms(ctx, lambda: [ctx.render_view(v, download=False) for v in range(V)])
            agree = call_ms(ctx, lambda: ctx.render_agreement(0))
            counts = [ctx.render_agreement(v) for v in range(V)]
        print(f"{N}^3, {V} views of 640x480: {nv} vertex voxels, {nt} triangles")
        print(f"  arvx_render_view: one view {one:.3f} ms | all {V} views {allv:.3f} ms "
              f"({allv / V:.3f} ms per view) | arvx_render_agreement {agree:.3f} ms | "
              f"arvx_color_visible {vis:.3f} ms, median of {REPS}")
        both, model_only, mask_only = (sum(c[k] for c in counts) for k in range(3))
        print(f"  agreement over the views: both {both}, model only {model_only}, mask only {mask_only}")


if __name__ == "__main__":
    main()
