#!/usr/bin/env python3
"""The visible colour pass against the plain one on the sphere scene (carve, then the colour pass;
36 views of 640x480): the surface, the voxels visible somewhere, and the
time of the C-ABI calls arvx_color and arvx_color_visible (tolerance 3 voxel edges) in both modes,
each the median of 21 calls (every call ends in the pass's one synchronisation).

    python tools/color_visible_time.py [N ...]      (default 100 512; GPU required)

Kernel times per launch (vis_clear_kernel, vis_splat_kernel, vis_splat_large_kernel,
vis_vote_kernel): run it under rocprofv3 --kernel-trace --stats."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ar_voxel_project_amd import capi, synthetic  # noqa: E402

V = 36
REPS = 21


def call_ms(fn):
    fn()  # warm-up (buffers sized)
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    grids = [int(a) for a in sys.argv[1:]] or [100, 512]
    capi.load_library()
    for N in grids:
        sc = synthetic.sphere_scene(N, V, with_images=True)
        tol = np.float32(3.0) * sc.voxel_size
        with capi.Context(N, N, N, sc.voxel_size) as ctx:
            ctx.set_views(sc.M, sc.masks, campos=sc.campos)
            ctx.set_images(sc.images)
            ctx.carve()
            ctx.color_visible(capi.COLOR_AVERAGE, tol)
            views = ctx.surface_visible()
            t = {}
            for name, mode in (("closest", capi.COLOR_CLOSEST), ("average", capi.COLOR_AVERAGE)):
                t[name] = (call_ms(lambda: ctx.color(mode)),
                           call_ms(lambda: ctx.color_visible(mode, tol)))
        print(f"{N}^3, {V} views of 640x480: {len(views)} coloured voxels, {np.count_nonzero(views)} visible "
              f"somewhere, mean {views.mean():.2f} visible views per voxel")
        for name, (plain, visible) in t.items():
            print(f"  {name}: arvx_color {plain:.3f} ms | arvx_color_visible {visible:.3f} ms "
                  f"({visible / plain:.2f}x), median of {REPS}")


if __name__ == "__main__":
    main()
