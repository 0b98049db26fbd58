#!/usr/bin/env python3
"""arvx_mesh_relax on the sphere scene's carved model (36 views of 640x480): the general adjacency beside
the welded smoother's lattice adjacency, on the same welded mesh, and on the refined mesh, which only
arvx_mesh_relax can smooth.  Every time is a host clock around calls that end in a synchronisation
(a download with no array), the median of REPS after a warm-up; the two sides of a comparison are
taken in turns in one loop.

    python tools/mesh_relax_time.py [N ...]      (default 512; GPU required)

  welded mesh    arvx_mc_mesh_welded alone; + the first arvx_mc_mesh_smooth(10) | + the first
                 arvx_mesh_relax(WELDED, 10) (each builds its CSRs: the difference to the first figure
                 is the build and one cached call); then the cached calls at 10 iterations, in turns
  refined mesh   arvx_mc_mesh_refined(B = 6) alone; + the first arvx_mesh_relax(REFINED, 10); the cached
                 call at 0 and 10 iterations
  positions of the two welded paths are compared bit for bit on the way.

Kernel times per launch: run it under rocprofv3 --kernel-trace --stats."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ar_voxel_project_amd import capi, synthetic  # noqa: E402

V = 36
REPS = 21


def in_turns(*fns):
    """The median time (ms) of each of fns, called in turns REPS times after one warm-up round."""
    for fn in fns:
        fn()
    t = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(a)) for a in t], [float(np.percentile(a, 90) - np.percentile(a, 10)) for a in t]


def main():
    grids = [int(a) for a in sys.argv[1:]] or [512]
    capi.load_library()
    for N in grids:
        sc = synthetic.sphere_scene(N, V)
        with capi.Context(N, N, N, sc.voxel_size) as ctx:
            ctx.set_views(sc.M, sc.masks)
            ctx.carve()

            def smooth(it):
                ctx.mc_mesh_smooth(it, download=False)
                ctx.mc_mesh_smooth_download(verts=False, normals=False)  # (the synchronisation)

            def relax(source, it):
                ctx.mesh_relax(source, it, download=False)
                ctx.mesh_relax_download(verts=False, normals=False, degree=False)  # (the synchronisation)

            nv, nt = ctx.mc_mesh_welded_count()
            (t_weld, t_ws, t_wr), (s_weld, s_ws, s_wr) = in_turns(
                lambda: ctx.mc_mesh_welded_count(),
                lambda: (ctx.mc_mesh_welded_count(), smooth(10)),
                lambda: (ctx.mc_mesh_welded_count(), relax(capi.MESH_WELDED, 10)))
            ctx.mc_mesh_welded_count()
            (t_s10, t_r10), (s_s10, s_r10) = in_turns(lambda: smooth(10), lambda: relax(capi.MESH_WELDED, 10))
            a = ctx.mc_mesh_smooth_download()
            b = ctx.mesh_relax_download()
            equal = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b[:2]))
            print(f"{N}^3 welded mesh: V = {nv}  T = {nt}   (median of {REPS}, in turns; +- : the 10-90 % spread)")
            print(f"  arvx_mc_mesh_welded {t_weld:.3f} ms +- {s_weld:.3f} | + first arvx_mc_mesh_smooth(10) {t_ws:.3f} ms "
                  f"+- {s_ws:.3f} | + first arvx_mesh_relax(WELDED, 10) {t_wr:.3f} ms +- {s_wr:.3f}")
            print(f"  cached CSRs, 10 iterations: arvx_mc_mesh_smooth {t_s10:.3f} ms +- {s_s10:.3f} | arvx_mesh_relax "
                  f"{t_r10:.3f} ms +- {s_r10:.3f}   positions and normals bit-equal: {equal}")
            rv, rt = ctx.mc_mesh_refined_count(6)
            (t_ref, t_rr), (s_ref, s_rr) = in_turns(
                lambda: ctx.mc_mesh_refined_count(6),
                lambda: (ctx.mc_mesh_refined_count(6), relax(capi.MESH_REFINED, 10)))
            ctx.mc_mesh_refined_count(6)
            (t_0, t_10), (s_0, s_10) = in_turns(lambda: relax(capi.MESH_REFINED, 0), lambda: relax(capi.MESH_REFINED, 10))
            deg = ctx.mesh_relax_download(verts=False, normals=False)[2]
            print(f"{N}^3 refined mesh (B = 6): V = {rv}  T = {rt}   largest valence {int(deg.max())}")
            print(f"  arvx_mc_mesh_refined {t_ref:.3f} ms +- {s_ref:.3f} | + first arvx_mesh_relax(REFINED, 10) {t_rr:.3f} ms "
                  f"+- {s_rr:.3f}")
            print(f"  cached CSRs: 0 iterations {t_0:.3f} ms +- {s_0:.3f} | 10: {t_10:.3f} ms +- {s_10:.3f}  (per iteration "
                  f"{(t_10 - t_0) / 10:.4f} ms)")
            print(f"  host_total_fallbacks {ctx.stats()['host_total_fallbacks']}")


if __name__ == "__main__":
    main()
