#!/usr/bin/env python3
"""The welded marching-cubes mesh against the reference's mesh on the sphere pipeline (carve,
average colour, handleUnseen, closure; 36 views of 640x480): V and T, the time of the C-ABI call
(arvx_mc_mesh_welded against arvx_mc_mesh: all kernels of the call and its one synchronisation,
no download), and the drop-in time with the mesh on the host (marchingCubesMeshWelded against
marchingCubesMesh, tools/cpp/arvx_mesh_weld_time).

    python tools/mesh_weld_time.py [N ...]      (default 100 512; GPU required)

Kernel times per launch: run it under rocprofv3 --kernel-trace --stats."""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ar_voxel_project_amd import capi, synthetic  # noqa: E402
from tests.test_cpp_host import write_scene  # noqa: E402

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
    sc64 = synthetic.sphere_scene(64, V, with_images=True)
    with tempfile.TemporaryDirectory() as d:
        scene = os.path.join(d, "scene.bin")
        masks3 = np.repeat(sc64.masks[..., None], 3, axis=-1)
        write_scene(scene, 1, 1, 1, 1.0, sc64.K, sc64.Rt, masks3, sc64.images, np.ones(1, np.uint8))
        for N in grids:
            sc = synthetic.sphere_scene(N, V, with_images=True)
            with capi.Context(N, N, N, sc.voxel_size) as ctx:
                ctx.set_views(sc.M, sc.masks, campos=sc.campos)
                ctx.set_images(sc.images)
                ctx.carve()
                ctx.color(capi.COLOR_AVERAGE)
                ctx.handle_unseen()
                ctx.closure(3, True, download=False)
                T = ctx.mc_mesh_count(True)
                nv, tw = ctx.mc_mesh_welded_count(True)
                assert tw == T
                t_mesh = call_ms(lambda: ctx.mc_mesh_count(True))
                t_weld = call_ms(lambda: ctx.mc_mesh_welded_count(True))
            print(f"{N}^3: V = {nv}  T = {T}  (V / 3T = {nv / max(1, 3 * T):.3f}; hand-off "
                  f"{(12 * nv + 24 * T) / 1e6:.1f} MB welded against {60 * T / 1e6:.1f} MB)")
            print(f"  C-ABI call, median of {REPS}: arvx_mc_mesh {t_mesh:.3f} ms | "
                  f"arvx_mc_mesh_welded {t_weld:.3f} ms")
            r = subprocess.run([os.path.join(ROOT, "tools", "cpp", "arvx_mesh_weld_time"), scene,
                                str(N), str(N), str(N), repr(float(sc.voxel_size)), "9"],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stderr + r.stdout)
            print("  " + r.stderr.strip())


if __name__ == "__main__":
    main()
