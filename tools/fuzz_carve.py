#!/usr/bin/env python3
"""A long random comparison of the carve with the oracle (GPU box; the committed tests hold a
short one): grids with ragged edges around the sizes where the kernels change regime (2^26 voxels:
dense classify kernel; item sharing below), slabs, view counts around 64, noise masks from single
pixels to large blocks, fresh and carved models, views in one call or in pieces.
    python tools/fuzz_carve.py <seconds> [seed]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ar_voxel_project_amd import capi  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import scenes  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
oracle = pyoracle
t_end = time.time() + budget
n = 0
while time.time() < t_end:
    big = rng.random() < 0.25
    flags = 0
    if big:  # around 2^26 voxels (dense classify kernel, whole coarse tiles or quarters)
        X = int(rng.choice([384, 400, 416, 448, 512])) + int(rng.integers(-3, 4))
        Y = int(rng.choice([384, 400, 416, 448])) + int(rng.integers(-3, 4))
        Z = int(rng.integers(380, 460))
        zr = None
        if rng.random() < 0.5:  # the oracle on a slab only (time)
            z0 = int(rng.integers(0, Z - 40))
            zr = (z0, z0 + int(rng.integers(8, 40)))
    else:
        X, Y, Z = (int(v) for v in rng.integers(5, 200, 3))
        # the large grids' kernels on a small grid (include/arvx/arvx.h: path flags)
        flags = int(rng.choice([0, capi.CARVE_DENSE_CLASSIFY])) | int(rng.choice([0, capi.CARVE_WHOLE_ITEMS]))
        zr = None
        if rng.random() < 0.3 and Z > 12:
            z0 = int(rng.integers(0, Z - 4))
            zr = (z0, int(rng.integers(z0 + 1, Z + 1)))
    V = int(rng.choice([1, 2, 5, 9, 36, 63, 64, 65, 72])) if not big else int(rng.choice([3, 8, 20]))
    W, H = int(rng.choice([64, 96, 160, 200, 333, 640])), int(rng.choice([48, 72, 120, 150, 251, 480]))
    E = 0.512
    s = np.float32(E / max(X, Y, Z))
    _, _, M = scenes.random_cameras(V, E, seed=int(rng.integers(1 << 30)), W=W, H=H,
                                    inside=bool(rng.random() < 0.2))
    masks = scenes.noise_masks(V, H, W, C=int(rng.choice([1, 3])), p_bg=float(rng.uniform(0.1, 0.9)),
                               block=int(rng.choice([1, 2, 5, 16, 64])), seed=int(rng.integers(1 << 30)))
    mode = int(rng.integers(0, 4))
    z0, z1 = zr if zr else (0, Z)
    planes = np.arange(z0, z1)
    want = oracle.carve_planes(X, Y, s, M, masks, planes)
    with capi.Context(X, Y, Z, s, z_range=zr) as ctx:
        ctx.set_views(M, masks)
        if mode == 0:
            ctx.carve(flags)
        elif mode == 1:  # twice: the second carve on a model that is not fresh
            ctx.carve(flags)
            ctx.carve(flags)
        elif mode == 2:  # the views in two pieces, the later ones first
            k = int(rng.integers(0, V + 1))
            if V - k:
                ctx.carve_views(k, V - k, flags)
            if k:
                ctx.carve_views(0, k, flags)
        else:  # view by view
            for i in rng.permutation(V):
                ctx.carve_views(int(i), 1, flags)
        got = ctx.download_state()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        print(f"MISMATCH case {n}: {X}x{Y}x{Z} z{zr} V={V} {W}x{H} mode {mode} flags {flags}: {len(bad)} voxels, "
              f"first {bad[0]} gpu {got[tuple(bad[0])]} oracle {want[tuple(bad[0])]}", flush=True)
        sys.exit(1)
    n += 1
    if n % 10 == 0:
        print(f"{n} cases ok ({time.time() - (t_end - budget):.0f} s)", flush=True)
print(f"fuzz ok: {n} cases in {budget:.0f} s")
