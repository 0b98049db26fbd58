#!/usr/bin/env python3
"""The visible colour pass's tolerance on the sphere scene, on the CPU (the numpy restatement,
tests/visibility.py): for tol = 0, sqrt(3) s, 2 s, 3 s, 4 s and 6 s, the share of (voxel, view) samples of
clearly front-facing voxels (cos > 0.3 between the sphere's normal at the voxel and the direction
to the camera) that are wrongly occluded, and of clearly back-facing ones (cos < -0.3) that are
wrongly visible; and, in closest mode with one colour per view, the share of voted voxels whose
colour comes from a camera on their own side, next to the plain pass's share.

    python tools/color_visible_tol.py [N [V [W H]]]      (default 64 36 320 240; no GPU)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ar_voxel_project_amd import synthetic as syn  # noqa: E402
from tests import np_restate as npr  # noqa: E402
from tests import visibility as vis  # noqa: E402
from tests.visibility import constant_images, own_side_share, view_of_colour  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    N = a[0] if a else 64
    V = a[1] if len(a) > 1 else 36
    W, H = (a[2], a[3]) if len(a) > 3 else (320, 240)
    sc = syn.sphere_scene(N, V, W=W, H=H)
    s = sc.voxel_size
    st = npr.carve(N, N, N, s, sc.M, sc.masks)
    model = np.zeros((N ** 3, 4), np.float32)
    model[:, 3] = (st.reshape(-1) & 1).astype(np.float32)
    xs, ys, zs = vis.surface_voxels(N, N, N, model)
    index = (zs.astype(np.int64) * N + ys) * N + xs
    p = vis.world_points(s, index, N, N)
    ctr = np.array([syn.EXTENT / 2, syn.EXTENT / 2, -syn.EXTENT / 2])
    nrm = (p - ctr) / np.linalg.norm(p - ctr, axis=1)[:, None]
    cams = vis.camera_centres(sc.Rt)
    images = constant_images(V, W, H)
    print(f"sphere {N}^3, {V} views of {W}x{H}: {len(xs)} surface voxels")
    print("tol        front-facing occluded   back-facing visible   own-side share (closest)")
    for name, k in (("0", 0.0), ("sqrt3 s", np.sqrt(3.0)), ("2 s", 2.0), ("3 s", 3.0), ("4 s", 4.0),
                    ("6 s", 6.0)):
        tol = np.float32(k) * s
        front = back = front_occ = back_vis = 0
        for v in range(V):
            zb = vis.depth_buffer(sc.M[v], s, xs, ys, zs, W, H)
            a2, inside, pix = vis.centre(sc.M[v], s, xs, ys, zs, W, H)
            seen = inside & (a2 > 0)
            visible = seen & (a2 <= (zb.reshape(-1)[pix] + tol).astype(np.float32))
            d = cams[v] - p
            cos = np.einsum("ij,ij->i", d / np.linalg.norm(d, axis=1)[:, None], nrm)
            f, b = seen & (cos > 0.3), seen & (cos < -0.3)
            front += f.sum()
            back += b.sum()
            front_occ += (f & ~visible).sum()
            back_vis += (b & visible).sum()
        got = vis.color_visible(N, N, N, s, sc.M, sc.campos, images, 0, model, tol)
        sel = got.has & (got.views > 0)
        share = own_side_share(sc, got.index[sel], view_of_colour(got.rgba[got.index[sel], :3], V))
        print(f"{name:9s}  {front_occ / front:8.4f} of {front:<9d}  {back_vis / back:8.4f} of {back:<9d} "
              f"{share:.4f} ({sel.sum()} voxels)")
    plain = npr.color(N, N, N, s, sc.M, sc.campos, images, 0, model)
    has = got.has
    idx = got.index[has]
    print(f"plain pass own-side share: {own_side_share(sc, idx, view_of_colour(plain[idx, :3], V)):.4f} "
          f"({has.sum()} voxels)")


if __name__ == "__main__":
    main()
