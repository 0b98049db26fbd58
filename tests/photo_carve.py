"""Vectorised numpy restatement of photo-consistency carving (arvx_photo_carve; the definition is in
include/arvx/arvx.h, next to arvx_color_visible), built on tests/visibility.py's centre, depth
buffer and surface, as color_visible is."""
from collections import namedtuple

import numpy as np

from tests import np_restate as npr
from tests import visibility as vis

F32, F64 = vis.F32, vis.F64

Photo = namedtuple("Photo", "state iterations removed sweeps")


def statistic(Ms, s, xs, ys, zs, images, tol, assoc_left=True):
    """-> (n, D) per voxel (xs, ys, zs) of the surface S those coordinates list: the number of views
    it is visible in and D = sum_c (n Q_c - S_c^2) of their centre samples, int64 (steps 2-3)."""
    Ms = np.asarray(Ms, F32).reshape(-1, 3, 4)
    tol = F32(tol)
    n = np.zeros(len(xs), np.int64)
    S = np.zeros((len(xs), 3), np.int64)
    Q = np.zeros((len(xs), 3), np.int64)
    for i in range(Ms.shape[0]):
        H, W = images[i].shape[:2]
        zb = vis.depth_buffer(Ms[i], s, xs, ys, zs, W, H, assoc_left)
        a2, inside, pix = vis.centre(Ms[i], s, xs, ys, zs, W, H, assoc_left)
        with np.errstate(invalid="ignore", over="ignore"):
            v = inside & (a2 > 0) & (a2 <= (zb.reshape(-1)[pix] + tol).astype(F32))
        rgb = images[i].reshape(H * W, 3)[pix][:, ::-1].astype(np.int64)
        S[v] += rgb[v]
        Q[v] += rgb[v] * rgb[v]
        n += v
    D = (n[:, None] * Q - S * S).sum(axis=1)
    return n, D


def inconsistent(n, D, max_std, min_views):
    """Step 4, in fp64."""
    with np.errstate(invalid="ignore"):  # (inf * 0 where max_std is +inf and no view sees the voxel)
        lim = (F64(F32(max_std)) * F64(F32(max_std))) * (n.astype(F64) * n.astype(F64))
        return (n >= min_views) & (D.astype(F64) > lim)


def photo_carve(X, Y, Z, s, Ms, images, state, max_std, min_views, tol, max_iterations,
                assoc_left=True):
    """arvx_photo_carve on the state bytes `state` (Z*Y*X; bit0 occupied, bit1 seen).  Returns
    Photo(state after the call, iterations run, voxels removed, the removed flat indices of each
    iteration)."""
    st = np.array(state, np.uint8).reshape(Z, Y, X)
    sweeps = []
    it = 0
    while it < max_iterations:
        occ = (st & 1) != 0
        zs, ys, xs = np.nonzero(npr.surface_mask(occ))
        n, D = statistic(Ms, s, xs, ys, zs, images, tol, assoc_left)
        bad = inconsistent(n, D, max_std, min_views)
        st[zs[bad], ys[bad], xs[bad]] &= np.uint8(0xFE)
        sweeps.append(((zs[bad].astype(np.int64) * Y + ys[bad]) * X + xs[bad]))
        it += 1
        if not bad.any():
            break
    return Photo(st.reshape(-1), it, int(sum(len(w) for w in sweeps)), sweeps)


def pit_masks(sc):
    """(pit, solid) bool (Z, Y, X): voxel centres inside the scene's pit, and inside the box
    outside the pit (synthetic.pit_box_scene)."""
    X, Y, Z = sc.X, sc.Y, sc.Z
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    w = np.stack(npr.to_word(sc.voxel_size, x, y, z), axis=-1).astype(F64)
    (lo, hi), (plo, phi) = sc.box, sc.pit
    in_box = np.all((w > lo) & (w < hi), axis=-1)
    in_pit = np.all((w > plo) & (w < phi), axis=-1)
    return in_pit & in_box, in_box & ~in_pit
