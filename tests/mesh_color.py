"""Numpy restatement of the mesh colours from the images (arvx_mesh_color; the definition is in
include/arvx/arvx.h, after the triangle render's block), built on the triangle render's restatement:
its projection (render_mesh.project) and its depth image (render_mesh.render(...).image.depth) per
view, then the candidate test, the integer bilinear sample and the vote per vertex.  Nothing here calls
the device or is derived from it."""
from collections import namedtuple

import numpy as np

from tests import render_mesh as rm

F32, F64, I64 = np.float32, np.float64, np.int64
CLOSEST, AVERAGE = 0, 1
FOREGROUND = 1

Colours = namedtuple("Colours", "rgb views coloured depth in_image visible")


def depth_buffers(M, s, verts, faces, W, H, assoc_left=True):
    """Step 2: D_v of every view, (V, H, W) float32 -- the triangle render's depth image."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    col = np.zeros_like(verts)
    return np.stack([rm.render(M[v], s, verts, col, faces, W, H, assoc_left=assoc_left).image.depth
                     for v in range(len(M))])


def sample(image, fx, fy):
    """Step 4: S per channel r, g, b (n, 3) int64 of the BGR image at fixed-point positions inside it."""
    H, W = image.shape[:2]
    I = image.astype(I64)
    c0, r0, wx, wy = fx >> 4, fy >> 4, fx & 15, fy & 15
    c1, r1 = np.minimum(c0 + 1, W - 1), np.minimum(r0 + 1, H - 1)
    assert np.all((wx == 0) | (c0 + 1 <= W - 1)) and np.all((wy == 0) | (r0 + 1 <= H - 1))
    S = ((16 - wx) * (16 - wy))[:, None] * I[r0, c0] + (wx * (16 - wy))[:, None] * I[r0, c1] + \
        ((16 - wx) * wy)[:, None] * I[r1, c0] + (wx * wy)[:, None] * I[r1, c1]
    assert S.min(initial=0) >= 0 and S.max(initial=0) <= 255 * 256
    return S[:, ::-1]


def background(mask):
    """The view's background plane as arvx_set_views derives it: a pixel is background where every
    channel of its mask is zero."""
    m = np.asarray(mask)
    return (m.reshape(m.shape[0], m.shape[1], -1) == 0).all(axis=2)


def color(M, s, verts, vertex_rgb, faces, images, mode, tol, flags=0, masks=None, assoc_left=True, depth=None):
    """-> Colours(rgb (Vn, 3) float32, views (Vn,) int32, coloured, depth (V, H, W), in_image (V, Vn),
    visible (V, Vn)).  depth: D_v computed before (depth_buffers), shared between calls."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    col = np.asarray(vertex_rgb, F32).reshape(-1, 3)
    V, (H, W) = len(M), images[0].shape[:2]
    Vn = len(verts)
    if depth is None:
        depth = depth_buffers(M, s, verts, faces, W, H, assoc_left)
    tol = F32(tol)
    n = np.zeros(Vn, np.int32)
    total = np.zeros((Vn, 3), np.uint64)   # AVERAGE
    best = np.full(Vn, np.inf, F32)        # CLOSEST
    best_S = np.zeros((Vn, 3), I64)
    in_image = np.zeros((V, Vn), bool)
    visible = np.zeros((V, Vn), bool)
    for v in range(V):
        pr = rm.project(M[v], s, verts, assoc_left)
        inside = pr.valid & (pr.fx >= 0) & (pr.fx <= 16 * (W - 1)) & (pr.fy >= 0) & (pr.fy <= 16 * (H - 1))
        k = np.flatnonzero(inside)
        fx, fy, a2 = pr.fx[k], pr.fy[k], pr.a2[k]
        cn, rn = (fx + 8) >> 4, (fy + 8) >> 4
        with np.errstate(over="ignore"):
            vis = a2 <= (depth[v][rn, cn] + tol).astype(F32)
        if flags & FOREGROUND:
            vis &= ~background(masks[v])[rn, cn]
        in_image[v, k] = True
        k, fx, fy, a2 = k[vis], fx[vis], fy[vis], a2[vis]
        visible[v, k] = True
        S = sample(images[v], fx, fy)
        n[k] += 1
        total[k] += S.astype(np.uint64)
        nearer = a2 < best[k]
        best[k[nearer]] = a2[nearer]
        best_S[k[nearer]] = S[nearer]
    rgb = col.copy()
    seen = n > 0
    if mode == CLOSEST:
        rgb[seen] = best_S[seen].astype(F32) / F32(256.0)
    else:
        rgb[seen] = (total[seen].astype(F64) / (256 * n[seen].astype(I64))[:, None].astype(F64)).astype(F32)
    return Colours(rgb, n, int(np.count_nonzero(seen)), depth, in_image, visible)
