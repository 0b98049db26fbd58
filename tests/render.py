"""Vectorised numpy restatement of the render (arvx_render; the definition is in
include/arvx/arvx.h, after the smoothing block), built on visibility's footprint and np_restate's
projection: a 64-bit (depth, index) minimum per pixel, resolved into id, depth and BGR images."""
from collections import namedtuple

import numpy as np

from tests import np_restate as npr
from tests import visibility as vis

F32 = npr.F32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

Rendered = namedtuple("Rendered", "bgr depth id")


def vertex_voxels(X, Y, Z, occupied):
    """The welded mesh's vertex voxels of an occupancy (Z, Y, X): occupied with an empty
    6-neighbour, as ascending flat indices."""
    occ = np.asarray(occupied, bool).reshape(Z, Y, X)
    return np.flatnonzero(npr.surface_mask(occ).reshape(-1)).astype(np.int64)


def keys(M, s, index, X, Y, W, H, assoc_left=True):
    """(H * W,) uint64: per pixel the minimum of bits(a2) << 32 | k over the vertex voxels k that
    splat with the pixel in their footprint; all-ones where there are none."""
    index = np.asarray(index, np.int64)
    x, y, z = index % X, (index // X) % Y, index // (X * Y)
    out = np.full(H * W, EMPTY, np.uint64)
    if not len(index):
        return out
    a2 = npr.project_raw(M, s, x, y, z, assoc_left)[0][2]
    ok, c0, c1, r0, r1 = vis.footprint(M, s, x, y, z, W, H, assoc_left)
    wc, hr = np.maximum(c1 - c0 + 1, 0), np.maximum(r1 - r0 + 1, 0)
    area = np.where(ok, wc * hr, 0)
    k = np.nonzero(area)[0]
    if len(k):
        word = (a2.astype(F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
            np.arange(len(index), dtype=np.uint64)
        rep = np.repeat(k, area[k])
        start = np.cumsum(area[k]) - area[k]
        j = np.arange(len(rep)) - np.repeat(start, area[k])  # rank within the footprint
        cols = c0[rep] + j % wc[rep]
        rows = r0[rep] + j // wc[rep]
        np.minimum.at(out, rows * W + cols, word[rep])
    return out


def channel(col):
    """(uint8_t)roundf(fminf(fmaxf(c, 0), 255)) of float32 colours."""
    c = np.asarray(col, F32)
    c = np.where(np.isnan(c), F32(0), np.clip(c, F32(0), F32(255)))
    return npr.round_half_away(c).astype(np.uint8)


def render(M, s, index, col, X, Y, W, H, background=None, assoc_left=True):
    """-> Rendered(bgr (H, W, 3) uint8, depth (H, W) float32, id (H, W) int32) of the vertex voxels
    `index` (ascending flat index) with colours col (Vn, 3), r g b."""
    key = keys(M, s, index, X, Y, W, H, assoc_left)
    empty = key == EMPTY
    ids = np.where(empty, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(empty, np.uint32(0x7F800000), (key >> np.uint64(32)).astype(np.uint32)).astype(np.uint32)
    bgr = np.zeros((H * W, 3), np.uint8) if background is None else \
        np.array(background, np.uint8).reshape(H * W, 3)
    if (~empty).any():
        c = channel(np.asarray(col, F32).reshape(-1, 3)[ids[~empty]])
        bgr[~empty] = c[:, ::-1]
    return Rendered(bgr.reshape(H, W, 3), depth.view(F32).reshape(H, W), ids.reshape(H, W))


def agreement(ids, mask):
    """-> (both, model_only, mask_only): covered pixels of an id image against a view's mask
    (foreground: any channel non-zero)."""
    m = np.asarray(mask)
    fg = (m != 0) if m.ndim == 2 else (m != 0).any(axis=-1)
    cov = np.asarray(ids) >= 0
    return (int(np.count_nonzero(cov & fg)), int(np.count_nonzero(cov & ~fg)),
            int(np.count_nonzero(~cov & fg)))
