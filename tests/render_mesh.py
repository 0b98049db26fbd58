"""Numpy restatement of the triangle render (arvx_render_mesh; the definition is in
include/arvx/arvx.h, after the render's block), built on np_restate's projection: int64 edge
functions over each triangle's pixel box, float64 weights, a 64-bit (depth, face) minimum per pixel,
resolved into id, depth and BGR images.  The (triangle, pixel) pairs are laid out flat, a slice of
triangles at a time; nothing here calls the device or is derived from it."""
from collections import namedtuple

import numpy as np

from tests import np_restate as npr
from tests.render import EMPTY, Rendered, channel

F32, F64, I64 = np.float32, np.float64, np.int64
FLT_MIN = np.finfo(np.float32).tiny
DRAWN, EMPTY_CLASS, FLAT, REFUSED = range(4)
LANE_PIXELS = 64  # pixel boxes above this go to the device's list (no part of the definition)
PAIRS = 1 << 21   # (triangle, pixel) pairs evaluated at a time

Projected = namedtuple("Projected", "fx fy a2 valid")
Result = namedtuple("Result", "image counts classes box")


def headlight(M):
    """The third row of M reordered to the voxel axes: world = (y s, x s, -z s)."""
    M = np.asarray(M, F32).reshape(3, 4)
    return np.array([M[2, 1], M[2, 0], -M[2, 2]], F32)


def project(M, s, verts, assoc_left=True):
    """Step 1: the fixed-point positions, a2 and VALID of the vertices."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    a, qu, qv = npr.project_raw(M, s, p[:, 0], p[:, 1], p[:, 2], assoc_left)
    with np.errstate(invalid="ignore"):
        valid = (a[2] >= FLT_MIN) & np.isfinite(qu) & np.isfinite(qv) & (np.abs(qu) <= 32768) & \
            (np.abs(qv) <= 32768)
        fx = npr.round_half_away(np.where(valid, qu * F32(16.0), F32(0)).astype(F32)).astype(I64)
        fy = npr.round_half_away(np.where(valid, qv * F32(16.0), F32(0)).astype(F32)).astype(I64)
    return Projected(fx, fy, a[2].astype(F32), valid)


def _edges(x, y, px, py, neg):
    """Step 3's E0, E1, E2 for corner arrays x, y of shape (3, n), negated where A < 0."""
    e0 = (x[1] - px) * (y[2] - py) - (x[2] - px) * (y[1] - py)
    e1 = (x[2] - px) * (y[0] - py) - (x[0] - px) * (y[2] - py)
    e2 = (x[0] - px) * (y[1] - py) - (x[1] - px) * (y[0] - py)
    sign = np.where(neg, -1, 1).astype(I64)
    return e0 * sign, e1 * sign, e2 * sign


def _weights(e, iz):
    t = [e[k].astype(F64) * iz[k] for k in range(3)]
    return t, (t[0] + t[1]) + t[2]


def _length(x, y, z):
    return np.sqrt(((x * x).astype(F32) + (y * y).astype(F32)).astype(F32) + (z * z).astype(F32)).astype(F32)


def shade(verts, faces, light):
    """Step 5's factor 0.25 + 0.75 f per face."""
    p = np.asarray(verts, F32).reshape(-1, 3)
    L = np.asarray(light, F32).reshape(3)
    f = np.asarray(faces, I64).reshape(-1, 3)
    a = (p[f[:, 2]] - p[f[:, 0]]).astype(F32)
    b = (p[f[:, 1]] - p[f[:, 0]]).astype(F32)
    c = [((a[:, 1] * b[:, 2]).astype(F32) - (a[:, 2] * b[:, 1]).astype(F32)).astype(F32),
         ((a[:, 2] * b[:, 0]).astype(F32) - (a[:, 0] * b[:, 2]).astype(F32)).astype(F32),
         ((a[:, 0] * b[:, 1]).astype(F32) - (a[:, 1] * b[:, 0]).astype(F32)).astype(F32)]
    l = _length(*c)
    m = _length(L[0], L[1], L[2])
    d = (((c[0] * L[0]).astype(F32) + (c[1] * L[1]).astype(F32)).astype(F32) + (c[2] * L[2]).astype(F32)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.abs(d) / (l * m).astype(F32)).astype(F32)
    f = np.where((l == 0) | (m == 0), F32(1), np.fmin(ratio, F32(1))).astype(F32)
    return (F32(0.25) + (F32(0.75) * f).astype(F32)).astype(F32)


def render(M, s, verts, vertex_rgb, faces, W, H, background=None, light=None, assoc_left=True):
    """-> Result(image = Rendered(bgr, depth, id), counts = (drawn, empty, flat, refused),
    classes (T,) the class of every triangle, box (T,) the pixels of its clipped box)."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    col = np.asarray(vertex_rgb, F32).reshape(-1, 3)
    faces = np.asarray(faces)
    faces = faces.reshape(-1, faces.shape[-1] if faces.ndim == 2 else 3)[:, :3].astype(I64)  # (records: i0 i1 i2)
    T = len(faces)
    pr = project(M, s, verts, assoc_left)
    key = np.full(H * W, EMPTY, np.uint64)
    classes = np.full(T, REFUSED, np.int64)
    box = np.zeros(T, np.int64)
    geo = None
    if T:
        ok = pr.valid[faces].all(axis=1)
        x = pr.fx[faces].T  # (3, T)
        y = pr.fy[faces].T
        A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        classes[ok & (A == 0)] = FLAT
        live = ok & (A != 0)
        neg = A < 0
        absA = np.abs(A)
        with np.errstate(divide="ignore"):
            iz = (F64(1.0) / pr.a2[faces].T.astype(F64))
        c0 = np.maximum(-((-x.min(axis=0)) // 16), 0)  # ceil, floor: towards +inf, -inf
        c1 = np.minimum(x.max(axis=0) // 16, W - 1)
        r0 = np.maximum(-((-y.min(axis=0)) // 16), 0)
        r1 = np.minimum(y.max(axis=0) // 16, H - 1)
        wc, hr = np.maximum(c1 - c0 + 1, 0), np.maximum(r1 - r0 + 1, 0)
        box = np.where(live, wc * hr, 0)
        classes[live] = EMPTY_CLASS
        geo = (x, y, neg, absA, iz)
        todo = np.flatnonzero(box)
        start = 0
        while start < len(todo):  # slices of triangles of at most PAIRS pairs (one triangle at least)
            end = start + max(1, int(np.searchsorted(np.cumsum(box[todo[start:]]), PAIRS, side="right")))
            k = todo[start:end]
            start = end
            rep = np.repeat(k, box[k])
            first = np.cumsum(box[k]) - box[k]
            j = np.arange(len(rep)) - np.repeat(first, box[k])  # rank within the box, row-major
            c = c0[rep] + j % wc[rep]
            r = r0[rep] + j // wc[rep]
            e = _edges(x[:, rep], y[:, rep], 16 * c, 16 * r, neg[rep])
            cov = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
            assert np.array_equal((e[0] + e[1] + e[2])[cov], absA[rep][cov])
            rep, c, r = rep[cov], c[cov], r[cov]
            if not len(rep):
                continue
            _, S = _weights([ek[cov] for ek in e], iz[:, rep])
            depth = (absA[rep].astype(F64) / S).astype(F32)
            assert (depth > 0).all()
            word = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rep.astype(np.uint64)
            np.minimum.at(key, r * W + c, word)
            classes[np.unique(rep)] = DRAWN
    empty = key == EMPTY
    ids = np.where(empty, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(empty, np.uint32(0x7F800000), (key >> np.uint64(32)).astype(np.uint32)).astype(np.uint32)
    bgr = np.zeros((H * W, 3), np.uint8) if background is None else \
        np.array(background, np.uint8).reshape(H * W, 3)
    pix = np.flatnonzero(~empty)
    if len(pix):  # step 5: the winner's edge functions once more
        x, y, neg, absA, iz = geo
        t = ids[pix].astype(I64)
        e = _edges(x[:, t], y[:, t], 16 * (pix % W), 16 * (pix // W), neg[t])
        w, S = _weights(e, iz[:, t])
        f = shade(verts, faces, light)[t] if light is not None else None
        out = np.empty((len(pix), 3), F32)
        for ch in range(3):
            cc = [col[faces[t, k], ch].astype(F64) for k in range(3)]
            n = (w[0] * cc[0] + w[1] * cc[1]) + w[2] * cc[2]
            v = (n / S).astype(F32)
            out[:, ch] = v if f is None else (f * v).astype(F32)
        bgr[pix] = channel(out)[:, ::-1]
    counts = tuple(int(np.count_nonzero(classes == k)) for k in range(4))
    image = Rendered(bgr.reshape(H, W, 3), depth.view(F32).reshape(H, W), ids.reshape(H, W))
    return Result(image, counts, classes, box)
