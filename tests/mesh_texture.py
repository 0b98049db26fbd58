"""Numpy restatement of the mesh textures (arvx_mesh_texture; the definition is in include/arvx/arvx.h,
after the mesh colours' block), built on the triangle render's restatement (tests/render_mesh.py) and
the mesh colours' (tests/mesh_color.py): the atlas layout in integers, the best view of every face, the
texels sampled from it or interpolated from the vertex colours, and the draw with the texture.  Nothing
here calls the device or is derived from it."""
from collections import namedtuple

import numpy as np

from tests import mesh_color as mcol
from tests import render_mesh as rm
from tests.render import Rendered, channel

F32, F64, I64 = np.float32, np.float64, np.int64
FOREGROUND = 1
R_MAX, AW_MAX, AH_MAX = 253, 16384, 32768

Layout = namedtuple("Layout", "R AW AH cw ch per_row rows cells T")
Texture = namedtuple("Texture", "atlas face_view face_uv counts layout visible depth")


# ---- step 1: the layout ---------------------------------------------------------------------------

def layout(T, R, AW):
    assert 1 <= R <= R_MAX
    cw, ch = R + 3, R + 2
    assert cw <= AW <= AW_MAX
    per_row = AW // cw
    cells = (T + 1) // 2
    rows = -(-cells // per_row)
    return Layout(R, AW, rows * ch, cw, ch, per_row, rows, cells, T)


def local_texels(R):
    """(i, j) of a face's texels, each (n,) int64 with n = (R + 2)(R + 3) / 2: i, j >= 0, i + j <= R + 1."""
    i, j = np.meshgrid(np.arange(R + 2), np.arange(R + 2), indexing="ij")
    keep = i + j <= R + 1
    return i[keep].astype(I64), j[keep].astype(I64)


def texel_xy(lay, f, i, j):
    """The atlas texel (x, y) of local texel (i, j) of face f (arrays broadcast)."""
    f, i, j = np.asarray(f, I64), np.asarray(i, I64), np.asarray(j, I64)
    k, half = f >> 1, f & 1
    x0, y0 = (k % lay.per_row) * lay.cw, (k // lay.per_row) * lay.ch
    return x0 + np.where(half == 0, i, lay.cw - 1 - i), y0 + np.where(half == 0, j, lay.ch - 1 - j)


def face_uv(lay):
    """(T, 3, 2) float32: the UV of corners 0, 1, 2 -- local texels (0, 0), (R, 0), (0, R)."""
    f = np.arange(lay.T, dtype=I64)[:, None]
    x, y = texel_xy(lay, f, np.array([[0, lay.R, 0]]), np.array([[0, 0, lay.R]]))
    uv = np.empty((lay.T, 3, 2), F32)
    if lay.T:
        uv[..., 0] = (x.astype(F32) + F32(0.5)) / F32(lay.AW)
        uv[..., 1] = (y.astype(F32) + F32(0.5)) / F32(lay.AH)
    return uv


# ---- step 2: the best view ------------------------------------------------------------------------

def areas(M, s, verts, faces, assoc_left=True):
    """A_v of every face in every view, (V, T) int64; corners that are not VALID give fx = fy = 0."""
    out = np.empty((len(M), len(faces)), I64)
    for v in range(len(M)):
        pr = rm.project(M[v], s, verts, assoc_left)
        x, y = pr.fx[faces].T, pr.fy[faces].T
        out[v] = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    return out


def best_view(visible, A, faces):
    """face_view (T,) int32 from the vertices' VISIBLE (V, Vn) and the areas (V, T)."""
    cand = visible[:, faces].all(axis=2) & (A != 0)
    size = np.where(cand, np.abs(A), -1)
    best = size.argmax(axis=0) if len(size) else np.zeros(len(faces), I64)  # (argmax: the first of equals)
    return np.where(cand.any(axis=0), best, -1).astype(np.int32)


# ---- steps 3 and 4: the texels --------------------------------------------------------------------

def _blend(b0, b1, b2, a0, a1, a2, R):
    return (((b0.astype(F64) * a0.astype(F64) + b1.astype(F64) * a1.astype(F64)) + b2.astype(F64) * a2.astype(F64))
            / F64(R)).astype(F32)


def face_texels(M, s, verts, col, faces, images, face_view, R, assoc_left=True):
    """-> (bgr (T, n, 3) uint8 of every face's n local texels in local_texels' order, clamped (T, n) bool:
    the texels whose fx or fy the clamp changed)."""
    W, H = images[0].shape[1], images[0].shape[0]
    i, j = local_texels(R)
    b1, b2, b0 = i[None, :], j[None, :], (R - i - j)[None, :]
    T, n = len(faces), len(i)
    out = np.zeros((T, n, 3), np.uint8)
    clamped = np.zeros((T, n), bool)
    fall = np.ones((T, n), bool)
    for v in np.unique(face_view[face_view >= 0]):
        k = np.flatnonzero(face_view == v)
        p = [verts[faces[k, c]] for c in range(3)]
        q = np.stack([_blend(b0, b1, b2, p[0][:, ax, None], p[1][:, ax, None], p[2][:, ax, None], R)
                      for ax in range(3)], axis=-1)  # (len(k), n, 3)
        pr = rm.project(M[v], s, q.reshape(-1, 3), assoc_left)
        ok = pr.valid
        fx, fy = np.clip(pr.fx[ok], 0, 16 * (W - 1)), np.clip(pr.fy[ok], 0, 16 * (H - 1))
        S = mcol.sample(images[v], fx, fy)  # (r, g, b)
        texel = ((S + 128) >> 8).astype(np.uint8)[:, ::-1]
        flat = np.flatnonzero(ok)
        rows, cols = k[flat // n], flat % n
        out[rows, cols] = texel
        fall[rows, cols] = False
        clamped[rows, cols] = (fx != pr.fx[ok]) | (fy != pr.fy[ok])
    rows, cols = np.nonzero(fall)
    if len(rows):
        c = [col[faces[rows, k]] for k in range(3)]
        w = np.stack([_blend(b0[0, cols], b1[0, cols], b2[0, cols], c[0][:, ch], c[1][:, ch], c[2][:, ch], R)
                      for ch in range(3)], axis=-1)
        out[rows, cols] = channel(w)[:, ::-1]
    return out, clamped


# ---- step 5: the product --------------------------------------------------------------------------

def texture(M, s, verts, vertex_rgb, faces, images, R, AW, tol, flags=0, masks=None, assoc_left=True, depth=None):
    """-> Texture(atlas (AH, AW, 3) uint8, face_view (T,) int32, face_uv (T, 3, 2) float32,
    counts (T, textured, AW, AH), layout, visible (V, Vn), depth (V, H, W))."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    col = np.asarray(vertex_rgb, F32).reshape(-1, 3)
    faces = np.asarray(faces)
    faces = faces.reshape(-1, faces.shape[-1] if faces.ndim == 2 else 3)[:, :3].astype(I64)
    T = len(faces)
    lay = layout(T, R, AW)
    assert lay.AH <= AH_MAX
    res = mcol.color(M, s, verts, col, faces, images, mcol.AVERAGE, tol, flags, masks, assoc_left, depth)
    fv = best_view(res.visible, areas(M, s, verts, faces, assoc_left), faces) if T else np.zeros(0, np.int32)
    atlas = np.zeros((lay.AH, lay.AW, 3), np.uint8)
    if T:
        bgr, _ = face_texels(M, s, verts, col, faces, images, fv, R, assoc_left)
        i, j = local_texels(R)
        x, y = texel_xy(lay, np.arange(T)[:, None], i[None, :], j[None, :])
        atlas[y, x] = bgr
    counts = (T, int(np.count_nonzero(fv >= 0)), lay.AW, lay.AH)
    return Texture(atlas, fv, face_uv(lay), counts, lay, res.visible, res.depth)


# ---- step 6: drawing ------------------------------------------------------------------------------

def drawn_texel(t1, t2, S, R):
    """(i, j) of the definition's step 6 for float64 weights."""
    i = np.floor((t1 / S) * F64(R) + 0.5)
    j = np.floor((t2 / S) * F64(R) + 0.5)
    return np.clip(i, 0, R).astype(I64), np.clip(j, 0, R).astype(I64)


def draw(M, s, verts, faces, tex, W, H, background=None, light=None, assoc_left=True):
    """The triangle render with source | ARVX_MESH_TEXTURED: -> Rendered(bgr, depth, id)."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces)
    faces = faces.reshape(-1, faces.shape[-1] if faces.ndim == 2 else 3)[:, :3].astype(I64)
    base = rm.render(M, s, verts, np.zeros_like(verts), faces, W, H, background, None, assoc_left).image
    bgr = base.bgr.reshape(H * W, 3).copy()
    ids = base.id.reshape(-1)
    pix = np.flatnonzero(ids >= 0)
    if len(pix):
        t = ids[pix].astype(I64)
        pr = rm.project(M, s, verts, assoc_left)
        x, y = pr.fx[faces[t]].T, pr.fy[faces[t]].T
        A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        e = rm._edges(x, y, 16 * (pix % W), 16 * (pix // W), A < 0)
        iz = F64(1.0) / pr.a2[faces[t]].T.astype(F64)
        w, S = rm._weights(e, iz)
        i, j = drawn_texel(w[1], w[2], S, tex.layout.R)
        assert (i + j <= tex.layout.R + 1).all()
        tx, ty = texel_xy(tex.layout, t, i, j)
        v = tex.atlas[ty, tx][:, ::-1].astype(F32)  # (r, g, b)
        if light is not None:
            v = (rm.shade(verts, faces, light)[t][:, None] * v).astype(F32)
        bgr[pix] = channel(v)[:, ::-1]
    return Rendered(bgr.reshape(H, W, 3), base.depth, base.id)
