"""The refined marching-cubes mesh (include/arvx/arvx.h, arvx_mc_mesh_refined) restated in numpy,
from the definition there: cut edges, their order, the faces over them, the inside test with float
coordinates, the bisection and the vertex colours.  Independent of the device and of mesh_weld.py."""
import numpy as np

from tests import np_restate as npr

F32 = np.float32
MODEL_RGB = (50.0, 168.0, 141.0)


def cut_edges(occ):
    """occ (Z, Y, X) bool -> (keys ascending, q (Vr, 3) lower ends x y z, axis (Vr,))."""
    Z, Y, X = occ.shape
    P = np.pad(np.asarray(occ, bool), 1, constant_values=False)  # index + 1
    base = P[:Z + 1, :Y + 1, :X + 1]
    other = (P[:Z + 1, :Y + 1, 1:X + 2], P[:Z + 1, 1:Y + 2, :X + 1], P[1:Z + 2, :Y + 1, :X + 1])
    keys = []
    for a in range(3):
        pz, py, px = np.nonzero(base != other[a])
        keys.append(((pz * (Y + 1) + py) * (X + 1) + px) * 3 + a)
    keys = np.sort(np.concatenate(keys).astype(np.int64))
    axis = keys % 3
    pt = keys // 3
    q = np.stack([pt % (X + 1) - 1, (pt // (X + 1)) % (Y + 1) - 1, pt // ((X + 1) * (Y + 1)) - 1], axis=1)
    return keys, q, axis


def _occupied(occ, p):
    Z, Y, X = occ.shape
    ok = ((p >= 0) & (p < np.array([X, Y, Z]))).all(axis=1)
    out = np.zeros(len(p), bool)
    out[ok] = occ[p[ok, 2], p[ok, 1], p[ok, 0]]
    return out


def inside(p, s, Ms, masks, assoc_left=True):
    """inside(p) of the definition for points p (n, 3) float32 voxel coordinates x y z."""
    p = np.asarray(p, F32)
    res = np.ones(len(p), bool)
    Ms = np.asarray(Ms, F32).reshape(-1, 3, 4)
    for M, mask in zip(Ms, masks):
        H, W = mask.shape[:2]
        _, u, v = npr.project_raw(M, s, p[:, 0], p[:, 1], p[:, 2], assoc_left)
        ru, rv = npr.round_half_away(u), npr.round_half_away(v)
        seen = (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)  # NaN compares false
        px = np.where(seen, ru, 0).astype(np.int64)
        py = np.where(seen, rv, 0).astype(np.int64)
        res &= ~(seen & npr.is_background(mask, px, py))
    return res


def faces_over(occ, keys):
    """(T, 3) vertex indices of the triangles of the reference's cell walk (x outermost, z
    innermost), corner k of a triangle being the rank of its cut edge in `keys`; and per triangle
    the occupied corners' voxels (T, 3, 3) -- the snapped vertices."""
    Z, Y, X = occ.shape
    rows = npr.mc_triangle_rows()
    corner = np.array(npr._MC_CORNER)
    P = np.pad(np.asarray(occ, bool), 1, constant_values=False)
    idx = np.zeros((X + 1, Y + 1, Z + 1), np.int64)  # cell (x, y, z) at [x + 1, y + 1, z + 1]
    for i, (a, b, c) in enumerate(corner):
        idx |= (~P[c:c + Z + 1, b:b + Y + 1, a:a + X + 1]).transpose(2, 1, 0).astype(np.int64) << i
    flat = idx.reshape(-1)
    ntri = np.array([len(r) // 3 for r in rows])[flat]
    off = np.concatenate([[0], np.cumsum(ntri)])
    T = int(off[-1])
    faces = np.zeros((T, 3), np.int64)
    snapped = np.zeros((T, 3, 3), np.int64)
    cx, cy, cz = np.unravel_index(np.arange(flat.size), idx.shape)
    cell = np.stack([cx, cy, cz], axis=1) - 1
    for i in np.unique(flat):
        sel = np.nonzero(flat == i)[0]
        row = rows[i]
        for k in range(len(row) // 3):
            for v in range(3):
                e = row[3 * k + v]
                a, b = e % 8, npr._MC_SECOND[e]
                lo = np.minimum(corner[a], corner[b])
                ax = int(np.nonzero(corner[a] != corner[b])[0][0])
                qq = cell[sel] + lo + 1
                key = ((qq[:, 2] * (Y + 1) + qq[:, 1]) * (X + 1) + qq[:, 0]) * 3 + ax
                r = np.searchsorted(keys, key)
                assert np.array_equal(keys[r], key), "a triangle uses an edge that is not cut"
                faces[off[sel] + k, v] = r
                snapped[off[sel] + k, v] = cell[sel] + corner[a if not (i >> a) & 1 else b]
    return faces, snapped


def refine(occ, s, Ms, masks, B, assoc_left=True, rgb=None):
    """-> dict: verts (Vr, 3) f32, faces (T, 3), face_rgb (T, 3), vertex_rgb (Vr, 3) f32, edges
    (Vr, 4) int32, cut (Vr,) int32, snapped (T, 3, 3).  rgb: (Z, Y, X, 3) float32 voxel colours
    (default MODEL_COLOR everywhere); Ms / masks may be empty (no views)."""
    occ = np.asarray(occ, bool)
    assert 0 <= B <= 10
    keys, q, axis = cut_edges(occ)
    n = len(keys)
    step = np.zeros((n, 3), np.int64)
    step[np.arange(n), axis] = 1
    low = _occupied(occ, q)
    assert np.array_equal(_occupied(occ, q + step), ~low)
    A = np.where(low[:, None], q, q + step)
    sgn = np.where(low, 1, -1)
    E = A + step * sgn[:, None]
    if len(masks):
        inA = inside(A.astype(F32), s, Ms, masks, assoc_left)
        sil = inA & ~inside(E.astype(F32), s, Ms, masks, assoc_left)
    else:
        sil = np.zeros(n, bool)
    lo, hi = np.zeros(n, np.int64), np.full(n, 1 << B, np.int64)
    d = (step * sgn[:, None]).astype(F32)
    for _ in range(B):
        mid = (lo + hi) // 2
        t = (mid.astype(F32) / F32(1 << B)).astype(F32)
        pts = (A.astype(F32) + d * t[:, None]).astype(F32)
        ins = np.zeros(n, bool)
        ins[sil] = inside(pts[sil], s, Ms, masks, assoc_left)
        lo, hi = np.where(ins, mid, lo), np.where(ins, hi, mid)
    cut = np.where(sil, lo + hi, 1 << B)
    t = (cut.astype(F32) / F32(1 << (B + 1))).astype(F32)
    verts = (A.astype(F32) + d * t[:, None]).astype(F32)
    edges = np.concatenate([A, (2 * axis + (~low) + 8 * (~sil))[:, None]], axis=1).astype(np.int32)
    if rgb is None:
        rgb = np.broadcast_to(np.array(MODEL_RGB, F32), occ.shape + (3,))
    vrgb = np.asarray(rgb, F32)[A[:, 2], A[:, 1], A[:, 0]] if n else np.zeros((0, 3), F32)
    faces, snapped = faces_over(occ, keys)
    if len(faces):
        c0, c1 = vrgb[faces[:, 0]], vrgb[faces[:, 1]]  # the third colour is the second's (`i + 1`)
        m = (((c0 + c1).astype(F32) + c1).astype(F32) / F32(3)).astype(F32)
        face_rgb = np.floor(np.abs(m.astype(np.float64)) + 0.5).astype(np.int64)
    else:
        face_rgb = np.zeros((0, 3), np.int64)
    return dict(verts=verts, faces=faces, face_rgb=face_rgb, vertex_rgb=vrgb.astype(F32), edges=edges,
                cut=cut.astype(np.int32), snapped=snapped, silhouette=sil)
