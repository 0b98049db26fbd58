"""Taubin smoothing and vertex normals of a welded mesh (arvx_mc_mesh_smooth, include/arvx/arvx.h)
restated in numpy.

Every operation is an fp32 numpy operation (rounded on its own); the sums run over the neighbour
or face slots in order, vectorised over the vertices.

neighbours(V, faces) -> (nbr (V, D) int64, deg (V,)): N(i) ascending in row i, padded with -1
step(p, nbr, deg, f): one Jacobi step with factor f
taubin(p, faces, iterations, lam, mu): 2 * iterations steps, factors lam, mu, lam, ...
incidences(V, faces): the (vertex, face) pairs the normals sum over
normals(q, faces): unit vertex normals, outward on the device's meshes
smooth(p, faces, iterations, lam, mu) -> (positions, normals)"""
import numpy as np


def neighbours(V, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    a = np.concatenate([a, a[:, ::-1]])
    a = a[a[:, 0] != a[:, 1]]
    # sorted by (i, j): each row's neighbours ascending (one-dimensional keys i * V + j: the order
    # of np.unique(a, axis=0), many times faster on a large mesh)
    key = np.unique(a[:, 0] * np.int64(max(V, 1)) + a[:, 1])
    a = np.stack([key // max(V, 1), key % max(V, 1)], axis=1)
    deg = np.bincount(a[:, 0], minlength=V).astype(np.int64)
    nbr = np.full((V, max(1, int(deg.max()) if V else 1)), -1, np.int64)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]]) if V else np.zeros(0, np.int64)
    slot = np.arange(len(a)) - start[a[:, 0]]
    nbr[a[:, 0], slot] = a[:, 1]
    return nbr, deg


def step(p, nbr, deg, f):
    p = np.asarray(p, np.float32)
    s = np.zeros_like(p)  # +0
    for r in range(nbr.shape[1]):
        on = deg > r
        s[on] = s[on] + p[nbr[on, r]]
    has = deg > 0
    m = s[has] / deg[has].astype(np.float32)[:, None]
    d = m - p[has]
    out = p.copy()
    out[has] = p[has] + np.float32(f) * d
    return out


def taubin(p, faces, iterations, lam=0.5, mu=-0.53, nbr_deg=None):
    """nbr_deg: neighbours(len(p), faces), where the caller keeps it for a mesh it smooths again."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    nbr, deg = neighbours(len(p), faces) if nbr_deg is None else nbr_deg
    for _ in range(iterations):
        p = step(p, nbr, deg, lam)
        p = step(p, nbr, deg, mu)
    return p


def face_cross(q, faces):
    """c_t = (q[i2] - q[i0]) x (q[i1] - q[i0]), component by component as the definition states."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = q[f[:, 2]] - q[f[:, 0]]
    b = q[f[:, 1]] - q[f[:, 0]]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def incidences(V, faces):
    """-> (inc (n, 2) int64 rows (vertex, face), each face once per distinct corner, ascending face
    per vertex; cnt (V,) faces per vertex; slot (n,) the row's place among its vertex's faces)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    T = max(len(f), 1)
    key = np.unique(f.reshape(-1) * np.int64(T) + np.repeat(np.arange(len(f), dtype=np.int64), 3))
    inc = np.stack([key // T, key % T], axis=1)
    cnt = np.bincount(inc[:, 0], minlength=V) if len(inc) else np.zeros(V, np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if V else np.zeros(0, np.int64)
    slot = np.arange(len(inc)) - start[inc[:, 0]] if len(inc) else np.zeros(0, np.int64)
    return inc, cnt, slot


def normals(q, faces, inc_cnt_slot=None):
    """inc_cnt_slot: incidences(len(q), faces), where the caller keeps it."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    V = len(q)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = face_cross(q, f)
    inc, cnt, slot = incidences(V, f) if inc_cnt_slot is None else inc_cnt_slot
    n = np.zeros((V, 3), np.float32)
    for r in range(int(cnt.max()) if V and len(inc) else 0):
        sel = slot == r
        n[inc[sel, 0]] = n[inc[sel, 0]] + c[inc[sel, 1]]
    l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    out = np.zeros_like(n)
    nz = l != 0
    out[nz] = n[nz] / l[nz, None]
    return out


def smooth(p, faces, iterations, lam=0.5, mu=-0.53, nbr_deg=None, inc_cnt_slot=None):
    q = taubin(p, faces, iterations, lam, mu, nbr_deg)
    return q, normals(q, faces, inc_cnt_slot)
