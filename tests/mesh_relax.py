"""Meshes for the tests of arvx_mesh_relax / arvx_mesh_relax_triangles, and tests/mesh_smooth.py's
definition in a form that takes a vertex of any valence.

fans(Ks, isolated, seed) -> (verts (V, 3) float32, faces (T, 3) int64, degree (V,) int64): one fan per K
    -- a hub and K rim vertices closed into a ring, faces (hub, r_k, r_k+1) --, every face twice with
    opposite windings, the faces shuffled and the vertices renumbered by a seeded permutation, plus
    `isolated` vertices no face uses.  degree is what the construction states: K for a hub, min(K, 3)
    for a rim vertex (K = 1: the one face is (hub, r, r); K = 2: two faces on the same three vertices),
    0 for an isolated vertex.

smooth(p, faces, iterations, lam, mu) -> (positions, normals, degree): tests/mesh_smooth.py's smooth().
    mesh_smooth keeps the neighbours in a dense (V, largest valence) table and walks every slot of it
    over all the vertices, which a hub of 50 000 neighbours among 50 000 vertices does not allow (20 GB,
    and minutes).  Here the rows are kept as CSRs; the rows of at most `cap` entries are summed slot by
    slot, vectorised over the vertices, exactly as mesh_smooth sums them, and a longer row is summed on
    its own with np.add.accumulate from +0, which adds one entry after the other in fp32 -- the same
    operations in the same order.  The cross products are mesh_smooth.face_cross.
    tests/test_mesh_relax_cpu.py holds the two equal, bit for bit, on meshes mesh_smooth can take, with
    `cap` below and above their valences."""
import numpy as np

from tests import mesh_smooth as ms

F32 = np.float32


def fans(Ks, isolated=0, seed=0):
    rng = np.random.default_rng(seed)
    verts, faces, degree = [], [], []
    base = 0
    for K in Ks:
        hub = base
        rim = base + 1 + np.arange(K)
        centre = rng.uniform(-50, 50, 3)
        ang = 2 * np.pi * (np.arange(K) + rng.uniform(-0.3, 0.3, K)) / K
        ring = np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.2, 0.2, K)], axis=1) * rng.uniform(0.5, 2.0)
        verts.append(centre + rng.uniform(-0.1, 0.1, 3) + [0, 0, 0.5])
        verts.extend(centre + ring)
        f = np.stack([np.full(K, hub), rim, np.roll(rim, -1)], axis=1)
        faces.append(f)
        faces.append(f[:, [0, 2, 1]])
        degree.extend([K] + [min(K, 3)] * K)
        base += K + 1
    for _ in range(isolated):
        verts.append(rng.uniform(-50, 50, 3))
        degree.append(0)
    verts = np.asarray(verts, np.float64).reshape(-1, 3).astype(F32)
    degree = np.asarray(degree, np.int64)
    faces = np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)
    V = len(verts)
    perm = rng.permutation(V)  # old index -> new index
    out_v, out_d = np.empty_like(verts), np.empty_like(degree)
    out_v[perm], out_d[perm] = verts, degree
    faces = perm[faces.astype(np.int64)].reshape(-1, 3)
    faces = faces[rng.permutation(len(faces))]
    return out_v, faces.astype(np.int64), out_d


def _csr(rows, cols, n):
    """The distinct (row, col) pairs, ascending: (cols in row order, count per row, start per row)."""
    width = np.int64(max(int(cols.max()) + 1 if len(cols) else 1, 1))
    key = np.unique(rows.astype(np.int64) * width + cols.astype(np.int64))
    r, c = key // width, key % width
    cnt = np.bincount(r, minlength=n).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    return c, cnt, start


def neighbours(V, faces):
    """N(i) as a CSR: (neighbour list, degree (V,), start (V,))."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    a = np.concatenate([a, a[:, ::-1]])
    a = a[a[:, 0] != a[:, 1]]
    return _csr(a[:, 0], a[:, 1], V)


def _row_sums(values, col, cnt, start, cap):
    """Per row the fp32 sum of values[col[.]] over the row's entries in order, from +0."""
    s = np.zeros((len(cnt), 3), F32)
    short = cnt <= cap
    for r in range(int(cnt[short].max()) if short.any() else 0):
        on = short & (cnt > r)
        s[on] = s[on] + values[col[start[on] + r]]
    for i in np.nonzero(~short)[0]:
        terms = np.concatenate([np.zeros((1, 3), F32), values[col[start[i]:start[i] + cnt[i]]]])
        s[i] = np.add.accumulate(terms, axis=0, dtype=F32)[-1]
    return s


def step(p, csr, f, cap=64):
    col, deg, start = csr
    s = _row_sums(p, col, deg, start, cap)
    has = deg > 0
    m = s[has] / deg[has].astype(F32)[:, None]
    d = m - p[has]
    out = p.copy()
    out[has] = p[has] + F32(f) * d
    return out


def normals(q, faces, cap=64):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(q)
    c = ms.face_cross(q, f).astype(F32) if len(f) else np.zeros((0, 3), F32)
    # (each face once per distinct corner, ascending face per vertex: mesh_smooth.incidences)
    col, cnt, start = _csr(f.reshape(-1), np.repeat(np.arange(len(f), dtype=np.int64), 3), V)
    n = _row_sums(c, col, cnt, start, cap)
    l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    out = np.zeros_like(n)
    nz = l != 0
    out[nz] = n[nz] / l[nz, None]
    return out


def smooth(p, faces, iterations, lam=0.5, mu=-0.53, cap=64):
    p = np.asarray(p, F32).reshape(-1, 3)
    csr = neighbours(len(p), faces)
    for _ in range(iterations):
        p = step(p, csr, lam, cap)
        p = step(p, csr, mu, cap)
    return p, normals(p, faces, cap), csr[1]


def bits(a):
    """float32 values as their bit patterns: every comparison of the relax tests is on these."""
    return np.ascontiguousarray(a, F32).view(np.uint32)
