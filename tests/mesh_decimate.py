"""Vertex clustering of a welded mesh (arvx_mc_mesh_decimate, include/arvx/arvx.h) restated in numpy.

Every operation on a position or a colour is an fp32 numpy operation (rounded on its own); the sums
run over the member slots of the clusters in order, vectorised over the clusters.

clusters(lattice, cell) -> (vmap (V,) int64, members (Vd,) int64, cluster (Vd, 3) int64): the
    non-empty clusters ascending by (z, y, x) -- the flat index order of any cluster grid
means(q, vmap, members): per decimated vertex, the sequential fp32 sum of its members' rows of q in
    ascending vertex index, divided by the count
faces(records, vmap) -> (kept (Td, W), keep (Td,) the surviving t, degenerate, duplicates): the
    mapped corners in the first three columns, the other columns unchanged
decimate(lattice, records, cell, q=None, col=None) -> dict with verts, records, rgb (col given),
    members, map"""
import numpy as np

# the random fills the device tests decimate (tests/test_mc_decimate_gpu.py); the CPU test checks on
# the oracle's meshes of the same models that they reach the cases the kernels can get wrong
FILLS = [((12, 9, 7), 0.3), ((70, 33, 20), 0.5), ((130, 5, 9), 0.7), ((64, 64, 8), 0.3)]
CELLS = (1, 2, 3, 4, 7, 64)


def fill_state(k):
    """Byte state (occupied | seen bits) of random fill k of FILLS."""
    (X, Y, Z), fill = FILLS[k]
    occ = np.random.default_rng(7100 + k).random(X * Y * Z) < fill
    return (occ * 1 | 2).astype(np.uint8)


def clusters(lattice, cell):
    l = np.asarray(lattice, np.float32).reshape(-1, 3)
    assert np.array_equal(l, np.floor(l)) and (l >= 0).all(), "lattice vertices"
    c = l.astype(np.int64) // int(cell)
    if len(c) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    key = c[:, ::-1]  # (z, y, x): np.unique sorts rows lexicographically
    uniq, vmap, members = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return vmap.reshape(-1).astype(np.int64), members.astype(np.int64), uniq[:, ::-1]


def means(q, vmap, members):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    Vd = len(members)
    # slot of vertex i inside its cluster: its position among the cluster's vertices, ascending i
    order = np.argsort(vmap, kind="stable")
    start = np.concatenate([[0], np.cumsum(members)[:-1]]) if Vd else np.zeros(0, np.int64)
    slot = np.empty(len(vmap), np.int64)
    slot[order] = np.arange(len(vmap)) - start[vmap[order]]
    s = np.zeros((Vd, q.shape[1]), np.float32)  # +0
    for r in range(int(members.max()) if Vd else 0):
        sel = np.nonzero(slot == r)[0]
        s[vmap[sel]] = s[vmap[sel]] + q[sel]
    return s / members.astype(np.float32)[:, None]


def faces(records, vmap):
    rec = np.asarray(records, np.uint32)
    rec = rec.reshape(len(rec), rec.shape[-1] if rec.ndim > 1 else 3)
    if len(rec) == 0:
        return rec.copy(), np.zeros(0, np.int64), 0, 0
    m = vmap[rec[:, :3].astype(np.int64)]
    proper = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    t = np.nonzero(proper)[0]
    # np.unique on the sorted triples: return_index gives the first -- the least t -- of every set
    _, first = np.unique(np.sort(m[t], axis=1), axis=0, return_index=True)
    keep = np.sort(t[first]) if len(t) else np.zeros(0, np.int64)
    out = rec[keep].copy()
    out[:, :3] = m[keep]
    return out, keep, int((~proper).sum()), int(len(t) - len(keep))


def decimate(lattice, records, cell, q=None, col=None):
    vmap, members, _ = clusters(lattice, cell)
    src = np.asarray(lattice if q is None else q, np.float32).reshape(-1, 3)
    out = {"verts": means(src, vmap, members), "members": members.astype(np.int32),
           "map": vmap.astype(np.int32)}
    out["records"], out["keep"], out["degenerate"], out["duplicates"] = faces(records, vmap)
    if col is not None:
        out["rgb"] = means(col, vmap, members)
    return out
