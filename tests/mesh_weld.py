"""The welded marching-cubes mesh (arvx_mc_mesh_welded, include/arvx/arvx.h) restated in numpy.

weld(verts, face_rgb): from an unwelded mesh -- triangle t has the vertices verts[3t .. 3t+2] --
to (vertices, faces, face_rgb): the distinct positions, compared as float values, ascending by
(z, y, x); faces[t][k] = index of verts[3t + k] in that list; the colours unchanged."""
import numpy as np


def weld(verts, face_rgb):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    assert len(v) == 3 * len(face_rgb)
    order = np.lexsort((v[:, 0], v[:, 1], v[:, 2]))  # last key first: z, then y, then x
    s = v[order]
    new = np.ones(len(s), bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)  # (float comparison: -0.0 == 0.0)
    rank = np.cumsum(new) - 1
    index = np.empty(len(v), np.int64)
    index[order] = rank
    return s[new], index.reshape(-1, 3).astype(np.uint32), np.asarray(face_rgb).astype(np.uint32)


def unweld(vertices, faces):
    """The unwelded vertex array (3T, 3) the welded mesh stands for."""
    return np.asarray(vertices)[np.asarray(faces, np.int64).reshape(-1)]


def lattice_index(vertices, X, Y):
    """Flat voxel index x + X (y + Y z) of lattice vertices (the device path's)."""
    lat = np.asarray(vertices).astype(np.int64)
    assert np.array_equal(lat.astype(np.float32), vertices)
    return lat[:, 0] + X * (lat[:, 1] + Y * lat[:, 2])


def surface_voxels(occ):
    """Occupied voxels with an empty 6-neighbour (outside the grid is empty), ascending flat
    index; occ: (Z, Y, X) bool."""
    p = np.pad(occ, 1)
    inner = occ.copy()
    for ax in range(3):
        for d in (1, -1):
            inner &= np.roll(p, d, axis=ax)[1:-1, 1:-1, 1:-1]
    return np.flatnonzero((occ & ~inner).ravel())
