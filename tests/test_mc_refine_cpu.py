"""The refined marching-cubes mesh without a GPU: the numpy restatement of the definition
(tests/mesh_refine.py) against the oracle's mesh, against arithmetic done by hand, and against a
carve of the same scene on a grid eight times finer; and that the entry points exist."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import mesh_refine as mr
from tests import np_restate as npr
from tests import scenes
from tests.test_mc_off import random_coloured_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "arvx", "arvx.h")
F32 = np.float32


def test_midpoints_and_manifold(oracle):
    """B = 0 is midpoint marching cubes over the oracle's triangles."""
    rng = np.random.default_rng(5)
    total = 0
    for X, Y, Z in [(6, 5, 4), (9, 9, 9), (3, 1, 2)]:
        rgba = random_coloured_model(rng, X, Y, Z, False)
        vox = rgba.reshape(Z, Y, X, 4)
        r = mr.refine(vox[..., 3] != 0, F32(0.01), [], [], 0, rgb=vox[..., :3])
        verts, face_rgb = oracle.mc_mesh(X, Y, Z, rgba, 0.5)
        T = len(face_rgb)
        total += T
        assert r["faces"].shape == (T, 3)
        assert np.array_equal(r["face_rgb"], face_rgb.astype(np.int64))
        A = r["edges"][:, :3]
        # every vertex half a step from its occupied end, along its axis, towards the empty end
        off = r["verts"] - A.astype(F32)
        assert np.array_equal(np.abs(off).sum(axis=1), np.full(len(A), 0.5, F32))
        assert (r["cut"] == 1).all() and (r["edges"][:, 3] >= 8).all()
        # the occupied end of corner k of face t is the oracle's snapped vertex 3 t + k
        assert np.array_equal(A[r["faces"]].reshape(-1, 3).astype(F32), verts)
        assert np.array_equal(r["snapped"].reshape(-1, 3).astype(F32), verts)
        f = r["faces"]
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert np.array_equal(np.unique(f), np.arange(len(A)))
    assert total > 500


def test_positions_are_exact_in_fp32():
    """A +- n / 2^(B+1) for B = 10 along a row of 4096: fp32 and fp64 give the same numbers."""
    A = np.arange(4096, dtype=np.int64)[:, None]
    n = np.arange(0, (1 << 11) + 1, dtype=np.int64)[None, :]
    for sgn in (1, -1):
        t32 = (n.astype(F32) / F32(1 << 11)).astype(F32)
        p32 = (A.astype(F32) + F32(sgn) * t32).astype(F32)
        p64 = A.astype(np.float64) + sgn * (n.astype(np.float64) / 2048.0)
        assert np.array_equal(p32.astype(np.float64), p64)
    # and the bisection's own points, mid / 2^B
    mid = np.arange(0, 1 << 10, dtype=np.int64)[None, :]
    p32 = (A.astype(F32) + (mid.astype(F32) / F32(1 << 10)).astype(F32)).astype(F32)
    assert np.array_equal(p32.astype(np.float64), A + mid / 1024.0)


@pytest.mark.parametrize("zoom,c,quarter", [(1, 5, False), (2, 9, True)])
def test_cut_of_a_straight_silhouette(zoom, c, quarter):
    """One view along z with pixel u = zoom * x, foreground the columns u < c; the model is what the
    carve leaves, x <= 4.  Along the edge from x = 4 to x = 5 the pixel is round(zoom * (4 + t)), half
    away from zero, and it stays in the foreground
      zoom 1, c 5: while 4 + t < 4.5, t < 1/2: the last inside point is mid = 2^(B-1) - 1, so
                   n = lo + hi = 2^B - 1 for B >= 1;
      zoom 2, c 9: while 8 + 2 t < 8.5, t < 1/4: mid = 2^(B-2) - 1 for B >= 2, n = 2^(B-1) - 1; for B = 1
                   the one point t = 1/2 is outside: n = 0 + 1.
    B = 0 is the midpoint, n = 1, either way."""
    X, Y, Z = 8, 4, 3
    s = F32(2.0 ** -5)
    M = scenes.flat_view(X, Y, s)
    M[0, 0, 1] *= zoom
    mask = np.zeros((1, Y, zoom * X), np.uint8)
    mask[:, :, :c] = 255
    occ = (npr.carve(X, Y, Z, s, M, mask) & 1).astype(bool)
    assert np.array_equal(occ, np.broadcast_to(np.arange(X) <= 4, (Z, Y, X)))
    for B in range(0, 11):
        r = mr.refine(occ, s, M, mask, B)
        sel = (r["edges"][:, 0] == 4) & ((r["edges"][:, 3] & 7) == 0)
        assert sel.sum() == Y * Z and (r["edges"][sel, 3] == 0).all()  # silhouette edges, towards +x
        if B == 0:
            n = 1
        elif quarter:
            n = 1 if B == 1 else (1 << (B - 1)) - 1
        else:
            n = (1 << B) - 1
        assert (r["cut"][sel] == n).all(), (B, np.unique(r["cut"][sel]), n)
        assert (r["verts"][sel, 0] == F32(4 + n / 2.0 ** (B + 1))).all()
        # the edges out of the image's rows are no silhouette edges: midpoints
        other = (r["edges"][:, 3] & 7) >= 2
        assert other.any() and (r["edges"][other, 3] >= 8).all() and (r["cut"][other] == 1 << B).all()


def test_bisection_moves_the_vertices_towards_the_hull():
    """Sphere scene, N = 16, 8 views of 320 x 240.  The truth is the carve of the same views on a
    grid eight times finer: its signed distance to the boundary between occupied and empty fine
    voxels, sampled at the vertices.  rms: 4 bisections < 1 < 0 (midpoints) < snapped."""
    N, f = 16, 8
    sc = scenes.syn.sphere_scene(N, 8, W=320, H=240)
    s = sc.voxel_size
    occ = (npr.carve(N, N, N, s, sc.M, sc.masks) & 1).astype(bool)
    fine = (npr.carve(N * f, N * f, N * f, F32(s / F32(f)), sc.M, sc.masks) & 1).astype(bool)
    assert occ.any() and fine.any()
    # fine voxel i sits at coarse coordinate i / f; the surface runs half a fine voxel off the centres
    sd = np.where(fine, ndimage.distance_transform_edt(fine) - 0.5,
                  -(ndimage.distance_transform_edt(~fine) - 0.5)) / f

    def rms(p):
        d = ndimage.map_coordinates(sd, (p[:, ::-1] * f).T.astype(np.float64), order=1, mode="nearest")
        return float(np.sqrt((d * d).mean()))

    res = {B: mr.refine(occ, s, sc.M, sc.masks, B) for B in (0, 1, 4)}
    assert res[4]["silhouette"].all()  # every cut edge of a silhouette carve leaves the hull
    err = {B: rms(r["verts"]) for B, r in res.items()}
    snapped = rms(res[0]["edges"][:, :3].astype(F32))
    print("rms distance to the hull (voxels): snapped %.4f, B=0 %.4f, B=1 %.4f, B=4 %.4f"
          % (snapped, err[0], err[1], err[4]))
    assert err[4] < err[1] < err[0] < snapped


def test_header_declarations_are_bound_and_exported(arvx):
    """The two entry points are declared, exported by the built libarvx.so and bound in capi.py."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(arvx_mc_mesh_refined[a-z_0-9]*)\s*\(", text)))
    assert names == ["arvx_mc_mesh_refined", "arvx_mc_mesh_refined_download"]
    lib = arvx.load_library()
    for n in names:
        assert n in arvx.SYMBOLS
        fn = getattr(lib, n)
        assert fn.argtypes is not None and fn.argtypes[0] is ctypes.c_void_p and fn.restype is ctypes.c_int, n
    # the argument checks need no GPU
    assert lib.arvx_mc_mesh_refined(None, 0, 6, None, None) == 1 and b"null" in lib.arvx_last_error()
    assert lib.arvx_mc_mesh_refined_download(None, None, None, None, None, None) == 1
    for m in ("mc_mesh_refined", "mc_mesh_refined_count"):
        assert callable(getattr(arvx.Context, m))
