"""The view windows (arvx.h, arvx_view_window_host) against a numpy restatement of rect_prepare
(tests/rect_window.py): every rectangle with which a carve kernel would read a view's summed-area
table -- coarse tiles of contiguous and of striped slabs, sub-tiles and 4 x 4 x 4 blocks of the
whole grid, on the raster of the grid and on that of a slab that starts at plane 5 -- lies inside
the part of the table the library says it writes.  Needs no GPU: the window is host arithmetic."""
import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import rect_window as rw
from tests import scenes

E = 0.512
GRIDS = [(24, 40, 16), (64, 64, 64)]
IMAGES = [(192, 160), (640, 480)]


def cameras(kind, W, H):
    if kind == "sphere":
        return np.asarray(syn.sphere_scene(32, 8, W=W, H=H).M, np.float32), None
    _, Rt, M = scenes.random_cameras(10, E, seed=71 if kind == "inside" else 72, W=W, H=H, inside=kind == "inside")
    # camera centres in world coordinates: -R^T t
    centres = -np.einsum("vji,vj->vi", Rt[:, :, :3].astype(np.float64), Rt[:, :, 3].astype(np.float64))
    return M, centres


def whole(W, H):
    return (0, H, 0, (W + 1 + 63) // 64 * 64 - 1)


def all_boxes(X, Y, Z):
    out = []
    for name, size in rw.BOX_SIZES.items():
        out.append((name, rw.grid_boxes(X, Y, Z, size)))
        if Z > 5:  # a slab whose first plane (halo included) is 5: its raster starts there
            b = rw.grid_boxes(X, Y, Z - 5, size)
            b[:, 4:] += 5
            out.append((name + ", slab from plane 5", b))
    return out


@pytest.mark.parametrize("W,H", IMAGES)
@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("kind", ["outside", "inside", "sphere"])
def test_every_rectangle_lies_in_the_window(arvx, kind, dims, W, H):
    X, Y, Z = dims
    s = np.float32(E / max(dims))
    M, centres = cameras(kind, W, H)
    boxes = all_boxes(X, Y, Z)
    reads = 0
    partial = 0
    for v in range(len(M)):
        r0, r1, c0, c1 = arvx.view_window_host(X, Y, Z, s, M[v], W, H)
        assert 0 <= r0 <= r1 <= H and 0 <= c0 <= c1 <= whole(W, H)[3], (v, r0, r1, c0, c1)
        # whole tiles: strip I holds the rows 64 I + 1 .. 64 I + 64 (strip 0 also row 0)
        assert (r0 == 0 or (r0 - 1) % 64 == 0) and (r1 == H or r1 % 64 == 0), (v, r0, r1)
        assert c0 % 64 == 0 and c1 % 64 == 63, (v, c0, c1)
        partial += (r0, r1, c0, c1) != whole(W, H)
        for name, b in boxes:
            rd, pxlo, pxhi, pylo, pyhi = rw.rectangles(M[v], b, s, W, H)
            reads += int(rd.sum())
            bad = rd & ((pylo < r0) | (pyhi + 1 > r1) | (pxlo < c0) | (pxhi + 1 > c1))
            assert not bad.any(), (f"view {v}, {name}: box {b[bad][0]} reads rows {pylo[bad][0]}..{pyhi[bad][0] + 1}, "
                                   f"columns {pxlo[bad][0]}..{pxhi[bad][0] + 1}; window {(r0, r1, c0, c1)}")
    assert reads > 0, "no rectangle reads a table: the scene tests nothing"
    if kind != "inside":
        assert partial > 0, "every view takes its whole table: the scene tests nothing"


@pytest.mark.parametrize("W,H", IMAGES)
def test_camera_inside_the_grid_takes_the_whole_table(arvx, W, H):
    X = Y = Z = 64
    s = np.float32(E / 64)
    M, centres = cameras("inside", W, H)
    hi = float(s) * 63
    inside = ((centres[:, 0] > 0) & (centres[:, 0] < hi) & (centres[:, 1] > 0) & (centres[:, 1] < hi) &
              (centres[:, 2] < 0) & (centres[:, 2] > -hi))
    assert inside.any(), "no camera inside the grid"
    for v in np.flatnonzero(inside):
        assert arvx.view_window_host(X, Y, Z, s, M[v], W, H) == whole(W, H), v


def test_window_follows_the_camera(arvx):
    """The benchmark's kind of scene: a ring of cameras at twice the extent sees the grid in the
    middle of 640 x 480, and the window leaves out tile columns on both sides in every view and
    strips in most: the tiles written are fewer than two thirds of all."""
    sc = syn.sphere_scene(64, 6)
    tiles = 0
    for v in range(6):
        r0, r1, c0, c1 = arvx.view_window_host(64, 64, 64, sc.voxel_size, sc.M[v], 640, 480)
        assert c0 > 0 and c1 < 640, (v, r0, r1, c0, c1)
        tiles += ((r1 - 1) // 64 - max(r0 - 1, 0) // 64 + 1) * (c1 // 64 - c0 // 64 + 1)
    assert tiles * 3 < 6 * 8 * 11 * 2, tiles


def test_refusals(arvx):
    import ctypes
    lib = arvx.load_library()
    rect = (ctypes.c_int * 4)(7, 7, 7, 7)
    M = (ctypes.c_float * 12)()
    assert lib.arvx_view_window_host(8, 8, 8, 0.1, None, 64, 64, rect) == 1  # ARVX_ERR_INVALID
    assert lib.arvx_view_window_host(0, 8, 8, 0.1, M, 64, 64, rect) == 1
    assert lib.arvx_view_window_host(8, 8, 8, 0.1, M, 0, 64, rect) == 1
    assert lib.arvx_view_window(None, 0, rect) == 1
    assert lib.arvx_ctx_set_view_window(None, 1) == 1
    assert lib.arvx_selftest_fill_view_tables(None, 0) == 1
    assert list(rect) == [7, 7, 7, 7]  # (a refused call writes nothing)
    assert {"arvx_ctx_set_view_window", "arvx_view_window", "arvx_view_window_host"} <= set(arvx.SYMBOLS)
