"""The triangle render's near plane (arvx_ctx_set_render_near; include/arvx/arvx.h) as
tests/render_mesh_clip.py restates it, on hand-made meshes: a camera inside a closed box, constant
colours, the depth bound, a clipped vertex beyond the valid range, both piece shapes in both windings.
No GPU; tests/test_render_mesh_clip_gpu.py draws the box and the hand-made faces on the device."""
import numpy as np

from tests import render_mesh as rm
from tests import render_mesh_clip as rmc
from tests.test_render_mesh_cpu import HAND_MESHES, M_XYZ, S1

F32 = np.float32
BOX_W, BOX_H = 40, 30
# a0 = 10 x + 19.5 z, a1 = 10 y + 14.5 z, a2 = z: a pinhole at the origin that looks along +z
M_BOX = np.array([[0, 10, -19.5, 0], [10, 0, -14.5, 0], [0, 0, -1, 0]], F32)
BOX_EDGE = 2.0
BOX_NEAR = BOX_EDGE / 100


def box(colour=(200, 100, 50)):
    """A closed axis-aligned box of 12 triangles, edge 2, centred on the origin: the camera of M_BOX
    stands at its centre."""
    verts = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    rgb = np.tile(np.array(colour, F32), (8, 1))
    return verts, rgb, faces


def same_images(a, b):
    return np.array_equal(a.bgr, b.bgr) and np.array_equal(a.id, b.id) and \
        np.array_equal(a.depth.view(np.uint32), b.depth.view(np.uint32))


def test_a_plane_in_front_of_every_corner_changes_nothing():
    for name in ("square", "slanted", "fronto"):
        verts, rgb, faces = HAND_MESHES[name]()
        Wm, Hm = (16, 14) if name != "slanted" else (28, 26)
        want = rm.render(M_XYZ, S1, verts, rgb, faces, Wm, Hm, light=(0.3, -1.0, 0.5))
        got = rmc.render(M_XYZ, S1, verts, rgb, faces, Wm, Hm, near=0.5, light=(0.3, -1.0, 0.5))
        assert same_images(got.image, want.image), name
        assert got.counts == want.counts and np.array_equal(got.classes, want.classes)
        assert got.clip == (0, 0, 0, 0) and (got.pieces.front == 3).all()
    # near = 0 is the render without a plane
    verts, rgb, faces = HAND_MESHES["classes"]()
    off = rmc.render(M_XYZ, S1, verts, rgb, faces, 16, 14)
    assert same_images(off.image, rm.render(M_XYZ, S1, verts, rgb, faces, 16, 14).image) and off.clip == (0,) * 4


def test_a_camera_inside_a_closed_box_sees_no_hole():
    """Watertightness: the clipped vertex of a shared edge is computed from the edge's ends in index
    order, so both faces get the same fixed-point corner and the inclusive edges leave no pixel out."""
    verts, rgb, faces = box()
    res = rmc.render(M_BOX, S1, verts, rgb, faces, BOX_W, BOX_H, near=BOX_NEAR)
    assert (res.image.id >= 0).all()
    assert not (res.pieces.cls == rm.REFUSED).any()
    behind, straddle, made, drawn = res.clip
    assert behind == 2 and straddle == 8 and made == 12  # (the wall behind; 4 one-front, 4 two-front)
    assert sum(res.counts) == 12 and res.counts[rm.REFUSED] == 2
    off = rm.render(M_BOX, S1, verts, rgb, faces, BOX_W, BOX_H)
    assert (off.image.id < 0).any() and off.counts[rm.REFUSED] == 10
    assert np.count_nonzero(res.image.id >= 0) > np.count_nonzero(off.image.id >= 0)


def test_a_constant_colour_stays_constant_and_no_depth_is_nearer_than_the_plane():
    colour = (200, 100, 50)
    verts, rgb, faces = box(colour)
    res = rmc.render(M_BOX, S1, verts, rgb, faces, BOX_W, BOX_H, near=BOX_NEAR)
    assert (res.image.bgr.reshape(-1, 3) == np.array(colour[::-1], np.uint8)).all()
    # S <= A / near up to one fp64 rounding per term, then one fp32 rounding
    bound = F32(BOX_NEAR) * (F32(1) - F32(2.0 ** -23))
    assert (res.image.depth >= bound).all()
    # a face that passes the camera closely: its pieces start on the plane, inside the picture
    verts = np.array([[-0.5, -0.3, -1], [0.54, 0.34, 1], [0.46, 0.4, 1]], F32)
    res = rmc.render(M_BOX, S1, verts, rgb[:3], np.array([[0, 1, 2]]), BOX_W, BOX_H, near=BOX_NEAR)
    covered = res.image.id >= 0
    assert covered.any() and res.image.depth.min() < 2 * BOX_NEAR
    assert (res.image.depth >= bound).all()
    assert (res.image.bgr[covered] == np.array(colour[::-1], np.uint8)).all()


def test_a_clipped_vertex_beyond_the_valid_range_refuses_the_piece():
    near = F32(rm.FLT_MIN) * F32(4)
    verts = np.array([[1, 1, 1], [1, 1, -1], [2, 1, -1]], F32)
    rgb = np.full((3, 3), 90, F32)
    faces = np.array([[0, 1, 2]], np.uint32)
    res = rmc.render(M_XYZ, S1, verts, rgb, faces, 16, 14, near=near)
    assert res.clip == (0, 1, 1, 0)
    assert res.pieces.cls.tolist() == [rm.REFUSED] and res.counts == (0, 0, 0, 1)
    assert (res.image.id < 0).all()
    _, _, valid, _, (qu, _) = rmc.clipped_vertex(
        [verts[:, 0].copy(), verts[:, 1].copy(), verts[:, 2].copy()], 0, 1, near)
    assert not valid and not abs(qu) <= 32768


def dyadic():
    """A one-front face and a two-front face whose every quantity is exact with near = 0.5: corners at
    depths 1 and -1 (t is 0.25 or 0.75), small integer positions."""
    verts = np.array([[2, 2, 1], [6, 2, -1], [2, 6, -1],       # one corner in front
                      [8, 4, 1], [12, 4, 1], [10, 8, -1]], F32)  # two in front
    rgb = np.array([[255, 0, 0], [0, 128, 0], [0, 0, 64], [64, 0, 32], [0, 16, 8], [128, 128, 0]], F32)
    return verts, rgb, np.array([[0, 1, 2], [3, 4, 5]], np.uint32)


def test_both_piece_shapes_in_both_windings():
    """Reversing a face's winding changes what it changes without a plane -- the signs, which are
    negated back, and the order of the sums -- and, for two corners in front, which diagonal splits
    the quadrilateral.  On a mesh whose weights are exact in fp64 neither shows: the images are equal."""
    verts, rgb, faces = dyadic()
    res = rmc.render(M_XYZ, S1, verts, rgb, faces, 30, 20, near=0.5, light=(0.2, 0.4, -1.0))
    assert res.pieces.front.tolist() == [1, 2, 2] and res.pieces.k.tolist() == [0, 0, 1]
    assert res.clip == (0, 2, 3, 3) and res.counts == (2, 0, 0, 0)
    assert set(np.unique(res.image.id)) == {-1, 0, 1}
    for perm in ((0, 2, 1), (1, 0, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1)):
        other = rmc.render(M_XYZ, S1, verts, rgb, faces[:, perm], 30, 20, near=0.5, light=(0.2, 0.4, -1.0))
        assert other.clip == res.clip and other.counts == res.counts, perm
        assert same_images(other.image, res.image), perm
    # the same faces at every rotation and winding of their vertex NUMBERS too (lo and hi swap)
    order = np.array([5, 3, 1, 4, 2, 0])
    inv = np.argsort(order)
    other = rmc.render(M_XYZ, S1, verts[order], rgb[order], inv[faces.astype(np.int64)], 30, 20, near=0.5,
                       light=(0.2, 0.4, -1.0))
    assert same_images(other.image, res.image) and other.clip == res.clip
