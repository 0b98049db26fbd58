"""The triangle render's definition (include/arvx/arvx.h) as tests/render_mesh.py restates it, on
hand-made meshes: shared edges, windings, fronto-parallel depth, the four classes, headlight.  No
GPU; tests/test_render_mesh_gpu.py draws the same meshes on the device."""
import numpy as np

from tests import render_mesh as rm

F32 = np.float32
# s = 1 and this camera: a0 = x, a1 = y, a2 = z of a vertex (x, y, z), so it lands on pixel (x / z, y / z)
S1 = F32(1.0)
M_XYZ = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, -1, 0]], F32)
W, H = 16, 14


def square():
    """Two triangles sharing the diagonal of the square of pixels [2, 10] x [3, 11], at depth 1."""
    verts = np.array([[2, 3, 1], [10, 3, 1], [10, 11, 1], [2, 11, 1]], F32)
    rgb = np.array([[10, 20, 30], [200, 20, 30], [200, 220, 30], [10, 220, 250]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return verts, rgb, faces


def slanted():
    """One triangle whose corners lie at depths 1, 2 and 4: every 1 / a2 and every weight is exact."""
    verts = np.array([[1, 1, 1], [26, 4, 2], [12, 48, 4]], F32)
    rgb = np.array([[255, 0, 0], [0, 128, 0], [0, 0, 64]], F32)
    return verts, rgb, np.array([[0, 1, 2]], np.uint32)


def fronto(z=F32(3.7)):
    """One triangle in the plane z."""
    q = np.array([[1.3, 0.8], [13.9, 2.1], [6.2, 12.4]], F32)
    verts = np.concatenate([q * z, np.full((3, 1), z, F32)], axis=1).astype(F32)
    rgb = np.array([[255, 10, 0], [0, 255, 10], [10, 0, 255]], F32)
    return verts, rgb, np.array([[0, 1, 2]], np.uint32)


def classes():
    """A drawn triangle, one with a corner behind the camera, one with collinear corners and one that
    lies between the pixel centres: faces 0 .. 3."""
    verts = np.array([[1, 1, 1], [6, 1, 1], [1, 6, 1],         # drawn
                      [8, 1, 1], [12, 1, 1], [10, 5, -1],      # a corner behind the camera
                      [1, 8, 1], [4, 10, 1], [7, 12, 1],       # collinear
                      [9.2, 9.2, 1], [9.7, 9.2, 1], [9.2, 9.7, 1]], F32)  # between the centres
    rgb = np.full((12, 3), 90, F32)
    return verts, rgb, np.arange(12, dtype=np.uint32).reshape(4, 3)


HAND_MESHES = {"square": square, "slanted": slanted, "fronto": fronto, "classes": classes}


def test_shared_diagonal_has_no_gap_and_the_lesser_face_wins():
    verts, rgb, faces = square()
    res = rm.render(M_XYZ, S1, verts, rgb, faces, W, H)
    ids = res.image.id
    inside = np.zeros((H, W), bool)
    inside[3:12, 2:11] = True
    assert np.array_equal(ids >= 0, inside)  # every pixel of the square, edges included, and no other
    assert res.counts == (2, 0, 0, 0)
    r, c = np.nonzero(inside)
    diag = (c - 2) == (r - 3)
    assert np.all(ids[r[diag], c[diag]] == 0)  # both faces cover the diagonal at depth 1: the lesser t
    assert np.all(ids[r[(c - 2) > (r - 3)], c[(c - 2) > (r - 3)]] == 0)
    assert np.all(ids[r[(c - 2) < (r - 3)], c[(c - 2) < (r - 3)]] == 1)
    assert np.all(res.image.depth[inside] == F32(1.0)) and np.all(np.isinf(res.image.depth[~inside]))
    # each face alone covers the diagonal too
    for t in range(2):
        alone = rm.render(M_XYZ, S1, verts, rgb, faces[t:t + 1], W, H).image.id
        assert np.all(alone[r[diag], c[diag]] == 0)
    # the corners take their vertex's colour, stored B, G, R
    assert tuple(res.image.bgr[3, 2]) == (30, 20, 10) and tuple(res.image.bgr[11, 10]) == (30, 220, 200)


def test_winding_changes_nothing_but_the_order_of_the_colour_sum():
    """(i0, i1, i2) -> (i0, i2, i1): A and the E change sign and are negated back, E1 and E2 swap
    with their corners.  On a mesh whose weights are exact in fp64 the sums do not depend on their
    order, so the images are the same bit for bit."""
    for mesh in (square, slanted):
        verts, rgb, faces = mesh()
        Wm, Hm = (16, 14) if mesh is square else (28, 26)
        a = rm.render(M_XYZ, S1, verts, rgb, faces, Wm, Hm, light=(1, 2, 3))
        b = rm.render(M_XYZ, S1, verts, rgb, faces[:, [0, 2, 1]], Wm, Hm, light=(1, 2, 3))
        assert a.counts == b.counts and (a.image.id >= 0).any()
        assert np.array_equal(a.image.id, b.image.id)
        assert np.array_equal(a.image.depth.view(np.uint32), b.image.depth.view(np.uint32))
        assert np.array_equal(a.image.bgr, b.image.bgr)


def test_fronto_parallel_depth_is_z_to_one_ulp():
    """S = sum(E_i / z) and depth = A / S: two roundings of 2^-53 each on top of 1 / z's, so the
    fp32 result is z or a neighbour of it."""
    for z in (F32(3.7), F32(0.013), F32(977.3)):
        verts, rgb, faces = fronto(z)
        res = rm.render(M_XYZ, S1, verts, rgb, faces, W, H)
        cov = res.image.id >= 0
        assert res.counts == (1, 0, 0, 0) and np.count_nonzero(cov) > 40
        ulps = np.abs(res.image.depth[cov].view(np.int32).astype(np.int64) - int(z.view(np.int32)))
        assert ulps.max() <= 1


def test_the_four_classes():
    verts, rgb, faces = classes()
    res = rm.render(M_XYZ, S1, verts, rgb, faces, W, H)
    assert list(res.classes) == [rm.DRAWN, rm.REFUSED, rm.FLAT, rm.EMPTY_CLASS]
    assert res.counts == (1, 1, 1, 1)
    assert set(np.unique(res.image.id)) == {-1, 0}
    # the drawn one: the closed triangle x, y >= 1, x + y <= 7
    r, c = np.mgrid[0:H, 0:W]
    assert np.array_equal(res.image.id == 0, (c >= 1) & (r >= 1) & (c + r <= 7))
    # a triangle off the image is EMPTY as well, and one beyond 32768 pixels REFUSED
    far = np.array([[40, 1, 1], [44, 1, 1], [40, 5, 1], [40000, 1, 1], [1, 2, 1], [2, 1, 1]], F32)
    res = rm.render(M_XYZ, S1, far, rgb[:6], [[0, 1, 2], [3, 4, 5]], W, H)
    assert res.counts == (0, 1, 0, 1) and np.all(res.image.id == -1)


def test_background_and_empty_mesh():
    bg = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)
    res = rm.render(M_XYZ, S1, np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), W, H,
                    background=bg)
    assert np.array_equal(res.image.bgr, bg) and np.all(res.image.id == -1) and res.counts == (0, 0, 0, 0)
    verts, rgb, faces = square()
    res = rm.render(M_XYZ, S1, verts, rgb, faces, W, H, background=bg)
    assert np.array_equal(res.image.bgr[res.image.id < 0], bg[res.image.id < 0])


def test_light():
    """The square faces the camera: lit along z it keeps its colours, lit along x it keeps a quarter."""
    verts, rgb, faces = square()
    rgb = np.full_like(rgb, 200)
    plain = rm.render(M_XYZ, S1, verts, rgb, faces, W, H).image.bgr
    front = rm.render(M_XYZ, S1, verts, rgb, faces, W, H, light=(0, 0, -5)).image.bgr
    side = rm.render(M_XYZ, S1, verts, rgb, faces, W, H, light=(3, 0, 0)).image.bgr
    dark = rm.render(M_XYZ, S1, verts, rgb, faces, W, H, light=(0, 0, 0)).image.bgr
    assert np.array_equal(front, plain) and np.array_equal(dark, plain)
    assert np.array_equal(side, plain // 4) and plain.max() == 200


def test_headlight():
    M = np.arange(12, dtype=F32).reshape(3, 4)
    assert np.array_equal(rm.headlight(M), np.array([9, 8, -10], F32))
    from ar_voxel_project_amd import capi
    assert np.array_equal(capi.headlight(M), rm.headlight(M))
    assert np.array_equal(rm.headlight(M_XYZ), np.array([0, 0, 1], F32))  # the camera looks along +z
