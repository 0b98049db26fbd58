"""The numpy restatement of the visible colour pass (tests/visibility.py) on its own, without a GPU:
it is the plain pass at tol = inf, it hides what lies behind, it does not splat voxels that reach
behind a camera, and on the sphere it takes each voxel's colour from a camera on its own side."""
import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import np_restate as npr
from tests import visibility as vis
from tests.visibility import constant_images, own_side_share, view_colours, view_of_colour


@pytest.mark.parametrize("mode", [0, 1])
def test_infinite_tolerance_is_the_plain_pass(oracle, mode):
    sc = syn.sphere_scene(32, 6, W=160, H=120, with_images=True)
    st = oracle.carve(32, 32, 32, sc.voxel_size, sc.M, sc.masks)
    model = oracle.model_from_state(st)
    got = vis.color_visible(32, 32, 32, sc.voxel_size, sc.M, sc.campos, sc.images, mode, model, np.inf)
    want = npr.color(32, 32, 32, sc.voxel_size, sc.M, sc.campos, sc.images, mode, model)
    assert np.array_equal(got.rgba, want)
    assert np.array_equal(want, oracle.color(32, 32, 32, sc.voxel_size, sc.M, sc.campos, sc.images,
                                             mode, model))
    assert np.all(got.views[got.has] > 0)  # (every voxel is in front of every camera here)


def _axis_views(d_front, d_back, f=8.0, cx=8.0, cy=8.0):
    """View 0 looks along +z (voxel z at depth z + d_front), view 1 along -z from beyond z = 3
    (voxel z at depth d_back - z); s = 1, both through the voxel column x = y = 0."""
    M = np.array([[[f, 0, -cx, cx * d_front], [0, f, -cy, cy * d_front], [0, 0, -1, d_front]],
                  [[f, 0, cx, cx * d_back], [0, f, cy, cy * d_back], [0, 0, 1, d_back]]], np.float32)
    campos = np.array([[0, 0, d_front], [0, 0, d_back]], np.float32)
    return M, campos


def _column_model(zs, Z=4):
    rgba = np.zeros((Z, 1, 1, 4), np.float32)
    rgba[list(zs), 0, 0, 3] = 1.0
    return rgba.reshape(-1, 4)


@pytest.mark.parametrize("mode", [0, 1])
def test_the_voxel_behind_is_hidden(mode):
    """Two voxels on one camera ray: in each view the front one is visible, the back one is not."""
    M, campos = _axis_views(5.0, 8.0)
    images = constant_images(2, 16, 16)
    rgba = _column_model((0, 3))
    got = vis.color_visible(1, 1, 4, 1.0, M, campos, images, mode, rgba, 1.0)
    assert list(got.index) == [0, 3]
    assert list(got.views) == [1, 1]
    rgb = view_colours(2).astype(np.float32)
    assert np.array_equal(got.rgba[0, :3], rgb[0]) and np.array_equal(got.rgba[3, :3], rgb[1])
    z0 = got.zbuf[0]
    assert z0[8, 8] == np.float32(5.0) and z0[0, 0] == np.inf
    assert got.zbuf[1][8, 8] == np.float32(5.0)  # voxel 3 is at depth 8 - 3
    # the plain pass mixes both views into both voxels
    plain = npr.color(1, 1, 4, np.float32(1.0), M, campos, images, mode, rgba)
    if mode == 1:
        assert np.array_equal(plain[0, :3], plain[3, :3])
    # with a tolerance above the gap (3) both are visible in both views again: the plain pass
    wide = vis.color_visible(1, 1, 4, 1.0, M, campos, images, mode, rgba, 3.5)
    assert list(wide.views) == [2, 2] and np.array_equal(wide.rgba, plain)


def test_a_voxel_reaching_behind_the_camera_does_not_splat():
    M, campos = _axis_views(0.3, 8.0)  # voxel 0 spans depths -0.2 .. 0.8 in view 0
    ok, *_ = vis.footprint(M[0], 1.0, np.array([0, 0]), np.array([0, 0]), np.array([0, 3]), 16, 16)
    assert list(ok) == [False, True]
    rgba = _column_model((0, 3))
    got = vis.color_visible(1, 1, 4, 1.0, M, campos, constant_images(2, 16, 16), 0, rgba, 0.0)
    # view 0: only voxel 3 splats, so it is visible there; voxel 0's centre (depth 0.3) projects
    # to pixel (8, 8), which voxel 3 covers from depth 3.3: voxel 0 is nearer, visible too
    assert got.zbuf[0][8, 8] == np.float32(3.3)
    assert got.views[0] == 1 + 0 and got.views[1] == 2


def _sphere_votes(N=40, V=12, tol_voxels=3.0):
    sc = syn.sphere_scene(N, V, W=160, H=120)
    images = constant_images(V, 160, 120)
    st = npr.carve(N, N, N, sc.voxel_size, sc.M, sc.masks)
    model = np.zeros((N ** 3, 4), np.float32)
    model[:, 3] = (st.reshape(-1) & 1).astype(np.float32)
    tol = np.float32(tol_voxels) * sc.voxel_size
    got = vis.color_visible(N, N, N, sc.voxel_size, sc.M, sc.campos, images, 0, model, tol)
    return sc, images, model, got


def test_closest_colour_comes_from_the_voxels_own_side():
    sc, images, model, got = _sphere_votes()
    V = sc.V
    sel = got.has & (got.views > 0)
    idx = got.index[sel]
    chosen = view_of_colour(got.rgba[idx, :3], V)
    assert np.all(chosen >= 0)
    share = own_side_share(sc, idx, chosen)
    assert share >= 0.99, share
    plain = npr.color(sc.X, sc.Y, sc.Z, sc.voxel_size, sc.M, sc.campos, images, 0, model)
    pchosen = view_of_colour(plain[idx, :3], V)
    assert own_side_share(sc, idx, pchosen) < share - 0.2
