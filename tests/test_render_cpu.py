"""The render's numpy restatement (tests/render.py) against its own definition: the depth image is
the visible colour pass's depth buffer, a voxel paints its footprint, the nearer voxel and then the
lower index win, and the three images agree on which pixels are empty."""
import numpy as np
import pytest

from tests import np_restate as npr
from tests import render as rnd
from tests import scenes
from tests import visibility as vis

W, H = 64, 48


def _random_block(N, seed):
    rng = np.random.default_rng(seed)
    occ = rng.random((N, N, N)) < 0.6
    index = rnd.vertex_voxels(N, N, N, occ)
    col = rng.integers(0, 256, (len(index), 3)).astype(np.float32)
    return index, col


@pytest.mark.parametrize("assoc_left", [True, False])
@pytest.mark.parametrize("inside", [False, True])
def test_depth_image_is_the_depth_buffer(inside, assoc_left):
    N = 8
    s = np.float32(0.512 / N)
    index, col = _random_block(N, 0)
    x, y, z = index % N, (index // N) % N, index // (N * N)
    _, _, M = scenes.random_cameras(6, 0.512, seed=2, W=W, H=H, inside=inside)
    some = 0
    for v in range(6):
        got = rnd.render(M[v], s, index, col, N, N, W, H, assoc_left=assoc_left)
        want = vis.depth_buffer(M[v], s, x, y, z, W, H, assoc_left)
        assert np.array_equal(got.depth.view(np.uint32), want.view(np.uint32))
        some += np.count_nonzero(got.id >= 0)
    assert some > 0


def _axis_camera(scale, a2):
    """u = scale * w1 / a2, v = scale * w0 / a2 with a constant a2: an orthographic view along z
    (world w0 = y * s, w1 = x * s)."""
    M = np.zeros((3, 4), np.float32)
    M[0, 1] = scale * a2
    M[1, 0] = scale * a2
    M[2, 3] = a2
    return M


def test_single_voxel_paints_exactly_its_footprint():
    N = 4
    s = np.float32(1.0)
    M = _axis_camera(8.0, 1.0)
    index = np.array([(1 * N + 2) * N + 1])  # voxel (x, y, z) = (1, 2, 1)
    bg = np.random.default_rng(1).integers(0, 256, (H, W, 3)).astype(np.uint8)
    got = rnd.render(M, s, index, [[10.0, 20.4, 300.0]], N, N, W, H, background=bg)
    ok, c0, c1, r0, r1 = vis.footprint(M, s, np.array([1]), np.array([2]), np.array([1]), W, H)
    assert ok[0] and (c0[0], c1[0], r0[0], r1[0]) == (4, 12, 12, 20)  # corners at 8 * (x, y -+ 0.5)
    inside = np.zeros((H, W), bool)
    inside[12:21, 4:13] = True
    assert np.array_equal(got.id, np.where(inside, 0, -1))
    assert np.array_equal(got.depth, np.where(inside, np.float32(1.0), np.float32(np.inf)))
    assert np.array_equal(got.bgr, np.where(inside[..., None], np.array([255, 20, 10], np.uint8), bg))


def test_nearer_voxel_wins_on_one_ray():
    """Two voxels on the camera's axis: a2 = 3 + w2 = 3 - z * s, so the higher z is nearer."""
    N = 4
    s = np.float32(1.0)
    M = np.zeros((3, 4), np.float32)
    M[0, 1] = M[1, 0] = 8.0
    M[0, 3] = M[1, 3] = 0.0
    M[2, 2], M[2, 3] = 1.0, 6.0  # a2 = 6 - z
    index = np.array([(0 * N + 1) * N + 1, (2 * N + 1) * N + 1])  # (1, 1, 0) and (1, 1, 2)
    col = np.array([[255, 0, 0], [0, 255, 0]], np.float32)
    got = rnd.render(M, s, index, col, N, N, W, H)
    # the far voxel's footprint is the smaller one and lies inside the near one's
    far = rnd.render(M, s, index[:1], col[:1], N, N, W, H)
    near = rnd.render(M, s, index[1:], col[1:], N, N, W, H)
    assert np.count_nonzero(far.id >= 0) > 0
    assert np.all(near.id[far.id >= 0] >= 0)
    assert np.array_equal(got.id, np.where(near.id >= 0, 1, -1))
    assert np.all(got.depth[got.id == 1] == np.float32(4.0))
    assert np.all(got.bgr[got.id == 1] == np.array([0, 255, 0], np.uint8))


def test_equal_depths_lower_index_wins():
    N = 8
    s = np.float32(1.0)
    M = _axis_camera(4.5, 1.0)  # footprints of x-neighbours overlap by a pixel or two
    occ = np.ones((N, N, N), bool)
    index = rnd.vertex_voxels(N, N, N, occ)
    col = np.zeros((len(index), 3), np.float32)
    got = rnd.render(M, s, index, col, N, N, W, H)
    x, y, z = index % N, (index // N) % N, index // (N * N)
    ok, c0, c1, r0, r1 = vis.footprint(M, s, x, y, z, W, H)
    assert ok.all()
    best = np.full((H, W), -1, np.int64)
    for k in range(len(index) - 1, -1, -1):  # descending, so the least k is written last
        best[r0[k]:r1[k] + 1, c0[k]:c1[k] + 1] = k
    assert np.array_equal(got.id, best)
    covered = got.id >= 0
    overlap = np.zeros((H, W), np.int64)
    for k in range(len(index)):
        overlap[r0[k]:r1[k] + 1, c0[k]:c1[k] + 1] += 1
    assert overlap.max() > 2 and np.all(got.depth[covered] == np.float32(1.0))


def test_empty_pixels_agree_in_all_three_images():
    N = 6
    s = np.float32(0.512 / N)
    index, col = _random_block(N, 3)
    col += 1.0  # (no vertex is black: a covered pixel differs from the zero background)
    col = np.minimum(col, 255.0)
    _, _, M = scenes.random_cameras(4, 0.512, seed=5, W=W, H=H)
    bg = np.random.default_rng(2).integers(0, 256, (H, W, 3)).astype(np.uint8)
    for v in range(4):
        plain = rnd.render(M[v], s, index, col, N, N, W, H)
        over = rnd.render(M[v], s, index, col, N, N, W, H, background=bg)
        empty = plain.id == -1
        assert 0 < np.count_nonzero(empty) < empty.size
        assert np.array_equal(empty, np.isinf(plain.depth))
        assert np.array_equal(empty, (plain.bgr == 0).all(axis=-1))
        assert np.array_equal(over.id, plain.id)
        assert np.array_equal(over.bgr[empty], bg[empty])
        assert np.array_equal(over.bgr[~empty], plain.bgr[~empty])
    assert np.array_equal(rnd.render(M[0], s, index[:0], col[:0], N, N, W, H, background=bg).bgr, bg)


def test_agreement_counts():
    ids = np.array([[0, -1, 3], [-1, -1, 7]])
    mask = np.array([[255, 0, 0], [9, 0, 1]], np.uint8)
    assert rnd.agreement(ids, mask) == (2, 1, 1)
    assert rnd.agreement(ids, np.stack([mask * 0, mask, mask * 0], axis=-1)) == (2, 1, 1)
