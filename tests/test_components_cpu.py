"""The numpy restatement of the connected components (tests/components.py) against
scipy.ndimage.label: labels as least flat index, the table and the keep rule, on the hand-built
states and on the carved three-ball scenes (through the CPU oracle) the device tests use -- with the
figures measured for those scenes."""
import numpy as np
import pytest
from scipy import ndimage

from tests import components as cc

HAND = {
    "random 33x17x9 p=.35": ((33, 17, 9), lambda: cc.random_occ((33, 17, 9), 0.35, 1)),
    "random 33x17x9 p=.15": ((33, 17, 9), lambda: cc.random_occ((33, 17, 9), 0.15, 2)),
    "random 65x5x3 p=.35": ((65, 5, 3), lambda: cc.random_occ((65, 5, 3), 0.35, 3)),
    "random 130x3x2 p=.15": ((130, 3, 2), lambda: cc.random_occ((130, 3, 2), 0.15, 4)),
    "random 64x16x16 p=.35": ((64, 16, 16), lambda: cc.random_occ((64, 16, 16), 0.35, 5)),
    "checkerboard": ((33, 17, 9), lambda: cc.checkerboard((33, 17, 9))),
    "blobs joined": ((65, 5, 3), lambda: cc.word_boundary_blobs(True)),
    "blobs apart": ((65, 5, 3), lambda: cc.word_boundary_blobs(False)),
    "comb": ((64, 16, 4), cc.comb),
    "serpentine": ((64, 16, 4), cc.serpentine),
    "two equal": ((33, 17, 9), cc.two_equal),
    "empty": ((33, 17, 9), lambda: np.zeros((9, 17, 33), bool)),
    "full": ((33, 17, 9), lambda: np.ones((9, 17, 33), bool)),
}


def scipy_labels(occ, connectivity):
    """Least flat index per component, -1 where empty, by scipy."""
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    lab, n = ndimage.label(occ, structure)
    out = np.full(occ.size, -1, np.int32)
    if n:
        idx = np.arange(occ.size).reshape(occ.shape)
        least = ndimage.minimum(idx, lab, np.arange(1, n + 1))
        out = np.where(lab.reshape(-1) > 0, np.asarray(least)[np.maximum(lab.reshape(-1), 1) - 1], -1).astype(np.int32)
    return out


def check(occ, dims, connectivity):
    st = cc.bytes_of(occ, seed=7)
    got = cc.labels(st, dims, connectivity)
    want = scipy_labels(occ, connectivity)
    assert np.array_equal(got, want)
    lab, size = cc.table(got)
    assert np.array_equal(lab, np.unique(want[want >= 0]))
    assert size.sum() == occ.sum() and np.all(np.diff(lab) > 0)
    assert np.array_equal(size, ndimage.sum(occ.reshape(-1), want, lab).astype(np.int32)) if len(lab) else True
    return lab, size


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built(name, connectivity):
    dims, make = HAND[name]
    occ = make()
    assert occ.shape == dims[::-1]
    check(occ, dims, connectivity)


def test_hand_built_shapes():
    """The hand-built states are what their names say."""
    lab, size = check(cc.checkerboard((33, 17, 9)), (33, 17, 9), 6)
    assert len(lab) == (33 * 17 * 9) // 2 and np.all(size == 1)  # every voxel its own component: thousands
    assert len(check(cc.checkerboard((33, 17, 9)), (33, 17, 9), 26)[0]) == 1
    for conn in (6, 26):
        assert len(check(cc.word_boundary_blobs(True), (65, 5, 3), conn)[0]) == 1
        assert len(check(cc.word_boundary_blobs(False), (65, 5, 3), conn)[0]) == 2
        lab, size = check(cc.comb(), (64, 16, 4), conn)
        assert list(lab) == [0]
        lab, size = check(cc.serpentine(), (64, 16, 4), conn)
        assert list(lab) == [0] and list(size) == [1040]
    # the serpentine is a path: no voxel has more than two 6-neighbours, two have one
    occ = cc.serpentine()
    pad = np.pad(occ, 1).astype(np.int32)
    nb = sum(np.roll(pad, d, axis) for axis in range(3) for d in (-1, 1))[1:-1, 1:-1, 1:-1][occ]
    assert nb.max() == 2 and (nb == 1).sum() == 2
    # the comb's teeth touch nothing but the plane x = X - 1
    comb = cc.comb().copy()
    comb[:, :, 63] = False
    assert len(check(comb, (64, 16, 4), 26)[0]) == 16
    lab, size = check(cc.two_equal(), (33, 17, 9), 6)
    assert sorted(size) == [3, 27, 27]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_keep_rule(connectivity):
    dims = (33, 17, 9)
    occ = cc.two_equal()
    st = cc.bytes_of(occ, seed=3)
    vl = cc.labels(st, dims, connectivity)
    lab, size = cc.table(vl)
    assert sorted(size) == [3, 27, 27]
    out, kept, removed = cc.keep(st, dims, connectivity, largest=True)
    first = lab[size == 27].min()  # of the two equal ones, the least label stays
    assert kept == 1 and removed == 30
    assert np.array_equal(out & 1, (vl == first).astype(np.uint8))
    assert np.array_equal(out & 2, st & 2)  # seen bits as they were
    out, kept, removed = cc.keep(st, dims, connectivity, min_voxels=4)
    assert kept == 2 and removed == 3 and (out & 1).sum() == 54
    out, kept, removed = cc.keep(st, dims, connectivity, min_voxels=28, largest=True)
    assert kept == 0 and removed == 57 and not (out & 1).any()
    out, kept, removed = cc.keep(st, dims, connectivity)
    assert kept == 3 and removed == 0 and np.array_equal(out, st)
    empty = np.zeros(33 * 17 * 9, np.uint8)
    out, kept, removed = cc.keep(empty, dims, connectivity, largest=True)
    assert kept == 0 and removed == 0 and np.array_equal(out, empty)


# What the carve of the three-ball scene leaves, as measured with the CPU oracle: the main sphere of
# radius 0.25 E at 32^3, of radius 0.2 E at 48^3 (components.RADIUS) -- at 48^3 a sphere of 0.25 E
# carves to 7344, 91, 58 and 23 voxels under both connectivities, and it is the smaller one whose
# carve the two connectivities split differently (one voxel hangs on by a corner).
FIGURES = {(32, 6): [2167, 31, 16, 8], (32, 26): [2167, 31, 16, 8],
           (48, 6): [3760, 90, 52, 23, 1], (48, 26): [3761, 90, 52, 23]}


@pytest.fixture(scope="module")
def carved(oracle):
    out = {}
    for N in (32, 48):
        sc = cc.three_ball_scene(N)
        out[N] = oracle.carve(N, N, N, sc.voxel_size, sc.M, sc.masks).reshape(-1)
    return out


@pytest.mark.parametrize("N,connectivity", sorted(FIGURES))
def test_carved_scene(carved, N, connectivity):
    st = carved[N]
    occ = (st & 1).astype(bool).reshape(N, N, N)
    got = cc.labels(st, (N, N, N), connectivity)
    assert np.array_equal(got, scipy_labels(occ, connectivity))
    lab, size = cc.table(got)
    assert sorted(size, reverse=True) == FIGURES[N, connectivity]
    out, kept, removed = cc.keep(st, (N, N, N), connectivity, min_voxels=10)
    assert kept == sum(s >= 10 for s in FIGURES[N, connectivity])
    assert removed == sum(s for s in FIGURES[N, connectivity] if s < 10)
    out, kept, removed = cc.keep(st, (N, N, N), connectivity, largest=True)
    assert kept == 1 and (out & 1).sum() == FIGURES[N, connectivity][0]
    assert np.array_equal(out & 2, st & 2)
