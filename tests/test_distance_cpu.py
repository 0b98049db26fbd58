"""The numpy restatement of the distance field and the ball morphology (tests/distance.py) against
scipy.ndimage: the signed squared distances recomputed from distance_transform_edt's nearest-site
indices (no square root is compared), the four ops against binary_erosion / binary_dilation with the
ball as structure, and the set properties of the definition; and the boundary: every arvx_distance* /
arvx_morph declaration of the header is bound and exported."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import distance as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "arvx", "arvx.h")

HAND = {
    "random 33x17x9 p=.02": ((33, 17, 9), lambda: dist.random_occ((33, 17, 9), 0.02, 1)),
    "random 33x17x9 p=.5": ((33, 17, 9), lambda: dist.random_occ((33, 17, 9), 0.5, 2)),
    "random 33x17x9 p=.98": ((33, 17, 9), lambda: dist.random_occ((33, 17, 9), 0.98, 3)),
    "random 65x5x3 p=.5": ((65, 5, 3), lambda: dist.random_occ((65, 5, 3), 0.5, 4)),
    "random 130x3x2 p=.98": ((130, 3, 2), lambda: dist.random_occ((130, 3, 2), 0.98, 5)),
    "random 4x40x3 p=.02": ((4, 40, 3), lambda: dist.random_occ((4, 40, 3), 0.02, 6)),
    "random 7x1x1 p=.5": ((7, 1, 1), lambda: dist.random_occ((7, 1, 1), 0.5, 7)),
    "random 1x7x1 p=.5": ((1, 7, 1), lambda: dist.random_occ((1, 7, 1), 0.5, 8)),
    "random 1x1x7 p=.5": ((1, 1, 7), lambda: dist.random_occ((1, 1, 7), 0.5, 9)),
    "1x1x1 occupied": ((1, 1, 1), lambda: np.ones((1, 1, 1), bool)),
    "1x1x1 empty": ((1, 1, 1), lambda: np.zeros((1, 1, 1), bool)),
    "checkerboard": ((33, 17, 9), lambda: dist.checkerboard((33, 17, 9))),
    "one occupied corner": ((33, 17, 9), lambda: dist.one_corner((33, 17, 9), True)),
    "one empty corner": ((33, 17, 9), lambda: dist.one_corner((33, 17, 9), False)),
    "two corners": ((33, 17, 9), lambda: dist.two_corners((33, 17, 9))),
    "ball": ((33, 17, 19), lambda: dist.solid_ball((33, 17, 19), 7)),
    "empty": ((33, 17, 9), lambda: np.zeros((9, 17, 33), bool)),
    "full": ((33, 17, 9), lambda: np.ones((9, 17, 33), bool)),
}
RADII = (0, 1, 2, 3, 9)


def _nearest_zero_sq(a):
    """int64: the squared distance of every element of `a` to its nearest zero element (which exists),
    from the indices scipy reports."""
    idx = ndimage.distance_transform_edt(a, return_distances=False, return_indices=True)
    grid = np.indices(a.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(axis=0)


def scipy_signed_sq(occ, border_occupied):
    out = np.empty(occ.shape, np.int64)
    if border_occupied:
        to_empty = _nearest_zero_sq(occ) if not occ.all() else np.full(occ.shape, dist.INF, np.int64)
    else:  # one shell of empty voxels: the nearest point outside the grid always lies in it
        to_empty = _nearest_zero_sq(np.pad(occ, 1, constant_values=False))[1:-1, 1:-1, 1:-1]
    to_occupied = _nearest_zero_sq(~occ) if occ.any() else np.full(occ.shape, dist.INF, np.int64)
    out[occ] = to_empty[occ]
    out[~occ] = -to_occupied[~occ]
    return out.astype(np.int32).reshape(-1)


def ball_structure(radius_sq):
    r = int(np.floor(np.sqrt(radius_sq)))
    z, y, x = np.meshgrid(*(np.arange(-r, r + 1),) * 3, indexing="ij")
    return x * x + y * y + z * z <= radius_sq


def scipy_morph(occ, op, radius_sq):
    s = ball_structure(radius_sq)
    if op == dist.ERODE:
        return ndimage.binary_erosion(occ, s, border_value=0)
    if op == dist.DILATE:
        return ndimage.binary_dilation(occ, s, border_value=0)
    if op == dist.OPEN:
        return ndimage.binary_dilation(ndimage.binary_erosion(occ, s, border_value=0), s, border_value=0)
    return ndimage.binary_erosion(ndimage.binary_dilation(occ, s, border_value=0), s, border_value=1)


@pytest.mark.parametrize("name", sorted(HAND))
def test_signed_sq_against_scipy(name):
    dims, make = HAND[name]
    occ = make()
    st = dist.bytes_of(occ, seed=7)
    for border_occupied in (False, True):
        got = dist.signed_sq(st, dims, border_occupied)
        assert got.dtype == np.int32
        assert np.array_equal(got, scipy_signed_sq(occ, border_occupied)), border_occupied
        assert np.all((got > 0) == occ.reshape(-1)) and not np.any(got == 0)


def test_signed_sq_special_values():
    dims = (33, 17, 9)
    n = 33 * 17 * 9
    z, y, x = np.meshgrid(np.arange(9), np.arange(17), np.arange(33), indexing="ij")
    full, empty = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    assert np.all(dist.signed_sq(empty, dims) == -dist.INF) and np.all(dist.signed_sq(empty, dims, True) == -dist.INF)
    assert np.all(dist.signed_sq(full, dims, True) == dist.INF)
    border = np.minimum.reduce([x + 1, 33 - x, y + 1, 17 - y, z + 1, 9 - z]) ** 2  # the pure border field
    assert np.array_equal(dist.signed_sq(full, dims), border.reshape(-1))
    assert np.all(np.abs(dist.signed_sq(dist.bytes_of(dist.checkerboard(dims)), dims)) == 1)
    d = dist.signed_sq(dist.bytes_of(dist.solid_ball((33, 17, 19), 7)), (33, 17, 19))
    assert d.max() == 50  # (the centre voxel: the nearest lattice points beyond radius 7 are (5, 5, 0) and (7, 1, 0))


def _state_of_sites(dims, sites, site_kind):
    X, Y, Z = dims
    occ = np.full((Z, Y, X), not site_kind)
    for x, y, z in sites:
        occ[z, y, x] = site_kind
    return occ.astype(np.uint8).reshape(-1)


@pytest.mark.parametrize("dims,sites", [
    ((33, 17, 9), [(0, 0, 0), (32, 16, 8), (5, 9, 4), (6, 9, 4), (20, 0, 3)]),
    ((70, 2, 3), [(69, 1, 2), (64, 0, 0), (63, 0, 0), (3, 1, 1)]),
    ((1, 40, 1), [(0, 0, 0), (0, 39, 0), (0, 17, 0)]),
    ((5, 4, 3), []),
    ((2, 1, 1), [(0, 0, 0), (1, 0, 0)]),
])
def test_signed_sq_sparse_against_signed_sq(dims, sites):
    """The direct minimum over a few sites and the borders is the separable route's field."""
    for site_kind in (False, True):
        st = _state_of_sites(dims, sites, site_kind)
        for border_occupied in (False, True):
            got = dist.signed_sq_sparse(dims, sites, site_kind, border_occupied)
            assert got.dtype == np.int32
            assert np.array_equal(got, dist.signed_sq(st, dims, border_occupied)), (site_kind, border_occupied)


@pytest.mark.parametrize("dims,seed", [((33, 17, 9), 2), ((5, 70, 1), 4), ((5, 1, 70), 5), ((1, 1, 9), 7)])
def test_signed_sq_near_against_signed_sq(dims, seed):
    """The minimum over a cube of offsets is the separable route's field where no distance exceeds the
    cube's half-width, and says so where one does."""
    st = dist.bytes_of(dist.random_occ(dims, 0.5, seed), seed=7)
    for border_occupied in (False, True):
        want = dist.signed_sq(st, dims, border_occupied)
        assert np.abs(want.astype(np.int64)).max() <= 64
        got = dist.signed_sq_near(st, dims, border_occupied)
        assert got.dtype == np.int32 and np.array_equal(got, want), border_occupied
    with pytest.raises(AssertionError):
        dist.signed_sq_near(dist.bytes_of(dist.one_corner((33, 17, 9), True)), (33, 17, 9))


@pytest.mark.parametrize("lines", [
    (([0, 39], False), ([5, 20, 33], True)),
    (([3], True), ([3, 4], True)),
    (([], False), ([], True)),
    (([0], False), ([39], False)),
    (([], True), ([7], True)),
])
def test_signed_sq_two_lines_against_signed_sq(lines):
    n = 40
    occ = np.empty((n, 2), bool)
    for x, (sites, kind) in enumerate(lines):
        occ[:, x] = not kind
        occ[sites, x] = kind
    st = occ.astype(np.uint8).reshape(-1)
    for border_occupied in (False, True):
        got = dist.signed_sq_two_lines(n, lines, border_occupied)
        assert got.dtype == np.int32
        assert np.array_equal(got, dist.signed_sq(st, (2, n, 1), border_occupied)), border_occupied
        assert np.array_equal(got, dist.signed_sq(st, (2, 1, n), border_occupied)), border_occupied


@pytest.mark.parametrize("name", sorted(HAND))
def test_morph_against_scipy_and_the_distance_route(name):
    dims, make = HAND[name]
    occ = make()
    st = dist.bytes_of(occ, seed=7)
    d = dist.signed_sq(st, dims).reshape(occ.shape)
    for R in RADII + (dims[0] ** 2 + dims[1] ** 2 + dims[2] ** 2,):
        got = {op: dist.morph_occ(occ, op, R) for op in (dist.ERODE, dist.DILATE, dist.OPEN, dist.CLOSE)}
        if R <= 9:  # (scipy's structure for the radius above the grid would be the grid cubed)
            for op in got:
                assert np.array_equal(got[op], scipy_morph(occ, op, R)), (op, R)
        else:
            assert not got[dist.ERODE].any() and not got[dist.OPEN].any()
            assert np.all(got[dist.DILATE] == occ.any()) and np.all(got[dist.CLOSE] == occ.any())
        # the distance route: one threshold each
        assert np.array_equal(got[dist.ERODE], d > R)
        assert np.array_equal(got[dist.DILATE], occ | (-d.astype(np.int64) <= R))
        B = got[dist.DILATE]
        dB = dist.signed_sq(B.astype(np.uint8).reshape(-1), dims, True).reshape(occ.shape)
        assert np.array_equal(got[dist.CLOSE], dB > R)
        # the set properties
        assert not (got[dist.OPEN] & ~occ).any() and not (occ & ~got[dist.CLOSE]).any()
        assert np.array_equal(dist.morph_occ(got[dist.OPEN], dist.OPEN, R), got[dist.OPEN])
        assert np.array_equal(dist.morph_occ(got[dist.CLOSE], dist.CLOSE, R), got[dist.CLOSE])
        if R == 0:
            assert all(np.array_equal(g, occ) for g in got.values())


def test_morph_state_bytes():
    """bit0 is the op's result, the seen bit stays everywhere, the paint bit goes, the counts compare
    the final occupancy with the initial one."""
    dims = (33, 17, 9)
    occ = dist.random_occ(dims, 0.5, 2)
    st = dist.bytes_of(occ, seed=3)
    assert (st & 4).any() and not (st & 4)[~occ.reshape(-1)].any()
    for op in (dist.ERODE, dist.DILATE, dist.OPEN, dist.CLOSE):
        out, removed, added = dist.morph(st, dims, op, 2)
        new = dist.morph_occ(occ, op, 2)
        assert np.array_equal(out & 1, new.reshape(-1)) and np.array_equal(out & 2, st & 2) and not (out & 0xFC).any()
        assert removed == (occ & ~new).sum() and added == (new & ~occ).sum() and min(removed, added) == 0
        assert removed + added > 0


def test_header_declarations_are_bound_and_exported(arvx):
    """Every arvx_distance* / arvx_morph* the header declares has its prototype in capi.py and is
    exported by the built libarvx.so; the constants agree with the header's."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(arvx_(?:distance|morph)[a-z_0-9]*)\s*\(", text)))
    assert names == ["arvx_distance", "arvx_distance_download", "arvx_morph"]
    lib = arvx.load_library()
    for n in names:
        assert n in arvx.SYMBOLS
        fn = getattr(lib, n)
        assert fn.argtypes is not None and fn.argtypes[0] is ctypes.c_void_p and fn.restype is ctypes.c_int, n
    assert lib.arvx_morph.argtypes[2] is ctypes.c_int64
    defines = dict(re.findall(r"#define\s+ARVX_((?:DISTANCE|MORPH)_[A-Z_]+)\s+(\d+)", text))
    assert len(defines) == 6
    for k, v in defines.items():
        assert getattr(arvx, k) == int(v), k
    # the argument checks need no GPU
    assert lib.arvx_distance(None, 0) == 1 and b"null" in lib.arvx_last_error()  # ARVX_ERR_INVALID
    assert lib.arvx_distance_download(None, None) == 1
    assert lib.arvx_morph(None, 0, 1, None, None) == 1
    for m in ("distance", "morph"):
        assert callable(getattr(arvx.Context, m))
