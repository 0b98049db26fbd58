"""The signed squared distance field and the ball morphology of include/arvx/arvx.h (arvx_distance,
arvx_morph) restated in numpy, and the hand-built states their tests share.  No scipy here, so that
scipy.ndimage can check it (tests/test_distance_cpu.py).

signed_sq goes the separable way (an exact min-plus per axis); morph is written from the ball's
offsets and never looks at a distance, so that the two routes check each other.

State bytes in, state bytes out: bit0 occupied, bit1 seen, bit2 painted, flat index x + X*(y + Y*z)."""
import numpy as np

INF = 2147483647  # ARVX_DISTANCE_INF
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
_BIG = np.int64(1) << 40  # "no site": above every squared distance of a grid the library accepts


def _occ(state, dims):
    X, Y, Z = dims
    return (np.asarray(state, np.uint8).reshape(Z, Y, X) & 1).astype(bool)


def _min_plus(f, axis, border_sites):
    """out[.., i, ..] = min over j of f[.., j, ..] + (i - j)^2 along one axis; with border_sites two
    more sites of value 0 at j = -1 and j = n.  One pass over the array per site."""
    f = np.moveaxis(f, axis, -1)
    n = f.shape[-1]
    i = np.arange(n, dtype=np.int64)
    out = np.full(f.shape, _BIG, np.int64)
    for j in range(n):
        np.minimum(out, f[..., j:j + 1] + (i - j) ** 2, out=out)
    if border_sites:
        np.minimum(out, np.minimum((i + 1) ** 2, (n - i) ** 2), out=out)
    return np.moveaxis(out, -1, axis)


def _to_sites(is_site, border_sites):
    """int64 (Z, Y, X): the squared distance of every voxel to the nearest site; >= _BIG / 2: none."""
    d = np.where(is_site, np.int64(0), _BIG)
    for axis in (2, 1, 0):
        d = _min_plus(d, axis, border_sites)
    return d


def signed_sq(state, dims, border_occupied=False):
    """int32 per voxel, flat index order: + the squared distance of an occupied voxel to the nearest
    empty site (the lattice points outside the grid among them unless border_occupied), - that of an
    empty voxel to the nearest occupied voxel, +-INF where there is no such site."""
    occ = _occ(state, dims)
    to_empty = _to_sites(~occ, not border_occupied)
    to_occupied = _to_sites(occ, False)
    d = np.where(occ, to_empty, to_occupied)
    d = np.where(d >= _BIG // 2, np.int64(INF), d)
    return np.where(occ, d, -d).astype(np.int32).reshape(-1)


def ball(radius_sq, dims):
    """The offsets (dx, dy, dz) with |o|^2 <= radius_sq.  An offset of X or more along x leaves the grid
    from every voxel, as one of exactly X does: the ball is cut there (and likewise along y and z)."""
    X, Y, Z = dims
    r = int(np.sqrt(float(radius_sq)))
    while r * r > radius_sq:
        r -= 1
    while (r + 1) * (r + 1) <= radius_sq:
        r += 1
    rx, ry, rz = min(r, X), min(r, Y), min(r, Z)
    return [(dx, dy, dz) for dz in range(-rz, rz + 1) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)
            if dx * dx + dy * dy + dz * dz <= radius_sq]


def _shifted(a, offs, outside, combine):
    """combine over o of a[i + o], `outside` standing for the lattice points off the grid."""
    Z, Y, X = a.shape
    rz = max(abs(o[2]) for o in offs)
    ry = max(abs(o[1]) for o in offs)
    rx = max(abs(o[0]) for o in offs)
    p = np.pad(a, ((rz, rz), (ry, ry), (rx, rx)), constant_values=outside)
    out = a.copy()
    for dx, dy, dz in offs:
        combine(out, p[rz + dz:rz + dz + Z, ry + dy:ry + dy + Y, rx + dx:rx + dx + X], out=out)
    return out


def dilate_occ(occ, radius_sq):
    """The voxels of the grid within the ball of an occupied voxel."""
    X, Y, Z = occ.shape[2], occ.shape[1], occ.shape[0]
    if radius_sq >= X * X + Y * Y + Z * Z:  # the ball joins any two voxels of the grid
        return np.full(occ.shape, bool(occ.any()))
    return _shifted(occ, ball(radius_sq, (X, Y, Z)), False, np.logical_or)


def erode_occ(occ, radius_sq, outside):
    """The occupied voxels whose whole ball is occupied, the points off the grid counting as `outside`."""
    X, Y, Z = occ.shape[2], occ.shape[1], occ.shape[0]
    if radius_sq >= X * X + Y * Y + Z * Z:  # the ball reaches every voxel of the grid, and leaves it
        return np.full(occ.shape, bool(occ.all() and outside))
    return _shifted(occ, ball(radius_sq, (X, Y, Z)), outside, np.logical_and)


def morph_occ(occ, op, radius_sq):
    if op == ERODE:
        return erode_occ(occ, radius_sq, False)
    if op == DILATE:
        return dilate_occ(occ, radius_sq)
    if op == OPEN:
        return dilate_occ(erode_occ(occ, radius_sq, False), radius_sq)
    assert op == CLOSE
    return erode_occ(dilate_occ(occ, radius_sq), radius_sq, True)


def morph(state, dims, op, radius_sq):
    """arvx_morph -> (state bytes, removed, added): bit0 becomes the op's result, the seen bit stays on
    every voxel, and the paint bit goes everywhere (the call drops the paint plane, as a carve does)."""
    st = np.asarray(state, np.uint8).reshape(-1)
    occ = _occ(st, dims)
    new = morph_occ(occ, op, radius_sq)
    out = (st & np.uint8(2)) | new.reshape(-1).astype(np.uint8)
    return out, int((occ & ~new).sum()), int((new & ~occ).sum())


# ---- hand-built states (occupancy as (Z, Y, X) bool) ------------------------------------------------

def bytes_of(occ, seed=0):
    """State bytes of an occupancy: bit0 as given, bit1 (seen) random, bit2 (painted) random on the
    occupied voxels, so that a test sees what is kept and what is dropped."""
    rng = np.random.default_rng(seed)
    seen = rng.random(occ.shape) < 0.5
    paint = (rng.random(occ.shape) < 0.25) & occ
    return (occ.astype(np.uint8) | (seen.astype(np.uint8) << 1) | (paint.astype(np.uint8) << 2)).reshape(-1)


def random_occ(dims, p, seed):
    X, Y, Z = dims
    return np.random.default_rng(seed).random((Z, Y, X)) < p


def checkerboard(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((x + y + z) & 1).astype(bool)


def one_corner(dims, value=True):
    """One voxel of the given kind in the corner (0, 0, 0), every other voxel of the other kind."""
    X, Y, Z = dims
    occ = np.full((Z, Y, X), not value)
    occ[0, 0, 0] = value
    return occ


def two_corners(dims):
    X, Y, Z = dims
    occ = np.zeros((Z, Y, X), bool)
    occ[0, 0, 0] = occ[Z - 1, Y - 1, X - 1] = True
    return occ


def solid_ball(dims, radius):
    """The voxels within `radius` of the grid's centre voxel."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return (x - X // 2) ** 2 + (y - Y // 2) ** 2 + (z - Z // 2) ** 2 <= radius * radius
