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


def signed_sq_sparse(dims, sites, site_kind, border_occupied=False):
    """signed_sq of the grid that is all of one kind except for the voxels `sites` ((x, y, z) each),
    which are occupied if site_kind and empty if not -- straight from the definition, a minimum over
    the listed sites and the six borders in int64, O(voxels * sites): for axes too long for the
    separable route's O(n^2).  -> int32 per voxel, flat index order."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z, dtype=np.int64), np.arange(Y, dtype=np.int64),
                          np.arange(X, dtype=np.int64), indexing="ij")
    listed = np.zeros((Z, Y, X), bool)
    for sx, sy, sz in sites:
        listed[sz, sy, sx] = True
    border = np.minimum.reduce([x + 1, X - x, y + 1, Y - y, z + 1, Z - z]) ** 2
    # the other voxels: the nearest listed site -- and the border, where the sites are the empty ones
    to_site = np.full((Z, Y, X), _BIG, np.int64)
    # the listed voxels: the nearest voxel that is not listed -- and the border, where those are empty
    to_rest = np.full(len(sites), _BIG, np.int64)
    for k, (sx, sy, sz) in enumerate(sites):
        d = (x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2
        np.minimum(to_site, d, out=to_site)
        if not listed.all():
            to_rest[k] = d[~listed].min()
    d = to_site
    for k, (sx, sy, sz) in enumerate(sites):
        d[sz, sy, sx] = to_rest[k]
    occ = listed if site_kind else ~listed
    if not border_occupied:  # (the border's sites are empty ones: the occupied voxels look for them)
        d = np.where(occ, np.minimum(d, border), d)
    d = np.where(d >= _BIG // 2, np.int64(INF), d)
    return np.where(occ, d, -d).astype(np.int32).reshape(-1)


def signed_sq_near(state, dims, border_occupied=False, reach=8):
    """signed_sq of a state in which every voxel has its nearest opposite site within `reach` (asserted):
    the minimum over the offsets of the cube of that half-width, straight from the definition, in int64,
    O(voxels * offsets) whatever the lengths of the axes -- for densely mixed states on a long axis."""
    occ = _occ(state, dims)
    Z, Y, X = occ.shape
    rz, ry, rx = min(reach, Z), min(reach, Y), min(reach, X)

    def to_sites(is_site, outside):
        p = np.pad(is_site, ((rz, rz), (ry, ry), (rx, rx)), constant_values=outside)
        d = np.full(occ.shape, _BIG, np.int64)
        for dz in range(-rz, rz + 1):
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    there = p[rz + dz:rz + dz + Z, ry + dy:ry + dy + Y, rx + dx:rx + dx + X]
                    np.minimum(d, np.where(there, np.int64(dx * dx + dy * dy + dz * dz), _BIG), out=d)
        return d

    d = np.where(occ, to_sites(~occ, not border_occupied), to_sites(occ, False))
    # (a site nearer than the one found would lie inside the cube too)
    assert d.max() <= reach * reach, "a voxel without an opposite site within reach"
    return np.where(occ, d, -d).astype(np.int32).reshape(-1)


def signed_sq_two_lines(n, lines, border_occupied=False):
    """signed_sq of a 2 x n x 1 grid (and of a 2 x 1 x n one: the flat order is the same, x + 2 j) whose
    line x is all of one kind except for the voxels lines[x] = (positions, site_kind) -- from
    signed_sq_sparse of each line alone, joined by the one step there is between the two lines."""
    to_empty, to_occupied, occ = [], [], []
    j = np.arange(n, dtype=np.int64)
    for sites, kind in lines:
        f = signed_sq_sparse((1, n, 1), [(0, int(k), 0) for k in sites], kind, True).astype(np.int64)
        to_empty.append(np.where(f > 0, np.where(f == INF, _BIG, f), 0))
        to_occupied.append(np.where(f < 0, np.where(f == -INF, _BIG, -f), 0))
        occ.append(f > 0)
    out = np.empty((n, 2), np.int64)
    for x in (0, 1):
        e = np.minimum(to_empty[x], to_empty[1 - x] + 1)
        if not border_occupied:  # (the line's two ends; the lattice point beside the voxel, off the grid)
            e = np.minimum.reduce([e, (j + 1) ** 2, (n - j) ** 2, np.ones(n, np.int64)])
        o = np.minimum(to_occupied[x], to_occupied[1 - x] + 1)
        d = np.where(occ[x], e, o)
        d = np.where(d >= _BIG // 2, np.int64(INF), d)
        out[:, x] = np.where(occ[x], d, -d)
    return out.astype(np.int32).reshape(-1)


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
