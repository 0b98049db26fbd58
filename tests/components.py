"""The connected components of include/arvx/arvx.h (arvx_components, arvx_components_keep) restated
in numpy, and the scenes and hand-built states their tests share.  No scipy here, so that
scipy.ndimage.label can check it (tests/test_components_cpu.py).

State bytes in, state bytes out: bit0 occupied, bit1 seen, flat index x + X*(y + Y*z).  A component's
label is the least flat index among its voxels; labels() returns it per voxel, -1 where empty."""
import numpy as np

from ar_voxel_project_amd import synthetic as syn


def offsets(connectivity):
    """The "backward" half of the neighbourhood as (dx, dy, dz): each adjacent pair once."""
    assert connectivity in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) >= (0, 0, 0):
                    continue
                if connectivity == 6 and abs(dx) + abs(dy) + abs(dz) != 1:
                    continue
                out.append((dx, dy, dz))
    assert len(out) == (3 if connectivity == 6 else 13)
    return out


def _edges(occ, connectivity):
    """All adjacent pairs of occupied voxels, as two arrays of flat indices (a > b)."""
    Z, Y, X = occ.shape
    idx = np.arange(occ.size, dtype=np.int64).reshape(Z, Y, X)
    ea, eb = [], []
    for dx, dy, dz in offsets(connectivity):
        def cut(d, n):  # the voxels that have a neighbour at +d, and those neighbours
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (za, zb), (ya, yb), (xa, xb) = cut(dz, Z), cut(dy, Y), cut(dx, X)
        both = occ[za, ya, xa] & occ[zb, yb, xb]
        ea.append(idx[za, ya, xa][both])
        eb.append(idx[zb, yb, xb][both])
    return np.concatenate(ea), np.concatenate(eb)


def labels(state, dims, connectivity=6):
    """int32 per voxel, flat index order: the least flat index of the voxel's component; -1 where
    the voxel is empty."""
    X, Y, Z = dims
    occ = (np.asarray(state, np.uint8).reshape(Z, Y, X) & 1).astype(bool)
    n = occ.size
    L = np.arange(n, dtype=np.int64)
    a, b = _edges(occ, connectivity)
    # hook the larger root of every pair under the smaller, then point everybody at its root, until
    # no pair has two roots: L[i] <= i throughout, so the root of a tree is its least index
    while a.size:
        ra, rb = L[a], L[b]
        differ = ra != rb
        a, b, ra, rb = a[differ], b[differ], ra[differ], rb[differ]
        if not a.size:
            break
        np.minimum.at(L, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            LL = L[L]
            if np.array_equal(LL, L):
                break
            L = LL
    out = np.where(occ.reshape(-1), L, -1).astype(np.int32)
    return out


def table(voxel_labels):
    """(labels ascending, sizes), int32 each."""
    lab, size = np.unique(voxel_labels[voxel_labels >= 0], return_counts=True)
    return lab.astype(np.int32), size.astype(np.int32)


def keep(state, dims, connectivity=6, min_voxels=1, largest=False, voxel_labels=None):
    """The rule of arvx_components_keep -> (state bytes, components kept, voxels removed): a component
    stays iff its size >= min_voxels and (not largest, or it has the greatest size, the least label
    among equals); the others' voxels lose bit0 and keep every other bit.  voxel_labels: labels(state,
    dims, connectivity) where the caller has them already."""
    st = np.asarray(state, np.uint8).reshape(-1).copy()
    vl = labels(st, dims, connectivity) if voxel_labels is None else voxel_labels
    lab, size = table(vl)
    stay = size >= min_voxels
    if largest and len(lab):
        best = int(np.argmax(size))  # (the first of the greatest: labels ascend, so the least label)
        only = np.zeros(len(lab), bool)
        only[best] = True
        stay &= only
    gone = np.isin(vl, lab[~stay])
    st[gone] &= np.uint8(0xFE)
    return st, int(stay.sum()), int(gone.sum())


# ---- the three-ball scene: a sphere and three specks that survive every silhouette ----------------

BALLS = (((0.36, 0.0, 0.0), 0.06), ((0.0, 0.36, 0.1), 0.05), ((-0.3, -0.3, -0.05), 0.04))


# the main sphere's radius, as a fraction of the extent, per grid size: the figures recorded for these
# scenes (tests/test_components_cpu.py, FIGURES) are those of 0.25 at 32^3 and of 0.2 at 48^3
RADIUS = {32: 0.25, 48: 0.2}


def three_ball_scene(N, V=8, W=160, H=120, with_images=False, radius_factor=None):
    """syn.sphere_scene(N, V, radius_factor) with three small spheres OR-ed into its masks: at centre
    c + off * E with radius r * E for (off, r) in BALLS, c the grid centre the ring cameras look at.
    radius_factor: RADIUS[N] (0.25 for other sizes) when not given."""
    if radius_factor is None:
        radius_factor = RADIUS.get(N, 0.25)
    sc = syn.sphere_scene(N, V, W=W, H=H, radius_factor=radius_factor, with_images=with_images)
    _, c = syn.ring_cameras(V)
    E = syn.EXTENT
    masks = sc.masks.copy()
    for off, r in BALLS:
        masks |= syn.sphere_masks(sc.K, sc.Rt, c + np.array(off) * E, r * E, W, H)
    sc.masks = masks
    return sc


# ---- hand-built states (occupancy as (Z, Y, X) bool -> bytes with a pattern of seen bits) ----------

def bytes_of(occ, seed=0):
    """State bytes of an occupancy: bit0 as given, bit1 (seen) random, so that a test sees it kept."""
    rng = np.random.default_rng(seed)
    seen = rng.random(occ.shape) < 0.5
    return (occ.astype(np.uint8) | (seen.astype(np.uint8) << 1)).reshape(-1)


def random_occ(dims, p, seed):
    X, Y, Z = dims
    return np.random.default_rng(seed).random((Z, Y, X)) < p


def checkerboard(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((x + y + z) & 1).astype(bool)


def word_boundary_blobs(joined):
    """65 x 5 x 3: a blob in x < 64 and one voxel column at x = 64, touching only through the pair
    (63, 2, 1) - (64, 2, 1) -- the boundary of the row's two 64-bit words; not joined: voxel x = 63
    of that row is empty."""
    occ = np.zeros((3, 5, 65), bool)
    occ[:, 1:4, 10:62] = True
    occ[1, 2, 62:64] = True
    occ[:, :, 64] = True
    if not joined:
        occ[1, 2, 63] = False
    return occ


def comb():
    """64 x 16 x 4: full rows at every even y that touch only in the plane x = X - 1."""
    occ = np.zeros((4, 16, 64), bool)
    occ[:, ::2, :] = True
    occ[:, :, 63] = True
    occ[1::2, :, :63] = False  # (the teeth of a plane do not touch the next plane's either)
    return occ


def serpentine():
    """64 x 16 x 4: one 6-connected path from voxel 0 through the full rows at even y of planes 0 and 2,
    turning through one voxel of the odd rows at alternate ends, through (0, 14, 1) from plane 0 to
    plane 2, ending in (0, 0, 3): 1040 voxels, every one with at most two neighbours."""
    occ = np.zeros((4, 16, 64), bool)
    for z in (0, 2):
        occ[z, ::2, :] = True
        for y in range(1, 14, 2):
            occ[z, y, 63 if y % 4 == 1 else 0] = True
    occ[1, 14, 0] = True
    occ[3, 0, 0] = True
    return occ


def two_equal():
    """33 x 17 x 9: two 3 x 3 x 3 cubes far apart, and a smaller third."""
    occ = np.zeros((9, 17, 33), bool)
    occ[5:8, 10:13, 20:23] = True
    occ[1:4, 2:5, 3:6] = True
    occ[0, 16, 30:33] = True
    return occ
