"""Numpy restatement of the vote carve (arvx_carve_votes; the definition is in include/arvx/arvx.h)
on top of the CPU oracle's single-view carve: oracle.carve_view on a FRESH state leaves, per voxel,
bit0 cleared iff the view sees the voxel as background (a miss) and bit1 set iff its pixel lies in
the image.  Summed over the views these are the two counts; step 3 of the definition applies them to
a given state."""
from collections import namedtuple

import numpy as np

Votes = namedtuple("Votes", "background inside")

# the two patches the project's damaged-mask figures were taken with: (view, rows, cols)
PATCHES = ((1, slice(50, 62), slice(70, 82)), (4, slice(60, 72), slice(85, 97)))
# ... moved onto the model of the 33 x 17 x 9 grid, which those two miss
PATCHES_SMALL = ((1, slice(66, 78), slice(70, 82)), (4, slice(72, 84), slice(68, 80)))


def damage(masks, patches=PATCHES):
    """A copy of `masks` with the patches zeroed: a segmentation that lost parts of the object."""
    out = np.array(masks, np.uint8)
    for v, rows, cols in patches:
        out[v, rows, cols] = 0
    return out


def per_view(oracle, X, Y, Z, s, M, masks, assoc_left=True):
    """Yields (miss, inside) of every view: bool per voxel, flat index order."""
    M = np.asarray(M, np.float32).reshape(-1, 3, 4)
    fresh = oracle.fresh_state(X, Y, Z)
    with oracle.variant("assoc_left" if assoc_left else "assoc_right"):
        for v in range(M.shape[0]):
            st = oracle.carve_view(X, Y, Z, s, M[v], masks[v], fresh).reshape(-1)
            yield (st & 1) == 0, (st & 2) != 0


def counts(oracle, X, Y, Z, s, M, masks, assoc_left=True):
    """-> Votes(background, inside): uint16 per voxel, flat index order."""
    assert len(masks) <= 65535
    bg = np.zeros(X * Y * Z, np.uint16)
    inside = np.zeros(X * Y * Z, np.uint16)
    for miss, ins in per_view(oracle, X, Y, Z, s, M, masks, assoc_left):
        bg += miss
        inside += ins
    return Votes(bg, inside)


def subtile_answers(oracle, X, Y, Z, s, M, masks, assoc_left=True):
    """What the views are to the 16 x 8 x 8 sub-tiles of a grid of whole sub-tiles: the number of
    (sub-tile, view) pairs in which no voxel is inside the image, every voxel is a miss, every voxel
    is inside and none a miss, and the rest -- (outside, background, foreground, mixed)."""
    assert X % 16 == 0 and Y % 8 == 0 and Z % 8 == 0
    n = [0, 0, 0, 0]

    def tiles(a, fn):
        return fn(a.reshape(Z // 8, 8, Y // 8, 8, X // 16, 16), axis=(1, 3, 5))

    for miss, ins in per_view(oracle, X, Y, Z, s, M, masks, assoc_left):
        out = ~tiles(ins, np.any)
        bg = tiles(miss, np.all)
        fg = tiles(ins & ~miss, np.all)
        n[0] += int(out.sum())
        n[1] += int(bg.sum())
        n[2] += int(fg.sum())
        n[3] += int((~out & ~bg & ~fg).sum())
    return tuple(n)


def apply(votes, state, max_misses):
    """Step 3: occ' = occ && bg <= max_misses, seen' = seen || in >= 1; -> state bytes (flat)."""
    st = np.array(state, np.uint8).reshape(-1)
    occ = ((st & 1) != 0) & (votes.background <= max_misses)
    seen = ((st & 2) != 0) | (votes.inside >= 1)
    return (st & np.uint8(0xFC)) | occ.astype(np.uint8) | (seen.astype(np.uint8) << 1)


def carve_votes(oracle, X, Y, Z, s, M, masks, max_misses, state=None, assoc_left=True):
    """arvx_carve_votes on `state` (None: a fresh model) -> (state bytes (flat), Votes)."""
    v = counts(oracle, X, Y, Z, s, M, masks, assoc_left)
    st = oracle.fresh_state(X, Y, Z) if state is None else state
    return apply(v, st, max_misses), v
