"""The greedy carve's path scenes (tests/test_fast_carve_scenes_cpu.py, test_fast_carve_paths_gpu.py)
and what the oracle's plane says about each: how many rows of tiles it has, which 64x16x16 tiles
the whole-tile pre-pass must seed, how often the way through them bends, how far the front has to
travel inside a tile.  Everything is derived from `want = oracle.fast_carve(...)`:

    carved  the voxels the oracle carved
    full    the tiles whose voxels inside the grid are all carved
    seeded  the 6-connected component of `full` that holds tile (0, 0, 0).  It is what the pre-pass
            seeds: the pre-pass grows the origin's component over completely OPEN tiles, every tile
            of that component is carved completely (it is connected to the origin through open
            voxels), and a completely carved tile is completely open -- so the two components are
            the same set.
    runs    over the seeded tiles, the greatest minimum number of straight runs (bends + 1) of a way
            from the origin tile: the rounds the pre-pass needs (a round = one fill along x, +y, -y,
            +z, -z each).  0-1 breadth-first search over (tile, direction).
    hops    the greatest breadth-first distance from voxel (0, 0, 0) inside the carved set, moves
            along the axis the wall image does not have counting nothing.
    tile_dist  the greatest breadth-first distance from the origin tile over the tiles that hold a
            carved voxel, face to face: a front that enters a tile only from a face neighbour
            cannot cross fewer tiles than that.
"""
import collections
import time

import numpy as np

from tests import scenes

S = np.float32(2.0 ** -6)
Scene = collections.namedtuple("Scene", "name dims axes walls form extra")
# form "mask": the wall image is the mask of a fresh model; "seen": pre-seen voxels under an
# all-background mask; extra(st): last changes to the uploaded state (a hole of one voxel)


def scene(name, dims, axes, walls, form="mask", extra=None):
    assert form in ("mask", "seen") and (extra is None or form == "seen")
    return Scene(name, dims, axes, walls, form, extra)


def both_forms(name, dims, axes, walls):
    return [scene(f"{name}-mask", dims, axes, walls), scene(f"{name}-seen", dims, axes, walls, "seen")]


def spiral(pitch=64):
    return lambda A, B: scenes.spiral_walls(A, B, pitch)


def serpentine(A, B):
    return scenes.serpentine_walls(A, B, 80, 48)


# the sealed box of the 8 x 587 x 973 spiral, in the room that a spiral of three turns (twelve walls)
# leaves in the middle: walls at 7 mod 16, 3 x 3 complete tiles inside (y tiles 15-17, z tiles 26-28)
BOX = (231, 407, 295, 471)
BOX_TILES = (slice(26, 29), slice(15, 18), slice(0, 1))  # [tz, ty, tx]
BOX_HOLE = (5, 231, 440)  # voxel (x, y, z) of the left wall


def spiral_box(A, B):
    return scenes.sealed_box(scenes.spiral_walls(A, B, 64, turns=12), BOX)


def open_hole(st):
    x, y, z = BOX_HOLE
    assert st[z, y, x] == 3
    st[z, y, x] = 1


def wall_planes(every=1000):
    """Pre-seen planes across z, each with a hole of one voxel: for the xy form the 'image' is not
    used as walls (they do not span an axis); see build()."""
    def extra(st):
        for k, z in enumerate(range(every - 1, st.shape[0], every)):
            st[z] = 3
            st[z, (5 * k) % st.shape[1], (3 * k) % st.shape[2]] = 1
    return extra


SPIRALS = (both_forms("spiral-2257", (8, 587, 973), "yz", spiral()) +
           both_forms("spiral-4096", (8, 1024, 1024), "yz", spiral()) +
           both_forms("spiral-4225", (8, 1040, 1040), "yz", spiral()))
SERPENTINES = [scene("serpentine-1024", (8, 512, 512), "yz", serpentine),
               scene("serpentine-1025", (8, 400, 656), "yz", serpentine),
               scene("serpentine-2words", (65, 264, 1000), "yz", serpentine)]
BOXES = [scene("box-sealed-mask", (8, 587, 973), "yz", spiral_box),
         scene("box-sealed-seen", (8, 587, 973), "yz", spiral_box, "seen"),
         scene("box-pinhole-seen", (8, 587, 973), "yz", spiral_box, "seen", open_hole)]
# bends along x: corridors of two complete tiles, 192 voxels in x and 48 in z
XSPIRALS = (both_forms("xspiral", (640, 16, 400), "xz", spiral((192, 48))) +
            [scene("xspiral-ragged", (650, 20, 410), "xz", spiral((192, 48)))])
COMBS = (both_forms("comb-1tile", (64, 16, 16), "yz", scenes.comb_walls) +
         both_forms("comb-4tiles", (70, 32, 32), "yz", scenes.comb_walls) +
         both_forms("comb-ragged", (40, 37, 21), "yz", scenes.comb_walls))
LONG = [scene("line-4100", (8, 16, 65600), "xy", lambda A, B: np.zeros((B, A), np.uint8), "seen", wall_planes())]
ALL = SPIRALS + SERPENTINES + BOXES + XSPIRALS + COMBS + LONG
BY_NAME = {sc.name: sc for sc in ALL}
assert len(BY_NAME) == len(ALL)


def names(group):
    return [sc.name for sc in group]


def build(sc):
    """(X, Y, Z, s, M, masks, state or None) of a scene."""
    X, Y, Z = sc.dims
    B, A = scenes.image_shape(sc.axes, X, Y, Z)
    img = sc.walls(A, B)
    assert img.shape == (B, A)
    M = scenes.axis_view(sc.axes, S)
    if sc.form == "mask":
        return X, Y, Z, S, M, img[None], None
    st = scenes.walls_as_state(img, sc.axes, X, Y, Z)
    if sc.extra:
        sc.extra(st)
    return X, Y, Z, S, M, np.zeros((1, B, A), np.uint8), st


# ---- what the oracle's plane says ---------------------------------------------------------------

def tiles_of(mask, reduce):
    """Per 64 x 16 x 16 tile [tz, ty, tx]: reduce ("all" / "any") of mask (Z, Y, X) over the tile's
    voxels inside the grid."""
    Z, Y, X = mask.shape
    tz, ty, tx = -(-Z // 16), -(-Y // 16), -(-X // 64)
    pad = np.full((tz * 16, ty * 16, tx * 64), reduce == "all", bool)
    pad[:Z, :Y, :X] = mask
    t = pad.reshape(tz, 16, ty, 16, tx, 64)
    return t.all(axis=(1, 3, 5)) if reduce == "all" else t.any(axis=(1, 3, 5))


DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def tile_component(tiles):
    """(member, dist): the 6-connected component of `tiles` that holds tile (0, 0, 0) and the
    breadth-first distance of its tiles from there (-1 outside)."""
    dist = np.full(tiles.shape, -1, np.int64)
    if tiles[0, 0, 0]:
        dist[0, 0, 0] = 0
        todo = collections.deque([(0, 0, 0)])
        while todo:
            p = todo.popleft()
            for d in DIRS:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if all(0 <= q[i] < tiles.shape[i] for i in range(3)) and tiles[q] and dist[q] < 0:
                    dist[q] = dist[p] + 1
                    todo.append(q)
    return dist >= 0, dist


def tile_runs(member):
    """Greatest, over the tiles of the component `member`, of the least number of straight runs
    from tile (0, 0, 0): 0-1 breadth-first search over (tile, direction)."""
    if not member[0, 0, 0]:
        return 0
    INF = 1 << 30
    cost = np.full(member.shape + (6,), INF, np.int64)
    cost[0, 0, 0, :] = 1
    todo = collections.deque(((0, 0, 0), k) for k in range(6))
    while todo:
        p, k = todo.popleft()
        c = cost[p + (k,)]
        for k2 in range(6):  # a bend on the spot: one run more
            if cost[p + (k2,)] > c + 1:
                cost[p + (k2,)] = c + 1
                todo.append((p, k2))
        d = DIRS[k]
        q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
        if all(0 <= q[i] < member.shape[i] for i in range(3)) and member[q] and cost[q + (k,)] > c:
            cost[q + (k,)] = c
            todo.appendleft((q, k))
    return int(cost.min(axis=3)[member].max())


def voxel_hops(carved, axes):
    """Greatest 0-1 breadth-first distance from voxel (0, 0, 0) inside `carved` (Z, Y, X); a move
    along the axis the wall image does not have costs nothing.  Small grids only."""
    if not carved[0, 0, 0]:
        return 0
    free = {"yz": 2, "xz": 1, "xy": 0}[axes]  # index into (z, y, x)
    INF = 1 << 30
    dist = np.full(carved.shape, INF, np.int64)
    dist[0, 0, 0] = 0
    todo = collections.deque([(0, 0, 0)])
    while todo:
        p = todo.popleft()
        c = dist[p]
        for d in DIRS:
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if not all(0 <= q[i] < carved.shape[i] for i in range(3)) or not carved[q]:
                continue
            w = 0 if d[free] else 1
            if dist[q] > c + w:
                dist[q] = c + w
                (todo.append if w else todo.appendleft)(q)
    return int(dist[carved & (dist < INF)].max())


Reference = collections.namedtuple(
    "Reference", "want seconds tile_rows carved_fraction full seeded n_full n_seeded runs tile_dist")
_cache = {}


def refer(want, seconds=0.0):
    """The figures of an oracle's plane."""
    want.setflags(write=False)
    carved = (want & 1) == 0
    full = tiles_of(carved, "all")
    seeded, _ = tile_component(full)
    _, dist = tile_component(tiles_of(carved, "any"))
    return Reference(want, seconds, full.shape[0] * full.shape[1], float(carved.mean()), full, seeded,
                     int(full.sum()), int(seeded.sum()), tile_runs(seeded), int(dist.max()))


def reference(sc, oracle):
    """The oracle's plane of a scene and its figures; computed once per process."""
    if sc.name not in _cache:
        X, Y, Z, s, M, masks, state = build(sc)
        t0 = time.perf_counter()
        want = oracle.fast_carve(X, Y, Z, s, M, masks, state=state)
        _cache[sc.name] = refer(want, time.perf_counter() - t0)
    return _cache[sc.name]


_hops = {}


def hops(sc, oracle):
    if sc.name not in _hops:
        _hops[sc.name] = voxel_hops((reference(sc, oracle).want & 1) == 0, sc.axes)
    return _hops[sc.name]
