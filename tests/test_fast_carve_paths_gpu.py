"""The greedy carve's whole-tile pre-pass and step loop at the sizes real grids have, on grids of a
few million voxels (scenes: tests/fast_carve_scenes.py, checked on their own by
tests/test_fast_carve_scenes_cpu.py).

Every case compares the whole state plane after Context.fast_carve() with the oracle's and then
checks Context.last_fast_carve_path() against what the oracle's plane says must have happened:
  * the pre-pass ran exactly on grids of at most 4096 rows of tiles, and seeded exactly the tiles
    of the origin's component of complete tiles -- a plane can be right with a pre-pass that seeds
    too little (the step kernel makes up for it), the count cannot;
  * the step kernel was launched in whole batches of 4, 4, 8, 8, ..., at least as often as the front
    needs and, where the scene fixes that number, no batch more.
Thin grids and walls put thousands of tile rows (thread slots 1-3 of the one-workgroup fill, the
64 KB of LDS at 4096 rows, no pre-pass above) and ways of 15-31 bends in all four directions into
them; combs put passages of hundreds of hops into one tile, which one launch (64 iterations)
cannot follow."""
import numpy as np
import pytest

from tests import fast_carve_scenes as fs
from tests import scenes
from tests.test_carve_gpu import assert_same

pytestmark = pytest.mark.gpu

MAX_TILE_ROWS = 4096  # kFloodMaxTileRows


def batch_boundary(n):
    """The launches issued once n are needed: the batches are 4, 4, 8, 8, ... and run whole."""
    return 4 if n <= 4 else -(-n // 8) * 8


def check_report(arvx, info, ref, dims, fresh, what):
    """The report of the last greedy carve against the oracle's plane; returns the launches."""
    print(f"{what}: {info}, oracle: full {ref.n_full} seeded {ref.n_seeded} runs {ref.runs} "
          f"tile_dist {ref.tile_dist}")
    prepass = ref.tile_rows <= MAX_TILE_ROWS and dims[0] <= 64 * 64
    assert info["tile_rows"] == ref.tile_rows, f"{what}: {info}"
    assert bool(info["bits"] & arvx.FLOOD_PREPASS) == prepass, f"{what}: pre-pass: {info}"
    assert bool(info["bits"] & arvx.FLOOD_FRESH) == fresh, f"{what}: fresh: {info}"
    assert info["seeded"] == (ref.n_seeded if prepass else 0), f"{what}: seeded tiles: {info}, oracle {ref.n_seeded}"
    n = info["launches"]
    assert n >= 4 and n == batch_boundary(n), f"{what}: {n} launches are no whole batches"
    return n


def carve_scene(arvx, oracle, name):
    """Run a scene of tests/fast_carve_scenes.py: plane and report; returns (reference, launches)."""
    sc = fs.BY_NAME[name]
    ref = fs.reference(sc, oracle)
    X, Y, Z, s, M, masks, state = fs.build(sc)
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, masks)
        if state is not None:
            ctx.upload_state(state)
        ctx.fast_carve()
        info = ctx.last_fast_carve_path()
        got = ctx.download_state()
    assert_same(got, ref.want, name)
    return ref, check_report(arvx, info, ref, sc.dims, state is None, name)


# ---- a. the pre-pass at scale: 1024 | 1025 and 4096 | 4225 rows of tiles, both forms of the walls ----

@pytest.mark.parametrize("name", fs.names(fs.SPIRALS + fs.SERPENTINES))
def test_prepass_at_scale(arvx, oracle, name):
    ref, launches = carve_scene(arvx, oracle, name)
    if ref.tile_rows > MAX_TILE_ROWS:
        # e. no pre-pass: every tile is entered from a face neighbour, one tile per launch at most
        assert launches >= ref.tile_dist, f"{name}: {launches} launches, {ref.tile_dist} tiles to cross"


# ---- b. sealed regions ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fs.names(fs.BOXES))
def test_sealed_box(arvx, oracle, name):
    """A box of walls around 3 x 3 complete tiles: closed, nothing in it is carved or seen; with a
    hole of one voxel it is carved by the step kernel, and the pre-pass still leaves it out."""
    ref, _ = carve_scene(arvx, oracle, name)
    a0, b0, a1, b1 = fs.BOX
    inside = ref.want[b0 + 1:b1, a0 + 1:a1, :]
    if name == "box-pinhole-seen":
        assert ((inside & 1) == 0).all() and ref.n_seeded == ref.n_full - 9
    else:
        assert (inside == 1).all() and ref.n_seeded == ref.n_full


# ---- c. bends along x: ten words per row, the neighbour bits across words --------------------------

@pytest.mark.parametrize("name", fs.names(fs.XSPIRALS))
def test_bends_along_x(arvx, oracle, name):
    ref, _ = carve_scene(arvx, oracle, name)
    assert ref.runs >= 6 and ref.full.shape[2] >= 10


# ---- d. passages longer than a launch's 64 iterations ----------------------------------------------

@pytest.mark.parametrize("name", fs.names(fs.COMBS))
def test_comb_outlasts_a_launch(arvx, oracle, name):
    """An iteration of flood_step_kernel moves the front one hop across the tile, a launch at most
    64 and one more for the hand-over to the next launch or tile: the tile has to wake itself."""
    sc = fs.BY_NAME[name]
    ref, launches = carve_scene(arvx, oracle, name)
    hops = fs.hops(sc, oracle)
    print(f"{name}: hops {hops} launches {launches}")
    assert hops > 128
    assert launches * 65 >= hops, f"{name}: {launches} launches cannot cover {hops} hops"
    if ref.full.size == 1:
        # one tile: the front is at hop 64 n - 1 after n launches (the first iteration of the first
        # launch fills the seed's row), so ceil((hops + 1) / 64) launches change something; one more
        # sees no change, and the batch it is in runs to its end -- no further batch follows
        assert launches == batch_boundary(-(-(hops + 1) // 64) + 1), f"{name}: {launches} launches for {hops} hops"


# ---- e. no pre-pass, a front of 4100 tiles ---------------------------------------------------------

def test_line_of_4100_tiles(arvx, oracle):
    """8 x 16 x 65600: 4100 tiles in a row, no pre-pass, pre-seen planes with one hole every 1000
    voxels.  Only the tiles next to one that changed are awake, so launch k + 1 fills tile k (any
    way through a 16 x 16 cross-section, through a hole too, is shorter than 64 hops): 4100
    launches change something, launch 4101 sees no change, the batch ends at 4104."""
    ref, launches = carve_scene(arvx, oracle, "line-4100")
    assert ref.tile_rows == 4100 and ref.tile_dist == 4099
    assert launches >= 4100
    assert launches <= batch_boundary(4101), f"{launches} launches: a batch went on after one that changed nothing"


# ---- f. thin grids with noise ----------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(8, 2112, 9), (9, 8, 2112), (3, 5, 4160)])
@pytest.mark.parametrize("preseen", [False, True])
def test_thin_noise_grids(arvx, oracle, dims, preseen):
    """The grids of test_long_thin_grids the greedy carve has not seen (tests/test_carve_gpu.py: its
    cameras and noise masks), fresh and with 3 % of the voxels seen before."""
    X, Y, Z = dims
    V, W, H = 4, 200, 60
    s = np.float32(0.512 / max(dims))
    _, _, M = scenes.random_cameras(V, 0.512, seed=sum(dims), W=W, H=H)
    masks = scenes.noise_masks(V, H, W, block=6, p_bg=0.6, seed=X + 2)
    state = None
    if preseen:
        state = np.where(np.random.default_rng(Z).random((Z, Y, X)) < 0.03, 3, 1).astype(np.uint8)
    what = f"thin {dims} {'pre-seen' if preseen else 'fresh'}"
    ref = fs.refer(oracle.fast_carve(X, Y, Z, s, M, masks, state=state))
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, masks)
        if state is not None:
            ctx.upload_state(state)
        ctx.fast_carve()
        info = ctx.last_fast_carve_path()
        got = ctx.download_state()
    assert_same(got, ref.want, what)
    check_report(arvx, info, ref, dims, not preseen, what)


# ---- g. one context, run after run -----------------------------------------------------------------

def test_reuse_of_the_work_buffer(arvx, oracle):
    """The flood buffer, the rows of the pre-pass and the wake flags stay in the context: a run must
    not see what the run before left there, and the report follows the last run.  4096 rows of
    tiles: spiral (fresh), serpentine as pre-seen walls, spiral again; then the report's life."""
    spiral = fs.BY_NAME["spiral-4096-mask"]
    ref = fs.reference(spiral, oracle)
    X, Y, Z, s, M, masks, _ = fs.build(spiral)
    walls = scenes.serpentine_walls(Y, Z, 80, 48)
    state2 = scenes.walls_as_state(walls, "yz", X, Y, Z)
    masks2 = np.zeros_like(masks)
    ref2 = fs.refer(oracle.fast_carve(X, Y, Z, s, M, masks2, state=state2))
    assert 0 < ref2.n_seeded == ref2.n_full != ref.n_seeded
    zeros = {"bits": 0, "seeded": 0, "launches": 0, "tile_rows": 0}
    with arvx.Context(X, Y, Z, s) as ctx:
        assert ctx.last_fast_carve_path() == zeros  # before the first greedy carve
        ctx.set_views(M, masks)
        assert ctx.last_fast_carve_path() == zeros
        ctx.fast_carve()
        first = ctx.last_fast_carve_path()
        assert_same(ctx.download_state(), ref.want, "first spiral")
        check_report(arvx, first, ref, spiral.dims, True, "first spiral")
        assert ctx.last_fast_carve_path() == first  # asking changes nothing

        ctx.set_views(M, masks2)
        ctx.upload_state(state2)
        assert ctx.last_fast_carve_path() == zeros  # the state the report described is gone
        ctx.fast_carve()
        info = ctx.last_fast_carve_path()
        assert_same(ctx.download_state(), ref2.want, "serpentine on the spiral's buffers")
        check_report(arvx, info, ref2, spiral.dims, False, "serpentine on the spiral's buffers")

        ctx.reset()
        assert ctx.last_fast_carve_path() == zeros
        ctx.set_views(M, masks)
        ctx.fast_carve()
        again = ctx.last_fast_carve_path()
        assert_same(ctx.download_state(), ref.want, "spiral again")
        assert again == first

        ctx.carve()  # a dense carve replaces the state: the greedy carve's report goes
        assert ctx.last_fast_carve_path() == zeros
        ctx.fast_carve()  # on the records the two carves left: nothing open is left to enter
        info = ctx.last_fast_carve_path()
        assert not info["bits"] & arvx.FLOOD_FRESH and info["bits"] & arvx.FLOOD_PREPASS
        assert info["tile_rows"] == ref.tile_rows and info["seeded"] == 0 and info["launches"] == 4
        assert_same(ctx.download_state(), oracle.fast_carve(X, Y, Z, s, M, masks, state=oracle.carve(
            X, Y, Z, s, M, masks, state=ref.want)), "greedy after dense")
