"""The scenes of tests/test_fast_carve_paths_gpu.py through the oracle alone: each has the
property it is run for -- thousands of rows of tiles on the intended side of the pre-pass's limits,
a way through the complete tiles that bends often, a passage inside a tile longer than the step
kernel's 64 iterations -- so that no later edit quietly turns a case into a convex blob.  The
figures are recomputed from the oracle's plane (tests/fast_carve_scenes.py), none is written down
here."""
import numpy as np
import pytest

from tests import fast_carve_scenes as fs


@pytest.mark.parametrize("name", fs.names(fs.ALL))
def test_scene_is_worth_running(oracle, name):
    sc = fs.BY_NAME[name]
    ref = fs.reference(sc, oracle)
    print(f"{name}: {sc.dims} tile_rows {ref.tile_rows} full {ref.n_full} seeded {ref.n_seeded} "
          f"runs {ref.runs} tile_dist {ref.tile_dist} carved {ref.carved_fraction:.3f} oracle {ref.seconds:.2f} s")
    assert 0.3 < ref.carved_fraction < 1.0
    assert ref.seconds < 3.0, "shrink the scene"
    X, Y, Z = sc.dims
    assert ref.tile_rows == -(-Y // 16) * -(-Z // 16)
    assert X * Y * Z <= 9.0e6 or name == "serpentine-2words"  # (two words along x at > 1024 tile rows)


@pytest.mark.parametrize("name,side", [("spiral-2257", "mid"), ("spiral-4096", "at 4096"), ("spiral-4225", "above"),
                                       ("serpentine-1024", "at 1024"), ("serpentine-1025", "mid"),
                                       ("serpentine-2words", "mid"), ("box-sealed", "mid"), ("line-4100", "above")])
def test_tile_rows_are_on_the_intended_side(oracle, name, side):
    """1024 rows: the last size at which every thread of the whole-tile fill owns one row; 4096: the
    last size with a pre-pass (64 KB of LDS)."""
    for sc in fs.ALL:
        if sc.name.startswith(name):
            rows = fs.reference(sc, oracle).tile_rows
            assert {"at 1024": rows == 1024, "mid": 1024 < rows < 4096, "at 4096": rows == 4096,
                    "above": rows > 4096}[side], f"{sc.name}: {rows}"


@pytest.mark.parametrize("name", fs.names(fs.SPIRALS + fs.SERPENTINES + fs.BOXES + fs.XSPIRALS))
def test_complete_tiles_and_bends(oracle, name):
    sc = fs.BY_NAME[name]
    ref = fs.reference(sc, oracle)
    assert ref.n_seeded > 0.7 * ref.full.size, "most of the grid is complete tiles the pre-pass can take"
    box = ref.full[fs.BOX_TILES]
    if name == "box-pinhole-seen":
        # carved through the hole: complete tiles, and no complete tile joins them to the origin's
        assert box.all() and not ref.seeded[fs.BOX_TILES].any()
        assert ref.n_seeded == ref.n_full - box.size and box.size >= 9
    elif sc in fs.BOXES:
        # closed: nothing in the box is carved or seen, so its tiles are not even `full` here -- they
        # are completely OPEN all the same, and only the walls keep the pre-pass out of them
        X, Y, Z, _, _, _, state = fs.build(sc)
        a0, b0, a1, b1 = fs.BOX
        inside = ref.want[b0 + 1:b1, a0 + 1:a1, :]
        assert (inside == 1).all() and not box.any() and box.size >= 9
        assert ref.n_seeded == ref.n_full
    else:
        assert ref.n_seeded == ref.n_full
    if sc in fs.SPIRALS + fs.BOXES:
        assert ref.runs >= 12
    if sc in fs.XSPIRALS:
        assert ref.runs >= 6
        assert ref.full.shape[2] >= 10 and ref.seeded[:, :, 1:].any()
    if name == "xspiral-ragged":
        assert sc.dims[0] % 64 == 10
    if name == "serpentine-2words":
        assert sc.dims[0] == 65 and ref.seeded[:, :, 1].any()


@pytest.mark.parametrize("name", fs.names(fs.COMBS))
def test_comb_passages_outlast_one_launch(oracle, name):
    """flood_step_kernel runs at most 64 iterations a launch; an iteration moves the front one row
    across (and all the way along) the tile."""
    sc = fs.BY_NAME[name]
    ref = fs.reference(sc, oracle)
    assert fs.hops(sc, oracle) > 128
    assert ref.n_seeded == 0, "no complete tile: all of it is the step kernel's work"


def test_long_line_crosses_every_tile(oracle):
    sc = fs.BY_NAME["line-4100"]
    ref = fs.reference(sc, oracle)
    assert ref.tile_rows == 4100 and ref.tile_dist == 4099
    carved = (ref.want & 1) == 0
    assert carved[-1].all(), "the far end is reached through every hole"


def test_derivations_on_a_hand_made_plane():
    """The tile figures on a plane small enough to check by eye: 2 x 3 x 2 tiles, an L of complete
    tiles from the origin, one complete tile apart from it."""
    carved = np.zeros((32, 48, 128), bool)
    carved[0:16, 0:48, 0:64] = True     # tiles (tz 0, ty 0..2, tx 0)
    carved[0:32, 32:48, 0:64] = True    # tile (tz 1, ty 2, tx 0)
    carved[16:32, 0:16, 64:128] = True  # tile (tz 1, ty 0, tx 1): complete, apart
    carved[16, 16, 0] = True            # a partly carved tile
    full = fs.tiles_of(carved, "all")
    assert full.shape == (2, 3, 2) and full.sum() == 5
    seeded, dist = fs.tile_component(full)
    assert seeded.sum() == 4 and not seeded[1, 0, 1] and dist[1, 2, 0] == 3
    assert fs.tile_runs(seeded) == 2  # along y, then along z
    assert fs.tiles_of(carved, "any").sum() == 6
    ragged = np.ones((17, 16, 65), bool)
    assert fs.tiles_of(ragged, "all").all() and fs.tiles_of(ragged, "all").shape == (2, 1, 2)
    line = np.zeros((3, 4, 2), bool)
    line[0, :, :] = True
    line[:, 3, :] = True
    assert fs.voxel_hops(line, "yz") == 5 and fs.voxel_hops(line, "xy") == 4
