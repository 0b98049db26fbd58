"""The engineered inputs of tests/color_edges.py reach what they are built for -- checked here from
the restatements alone, without a GPU.  A scene that misses its edge would let a wrong kernel pass
tests/test_color_edges_gpu.py: late views that decide nothing hide a view loop that stops at 256,
camera positions that never tie hide a wrong comparison, a wave without a stray lane hides the
division fallback."""
import numpy as np
import pytest

from tests import color_edges as ce
from tests import np_restate as npr
from tests import visibility as vis


def differing(a, b, index):
    return int((a[index, :3] != b[index, :3]).any(axis=1).sum())


# ---- A: more than 256 views ---------------------------------------------------------------------

@pytest.mark.parametrize("assoc", [1, 0])
@pytest.mark.parametrize("V", [257, 300])
def test_late_views_decide_the_colour(oracle, V, assoc):
    key = ("many", V)
    x, y, z, index, smp = ce.surface_samples(key, assoc)
    assert len(index) > 1500  # (most of the 3003 voxels are surface voxels)
    late = ce.closest_view(smp.inside, smp.depth) >= ce.LDS_VIEWS
    assert late.sum() >= 50, "the last camera is the nearest one to part of the grid"
    assert (smp.inside[ce.LDS_VIEWS:].any(axis=0)).sum() >= 50
    for mode in (0, 1):
        full = ce.oracle_color(oracle, key, V, mode, assoc)
        head = ce.oracle_color(oracle, key, ce.LDS_VIEWS, mode, assoc)
        assert differing(full, head, index) >= 50, f"mode {mode}: a vote over views[:256] would pass"
    # the closest colours that differ are those of the voxels a late view wins (where the late
    # pixel's colour is not by chance the earlier winner's)
    full = ce.oracle_color(oracle, key, V, 0, assoc)
    head = ce.oracle_color(oracle, key, ce.LDS_VIEWS, 0, assoc)
    assert not (full[index[~late], :3] != head[index[~late], :3]).any()


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_and_numpy_agree_at_257_views(oracle, mode):
    sc = ce.many_views(257)
    want = npr.color(sc.X, sc.Y, sc.Z, sc.s, sc.M, sc.campos, sc.images, mode,
                     oracle.model_from_state(sc.state))
    assert np.array_equal(want, ce.oracle_color(oracle, ("many", 257), 257, mode, 1))


@pytest.mark.parametrize("tol", [2.0, np.inf])
@pytest.mark.parametrize("mode", [0, 1])
def test_late_views_decide_the_visible_colour(mode, tol):
    key = ("many", 257)
    full = ce.restated_visible(key, 257, mode, tol, 1)
    head = ce.restated_visible(key, ce.LDS_VIEWS, mode, tol, 1)
    assert np.array_equal(full.index, head.index)
    assert differing(full.rgba, head.rgba, full.index) >= 50
    if np.isfinite(tol):  # both branches of the vote
        assert 0 < np.count_nonzero(full.views) < len(full.views)


@pytest.mark.parametrize("iterations", [1, 3])
def test_late_views_decide_the_photo_carve(iterations):
    key = ("many_photo", 257)
    args = (ce.PHOTO_MAX_STD, ce.PHOTO_MIN_VIEWS, 3.0, iterations)
    full = ce.restated_photo(key, 257, *args)
    head = ce.restated_photo(key, ce.LDS_VIEWS, *args)
    assert head.removed == 0, "the first 256 views agree with each other"
    assert full.removed >= 50 and full.iterations == iterations
    if iterations > 1:  # later sweeps remove voxels the first one uncovered
        assert all(len(w) > 0 for w in full.sweeps)


# ---- B: depth ties and near-ties ----------------------------------------------------------------

def test_tie_scene_reaches_every_ordering(oracle):
    sc = ce.tie_scene()
    x, y, z, index, smp = ce.surface_samples(("ties",))
    assert smp.inside.all(), "every view sees the whole grid"
    assert np.array_equal(np.sqrt(smp.sum).astype(np.float32), smp.depth)  # (the sums are depth's)
    classes = ce.tie_classes(smp)
    counts = {k: int(v.sum()) for k, v in classes.items()}
    print(counts)
    for name in ("tie", "smaller", "larger", "closer", "triple"):
        assert counts[name] >= 50, counts
    # the mirrored pair ties exactly on the plane through voxel x = 8, and only there
    assert np.array_equal(smp.sum[0] == smp.sum[2], x == 8) and (x == 8).sum() >= 50
    # the votes a wrong comparison would give differ from the reference's in many voxels
    w = ce.closest_view(smp.inside, smp.depth)
    assert np.count_nonzero(ce.smallest_sum_view(smp.inside, smp.sum) != w) >= 50
    assert np.count_nonzero(ce.last_closest_view(smp.inside, smp.depth) != w) >= 50
    # D takes the colour where its fp32 depth is strictly smaller
    assert np.count_nonzero(w == ce.TIE_D) >= 50 and np.count_nonzero(w < ce.TIE_D) >= 50
    # the constant images name the winner, and the C oracle picks the same one
    want = ce.oracle_color(oracle, ("ties",), sc.V, 0, 1)
    assert np.array_equal(vis.view_of_colour(want[index, :3], sc.V), w)


def test_visible_vote_of_the_tie_scene_has_its_own_winner():
    sc = ce.tie_scene()
    x, y, z, index, smp = ce.surface_samples(("ties",))
    w = ce.closest_view(smp.inside, smp.depth)
    got = ce.restated_visible(("ties",), sc.V, 0, 2.0, 1)
    assert np.array_equal(got.index, index)
    vw = vis.view_of_colour(got.rgba[index, :3], sc.V)
    assert np.count_nonzero((vw != w) & (got.views > 0)) >= 50
    assert 0 < np.count_nonzero(got.views) < len(got.views)


@pytest.mark.parametrize("n", ce.HALF_MEAN_N)
def test_half_means_round_away_from_zero(oracle, n):
    sc = ce.half_mean_scene(n)
    x, y, z, index, smp = ce.surface_samples(("half_mean", n))
    assert smp.inside.all() and len(index) >= 50
    bgr = sc.images[:, 0, 0].astype(np.float64)
    assert np.array_equal(bgr.mean(axis=0)[::-1], np.array(ce.HALF_MEAN_RGB) - 0.5)
    want = ce.oracle_color(oracle, ("half_mean", n), n, 1, 1)
    assert (want[index, :3] == np.array(ce.HALF_MEAN_RGB, np.float32)).all()


# ---- C: the IEEE division in part of a wave -----------------------------------------------------

@pytest.mark.parametrize("extremes", [True, False])
def test_mixed_division_scene_mixes_lanes(oracle, extremes):
    sc, on_views = ce.mixed_division_scene(extremes)
    x, y, z, index, smp = ce.surface_samples(("mixed", extremes))
    tame = ce.tame_rows(smp.a0, smp.a1, smp.a2)
    wave = np.arange(len(index)) // 64  # one lane per list entry, 64 consecutive entries a wave
    for v, (vx, vy, vz) in zip(on_views, ce.MIX_ON_VOXEL):
        assert oracle.project_raw(sc.M[v], sc.s, vx, vy, vz)[2] == 0.0
        at = np.nonzero(index == (vz * sc.Y + vy) * sc.X + vx)[0]
        assert len(at) == 1, "the voxel the camera sits on is a surface voxel"
        assert smp.a2[v, at[0]] == 0.0 and not tame[v, at[0]]
        mates = wave == wave[at[0]]
        assert 0 < np.count_nonzero(~tame[v, mates]) < np.count_nonzero(tame[v, mates])
    mixed = [v for v in range(sc.V) if len(set(wave[~tame[v]]) & set(wave[tame[v]]))]
    assert set(on_views) <= set(mixed)
    if extremes:
        whole = [v for v in range(sc.V) if not tame[v].any()]
        assert whole == [5], "the view scaled by 2^70 is untame in every lane"
        behind = (smp.a2 < 0).sum(axis=1)
        assert np.count_nonzero(behind) >= 3, "cameras inside the grid: voxels behind them"
    for mode in (0, 1):
        want = npr.color(sc.X, sc.Y, sc.Z, sc.s, sc.M, sc.campos, sc.images, mode,
                         oracle.model_from_state(sc.state))
        assert np.array_equal(want, ce.oracle_color(oracle, ("mixed", extremes), sc.V, mode, 1))


# ---- D: every voxel on a pixel rounding tie -----------------------------------------------------

@pytest.mark.parametrize("eps_ulps", ce.PIX_EPS)
def test_rounding_tie_scene_is_on_the_ties(eps_ulps):
    sc = ce.rounding_tie_scene(eps_ulps)
    x, y, z, index, smp = ce.surface_samples(("pixel_ties", eps_ulps))
    assert smp.inside.all() and len(index) > 10000
    half = np.float32(0.5)
    c = ce.ulps(half, eps_ulps)
    for v, (cu, cv) in enumerate(((c, half), (half, c), (c, c))):
        _, qu, qv = npr.project_raw(sc.M[v], sc.s, x, y, z)
        # the quotients are the exact sums rounded once: within the rounding of x + 1/2 of the tie
        assert np.array_equal(qu, (x.astype(np.float32) + cu).astype(np.float32))
        assert np.array_equal(qv, (y.astype(np.float32) + cv).astype(np.float32))
        assert np.all(np.abs(qu - (x + 0.5)) <= abs(eps_ulps) * 2.0 ** -19)
        # the images tell one pixel from the next in both directions
        px, py = smp.pix[v] % sc.W, smp.pix[v] // sc.W
        bgr = sc.images[v].reshape(-1, 3)[smp.pix[v]]
        assert np.array_equal(bgr[:, 0], px) and np.array_equal(bgr[:, 1], py)
    w = ce.closest_view(smp.inside, smp.depth)
    assert np.bincount(w, minlength=3).min() >= 50  # every view is the closest somewhere
