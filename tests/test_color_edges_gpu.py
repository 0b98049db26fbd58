"""The colour votes on the device (color_vote_kernel, vis_vote_kernel, photo_consist_kernel and
color_samples_kernel) bit for bit against the restatements on the engineered inputs of
tests/color_edges.py: more than 256 views (the plain view loop), depth ties and near-ties (the
closest-colour shortcut), averages on k + 1/2, waves in which only some lanes take the IEEE
division, and every voxel on a pixel rounding tie.  tests/test_color_edges_cpu.py checks that the
inputs reach those edges."""
import numpy as np
import pytest

from tests import color_edges as ce
from tests import visibility as vis
from tests.test_color_visible_gpu import check_against_restatement

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_context(arvx, sc, assoc=1):
    ctx = arvx.Context(sc.X, sc.Y, sc.Z, sc.s, assoc=assoc)
    ctx.set_views(sc.M, np.full((sc.V, sc.H, sc.W), 255, np.uint8), campos=sc.campos)
    ctx.set_images(sc.images)
    ctx.upload_state(sc.state)
    return ctx


def voted(ctx, mode):
    ctx.color(mode)
    idx, rgb = ctx.surface()
    return idx, rgb, ctx.surface_depth(), ctx.export_model(False), ctx.export_model(True)


def check_color(got, want, oracle, sc, key, assoc):
    """The surface list, the colours, the minimum sample depths and both exports."""
    idx, rgb, depth, plain, unseen = got
    x, y, z, index, smp = ce.surface_samples(key, assoc)
    has = smp.inside.any(axis=0)
    assert np.array_equal(idx, index[has]), "coloured surface voxels"
    assert np.array_equal(bits(rgb), bits(want[idx, :3])), "surface colours"
    assert np.array_equal(bits(depth), bits(ce.min_depth(smp)[has])), "surface_depth"
    assert np.array_equal(bits(plain), bits(want)), "exported Model::voxels"
    assert np.array_equal(bits(unseen), bits(oracle.handle_unseen(sc.state, want))), "after handleUnseen"


def check_samples(ctx, sc, key):
    """arvx_color_samples of the whole surface list and a few voxels off it, sample for sample."""
    x, y, z, index, smp = ce.surface_samples(key)
    N = sc.X * sc.Y * sc.Z
    extra = np.setdiff1d(np.array([0, N // 3 + 1, N // 2, N - 1], np.int64), index)
    if len(extra):
        ask = np.concatenate([index, extra])
        ex = ce.samples(sc, extra % sc.X, (extra // sc.X) % sc.Y, extra // (sc.X * sc.Y))
        smp = type(smp)(**{k: np.concatenate([a, getattr(ex, k)], axis=1) for k, a in vars(smp).items()})
    else:
        ask = index
    got = ctx.color_samples(ask)
    assert got.shape == (len(ask), sc.V)
    inside = smp.inside.T
    assert np.array_equal(got["valid"].astype(bool), inside), "validity"
    bgr = np.stack([sc.images[v].reshape(-1, 3)[smp.pix[v]] for v in range(sc.V)], axis=1)
    for name, ch in (("r", 2), ("g", 1), ("b", 0)):
        assert np.array_equal(got[name][inside], bgr[..., ch][inside]), name
        assert not got[name][~inside].any()
    assert np.array_equal(bits(got["depth"])[inside], bits(smp.depth.T)[inside]), "depth"
    assert not bits(got["depth"])[~inside].any()
    return got[:len(index)], smp.inside[:, :len(index)]


def visible(ctx, mode, tol):
    ctx.color_visible(mode, tol)
    idx, rgb = ctx.surface()
    return idx, rgb, ctx.surface_depth(), ctx.surface_visible(), \
        np.stack([ctx.view_depth(v) for v in range(ctx.V)])


def check_visible(got, sc, key, mode, tol_voxels, assoc=1):
    want = ce.restated_visible(key, sc.V, mode, tol_voxels, assoc)
    check_against_restatement(got, want, sc.X, sc.Y, sc.Z, sc.s, sc.M, sc.campos, sc.state, assoc)
    return want


def check_visible_inf_is_plain(ctx, mode, plain):
    ctx.color_visible(mode, np.inf)
    idx, rgb = ctx.surface()
    assert np.array_equal(idx, plain[0]) and np.array_equal(bits(rgb), bits(plain[1]))
    assert np.array_equal(bits(ctx.surface_depth()), bits(plain[2]))
    assert np.array_equal(bits(ctx.export_model(True)), bits(plain[4]))


def check_photo(arvx, sc, key, max_std, min_views, tol_voxels, iterations, assoc=1):
    want = ce.restated_photo(key, sc.V, max_std, min_views, tol_voxels, iterations, assoc)
    with open_context(arvx, sc, assoc) as ctx:
        it, removed = ctx.photo_carve(max_std, min_views, np.float32(tol_voxels) * sc.s, iterations)
        state = ctx.download_state().reshape(-1)
    assert (it, removed) == (want.iterations, want.removed)
    assert np.array_equal(state, want.state)
    return want


# ---- A: more than 256 views ---------------------------------------------------------------------

@pytest.mark.parametrize("assoc", [1, 0])
@pytest.mark.parametrize("V", ce.MANY_V)
def test_color_of_many_views(arvx, oracle, V, assoc):
    """256 views are the last to go through LDS; 257 and 300 take the plain loop, and there a late
    view decides the colour of many voxels (the last camera is the nearest one to the middle of
    the grid): a loop that stops at 256 views, or reads them wrongly, shows in both modes."""
    key = ("many", V)
    sc = ce.many_views(V)
    with open_context(arvx, sc, assoc) as ctx:
        for mode in (0, 1):
            want = ce.oracle_color(oracle, key, V, mode, assoc)
            if V > ce.LDS_VIEWS:
                head = ce.oracle_color(oracle, key, ce.LDS_VIEWS, mode, assoc)
                assert (want[:, :3] != head[:, :3]).any(axis=1).sum() >= 50, "the late views decide"
            check_color(voted(ctx, mode), want, oracle, sc, key, assoc)


def test_color_samples_of_257_views(arvx):
    sc = ce.many_views(257)
    with open_context(arvx, sc) as ctx:
        got, inside = check_samples(ctx, sc, ("many", 257))
    assert inside[ce.LDS_VIEWS].sum() >= 50 and got["valid"][:, ce.LDS_VIEWS].sum() >= 50


@pytest.mark.parametrize("tol", [2.0, np.inf])
@pytest.mark.parametrize("mode", [0, 1])
def test_color_visible_of_257_views(arvx, mode, tol):
    key = ("many", 257)
    sc = ce.many_views(257)
    with open_context(arvx, sc) as ctx:
        got = visible(ctx, mode, np.float32(tol) * sc.s)
    want = check_visible(got, sc, key, mode, tol)
    head = ce.restated_visible(key, ce.LDS_VIEWS, mode, tol, 1)
    assert (want.rgba[want.index, :3] != head.rgba[want.index, :3]).any(axis=1).sum() >= 50


@pytest.mark.parametrize("iterations", [1, 3])
def test_photo_carve_of_257_views(arvx, iterations):
    """The first 256 views agree on every voxel; what is removed is removed because of view 256."""
    key = ("many_photo", 257)
    args = (ce.PHOTO_MAX_STD, ce.PHOTO_MIN_VIEWS, 3.0, iterations)
    want = check_photo(arvx, ce.many_views_photo(257), key, *args)
    assert want.removed >= 50 and ce.restated_photo(key, ce.LDS_VIEWS, *args).removed == 0


# ---- B: depth ties and near-ties ----------------------------------------------------------------

def test_closest_colour_on_depth_ties(arvx, oracle):
    """Exact ties, equal fp32 depths with a later smaller or larger fp64 sum, the triple
    sum_B < sum_C < sum_A, and a later strictly closer view: the first view of the smallest fp32
    depth keeps the colour, in the plain vote, in the visible vote (its own pair of running
    minima) and in the sample lists."""
    key = ("ties",)
    sc = ce.tie_scene()
    x, y, z, index, smp = ce.surface_samples(key)
    counts = {k: int(v.sum()) for k, v in ce.tie_classes(smp).items()}
    assert min(counts.values()) >= 50, counts
    winner = ce.closest_view(smp.inside, smp.depth)
    with open_context(arvx, sc) as ctx:
        want = ce.oracle_color(oracle, key, sc.V, 0, 1)
        plain = voted(ctx, 0)
        check_color(plain, want, oracle, sc, key, 1)
        assert np.array_equal(vis.view_of_colour(plain[1], sc.V), winner), "the view that keeps the colour"
        got, _ = check_samples(ctx, sc, key)
        assert np.array_equal(np.argmin(got["depth"], axis=1), winner)  # (every sample is valid)
        check_visible_inf_is_plain(ctx, 0, plain)
        check_visible(visible(ctx, 0, np.float32(2.0) * sc.s), sc, key, 0, 2.0)


@pytest.mark.parametrize("n", ce.HALF_MEAN_N)
def test_average_colour_on_half_means(arvx, oracle, n):
    """Means of exactly k + 1/2 over 2, 4 and 8 views round away from zero (.cpp:64-65)."""
    key = ("half_mean", n)
    sc = ce.half_mean_scene(n)
    want = ce.oracle_color(oracle, key, n, 1, 1)
    with open_context(arvx, sc) as ctx:
        plain = voted(ctx, 1)
        check_color(plain, want, oracle, sc, key, 1)
        assert len(plain[0]) >= 50 and (plain[1] == np.array(ce.HALF_MEAN_RGB, np.float32)).all()
        check_visible_inf_is_plain(ctx, 1, plain)
        check_visible(visible(ctx, 1, np.float32(2.0) * sc.s), sc, key, 1, 2.0)


# ---- C: the IEEE division in part of a wave -----------------------------------------------------

@pytest.mark.parametrize("assoc", [1, 0])
def test_color_with_untame_lanes_among_tame_ones(arvx, oracle, assoc):
    """Cameras on a voxel (a2 == 0 there: 0/0 and x/0, outside), cameras inside the grid and a view
    scaled by 2^70 between ordinary views: in the on-voxel views a few lanes of a wave leave the
    range of the shared reciprocal and the wave takes `/`."""
    key = ("mixed", True)
    sc, on_views = ce.mixed_division_scene(True)
    x, y, z, index, smp = ce.surface_samples(key, assoc)
    tame = ce.tame_rows(smp.a0, smp.a1, smp.a2)
    wave = np.arange(len(index)) // 64
    for v in on_views:
        stray = np.nonzero(smp.a2[v] == 0.0)[0]
        assert len(stray) and all(tame[v, wave == wave[k]].any() for k in stray)
    with open_context(arvx, sc, assoc) as ctx:
        for mode in (0, 1):
            check_color(voted(ctx, mode), ce.oracle_color(oracle, key, sc.V, mode, assoc), oracle, sc,
                        key, assoc)
        if assoc == 1:
            check_samples(ctx, sc, key)


def test_photo_carve_with_untame_lanes_among_tame_ones(arvx):
    sc, _ = ce.mixed_division_scene(True)
    want = check_photo(arvx, sc, ("mixed", True), 40.0, 2, 3.0, 1)
    assert want.removed >= 50


@pytest.mark.parametrize("mode", [0, 1])
def test_color_visible_with_cameras_on_voxels(arvx, mode):
    sc, _ = ce.mixed_division_scene(False)
    with open_context(arvx, sc) as ctx:
        for tol in (2.0, np.inf):
            check_visible(visible(ctx, mode, np.float32(tol) * sc.s), sc, ("mixed", False), mode, tol)


# ---- D: every voxel on a pixel rounding tie -----------------------------------------------------

@pytest.mark.parametrize("eps_ulps", ce.PIX_EPS)
def test_every_voxel_on_a_rounding_tie_through_the_colour_kernels(arvx, oracle, eps_ulps):
    """u = x + 1/2, v = y + 1/2 (+ a few ulps) in every voxel; the images encode the pixel (b = px,
    g = py, r the view), so one pixel off in any voxel shows in the closest colour, in the mean
    and in the samples."""
    key = ("pixel_ties", eps_ulps)
    sc = ce.rounding_tie_scene(eps_ulps)
    with open_context(arvx, sc) as ctx:
        for mode in (0, 1):
            plain = voted(ctx, mode)
            check_color(plain, ce.oracle_color(oracle, key, sc.V, mode, 1), oracle, sc, key, 1)
            check_visible_inf_is_plain(ctx, mode, plain)
        check_samples(ctx, sc, key)
