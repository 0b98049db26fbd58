"""The table of cached voxel pixels (arvx.h, arvx_ctx_set_pixel_cache_limit) against the carve that
projects, against the carve with the block table alone, and against the CPU oracle.

Together with its table of block rectangles a context that runs the large grids' kernels tabulates
the pixel of every (voxel, view), and the exact kernel of the fresh carves that follow reads the
views that fit instead of projecting them.  Every case is a small grid pushed onto those kernels with
CARVE_DENSE_CLASSIFY | CARVE_WHOLE_ITEMS (tests/test_rect_cache_gpu.py), carved three times from a
fresh model by three contexts: both tables, the block table alone (pixel limit 0), no table.
Asserted:
    the path bits of every carve -- the third carve of the first context reads the pixels;
    selftest_pixel_cache finds no byte that differs from a recomputation;
    states, `listed` and `items` of the three contexts are equal carve by carve;
    the state equals the oracle's."""
import numpy as np
import pytest

from ar_voxel_project_amd import synthetic
from tests import rect_window, scenes
from tests.test_carve_gpu import assert_same
from tests.test_carve_paths_gpu import check_work, noise_scene, nontrivial
from tests.test_rect_cache_gpu import cached, flags_of, fresh_carves, same_answers

pytestmark = pytest.mark.gpu


def reads_pixels(arvx, info):
    return bool(info["bits"] & arvx.PATH_PIXEL_TABLE)


def table_bytes(dims, V, striped=False):
    """Bytes of the table of pixels: 1 KB per (record, view) -- records are padded to whole coarse
    tiles of 64 x 32 x 32 voxels, 64 records each -- plus the words of the views that do not fit."""
    X, Y, Z = dims
    cy, cz = (64, 8) if striped else (32, 32)
    coarse = -(-X // 64) * -(-Y // cy) * -(-Z // cz)
    return coarse * 64 * 1024 * V + ((V + 63) // 64 + 1) * 8


def check_case(arvx, want, dims, s, M, masks, what, pixels=True, blocks=True, limit=None, rect_limit=None,
               first=0, count=None, fits=None, **ctx_kw):
    """pixels / blocks: whether the second and third carve are expected to read the two tables.
    fits(list of bool per view): further assertions on the views that are read.  Returns that list."""
    nontrivial(want, what)
    with arvx.Context(*dims, s, **ctx_kw) as plain, arvx.Context(*dims, s, **ctx_kw) as block, \
            arvx.Context(*dims, s, **ctx_kw) as ctx:
        plain.set_rect_cache_limit(0)
        block.set_pixel_cache_limit(0)
        if limit is not None:
            ctx.set_pixel_cache_limit(limit)
        if rect_limit is not None:
            ctx.set_rect_cache_limit(rect_limit)
        for c in (plain, block, ctx):
            c.set_views(M, masks)
        ref = fresh_carves(arvx, plain, 3, f"{what} [no table]", first, count)
        mid = fresh_carves(arvx, block, 3, f"{what} [block table]", first, count)
        got = fresh_carves(arvx, ctx, 3, what, first, count)
        selftest = ctx.selftest_pixel_cache()
        views = ctx.pixel_cache_views(len(M))
        assert plain.selftest_pixel_cache() == -1 and block.selftest_pixel_cache() == -1, what
        assert not any(block.pixel_cache_views(len(M))), what
    for k in range(3):
        assert not cached(arvx, ref[k][1]) and not reads_pixels(arvx, ref[k][1]), f"{what} [no table] carve {k}"
        assert cached(arvx, mid[k][1]) == (k > 0) and not reads_pixels(arvx, mid[k][1]), f"{what} [block table] carve {k}"
        assert cached(arvx, got[k][1]) == (blocks and k > 0), f"{what} carve {k}: {got[k][1]}"
        assert reads_pixels(arvx, got[k][1]) == (pixels and k > 0), f"{what} carve {k}: {got[k][1]}"
        same_answers(got[k], ref[k], f"{what} carve {k}")
        same_answers(mid[k], ref[k], f"{what} [block table] carve {k}")
        assert_same(got[k][0], want, f"{what} carve {k}")
    check_work(got[2][1]["listed"], got[2][1]["items"], what)
    assert selftest == (0 if pixels else -1), f"{what}: self-test {selftest}"
    assert pixels or not any(views), what
    if fits:
        fits(views)
    return views


def test_ragged_grid(arvx, oracle):
    """No edge a multiple of a block's: blocks and lanes clipped by the grid."""
    dims = (40, 24, 20)
    s, _, M, masks = noise_scene(dims, 8, W=192, H=160, seed=401, block=5)
    check_case(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, "40x24x20")


def ring_scene(N, V, d, with_masks=True):
    """The sphere scene's ring cameras at distance d * extent, 640 x 480, the sphere's silhouettes."""
    E = synthetic.EXTENT
    K32 = synthetic.K_DATASET.astype(np.float32)
    Rt, centre = synthetic.ring_cameras(V, E, dist_factor=d)
    M = synthetic.compose_m(K32, Rt)
    masks = None
    if with_masks:
        masks = synthetic.sphere_masks(K32, Rt, centre, 0.35 * E, synthetic.IMAGE_W, synthetic.IMAGE_H)
    return np.float32(E / N), M, masks


def block_spans(N, s, M, W, H):
    """Per view the widest block rectangle that reads (pxhi - pxlo or pyhi - pylo), from the numpy
    restatement of rect_prepare."""
    boxes = rect_window.grid_boxes(N, N, N, rect_window.BOX_SIZES["block"])
    out = []
    for Mv in M:
        reads, pxlo, pxhi, pylo, pyhi = rect_window.rectangles(Mv, boxes, s, W, H)
        out.append(int(max((pxhi - pxlo)[reads].max(), (pyhi - pylo)[reads].max())) if reads.any() else 0)
    return out


def test_some_views_do_not_fit(arvx, oracle):
    """64^3 under ring cameras at a distance where the block rectangles of the views at the lower
    elevation are wider than 16 pixels and those of the others are not: a rectangle of span <= 15
    holds every pixel of its block within 15 of its origin, one of span >= 18 holds two more than a
    pixel of slack apart.  The views that overflow are projected, the rest read."""
    N, V, W, H = 64, 8, synthetic.IMAGE_W, synthetic.IMAGE_H
    chosen = None
    for d in np.arange(2.0, 6.0, 0.05):  # (on the CPU: the first distance with views of both kinds)
        s, M, _ = ring_scene(N, V, float(d), with_masks=False)
        spans = block_spans(N, s, M, W, H)
        if min(spans) <= 15 and max(spans) >= 18:
            chosen = (float(d), spans)
            break
    assert chosen, "no distance with fitting and overflowing views"
    d, spans = chosen
    s, M, masks = ring_scene(N, V, d)

    def fits(views):
        assert any(views) and not all(views), f"distance {d}: spans {spans}, fits {views}"
        for v, span in enumerate(spans):
            if span <= 15:
                assert views[v], f"view {v}: span {span} must fit"
            if span >= 18:
                assert not views[v], f"view {v}: span {span} cannot fit"

    check_case(arvx, oracle.carve(N, N, N, s, M, masks), (N, N, N), s, M, masks, f"ring at {d:.2f} E", fits=fits)


def test_cameras_close_and_inside(arvx, oracle):
    """Cameras close to and inside the grid: entries "outside" and "mixed without a look" among the
    blocks of the queued sub-tiles -- such a (sub-tile, view) pair is projected, its neighbours read."""
    dims = (70, 33, 40)
    s, _, M, masks = noise_scene(dims, 7, seed=311, block=3, inside=True)
    check_case(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, "cameras inside")


def test_two_chunks_and_a_view_range(arvx, oracle):
    """70 views of 64 x 48 pixels carved as carve_views(5, 65): two chunks, and a chunk's views are
    no aligned word of the mask of views that do not fit."""
    V, dims = 70, (40, 40, 40)
    s, _, M, masks = noise_scene(dims, V, W=64, H=48, seed=421, block=2, p_bg=0.05)
    want = oracle.carve(*dims, s, M[5:], masks[5:])
    check_case(arvx, want, dims, s, M, masks, "views 5..69", first=5, count=V - 5)


def test_slab_with_halo(arvx, oracle):
    dims, zr = (100, 40, 48), (13, 40)
    s, _, M, masks = noise_scene(dims, 5, seed=331, block=5)
    want = oracle.carve_planes(dims[0], dims[1], s, M, masks, np.arange(*zr))
    check_case(arvx, want, dims, s, M, masks, f"slab {zr} halo 2", z_range=zr, halo=2)


def test_striped(arvx, oracle):
    dims, world, rank = (70, 33, 40), 3, 1
    s, _, M, masks = noise_scene(dims, 9, seed=341, block=5)
    want = oracle.carve(*dims, s, M, masks)[arvx.stripe_planes(dims[2], world, rank)]
    check_case(arvx, want, dims, s, M, masks, "stripes 3/1", stripes=(world, rank))


def test_assoc_right(arvx, oracle):
    dims = (70, 33, 40)
    s, _, M, masks = noise_scene(dims, 6, seed=91, block=3)
    with oracle.variant("assoc_right"):
        want = oracle.carve(*dims, s, M, masks)
    check_case(arvx, want, dims, s, M, masks, "assoc right", assoc=arvx.ASSOC_RIGHT)


def test_assoc_changes_between_carves(arvx, oracle):
    """The table follows the grouping of the row sums: after a change the one that stands counts as
    none, and the next carve that could read it builds it again -- scenes.assoc_kat's voxel takes the
    state of the new grouping."""
    X, Y, Z, s, M, masks, (tx, ty, tz), st_right, st_left = scenes.assoc_kat(8)
    dims = (70, 33, 40)
    s2, _, M2, masks2 = noise_scene(dims, 6, seed=91, block=3)
    for (d, sv, Mv, mv) in (((X, Y, Z), s, M, masks), (dims, s2, M2, masks2)):
        with arvx.Context(*d, sv, assoc=arvx.ASSOC_LEFT) as ctx:
            ctx.set_views(Mv, mv)
            for name, assoc in (("assoc_left", arvx.ASSOC_LEFT), ("assoc_right", arvx.ASSOC_RIGHT),
                                ("assoc_left", arvx.ASSOC_LEFT)):
                with oracle.variant(name):
                    want = oracle.carve(*d, sv, Mv, mv)
                if d == (X, Y, Z):
                    assert want[tz, ty, tx] == (st_left if assoc == arvx.ASSOC_LEFT else st_right)
                ctx.set_assoc(assoc)
                got = fresh_carves(arvx, ctx, 3, f"{d} {name}")
                for k in range(3):
                    assert_same(got[k][0], want, f"{d} {name} carve {k}")
                assert reads_pixels(arvx, got[2][1]), f"{d} {name}: {got[2][1]}"
                assert ctx.selftest_pixel_cache() == 0, f"{d} {name}"
            ctx.set_assoc(arvx.ASSOC_RIGHT)
            assert ctx.selftest_pixel_cache() == -1, f"{d}: the other grouping's table counts as none"
            assert not any(ctx.pixel_cache_views(len(Mv)))


def test_validity(arvx, oracle):
    """A changed matrix, a new image size, another number of views: computed once more, then both
    tables again -- those of the new cameras.  A model that is not fresh and CARVE_NO_CULL read neither."""
    dims = (72, 40, 56)
    s, _, M, masks = noise_scene(dims, 5, seed=351, block=5)
    M2 = M.copy()
    M2[2] = noise_scene(dims, 5, seed=352)[2][4]
    s3, _, M3, masks3 = noise_scene(dims, 5, W=96, H=80, seed=353, block=3)
    s4, _, M4, masks4 = noise_scene(dims, 7, W=96, H=80, seed=354, block=3)
    assert s3 == s and s4 == s
    with arvx.Context(*dims, s) as ctx:
        for what, Mk, mk in (("first cameras", M, masks), ("one matrix changed", M2, masks),
                             ("new image size", M3, masks3), ("two more views", M4, masks4)):
            want = oracle.carve(*dims, s, Mk, mk)
            nontrivial(want, what)
            got = []
            for k in range(3):
                ctx.set_views(Mk, mk)  # (a pipeline sends its views with every batch of masks)
                got += fresh_carves(arvx, ctx, 1, f"{what} carve {k}")
            for k in range(3):
                assert cached(arvx, got[k][1]) == (k > 0), f"{what} carve {k}: {got[k][1]}"
                assert reads_pixels(arvx, got[k][1]) == (k > 0), f"{what} carve {k}: {got[k][1]}"
                assert_same(got[k][0], want, f"{what} carve {k}")
            assert ctx.selftest_pixel_cache() == 0, what
            ctx.carve(flags_of(arvx))  # not fresh
            info = ctx.last_carve_path()
            assert not cached(arvx, info) and not reads_pixels(arvx, info), f"{what}, not fresh: {info}"
            assert_same(ctx.download_state(), want, f"{what}, not fresh")
            ctx.reset()
            ctx.carve(arvx.CARVE_NO_CULL)
            info = ctx.last_carve_path()
            assert not cached(arvx, info) and not reads_pixels(arvx, info), f"{what}, no cull: {info}"
            assert_same(ctx.download_state(), want, f"{what}, no cull")


LIMIT_DIMS, LIMIT_V = (40, 24, 20), 8
LIMIT_NEED = table_bytes(LIMIT_DIMS, LIMIT_V)


@pytest.mark.parametrize("limit,rect_limit,pixels,blocks",
                         [(LIMIT_NEED - 1, None, False, True), (LIMIT_NEED, None, True, True),
                          (0, None, False, True), (None, 0, False, False)],
                         ids=["below", "at", "zero", "no-block-table"])
def test_limit(arvx, oracle, limit, rect_limit, pixels, blocks):
    """40 x 24 x 20 voxels, 8 views: one coarse tile of 64 records x 8 views x 1 KB, and two words of
    views that do not fit = 524 304 bytes.  Below the need, with limit 0 and without a block table
    there is no table of pixels."""
    assert LIMIT_NEED == 524304
    s, _, M, masks = noise_scene(LIMIT_DIMS, LIMIT_V, W=192, H=160, seed=401, block=5)
    check_case(arvx, oracle.carve(*LIMIT_DIMS, s, M, masks), LIMIT_DIMS, s, M, masks,
               f"limit {limit} / {rect_limit}", pixels=pixels, blocks=blocks, limit=limit, rect_limit=rect_limit)
