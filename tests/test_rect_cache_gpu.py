"""The table of cached block rectangles (arvx.h, arvx_ctx_set_rect_cache_limit) against the carve
that computes its rectangles, and against the CPU oracle.

From its second consecutive carve under the same cameras a context that runs the large grids'
kernels loads the pixel rectangles of its 4 x 4 x 4 blocks (exact kernel, fresh model, unshared
items) from a table instead of computing them.  Every case here is a small grid pushed onto those
kernels with CARVE_DENSE_CLASSIFY | CARVE_WHOLE_ITEMS, as tests/test_carve_paths_gpu.py does, carved
several times from a fresh model by two contexts: one with the table, one with the limit set to 0.
Asserted for every carve:
    the path bit says whether the block tests came from the table;
    selftest_rect_cache finds no entry that differs from a recomputation;
    the states of the two contexts are equal, and so are `listed` and `items` of
    last_carve_path -- the answers of the tests did not move, not only the final voxels;
    the state equals the oracle's."""
import numpy as np
import pytest

from tests.test_carve_gpu import assert_same
from tests.test_carve_paths_gpu import check_path, check_work, noise_scene, nontrivial

pytestmark = pytest.mark.gpu


def flags_of(arvx):
    return arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS


def cached(arvx, info):
    return bool(info["bits"] & arvx.PATH_RECT_BLOCKS)


def fresh_carves(arvx, ctx, n, what, first=0, count=None):
    """n carves of a fresh model: [(state, info)]"""
    out = []
    for k in range(n):
        ctx.reset()
        if count is None:
            ctx.carve(flags_of(arvx))
        else:
            ctx.carve_views(first, count, flags_of(arvx))
        info = ctx.last_carve_path()
        check_path(arvx, info, flags_of(arvx), f"{what} carve {k}", fresh=True)
        out.append((ctx.download_state(), info))
    return out


def same_answers(a, b, what):
    assert_same(a[0], b[0], what)
    assert (a[1]["listed"], a[1]["items"]) == (b[1]["listed"], b[1]["items"]), f"{what}: {a[1]} / {b[1]}"


def check_case(arvx, want, dims, s, M, masks, what, table=True, limit=None, first=0, count=None, **ctx_kw):
    """Three fresh carves with the table and three without; table: whether the block tests are
    expected to come from it from the second carve on."""
    nontrivial(want, what)
    with arvx.Context(*dims, s, **ctx_kw) as plain, arvx.Context(*dims, s, **ctx_kw) as ctx:
        plain.set_rect_cache_limit(0)
        if limit is not None:
            ctx.set_rect_cache_limit(limit)
        for c in (plain, ctx):
            c.set_views(M, masks)
        ref = fresh_carves(arvx, plain, 3, f"{what} [no table]", first, count)
        got = fresh_carves(arvx, ctx, 3, what, first, count)
        selftest = ctx.selftest_rect_cache()
        assert plain.selftest_rect_cache() == -1, what
    for k in range(3):
        assert not cached(arvx, ref[k][1]), f"{what} [no table] carve {k}: {ref[k][1]}"
        assert cached(arvx, got[k][1]) == (table and k > 0), f"{what} carve {k}: {got[k][1]}"
        same_answers(got[k], ref[k], f"{what} carve {k}")
        assert_same(got[k][0], want, f"{what} carve {k}")
    check_work(got[2][1]["listed"], got[2][1]["items"], what)
    assert selftest == (0 if table else -1), f"{what}: self-test {selftest}"


def test_ragged_grid(arvx, oracle):
    """No edge a multiple of a tile: clipped boxes, sub-tiles and blocks partly outside the grid."""
    dims = (72, 40, 56)
    s, _, M, masks = noise_scene(dims, 5, seed=301, block=5)
    check_case(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, "72x40x56")


def test_cameras_close_and_inside(arvx, oracle):
    """Cameras close to and inside the grid: rectangles outside the image, and boxes whose
    denominator may vanish ("mixed" without a look)."""
    dims = (70, 33, 40)
    s, _, M, masks = noise_scene(dims, 7, seed=311, block=3, inside=True)
    check_case(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, "cameras inside")


def test_two_chunks_and_a_view_range(arvx, oracle):
    """More than 64 views at a tiny image size, carved as carve_views(5, V - 5): two chunks of masks,
    v0 > 0 -- the table is indexed by the context's view, not by the carve's."""
    V, dims = 70, (40, 40, 40)
    s, _, M, masks = noise_scene(dims, V, W=48, H=36, seed=321, block=2, p_bg=0.05)
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


def test_validity(arvx, oracle):
    """First carve: computed.  Second and third: from the table.  A changed matrix, then a new image
    size: computed once more, then from the table again -- that of the new cameras.  A carve of a
    model that is not fresh computes (its exact kernel has no table variant)."""
    dims = (72, 40, 56)
    s, _, M, masks = noise_scene(dims, 5, seed=351, block=5)
    M2 = M.copy()
    M2[2] = noise_scene(dims, 5, seed=352)[2][4]
    s3, _, M3, masks3 = noise_scene(dims, 5, W=96, H=80, seed=353, block=3)
    assert s3 == s
    with arvx.Context(*dims, s) as ctx, arvx.Context(*dims, s) as plain:
        plain.set_rect_cache_limit(0)
        for what, Mk, mk in (("first cameras", M, masks), ("one matrix changed", M2, masks),
                             ("new image size", M3, masks3)):
            want = oracle.carve(*dims, s, Mk, mk)
            nontrivial(want, what)
            plain.set_views(Mk, mk)
            ref = fresh_carves(arvx, plain, 1, f"{what} [no table]")[0]
            assert_same(ref[0], want, f"{what} [no table]")
            got = []
            for k in range(3):
                ctx.set_views(Mk, mk)  # (a pipeline sends its views with every batch of masks)
                got += fresh_carves(arvx, ctx, 1, f"{what} carve {k}")
            for k in range(3):
                assert cached(arvx, got[k][1]) == (k > 0), f"{what} carve {k}: {got[k][1]}"
                same_answers(got[k], ref, f"{what} carve {k}")
            assert ctx.selftest_rect_cache() == 0, what
            ctx.carve(flags_of(arvx))  # not fresh
            info = ctx.last_carve_path()
            assert not cached(arvx, info), f"{what}, not fresh: {info}"
            assert_same(ctx.download_state(), want, f"{what}, not fresh")


def test_block_rectangle_too_large_for_an_entry(arvx, oracle):
    """Images of 1100 x 1030 pixels leave a block entry five bits for a rectangle's width and height;
    a 4 x 4 x 4 block of a 40^3 grid that fills the image spans about a hundred pixels.  The table
    is given up and the results are equal."""
    dims = (40, 40, 40)
    s, _, M, masks = noise_scene(dims, 3, W=1100, H=1030, seed=361, block=9)
    check_case(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, "large rectangles", table=False)


@pytest.mark.parametrize("limit,table", [(1000, False), (163839, False), (163840, True)])
def test_limit(arvx, oracle, limit, table):
    """72 x 40 x 56 voxels, 5 views: 512 records x 16 blocks x 5 views x 4 bytes = 163 840 bytes; a
    limit below the need leaves the carve without a table."""
    dims = (72, 40, 56)
    s, _, M, masks = noise_scene(dims, 5, seed=301, block=5)
    check_case(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, f"limit {limit}", table=table, limit=limit)
