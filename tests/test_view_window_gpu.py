"""The view windows on the device (arvx.h, "View windows"): arvx_set_views writes only the part of
each summed-area table that the context's grid projects into.

Small images that still take the one-launch derivation (W a multiple of 64): 192 x 160 -- three tile
columns and the one of table column W, two and a half strips -- and 256 x 200.  The grids span 0.6 of
the extent the random cameras look at, so that they sit off-centre in the images: windows that leave
out tiles on different sides, windows clipped at an image edge, and -- cameras inside -- whole tables.

  in-window entries   the raw table inside the window is numpy's; outside it the poison is still
                      there (the tiles were skipped, not rewritten); the completed table is numpy's;
  poisoned table      every byte of the table buffer 0xA5, then set_views, reset, carve: the state is
                      the oracle's and that of a context with the window off -- on every carve path;
  changing cameras    the window moves with the matrices;
  completion          selftest_view_tables after a windowed derivation, then the carve again."""
import numpy as np
import pytest

from tests import scenes
from tests import vote_carve as vc
from tests.test_carve_gpu import assert_same
from tests.test_carve_paths_gpu import check_path, nontrivial

pytestmark = pytest.mark.gpu
E = 0.512
POISON = 0xA5


def scene(dims, V, W=192, H=160, seed=0, C=1, inside=False, block=5, frac=0.6):
    s = np.float32(frac * E / max(dims))
    _, _, M = scenes.random_cameras(V, E, seed=seed, W=W, H=H, inside=inside)
    masks = scenes.noise_masks(V, H, W, C=C, seed=seed + 1000, block=block)
    return s, M, masks


def whole(W, H):
    return (0, H, 0, (W + 1 + 63) // 64 * 64 - 1)


def np_table(mask):
    fg = ~(mask.reshape(mask.shape[0], mask.shape[1], -1) == 0).all(axis=2)
    H, W = fg.shape
    full = np.zeros((H + 1, W + 1), np.int64)
    full[1:, 1:] = np.cumsum(np.cumsum(fg, axis=0, dtype=np.int64), axis=1)
    return (full & 0xffff).astype(np.uint16)


def windows(ctx, V):
    return [ctx.view_window(v) for v in range(V)]


def some_partial(wins, W, H, what):
    assert any(w != whole(W, H) for w in wins), f"{what}: every view takes its whole table: {wins}"


def poisoned_views(ctx, M, masks):
    """set_views over a table buffer whose every byte is POISON"""
    ctx.set_views(M, masks)
    ctx.selftest_fill_view_tables(POISON)
    ctx.set_views(M, masks)


def check_carve(arvx, want, dims, s, M, masks, what, carve, **ctx_kw):
    """carve(ctx) -> state, on a context with windows over a poisoned table and on one without."""
    _, H, W = masks.shape[:3]
    with arvx.Context(*dims, s, **ctx_kw) as ctx, arvx.Context(*dims, s, **ctx_kw) as plain:
        plain.set_view_window(False)
        poisoned_views(ctx, M, masks)
        plain.set_views(M, masks)
        wins = windows(ctx, len(M))
        assert windows(plain, len(M)) == [whole(W, H)] * len(M), what
        got = carve(ctx)
        ref = carve(plain)
    some_partial(wins, W, H, what)
    assert_same(ref, want, f"{what} [window off]")
    assert_same(got, want, what)


def fresh_carve(flags=0, path=None):
    def run(ctx):
        ctx.reset()
        ctx.carve(flags)
        if path:
            path(ctx.last_carve_path())
        return ctx.download_state()
    return run


@pytest.mark.parametrize("W,H,C", [(192, 160, 1), (256, 200, 1), (192, 160, 3)])
def test_entries_inside_the_window(arvx, W, H, C):
    V, dims = 6, (64, 64, 64)
    s, M, masks = scene(dims, V, W=W, H=H, seed=402, C=C, block=7)
    masks[1] = 255  # every pixel foreground
    with arvx.Context(*dims, s) as ctx:
        poisoned_views(ctx, M, masks)
        wins = windows(ctx, V)
        some_partial(wins, W, H, f"{W}x{H}x{C}")
        for v in range(V):
            r0, r1, c0, c1 = wins[v]
            want = np_table(masks[v])
            raw = ctx.selftest_view_table_raw(v, H)
            inside = np.zeros(raw.shape, bool)
            inside[r0:r1 + 1, c0:c1 + 1] = True
            cols = np.arange(raw.shape[1]) <= W  # (beyond column W: the rows' padding, any value)
            bad = np.argwhere((raw[:, :W + 1] != want) & inside[:, :W + 1])
            assert bad.size == 0, f"view {v}: {len(bad)} entries in the window {wins[v]} differ, first at {bad[0]}"
            assert (raw[~inside & cols[None, :]] == POISON * 0x101).all(), f"view {v}: entries outside {wins[v]} written"
        for v in range(V):  # (completes the tables at its first call)
            _, table = ctx.selftest_view_tables(v, W, H)
            assert np.array_equal(table, np_table(masks[v])), f"view {v}: completed table"
            raw = ctx.selftest_view_table_raw(v, H)
            assert np.array_equal(raw[:, :W + 1], table), f"view {v}: raw table after the completion"


def test_poisoned_default_path_dense(arvx, oracle):
    """The large grids' kernels (dense classify, block-mapped exact kernel) on 64^3; carved three
    times, so that the block rectangles of the second and third carve come from the cache."""
    dims = (64, 64, 64)
    s, M, masks = scene(dims, 6, seed=402)
    want = oracle.carve(*dims, s, M, masks)
    nontrivial(want, "dense")
    flags = arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS

    def carve(ctx):
        out = None
        for k in range(3):
            ctx.reset()
            ctx.carve(flags)
            check_path(arvx, ctx.last_carve_path(), flags, f"carve {k}", fresh=True)
            st = ctx.download_state()
            assert out is None or np.array_equal(out, st), f"carve {k} differs from carve 0"
            out = st
        return out
    check_carve(arvx, want, dims, s, M, masks, "dense", carve)


def test_poisoned_dense_classify_shared_items(arvx, oracle):
    dims = (72, 40, 56)
    s, M, masks = scene(dims, 5, W=256, H=200, seed=403)
    want = oracle.carve(*dims, s, M, masks)
    nontrivial(want, "dense, shared items")
    flags = arvx.CARVE_DENSE_CLASSIFY
    check_carve(arvx, want, dims, s, M, masks, "dense, shared items",
                fresh_carve(flags, lambda info: check_path(arvx, info, flags, "dense, shared items", fresh=True)))


def test_poisoned_small_grid_item_sharing(arvx, oracle):
    dims = (33, 17, 40)
    s, M, masks = scene(dims, 6, seed=401, block=3)
    want = oracle.carve(*dims, s, M, masks)
    nontrivial(want, "small grid")

    def path(info):
        assert info["bits"] & arvx.PATH_ITEM_SHARING and not info["bits"] & arvx.PATH_DENSE_CLASSIFY, info
    check_carve(arvx, want, dims, s, M, masks, "small grid", fresh_carve(0, path))


def test_poisoned_not_fresh_and_fused(arvx, oracle):
    """A model that is not fresh (the second carve reads the records), and the fused kernel."""
    dims = (40, 40, 40)
    s, M, masks = scene(dims, 6, seed=402, block=3)
    want = oracle.carve(*dims, s, M, masks)
    nontrivial(want, "not fresh")

    def twice(ctx):
        ctx.reset()
        ctx.carve_views(0, 3)
        ctx.carve_views(3, 3)
        return ctx.download_state()
    check_carve(arvx, want, dims, s, M, masks, "not fresh", twice)
    check_carve(arvx, want, dims, s, M, masks, "fused", fresh_carve(arvx.CARVE_FUSED))


def test_poisoned_slab_with_halo(arvx, oracle):
    dims, zr = (100, 40, 48), (13, 40)
    s, M, masks = scene(dims, 5, seed=403)
    want = oracle.carve_planes(dims[0], dims[1], s, M, masks, np.arange(*zr))
    nontrivial(want, "slab")
    for flags in (0, arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS):
        check_carve(arvx, want, dims, s, M, masks, f"slab {zr} halo 2, flags {flags}", fresh_carve(flags),
                    z_range=zr, halo=2)


def test_poisoned_stripes(arvx, oracle):
    dims, world, rank = (70, 33, 40), 3, 1
    s, M, masks = scene(dims, 6, seed=402)
    want = oracle.carve(*dims, s, M, masks)[arvx.stripe_planes(dims[2], world, rank)]
    nontrivial(want, "stripes")
    for flags in (0, arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS):
        check_carve(arvx, want, dims, s, M, masks, f"stripes 3/1, flags {flags}", fresh_carve(flags),
                    stripes=(world, rank))


def test_poisoned_no_cull(arvx, oracle):
    """The brute-force carve reads no table at all: the bit planes are complete."""
    dims = (33, 17, 40)
    s, M, masks = scene(dims, 6, seed=401, block=3)
    want = oracle.carve(*dims, s, M, masks)

    def path(info):
        assert info["bits"] & arvx.PATH_BRUTE_FORCE, info
    check_carve(arvx, want, dims, s, M, masks, "no cull", fresh_carve(arvx.CARVE_NO_CULL, path))


@pytest.mark.parametrize("assoc", [1, 0])
def test_poisoned_vote_carve(arvx, oracle, assoc):
    dims = (64, 48, 32)
    s, M, masks = scene(dims, 6, seed=402, block=9)
    votes = vc.counts(oracle, *dims, s, M, masks, assoc == 1)
    fresh = oracle.fresh_state(*dims)
    for K in (0, 2):
        want = vc.apply(votes, fresh, K).reshape(fresh.shape)
        nontrivial(want, f"votes {K}")

        def carve(ctx):
            ctx.reset()
            ctx.carve_votes(K, counts=True)
            bg, inside = ctx.votes()
            assert np.array_equal(bg, votes.background) and np.array_equal(inside, votes.inside), K
            ctx.reset()
            ctx.carve_votes(K)  # (the early exits)
            return ctx.download_state()
        check_carve(arvx, want, dims, s, M, masks, f"votes {K}", carve, assoc=assoc)


def test_changing_cameras(arvx, oracle):
    """New matrices between two derivations: the window moves, and what the first derivation left
    outside its window is not read by the second carve.  Then the first cameras again, with other
    masks: the entries the second window did not cover are those of the old masks until rewritten."""
    dims = (64, 64, 64)
    s, M1, masks1 = scene(dims, 6, seed=402)
    _, M2, masks2 = scene(dims, 6, seed=403)
    flags = arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS
    with arvx.Context(*dims, s) as ctx:
        poisoned_views(ctx, M1, masks1)
        seen = []
        for what, M, masks in (("first", M1, masks1), ("second", M2, masks2), ("first again", M1, masks2),
                               ("second, flags 0", M2, masks1)):
            ctx.set_views(M, masks)
            seen.append(windows(ctx, 6))
            ctx.reset()
            ctx.carve(0 if "flags 0" in what else flags)
            want = oracle.carve(*dims, s, M, masks)
            nontrivial(want, what)
            assert_same(ctx.download_state(), want, what)
    some_partial(seen[0], 192, 160, "first")
    some_partial(seen[1], 192, 160, "second")
    assert seen[0] != seen[1] and seen[2] == seen[0] and seen[3] == seen[1], seen


def test_image_edge_and_whole_table_three_channels(arvx, oracle):
    """Cameras close to and inside the grid, three-channel masks (views_strip_kernel<3>): windows
    clipped at an image edge (they start at row or column 0, or end at the last) beside a view that
    takes its whole table."""
    dims, W, H = (64, 64, 64), 192, 160
    s, M, masks = scene(dims, 6, seed=402, C=3, inside=True)
    want = oracle.carve(*dims, s, M, masks)
    nontrivial(want, "image edge")
    with arvx.Context(*dims, s) as ctx:
        poisoned_views(ctx, M, masks)
        wins = windows(ctx, 6)
        for flags in (0, arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS):
            ctx.reset()
            ctx.carve(flags)
            assert_same(ctx.download_state(), want, f"image edge, flags {flags}")
    full = whole(W, H)
    assert full in wins, wins
    clipped = [w for w in wins if w != full and (w[0] == 0 or w[1] == H or w[2] == 0 or w[3] == full[3])]
    assert clipped, wins


def test_completion_then_carve(arvx, oracle):
    dims = (64, 64, 64)
    s, M, masks = scene(dims, 6, seed=402)
    want = oracle.carve(*dims, s, M, masks)
    flags = arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS
    with arvx.Context(*dims, s) as ctx:
        poisoned_views(ctx, M, masks)
        ctx.reset()
        ctx.carve(flags)
        first = ctx.download_state()
        for v in range(6):
            _, table = ctx.selftest_view_tables(v, 192, 160)
            assert np.array_equal(table, np_table(masks[v])), v
        assert windows(ctx, 6) != [whole(192, 160)] * 6  # (the windows are the last derivation's)
        ctx.reset()
        ctx.carve(flags)
        assert_same(ctx.download_state(), first, "after the completion")
        assert_same(first, want, "windowed")
        ctx.set_views(M, masks)  # partial again
        ctx.reset()
        ctx.carve(flags)
        assert_same(ctx.download_state(), want, "derived again")


def test_window_switch(arvx):
    """Off: whole tables from the next derivation on; on again: the cameras' windows."""
    dims, W, H = (64, 64, 64), 192, 160
    s, M, masks = scene(dims, 6, seed=402)
    with arvx.Context(*dims, s) as ctx:
        ctx.set_views(M, masks)
        on = windows(ctx, 6)
        ctx.set_view_window(False)
        assert windows(ctx, 6) == on  # (what the last derivation wrote)
        ctx.set_views(M, masks)
        assert windows(ctx, 6) == [whole(W, H)] * 6
        ctx.set_view_window(True)
        ctx.set_views(M, masks)
        assert windows(ctx, 6) == on
        # masks of a format the one-launch derivation does not take: whole tables
        m2 = scenes.noise_masks(6, 150, 190, seed=5, block=5)
        _, _, M2 = scenes.random_cameras(6, E, seed=402, W=190, H=150)
        ctx.set_views(M2, m2)
        assert windows(ctx, 6) == [whole(190, 150)] * 6
        for v in range(6):
            _, table = ctx.selftest_view_tables(v, 190, 150)
            assert np.array_equal(table, np_table(m2[v])), v
