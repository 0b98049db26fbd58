"""The large grids' carve kernels on small grids, against the CPU oracle.

arvx_carve chooses two of its kernels by the number of voxels: from 2^26 voxels on the sub-tile
classification is carve_classify_dense_kernel, and above 2^26 the exact kernel runs its unshared
instantiations <LEFT, false, FRESH>.  Those carve the benchmark's 512^3 and the 1024^3 target, and
no small scene reaches them on its own.  The path flags (include/arvx/arvx.h) take that choice on
any grid:
    DENSE | WHOLE   what a grid above 2^26 voxels runs
    DENSE           the combination of a grid of exactly 2^26 voxels (dense classify, shared items)
Every case here runs under both unless it says otherwise, compares the whole state plane with the
oracle exactly, and asserts from Context.last_carve_path() that the intended kernels ran and had
work: at least one coarse tile listed and one sub-tile queued -- or the module could silently go
back to testing the small grids' kernels.  The oracle's plane of every case holds occupied and
carved voxels (0 < occupied fraction < 1), so that no trivial scene passes.  The all-background
and all-foreground masks and two of the extreme geometries cannot have either property; each says
so where it is exempt, and asserts that its plane is indeed constant."""
import numpy as np
import pytest

from tests import scenes
from tests.test_carve_gpu import assert_same, planes_of

pytestmark = pytest.mark.gpu

E = 0.512  # extent the cameras of scenes.random_cameras frame


def paths(arvx):
    d, w = arvx.CARVE_DENSE_CLASSIFY, arvx.CARVE_WHOLE_ITEMS
    return (("dense+whole", d | w), ("dense", d))


def check_path(arvx, info, flags, what, fresh=None, sharing=None):
    """The kernels `flags` ask for are the ones the last carve launched."""
    bits = info["bits"]
    assert bits & arvx.PATH_DENSE_CLASSIFY and info["dense_grid"] > 0, f"{what}: not the dense classify kernel: {info}"
    assert not bits & (arvx.PATH_FUSED | arvx.PATH_BRUTE_FORCE | arvx.PATH_STREAM), f"{what}: not the split carve: {info}"
    if sharing is None:
        sharing = not flags & arvx.CARVE_WHOLE_ITEMS
    assert bool(bits & arvx.PATH_ITEM_SHARING) == sharing, f"{what}: item sharing: {info}"
    if fresh is not None:
        assert bool(bits & arvx.PATH_FRESH) == fresh, f"{what}: fresh: {info}"


def check_work(listed, items, what):
    assert listed >= 1, f"{what}: no coarse tile listed"
    assert items >= 1, f"{what}: no sub-tile queued for the exact kernel"


def nontrivial(want, what):
    occ = float((want & 1).mean())
    assert 0.0 < occ < 1.0, f"{what}: trivial scene, occupied fraction {occ}"


def carve_on_path(arvx, dims, s, M, masks, flags, what, steps=None, state=None, work=True, after_step=None,
                  **ctx_kw):
    """The state after carve_views(first, count, flags) for every step (default: all views at once),
    from a fresh model or from `state`; the path of every step and the work of all are checked.
    after_step(k, ctx): called after step k."""
    X, Y, Z = dims
    with arvx.Context(X, Y, Z, s, **ctx_kw) as ctx:
        ctx.set_views(M, masks)
        if state is not None:
            ctx.upload_state(state)
        listed = items = 0
        for k, (first, count) in enumerate(steps or [(0, len(M))]):
            ctx.carve_views(first, count, flags)
            info = ctx.last_carve_path()
            check_path(arvx, info, flags, f"{what} step {k}", fresh=(state is None and k == 0))
            listed += info["listed"]
            items += info["items"]
            if after_step:
                after_step(k, ctx)
        got = ctx.download_state()
    if work:
        check_work(listed, items, what)
    return got


def both_paths(arvx, want, dims, s, M, masks, what, trivial=False, **kw):
    if trivial:
        assert float((want & 1).mean()) in (0.0, 1.0), f"{what}: exempt as a constant plane, and is none"
    else:
        nontrivial(want, what)
    for name, flags in paths(arvx):
        got = carve_on_path(arvx, dims, s, M, masks, flags, f"{what} [{name}]", work=not trivial, **kw)
        assert_same(got, want, f"{what} [{name}]")


def noise_scene(dims, V, W=160, H=120, seed=0, inside=False, **mask_kw):
    s = np.float32(E / max(dims))
    _, Rt, M = scenes.random_cameras(V, E, seed=seed, W=W, H=H, inside=inside)
    masks = scenes.noise_masks(V, H, W, seed=seed + 1000, **mask_kw)
    return s, Rt, M, masks


def ball_noise_scene(V, W, H, seed, p_bg=0.3):
    """Random cameras outside a ball in the middle of the grid; the masks are the ball's silhouette
    on noise: what lies in the ball survives any number of views, everything else is carved pixel
    by pixel.  About a quarter of a mask is background."""
    K, Rt, M = scenes.random_cameras(V, E, seed=seed, W=W, H=H)
    ball = scenes.syn.sphere_masks(K, Rt, np.array([E / 2, E / 2, -E / 2]), 0.3 * E, W=W, H=H)
    noise = scenes.noise_masks(V, H, W, p_bg=p_bg, block=2, seed=seed + 1000)
    return M, np.where(ball > 0, ball, noise).astype(np.uint8)


# ---- grid edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(10, 10, 5), (64, 32, 32), (65, 33, 33), (70, 9, 33), (33, 17, 9),
                                  (130, 20, 20), (100, 100, 50), (2112, 8, 9), (8, 2112, 9), (9, 8, 2112)])
def test_grid_edges(arvx, oracle, dims):
    """Exactly one coarse tile (64 x 32 x 32); edge coarse tiles that hold one voxel layer, so that
    most of their sub-tiles lie outside the grid; ragged x, y and z; thousands of coarse tiles along
    one axis."""
    s, _, M, masks = noise_scene(dims, 5, seed=sum(dims), block=5)
    both_paths(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, f"grid {dims}")


# ---- view grouping --------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 3, 4, 5, 15, 16, 17, 36, 63, 64, 65, 130, 256])
def test_view_grouping(arvx, oracle, V):
    """A quarter unit of the dense kernel packs 4 of the coarse tile's mixed views per wave group,
    the groups dealt to 4 waves: view counts below, at and above one group, one round of the waves
    (16) and one chunk (64), up to the 256 the split carve takes.  Small images and little
    background keep most views mixed."""
    dims = (40, 40, 40)
    s = np.float32(E / 40)
    M, masks = ball_noise_scene(V, 48, 36, seed=V)
    both_paths(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, f"V={V}")


# ---- view ranges ----------------------------------------------------------------------------------

def test_view_range_across_two_chunks(arvx, oracle):
    """carve_views(37, 63) then carve_views(0, 37) of 100 views: v0 is no multiple of 64, and the
    views 37..99 lie on both sides of view 64 while being one chunk of their carve."""
    V, dims = 100, (40, 40, 40)
    s = np.float32(E / 40)
    M, masks = ball_noise_scene(V, 48, 36, seed=21)
    want = oracle.carve(*dims, s, M, masks)
    both_paths(arvx, want, dims, s, M, masks, "views 37.. then 0..37", steps=[(37, V - 37), (0, 37)])
    # ... and a range of two chunks that starts inside the first
    first = oracle.carve(*dims, s, M[5:], masks[5:])
    nontrivial(first, "views 5..99")
    for name, flags in paths(arvx):
        got = carve_on_path(arvx, dims, s, M, masks, flags, f"views 5..99 [{name}]", steps=[(5, V - 5)])
        assert_same(got, first, f"views 5..99 [{name}]")


def test_view_by_view_in_random_order(arvx, oracle):
    V, dims = 9, (70, 33, 40)
    s, _, M, masks = noise_scene(dims, V, seed=31, block=3)
    order = [int(i) for i in np.random.default_rng(32).permutation(V)]
    after = [oracle.fresh_state(*dims)]  # the oracle's plane after every step
    for i in order:
        after.append(oracle.carve_view(*dims, s, M[i], masks[i], after[-1]))
    nontrivial(after[-1], "view by view")
    for name, flags in paths(arvx):
        def same_after(k, ctx):
            assert_same(ctx.download_state(), after[k + 1], f"after view {order[k]} [{name}]")

        got = carve_on_path(arvx, dims, s, M, masks, flags, f"view by view [{name}]",
                            steps=[(i, 1) for i in order], after_step=same_after)
        assert_same(got, after[-1], f"view by view [{name}]")


# ---- models that are not fresh --------------------------------------------------------------------

def test_random_uploaded_state(arvx, oracle):
    """Every combination of occupied / seen, 4 % of the voxels carved and seen already: the records
    are read before they are written, and sub-tiles that no view decides keep what they hold."""
    dims = (70, 33, 40)
    s, _, M, masks = noise_scene(dims, 5, seed=41, block=5)
    rng = np.random.default_rng(42)
    st0 = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=dims[::-1], p=[0.16, 0.4, 0.04, 0.4])
    want = oracle.carve(*dims, s, M, masks, state=st0)
    both_paths(arvx, want, dims, s, M, masks, "random uploaded state", state=st0)


def test_same_carve_twice(arvx, oracle):
    dims = (100, 40, 48)
    s, _, M, masks = noise_scene(dims, 5, seed=51, block=5)
    want = oracle.carve(*dims, s, M, masks)
    both_paths(arvx, want, dims, s, M, masks, "carve twice", steps=[(0, 5), (0, 5)])


def test_tile_summary_is_dropped_on_the_large_grid_path(arvx, oracle):
    """The sequence of test_tile_summary_is_dropped_when_something_else_writes_the_state (upload,
    upload of planes, closure, carve again) with the large grids' kernels.  Its one flat view
    decides every coarse tile as a whole -- the mask's border lies on a coarse-tile border --, so no
    step queues a sub-tile (asserted).  A fresh model lists nothing either, nor does a second carve
    while the summary stands; once it is dropped, the carve of a model that is not fresh lists the
    tiles whose voxels keep their occupancy."""
    X, Y, Z = 64, 96, 64
    s = np.float32(0.01)
    M = scenes.flat_view(X, Y, s)
    masks = np.full((1, Y, X), 255, np.uint8)
    masks[0, :32, :] = 0
    want1 = oracle.carve(X, Y, Z, s, M, masks)
    nontrivial(want1, "flat view")
    flags = arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, masks)

        def carve(what, fresh=False):
            ctx.carve(flags)
            info = ctx.last_carve_path()
            check_path(arvx, info, flags, what, fresh=fresh)
            assert info["items"] == 0, f"{what}: {info}"
            return info

        assert carve("first carve", fresh=True)["listed"] == 0
        assert_same(ctx.download_state(), want1, "first carve")
        assert carve("second carve")["listed"] == 0  # (the summary settles every tile)
        assert_same(ctx.download_state(), want1, "second carve")
        full = np.full((Z, Y, X), 1, np.uint8)
        ctx.upload_state(full)
        assert carve("after an upload")["listed"] >= 1
        assert_same(ctx.download_state(), want1, "after an upload")
        ctx.upload_planes(*planes_of(full))
        assert carve("after an upload of planes")["listed"] >= 1
        assert_same(ctx.download_state(), want1, "after an upload of planes")
        idx, _ = ctx.closure(3, True)
        after = ctx.download_state()
        filled = np.zeros(X * Y * Z, bool)
        filled[idx] = True
        filled = filled.reshape(Z, Y, X)
        assert filled[:, 31, :].all() and not filled[:, :31, :].any()
        assert carve("after the closure")["listed"] >= 1
        assert_same(ctx.download_state(), oracle.carve(X, Y, Z, s, M, masks, state=after), "after the closure")
        assert ((ctx.download_state() & 1) == 0)[filled].all()


# ---- masks ----------------------------------------------------------------------------------------

MASK_DIMS = (70, 40, 36)


@pytest.mark.parametrize("fill", [0, 255])
def test_all_background_and_all_foreground(arvx, oracle, fill):
    """No rectangle is mixed: every coarse tile is decided as a whole, nothing is listed or queued
    and the plane is all carved or all occupied (exempt from both checks), but the launches run."""
    s, _, M, _ = noise_scene(MASK_DIMS, 4, seed=61)
    masks = np.full((4, 120, 160), fill, np.uint8)
    want = oracle.carve(*MASK_DIMS, s, M, masks)
    both_paths(arvx, want, MASK_DIMS, s, M, masks, f"fill {fill}", trivial=True)


@pytest.mark.parametrize("kw", [dict(block=1), dict(block=5), dict(block=64, seed=66), dict(block=2, p_bg=0.02),
                                dict(block=2, p_bg=0.9), dict(block=3, C=3), dict(block=3, W=33, H=17),
                                dict(block=3, W=97, H=61, C=3), dict(block=7, W=640, H=480)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k != "seed"))
def test_masks(arvx, oracle, kw):
    """Single-pixel noise (every sub-tile becomes an item), blocks near a sub-tile's rectangle and
    far beyond it (rectangles decided at either level), hardly any and mostly background, one and
    three channels, image widths that are no multiple of 32."""
    kw = dict(kw)
    W, H = kw.pop("W", 160), kw.pop("H", 120)
    s, _, M, masks = noise_scene(MASK_DIMS, 4, W=W, H=H, seed=kw.pop("seed", 71 + W), **kw)
    want = oracle.carve(*MASK_DIMS, s, M, masks)
    both_paths(arvx, want, MASK_DIMS, s, M, masks, f"masks {kw} {W}x{H}")


# ---- geometry -------------------------------------------------------------------------------------

def test_cameras_inside_the_grid(arvx, oracle):
    dims, V = (48, 48, 48), 7
    s, Rt, M, masks = noise_scene(dims, V, seed=81, inside=True, block=2)
    cam = np.array([-Rt[i, :, :3].astype(np.float64).T @ Rt[i, :, 3] for i in range(V)])
    inside = np.all((cam >= [0, 0, -E]) & (cam <= [E, E, 0]), axis=1)
    assert inside.sum() >= 2, "the scene is meant to have cameras inside the grid"
    both_paths(arvx, oracle.carve(*dims, s, M, masks), dims, s, M, masks, "cameras inside")


# Scenes in which nothing is mixed, exempt like the constant masks: the principal point of
# offcentre_principal lies so far outside the image that no view sees any voxel (the oracle's
# plane: all occupied, none seen), and far_camera's grid covers about one pixel, which the masks of
# block 12 make background in some view for all of it (all carved).
NOTHING_MIXED = {("offcentre_principal", 1), ("offcentre_principal", 12), ("far_camera", 12)}


@pytest.mark.parametrize("case", scenes.EXTREME_GEOMETRY_CASES)
def test_extreme_geometry(arvx, oracle, case):
    """test_carve_gpu.py::test_extreme_geometry's scenes: the margins of the rectangle tests scale
    with |M|, |w| and 1/depth."""
    N, V, W, H, s, M = scenes.extreme_geometry(case)
    s = np.float32(s)
    for block in (1, 12):
        masks = scenes.noise_masks(V, H, W, block=block, p_bg=0.5, seed=block)
        want = oracle.carve(N, N, N, s, M, masks)
        both_paths(arvx, want, (N, N, N), s, M, masks, f"{case} block={block}",
                   trivial=(case, block) in NOTHING_MIXED)


# ---- association ----------------------------------------------------------------------------------

@pytest.mark.parametrize("carved", [False, True], ids=["fresh", "carved"])
@pytest.mark.parametrize("name,assoc", [("assoc_left", 1), ("assoc_right", 0)])
def test_association(arvx, oracle, name, assoc, carved):
    """Both groupings of the M*world row sums on a fresh and on a carved model: under DENSE | WHOLE
    the four instantiations <LEFT, false, FRESH> of the exact kernel.  scenes.assoc_kat's voxel
    tells the groupings apart; a noise scene checks the rest of the plane."""
    X, Y, Z, s, M, masks, (tx, ty, tz), st_right, st_left = scenes.assoc_kat(8)
    state = np.full((Z, Y, X), 1, np.uint8) if carved else None
    with oracle.variant(name):
        want = oracle.carve(X, Y, Z, s, M, masks)
    assert want[tz, ty, tx] == (st_left if assoc else st_right)
    both_paths(arvx, want, (X, Y, Z), s, M, masks, f"kat {name}", state=state, assoc=assoc)
    dims = (70, 33, 40)
    s, _, M, masks = noise_scene(dims, 6, seed=91, block=3)
    state = None
    if carved:
        state = np.random.default_rng(92).choice(np.array([0, 1, 2, 3], np.uint8), size=dims[::-1])
    with oracle.variant(name):
        want = oracle.carve(*dims, s, M, masks, state=state)
    both_paths(arvx, want, dims, s, M, masks, f"noise {name}", state=state, assoc=assoc)


# ---- slabs and stripes ----------------------------------------------------------------------------

@pytest.mark.parametrize("zr", [(5, 17), (13, 40)])
def test_slabs(arvx, oracle, zr):
    """z0 no multiple of 8: the dense kernel's boxes go through global_z with an offset."""
    dims = (100, 40, 48)
    s, _, M, masks = noise_scene(dims, 5, seed=101, block=5)
    want = oracle.carve_planes(dims[0], dims[1], s, M, masks, np.arange(*zr))
    both_paths(arvx, want, dims, s, M, masks, f"slab {zr}", z_range=zr)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("dims", [(64, 96, 64), (70, 33, 40)])
def test_stripes(arvx, oracle, dims, world):
    """Striped contexts have coarse tiles of 64 x 64 x 8 voxels, 32 sub-tiles: the dense kernel's
    quarter unit is 8 sub-tiles x 8 view slots there, which no grid below 2^26 local voxels ran."""
    X, Y, Z = dims
    s, _, M, masks = noise_scene(dims, 9, seed=111, block=5)
    want = oracle.carve(X, Y, Z, s, M, masks)
    nontrivial(want, f"stripes {dims}")
    for name, flags in paths(arvx):
        got = np.zeros_like(want)
        for rank in range(world):
            what = f"stripes {dims} world={world} rank={rank} [{name}]"
            if rank >= Z // 8:  # (a rank without planes is refused)
                with pytest.raises(arvx.ArvxError):
                    arvx.Context(X, Y, Z, s, stripes=(world, rank))
                continue
            planes = arvx.stripe_planes(Z, world, rank)
            part = carve_on_path(arvx, dims, s, M, masks, flags, what, stripes=(world, rank))
            assert_same(part, want[planes], what)
            got[planes] = part
        assert_same(got, want, f"stripes {dims} world={world} [{name}]")


# ---- the exact kernel's hand-out without sharing --------------------------------------------------

def _whole_grid_views(V, W=640, H=480):
    """Ring cameras that frame the whole grid of extent E."""
    return scenes.syn.sphere_scene(32, V, W=W, H=H).M


@pytest.mark.parametrize("N,lo,hi", [(96, 0.0, 1.0), (192, 1.0, 3.0), (288, 4.0, 8.0)])
def test_unshared_hand_out(arvx, oracle, N, lo, hi):
    """The persistent exact kernel runs 16 waves per compute unit; every wave takes one item by its
    index and draws the rest from a pool.  Single-pixel noise makes every sub-tile an item: fewer
    items than waves (no pool), about two per wave (a small pool: look before draw) and about six
    (a large pool: walk), none of them shared between waves."""
    import torch
    V = 3
    s = np.float32(E / N)
    M = _whole_grid_views(V)
    masks = scenes.noise_masks(V, 480, 640, block=1, p_bg=0.3, seed=N)
    flags = arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS
    with arvx.Context(N, N, N, s) as ctx:
        ctx.set_views(M, masks)
        ctx.carve(flags)
        info = ctx.last_carve_path()
        got = ctx.download_state()
    check_path(arvx, info, flags, f"{N}^3", fresh=True)
    check_work(info["listed"], info["items"], f"{N}^3")
    waves = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    ratio = info["items"] / waves
    assert lo < ratio < hi, f"{N}^3: {info['items']} items on {waves} waves"
    want = oracle.carve(N, N, N, s, M, masks)
    nontrivial(want, f"{N}^3")
    assert_same(got, want, f"{N}^3 unshared items")


# ---- whole coarse tiles as units ------------------------------------------------------------------

def test_whole_tile_units_512x512x400(arvx, oracle):
    """The dense kernel takes whole coarse tiles (64 sub-tiles x 1 view slot per wave) only when the
    listed tiles fill its grid of 6 workgroups per compute unit: the real size.  Planes spread over
    z, with the first, the last and both sides of coarse-tile borders, against the oracle."""
    X, Y, Z, V = 512, 512, 400, 3
    s = np.float32(E / 512)
    M = _whole_grid_views(V)
    masks = scenes.noise_masks(V, 480, 640, block=3, p_bg=0.4, seed=5)
    flags = arvx.CARVE_DENSE_CLASSIFY | arvx.CARVE_WHOLE_ITEMS
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.set_views(M, masks)
        ctx.carve(flags)
        info = ctx.last_carve_path()
        ncoarse = -(-X // 64) * -(-Y // 32) * -(-Z // 32)
        if ncoarse < info["dense_grid"]:
            pytest.skip(f"the grid's {ncoarse} coarse tiles cannot fill the dense kernel's grid of "
                        f"{info['dense_grid']} workgroups on this device: no whole-tile units at this size")
        assert info["listed"] >= info["dense_grid"], f"quarter units, not whole coarse tiles: {info}"
        got = ctx.download_state()
    check_path(arvx, info, flags, "512x512x400", fresh=True, sharing=False)  # (above 2^26 voxels)
    check_work(info["listed"], info["items"], "512x512x400")
    planes = np.unique(np.concatenate([np.arange(0, Z, 13), [0, 1, 31, 32, 63, 64, 191, 192, 383, 384, Z - 2, Z - 1]]))
    assert 35 <= len(planes) <= 45
    want = oracle.carve_planes(X, Y, s, M, masks, planes)
    nontrivial(want, "512x512x400")
    assert_same(got[planes], want, "512x512x400, planes spread over z")


# ---- a short fuzz ---------------------------------------------------------------------------------

def _some_subtile_is_mixed(want):
    """Some run of 16 voxels along x, aligned to 16, holds an occupied and a carved voxel.  The run
    lies in one sub-tile (16 x 8 x 8, aligned to 16 in x whatever the slab), and a sub-tile that the
    rectangle tests settle on a fresh model is all carved or all occupied: this one has to be
    queued for the exact kernel, and its coarse tile listed."""
    occ = (want & 1).astype(bool)
    pad = -occ.shape[2] % 16
    some = np.pad(occ, ((0, 0), (0, 0), (0, pad)), constant_values=False)
    every = np.pad(occ, ((0, 0), (0, 0), (0, pad)), constant_values=True)
    shape = occ.shape[:2] + (-1, 16)
    return bool((some.reshape(shape).any(axis=3) & ~every.reshape(shape).all(axis=3)).any())


def test_fuzz_paths_against_oracle(arvx, oracle):
    """test_fuzz_against_oracle with the path bits drawn per case (at least one of them set: neither
    is what that test runs; the kernels each asks for are asserted), grids of 4..90, every third
    case a slab, 100 cases.  A draw whose oracle plane has no sub-tile with occupied and carved
    voxels is drawn again, so that every case has a non-trivial plane and has to list a coarse tile
    and queue a sub-tile."""
    rng = np.random.default_rng(2605)
    d, w = arvx.CARVE_DENSE_CLASSIFY, arvx.CARVE_WHOLE_ITEMS
    for i in range(100):
        flags = int(rng.choice([d, w, d | w]))
        while True:
            X, Y, Z = (int(rng.integers(4, 91)) for _ in range(3))
            V = int(rng.integers(1, 20))
            W, H = int(rng.integers(8, 120)), int(rng.integers(8, 90))
            zr = None
            if i % 3 == 2:
                z0 = int(rng.integers(0, Z - 1))
                zr = (z0, int(rng.integers(z0 + 1, Z + 1)))
            s = np.float32(E / max(X, Y, Z))
            _, _, M = scenes.random_cameras(V, E, seed=int(rng.integers(1 << 30)), W=W, H=H,
                                            inside=rng.random() < 0.4)
            masks = scenes.noise_masks(V, H, W, C=int(rng.choice([1, 3])),
                                       p_bg=float(rng.uniform(0.2, 0.8)),
                                       block=int(rng.choice([1, 3, 8, 32])),
                                       seed=int(rng.integers(1 << 30)))
            want = oracle.carve_planes(X, Y, s, M, masks, np.arange(*(zr or (0, Z))))
            if _some_subtile_is_mixed(want):
                break
        what = f"case {i}: {X}x{Y}x{Z} z{zr} V={V} {W}x{H} flags={flags}"
        nontrivial(want, what)
        with arvx.Context(X, Y, Z, s, z_range=zr) as ctx:
            ctx.set_views(M, masks)
            ctx.carve(flags)
            info = ctx.last_carve_path()
            got = ctx.download_state()
        assert bool(info["bits"] & arvx.PATH_DENSE_CLASSIFY) == bool(flags & d), f"{what}: {info}"
        assert bool(info["bits"] & arvx.PATH_ITEM_SHARING) == (not flags & w), f"{what}: {info}"
        assert info["bits"] & arvx.PATH_FRESH and not info["bits"] & (arvx.PATH_FUSED | arvx.PATH_BRUTE_FORCE), what
        check_work(info["listed"], info["items"], what)
        assert_same(got, want, what)
