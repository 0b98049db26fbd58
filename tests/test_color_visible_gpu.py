"""The visible colour pass on the device (arvx_color_visible) bit for bit against the numpy
restatement (tests/visibility.py) on states the oracle carved: colours, visible-view counts and
every view's depth buffer; large footprints and cameras inside the grid; tol = inf against
arvx_color; the property the pass exists for; the stages after it; its refusals; the CLI."""
import os
import subprocess

import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import np_restate as npr
from tests import scenes
from tests import visibility as vis
from tests.test_cli_gpu import CLI, YML, write_inputs
from tests.visibility import constant_images, own_side_share, view_of_colour

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 1, 3  # ARVX_ERR_* (include/arvx/arvx.h)


def run_visible(arvx, X, Y, Z, s, M, campos, images, state, mode, tol, assoc=1):
    """-> (surface index, rgb, depth, visible counts, depth buffers (V, H, W)) from the device."""
    V, H, W = images.shape[:3]
    with arvx.Context(X, Y, Z, s, assoc=assoc) as ctx:
        ctx.set_views(M, np.full((V, H, W), 255, np.uint8), campos=campos)
        ctx.set_images(images)
        ctx.upload_state(state)
        ctx.color_visible(mode, tol)
        idx, rgb = ctx.surface()
        depth = ctx.surface_depth()
        views = ctx.surface_visible()
        zb = np.stack([ctx.view_depth(v) for v in range(V)])
    return idx, rgb, depth, views, zb


def check_against_restatement(got, want, X, Y, Z, s, M, campos, state, assoc):
    idx, rgb, depth, views, zb = got
    sel = want.has
    assert np.array_equal(idx, want.index[sel]), "coloured voxels"
    assert np.array_equal(rgb, want.rgba[idx, :3]), "colours"
    assert np.array_equal(views, want.views[sel]), "visible-view counts"
    assert np.array_equal(zb.view(np.uint32), want.zbuf.view(np.uint32)), "depth buffers"
    x, y, z = idx % X, (idx // X) % Y, idx // (X * Y)
    best = np.full(len(idx), np.inf, np.float32)  # the minimum over all samples, as arvx_color
    for v in range(len(M)):
        _, inside, _ = vis.centre(M[v], s, x, y, z, zb.shape[2], zb.shape[1], assoc == 1)
        d = npr.depth(campos[v], s, x, y, z)
        best = np.where(inside & (d < best), d, best)
    assert np.array_equal(depth, best), "sample depths"


@pytest.mark.parametrize("assoc", [1, 0])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dims,V", [((32, 32, 32), 6), ((50, 50, 25), 36), ((33, 17, 9), 72),
                                    ((32, 32, 32), 72), ((33, 17, 9), 6)])
def test_parity(arvx, oracle, dims, V, mode, assoc):
    X, Y, Z = dims
    sc = syn.sphere_scene(32, V, W=160, H=120, with_images=True)
    s = np.float32(0.512 / max(dims))
    st = oracle.carve(X, Y, Z, s, sc.M, sc.masks)
    model = oracle.model_from_state(st)
    tol = np.float32(2.0) * s
    want = vis.color_visible(X, Y, Z, s, sc.M, sc.campos, sc.images, mode, model, tol, assoc == 1)
    got = run_visible(arvx, X, Y, Z, s, sc.M, sc.campos, sc.images, st, mode, tol, assoc)
    check_against_restatement(got, want, X, Y, Z, s, sc.M, sc.campos, st, assoc)
    # both branches of the vote: voxels visible somewhere, and voxels that take the fallback
    assert len(got[0]) > 0 and 0 < np.count_nonzero(got[3]) < len(got[3])


@pytest.mark.parametrize("assoc", [1, 0])
@pytest.mark.parametrize("N,seed", [(4, 0), (6, 1), (8, 2)])
def test_large_footprints_and_cameras_inside(arvx, N, seed, assoc):
    """Large voxels and cameras inside the grid: footprints span most of the image (the
    large-footprint list) and corners fall behind cameras (no splat)."""
    V, W, H = 12, 160, 120
    extent = 0.512
    s = np.float32(extent / N)
    K, Rt, M = scenes.random_cameras(V, extent, seed=seed, W=W, H=H, inside=True)
    campos = syn.campos_from_rt(Rt)
    images = syn.pattern_images(V, W, H, seed=seed + 3)
    rng = np.random.default_rng(seed)
    st = np.where(rng.random((N, N, N)) < 0.6, 3, 2).astype(np.uint8)
    model = np.zeros((N ** 3, 4), np.float32)
    model[:, 3] = (st.reshape(-1) & 1).astype(np.float32)
    large = behind = 0
    xs, ys, zs = vis.surface_voxels(N, N, N, model)
    for v in range(V):
        a2 = npr.project_raw(M[v], s, xs, ys, zs, assoc == 1)[0][2]
        ok, c0, c1, r0, r1 = vis.footprint(M[v], s, xs, ys, zs, W, H, assoc == 1)
        large += np.count_nonzero(ok & ((c1 - c0 + 1) * (r1 - r0 + 1) > 16))
        behind += np.count_nonzero((a2 > 0) & ~ok)
    assert large > 0 and behind > 0  # (the scene reaches both paths)
    for mode in (0, 1):
        for tol in (np.float32(0.0), np.float32(2.0) * s, np.float32(np.inf)):
            want = vis.color_visible(N, N, N, s, M, campos, images, mode, model, tol, assoc == 1)
            got = run_visible(arvx, N, N, N, s, M, campos, images, st, mode, tol, assoc)
            check_against_restatement(got, want, N, N, N, s, M, campos, st, assoc)


@pytest.mark.parametrize("mode", [0, 1])
def test_large_footprint_list_overflow(arvx, mode):
    """More large footprints than the first call's list has room for (64 Ki + a quarter of the
    surface list): the rest are swept by the splat's own waves.  The second call on the context
    sizes the list from the first one's count and takes the list path for all of them; both are
    bit-exact."""
    N, V, W, H, seed = 24, 36, 160, 120, 4
    s = np.float32(0.512 / N)
    K, Rt, M = scenes.random_cameras(V, 0.512, seed=seed, W=W, H=H, inside=True)
    campos = syn.campos_from_rt(Rt)
    images = syn.pattern_images(V, W, H, seed=seed)
    rng = np.random.default_rng(seed)
    st = np.where(rng.random((N, N, N)) < 0.6, 3, 2).astype(np.uint8)
    model = np.zeros((N ** 3, 4), np.float32)
    model[:, 3] = (st.reshape(-1) & 1).astype(np.float32)
    xs, ys, zs = vis.surface_voxels(N, N, N, model)
    large = 0
    for v in range(V):
        ok, c0, c1, r0, r1 = vis.footprint(M[v], s, xs, ys, zs, W, H)
        large += np.count_nonzero(ok & ((c1 - c0 + 1) * (r1 - r0 + 1) > 16))
    assert large > (1 << 16) + (5 * N ** 3) // 16  # (beyond the first list for any capacity)
    tol = np.float32(2.0) * s
    want = vis.color_visible(N, N, N, s, M, campos, images, mode, model, tol)
    with arvx.Context(N, N, N, s) as ctx:
        ctx.set_views(M, np.full((V, H, W), 255, np.uint8), campos=campos)
        ctx.set_images(images)
        ctx.upload_state(st)
        for _ in range(2):
            ctx.color_visible(mode, tol)
            idx, rgb = ctx.surface()
            got = idx, rgb, ctx.surface_depth(), ctx.surface_visible(), \
                np.stack([ctx.view_depth(v) for v in range(V)])
            check_against_restatement(got, want, N, N, N, s, M, campos, st, 1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N,V", [(32, 6), (64, 36)])
def test_infinite_tolerance_is_arvx_color(arvx, oracle, N, V, mode):
    sc = syn.sphere_scene(N, V, W=320, H=240, with_images=True)
    st = oracle.carve(N, N, N, sc.voxel_size, sc.M, sc.masks)
    with arvx.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.upload_state(st)
        ctx.color(mode)
        plain = ctx.surface(), ctx.surface_depth(), ctx.export_model(True)
        ctx.color_visible(mode, np.inf)
        got = ctx.surface(), ctx.surface_depth(), ctx.export_model(True)
        views = ctx.surface_visible()
    assert np.array_equal(got[0][0], plain[0][0]) and np.array_equal(got[0][1], plain[0][1])
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])
    assert np.all(views > 0)


def _sphere(arvx, oracle, N, V, mode, tol_voxels, W=320, H=240):
    sc = syn.sphere_scene(N, V, W=W, H=H)
    images = constant_images(V, W, H)
    st = oracle.carve(N, N, N, sc.voxel_size, sc.M, sc.masks)
    with arvx.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(images)
        ctx.upload_state(st)
        ctx.color(mode)
        plain = ctx.surface()
        ctx.color_visible(mode, np.float32(tol_voxels) * sc.voxel_size)
        idx, rgb = ctx.surface()
        views = ctx.surface_visible()
    assert np.array_equal(idx, plain[0])
    return sc, idx, rgb, views, plain[1]


def test_closest_colour_comes_from_the_voxels_own_side(arvx, oracle):
    """One constant colour per view, so a closest-mode colour names its view: the chosen camera
    is on the voxel's side of the sphere, (c - p) . (p - centre) > 0, for >= 99 % of the voxels
    that are visible somewhere.  The plain pass reaches far less (about 44 %: DESIGN.md)."""
    sc, idx, rgb, views, plain_rgb = _sphere(arvx, oracle, 64, 36, 0, 3.0)
    sel = views > 0
    assert sel.mean() > 0.7
    share = own_side_share(sc, idx[sel], view_of_colour(rgb[sel], sc.V))
    plain = own_side_share(sc, idx[sel], view_of_colour(plain_rgb[sel], sc.V))
    assert share >= 0.99, share
    assert plain < 0.6, plain


def test_average_colour_is_the_facing_views(arvx, oracle):
    """Average mode, with the views' R and G turning once around a circle with the ring's azimuth
    (view_colours): a voxel on the sphere's side carries the mean of the views that face it, so its
    (R, G) - 128 points along its normal's azimuth and is far from (128, 128), the all-view mean --
    which is what the plain pass gives it."""
    sc, idx, rgb, views, plain_rgb = _sphere(arvx, oracle, 64, 36, 1, 3.0)
    sel = views > 0
    p = vis.world_points(sc.voxel_size, idx[sel], sc.X, sc.Y)
    ctr = np.array([syn.EXTENT / 2, syn.EXTENT / 2, -syn.EXTENT / 2])
    nrm = (p - ctr) / np.linalg.norm(p - ctr, axis=1)[:, None]
    side = np.abs(nrm[:, 2]) < 0.5  # (voxels facing up see every camera of the ring)
    assert side.sum() > 1000
    rg, prg = rgb[sel][side, :2] - 128, plain_rgb[sel][side, :2] - 128
    phi = np.arctan2(nrm[side, 1], nrm[side, 0])
    off = np.abs((np.arctan2(rg[:, 1], rg[:, 0]) - phi + np.pi) % (2 * np.pi) - np.pi)
    assert np.mean((off < np.deg2rad(30)) & (np.linalg.norm(rg, axis=1) > 40)) >= 0.99
    assert np.mean(np.linalg.norm(prg, axis=1) > 40) < 0.05


def test_downstream_stages_take_the_visible_colours(arvx, oracle):
    N, V = 40, 12
    sc = syn.sphere_scene(N, V, W=160, H=120, with_images=True)
    s = sc.voxel_size
    st = oracle.carve(N, N, N, s, sc.M, sc.masks)
    tol = np.float32(3.0) * s
    coloured = vis.color_visible(N, N, N, s, sc.M, sc.campos, sc.images, 1, oracle.model_from_state(st),
                                 tol).rgba
    unseen = oracle.handle_unseen(st, coloured)
    closed = oracle.closure(N, N, N, unseen)
    verts, frgb = oracle.mc_mesh(N, N, N, closed)
    with arvx.Context(N, N, N, s) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.carve()
        ctx.color_visible(arvx.COLOR_AVERAGE, tol)
        assert np.array_equal(ctx.export_model(False), coloured)
        assert np.array_equal(ctx.export_model(True), unseen)
        ctx.handle_unseen()
        ctx.closure(3, True)
        assert np.array_equal(ctx.export_model(True), closed)
        gv, grgb = ctx.mc_mesh(True)
    assert np.array_equal(gv, verts) and np.array_equal(grgb, frgb)


def test_pipeline_256(arvx, oracle):
    """carve -> visible colour -> handleUnseen -> closure -> mesh at 256^3, 8 views of 640x480."""
    N, V = 256, 8
    sc = syn.sphere_scene(N, V, with_images=True)
    s = sc.voxel_size
    st = oracle.carve(N, N, N, s, sc.M, sc.masks)
    tol = np.float32(3.0) * s
    want = vis.color_visible(N, N, N, s, sc.M, sc.campos, sc.images, 0, oracle.model_from_state(st), tol)
    unseen = oracle.handle_unseen(st, want.rgba)
    closed = oracle.closure(N, N, N, unseen)
    with arvx.Context(N, N, N, s) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.carve()
        ctx.color_visible(arvx.COLOR_CLOSEST, tol)
        idx, _ = ctx.surface()
        views = ctx.surface_visible()
        zb = np.stack([ctx.view_depth(v) for v in range(V)])
        ctx.handle_unseen()
        ctx.closure(3, True, download=False)
        got = ctx.export_model(True)
        gv, grgb = ctx.mc_mesh(True)
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert len(idx) > 50000
    assert np.array_equal(views, want.views[want.has])
    assert np.array_equal(zb.view(np.uint32), want.zbuf.view(np.uint32))
    assert np.array_equal(got, closed)
    verts, frgb = oracle.mc_mesh(N, N, N, closed)
    assert np.array_equal(gv, verts) and np.array_equal(grgb, frgb)


def _err(arvx, fn, code):
    with pytest.raises(arvx.ArvxError) as e:
        fn()
    assert e.value.code == code, str(e.value)


def test_refusals(arvx, oracle):
    N, V = 16, 4
    sc = syn.sphere_scene(N, V, W=64, H=48, with_images=True)
    st = oracle.carve(N, N, N, sc.voxel_size, sc.M, sc.masks)
    lib = arvx.load_library()
    with arvx.Context(N, N, N, sc.voxel_size) as ctx:
        _err(arvx, lambda: ctx.color_visible(0, 1.0), ERR_STATE)  # no views yet
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        _err(arvx, lambda: ctx.color_visible(0, 1.0), ERR_STATE)  # no images yet
        ctx.set_images(sc.images)
        ctx.carve()
        _err(arvx, lambda: ctx.surface_visible(), ERR_STATE)  # before the call
        _err(arvx, lambda: ctx.view_depth(0), ERR_STATE)
        ctx.color(0)
        _err(arvx, lambda: ctx.surface_visible(), ERR_STATE)  # after a plain arvx_color
        _err(arvx, lambda: ctx.view_depth(0), ERR_STATE)
        for mode, tol in ((2, 1.0), (-1, 1.0), (0, float("nan")), (1, -1.0), (0, -np.inf)):
            _err(arvx, lambda: ctx.color_visible(mode, tol), ERR_INVALID)
        # a refused call leaves the plain colour list as it was
        assert ctx.surface()[0].size > 0
        ctx.color_visible(0, np.inf)
        assert ctx.surface_visible().size == ctx.surface()[0].size
        for v in (-1, V):
            _err(arvx, lambda: ctx.view_depth(v), ERR_INVALID)
        assert np.isfinite(ctx.view_depth(V - 1)).any()
        # the lifetimes: set_views, set_images and a carve drop the result
        for drop in (lambda: ctx.set_views(sc.M, sc.masks, campos=sc.campos),
                     lambda: ctx.set_images(sc.images), lambda: ctx.carve()):
            ctx.set_images(sc.images)  # (set_views takes the images with it)
            ctx.color_visible(1, 0.0)
            ctx.view_depth(0)
            drop()
            _err(arvx, lambda: ctx.view_depth(0), ERR_STATE)
            _err(arvx, lambda: ctx.surface_visible(), ERR_STATE)
        # handleUnseen keeps the colour list and with it the result
        ctx.color_visible(1, 0.0)
        ctx.handle_unseen()
        assert ctx.surface_visible().size > 0
        assert lib.arvx_surface_visible_download(ctx._h, None) == ERR_INVALID
    # slab and striped contexts
    with arvx.Context(N, N, N, sc.voxel_size, z_range=(4, 12)) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.upload_state(st[4:12])
        _err(arvx, lambda: ctx.color_visible(0, 1.0), ERR_STATE)
        ctx.color(0)  # (the plain pass runs there)
    with arvx.Context(N, N, N, sc.voxel_size, stripes=(2, 0)) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        _err(arvx, lambda: ctx.color_visible(0, 1.0), ERR_STATE)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from ar_voxel_project_amd import build
        build.build_host_tests()
    return CLI


@pytest.mark.parametrize("color", [2, 1])
def test_cli_visible(cli, oracle, tmp_path, color):
    X, Y, Z = 40, 36, 20
    s = np.float32(0.512 / 40)
    sc = scenes.syn.sphere_scene(64, 5, with_images=True)
    d = str(tmp_path)
    write_inputs(d, sc)
    out = os.path.join(d, "mesh.off")
    cmd = [cli, "-c=5", f"-images={d}/images", f"-masks={d}/masks", f"-poses={d}/poses.txt",
           f"-calibration={YML}", f"-x={X}", f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}",
           "-carve=1", f"-color={color}", "-postprocessing=true", "-visible=true",
           "-scale=2.0", "-dx=0.5", f"-outFile={out}"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "LOG - CR: color reconstruction finished." in r.stdout
    M = oracle.compose(sc.K, sc.Rt)
    st = oracle.carve(X, Y, Z, s, M, sc.masks)
    tol = np.float32(3.0) * s  # (the default -visibleTol)
    model = vis.color_visible(X, Y, Z, s, M, sc.campos, sc.images, color - 1, oracle.model_from_state(st),
                              tol).rgba
    model = oracle.closure(X, Y, Z, oracle.handle_unseen(st, model))
    verts, rgb = oracle.mc_mesh(X, Y, Z, model)
    want = oracle.off_text(verts, rgb, np.float32(2.0) * s, (0.5, 0.0, 0.0))
    assert open(out, "rb").read() == want.encode()
    # and the tolerance flag reaches the pass: -visibleTol=0 changes the mesh's colours
    r = subprocess.run(cmd[:-1] + ["-visibleTol=0", f"-outFile={out}0"], capture_output=True, text=True,
                       cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    model0 = vis.color_visible(X, Y, Z, s, M, sc.campos, sc.images, color - 1, oracle.model_from_state(st),
                               0.0).rgba
    model0 = oracle.closure(X, Y, Z, oracle.handle_unseen(st, model0))
    verts0, rgb0 = oracle.mc_mesh(X, Y, Z, model0)
    assert open(out + "0", "rb").read() == oracle.off_text(verts0, rgb0, np.float32(2.0) * s,
                                                            (0.5, 0.0, 0.0)).encode()
