"""The vote carve on the device (arvx_carve_votes) bit for bit against the numpy restatement
(tests/vote_carve.py): state and both counts for several tolerances, in both groupings, on damaged
sphere masks, on grids that reach past the images and on block-noise masks; the four flag
combinations; max_misses = 0 against the plain carve; the lazy state a fresh carve leaves; the stages
and carves after it; its refusals; the CLI.

(One refusal of arvx.h cannot be reached from outside: more than 65535 views -- arvx_set_views takes
at most 4096.)"""
import os
import subprocess

import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import scenes
from tests import vote_carve as vc
from tests.test_cli_gpu import CLI, YML, write_inputs

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 1, 3  # ARVX_ERR_* (include/arvx/arvx.h)


def sphere(dims, V, patches=vc.PATCHES, s=None):
    sc = syn.sphere_scene(32, V, W=160, H=120)
    return sc.M, vc.damage(sc.masks, patches), np.float32(0.512 / max(dims)) if s is None else np.float32(s)


def noise(X, Y, Z, V=6, W=320, H=240):
    _, _, M = scenes.random_cameras(V, 0.3, seed=X + Z, W=W, H=H)
    return M, scenes.noise_masks(V, H, W, block=24, p_bg=0.45, seed=X), np.float32(0.3 / 128)


def check_parity(arvx, oracle, dims, M, masks, s, assoc, Ks, votes=None):
    X, Y, Z = dims
    if votes is None:
        votes = vc.counts(oracle, X, Y, Z, s, M, masks, assoc == 1)
    fresh = oracle.fresh_state(X, Y, Z)
    with arvx.Context(X, Y, Z, s, assoc=assoc) as ctx:
        ctx.set_views(M, masks)
        for K in Ks:
            ctx.reset()
            ctx.carve_votes(K, counts=True)
            bg, inside = ctx.votes()
            assert np.array_equal(bg, votes.background), K
            assert np.array_equal(inside, votes.inside), K
            assert np.array_equal(ctx.download_state().reshape(-1), vc.apply(votes, fresh, K)), K
            ctx.reset()
            ctx.carve_votes(K)  # (the early exits)
            assert np.array_equal(ctx.download_state().reshape(-1), vc.apply(votes, fresh, K)), K
    return votes


@pytest.mark.parametrize("assoc", [1, 0])
@pytest.mark.parametrize("dims,V,patches", [((32, 32, 32), 6, vc.PATCHES), ((33, 17, 9), 12, vc.PATCHES_SMALL),
                                            ((50, 50, 25), 72, vc.PATCHES), ((32, 32, 32), 130, vc.PATCHES)])
def test_parity_sphere(arvx, oracle, dims, V, patches, assoc):
    """Partial tiles (33 x 17 x 9), two chunks of views (72) and three (130)."""
    M, masks, s = sphere(dims, V, patches)
    votes = check_parity(arvx, oracle, dims, M, masks, s, assoc, (0, 1, 3, V))
    fresh = oracle.fresh_state(*dims)
    k0, k1 = vc.apply(votes, fresh, 0), vc.apply(votes, fresh, 1)
    assert ((k1 & 1) > (k0 & 1)).any()  # the damage shows: one tolerated miss keeps voxels the carve loses
    assert 0 < (k0 & 1).sum() and votes.background.max() > 3


@pytest.mark.parametrize("assoc", [1, 0])
def test_parity_grid_past_the_images(arvx, oracle, assoc):
    """Voxel size 0.025 at 32^3: the grid reaches past what the cameras see -- voxels
    inside no image, and sub-tiles that are partly inside one."""
    dims, V = (32, 32, 32), 6
    M, masks, s = sphere(dims, V, s=0.025)
    votes = check_parity(arvx, oracle, dims, M, masks, s, assoc, (0, 1, 3, V))
    assert (votes.inside == 0).any() and (votes.inside == V).any()
    tiles = votes.inside.reshape(4, 8, 4, 8, 2, 16)
    assert (tiles.min(axis=(1, 3, 5)) < tiles.max(axis=(1, 3, 5))).any()


@pytest.mark.parametrize("assoc", [1, 0])
def test_parity_block_noise(arvx, oracle, assoc):
    """128 x 96 x 64, random cameras, block-noise masks: sub-tiles of all four rectangle answers."""
    dims = (128, 96, 64)
    M, masks, s = noise(*dims)
    answers = vc.subtile_answers(oracle, *dims, s, M, masks, assoc == 1)
    assert min(answers) > 0, answers  # (outside, background, foreground, mixed)
    check_parity(arvx, oracle, dims, M, masks, s, assoc, (0, 1, 3, len(masks)))


@pytest.mark.parametrize("dims,V,patches,K", [((32, 32, 32), 6, vc.PATCHES, 1), ((33, 17, 9), 12, vc.PATCHES_SMALL, 2),
                                              ((128, 96, 64), 0, None, 1)])
def test_flag_combinations(arvx, oracle, dims, V, patches, K):
    """Cull against no cull, counts against no counts: one state; the counts do not depend on the cull."""
    M, masks, s = sphere(dims, V, patches) if V else noise(*dims)
    got = {}
    with arvx.Context(*dims, s) as ctx:
        ctx.set_views(M, masks)
        for counts in (False, True):
            for cull in (True, False):
                ctx.reset()
                ctx.carve_votes(K, counts=counts, cull=cull)
                got[counts, cull] = (ctx.download_state(), ctx.votes() if counts else None)
    want, votes = vc.carve_votes(oracle, *dims, s, M, masks, K)
    for key, (st, v) in got.items():
        assert np.array_equal(st.reshape(-1), want), key
        if v is not None:
            assert np.array_equal(v[0], votes.background) and np.array_equal(v[1], votes.inside), key


@pytest.mark.parametrize("dims,V,patches", [((32, 32, 32), 6, vc.PATCHES), ((50, 50, 25), 72, vc.PATCHES),
                                            ((128, 96, 64), 0, None)])
def test_zero_misses_is_the_carve(arvx, oracle, dims, V, patches):
    M, masks, s = sphere(dims, V, patches) if V else noise(*dims)
    half = oracle.carve(*dims, s, M[:3], masks[:3])
    assert 0 < (half & 1).mean() < 1
    with arvx.Context(*dims, s) as a, arvx.Context(*dims, s) as b:
        a.set_views(M, masks)
        b.set_views(M, masks)
        a.carve()
        b.carve_votes(0)
        assert np.array_equal(a.download_state(), b.download_state())
        a.upload_state(half)
        b.upload_state(half)
        a.carve()
        b.carve_votes(0)
        assert np.array_equal(a.download_state(), b.download_state())


def test_lazy_state(arvx, oracle):
    """The state a default carve_views(0, 3) of a fresh 128 x 96 x 64 model leaves -- coarse tiles that
    exist only as their code (tests/test_photo_carve_gpu.py::test_lazy_state) -- and the same state
    uploaded give the same result: the restatement's."""
    dims = (128, 96, 64)
    M, masks, s = noise(*dims)
    with arvx.Context(*dims, s) as ctx:
        ctx.set_views(M, masks)
        ctx.carve_views(0, 3)
        ctx.carve_votes(1, counts=True)
        lazy, votes_lazy = ctx.download_state(), ctx.votes()
        ctx.reset()
        ctx.carve_views(0, 3)
        st = ctx.download_state()
        ctx.upload_state(st)
        ctx.carve_votes(1, counts=True)
        uploaded, votes_up = ctx.download_state(), ctx.votes()
    assert 0 < (st & 1).mean() < 0.9
    want, votes = vc.carve_votes(oracle, *dims, s, M, masks, 1, state=st)
    assert ((want & 1) < (st.reshape(-1) & 1)).any()  # (the call has something left to empty)
    assert np.array_equal(lazy.reshape(-1), want) and np.array_equal(uploaded, lazy)
    for v in (votes_lazy, votes_up):
        assert np.array_equal(v[0], votes.background) and np.array_equal(v[1], votes.inside)


def _after(ctx):
    out = [ctx.download_state()]
    ctx.color(1)
    out += list(ctx.surface())
    ctx.handle_unseen()
    out.append(ctx.download_state())
    r = ctx.closure(3, True)
    out += [np.asarray(a) for a in (r if isinstance(r, tuple) else (r,))]
    out.append(ctx.download_state())
    out += [np.asarray(a) for a in ctx.mc_mesh_welded(True, True)]
    return out


def test_stages_after(arvx, oracle):
    dims, V = (50, 50, 25), 36
    sc = syn.sphere_scene(32, V, W=160, H=120, with_images=True)
    masks, s = vc.damage(sc.masks), np.float32(0.512 / 50)
    want, _ = vc.carve_votes(oracle, *dims, s, sc.M, masks, 2)
    with arvx.Context(*dims, s) as ctx:
        ctx.set_views(sc.M, masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.carve_votes(2)
        got = _after(ctx)
    with arvx.Context(*dims, s) as ctx:
        ctx.set_views(sc.M, masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.upload_state(want)
        ref = _after(ctx)
    assert len(got) == len(ref) and len(got[1]) > 0
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dims,V", [((50, 50, 25), 36), ((128, 96, 64), 0)])
def test_carves_after(arvx, oracle, dims, V):
    """carve_votes(1), then two plain views: the context is a correct input of the carve again -- and
    what those carves settle for whole coarse tiles is still right after another vote carve."""
    M, masks, s = sphere(dims, V) if V else noise(*dims)
    want, _ = vc.carve_votes(oracle, *dims, s, M, masks, 1)
    with arvx.Context(*dims, s) as ctx:
        ctx.set_views(M, masks)
        ctx.carve_votes(1)
        assert np.array_equal(ctx.download_state().reshape(-1), want)
        ctx.carve_views(0, 2)
        got = ctx.download_state()
        ctx.carve_votes(len(masks))  # (changes nothing: every voxel the views see is seen already)
        assert np.array_equal(ctx.download_state(), got)
        ctx.carve()
        full = ctx.download_state()
    st = want
    for v in range(2):
        st = oracle.carve_view(*dims, s, M[v], masks[v], st)
    assert np.array_equal(got, st)
    assert np.array_equal(full, oracle.carve(*dims, s, M, masks, state=st))


def _err(arvx, fn, code):
    with pytest.raises(arvx.ArvxError) as e:
        fn()
    assert e.value.code == code, str(e.value)


def test_refusals(arvx, oracle):
    import ctypes as C
    N, V = 16, 4
    sc = syn.sphere_scene(N, V, W=64, H=48)
    st = oracle.carve(N, N, N, sc.voxel_size, sc.M[:2], sc.masks[:2])
    with arvx.Context(N, N, N, sc.voxel_size) as ctx:
        lib = ctx._lib
        _err(arvx, lambda: ctx.carve_votes(1), ERR_STATE)  # no views
        _err(arvx, ctx.votes, ERR_STATE)  # no counts
        Ms = np.ascontiguousarray(sc.M, np.float32)
        f32p = C.POINTER(C.c_float)
        assert lib.arvx_set_views(ctx._h, V, Ms.ctypes.data_as(f32p), None, None, 64, 48, 1, 64) == 0
        _err(arvx, lambda: ctx.carve_votes(1), ERR_STATE)  # views set with masks == NULL
        ctx.set_views(sc.M, sc.masks)
        ctx.upload_state(st)
        for K in (-1, 65536):
            _err(arvx, lambda: ctx.carve_votes(K), ERR_INVALID)
        for flags in (4, 1 | 8, 0x80000000):
            assert lib.arvx_carve_votes(ctx._h, 1, flags) == ERR_INVALID
        _err(arvx, ctx.votes, ERR_STATE)
        assert np.array_equal(ctx.download_state(), st)  # (refused: nothing changed)
        ctx.carve_votes(65535, counts=True)  # (the largest tolerance: only seen bits)
        bg, inside = ctx.votes()
        assert np.array_equal(ctx.download_state().reshape(-1) & 1, st.reshape(-1) & 1)
        assert lib.arvx_votes_download(ctx._h, None, None) == 0  # (either pointer may be null)
        _err(arvx, lambda: ctx.carve_votes(-1), ERR_INVALID)
        assert np.array_equal(ctx.votes()[0], bg)  # (a refused call keeps the counts)
        # the counts live until the state or the views are replaced
        ctx.carve()
        _err(arvx, ctx.votes, ERR_STATE)
        ctx.carve_votes(1, counts=True)
        ctx.carve_votes(1)
        _err(arvx, ctx.votes, ERR_STATE)
        ctx.carve_votes(1, counts=True)
        ctx.set_views(sc.M, sc.masks)
        _err(arvx, ctx.votes, ERR_STATE)
    with arvx.Context(N, N, N, sc.voxel_size, z_range=(4, 12)) as ctx:
        ctx.set_views(sc.M, sc.masks)
        ctx.upload_state(st[4:12])
        _err(arvx, lambda: ctx.carve_votes(1), ERR_STATE)
        assert np.array_equal(ctx.download_state(), st[4:12])
    with arvx.Context(N, N, N, sc.voxel_size, stripes=(2, 0)) as ctx:
        ctx.set_views(sc.M, sc.masks)
        _err(arvx, lambda: ctx.carve_votes(1), ERR_STATE)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        from ar_voxel_project_amd import build
        build.build_host_tests()
    return CLI


def test_cli_misses(cli, oracle, tmp_path):
    X, Y, Z = 40, 36, 20
    s = np.float32(0.512 / 40)
    sc = syn.sphere_scene(64, 5, with_images=True)  # (the calibration file's images: 640 x 480)
    sc.masks = vc.damage(sc.masks, ((1, slice(200, 248), slice(280, 328)), (4, slice(240, 288), slice(340, 388))))
    d = str(tmp_path)
    write_inputs(d, sc)
    out = os.path.join(d, "mesh.off")
    cmd = [cli, "-c=5", f"-images={d}/images", f"-masks={d}/masks", f"-poses={d}/poses.txt",
           f"-calibration={YML}", f"-x={X}", f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}",
           "-carve=1", "-color=2", "-postprocessing=true", "-misses=1", "-scale=2.0", "-dx=0.5",
           f"-outFile={out}"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "LOG - VC: starting carving process (version 1, up to 1 misses)." in r.stdout
    M = oracle.compose(sc.K, sc.Rt)
    st, votes = vc.carve_votes(oracle, X, Y, Z, s, M, sc.masks, 1)
    assert (st & 1).sum() > (vc.apply(votes, oracle.fresh_state(X, Y, Z), 0) & 1).sum()  # (-misses matters)
    st = st.reshape(Z, Y, X)
    model = oracle.color(X, Y, Z, s, M, sc.campos, sc.images, 1, oracle.model_from_state(st))
    model = oracle.closure(X, Y, Z, oracle.handle_unseen(st, model))
    verts, rgb = oracle.mc_mesh(X, Y, Z, model)
    want = oracle.off_text(verts, rgb, np.float32(2.0) * s, (0.5, 0.0, 0.0))
    assert open(out, "rb").read() == want.encode()
