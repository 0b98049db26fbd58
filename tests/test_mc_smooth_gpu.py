"""arvx_mc_mesh_smooth on the device, every layer: the C-ABI through capi.Context.mc_mesh_smooth,
the C++ marchingCubesSmoothed through tools/cpp/arvx_cli -smooth.

The smoothed positions and the vertex normals must be, bit for bit, the numpy restatement of the
definition (tests/mesh_smooth.py) applied to the device's own welded mesh."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_smooth as ms
from tests import mesh_weld as mw
from tests import scenes
from tests.test_cli_gpu import cli, expected  # noqa: F401
from tests.test_cpp_host import write_scene
from tests.test_mc_off import off1, random_coloured_model, state_of  # noqa: F401
from tests.test_mc_weld_cpu import parse_off

pytestmark = pytest.mark.gpu

# (iterations, lambda, mu): the default factors, mu = 0 (Laplacian), other factors; one after
# the other on the same welded mesh, so that every call after the first reuses the cached CSRs
PARAMS = [(0, 0.5, -0.53), (1, 0.5, -0.53), (10, 0.5, -0.53), (1, 0.5, 0.0), (10, 0.5, 0.0),
          (2, 0.33, -0.34), (1, 0.5, -0.53)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def welded_download(ctx, nv, nt):
    """arvx_mc_mesh_welded_download of the mesh the context holds, without building it again."""
    verts = np.empty((nv, 3), np.float32)
    records = np.empty((nt, 6), np.uint32)
    ctx._ck(ctx._lib.arvx_mc_mesh_welded_download(ctx._h, verts.ctypes.data, records.ctypes.data, None))
    return verts, records[:, :3]


def check_smooth(ctx, apply_unseen=False, params=PARAMS):
    """Every parameter set against the restatement on the device's welded mesh; the welded
    download keeps the lattice positions.  Returns (V, T)."""
    wv, faces, _ = ctx.mc_mesh_welded(apply_unseen)
    for it, lam, mu in params:
        q, n = ctx.mc_mesh_smooth(it, lam, mu)
        wq, wn = ms.smooth(wv, faces, it, lam, mu)
        assert q.shape == wv.shape and n.shape == wv.shape
        assert np.array_equal(bits(q), bits(wq)), (it, lam, mu)
        assert np.array_equal(bits(n), bits(wn)), (it, lam, mu)
        # either array alone
        q1, n1 = ctx.mc_mesh_smooth_download(verts=True, normals=False)
        q2, n2 = ctx.mc_mesh_smooth_download(verts=False, normals=True)
        assert n1 is None and q2 is None
        assert np.array_equal(bits(q1), bits(q)) and np.array_equal(bits(n2), bits(n))
    lv, lf = welded_download(ctx, len(wv), len(faces))
    assert np.array_equal(lv, wv) and np.array_equal(lf, faces)
    assert np.array_equal(lv, np.floor(lv))  # (lattice points)
    return len(wv), len(faces)


def test_smoothed_mesh_of_1_off(arvx, off1):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    with arvx.Context(X, Y, Z, off1["s"]) as ctx:
        ctx.upload_state(state_of(off1["occ"]))
        nv, nt = check_smooth(ctx)
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert (nv, nt) == (5704, off1["nf"])


def test_smoothed_mesh_random_fills(arvx):
    """30 / 50 / 70 % random fills (vertices with no neighbour, faces (i, i, i), high degrees),
    models that touch the grid's faces, rows that end inside a 64-bit word."""
    rng = np.random.default_rng(59)
    for dims, fill in [((12, 9, 7), 0.3), ((70, 33, 20), 0.5), ((130, 5, 9), 0.7), ((64, 64, 8), 0.3),
                       ((100, 80, 40), 0.5)]:
        X, Y, Z = dims
        occ = rng.random(X * Y * Z) < fill
        with arvx.Context(X, Y, Z, 0.01) as ctx:
            ctx.upload_state((occ * 1 | 2).astype(np.uint8))
            check_smooth(ctx)


def test_smoothed_mesh_colour_and_unseen(arvx):
    """A coloured model with UNSEEN paint: apply_unseen changes the mesh, and the smoothing follows
    the welded mesh of the last call."""
    rng = np.random.default_rng(61)
    X, Y, Z = 40, 30, 20
    rgba = random_coloured_model(rng, X, Y, Z, False)
    occ = rgba[:, 3] != 0
    seen = rng.random(len(rgba)) < 0.8
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state((occ * 1 | seen * 2).astype(np.uint8))
        check_smooth(ctx, False, PARAMS[:3])
        ctx.handle_unseen()
        check_smooth(ctx, True, PARAMS[:3])


@pytest.mark.parametrize("dims,voxel", [((1, 1, 1), (0, 0, 0)), ((5, 6, 7), (2, 3, 4)),
                                        ((65, 3, 2), (64, 2, 1))])
def test_smoothed_mesh_single_voxel(arvx, dims, voxel):
    """One vertex, every face (i, i, i): no neighbours, the position unchanged, normal 0."""
    X, Y, Z = dims
    state = np.full((Z, Y, X), 2, np.uint8)
    state[voxel[2], voxel[1], voxel[0]] = 3
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state(state.reshape(-1))
        assert check_smooth(ctx)[0] == 1
        q, n = ctx.mc_mesh_smooth(5)
    assert np.array_equal(q, np.float32([voxel])) and np.array_equal(n, np.zeros((1, 3), np.float32))


def test_smoothed_mesh_empty_model(arvx):
    with arvx.Context(20, 10, 5, 0.01) as ctx:
        ctx.upload_state(np.full(20 * 10 * 5, 2, np.uint8))
        assert ctx.mc_mesh_welded_count() == (0, 0)
        q, n = ctx.mc_mesh_smooth(3)
    assert q.shape == (0, 3) and n.shape == (0, 3)


N = 256


@pytest.fixture(scope="module")
def scene():
    return scenes.syn.sphere_scene(N, 8, with_images=True)


def test_smoothed_mesh_pipeline_256(arvx, scene):
    """carve, colour, handleUnseen, closure at 256^3: closure fills among the vertices."""
    sc = scene
    with arvx.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.carve()
        ctx.color(arvx.COLOR_AVERAGE)
        ctx.handle_unseen()
        ctx.closure(3, True, download=False)
        nv, nt = check_smooth(ctx, True, [(0, 0.5, -0.53), (1, 0.5, -0.53), (10, 0.5, -0.53), (10, 0.5, 0.0)])
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert nv > 50000 and nt > nv


def test_state_and_argument_errors(arvx):
    rng = np.random.default_rng(67)
    with arvx.Context(16, 16, 16, 0.01) as ctx:
        ctx.upload_state(((rng.random(16 ** 3) < 0.5) * 1 | 2).astype(np.uint8))
        with pytest.raises(arvx.ArvxError) as e:  # no welded mesh
            ctx.mc_mesh_smooth(1)
        assert e.value.code == 3
        ctx.mc_mesh_welded()
        with pytest.raises(arvx.ArvxError) as e:  # download before smooth
            ctx.mc_mesh_smooth_download()
        assert e.value.code == 3
        for args in [(-1, 0.5, -0.53), (1, float("nan"), -0.53), (1, 0.5, float("inf"))]:
            with pytest.raises(arvx.ArvxError) as e:
                ctx.mc_mesh_smooth(*args)
            assert e.value.code == 1, args
        ctx.mc_mesh_smooth(1)
        ctx.mc_mesh_smooth_download()
        ctx.mc_mesh_welded()  # a new welded mesh: the smoothed one is gone
        with pytest.raises(arvx.ArvxError) as e:
            ctx.mc_mesh_smooth_download()
        assert e.value.code == 3
        # through the C-ABI: null context, both download pointers null
        assert ctx._lib.arvx_mc_mesh_smooth(None, 1, C.c_float(0.5), C.c_float(-0.53)) != 0
        ctx.mc_mesh_smooth(1, download=False)
        assert ctx._lib.arvx_mc_mesh_smooth_download(ctx._h, None, None) == 0


def test_slab_and_striped_contexts_are_refused(arvx):
    for kw in (dict(z_range=(0, 16)), dict(z_range=(16, 32)), dict(stripes=(2, 0))):
        with arvx.Context(16, 16, 32, 0.01, **kw) as ctx:
            with pytest.raises(arvx.ArvxError) as e:
                ctx.mc_mesh_smooth(1)
            assert e.value.code == 3


def test_cli_smooth_flag(cli, oracle, tmp_path):  # noqa: F811
    """arvx_cli -c=5 -smooth=3 writes the welded mesh of the run with its vertices smoothed on the
    device, through the writer's scale and translation; without -smooth the run writes the
    reference's bytes."""
    X, Y, Z = 40, 36, 20
    s = np.float32(0.512 / 40)
    scale, dx = 1.5, 0.25
    sc = scenes.syn.sphere_scene(64, 5, W=160, H=120, with_images=True)
    d = str(tmp_path)
    scene = os.path.join(d, "scene.bin")
    write_scene(scene, 1, 1, 1, 1.0, sc.K, sc.Rt, sc.masks, sc.images, np.ones(1, np.uint8))
    outs = {}
    for flag in ([], ["-smooth=3"]):
        out = os.path.join(d, f"m{len(flag)}.off")
        r = subprocess.run([cli, "-c=5", f"-scene={scene}", "-calibration=none.yml", f"-x={X}",
                            f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}", "-color=2", f"-scale={scale}",
                            f"-dx={dx}", f"-outFile={out}"] + flag, capture_output=True, text=True, cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "LOG - MC: Mesh written, marchingCubes completed." in r.stdout
        outs[bool(flag)] = out
    model = expected(oracle, sc, X, Y, Z, s, 1, 2, True)
    verts, rgb = oracle.mc_mesh(X, Y, Z, model)
    factor = np.float32(scale) * s
    assert open(outs[False], "rb").read() == oracle.off_text(verts, rgb, factor, (dx, 0.0, 0.0)).encode()
    wv, wf, wrgb = mw.weld(verts, rgb)
    q = ms.taubin(wv, wf, 3)
    v1, f1, rgb1 = parse_off(outs[True])
    assert np.array_equal(f1, wf) and np.array_equal(rgb1, wrgb)
    t = np.float32([dx, 0.0, 0.0])
    placed = q * factor + t  # (fp32 multiply, then fp32 add: SimpleMesh::WriteMesh)
    lines = open(outs[True]).read().split("\n")[2:2 + len(q)]
    assert lines == [" ".join("%g" % c for c in p) for p in placed.astype(np.float64)]
    assert not np.array_equal(q, wv)
