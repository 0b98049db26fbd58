"""arvx_mc_mesh_welded on the device, every layer: the C-ABI through capi.Context.mc_mesh_welded,
the C++ marchingCubesWelded through tools/cpp/arvx_cli -weld.

The welded mesh must be, bit for bit, the numpy restatement of its definition (tests/mesh_weld.py)
applied to the device's unwelded mesh and to the oracle's; its vertex colours must be the model's
colours at the vertex voxels, and they must give every face colour back through the reference's
rule round(((col[a] + col[b]) + col[b]) / 3)."""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_weld as mw
from tests import scenes
from tests.test_cli_gpu import cli, expected  # noqa: F401
from tests.test_cpp_host import write_scene
from tests.test_mc_off import coloured_model, off1, off23, random_coloured_model, state_of  # noqa: F401
from tests.test_mc_weld_cpu import parse_off

pytestmark = pytest.mark.gpu


def face_rule(vrgb, faces):
    """round(((c0 + c1) + c1) / 3) per channel in fp32, rounding half away from zero."""
    a = vrgb[faces[:, 0].astype(np.int64)].astype(np.float32)
    b = vrgb[faces[:, 1].astype(np.int64)].astype(np.float32)
    q = ((a + b) + b) / np.float32(3)
    return np.floor(q.astype(np.float64) + 0.5).astype(np.uint32)


def check_welded(ctx, oracle, X, Y, apply_unseen, model=None):
    """The device's welded mesh against weld(device mesh) and weld(oracle mesh of `model`, or of
    the model the context exports); returns (V, T)."""
    wv, faces, frgb, vrgb = ctx.mc_mesh_welded(apply_unseen, vertex_colors=True)
    v, rgb = ctx.mc_mesh(apply_unseen)
    want = mw.weld(v, rgb)
    for got, w in zip((wv, faces, frgb), want):
        assert got.dtype == w.dtype and np.array_equal(got, w)
    exported = ctx.export_model(apply_unseen)
    ov, orgb = oracle.mc_mesh(X, Y, ctx.Z, exported if model is None else model)
    for got, w in zip((wv, faces, frgb), mw.weld(ov, orgb)):
        assert np.array_equal(got, w)
    # vertex colours: the model's colours at the vertex voxels; the faces follow from them
    assert np.array_equal(vrgb, exported[mw.lattice_index(wv, X, Y), :3])
    assert np.array_equal(face_rule(vrgb, faces), frgb)
    # without vertex colours: the same mesh
    wv2, faces2, frgb2 = ctx.mc_mesh_welded(apply_unseen)
    assert np.array_equal(wv2, wv) and np.array_equal(faces2, faces) and np.array_equal(frgb2, frgb)
    return len(wv), len(faces)


def test_welded_mesh_of_1_off(arvx, oracle, off1):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    with arvx.Context(X, Y, Z, off1["s"]) as ctx:
        ctx.upload_state(state_of(off1["occ"]))
        nv, nt = check_welded(ctx, oracle, X, Y, False)
        wv, faces, _ = ctx.mc_mesh_welded()
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert (nv, nt) == (5704, off1["nf"])
    assert np.array_equal(mw.lattice_index(wv, X, Y), off1["surface_index"])


@pytest.mark.parametrize("name", ["2", "3"])
def test_welded_mesh_of_2_off_and_3_off(arvx, oracle, off1, off23, name):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    with arvx.Context(X, Y, Z, off1["s"]) as ctx:
        ctx.upload_state(state_of(off1["occ"]))
        ctx.upload_colors(off1["surface_index"].astype(np.int64), off23["vox_rgb" + name])
        check_welded(ctx, oracle, X, Y, False,
                     coloured_model(oracle, off1, off23["vox_rgb" + name]))
        _, _, frgb = ctx.mc_mesh_welded()
    assert np.array_equal(frgb.astype(np.uint8), off23["face_rgb" + name])


def test_welded_mesh_random_fills(arvx, oracle):
    """Colour lists, UNSEEN paint and closure colours on random models: rows that end inside a
    64-bit word, models that touch every face of the grid, list sizes past the first guess."""
    rng = np.random.default_rng(31)
    for dims in [(12, 9, 7), (70, 33, 20), (130, 5, 9), (64, 64, 8), (200, 150, 40)]:
        X, Y, Z = dims
        rgba = random_coloured_model(rng, X, Y, Z, False).reshape(Z, Y, X, 4)
        for face in (np.s_[0], np.s_[-1], np.s_[:, 0], np.s_[:, -1], np.s_[:, :, 0], np.s_[:, :, -1]):
            rgba[face] = [77, 88, 99, 1]  # every face of the grid is occupied
        rgba = rgba.reshape(-1, 4)
        occ = rgba[:, 3] != 0
        seen = rng.random(len(rgba)) < 0.8
        state = (occ * 1 | seen * 2).astype(np.uint8)
        plain = occ & ~((rgba[:, :3] == [50, 168, 141]).all(1)) & ~((rgba[:, :3] == [204, 0, 0]).all(1))
        idx = np.flatnonzero(plain)
        with arvx.Context(X, Y, Z, 0.01) as ctx:
            ctx.upload_state(state)
            ctx.upload_colors(idx, rgba[idx, :3])
            check_welded(ctx, oracle, X, Y, False)
            ctx.handle_unseen()
            check_welded(ctx, oracle, X, Y, True)
            ctx.closure(3, True)
            check_welded(ctx, oracle, X, Y, True)


@pytest.mark.parametrize("dims,voxel", [((1, 1, 1), (0, 0, 0)), ((5, 6, 7), (2, 3, 4)),
                                        ((65, 3, 2), (64, 2, 1))])
def test_welded_mesh_single_voxel(arvx, oracle, dims, voxel):
    X, Y, Z = dims
    state = np.full((Z, Y, X), 2, np.uint8)
    state[voxel[2], voxel[1], voxel[0]] = 3
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state(state.reshape(-1))
        nv, nt = check_welded(ctx, oracle, X, Y, False)
        wv, _, _ = ctx.mc_mesh_welded()
    assert nv == 1 and nt > 0 and np.array_equal(wv, np.float32([voxel]))


def test_welded_mesh_empty_model(arvx):
    with arvx.Context(20, 10, 5, 0.01) as ctx:
        ctx.upload_state(np.full(20 * 10 * 5, 2, np.uint8))
        wv, faces, frgb, vrgb = ctx.mc_mesh_welded(vertex_colors=True)
    assert wv.shape == (0, 3) and faces.shape == (0, 3) and frgb.shape == (0, 3) and vrgb.shape == (0, 3)


N = 256


@pytest.fixture(scope="module")
def scene():
    return scenes.syn.sphere_scene(N, 8, with_images=True)


@pytest.mark.parametrize("apply_unseen", [True, False])
def test_welded_mesh_pipeline_256(arvx, oracle, scene, apply_unseen):
    """carve, colour, [handleUnseen,] closure at 256^3: the closure's fills are vertices, and
    their vertex colours are the closure's colours."""
    sc = scene
    with arvx.Context(N, N, N, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.carve()
        ctx.color(arvx.COLOR_AVERAGE)
        if apply_unseen:
            ctx.handle_unseen()
        fidx, frgba = ctx.closure(3, apply_unseen)
        nv, nt = check_welded(ctx, oracle, N, N, apply_unseen)
        wv, _, _, vrgb = ctx.mc_mesh_welded(apply_unseen, vertex_colors=True)
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert nv > 50000 and nt > nv
    vidx = mw.lattice_index(wv, N, N)
    filled = np.isin(vidx, fidx)
    assert filled.any()
    at = np.searchsorted(fidx, vidx[filled])
    assert np.array_equal(vrgb[filled], frgba[at, :3])


def test_slab_and_striped_contexts_are_refused(arvx):
    for kw in (dict(z_range=(0, 16)), dict(z_range=(16, 32)), dict(stripes=(2, 0))):
        with arvx.Context(16, 16, 32, 0.01, **kw) as ctx:
            with pytest.raises(arvx.ArvxError) as e:
                ctx.mc_mesh_welded()
            assert e.value.code == 3 and "whole-grid" in str(e.value)


def test_cli_weld_flag(cli, oracle, tmp_path):  # noqa: F811
    """arvx_cli -c=5 -weld writes the welded form of the OFF the same run writes without -weld;
    that one keeps its bytes."""
    X, Y, Z = 40, 36, 20
    s = np.float32(0.512 / 40)
    sc = scenes.syn.sphere_scene(64, 5, W=160, H=120, with_images=True)
    d = str(tmp_path)
    scene = os.path.join(d, "scene.bin")
    write_scene(scene, 1, 1, 1, 1.0, sc.K, sc.Rt, sc.masks, sc.images, np.ones(1, np.uint8))
    outs = {}
    for weld in (False, True):
        out = os.path.join(d, f"m{int(weld)}.off")
        r = subprocess.run([cli, "-c=5", f"-scene={scene}", "-calibration=none.yml", f"-x={X}",
                            f"-y={Y}", f"-z={Z}", f"-size={float(s)!r}", "-color=2", "-scale=1.5",
                            "-dx=0.25", f"-outFile={out}"] + (["-weld"] if weld else []),
                           capture_output=True, text=True, cwd=d)
        assert r.returncode == 0, r.stderr + r.stdout
        assert "LOG - MC: Mesh written, marchingCubes completed." in r.stdout
        outs[weld] = out
    model = expected(oracle, sc, X, Y, Z, s, 1, 2, True)
    verts, rgb = oracle.mc_mesh(X, Y, Z, model)
    want = oracle.off_text(verts, rgb, np.float32(1.5) * s, (0.25, 0.0, 0.0))
    assert open(outs[False], "rb").read() == want.encode()
    v0, f0, rgb0 = parse_off(outs[False])
    assert np.array_equal(f0.reshape(-1), np.arange(3 * len(f0)))
    wv, wf, wrgb = mw.weld(v0, rgb0)
    v1, f1, rgb1 = parse_off(outs[True])
    assert len(v1) < len(v0)
    assert np.array_equal(v1, wv) and np.array_equal(f1, wf) and np.array_equal(rgb1, wrgb)
