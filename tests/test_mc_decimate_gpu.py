"""arvx_mc_mesh_decimate on the device, every layer: the C-ABI through capi.Context.mc_mesh_decimate,
the C++ marchingCubesDecimated through tools/cpp/arvx_cli -decimate.

The decimated mesh must be, bit for bit, the numpy restatement of the definition
(tests/mesh_decimate.py) applied to the device's own welded (and smoothed) mesh.  That the models
used here reach the cases the kernels can get wrong is asserted in tests/test_mc_decimate_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_decimate as md
from tests import mesh_smooth as ms
from tests import mesh_weld as mw
from tests import scenes
from tests.test_cli_gpu import cli, expected  # noqa: F401
from tests.test_cpp_host import write_scene
from tests.test_mc_off import off1, random_coloured_model, state_of  # noqa: F401
from tests.test_mc_weld_cpu import parse_off

pytestmark = pytest.mark.gpu

SMOOTHINGS = [(1, 0.5, -0.53), (10, 0.5, 0.0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def welded_download(ctx, nv, nt):
    """arvx_mc_mesh_welded_download of the mesh the context holds, without building it again."""
    verts = np.empty((nv, 3), np.float32)
    records = np.empty((nt, 6), np.uint32)
    vrgb = np.empty((nv, 3), np.float32)
    ctx._ck(ctx._lib.arvx_mc_mesh_welded_download(ctx._h, verts.ctypes.data, records.ctypes.data,
                                                  vrgb.ctypes.data))
    return verts, records, vrgb


def same(got, want, q, what):
    """A downloaded decimated mesh against the restatement `want` (of the lattice source) with the
    positions of source q (None: the lattice)."""
    verts, records, rgb, members, vmap = got
    wverts = want["verts"] if q is None else md.means(q, want["map"].astype(np.int64), want["members"])
    assert verts.shape == wverts.shape and records.shape == want["records"].shape, what
    assert np.array_equal(bits(verts), bits(wverts)), what
    assert np.array_equal(bits(rgb), bits(want["rgb"])), what
    assert np.array_equal(records, want["records"]), what
    assert np.array_equal(members, want["members"]) and np.array_equal(vmap, want["map"]), what


def check_decimate(ctx, apply_unseen=False, cells=md.CELLS, smoothings=()):
    """Every cell, one call after the other on the same context, from the lattice and from every
    smoothing, against the restatement on the device's welded mesh; after every decimation the
    welded and the smoothed mesh are what they were.  Returns {cell: (Vd, Td)}."""
    wv, faces, frgb, vrgb = ctx.mc_mesh_welded(apply_unseen, vertex_colors=True)
    rec = np.ascontiguousarray(np.hstack([faces, frgb]).astype(np.uint32))
    want = {cell: md.decimate(wv, rec, cell, col=vrgb) for cell in cells}
    counts = {}
    for params in (None,) + tuple(smoothings):
        q = n = None
        if params is not None:
            q, n = ctx.mc_mesh_smooth(*params)
        for cell in cells:
            source = 0 if params is None else 1
            got = ctx.mc_mesh_decimate(cell, source)
            same(got, want[cell], q, (cell, params))
            counts[cell] = ctx.mc_mesh_decimate(cell, source, download=False)
            assert counts[cell] == (len(want[cell]["verts"]), len(want[cell]["records"]))
            lv, lrec, lrgb = welded_download(ctx, len(wv), len(rec))
            assert np.array_equal(bits(lv), bits(wv)) and np.array_equal(lrec, rec)
            assert np.array_equal(bits(lrgb), bits(vrgb))
            if params is not None:
                q2, n2 = ctx.mc_mesh_smooth_download()
                assert np.array_equal(bits(q2), bits(q)) and np.array_equal(bits(n2), bits(n))
    if 1 in cells:
        assert counts[1][0] == len(wv)
    return counts


def test_decimated_mesh_of_1_off(arvx, off1):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    with arvx.Context(X, Y, Z, off1["s"]) as ctx:
        ctx.upload_state(state_of(off1["occ"]))
        counts = check_decimate(ctx, smoothings=SMOOTHINGS)
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert counts[1][0] == 5704 and counts[1][1] < off1["nf"] and counts[2][0] < 5704 / 3


@pytest.mark.parametrize("k", range(len(md.FILLS)))
def test_decimated_mesh_random_fills(arvx, k):
    """The fills tests/test_mc_decimate_cpu.py examines: degenerate and repeated faces, clusters
    across two words of a row, clusters the grid's end cuts short."""
    X, Y, Z = md.FILLS[k][0]
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state(md.fill_state(k))
        check_decimate(ctx, smoothings=SMOOTHINGS)
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_decimated_mesh_colour_and_unseen(arvx):
    """A coloured model with UNSEEN paint under both apply_unseen: the colours are means too."""
    rng = np.random.default_rng(79)
    X, Y, Z = 40, 30, 20
    rgba = random_coloured_model(rng, X, Y, Z, False).reshape(-1, 4)
    occ = rgba[:, 3] != 0
    seen = rng.random(len(rgba)) < 0.8
    plain = occ & ~((rgba[:, :3] == [50, 168, 141]).all(1)) & ~((rgba[:, :3] == [204, 0, 0]).all(1))
    idx = np.flatnonzero(plain)
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state((occ * 1 | seen * 2).astype(np.uint8))
        ctx.upload_colors(idx, rgba[idx, :3])
        check_decimate(ctx, False, smoothings=SMOOTHINGS[:1])
        _, _, rgb0, _, _ = ctx.mc_mesh_decimate(2)
        ctx.handle_unseen()
        check_decimate(ctx, True, smoothings=SMOOTHINGS[:1])
        _, _, rgb1, _, _ = ctx.mc_mesh_decimate(2)
    assert len(np.unique(rgb0, axis=0)) > 100  # (colours, not one default)
    assert not np.array_equal(rgb0, rgb1)


@pytest.mark.parametrize("dims,voxel", [((1, 1, 1), (0, 0, 0)), ((65, 3, 2), (64, 2, 1))])
def test_decimated_mesh_single_voxel(arvx, dims, voxel):
    """One vertex, every face (i, i, i): one decimated vertex at the voxel, no face."""
    X, Y, Z = dims
    state = np.full((Z, Y, X), 2, np.uint8)
    state[voxel[2], voxel[1], voxel[0]] = 3
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state(state.reshape(-1))
        counts = check_decimate(ctx, smoothings=SMOOTHINGS[:1])
        verts, records, _, members, vmap = ctx.mc_mesh_decimate(3)
    assert set(counts.values()) == {(1, 0)}
    assert np.array_equal(verts, np.float32([voxel])) and records.shape == (0, 6)
    assert members.tolist() == [1] and vmap.tolist() == [0]


def test_decimated_mesh_empty_model(arvx):
    with arvx.Context(20, 10, 5, 0.01) as ctx:
        ctx.upload_state(np.full(20 * 10 * 5, 2, np.uint8))
        assert ctx.mc_mesh_welded_count() == (0, 0)
        assert ctx.mc_mesh_decimate(2, download=False) == (0, 0)
        out = ctx.mc_mesh_decimate(2)
        ctx.mc_mesh_smooth(1, download=False)
        assert ctx.mc_mesh_decimate(2, 1, download=False) == (0, 0)
    assert [a.shape for a in out] == [(0, 3), (0, 6), (0, 3), (0,), (0,)]


def test_buffers_are_reused_and_grown(arvx):
    """One context, meshes and cells of changing size one after the other: a small mesh after a
    large one, a fine cell after a coarse one."""
    X, Y, Z = 70, 33, 20
    rng = np.random.default_rng(83)
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        for fill, cells in [(0.02, (64, 1)), (0.5, (7, 2, 1, 64)), (0.05, (3, 1))]:
            ctx.upload_state(((rng.random(X * Y * Z) < fill) * 1 | 2).astype(np.uint8))
            check_decimate(ctx, cells=cells)
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_download_pointers_one_at_a_time(arvx):
    with arvx.Context(12, 9, 7, 0.01) as ctx:
        ctx.upload_state(md.fill_state(0))
        ctx.mc_mesh_welded()
        full = ctx.mc_mesh_decimate(2)
        names = ["verts", "faces", "vertex_rgb", "members", "vmap"]
        for k, name in enumerate(names):
            one = ctx.mc_mesh_decimate_download(**{n: n == name for n in names})
            assert [a is not None for a in one] == [n == name for n in names]
            assert one[k].tobytes() == full[k].tobytes() and one[k].shape == full[k].shape
        assert ctx._lib.arvx_mc_mesh_decimate_download(ctx._h, None, None, None, None, None) == 0


def test_state_and_argument_errors(arvx):
    with arvx.Context(12, 9, 7, 0.01) as ctx:
        ctx.upload_state(md.fill_state(0))
        with pytest.raises(arvx.ArvxError) as e:  # no welded mesh
            ctx.mc_mesh_decimate(2)
        assert e.value.code == 3
        ctx.mc_mesh_welded()
        with pytest.raises(arvx.ArvxError) as e:  # download before a decimation
            ctx.mc_mesh_decimate_download()
        assert e.value.code == 3
        with pytest.raises(arvx.ArvxError) as e:  # SMOOTHED without a smoothed mesh
            ctx.mc_mesh_decimate(2, arvx.DECIMATE_SMOOTHED)
        assert e.value.code == 3
        full = ctx.mc_mesh_decimate(2)
        assert len(full[0]) > 1
        # every refusal leaves that result downloadable
        for cell, source in [(0, 0), (65, 0), (-1, 0), (2, 2), (2, -1)]:
            with pytest.raises(arvx.ArvxError) as e:
                ctx.mc_mesh_decimate(cell, source)
            assert e.value.code == 1, (cell, source)
        with pytest.raises(arvx.ArvxError) as e:
            ctx.mc_mesh_decimate(3, arvx.DECIMATE_SMOOTHED)
        assert e.value.code == 3
        n = C.c_int64()
        assert ctx._lib.arvx_mc_mesh_decimate(ctx._h, 2, 0, None, C.byref(n)) == 1
        assert ctx._lib.arvx_mc_mesh_decimate(ctx._h, 2, 0, C.byref(n), None) == 1
        assert ctx._lib.arvx_mc_mesh_decimate(None, 2, 0, C.byref(n), C.byref(n)) == 1
        again = ctx.mc_mesh_decimate_download()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, full))
        # a smoothed mesh on this welded mesh: SMOOTHED is accepted
        ctx.mc_mesh_smooth(1, download=False)
        ctx.mc_mesh_decimate(2, arvx.DECIMATE_SMOOTHED)
        # a new welded mesh: the decimated one and the smoothed one are gone
        ctx.mc_mesh_welded()
        with pytest.raises(arvx.ArvxError) as e:
            ctx.mc_mesh_decimate_download()
        assert e.value.code == 3
        with pytest.raises(arvx.ArvxError) as e:
            ctx.mc_mesh_decimate(2, arvx.DECIMATE_SMOOTHED)
        assert e.value.code == 3


def test_slab_and_striped_contexts_are_refused(arvx):
    for kw in (dict(z_range=(0, 16)), dict(z_range=(16, 32)), dict(stripes=(2, 0))):
        with arvx.Context(16, 16, 32, 0.01, **kw) as ctx:
            with pytest.raises(arvx.ArvxError) as e:
                ctx.mc_mesh_decimate(2)
            assert e.value.code == 3


def test_other_mesh_products_are_unchanged(arvx):
    """A render and the unwelded mesh return after a decimation what they returned before."""
    sc = scenes.syn.sphere_scene(32, 4, W=80, H=60, with_images=True)
    with arvx.Context(32, 32, 32, sc.voxel_size) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.carve()
        mv, mrgb = ctx.mc_mesh()
        ctx.mc_mesh_welded()
        r0 = ctx.render(sc.M[0], 80, 60)
        ctx.mc_mesh_decimate(2)
        ctx.mc_mesh_smooth(2, download=False)
        ctx.mc_mesh_decimate(3, arvx.DECIMATE_SMOOTHED)
        r1 = ctx.render(sc.M[0], 80, 60)
        mv1, mrgb1 = ctx.mc_mesh()
    assert all(np.array_equal(a, b) for a, b in zip(r0, r1))
    assert np.array_equal(mv, mv1) and np.array_equal(mrgb, mrgb1)


@pytest.mark.parametrize("smooth", [0, 3])
def test_cli_decimate_flag(cli, oracle, tmp_path, smooth):  # noqa: F811
    """arvx_cli -c=5 -weld -decimate=2 and -smooth=3 -decimate=2 write the decimated welded mesh of
    the run, through the writer's scale and translation."""
    X, Y, Z = 40, 36, 20
    s = np.float32(0.512 / 40)
    scale, dx = 1.5, 0.25
    sc = scenes.syn.sphere_scene(64, 5, W=160, H=120, with_images=True)
    d = str(tmp_path)
    scene = os.path.join(d, "scene.bin")
    write_scene(scene, 1, 1, 1, 1.0, sc.K, sc.Rt, sc.masks, sc.images, np.ones(1, np.uint8))
    out = os.path.join(d, "m.off")
    flag = ["-smooth=3", "-decimate=2"] if smooth else ["-weld", "-decimate=2"]
    r = subprocess.run([cli, "-c=5", f"-scene={scene}", "-calibration=none.yml", f"-x={X}", f"-y={Y}",
                        f"-z={Z}", f"-size={float(s)!r}", "-color=2", f"-scale={scale}", f"-dx={dx}",
                        f"-outFile={out}"] + flag, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "LOG - MC: Mesh written, marchingCubes completed." in r.stdout
    model = expected(oracle, sc, X, Y, Z, s, 1, 2, True)
    verts, rgb = oracle.mc_mesh(X, Y, Z, model)
    wv, wf, wrgb = mw.weld(verts, rgb)
    rec = np.hstack([wf, wrgb]).astype(np.uint32)
    want = md.decimate(wv, rec, 2, q=ms.taubin(wv, wf, smooth) if smooth else None)
    assert 0 < len(want["verts"]) < len(wv) / 3 and 0 < len(want["records"]) < len(rec) / 3
    _, f1, rgb1 = parse_off(out)
    assert np.array_equal(f1, want["records"][:, :3]) and np.array_equal(rgb1, want["records"][:, 3:])
    factor = np.float32(scale) * s
    placed = want["verts"] * factor + np.float32([dx, 0.0, 0.0])  # (fp32 multiply, then fp32 add)
    lines = open(out).read().split("\n")[2:2 + len(placed)]
    assert lines == [" ".join("%g" % c for c in p) for p in placed.astype(np.float64)]
