"""The second attempt of every call that builds a list of unknown length, forced: on a
fresh context no pool has a size yet, so each list gets its first-capacity room, and every list of
the scene (tests/list_retry.py) is longer than that -- tests/test_list_retry_cpu.py asserts it.  The
first run of a stage on a fresh context therefore launches twice; its results must equal what the
suite compares that stage with everywhere else.  The second run on the same context finds pools with
room for all -- the single-attempt path -- and must give the same arrays.

A list stage runs its second attempt only where its own pools are fresh: the cell list's pool is
shared by arvx_mc_cells, arvx_mc_mesh, arvx_mc_mesh_welded and arvx_mc_mesh_refined, the surface list's
by arvx_color, arvx_color_visible and arvx_photo_carve, and the closure fills the noise almost solid
(few cells).  So each of those entry points also gets a context of its own, next to the sequence on one
context."""
import numpy as np
import pytest

from tests import list_retry as lr
from tests import mesh_weld as mw

pytestmark = pytest.mark.gpu

X, Y, Z = lr.X, lr.Y, lr.Z


@pytest.fixture(scope="module")
def sc():
    return lr.scene()


@pytest.fixture(scope="module")
def want(oracle, sc):
    return lr.references(oracle, sc)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_mesh(got, mesh):
    for g, w in zip(got, mesh):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def check_welded(ctx, got, mesh, unwelded):
    """As tests/test_mc_weld_gpu.py: the weld of the oracle's mesh and of the device's unwelded one;
    the vertex colours are the model's at the vertex voxels."""
    wv, faces, frgb, vrgb = got
    for w in (mesh, mw.weld(*unwelded)):
        assert np.array_equal(wv, w[0]) and np.array_equal(faces, w[1]) and np.array_equal(frgb, w[2])
    assert np.array_equal(vrgb, ctx.export_model(False)[mw.lattice_index(wv, X, Y), :3])


def coloured(ctx, arvx, want):
    ctx.color(arvx.COLOR_AVERAGE)
    idx, rgb = ctx.surface()
    model = ctx.export_model(False)
    assert np.array_equal(model, want.coloured)
    assert np.all(np.diff(idx) > 0) and np.array_equal(rgb, want.coloured[idx, :3])
    return [idx, rgb, model]


def stage_sequence(ctx, arvx, want):
    """The pipeline on one context: the surface list and the fills run their second attempt."""
    out = coloured(ctx, arvx, want)
    fidx, frgba = ctx.closure(3, False)
    closed = ctx.export_model(False)
    assert np.array_equal(closed, want.closed)
    filled = np.flatnonzero((want.closed[:, 3] != 0) & (want.coloured[:, 3] == 0))
    assert np.array_equal(fidx, filled) and np.array_equal(frgba, want.closed[filled])
    cells = ctx.mc_cells()
    assert np.array_equal(cells, want.cells_closed)
    mesh = ctx.mc_mesh(False)
    check_mesh(mesh, want.mesh_closed)
    welded = ctx.mc_mesh_welded(False, vertex_colors=True)
    check_welded(ctx, welded, want.welded_closed, mesh)
    return out + [fidx, frgba, closed, cells, *mesh, *welded]


def stage_cells(ctx, arvx, want):
    cells = ctx.mc_cells()
    assert np.array_equal(cells, want.cells)
    return [cells]


def stage_mesh(ctx, arvx, want):
    out = coloured(ctx, arvx, want)
    mesh = ctx.mc_mesh(False)
    check_mesh(mesh, want.mesh)
    return out + [*mesh]


def stage_welded(ctx, arvx, want):
    out = coloured(ctx, arvx, want)
    welded = ctx.mc_mesh_welded(False, vertex_colors=True)
    check_welded(ctx, welded, want.welded, ctx.mc_mesh(False))
    return out + [*welded]


def stage_refined(ctx, arvx, want):
    """As check_refined of tests/test_mc_refine_gpu.py, against the restatement of the state and the
    colours the context holds: positions and colours bit for bit, edges, cuts and faces equal."""
    out = coloured(ctx, arvx, want)
    assert ctx.assoc == arvx.ASSOC_LEFT
    assert np.array_equal(ctx.download_state().reshape(-1) & 1, want.coloured[:, 3] != 0)
    verts, faces, frgb, vrgb, edges, cut = ctx.mc_mesh_refined(lr.BISECTIONS, False, vertex_colors=True,
                                                               details=True)
    w = want.refined
    assert verts.shape == w["verts"].shape and faces.shape == w["faces"].shape
    assert np.array_equal(edges, w["edges"]) and np.array_equal(cut, w["cut"])
    assert np.array_equal(bits(verts), bits(w["verts"])) and np.array_equal(bits(vrgb), bits(w["vertex_rgb"]))
    assert np.array_equal(faces, w["faces"]) and np.array_equal(frgb, w["face_rgb"])
    return out + [verts, faces, frgb, vrgb, edges, cut]


def stage_visible(ctx, arvx, want):
    """As tests/test_color_visible_gpu.py: coloured voxels, colours, visible-view counts, depth buffers."""
    ctx.color_visible(lr.MODE, lr.TOL)
    idx, rgb = ctx.surface()
    views = ctx.surface_visible()
    zb = np.stack([ctx.view_depth(v) for v in range(lr.V)])
    w = want.visible
    assert np.array_equal(idx, w.index[w.has]) and np.array_equal(rgb, w.rgba[idx, :3])
    assert np.array_equal(views, w.views[w.has])
    assert np.array_equal(zb.view(np.uint32), w.zbuf.view(np.uint32))
    return [idx, rgb, views, zb]


def stage_photo(ctx, arvx, want):
    """As tests/test_photo_carve_gpu.py: iterations, removals and the final state."""
    it, removed = ctx.photo_carve(lr.PHOTO["max_std"], lr.PHOTO["min_views"], lr.TOL, lr.PHOTO["iterations"])
    state = ctx.download_state().reshape(-1)
    assert (it, removed) == (want.photo.iterations, want.photo.removed)
    assert np.array_equal(state, want.photo.state)
    return [np.array([it, removed]), state]


@pytest.mark.parametrize("stage", [stage_sequence, stage_cells, stage_mesh, stage_welded, stage_refined,
                                   stage_visible, stage_photo], ids=lambda f: f.__name__[6:])
def test_second_attempt_then_single_attempt(arvx, sc, want, stage):
    with arvx.Context(X, Y, Z, lr.S) as ctx:  # fresh: no pool has a size
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        runs = []
        for _ in range(2):  # the second attempt inside the first run; the single-attempt path in the second
            ctx.upload_state(sc.state)
            runs.append(stage(ctx, arvx, want))
        assert ctx.stats()["host_total_fallbacks"] == 0
    assert len(runs[0]) == len(runs[1])
    for first, again in zip(*runs):
        assert first.dtype == again.dtype and np.array_equal(first, again)
