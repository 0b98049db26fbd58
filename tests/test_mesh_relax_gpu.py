"""arvx_mesh_relax and arvx_mesh_relax_triangles on the device, every layer, against the numpy
restatement of arvx_mc_mesh_smooth's definition (tests/mesh_smooth.py) applied to the mesh the context
downloads or the caller gives.  Every comparison is bit for bit on float32.view(uint32): no tolerances.

Where a mesh has a vertex of thousands of neighbours, mesh_smooth's dense neighbour table does not fit
(tests/mesh_relax.py says why); such a mesh is compared with mesh_relax.smooth, the same definition on
CSRs, which tests/test_mesh_relax_cpu.py holds equal to mesh_smooth.smooth bit for bit.  Every mesh
mesh_smooth can take is compared with mesh_smooth itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import mesh_color as mcol
from tests import mesh_relax as mr
from tests import mesh_smooth as ms
from tests import mesh_texture as mtex
from tests.mesh_relax import bits

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 1, 3  # ARVX_ERR_* (include/arvx/arvx.h)
F32 = np.float32
W, H = 160, 120
N = 32
S = F32(0.512 / N)

# one after the other on one mesh, so that the calls after the first run on the cached CSRs
PARAMS = [(0, 0.5, -0.53), (1, 0.5, -0.53), (10, 0.5, -0.53), (3, 0.5, 0.0), (2, 0.33, -0.34)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def code_of(arvx, call, *args, **kw):
    with pytest.raises(arvx.ArvxError) as e:
        call(*args, **kw)
    return e.value.code


@pytest.fixture(scope="module")
def sphere():
    return syn.sphere_scene(N, V=6, W=W, H=H, with_images=True)


def carved(arvx, sc):
    ctx = arvx.Context(N, N, N, S)
    ctx.set_views(sc.M, sc.masks, campos=sc.campos)
    ctx.set_images(sc.images)
    ctx.carve()
    return ctx


# ---- 1. the welded base: the restatement and the lattice smoother ---------------------------------

@pytest.mark.parametrize("dims,fill", [((12, 9, 7), 0.3), ((70, 33, 20), 0.5), ((64, 64, 8), 0.3)])
def test_welded_base_against_both_yardsticks(arvx, dims, fill):
    X, Y, Z = dims
    occ = np.random.default_rng(71).random(X * Y * Z) < fill
    with arvx.Context(X, Y, Z, 0.01) as ctx:
        ctx.upload_state((occ * 1 | 2).astype(np.uint8))
        wv, wf, _ = ctx.mc_mesh_welded()
        nbr_deg, inc = ms.neighbours(len(wv), wf), ms.incidences(len(wv), wf)
        assert nbr_deg[1].max() > 6
        for it, lam, mu in PARAMS:
            q, n, d = ctx.mesh_relax(arvx.MESH_WELDED, it, lam, mu)
            wq, wn = ms.smooth(wv, wf, it, lam, mu, nbr_deg, inc)
            sq, sn = ctx.mc_mesh_smooth(it, lam, mu)  # (the lattice adjacency's kernels)
            assert same(q, wq) and same(n, wn), (it, lam, mu)
            assert same(q, sq) and same(n, sn), (it, lam, mu)
            assert d.dtype == np.int32 and np.array_equal(d, nbr_deg[1])
            assert ctx.mesh_relax_info() == (arvx.MESH_WELDED, len(wv), len(wf))
        # the other products stay what they were
        aq, an = ctx.mc_mesh_smooth_download()
        assert same(aq, sq) and same(an, sn)
        lv, rec = np.empty_like(wv), np.empty((len(wf), 6), np.uint32)
        ctx._ck(ctx._lib.arvx_mc_mesh_welded_download(ctx._h, lv.ctypes.data, rec.ctypes.data, None))
        assert np.array_equal(lv, wv) and np.array_equal(rec[:, :3], wf)
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- 2. every base ---------------------------------------------------------------------------------

def check_base(arvx, ctx, source, verts, faces, params=((2, 0.5, -0.53), (0, 0.5, -0.53))):
    out = None
    for it, lam, mu in params:
        q, n, d = ctx.mesh_relax(source, it, lam, mu)
        wq, wn = ms.smooth(verts, faces, it, lam, mu)
        assert same(q, wq) and same(n, wn), (source, it)
        assert np.array_equal(d, ms.neighbours(len(verts), faces)[1])
        assert ctx.mesh_relax_info() == (source, len(verts), len(faces))
        out = out or (q, n, d)
    return out


def test_every_base(arvx, sphere):
    with carved(arvx, sphere) as ctx:
        wv, wf, _ = ctx.mc_mesh_welded()
        assert len(wv) > 500
        sv, _ = ctx.mc_mesh_smooth(3)
        check_base(arvx, ctx, arvx.MESH_SMOOTHED, sv, wf)  # (relaxing the smoothed positions)
        assert not np.array_equal(sv, wv)
        for source in (arvx.DECIMATE_LATTICE, arvx.DECIMATE_SMOOTHED):
            for cell in (2, 4):
                dv, drec, _, _, _ = ctx.mc_mesh_decimate(cell, source)
                assert len(dv) > 20 and len(drec) > 20
                check_base(arvx, ctx, arvx.MESH_DECIMATED, dv, drec[:, :3])
        for B in (0, 4):
            rv, rf, _ = ctx.mc_mesh_refined(B)
            assert len(rv) > 500
            # the row kernels' launch sized by one compute unit, then by the device's: the same bits
            ctx.selftest_compute_units(1)
            one = check_base(arvx, ctx, arvx.MESH_REFINED, rv, rf)
            ctx.selftest_compute_units(0)
            ctx.mc_mesh_refined(B)  # (a new base: the CSRs are built again)
            all_cus = check_base(arvx, ctx, arvx.MESH_REFINED, rv, rf)
            assert same(one[0], all_cus[0]) and same(one[1], all_cus[1]) and np.array_equal(one[2], all_cus[2])
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- 3. a caller's meshes: the row classes -----------------------------------------------------------

def row_thresholds():
    """kRelaxLaneRow and kRelaxBlockRow as the kernels' header names them."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "ar_voxel_project_amd", "csrc",
                            "mesh_relax_kernels.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
                 for name in ("kRelaxLaneRow", "kRelaxBlockRow"))


def around(t):
    """Fan sizes K whose hub rows end at t - 1, t, t + 1 slots: the hub of a fan with K >= 3 has 4 K
    neighbour slots before the unique pass (two per face, every face twice), 2 K incidences, K neighbours."""
    return sorted({max(t // div + k, 1) for div in (4, 2, 1) for k in (-1, 0, 1)})


def check_fans(arvx, ctx, Ks, isolated, seed, reference):
    verts, faces, degree = mr.fans(Ks, isolated, seed)
    first = True
    for it in (0, 1, 3):
        q, n, d = ctx.mesh_relax_triangles(verts, faces, it, 0.5, -0.53)
        if first:  # (the degrees first: every class of row was reached, and made unique)
            assert np.array_equal(d, degree)
            assert sorted(d[d > 3].tolist()) == sorted(K for K in Ks if K > 3)
            first = False
        wq, wn = reference(verts, faces, it)
        assert same(q, wq), it
        assert same(n, wn), it
        assert np.array_equal(d, degree)
        if it == 0:
            assert same(q, verts)
    return verts, faces, degree


def by_mesh_smooth(verts, faces, it):
    return ms.smooth(verts, faces, it, 0.5, -0.53)


def by_csr_form(verts, faces, it):
    return mr.smooth(verts, faces, it, 0.5, -0.53)[:2]


def test_fans_short_rows_and_the_first_threshold(arvx):
    lane, block = row_thresholds()
    assert (lane, block) == (48, 8192)  # (what around() is told below; a new value needs a look at this test)
    Ks = [1, 2, 3] + around(lane)
    assert {11, 12, 13, 23, 24, 25, 47, 48, 49} <= set(Ks)
    with arvx.Context(8, 8, 8, 0.01) as ctx:
        verts, _, degree = check_fans(arvx, ctx, Ks, 5, 3, by_mesh_smooth)
        assert (degree == 0).sum() == 5
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_fans_the_second_threshold_and_5000(arvx):
    _, block = row_thresholds()
    Ks = around(block) + [5000]
    assert {2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193} <= set(Ks)
    with arvx.Context(8, 8, 8, 0.01) as ctx:
        check_fans(arvx, ctx, Ks, 2, 4, by_csr_form)


def test_fans_a_hub_of_50000(arvx):
    with arvx.Context(8, 8, 8, 0.01) as ctx:
        check_fans(arvx, ctx, [50000, 7], 1, 6, by_csr_form)


def test_fans_300_hubs_of_300_on_one_compute_unit(arvx):
    """The listed rows' launch goes past its first round: 600 rows (a neighbour row and an incidence row
    per hub) on the two workgroups one compute unit gets.  Against mesh_smooth itself."""
    verts, faces, degree = mr.fans([300] * 300, 0, 8)
    with arvx.Context(8, 8, 8, 0.01) as ctx:
        ctx.selftest_compute_units(1)
        q, n, d = ctx.mesh_relax_triangles(verts, faces, 1, 0.5, -0.53)
        assert np.array_equal(d, degree) and (d == 300).sum() == 300
        wq, wn = ms.smooth(verts, faces, 1, 0.5, -0.53)
        assert same(q, wq) and same(n, wn)
        ctx.selftest_compute_units(0)
        q2, n2, d2 = ctx.mesh_relax_triangles(verts, faces, 1, 0.5, -0.53)
        assert same(q, q2) and same(n, n2) and np.array_equal(d, d2)


# ---- 4. degenerate input ------------------------------------------------------------------------------

def test_degenerate_input(arvx):
    rng = np.random.default_rng(2)
    verts = rng.uniform(-4, 4, (12, 3)).astype(F32)
    cases = [
        [[0, 0, 0]], [[1, 1, 2]], [[3, 4, 3]], [[5, 6, 6]],            # (i,i,i) (i,i,j) (i,j,i) (i,j,j)
        [[7, 8, 9], [7, 8, 9], [7, 8, 9]],                             # the same face three times
        [[0, 0, 0], [1, 1, 2], [3, 4, 3], [5, 6, 6], [7, 8, 9], [7, 8, 9], [7, 8, 9], [9, 10, 7], [2, 5, 8],
         [0, 3, 10]],
    ]
    with arvx.Context(8, 8, 8, 0.01) as ctx:
        for faces in cases:
            faces = np.asarray(faces, np.int64)
            for it in (0, 2):
                q, n, d = ctx.mesh_relax_triangles(verts, faces, it, 0.5, -0.53)
                wq, wn = ms.smooth(verts, faces, it, 0.5, -0.53)
                wd = ms.neighbours(len(verts), faces)[1]
                assert same(q, wq) and same(n, wn) and np.array_equal(d, wd), (faces.tolist(), it)
                none = wd == 0
                assert none.any() and same(q[none], verts[none]) and not n[none].any()
        # (T, 6) records: r, g, b are not read
        rec = np.concatenate([faces, np.full((len(faces), 3), 0xFFFFFFFF, np.int64)], axis=1).astype(np.uint32)
        q6, n6, d6 = ctx.mesh_relax_triangles(verts, rec, 2, 0.5, -0.53)
        assert same(q6, q) and same(n6, n) and np.array_equal(d6, d)
        # nv = 1; nt = 0; nv = 0
        q, n, d = ctx.mesh_relax_triangles(verts[:1], np.array([[0, 0, 0]]), 3, 0.5, -0.53)
        assert same(q, verts[:1]) and not n.any() and d.tolist() == [0]
        q, n, d = ctx.mesh_relax_triangles(verts, np.zeros((0, 3), np.int64), 3, 0.5, -0.53)
        assert same(q, verts) and n.shape == (12, 3) and not n.any() and not d.any()
        q, n, d = ctx.mesh_relax_triangles(np.zeros((0, 3), F32), np.zeros((0, 3), np.int64), 3, 0.5, -0.53)
        assert q.shape == (0, 3) and n.shape == (0, 3) and d.shape == (0,)
        with pytest.raises(arvx.ArvxError):  # (no product was made on the way)
            ctx.mesh_relax_info()


# ---- 5. the consumers of MESH_RELAXED ---------------------------------------------------------------

def test_consumers_of_the_relaxed_mesh(arvx, sphere):
    """render_mesh, mesh_color and mesh_texture of MESH_RELAXED with REFINED as base.  The atlas is compared
    with tests/mesh_texture.py's, which takes any positions."""
    sc = sphere
    with carved(arvx, sc) as ctx:
        rv, rf, _, rrgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        q, _, _ = ctx.mesh_relax(arvx.MESH_REFINED, 3)
        assert same(q, ms.taubin(rv, rf, 3)) and not np.array_equal(q, rv)
        M = sc.M[2]
        light = arvx.headlight(M)
        got = ctx.render_mesh(arvx.MESH_RELAXED, M, W, H, light=light)
        want = ctx.render_triangles(q, rrgb, rf, M, W, H, light=light)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        assert (got[2] >= 0).any() and (got[2] < 0).any()
        got0_id = got[2].tobytes()  # (the faces under the pixels: the same whatever colours them)
        own = ctx.render_mesh(arvx.MESH_REFINED, M, W, H, light=light)
        assert own[1].tobytes() != got[1].tobytes()  # (the base's own positions draw another image)
        depth = got[1][np.isfinite(got[1]) & (got[2] >= 0)]
        ctx.set_render_near(float(np.median(depth)))  # (a plane through the middle of the model)
        got = ctx.render_mesh(arvx.MESH_RELAXED, M, W, H, light=light)
        want = ctx.render_triangles(q, rrgb, rf, M, W, H, light=light)
        assert ctx.render_mesh_clip_stats()[1] > 0
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        ctx.set_render_near(0.0)
        tol = float(F32(1.5) * S)
        for mode in (arvx.COLOR_CLOSEST, arvx.COLOR_AVERAGE):
            rgb, views, coloured = ctx.mesh_color(arvx.MESH_RELAXED, mode, tol)
            w = mcol.color(sc.M, S, q, rrgb, rf, sc.images, mode, tol, 0, sc.masks)
            assert np.array_equal(views, w.views) and same(rgb, w.rgb) and coloured == w.coloured > 0
        drawn = ctx.render_mesh(arvx.MESH_RELAXED | arvx.MESH_IMAGE_COLORS, M, W, H)
        want = ctx.render_triangles(q, rgb, rf, M, W, H)
        for a, b in zip(drawn, want):
            assert a.tobytes() == b.tobytes()
        atlas, face_view, face_uv, counts = ctx.mesh_texture(arvx.MESH_RELAXED, 4, 256, tol)
        t = mtex.texture(sc.M, S, q, rrgb, rf, sc.images, 4, 256, tol)
        assert counts == t.counts and counts[1] > 0 and np.array_equal(face_view, t.face_view)
        assert atlas.tobytes() == t.atlas.tobytes() and same(face_uv, t.face_uv)
        tex = ctx.render_mesh(arvx.MESH_RELAXED | arvx.MESH_TEXTURED, M, W, H)
        assert (tex[2] >= 0).any() and tex[2].tobytes() == got0_id
        assert ctx.mesh_relax_info() == (arvx.MESH_REFINED, len(rv), len(rf))


# ---- 6. lifetimes and refusals ------------------------------------------------------------------------

def gone(arvx, ctx):
    return (code_of(arvx, ctx.mesh_relax_info) == ERR_STATE and code_of(arvx, ctx.mesh_relax_download) == ERR_STATE
            and code_of(arvx, ctx.render_mesh, arvx.MESH_RELAXED, np.eye(3, 4), 8, 8) == ERR_STATE)


def test_lifetimes(arvx, sphere):
    sc = sphere
    tol = float(F32(1.5) * S)
    M = sc.M[0]
    with carved(arvx, sc) as ctx:
        assert gone(arvx, ctx)
        assert code_of(arvx, ctx.mesh_relax, arvx.MESH_WELDED) == ERR_STATE  # no welded mesh
        wv, wf, _ = ctx.mc_mesh_welded()
        for src in (arvx.MESH_SMOOTHED, arvx.MESH_DECIMATED, arvx.MESH_REFINED):
            assert code_of(arvx, ctx.mesh_relax, src) == ERR_STATE
        assert gone(arvx, ctx)
        # base WELDED: what leaves it alone
        first = ctx.mesh_relax(arvx.MESH_WELDED, 2)
        info = (arvx.MESH_WELDED, len(wv), len(wf))
        state = ctx.download_state()
        ctx.carve()
        ctx.upload_state(state)
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.render_mesh(arvx.MESH_WELDED, M, W, H)
        ctx.render_mesh(arvx.MESH_RELAXED, M, W, H)
        ctx.mc_mesh_smooth(1)
        ctx.mc_mesh_decimate(2)
        ctx.mc_mesh_refined(2)
        assert ctx.mesh_relax_info() == info
        assert all(same(a, b) for a, b in zip(ctx.mesh_relax_download(), first))
        # ... and what is made of it ends with it
        ctx.mesh_color(arvx.MESH_RELAXED, arvx.COLOR_AVERAGE, tol)
        ctx.render_mesh(arvx.MESH_RELAXED | arvx.MESH_IMAGE_COLORS, M, W, H)
        ctx.mesh_texture(arvx.MESH_RELAXED, 3, 256, tol)
        ctx.render_mesh(arvx.MESH_RELAXED | arvx.MESH_TEXTURED, M, W, H)
        smooth_before = ctx.mc_mesh_smooth_download()
        ctx.mesh_relax(arvx.MESH_WELDED, 1)  # replaced: its image colours and its texture are gone
        for bit in (arvx.MESH_IMAGE_COLORS, arvx.MESH_TEXTURED):
            assert code_of(arvx, ctx.render_mesh, arvx.MESH_RELAXED | bit, M, W, H) == ERR_STATE
        assert all(same(a, b) for a, b in zip(ctx.mc_mesh_smooth_download(), smooth_before))
        ctx.mesh_color(arvx.MESH_RELAXED, arvx.COLOR_AVERAGE, tol)
        ctx.mesh_texture(arvx.MESH_WELDED, 3, 256, tol)  # (a texture of another source stays)
        ctx.mc_mesh_welded()
        assert gone(arvx, ctx)
        assert code_of(arvx, ctx.render_mesh, arvx.MESH_RELAXED | arvx.MESH_IMAGE_COLORS, M, W, H) == ERR_STATE
        # base SMOOTHED: the smoother and the welded mesh end it
        ctx.mc_mesh_smooth(2)
        ctx.mesh_relax(arvx.MESH_SMOOTHED, 1)
        ctx.mc_mesh_decimate(2)
        ctx.mc_mesh_refined(2)
        assert ctx.mesh_relax_info()[0] == arvx.MESH_SMOOTHED
        ctx.mc_mesh_smooth(1)
        assert gone(arvx, ctx)
        ctx.mesh_relax(arvx.MESH_SMOOTHED, 1)
        ctx.mc_mesh_welded()
        assert gone(arvx, ctx)
        # base DECIMATED: the decimation and the welded mesh end it
        ctx.mc_mesh_decimate(2)
        ctx.mesh_relax(arvx.MESH_DECIMATED, 1)
        ctx.mc_mesh_smooth(1)
        ctx.mc_mesh_refined(2)
        assert ctx.mesh_relax_info()[0] == arvx.MESH_DECIMATED
        ctx.mc_mesh_decimate(4)
        assert gone(arvx, ctx)
        ctx.mesh_relax(arvx.MESH_DECIMATED, 1)
        ctx.mc_mesh_welded()
        assert gone(arvx, ctx)
        # base REFINED: only the refined mesh ends it
        rv, rf, _ = ctx.mc_mesh_refined(2)
        ctx.mesh_relax(arvx.MESH_REFINED, 1)
        ctx.mc_mesh_welded()
        ctx.mc_mesh_smooth(1)
        ctx.mc_mesh_decimate(2)
        assert ctx.mesh_relax_info() == (arvx.MESH_REFINED, len(rv), len(rf))
        ctx.mesh_relax(arvx.MESH_WELDED, 1)  # the next product replaces it
        assert ctx.mesh_relax_info()[0] == arvx.MESH_WELDED
        ctx.mesh_relax(arvx.MESH_REFINED, 1)
        ctx.mc_mesh_refined(2)
        assert gone(arvx, ctx)


def test_refusals(arvx, sphere):
    lib = arvx.load_library()
    f = C.c_float
    with carved(arvx, sphere) as ctx:
        wv, wf, _ = ctx.mc_mesh_welded()
        first = ctx.mesh_relax(arvx.MESH_WELDED, 2)
        info = (arvx.MESH_WELDED, len(wv), len(wf))

        def unchanged():
            return ctx.mesh_relax_info() == info and all(same(a, b) for a, b in zip(ctx.mesh_relax_download(), first))

        for args in [(arvx.MESH_WELDED, -1, 0.5, -0.53), (arvx.MESH_WELDED, 1, float("nan"), -0.53),
                     (arvx.MESH_WELDED, 1, 0.5, float("inf")), (7, 1, 0.5, -0.53), (4, 1, 0.5, -0.53), (-1, 1, 0.5, -0.53),
                     (arvx.MESH_RELAXED, 1, 0.5, -0.53), (arvx.MESH_WELDED | arvx.MESH_IMAGE_COLORS, 1, 0.5, -0.53),
                     (arvx.MESH_WELDED | arvx.MESH_TEXTURED, 1, 0.5, -0.53)]:
            assert code_of(arvx, ctx.mesh_relax, *args) == ERR_INVALID, args
            assert unchanged()
        for src in (arvx.MESH_SMOOTHED, arvx.MESH_DECIMATED, arvx.MESH_REFINED):
            assert code_of(arvx, ctx.mesh_relax, src) == ERR_STATE
            assert unchanged()
        # a caller's mesh
        v = np.arange(12, dtype=F32).reshape(4, 3)
        rec = np.zeros((2, 6), np.uint32)
        rec[:, :3] = [[0, 1, 2], [1, 2, 3]]
        out = np.empty((4, 3), F32)

        def tri(nv, verts, nt, faces, it=1, lam=0.5, mu=-0.53):
            return lib.arvx_mesh_relax_triangles(ctx._h, nv, verts, nt, faces, it, f(lam), f(mu), out.ctypes.data, None,
                                                 None)

        vp, fp = v.ctypes.data, rec.ctypes.data
        assert tri(4, vp, 2, fp) == 0 and same(out, ms.taubin(v, rec[:, :3], 1))
        bad = rec.copy()
        bad[1, 2] = 4
        nan, big, edge = v.copy(), v.copy(), v.copy()
        nan[2, 1] = np.nan
        big[3, 0] = F32(2.0 ** 20 + 1)
        edge[3, 0] = -F32(2.0 ** 20)
        inf = v.copy()
        inf[0, 2] = -np.inf
        for args in [(-1, vp, 2, fp), (4, vp, -1, fp), (4, None, 2, fp), (4, vp, 2, None), (4, vp, 2, bad.ctypes.data),
                     (4, nan.ctypes.data, 2, fp), (4, big.ctypes.data, 2, fp), (4, inf.ctypes.data, 2, fp),
                     (4, vp, (2 ** 31 - 1) // 6 + 1, fp), ((2 ** 31 - 1) // 3 + 1, vp, 2, fp),
                     (4, vp, 2, fp, -1), (4, vp, 2, fp, 1, float("nan")), (4, vp, 2, fp, 1, 0.5, float("-inf"))]:
            assert tri(*args) == ERR_INVALID, args
            assert unchanged()
        assert tri(4, edge.ctypes.data, 2, fp) == 0  # (2^20 itself is in range)
        assert tri(0, None, 0, None) == 0 and tri(4, vp, 0, None) == 0
        assert unchanged()
        # the raw C-ABI: a null context, every download pointer null, null info
        assert lib.arvx_mesh_relax(None, 0, 1, f(0.5), f(-0.53)) != 0
        assert lib.arvx_mesh_relax_info(None, (C.c_int64 * 3)()) != 0
        assert lib.arvx_mesh_relax_download(None, None, None, None) != 0
        assert lib.arvx_mesh_relax_triangles(None, 0, None, 0, None, 1, f(0.5), f(-0.53), None, None, None) != 0
        assert lib.arvx_mesh_relax_info(ctx._h, None) == ERR_INVALID
        assert lib.arvx_mesh_relax_download(ctx._h, None, None, None) == 0
        assert tri(4, vp, 2, fp) == 0
        assert lib.arvx_mesh_relax_triangles(ctx._h, 4, vp, 2, fp, 1, f(0.5), f(-0.53), None, None, None) == 0
        assert unchanged()


def test_slab_and_striped_contexts_are_refused(arvx):
    v = np.zeros((3, 3), F32)
    for kw in (dict(z_range=(0, 16)), dict(z_range=(16, 32)), dict(stripes=(2, 0))):
        with arvx.Context(16, 16, 32, 0.01, **kw) as ctx:
            assert code_of(arvx, ctx.mesh_relax, arvx.MESH_WELDED) == ERR_STATE
            assert code_of(arvx, ctx.mesh_relax_triangles, v, [[0, 1, 2]], 1) == ERR_STATE
            assert code_of(arvx, ctx.mesh_relax_info) == ERR_STATE
