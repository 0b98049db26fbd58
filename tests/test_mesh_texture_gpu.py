"""arvx_mesh_texture on the device, every layer, against the numpy restatement of its definition
(tests/mesh_texture.py) fed with the mesh arrays the context downloads: the atlas, the faces' views,
their UVs (as bits) and the four counts compared with np.array_equal, no tolerances.  The four sources in
both row-sum groupings; an odd number of faces; occlusion between two walls; faces nobody sees; a tie;
the foreground flag; the self-test hooks of the shared depth pass; cameras inside the grid and corners
on the image's border; drawing with the texture; the interplay with arvx_mesh_color; refusals and
lifetimes.  What each scene must hold is asserted on the restatement alone in
tests/test_mesh_texture_cpu.py."""
import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import mesh_color as mcol
from tests import mesh_texture as mt
from tests import render_mesh as rm
from tests.test_mesh_color_cpu import EDGE_H, EDGE_W, WALLS_N, edge_scene, noise_image, walls_scene, walls_state
from tests.test_mesh_color_gpu import set_views_without_masks
from tests.test_mesh_texture_cpu import (LARGE_V, ODD_CELL, ODD_N, far_side_pairs, hidden_pairs, large_scene, tie_scene,
                                         unowned)
from tests.test_render_gpu import _err, same, upload_random_colours
from tests.test_render_mesh_gpu import SOURCES, build_meshes, large_context

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 1, 3  # ARVX_ERR_* (include/arvx/arvx.h)
F32, I64 = np.float32, np.int64
W, H = 160, 120


@pytest.fixture(scope="module")
def sphere():
    return syn.sphere_scene(32, V=6, W=W, H=H, with_images=True)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check(got, want):
    """(atlas, face_view, face_uv, counts) of a mesh_texture call against the restatement's."""
    atlas, view, uv, counts = got
    assert atlas.dtype == np.uint8 and view.dtype == np.int32 and uv.dtype == np.float32
    assert counts == want.counts, (counts, want.counts)
    assert np.array_equal(view, want.face_view), "face_view"
    assert atlas.shape == want.atlas.shape and np.array_equal(atlas, want.atlas), "atlas"
    assert np.array_equal(bits(uv), bits(want.face_uv)), "face_uv"


def faces3(faces):
    return np.asarray(faces)[:, :3].astype(I64)


def sphere_context(arvx, oracle, sc, N, assoc=1):
    s = F32(0.512 / N)
    ctx = arvx.Context(N, N, N, s, assoc=assoc)
    ctx.set_views(sc.M, sc.masks, campos=sc.campos)
    ctx.set_images(sc.images)
    ctx.upload_state(oracle.carve(N, N, N, s, sc.M, sc.masks))
    ctx.color(arvx.COLOR_AVERAGE)
    return ctx, s


# ---- parity per source ---------------------------------------------------------------------------

@pytest.mark.parametrize("dims,assoc", [((16, 16, 16), 1), ((16, 16, 16), 0), ((33, 17, 9), 1)])
def test_parity_per_source(arvx, oracle, sphere, dims, assoc):
    """carve (the oracle's) -> colour -> the four meshes (decimated with C = 2, refined with B = 2); each
    textured at R = 1 and 4 into an atlas that cw divides and into one with padding and a part-filled
    last row."""
    X, Y, Z = dims
    sc = sphere
    s = F32(0.512 / max(dims))
    left = assoc == 1
    st = oracle.carve(X, Y, Z, s, sc.M, sc.masks)
    with arvx.Context(X, Y, Z, s, assoc=assoc) as ctx:
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images)
        ctx.upload_state(st)
        ctx.color(arvx.COLOR_AVERAGE)
        meshes = build_meshes(arvx, ctx, B=2)
        for name in SOURCES:
            src, verts, rgb, faces = meshes[name]
            T = len(faces)
            assert T > 100 and len(verts) > 50, name
            depth = mcol.depth_buffers(sc.M, s, verts, faces, W, H, left)
            tol = 0.5 * float(s)
            per_row = next(n for n in (15, 14, 13) if ((T + 1) // 2) % n)
            for R in (1, 4):
                for AW in (16 * (R + 3), per_row * (R + 3) + 2):
                    want = mt.texture(sc.M, s, verts, rgb, faces, sc.images, R, AW, tol, assoc_left=left, depth=depth)
                    check(ctx.mesh_texture(src, R, AW, tol), want)
                    assert 0 < want.counts[1] < T and want.atlas.any()
                    if AW % (R + 3):
                        assert ((T + 1) // 2) % want.layout.per_row, "a part-filled last row"
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- an odd number of faces ------------------------------------------------------------------------

def test_odd_number_of_faces(arvx, oracle, sphere):
    sc = sphere
    ctx, s = sphere_context(arvx, oracle, sc, ODD_N)
    with ctx:
        ctx.mc_mesh_welded(False)
        dv, drec, drgb, _, _ = ctx.mc_mesh_decimate(ODD_CELL)
        T = len(drec)
        assert T % 2 == 1
        for R, AW in ((3, 30), (3, 6 * ((T + 1) // 2)), (253, 256)):  # (the last cell ends a row; one cell a row)
            want = mt.texture(sc.M, s, dv, drgb, drec[:, :3], sc.images, R, AW, np.inf)
            got = ctx.mesh_texture(arvx.MESH_DECIMATED, R, AW, np.inf)
            check(got, want)
            i, j = mt.local_texels(R)
            x, y = mt.texel_xy(want.layout, T, i, j)
            assert not got[0][y, x].any() and not got[0][unowned(want.layout)].any()
            assert got[0][mt.texel_xy(want.layout, T - 1, i, j)[::-1]].any()


# ---- occlusion -----------------------------------------------------------------------------------

def test_occlusion_between_two_walls(arvx):
    s, M, images = walls_scene()
    st = walls_state()
    with arvx.Context(WALLS_N, WALLS_N, WALLS_N, s) as ctx:
        ctx.upload_state(st)
        upload_random_colours(ctx, st, 0)
        set_views_without_masks(arvx, ctx, M, W, H)
        ctx.set_images(images)
        verts, faces, _, rgb = ctx.mc_mesh_refined(0, vertex_colors=True)
        f = faces3(faces)
        want = mt.texture(M, s, verts, rgb, f, images, 2, 200, 0.5 * float(s))
        got = ctx.mesh_texture(arvx.MESH_REFINED, 2, 200, 0.5 * float(s))
        check(got, want)
        view = got[1]
        seen = np.flatnonzero(view >= 0)
        # no face takes a view in which one of its corners is hidden ...
        hidden = hidden_pairs(want, f)
        assert hidden.sum() > 0.2 * hidden.size and not hidden[view[seen], seen].any()
        # ... and the far side of the far wall never takes a view that looks through both walls
        far = far_side_pairs(M, s, verts, f)
        assert far.any(axis=0).sum() > 200 and not far[view[seen], seen].any()
        assert (view[far.any(axis=0)] >= 0).sum() > 100
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- faces nobody sees ---------------------------------------------------------------------------

@pytest.mark.parametrize("nv", [1, 2])
def test_faces_nobody_sees(arvx, oracle, sphere, nv):
    sc = sphere
    N = 16
    s = F32(0.512 / N)
    ctx, _ = sphere_context(arvx, oracle, sc, N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        ctx.set_views(sc.M[:nv], sc.masks[:nv], campos=sc.campos[:nv])
        ctx.set_images(sc.images[:nv])
        want = mt.texture(sc.M[:nv], s, verts, rgb, faces, sc.images[:nv], 4, 128, 0.5 * float(s))
        got = ctx.mesh_texture(arvx.MESH_REFINED, 4, 128, 0.5 * float(s))
        check(got, want)
        T, textured = got[3][:2]
        assert 0 < textured < T and textured == np.count_nonzero(got[1] >= 0)
        # an unseen face's texels are step 4's: its corner texels are its corners' colours
        f = faces3(faces)
        unseen = np.flatnonzero(got[1] < 0)
        x, y = mt.texel_xy(want.layout, unseen[:, None], np.array([[0, 4, 0]]), np.array([[0, 0, 4]]))
        assert np.array_equal(got[0][y, x], mt.channel(rgb[f[unseen]])[..., ::-1])


# ---- a tie ---------------------------------------------------------------------------------------

def test_tie_goes_to_the_lower_index(arvx, oracle, sphere):
    sc = sphere
    N = 16
    s = F32(0.512 / N)
    M, masks, images = tie_scene(sc)
    ctx, _ = sphere_context(arvx, oracle, sc, N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        ctx.set_views(M, masks)
        ctx.set_images(images)
        want = mt.texture(M, s, verts, rgb, faces, images, 2, 64, 0.5 * float(s))
        got = ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, 0.5 * float(s))
        check(got, want)
        assert np.count_nonzero(got[1] == 0) > 50 and not (got[1] == 1).any()


# ---- the foreground flag -------------------------------------------------------------------------

def test_foreground_flag(arvx, oracle, sphere):
    sc = sphere
    ctx, s = sphere_context(arvx, oracle, sc, 16)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        args = (sc.M, s, verts, rgb, faces, sc.images, 2, 64, 0.5 * float(s))
        off = mt.texture(*args)
        on = mt.texture(*args, mt.FOREGROUND, sc.masks, depth=off.depth)
        check(ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, 0.5 * float(s)), off)
        check(ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, 0.5 * float(s), arvx.MESH_TEXTURE_FOREGROUND), on)
        assert np.count_nonzero(on.face_view != off.face_view) > 0.05 * len(faces)
        assert ((on.face_view >= 0) & (off.face_view >= 0) & (on.face_view != off.face_view)).any()
        set_views_without_masks(arvx, ctx, sc.M, W, H)
        ctx.set_images(sc.images)
        _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, 0.0, arvx.MESH_TEXTURE_FOREGROUND), ERR_STATE)
        check(ctx.mesh_texture_download() + (ctx.mesh_texture_info(),), on)  # (the refused call left it)
        check(ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, 0.5 * float(s)), off)


# ---- the self-test hooks of the depth pass -------------------------------------------------------

def test_selftest_hooks(arvx):
    """Batches of 1 and 2 views and the default; a list of large boxes with no room and the default: the
    large scene puts most pixel boxes on the list."""
    s, M, _ = large_scene()
    images = syn.pattern_images(LARGE_V, W, H, seed=4)
    ctx, verts, rgb, faces = large_context(arvx, 1)
    with ctx:
        set_views_without_masks(arvx, ctx, M, W, H)
        ctx.set_images(images)
        want = mt.texture(M, s, verts, rgb, faces, images, 4, 64, 0.25 * float(s))
        boxes = rm.render(M[0], s, verts, rgb, faces, W, H).box
        assert np.count_nonzero(boxes > rm.LANE_PIXELS) > 4
        for batch in (1, 2, 0):
            for cap in (0, -1):
                ctx.selftest_mesh_color_batch(batch)
                ctx.selftest_render_mesh_list(cap)
                check(ctx.mesh_texture(arvx.MESH_REFINED, 4, 64, 0.25 * float(s)), want)
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- cameras inside the grid, corners on the image's border --------------------------------------

@pytest.mark.parametrize("assoc", [1, 0])
def test_cameras_inside_the_grid(arvx, assoc):
    s, M, _ = large_scene()
    images = syn.pattern_images(LARGE_V, W, H, seed=4)
    ctx, verts, rgb, faces = large_context(arvx, assoc)
    left = assoc == 1
    with ctx:
        set_views_without_masks(arvx, ctx, M, W, H)
        ctx.set_images(images)
        f = faces3(faces)
        for R in (1, 4):
            want = mt.texture(M, s, verts, rgb, f, images, R, 64, 0.25 * float(s), assoc_left=left)
            got = ctx.mesh_texture(arvx.MESH_REFINED, R, 64, 0.25 * float(s))
            check(got, want)
        behind = np.stack([~rm.project(M[v], s, verts, left).valid for v in range(LARGE_V)])[:, f].any(axis=2)
        seen = np.flatnonzero(got[1] >= 0)
        assert behind.any() and 0 < len(seen) < len(f) and not behind[got[1][seen], seen].any()


def test_corners_on_the_border_of_an_odd_image(arvx):
    X, Y, Z, s, M, st = edge_scene()
    images = noise_image(EDGE_W, EDGE_H)
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.upload_state(st)
        set_views_without_masks(arvx, ctx, M, EDGE_W, EDGE_H)
        ctx.set_images(images)
        verts, faces, _, rgb = ctx.mc_mesh_refined(0, vertex_colors=True)
        f = faces3(faces)
        pr = rm.project(M[0], s, verts)
        last = pr.valid & ((pr.fx == 16 * (EDGE_W - 1)) | (pr.fy == 16 * (EDGE_H - 1)))
        for R in (3, 8):
            want = mt.texture(M, s, verts, rgb, f, images, R, 50, np.inf)
            check(ctx.mesh_texture(arvx.MESH_REFINED, R, 50, np.inf), want)
            assert (last[f].any(axis=1) & (want.face_view == 0)).any() and 0 < want.counts[1] < len(f)
            _, clamped = mt.face_texels(M, s, verts, rgb, f, images, want.face_view, R)
            assert clamped.any()


# ---- drawing --------------------------------------------------------------------------------------

def test_drawing_with_the_texture(arvx, oracle, sphere):
    sc = sphere
    ctx, s = sphere_context(arvx, oracle, sc, 16)
    from tests import scenes
    _, _, extra = scenes.random_cameras(2, 0.512, seed=1, W=97, H=61)
    with ctx:
        meshes = build_meshes(arvx, ctx)
        for name, R in zip(SOURCES, (1, 2, 5, 3)):
            src, verts, rgb, faces = meshes[name]
            got = ctx.mesh_texture(src, R, 40 * (R + 3) + 1, 0.5 * float(s))
            tex = mt.texture(sc.M, s, verts, rgb, faces, sc.images, R, 40 * (R + 3) + 1, 0.5 * float(s))
            check(got, tex)
            bit = src | arvx.MESH_TEXTURED
            for light in (None, arvx.headlight(sc.M[2])):
                want = mt.draw(sc.M[2], s, verts, faces, tex, W, H, light=light)
                drawn = ctx.render_mesh_view(bit, 2, light=light)
                same(drawn, want)
                plain = ctx.render_mesh_view(src, 2, light=light)
                same(plain, rm.render(sc.M[2], s, verts, rgb, faces, W, H, light=light).image)
                assert np.array_equal(bits(drawn[1]), bits(plain[1])) and np.array_equal(drawn[2], plain[2])
                assert (want.id >= 0).any() and not np.array_equal(drawn[0], plain[0])
                same(ctx.render_mesh(bit, extra[1], 97, 61, light=light),
                     mt.draw(extra[1], s, verts, faces, tex, 97, 61, light=light))
            counts = ctx.render_mesh_agreement(src, 1)
            assert ctx.render_mesh_agreement(bit, 1) == counts  # (and it is the current render)
            same(ctx.render_download(), mt.draw(sc.M[1], s, verts, faces, tex, W, H))
            _err(arvx, lambda: ctx.render_mesh_view(bit | arvx.MESH_IMAGE_COLORS, 2), ERR_INVALID)
            check(ctx.mesh_texture_download() + (ctx.mesh_texture_info(),), tex)  # (it outlives the renders)


# ---- the interplay with the mesh colours --------------------------------------------------------

def test_interplay_with_mesh_color(arvx, oracle, sphere):
    sc = sphere
    ctx, s = sphere_context(arvx, oracle, sc, 16)
    tol = 0.5 * float(s)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        depth = mcol.depth_buffers(sc.M, s, verts, faces, W, H)
        col = mcol.color(sc.M, s, verts, rgb, faces, sc.images, arvx.COLOR_AVERAGE, tol, depth=depth)
        tex = mt.texture(sc.M, s, verts, rgb, faces, sc.images, 3, 96, tol, depth=depth)

        def both_intact():
            got_rgb, got_views = ctx.mesh_color_download()
            assert np.array_equal(bits(got_rgb), bits(col.rgb)) and np.array_equal(got_views, col.views)
            check(ctx.mesh_texture_download() + (ctx.mesh_texture_info(),), tex)
            for v in (0, sc.V - 1):
                d = ctx.mesh_color_depth(v)
                assert np.array_equal(bits(d), bits(depth[v]))
                assert np.array_equal(bits(d), bits(ctx.render_mesh_view(arvx.MESH_REFINED, v)[1]))

        ctx.mesh_color(arvx.MESH_REFINED, arvx.COLOR_AVERAGE, tol)
        check(ctx.mesh_texture(arvx.MESH_REFINED, 3, 96, tol), tex)
        both_intact()
        # the texture call used other views' keys?  Texture a different mesh in between: the colours' depth stays
        ctx.mc_mesh_welded(False)
        ctx.mesh_texture(arvx.MESH_WELDED, 1, 64, tol)
        assert np.array_equal(bits(ctx.mesh_color_depth(0)), bits(depth[0]))
        # ... and the reverse order
        check(ctx.mesh_texture(arvx.MESH_REFINED, 3, 96, tol), tex)
        ctx.mesh_color(arvx.MESH_REFINED, arvx.COLOR_AVERAGE, tol)
        both_intact()
        # both drawn from their own products
        same(ctx.render_mesh_view(arvx.MESH_REFINED | arvx.MESH_IMAGE_COLORS, 1),
             rm.render(sc.M[1], s, verts, col.rgb, faces, W, H).image)
        same(ctx.render_mesh_view(arvx.MESH_REFINED | arvx.MESH_TEXTURED, 1), mt.draw(sc.M[1], s, verts, faces, tex, W, H))


# ---- refusals and lifetimes ---------------------------------------------------------------------

def test_refusals_and_lifetimes(arvx, oracle):
    N, V, Wr, Hr = 16, 4, 64, 48
    sc = syn.sphere_scene(N, V, W=Wr, H=Hr, with_images=True)
    s = sc.voxel_size
    tol = float(s)
    st = oracle.carve(N, N, N, s, sc.M, sc.masks)
    lib = arvx.load_library()
    every = (arvx.MESH_WELDED, arvx.MESH_SMOOTHED, arvx.MESH_DECIMATED, arvx.MESH_REFINED)
    BIT = arvx.MESH_TEXTURED
    out4 = (arvx.C.c_int64 * 4)()

    def product(ctx):
        atlas, view, uv = ctx.mesh_texture_download()
        return atlas.tobytes(), view.tobytes(), uv.tobytes(), ctx.mesh_texture_info()

    with arvx.Context(N, N, N, s) as ctx:
        ctx.upload_state(st)
        # no mesh, no views, no images, no product
        for src in every:
            _err(arvx, lambda: ctx.mesh_texture(src, 2, 64, tol), ERR_STATE)
        _err(arvx, lambda: ctx.mesh_texture_download(), ERR_STATE)
        _err(arvx, lambda: ctx.mesh_texture_info(), ERR_STATE)
        wv, wf, _, wrgb = ctx.mc_mesh_welded(False, vertex_colors=True)
        for src in every[1:]:
            _err(arvx, lambda: ctx.mesh_texture(src, 2, 64, tol), ERR_STATE)
        _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol), ERR_STATE)  # no views
        set_views_without_masks(arvx, ctx, sc.M, Wr, Hr)
        _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol), ERR_STATE)  # no images
        ctx.set_images(sc.images)
        _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol, arvx.MESH_TEXTURE_FOREGROUND), ERR_STATE)
        _err(arvx, lambda: ctx.render_mesh(arvx.MESH_WELDED | BIT, sc.M[0], Wr, Hr), ERR_STATE)  # no product
        _err(arvx, lambda: ctx.render_mesh_view(arvx.MESH_WELDED | BIT, 0), ERR_STATE)
        _err(arvx, lambda: ctx.render_mesh_agreement(arvx.MESH_WELDED | BIT, 0), ERR_STATE)
        want = mt.texture(sc.M, s, wv, wrgb, wf, sc.images, 2, 64, tol)
        check(ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol), want)
        first = product(ctx)
        # every refused call leaves that product downloadable
        for src in (-1, 4, BIT, arvx.MESH_WELDED | BIT, arvx.MESH_IMAGE_COLORS):
            _err(arvx, lambda: ctx.mesh_texture(src, 2, 64, tol), ERR_INVALID)
        for R in (0, -1, 254):
            _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, R, 4096, tol), ERR_INVALID)
        for AW in (4, 0, -5, 16385):  # (cw = 5)
            _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 2, AW, tol), ERR_INVALID)
        T = len(wf)
        rows = -(-((T + 1) // 2) // 1)
        assert rows * 102 > 32768  # one cell a row at R = 100: too high
        _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 100, 103, tol), ERR_INVALID)
        for flags in (2, 0x100, 3):
            _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol, flags), ERR_INVALID)
        for bad in (np.nan, -1.0, -np.inf):
            _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, bad), ERR_INVALID)
        assert lib.arvx_mesh_texture(ctx._h, 0, 2, 64, tol, 0, None) == ERR_INVALID
        assert lib.arvx_mesh_texture_info(ctx._h, None) == ERR_INVALID
        _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, tol), ERR_STATE)  # (no such mesh)
        for src in (arvx.MESH_REFINED | BIT, arvx.MESH_SMOOTHED | BIT):  # a mesh that is not there
            _err(arvx, lambda: ctx.render_mesh(src, sc.M[0], Wr, Hr), ERR_STATE)
        for src in (4 | BIT, BIT | arvx.MESH_IMAGE_COLORS, 0x800):
            _err(arvx, lambda: ctx.render_mesh(src, sc.M[0], Wr, Hr), ERR_INVALID)
        assert product(ctx) == first
        assert lib.arvx_mesh_texture_download(ctx._h, None, None, None) == 0  # (any pointer may be null)
        # new views and images, colour calls, arvx_mesh_color and a render keep it; it ends no render
        ctx.set_views(sc.M, sc.masks, campos=sc.campos)
        ctx.set_images(sc.images[::-1])
        ctx.color(arvx.COLOR_CLOSEST)
        ctx.mesh_color(arvx.MESH_WELDED, arvx.COLOR_AVERAGE, tol)
        drawn = ctx.render_mesh(arvx.MESH_WELDED | BIT, sc.M[0], Wr, Hr)
        same(drawn, mt.draw(sc.M[0], s, wv, wf, want, Wr, Hr))
        assert product(ctx) == first
        other = ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol)  # the next call replaces it: the images' order
        assert not np.array_equal(other[0], want.atlas) and product(ctx) != first
        for a, b in zip(drawn, ctx.render_download()):  # ... and keeps the current render
            assert a.tobytes() == b.tobytes()
        ctx.mesh_color_download()  # (and the colours' product)
        ctx.set_images(sc.images)
        # a product of another source is not drawn
        sv, _ = ctx.mc_mesh_smooth(2)
        dv, drec, drgb, _, _ = ctx.mc_mesh_decimate(2)
        rv, rf, _, rrgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        ctx.mesh_texture_info()  # (WELDED: the three calls kept it)
        for src in every[1:]:
            _err(arvx, lambda: ctx.render_mesh(src | BIT, sc.M[0], Wr, Hr), ERR_STATE)
        # SMOOTHED ends at the next smooth, DECIMATED at the next decimate, REFINED at the next refined
        check(ctx.mesh_texture(arvx.MESH_SMOOTHED, 3, 70, tol), mt.texture(sc.M, s, sv, wrgb, wf, sc.images, 3, 70, tol))
        _err(arvx, lambda: ctx.render_mesh(arvx.MESH_WELDED | BIT, sc.M[0], Wr, Hr), ERR_STATE)
        ctx.mc_mesh_decimate(2)
        ctx.mc_mesh_refined(4)
        ctx.render_mesh(arvx.MESH_SMOOTHED | BIT, sc.M[0], Wr, Hr)
        ctx.mc_mesh_smooth(2)
        _err(arvx, lambda: ctx.mesh_texture_download(), ERR_STATE)
        _err(arvx, lambda: ctx.render_mesh(arvx.MESH_SMOOTHED | BIT, sc.M[0], Wr, Hr), ERR_STATE)
        ctx.render_download()  # (the render it was drawn into stays)
        check(ctx.mesh_texture(arvx.MESH_DECIMATED, 3, 70, tol),
              mt.texture(sc.M, s, dv, drgb, drec[:, :3], sc.images, 3, 70, tol))
        ctx.mc_mesh_smooth(1)
        ctx.mc_mesh_refined(4)
        ctx.mesh_texture_download()
        ctx.mc_mesh_decimate(2)
        _err(arvx, lambda: ctx.mesh_texture_info(), ERR_STATE)
        ref = mt.texture(sc.M, s, rv, rrgb, rf, sc.images, 3, 70, tol)
        check(ctx.mesh_texture(arvx.MESH_REFINED, 3, 70, tol), ref)
        kept = product(ctx)
        ctx.carve()  # (a carve has whatever effect it has on the source mesh -- none -- and nothing more)
        assert product(ctx) == kept
        # a new welded mesh keeps a REFINED product; a new refined mesh ends it, and not a WELDED one
        ctx.mc_mesh_welded(False)
        assert product(ctx) == kept
        ctx.mc_mesh_refined(0)
        _err(arvx, lambda: ctx.mesh_texture_download(), ERR_STATE)
        ctx.mesh_texture(arvx.MESH_WELDED, 2, 64, tol)
        kept = product(ctx)
        ctx.mc_mesh_refined(4)
        assert product(ctx) == kept
        ctx.mc_mesh_welded(False)
        _err(arvx, lambda: ctx.mesh_texture_download(), ERR_STATE)
        # an empty mesh gives AH = 0 and empty arrays, and draws the background
        ctx.upload_state(np.full((N, N, N), 2, np.uint8))
        ctx.mc_mesh_refined(0)
        atlas, view, uv, counts = ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, tol)
        assert atlas.shape == (0, 64, 3) and view.shape == (0,) and uv.shape == (0, 3, 2) and counts == (0, 0, 64, 0)
        assert not ctx.render_mesh(arvx.MESH_REFINED | BIT, sc.M[0], Wr, Hr)[0].any()
        assert ctx.stats()["host_total_fallbacks"] == 0
    # slab and striped contexts never have a mesh to texture
    for kw in (dict(z_range=(4, 12)), dict(stripes=(2, 0))):
        with arvx.Context(N, N, N, s, **kw) as ctx:
            ctx.set_views(sc.M, sc.masks, campos=sc.campos)
            for src in every:
                _err(arvx, lambda: ctx.mesh_texture(src, 2, 64, tol), ERR_STATE)
            _err(arvx, lambda: ctx.mesh_texture_download(), ERR_STATE)
