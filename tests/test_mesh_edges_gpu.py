"""arvx_mesh_color and arvx_mesh_texture on the device where their kernels change path, bit for bit against
the numpy restatements (tests/mesh_color.py, tests/mesh_texture.py) fed with the mesh arrays the context
downloads: more than 32 views (a second and third word of view bits per vertex, ties across a word, the
depth pass in batches of 65 views, words left behind by a longer set of views); the foreground flags on
a background plane whose last word is partial, with one view and with 65; the atlas 16384 texels wide
and 32436 high, drawn as well; the one to three texels behind the fill's last whole group of four, over
stale bytes.  The scenes are tests/mesh_edges.py's; what each must hold is asserted on the restatement
alone in tests/test_mesh_edges_cpu.py and repeated here on the meshes the device built."""
import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import mesh_color as mcol
from tests import mesh_edges as me
from tests import mesh_texture as mt
from tests.test_mesh_color_cpu import EDGE_H, EDGE_W, edge_scene, noise_image
from tests.test_mesh_color_gpu import check as check_colours
from tests.test_mesh_texture_gpu import bits, check, sphere_context
from tests.test_render_gpu import _err, same

pytestmark = pytest.mark.gpu
ERR_INVALID = 1  # ARVX_ERR_INVALID (include/arvx/arvx.h)
S, TOL = me.S, me.TOL


@pytest.fixture(scope="module")
def sphere():
    return syn.sphere_scene(32, V=6, W=160, H=120, with_images=True)


def held_texture(ctx):
    return ctx.mesh_texture_download() + (ctx.mesh_texture_info(),)


def parity(arvx, ctx, src, M, masks, images, verts, rgb, faces, left=True, R=2, AW=64, flags=(0, 1)):
    """The texture and the colours in both modes per flag, and three views' depth buffers, against the
    restatements: -> {flag: Texture}."""
    V, (H, W) = len(M), images[0].shape[:2]
    assert arvx.MESH_TEXTURE_FOREGROUND == mt.FOREGROUND and arvx.MESH_COLOR_FOREGROUND == mcol.FOREGROUND
    depth = mcol.depth_buffers(M, S, verts, faces, W, H, left)
    out = {}
    for flag in flags:
        out[flag] = mt.texture(M, S, verts, rgb, faces, images, R, AW, TOL, flag, masks, left, depth)
        check(ctx.mesh_texture(src, R, AW, TOL, flag), out[flag])
        for mode in (arvx.COLOR_CLOSEST, arvx.COLOR_AVERAGE):
            want = mcol.color(M, S, verts, rgb, faces, images, mode, TOL, flag, masks, left, depth)
            check_colours(ctx.mesh_color(src, mode, TOL, flag), want)
            assert 0 < want.coloured
    for v in sorted({0, 31, min(32, V - 1), V - 1}):
        assert np.array_equal(bits(ctx.mesh_color_depth(v)), bits(depth[v])), v
    return out


# ---- A: more than 32 views ------------------------------------------------------------------------

@pytest.mark.parametrize("V,assoc", [(32, 1), (33, 1), (40, 1), (40, 0), (65, 1)])
def test_more_than_32_views(arvx, oracle, V, assoc):
    """The refined mesh (B = 4) of the sphere under V views of 64 x 48; at V = 40 the welded mesh too, in
    both row-sum groupings."""
    sc = me.many_views(V)
    ctx, _ = sphere_context(arvx, oracle, sc, me.N, assoc)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        got = parity(arvx, ctx, arvx.MESH_REFINED, sc.M, sc.masks, sc.images, verts, rgb, faces, assoc == 1)
        me.assert_word_reach(me.word_reach(got[0], V), V)
        assert (got[0].face_view != got[1].face_view).any()
        if V == 40:
            wv, wf, _, wrgb = ctx.mc_mesh_welded(False, vertex_colors=True)
            parity(arvx, ctx, arvx.MESH_WELDED, sc.M, sc.masks, sc.images, wv, wrgb, wf, assoc == 1, R=3, AW=6 * 31 + 2)
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_ties_across_a_word(arvx, oracle):
    """View 3 again as view 35, view 31 again as view 32: the first of equal areas wins, whichever word the
    second one's bit lies in."""
    sc = me.tie_views()
    M, masks, images = sc.M, sc.masks, sc.images
    ctx, _ = sphere_context(arvx, oracle, sc, me.N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        want = parity(arvx, ctx, arvx.MESH_REFINED, M, masks, images, verts, rgb, faces)
        for flag in (0, 1):
            view = ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, TOL, flag)[1]
            for n in (me.faces_per_view(view, 40), me.faces_per_view(want[flag].face_view, 40)):
                assert all(n[a] >= me.TIE_MANY[a] and n[b] == 0 for a, b in me.TIE_PAIRS), n
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_batches_of_65_views(arvx, oracle):
    """The depth pass in launches of 7 views (ten launches, the last of 2), of 32 (the last of 1) and of
    all 65: the same texture, colours and depth buffers each time."""
    V = 65
    sc = me.many_views(V)
    ctx, _ = sphere_context(arvx, oracle, sc, me.N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        assert (64 << 20) // (16 * len(verts)) > V  # (the default bound holds all 65)
        depth = mcol.depth_buffers(sc.M, S, verts, faces, me.MANY_W, me.MANY_H)
        tex = mt.texture(sc.M, S, verts, rgb, faces, sc.images, 2, 64, TOL, depth=depth)
        col = mcol.color(sc.M, S, verts, rgb, faces, sc.images, arvx.COLOR_AVERAGE, TOL, depth=depth)
        for batch in (7, 32, 0):
            ctx.selftest_mesh_color_batch(batch)
            check(ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, TOL), tex)
            check_colours(ctx.mesh_color(arvx.MESH_REFINED, arvx.COLOR_AVERAGE, TOL), col)
            for v in (0, 6, 7, 31, 32, 63, 64):  # (the first and last views of launches of 7 and of 32)
                assert np.array_equal(bits(ctx.mesh_color_depth(v)), bits(depth[v])), (batch, v)
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_words_left_by_a_longer_set_of_views(arvx, oracle):
    """65 views, then the first 33 of them on the same context and mesh: two words per vertex where the
    call before wrote three."""
    sc = me.many_views(65)
    ctx, _ = sphere_context(arvx, oracle, sc, me.N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        full = mt.texture(sc.M, S, verts, rgb, faces, sc.images, 2, 64, TOL)
        check(ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, TOL), full)
        ctx.set_views(sc.M[:33], sc.masks[:33], campos=sc.campos[:33])
        ctx.set_images(sc.images[:33])
        part = mt.texture(sc.M[:33], S, verts, rgb, faces, sc.images[:33], 2, 64, TOL, depth=full.depth[:33])
        assert np.count_nonzero(full.face_view > 32) > 100 and np.count_nonzero(part.face_view == 32) >= 5
        check(ctx.mesh_texture(arvx.MESH_REFINED, 2, 64, TOL), part)
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- B: a plane whose last word is partial ---------------------------------------------------------

def test_flags_on_a_partial_last_word(arvx):
    """97 x 61: 5917 pixels, 29 bits in the plane's last word, and vertices whose nearest pixel lies there on
    either side of the mask."""
    X, Y, Z, s, M, st = edge_scene()
    masks, images = me.edge_masks(), noise_image(EDGE_W, EDGE_H)
    with arvx.Context(X, Y, Z, s) as ctx:
        ctx.upload_state(st)
        ctx.set_views(M, masks)
        ctx.set_images(images)
        verts, faces, _, rgb = ctx.mc_mesh_refined(0, vertex_colors=True)
        fg, bg = me.last_word_vertices(M, s, verts, masks)
        assert fg.sum() >= 2 and bg.sum() >= 2
        args = (M, s, verts, rgb, faces, images)
        depth = mcol.depth_buffers(M, s, verts, faces, EDGE_W, EDGE_H)
        for mode in (arvx.COLOR_CLOSEST, arvx.COLOR_AVERAGE):
            off = mcol.color(*args, mode, np.inf, depth=depth)
            on = mcol.color(*args, mode, np.inf, mcol.FOREGROUND, masks, depth=depth)
            got_off = ctx.mesh_color(arvx.MESH_REFINED, mode, np.inf)
            got_on = ctx.mesh_color(arvx.MESH_REFINED, mode, np.inf, arvx.MESH_COLOR_FOREGROUND)
            check_colours(got_off, off)
            check_colours(got_on, on)
            assert got_off[1][fg | bg].all() and got_on[1][fg].all() and not got_on[1][bg].any()
        for R in (3, 8):
            off = mt.texture(*args, R, 50, np.inf, depth=depth)
            on = mt.texture(*args, R, 50, np.inf, mt.FOREGROUND, masks, depth=depth)
            check(ctx.mesh_texture(arvx.MESH_REFINED, R, 50, np.inf), off)
            got = ctx.mesh_texture(arvx.MESH_REFINED, R, 50, np.inf, arvx.MESH_TEXTURE_FOREGROUND)
            check(got, on)
            changed = np.flatnonzero(got[1] != off.face_view)
            assert bg[np.asarray(faces)[changed, :3].astype(np.int64)].any() and 0 < on.counts[1] < off.counts[1]
        assert ctx.stats()["host_total_fallbacks"] == 0


def test_65_planes_of_an_odd_size(arvx, oracle):
    """65 views of 97 x 61: plane v starts v * bgWords words in, and no plane ends on a whole word."""
    V = 65
    sc = me.many_views(V, EDGE_W, EDGE_H)
    ctx, _ = sphere_context(arvx, oracle, sc, me.N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        got = parity(arvx, ctx, arvx.MESH_REFINED, sc.M, sc.masks, sc.images, verts, rgb, faces)
        me.assert_word_reach(me.word_reach(got[0], V), V)
        dropped = (got[0].visible & ~got[1].visible).any(axis=1)
        assert dropped[:32].any() and dropped[32:].any()
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- C: the atlas at its limits -------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["wide", "tall"])
def test_atlas_at_its_limits(arvx, oracle, sphere, shape):
    """T = 1224.  Wide: R = 26 in 16384 columns, the first row of cells full, 28 padding columns.  Tall:
    R = 51, one cell a row, 32436 rows; R = 52 would need 33048 and is refused."""
    sc = sphere
    ctx, s = sphere_context(arvx, oracle, sc, me.N)
    with ctx:
        verts, faces, _, rgb = ctx.mc_mesh_refined(4, vertex_colors=True)
        T = len(faces)
        R, AW = (me.WIDE_R, me.WIDE_AW) if shape == "wide" else me.tall_geometry(T)
        tex = mt.texture(sc.M, s, verts, rgb, faces, sc.images, R, AW, TOL)
        lay = tex.layout
        nz = me.owned_nonzero(tex)
        if shape == "wide":
            assert lay.AW == mt.AW_MAX and lay.AW % lay.cw and lay.cells > lay.per_row
            assert np.flatnonzero(nz.any(axis=0)).max() >= 16000
        else:
            assert lay.per_row == 1 and mt.AH_MAX - lay.cells < lay.AH <= mt.AH_MAX
            assert nz[lay.AH - lay.ch:].any()
        check(ctx.mesh_texture(arvx.MESH_REFINED, R, AW, TOL), tex)
        if shape == "tall":
            _err(arvx, lambda: ctx.mesh_texture(arvx.MESH_REFINED, R + 1, R + 4, TOL), ERR_INVALID)
            check(held_texture(ctx), tex)  # (the refused call left it)
        bit = arvx.MESH_REFINED | arvx.MESH_TEXTURED
        for v, light in ((2, None), (5, arvx.headlight(sc.M[5]))):
            want = mt.draw(sc.M[v], s, verts, faces, tex, 160, 120, light=light)
            same(ctx.render_mesh_view(bit, v, light=light), want)
            assert (want.id >= 0).any() and want.bgr[want.id >= 0].any()
        check(held_texture(ctx), tex)
        assert ctx.stats()["host_total_fallbacks"] == 0


# ---- D: the tail of the fill ----------------------------------------------------------------------

@pytest.mark.parametrize("residue", sorted(me.TAIL))
def test_tail_of_the_fill_over_stale_bytes(arvx, oracle, sphere, residue):
    """The decimated sphere (cell 3, T = 94) at one geometry per residue of AW * AH mod 4, directly after a
    larger atlas of the same mesh whose bytes are not zero where the tail's texels go."""
    sc = sphere
    geometry, before, _ = me.TAIL[residue]
    ctx, s = sphere_context(arvx, oracle, sc, me.N)
    with ctx:
        ctx.mc_mesh_welded(False)
        dv, drec, drgb, _, _ = ctx.mc_mesh_decimate(me.TAIL_CELL)
        df = drec[:, :3]
        assert len(df) == me.TAIL_T
        depth = mcol.depth_buffers(sc.M, s, dv, df, 160, 120)
        tex, prior = (mt.texture(sc.M, s, dv, drgb, df, sc.images, R, AW, TOL, depth=depth) for R, AW in (geometry, before))
        me.assert_tail(residue, tex, prior)
        if residue == 2:
            assert tex.layout.AW % 4 and len(me.straddling_lanes(tex)) > 0
        check(ctx.mesh_texture(arvx.MESH_DECIMATED, *before, TOL), prior)
        check(ctx.mesh_texture(arvx.MESH_DECIMATED, *geometry, TOL), tex)
        assert ctx.stats()["host_total_fallbacks"] == 0
