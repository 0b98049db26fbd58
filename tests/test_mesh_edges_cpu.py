"""What the scenes of tests/mesh_edges.py must hold, asserted on the restatements alone
(tests/mesh_color.py, tests/mesh_texture.py), so that the device's parity in
tests/test_mesh_edges_gpu.py cannot pass vacuously: faces and vertices on either side of the 32-view
word, ties across it, vertices in the partial last word of a background plane on either side of the
mask, owned texels at the far ends of the widest and the highest atlas, and which of the atlas's last
one to three texels a face owns.  The counts are printed.  No GPU."""
import numpy as np
import pytest

from ar_voxel_project_amd import synthetic as syn
from tests import mesh_color as mcol
from tests import mesh_decimate as md
from tests import mesh_edges as me
from tests import mesh_refine as mr
from tests import mesh_texture as mt
from tests.test_mesh_color_cpu import EDGE_H, EDGE_W, H, W, edge_scene, noise_image, refined_sphere
from tests.test_mesh_texture_cpu import faces_of, unowned, welded

I64 = np.int64
DIMS = (me.N, me.N, me.N)


def textured(M, masks, images, s, mesh, R=2, AW=64, flags=0, depth=None, tol=me.TOL):
    return mt.texture(M, s, mesh["verts"], mesh["vertex_rgb"], faces_of(mesh), images, R, AW, tol, flags, masks,
                      depth=depth)


@pytest.fixture(scope="module")
def sphere():
    return syn.sphere_scene(32, V=6, W=W, H=H, with_images=True)


# ---- A: more than 32 views ------------------------------------------------------------------------

@pytest.mark.parametrize("V,size", [(V, (me.MANY_W, me.MANY_H)) for V in me.MANY_V] + [(65, (EDGE_W, EDGE_H))])
def test_faces_and_vertices_on_both_sides_of_the_word(oracle, V, size):
    """V = 32: 23 faces take view 31.  V = 33 (the last camera lowered): 929 faces below view 32, 71 at it,
    23 take view 31, 10 vertices only view 32 sees, one or more that all 33 see.  V = 40 (T = 1136): 797
    and 191, 19 and 36, 5 vertices only the high views see.  V = 65: 505 and 509, 9 and 26, 14 take view
    64, 52 vertices only the high views see; at 97 x 61: 587 and 581, 16 and 25, 22 take view 64."""
    sc = me.many_views(V, *size)
    s, mesh = refined_sphere(oracle, sc, DIMS)
    assert s == me.S
    tex = textured(sc.M, sc.masks, sc.images, s, mesh)
    reach = me.word_reach(tex, V)
    print(f"V = {V} at {size}: {len(tex.face_view)} faces, {len(mesh['verts'])} vertices, {reach}")
    me.assert_word_reach(reach, V)
    fg = textured(sc.M, sc.masks, sc.images, s, mesh, flags=mt.FOREGROUND, depth=tex.depth)
    assert (fg.face_view != tex.face_view).any()
    dropped = (tex.visible & ~fg.visible).any(axis=1)  # (per view: the flag drops a vertex there)
    assert dropped[:32].any() and (V <= 32 or dropped[32:].any())


def test_a_tie_across_a_word_goes_to_the_lower_index(oracle):
    sc = me.tie_views()
    M, masks, images, s = sc.M, sc.masks, sc.images, me.S
    st = oracle.carve(me.N, me.N, me.N, s, M, masks)
    mesh = mr.refine((st & 1).astype(bool).reshape(DIMS), s, M, masks, 4)
    A = np.abs(mt.areas(M, s, mesh["verts"], faces_of(mesh)))
    for a, b in me.TIE_PAIRS:
        assert np.array_equal(A[a], A[b]) and not np.array_equal(images[a], images[b])
    for flags in (0, mt.FOREGROUND):
        tex = textured(M, masks, images, s, mesh, flags=flags)
        n = me.faces_per_view(tex.face_view, 40)
        print(f"ties, flags {flags}: view 3 {n[3]}, view 31 {n[31]}, view 32 {n[32]}, view 35 {n[35]}")
        assert all(n[a] >= me.TIE_MANY[a] and n[b] == 0 for a, b in me.TIE_PAIRS)
        assert np.array_equal(tex.visible[3], tex.visible[35]) and np.array_equal(tex.visible[31], tex.visible[32])


def test_a_shorter_set_of_views_leaves_words_behind(oracle):
    """The first 33 of the 65 views on the mesh refined under all 65: fewer words per vertex than the call
    before wrote, and faces whose best view was one of the 32 that left."""
    sc = me.many_views(65)
    s, mesh = refined_sphere(oracle, sc, DIMS)
    full = textured(sc.M, sc.masks, sc.images, s, mesh)
    part = textured(sc.M[:33], sc.masks[:33], sc.images[:33], s, mesh)
    assert np.count_nonzero(full.face_view > 32) > 100 and np.count_nonzero(part.face_view == 32) >= 5
    assert np.count_nonzero((full.face_view > 32) & (part.face_view < 0)) > 0


# ---- B: a plane whose last word is partial ---------------------------------------------------------

def test_edge_masks_split_the_vertices_of_the_last_word():
    """Six in-image vertices have their nearest pixel at index 5888 or above; the mask puts four on its
    foreground and two on its background, and the flag takes the latter's only view."""
    X, Y, Z, s, M, st = edge_scene()
    assert EDGE_W * EDGE_H == 5917 and me.EDGE_LAST_WORD == 5888
    mesh = mr.refine((st & 1).astype(bool), s, [], [], 0)
    masks, images = me.edge_masks(), noise_image(EDGE_W, EDGE_H)
    assert masks.shape == (1, EDGE_H, EDGE_W) and masks.dtype == np.uint8
    fg, bg = me.last_word_vertices(M, s, mesh["verts"], masks)
    print(f"edge scene: {len(mesh['verts'])} vertices, in the last word {fg.sum()} foreground, {bg.sum()} background")
    assert fg.sum() >= 2 and bg.sum() >= 2
    args = (M, s, mesh["verts"], mesh["vertex_rgb"], faces_of(mesh), images)
    off = mcol.color(*args, mcol.CLOSEST, np.inf)
    on = mcol.color(*args, mcol.CLOSEST, np.inf, mcol.FOREGROUND, masks, depth=off.depth)
    assert off.views[fg | bg].all() and on.views[fg].all() and not on.views[bg].any()
    for R in (3, 8):
        t_off = mt.texture(*args, R, 50, np.inf, depth=off.depth)
        t_on = mt.texture(*args, R, 50, np.inf, mt.FOREGROUND, masks, depth=off.depth)
        changed = np.flatnonzero(t_on.face_view != t_off.face_view)
        print(f"R = {R}: {len(t_off.face_view)} faces, {t_off.counts[1]} textured, {t_on.counts[1]} with the flag")
        assert len(changed) > 0 and 0 < t_on.counts[1] < t_off.counts[1]
        assert bg[faces_of(mesh)[changed]].any()  # (a face that lost its view to a last-word vertex)
        assert (fg[faces_of(mesh)].any(axis=1) & (t_on.face_view == 0)).any()  # (and one that kept it through one)


# ---- C: the atlas at its limits -------------------------------------------------------------------

def test_wide_and_tall_atlases_are_owned_at_their_far_ends(oracle, sphere):
    """The refined 16^3 sphere has T = 1224 faces, 612 cells.  Wide: R = 26, AW = 16384, 564 cells in the
    first row, 48 in the second, 28 padding columns.  Tall: R = 51, AW = 54, AH = 32436."""
    sc = sphere
    s, mesh = refined_sphere(oracle, sc, DIMS)
    T = len(mesh["faces"])
    assert T == 1224
    wide = textured(sc.M, sc.masks, sc.images, s, mesh, me.WIDE_R, me.WIDE_AW)
    lay = wide.layout
    assert lay.AW == 16384 and lay.AW % lay.cw != 0 and lay.cells > lay.per_row == 564 and lay.AH == 2 * lay.ch
    nz = me.owned_nonzero(wide)
    xs = np.flatnonzero(nz.any(axis=0))
    print(f"wide: {lay.AW} x {lay.AH}, the last non-black column {xs.max()}")
    assert xs.max() == lay.per_row * lay.cw - 1 >= 16000 and not wide.atlas[unowned(lay)].any()
    R, AW = me.tall_geometry(T)
    assert (R, AW) == (51, 54)
    tall = textured(sc.M, sc.masks, sc.images, s, mesh, R, AW, depth=wide.depth)
    lay = tall.layout
    assert lay.per_row == 1 and lay.AH == 32436 > mt.AH_MAX - lay.cells
    assert mt.layout(T, R + 1, R + 4).AH > mt.AH_MAX  # (the next resolution is refused)
    nz = me.owned_nonzero(tall)
    ys = np.flatnonzero(nz.any(axis=1))
    print(f"tall: {lay.AW} x {lay.AH}, the last non-black row {ys.max()}")
    assert ys.max() >= lay.AH - lay.ch > 32000


# ---- D: the tail of the fill ----------------------------------------------------------------------

def tail_mesh(oracle, sc):
    st = oracle.carve(me.N, me.N, me.N, me.S, sc.M, sc.masks)
    wv, wf = welded(oracle, me.N, st)
    d = md.decimate(wv, wf, me.TAIL_CELL)
    return d["verts"], d["records"][:, :3].astype(I64)


def test_tail_texels_per_residue(oracle, sphere):
    """AW * AH mod 4 = 2: both tail texels are a face's; 3: the first two, the third is padding; 1: padding.
    The atlas textured in front of each has no zero byte where the tail is written."""
    sc = sphere
    dv, df = tail_mesh(oracle, sc)
    assert len(df) == me.TAIL_T
    col = np.full_like(dv, 77)
    depth = mcol.depth_buffers(sc.M, me.S, dv, df, W, H)
    for residue, (geometry, before, _) in me.TAIL.items():
        tex, prior = (mt.texture(sc.M, me.S, dv, col, df, sc.images, R, AW, me.TOL, depth=depth)
                      for R, AW in (geometry, before))
        me.assert_tail(residue, tex, prior)
        lanes = me.straddling_lanes(tex)
        print(f"residue {residue}: {tex.layout.AW} x {tex.layout.AH} after {prior.layout.AW} x {prior.layout.AH}, "
              f"{tex.counts[1]} of {me.TAIL_T} textured, {len(lanes)} lanes over a row's end")
        if residue == 2:
            assert tex.layout.AW % 4 != 0 and len(lanes) > 0
