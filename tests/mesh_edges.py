"""The scenes of tests/test_mesh_edges_cpu.py and tests/test_mesh_edges_gpu.py: the mesh colours and
textures (tests/mesh_color.py, tests/mesh_texture.py) where their kernels change path -- more than 32
views, a background plane whose last word is partial, an atlas at its greatest width and height, the
one to three texels behind the last whole group of four.  Cameras, masks, atlas geometries and the
questions both files ask of a restatement's result; nothing here calls the device."""
import numpy as np

from ar_voxel_project_amd import synthetic as syn
from tests import mesh_texture as mt
from tests import render_mesh as rm
from tests.test_mesh_color_cpu import EDGE_H, EDGE_W

F32 = np.float32
N = 16                         # every grid here is 16^3 (the edge scene is its own)
S = F32(0.512 / N)
TOL = 0.5 * float(S)

# ---- A: more than 32 views ------------------------------------------------------------------------

MANY_V = (32, 33, 40, 65)
MANY_W, MANY_H = 64, 48
LOW_LAST_ELEVATION = 18.0      # degrees: the last camera at V = 33 (the ring's even cameras stand at 25)


def many_views(V, W=MANY_W, H=MANY_H):
    """syn.sphere_scene(16, V) at W x H with images.  At V = 33 the ring gives view 32 nothing of its own
    (it stands between views 31 and 0, and every vertex it sees they see): there the last camera is
    lowered to 18 degrees, which leaves it vertices that no other view sees and still some vertex that
    all 33 see."""
    sc = syn.sphere_scene(N, V, W=W, H=H, with_images=True)
    if V != 33:
        return sc
    E = syn.EXTENT
    centre = np.array([E / 2, E / 2, -E / 2])
    az, el = 2.0 * np.pi * (V - 1) / V, np.deg2rad(LOW_LAST_ELEVATION)
    Rt = sc.Rt.copy()
    Rt[V - 1] = syn.look_at_rt(centre + 2.0 * E * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az),
                                                            -np.sin(el)]), centre)
    masks = syn.sphere_masks(sc.K, Rt, centre, 0.35 * E, W, H)
    return syn.Scene(N, syn.compose_m(sc.K, Rt), Rt, masks, sc.voxel_size, sc.images, sc.K)


TIE_PAIRS = ((3, 35), (31, 32))  # (the view, the index it is given again at): one pair across a word, one next to it
TIE_MANY = {3: 15, 31: 20}       # faces each first view must win (the restatement gives view 3 only 16, view 31 22)


def tie_views():
    """The V = 40 scene with view 3 given again as view 35 and view 31 as view 32, masks copied, under
    other images."""
    sc = many_views(40)
    Rt, masks = sc.Rt.copy(), sc.masks.copy()
    for a, b in TIE_PAIRS:
        Rt[b], masks[b] = Rt[a], masks[a]
    images = syn.pattern_images(40, MANY_W, MANY_H, seed=9)
    return syn.Scene(N, syn.compose_m(sc.K, Rt), Rt, masks, sc.voxel_size, images, sc.K)


def faces_per_view(face_view, V):
    fv = np.asarray(face_view)
    return np.bincount(fv[fv >= 0], minlength=V)


def word_reach(tex, V):
    """What a many-view scene holds, from a restatement's Texture: faces that chose a view below 32, at
    or above 32, views 31, 32 and V - 1; vertices VISIBLE only below 32, only at or above, and the most
    views that see one vertex."""
    n = faces_per_view(tex.face_view, V)
    low, high = tex.visible[:32].any(axis=0), tex.visible[32:].any(axis=0)
    return dict(below=int(n[:32].sum()), above=int(n[32:].sum()), v31=int(n[31]), v32=int(n[32]) if V > 32 else 0,
                last=int(n[V - 1]), only_low=int(np.count_nonzero(low & ~high)),
                only_high=int(np.count_nonzero(high & ~low)), most=int(tex.visible.sum(axis=0).max()))


def assert_word_reach(reach, V):
    """The conditions on word_reach's counts, as the CPU file proves them and the GPU file repeats them on
    the mesh the device built."""
    if V == 32:
        assert reach["v31"] >= 10, reach
        return
    assert reach["below"] >= 10 and reach["above"] >= 10, reach
    assert reach["v31"] >= 5 and reach["v32"] >= 5, reach
    assert reach["last"] >= 1 or V != 65, reach
    assert reach["only_high"] >= 1 and reach["only_low"] >= 1 and reach["most"] > 32, reach


# ---- B: a plane whose last word is partial ---------------------------------------------------------

EDGE_LAST_WORD = 32 * ((EDGE_W * EDGE_H) // 32)  # 5888: the first pixel of the 29-bit word


def edge_masks():
    """(1, 61, 97) uint8: seeded, three pixels in ten background (0), the others 255."""
    return np.where(np.random.default_rng(11).random((1, EDGE_H, EDGE_W)) < 0.3, 0, 255).astype(np.uint8)


def last_word_vertices(M, s, verts, masks):
    """-> (fg, bg) bool per vertex: in the image with the nearest pixel in the plane's last word, on the
    mask's foreground and on its background."""
    pr = rm.project(M[0], s, np.asarray(verts, F32).reshape(-1, 3))
    inside = pr.valid & (pr.fx >= 0) & (pr.fx <= 16 * (EDGE_W - 1)) & (pr.fy >= 0) & (pr.fy <= 16 * (EDGE_H - 1))
    cn, rn = np.where(inside, (pr.fx + 8) >> 4, 0), np.where(inside, (pr.fy + 8) >> 4, 0)
    last = inside & (rn * EDGE_W + cn >= EDGE_LAST_WORD)
    fg = masks[0].reshape(EDGE_H, EDGE_W, -1).any(axis=2)[rn, cn]
    return last & fg, last & ~fg


# ---- C: the atlas at its limits -------------------------------------------------------------------

WIDE_R, WIDE_AW = 26, mt.AW_MAX  # cw = 29: 564 cells a row (612 cells fill one), 28 padding columns


def tall_geometry(T):
    """(R, AW) of the highest atlas with one cell a row that arvx_mesh_texture accepts for T faces."""
    R = mt.AH_MAX // ((T + 1) // 2) - 2
    return R, R + 3


def owned_nonzero(tex):
    """(AH, AW) bool: the texel belongs to a face and is not black in the restatement."""
    lay = tex.layout
    owner = np.zeros((lay.AH, lay.AW), bool)
    i, j = mt.local_texels(lay.R)
    x, y = mt.texel_xy(lay, np.arange(lay.T)[:, None], i[None, :], j[None, :])
    owner[y, x] = True
    return owner & tex.atlas.any(axis=2)


# ---- D: the tail of the fill ----------------------------------------------------------------------
# The 16^3 sphere's welded mesh decimated with cell 3 has T = 94 faces: 47 cells, an odd number, and T
# even.  Per residue of AW * AH mod 4 the geometry (R, AW), and in front of it the geometry whose atlas is
# at least as large and whose bytes are not zero where the tail's will be written.

TAIL_CELL, TAIL_T = 3, 94
TAIL = {
    # residue: ((R, AW), (the R, AW textured directly before), the tail texels that a face owns)
    2: ((3, 282), (4, 42), (True, True)),            # 47 cells a row, no padding: 282 x 5
    3: ((5, 377), (6, 54), (True, True, False)),    # 47 cells a row and one padding column: 377 x 7
    1: ((5, 9), (7, 40), (False,)),                 # one cell a row and one padding column: 9 x 329
}


def tail_texels(lay):
    """(y, x) of the AW * AH mod 4 texels behind the last whole group of four."""
    ntex = lay.AW * lay.AH
    flat = np.arange(ntex - ntex % 4, ntex)
    return flat // lay.AW, flat % lay.AW


def assert_tail(residue, tex, before):
    """tex: the restatement at TAIL[residue]'s geometry, before: at the geometry textured in front of it."""
    owned = TAIL[residue][2]
    lay = tex.layout
    ntex = lay.AW * lay.AH
    assert lay.T % 2 == 0 and lay.cells % lay.per_row == 0 and ntex % 4 == residue == len(owned)
    assert residue != 2 or (lay.cells % 2 == 1 and lay.AW == lay.per_row * lay.cw)  # (an exact fit of an odd number)
    y, x = tail_texels(lay)
    assert np.array_equal(owned_nonzero(tex)[y, x], owned) and not tex.atlas[y, x][~np.array(owned)].any()
    stale = before.atlas.reshape(-1)
    assert len(stale) >= 3 * ntex and stale[3 * ntex - 16:3 * ntex].all()  # (stale bytes where the tail goes ...)
    assert (stale[3 * (ntex - residue):3 * ntex].reshape(-1, 3) != tex.atlas[y, x]).any(axis=1).all()  # (... not the tail's)


def straddling_lanes(tex):
    """The lanes of the fill whose four texels lie in two atlas rows with a face's non-black texel on
    either side of the row's end."""
    lay = tex.layout
    ok = owned_nonzero(tex).reshape(-1)
    first = 4 * np.arange(lay.AW * lay.AH // 4)
    row = (first[:, None] + np.arange(4)) // lay.AW
    two = row[:, 0] != row[:, 3]
    here = (ok[first[:, None] + np.arange(4)] & (row == row[:, :1])).any(axis=1)
    there = (ok[first[:, None] + np.arange(4)] & (row != row[:, :1])).any(axis=1)
    return np.flatnonzero(two & here & there)
