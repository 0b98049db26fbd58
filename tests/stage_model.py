"""Reference state machines for sequences of calls (test infrastructure, plain numpy over
oracle/pyoracle.py).

CtxModel restates what include/arvx/arvx.h promises for a whole-grid context, call by call:
the state bytes (bit0 occupied, bit1 seen, bit2 painted UNSEEN_COLOR), the colour list, the
closure list and the flags that decide refusals (ARVX_ERR_STATE).  HostModel is the reference's
own Model (src/Model.{h,cpp}): RGBA per voxel plus the seen bits, on which carve, the colour
passes, handleUnseen and applyClosure act as in src/VoxelCarving.cpp, src/ColorReconstruction.h
and src/Postprocessing3d.cpp.  replay() runs a recorded list of operations on a CtxModel and on
something with the same methods (the device context's driver in tests/test_stage_sequences_gpu.py),
so that any failing sequence can be pinned as a plain list.

The stages beyond the reference's pipeline are restated too, each from its section of arvx.h and
"What the context's results belong to" there, on top of the numpy restatements the stages' own tests
use: the vote carve (tests/vote_carve.py) and its counts, photo-consistency carving
(tests/photo_carve.py), the components' labelling and arvx_components_keep (tests/components.py), the
distance field and arvx_morph (tests/distance.py).  The vote counts, the labelling and the field are
results of the context like the colour and closure lists: CtxModel holds them for as long as arvx.h
says they live, and their downloads are refused before and after.

So are the products: the cell list, the unwelded, welded, smoothed, decimated and refined meshes, the
render of the welded mesh and the visible colour pass, each on the numpy restatement its own tests
use (tests/mesh_weld.py, mesh_smooth.py, mesh_decimate.py, mesh_refine.py, render.py,
visibility.py).  A product is BUILT by a call (mc_cells_build, mc_mesh_build, weld, smooth, decimate,
refine, render / render_view / render_agreement, color_visible) and held from then on until arvx.h
says it ends; its download (mc_cells_list, mc_mesh_held, welded_held, smooth_held, decimate_held,
refined_held, render_held, surface_visible, view_depth) is an observation of its own that builds
nothing, so that a sequence can ask for a product after other calls have run.  Not restated:
arvx_ctx_set_projection_assoc."""
import numpy as np

from tests import (components, distance, mesh_decimate, mesh_refine, mesh_smooth, mesh_weld, occ_codec,
                   photo_carve, vote_carve)
from tests import render as render_np
from tests import visibility

OCC, SEEN, PAINT = 1, 2, 4
MODEL_COLOR = np.array([50, 168, 141, 1], np.float32)
UNSEEN_COLOR = np.array([204, 0, 0, 1], np.float32)


class Refused(Exception):
    """The C-ABI answers ARVX_ERR_STATE for this call in this state."""


def closure_any_kernel(model, X, Y, Z, ksize):
    """numpy restatement of applyClosure for any odd kernel size (the oracle's C
    version is the literal 3x3x3 one): mean RGBA of the occupied neighbours, summed in
    the reference's x, y, z offset order in fp32."""
    r = (ksize - 1) // 2
    m = np.asarray(model, np.float32).reshape(Z, Y, X, 4)
    occ = m[..., 3] != 0
    out = m.copy()
    pad = np.zeros((Z + 2 * r, Y + 2 * r, X + 2 * r, 4), np.float32)
    pad[r:r + Z, r:r + Y, r:r + X] = np.where(occ[..., None], m, 0)
    pocc = np.zeros((Z + 2 * r, Y + 2 * r, X + 2 * r), np.float32)
    pocc[r:r + Z, r:r + Y, r:r + X] = occ
    acc = np.zeros((Z, Y, X, 4), np.float32)
    cnt = np.zeros((Z, Y, X), np.float32)
    for a in range(-r, r + 1):          # x offset outermost (src/Postprocessing3d.cpp:31-48)
        for b in range(-r, r + 1):
            for c in range(-r, r + 1):
                sl = (slice(r + c, r + c + Z), slice(r + b, r + b + Y), slice(r + a, r + a + X))
                acc = (acc + pad[sl]).astype(np.float32)
                cnt += pocc[sl]
    fill = (~occ) & (cnt > 0)
    out[fill] = (acc[fill] / cnt[fill][:, None]).astype(np.float32)
    return out.reshape(-1, 4)


def row_planes(bits, X, Y, Z):
    """(Z*Y*X,) bool -> the bit plane with rows padded to 32-bit words (arvx_state_download_planes)."""
    wpr = (X + 31) // 32
    b = np.zeros((Z, Y, wpr * 32), np.uint8)
    b[..., :X] = np.asarray(bits, bool).reshape(Z, Y, X)
    return np.packbits(b, axis=-1, bitorder="little").view(np.uint32).reshape(-1)


def planes_to_bits(plane, X, Y, Z):
    wpr = (X + 31) // 32
    u8 = np.ascontiguousarray(plane, np.uint32).view(np.uint8).reshape(Z, Y, wpr * 4)
    return np.unpackbits(u8, axis=-1, bitorder="little")[..., :X].reshape(-1).astype(bool)


def decode_packet(pk, n, need):
    """A state packet (arvx_state_download_packets) -> its n 64-bit words; checks the header
    (mixed-word count and the per-group offsets) on the way."""
    pk = np.asarray(pk, np.uint64)
    nb = (n + 63) // 64
    H = occ_codec.header_words(n)
    ones = np.unpackbits(pk[1:1 + nb].view(np.uint8), bitorder="little")[:n].astype(bool)
    mixed = np.unpackbits(pk[1 + nb:1 + 2 * nb].view(np.uint8), bitorder="little")[:n].astype(bool)
    assert int(pk[0]) == need == int(mixed.sum()), (int(pk[0]), need, int(mixed.sum()))
    per_group = np.add.reduceat(np.pad(mixed, (0, nb * 64 - n)).astype(np.int64), np.arange(0, nb * 64, 64))
    offs = np.concatenate([[0], np.cumsum(per_group)[:-1]]).astype(np.uint32)
    assert np.array_equal(pk[1 + 2 * nb:H].view(np.uint32)[:nb], offs)
    w = np.zeros(n, np.uint64)
    w[ones] = occ_codec.ONES
    w[mixed] = pk[H:H + need]
    return w


def flat_words64(bits):
    """(N,) bool, N a multiple of 64 -> N / 64 words, bit i % 64 of word i / 64 = voxel i."""
    return np.packbits(np.asarray(bits, np.uint8), bitorder="little").view(np.uint64)


class Scene:
    """Views, masks and images of one test, and the oracle to carve and colour with."""

    def __init__(self, oracle, X, Y, Z, s, M, campos, masks, images):
        self.oracle, self.X, self.Y, self.Z, self.s = oracle, X, Y, Z, np.float32(s)
        self.M, self.campos, self.masks, self.images = M, campos, masks, images


def make_scene(oracle, X, Y, Z, seed, V=8, W=96, H=72):
    """Random cameras and noise masks (tests/scenes.py) over an X x Y x Z grid, so that coarse
    tiles get every code: views 0 and 1 also have a wide background band (whole tiles carved and
    seen), and some cameras miss parts of the grid (tiles never seen)."""
    from tests import scenes
    s = np.float32(0.512 / max(X, Y, Z))
    base = scenes.syn.sphere_scene(32, V, W=W, H=H, with_images=True)
    # the sphere's cameras leave parts of the grid unseen; random cameras mixed in see it from
    # anywhere, and noise punches background holes into every mask
    _, Rt2, M2 = scenes.random_cameras(V, 0.512, seed=seed, W=W, H=H)
    Rt = np.ascontiguousarray(np.where(np.arange(V)[:, None, None] % 3 == 2, Rt2, base.Rt), np.float32)
    M = np.ascontiguousarray(np.where(np.arange(V)[:, None, None] % 3 == 2, M2, base.M), np.float32)
    noise = scenes.noise_masks(V, H, W, p_bg=0.04, block=3, seed=seed)
    masks = np.where(np.arange(V)[:, None, None] % 3 == 2, noise, base.masks * (noise != 0)).astype(np.uint8)
    masks[0, :, : W // 4] = 0
    rng = np.random.default_rng(seed + 1)
    images = rng.integers(0, 256, size=(V, H, W, 3), dtype=np.uint8)
    sc = Scene(oracle, X, Y, Z, s, M, np.ascontiguousarray(Rt[:, :, 3]), masks, images)
    sc.K = base.K
    sc.Rt = Rt
    return sc


def random_state(seed, X, Y, Z, paint=True, empty_paint=False):
    """Blocky random state bytes; bit2 (painted UNSEEN_COLOR) only on occupied voxels, as a host
    Model's handleUnseen leaves it -- with empty_paint, on some empty voxels as well."""
    rng = np.random.default_rng(seed)
    b = 4
    coarse = rng.random((3, (Z + b - 1) // b, (Y + b - 1) // b, (X + b - 1) // b))
    up = np.repeat(np.repeat(np.repeat(coarse, b, 1), b, 2), b, 3)[:, :Z, :Y, :X]
    fine = rng.random((3, Z, Y, X))
    occ = np.where(up[0] < 0.5, fine[0] < 0.9, fine[0] < 0.1)
    seen = np.where(up[1] < 0.5, fine[1] < 0.95, fine[1] < 0.2)
    st = (occ * OCC | seen * SEEN).astype(np.uint8)
    if paint:
        st |= ((up[2] < 0.3) & (occ | (empty_paint & (fine[2] < 0.2))) & (fine[2] < 0.7)).astype(np.uint8) * PAINT
    return st.reshape(-1)


class CtxModel:
    """What arvx.h says a whole-grid context holds after each call.  Views are given as index
    ranges into a Scene's view set (set_views(lo, hi): views lo..hi-1)."""

    def __init__(self, scene):
        self.sc = scene
        X, Y, Z = scene.X, scene.Y, scene.Z
        self.N = X * Y * Z
        self.st = np.full(self.N, OCC, np.uint8)  # a fresh model: occupied, unseen
        self.paint = None      # bool plane (bit2 of an upload), None: none
        self.views = None      # (lo, hi) into the scene's views
        self.images = False
        self.colors = None     # (index, rgb) of the voxels the colour list colours
        self.clo = None        # (index, rgba, apply_unseen) of the closure's list
        self.fills = False     # the state holds an earlier closure's fills
        self.counts = None     # (background, inside) of a vote carve that kept its counts
        self.comp = None       # per-voxel labels of the last components()
        self.field = None      # [occupancy bytes, border_occupied, the field once somebody asked] of distance()
        # the products, each None until its first build
        self.cells = None      # the cell list of the last arvx_mc_cells / mesh that ran it
        self.mesh = None       # (verts, face_rgb) of the last arvx_mc_mesh
        self.welded = None     # dict of the last arvx_mc_mesh_welded: verts, faces, face_rgb, vrgb, index
        self.smoothed = None   # (positions, normals) of the last smooth on self.welded
        self.decimated = None  # the five arrays of the last decimate on self.welded
        self.refined = None    # the five arrays of the last arvx_mc_mesh_refined, and its silhouette flags
        self.rendered = None   # render.Rendered of the last render of self.welded
        self.visible = None    # (the colour list it filled, visible-view counts, depth buffers)

    RENDER_SIZES = [(96, 72), (50, 37)]  # (the views' size and one that is not)

    def render_camera(self, cam, size):
        """Camera `cam` of the render cameras -- random ones, none of them a view of the scene --
        for image size RENDER_SIZES[size]."""
        from tests import scenes
        sc = self.sc
        cams = getattr(sc, "render_cams", None)
        if cams is None:
            cams = sc.render_cams = {}
        if size not in cams:
            W, H = self.RENDER_SIZES[size]
            cams[size] = np.ascontiguousarray(scenes.random_cameras(4, 0.512, seed=977 + size, W=W, H=H)[2],
                                              np.float32)
        return cams[size][cam]

    def resolve(self, name, args):
        """Concrete arguments of an operation recorded with a seed: ("upload_state", seed),
        ("upload_planes", seed), ("upload_colors", seed) -- colours for a random part of the
        voxels occupied right now."""
        sc = self.sc
        if name == "upload_state":  # (seed[, empty_paint])
            return (random_state(args[0], sc.X, sc.Y, sc.Z, empty_paint=bool(args[1:] and args[1])),)
        if name == "upload_planes":
            st = random_state(args[0], sc.X, sc.Y, sc.Z, paint=False)
            return (row_planes(st & OCC, sc.X, sc.Y, sc.Z), row_planes(st & SEEN, sc.X, sc.Y, sc.Z))
        if name == "upload_colors":
            rng = np.random.default_rng(args[0])
            occ = np.flatnonzero(self.st & OCC)
            idx = occ[rng.random(len(occ)) < 0.4]
            return idx, rng.integers(0, 256, size=(len(idx), 3)).astype(np.float32)
        if name == "render":  # (camera, size, background seed or None) -> (M, W, H, background)
            cam, size, bg = args
            W, H = self.RENDER_SIZES[size]
            back = None if bg is None else \
                np.random.default_rng(bg).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
            return self.render_camera(cam, size), W, H, back
        return args

    # ---- calls ----------------------------------------------------------------------------
    def _state_results_gone(self):
        """The vote counts, the labelling and the field describe the state they were taken from:
        every call that replaces it ends them (arvx.h: arvx_carve_votes, arvx_components,
        arvx_distance)."""
        self.counts = None
        self.comp = None
        self.field = None

    def _state_changes(self, keep_paint=False):
        self.colors = None
        self.clo = None
        self.fills = False
        if not keep_paint:
            self.paint = None
        self._state_results_gone()
        # arvx.h, the render: it "lives until ... a call that replaces the state the mesh was built
        # from"; every caller of this method is in that list, handleUnseen and the closure are not
        self.rendered = None

    def _fills_ok(self):
        if self.fills and self.clo is None:
            raise Refused("the closure's fills have lost their colours")

    def set_views(self, lo, hi):
        self.views = (lo, hi)
        self.images = False
        self.colors = None
        self.clo = None
        self.counts = None  # (they are sums over the views)

    def set_images(self):
        if self.views is None:
            raise Refused("set_images before set_views")
        self.images = True
        self.colors = None
        self.clo = None

    def _v(self, first=0, count=None):
        lo, hi = self.views
        count = hi - lo - first if count is None else count
        return slice(lo + first, lo + first + count)

    def carve(self, first=0, count=None):
        if self.views is None:
            raise Refused("carve before set_views")
        sc, v = self.sc, self._v(first, count)
        st = sc.oracle.carve(sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.masks[v], state=self.st & 3)
        self._state_changes()
        self.st = st.reshape(-1)

    def fast_carve(self):
        if self.views is None:
            raise Refused("fast_carve before set_views")
        sc, v = self.sc, self._v()
        st = sc.oracle.fast_carve(sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.masks[v], state=self.st & 3)
        self._state_changes()
        self.st = st.reshape(-1)

    def carve_votes(self, max_misses, counts):
        """arvx_carve_votes(max_misses, ARVX_VOTES_COUNTS iff counts): a carve as far as the other
        results go."""
        if self.views is None:
            raise Refused("carve_votes before set_views")
        sc, v = self.sc, self._v()
        st, votes = vote_carve.carve_votes(sc.oracle, sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.masks[v],
                                           max_misses, state=self.st & 3)
        self._state_changes()
        self.st = st.reshape(-1)
        if counts:
            self.counts = (votes.background, votes.inside)

    def photo_carve(self, max_std, min_views, tol_voxels, max_iterations):
        """arvx_photo_carve with a tolerance of tol_voxels voxel edges (0 and inf are allowed)
        -> (iterations, removed)."""
        if self.views is None or not self.images:
            raise Refused("photo_carve without views / images")
        self._fills_ok()
        sc, v = self.sc, self._v()
        ph = photo_carve.photo_carve(sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.images[v], self.st & 3, max_std,
                                     min_views, np.float32(tol_voxels) * sc.s, max_iterations)
        self._state_changes()  # (even when nothing was removed)
        self.st = ph.state
        return ph.iterations, ph.removed

    def components(self, connectivity):
        """arvx_components -> the number of components; the labelling stays for the two downloads."""
        sc = self.sc
        self.comp = components.labels(self.st, (sc.X, sc.Y, sc.Z), connectivity)
        return len(components.table(self.comp)[0])

    def keep_components(self, connectivity, min_voxels, largest):
        """arvx_components_keep -> (components kept, voxels removed)."""
        self._fills_ok()
        sc = self.sc
        st, kept, removed = components.keep(self.st & 3, (sc.X, sc.Y, sc.Z), connectivity, min_voxels,
                                            bool(largest))
        self._state_changes()  # (the labelling of an earlier components() with it: none is left)
        self.st = st
        return kept, removed

    def distance(self, border_occupied):
        """arvx_distance.  (The field itself is worked out when distance_field asks for it: until
        then no call can have changed the occupancy without dropping it.)"""
        self.field = [(self.st & OCC).copy(), bool(border_occupied), None]

    def morph(self, op, radius_sq):
        """arvx_morph -> (removed, added)."""
        self._fills_ok()
        sc = self.sc
        st, removed, added = distance.morph(self.st & 3, (sc.X, sc.Y, sc.Z), op, radius_sq)
        self._state_changes()  # (even for a radius of 0; no field is left)
        self.st = st
        return removed, added

    def color(self, mode):
        if self.views is None or not self.images:
            raise Refused("color without views / images")
        sc, v = self.sc, self._v()
        # which voxels the pass colours: every occupied surface voxel with a sample.  A sentinel
        # colour no pixel can produce marks the ones it left alone.
        base = np.zeros((self.N, 4), np.float32)
        base[(self.st & OCC) != 0] = (-1, -1, -1, 1)
        out = sc.oracle.color(sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.campos[v], sc.images[v], mode, base)
        idx = np.flatnonzero(((self.st & OCC) != 0) & (out[:, 0] >= 0))
        self.colors = (idx, out[idx, :3].copy())
        self.clo = None

    def upload_colors(self, index, rgb):
        self.colors = (np.asarray(index, np.int64), np.asarray(rgb, np.float32).reshape(-1, 3))
        self.clo = None

    def handle_unseen(self):
        self.st = self.st | ((self.st & SEEN) == 0).astype(np.uint8)
        self.clo = None
        self._state_results_gone()

    def painted(self, apply_unseen):
        p = np.zeros(self.N, bool) if self.paint is None else self.paint.copy()
        if apply_unseen:
            p |= (self.st & SEEN) == 0
        return p

    def _model(self, apply_unseen, with_closure=True):
        out = np.zeros((self.N, 4), np.float32)
        out[(self.st & OCC) != 0] = MODEL_COLOR
        painted = self.painted(apply_unseen)
        out[painted] = UNSEEN_COLOR
        if self.colors is not None:
            idx, rgb = self.colors
            keep = ~painted[idx]
            out[idx[keep], :3] = rgb[keep]
            out[idx[keep], 3] = 1
        if with_closure and self.clo is not None:
            out[self.clo[0]] = self.clo[1]
        return out

    def closure(self, k, apply_unseen):
        if self.clo is not None or self.fills:
            raise Refused("closure already applied to this model state")
        sc = self.sc
        before = self._model(apply_unseen, with_closure=False)
        after = closure_any_kernel(before, sc.X, sc.Y, sc.Z, k)
        idx = np.flatnonzero((after[:, 3] != 0) & (before[:, 3] == 0))
        self.st = self.st.copy()
        self.st[idx] |= OCC
        self.clo = (idx, after[idx].copy(), bool(apply_unseen))
        self.fills = len(idx) > 0
        # arvx.h names the closure among the calls that end the three results, whatever it fills
        self._state_results_gone()

    def upload_state(self, state):
        state = np.asarray(state, np.uint8).reshape(-1)
        self._state_changes()
        self.st = state & 3
        p = (state & PAINT) != 0
        self.paint = p if p.any() else None

    def upload_planes(self, occ, seen):
        sc = self.sc
        self._state_changes()
        self.st = (planes_to_bits(occ, sc.X, sc.Y, sc.Z) * OCC |
                   planes_to_bits(seen, sc.X, sc.Y, sc.Z) * SEEN).astype(np.uint8)

    def reset(self):
        self._state_changes()
        self.st = np.full(self.N, OCC, np.uint8)

    # ---- observations ---------------------------------------------------------------------
    def download_state(self):
        return self.st | (self.painted(False) * PAINT).astype(np.uint8)

    def download_planes(self):
        sc = self.sc
        return (row_planes(self.st & OCC, sc.X, sc.Y, sc.Z), row_planes(self.st & SEEN, sc.X, sc.Y, sc.Z))

    def download_packets(self):
        """(occupancy words, seen words) as 64-bit flat words (X % 32 == 0, X * Y % 64 == 0)."""
        return flat_words64(self.st & OCC), flat_words64(self.st & SEEN)

    def _flag_ok(self, apply_unseen):
        self._fills_ok()
        if self.clo is not None and bool(apply_unseen) != self.clo[2]:
            raise Refused("closure computed with the other apply_unseen")

    def export_model(self, apply_unseen):
        self._flag_ok(apply_unseen)
        return self._model(apply_unseen)

    def surface(self):
        if self.colors is None:
            raise Refused("no colour result")
        return self.colors

    def closure_list(self):
        if self.clo is None:
            raise Refused("no closure result")
        return self.clo[0], self.clo[1]

    def votes(self):
        if self.counts is None:
            raise Refused("no vote counts")
        return self.counts

    def component_table(self):
        if self.comp is None:
            raise Refused("no labelling")
        return components.table(self.comp)

    def component_labels(self):
        if self.comp is None:
            raise Refused("no labelling")
        return self.comp

    def distance_field(self):
        """arvx_distance_download alone: the field of the last distance()."""
        if self.field is None:
            raise Refused("no distance field")
        sc = self.sc
        if self.field[2] is None:
            self.field[2] = distance.signed_sq(self.field[0], (sc.X, sc.Y, sc.Z), self.field[1])
        return self.field[2]

    def _cells_now(self):
        """The cell list of the occupancy as it is now -- worked out when mc_cells_list asks for it,
        from the occupancy kept here (as distance() does with its field)."""
        return [np.packbits((self.st & OCC).astype(bool)), None]

    def mc_cells(self):
        """arvx_mc_cells and its download at once."""
        self.mc_cells_build()
        return self.mc_cells_list()

    def mc_model(self, apply_unseen):
        """The model the meshes are built from: the state's occupancy in export_model's colours."""
        self._flag_ok(apply_unseen)
        m = self._model(apply_unseen)
        m[(self.st & OCC) == 0] = 0
        return m

    def mc_mesh(self, apply_unseen):
        """arvx_mc_mesh and its download at once."""
        self.mc_mesh_build(apply_unseen)
        return self.mc_mesh_held()

    def mc_mesh_welded(self, apply_unseen):
        """arvx_mc_mesh_welded and its download (without the vertex colours) at once."""
        self.weld(apply_unseen)
        return self.welded_held()[:3]

    # ---- the products: builds ---------------------------------------------------------------
    def mc_cells_build(self):
        """arvx_mc_cells -> the number of cells.  The list is a function of the occupancy at the
        call; no later call but the next cell walk touches it."""
        self.cells = self._cells_now()
        return len(self.mc_cells_list())

    def mc_mesh_build(self, apply_unseen):
        """arvx_mc_mesh -> T.  "Runs arvx_mc_cells itself"."""
        sc = self.sc
        model = self.mc_model(apply_unseen)  # (the refusals)
        self.mesh = sc.oracle.mc_mesh(sc.X, sc.Y, sc.Z, model)
        self.cells = self._cells_now()
        return len(self.mesh[1])

    def weld(self, apply_unseen):
        """arvx_mc_mesh_welded -> (V, T).  A new welded mesh ends the smoothed and the decimated
        mesh and the render of the old one; a refused call leaves all of them."""
        sc = self.sc
        model = self.mc_model(apply_unseen)
        verts, faces, face_rgb = mesh_weld.weld(*sc.oracle.mc_mesh(sc.X, sc.Y, sc.Z, model))
        index = mesh_weld.lattice_index(verts, sc.X, sc.Y)
        self.welded = dict(verts=verts, faces=faces, face_rgb=face_rgb, index=index,
                           vrgb=np.ascontiguousarray(model[index, :3]), nbr=None, inc=None)
        self.cells = self._cells_now()
        self.smoothed = self.decimated = self.rendered = None
        return len(verts), len(faces)

    def smooth(self, iterations, lam, mu):
        """arvx_mc_mesh_smooth on the last welded mesh; the neighbour and incidence structures are
        the mesh's and are kept with it."""
        w = self.welded
        if w is None:
            raise Refused("no welded mesh")
        V = len(w["verts"])
        if w["nbr"] is None:
            w["nbr"] = mesh_smooth.neighbours(V, w["faces"])
            w["inc"] = mesh_smooth.incidences(V, w["faces"])
        self.smoothed = mesh_smooth.smooth(w["verts"], w["faces"], iterations, lam, mu, w["nbr"], w["inc"])

    def decimate(self, cell, source):
        """arvx_mc_mesh_decimate(cell, source: 0 LATTICE, 1 SMOOTHED) -> (Vd, Td)."""
        w = self.welded
        if w is None:
            raise Refused("no welded mesh")
        if source == 1 and self.smoothed is None:
            raise Refused("no smoothed mesh on this welded mesh")
        records = np.concatenate([w["faces"], w["face_rgb"]], axis=1).astype(np.uint32).reshape(-1, 6)
        d = mesh_decimate.decimate(w["verts"], records, cell, self.smoothed[0] if source == 1 else None, w["vrgb"])
        self.decimated = (d["verts"], d["records"].reshape(-1, 6), d["rgb"], d["members"], d["map"])
        return len(d["verts"]), len(d["records"])

    def refine(self, bisections, apply_unseen):
        """arvx_mc_mesh_refined -> (Vr, T): a snapshot of the state and the views at the call."""
        sc = self.sc
        if bisections > 0 and self.views is None:
            raise Refused("the bisection needs views")
        model = self.mc_model(apply_unseen)
        occ = ((self.st & OCC) != 0).reshape(sc.Z, sc.Y, sc.X)
        v = self._v() if self.views is not None else slice(0, 0)
        r = mesh_refine.refine(occ, sc.s, sc.M[v], sc.masks[v], bisections,
                               rgb=model[:, :3].reshape(sc.Z, sc.Y, sc.X, 3))
        records = np.concatenate([r["faces"], r["face_rgb"]], axis=1).astype(np.uint32).reshape(-1, 6)
        self.refined = (r["verts"], records, r["vertex_rgb"], r["edges"], r["cut"], r["silhouette"])
        self.cells = self._cells_now()
        return len(r["verts"]), len(records)

    def _render(self, M, W, H, background):
        w, sc = self.welded, self.sc
        if w is None:
            raise Refused("no welded mesh")
        # the held mesh with the colours it was built with, whatever the state is by now
        self.rendered = render_np.render(M, sc.s, w["index"], w["vrgb"], sc.X, sc.Y, W, H, background)

    def render(self, M, W, H, background):
        self._render(M, W, H, background)

    def _view_camera(self, view):
        if self.welded is None:
            raise Refused("no welded mesh")
        if self.views is None:
            raise Refused("render_view without views")
        sc = self.sc
        k = self.views[0] + view
        return k, sc.M[k], sc.masks.shape[2], sc.masks.shape[1]

    def render_view(self, view):
        _, M, W, H = self._view_camera(view)
        self._render(M, W, H, None)

    def render_agreement(self, view):
        """-> (covered and foreground, covered and background, uncovered and foreground); the render
        stays as the current one."""
        k, M, W, H = self._view_camera(view)
        self._render(M, W, H, None)
        return render_np.agreement(self.rendered.id, self.sc.masks[k])

    def color_visible(self, mode, tol_voxels):
        """arvx_color_visible with a tolerance of tol_voxels voxel edges: it fills the colour list,
        with the colour list's lifetime."""
        if self.views is None or not self.images:
            raise Refused("color_visible without views / images")
        sc, v = self.sc, self._v()
        base = np.zeros((self.N, 4), np.float32)
        base[(self.st & OCC) != 0] = (-1, -1, -1, 1)
        r = visibility.color_visible(sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.campos[v], sc.images[v], mode, base,
                                     np.float32(tol_voxels) * sc.s)
        idx = r.index[r.has]
        self.colors = (idx, r.rgba[idx, :3].copy())
        self.clo = None
        self.visible = (self.colors, r.views[r.has].astype(np.int32), r.zbuf)

    # ---- the products: downloads that build nothing -------------------------------------------
    def mc_cells_list(self):
        if self.cells is None:
            raise Refused("no cell list")
        if self.cells[1] is None:
            sc = self.sc
            occ = np.zeros((self.N, 4), np.float32)
            occ[:, 3] = np.unpackbits(self.cells[0])[:self.N]
            self.cells[1] = sc.oracle.mc_cells(sc.X, sc.Y, sc.Z, occ)
        return self.cells[1]

    def mc_mesh_held(self):
        """arvx_mc_mesh_download[_faces]: before any arvx_mc_mesh the mesh has no triangle."""
        if self.mesh is None:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
        return self.mesh

    def welded_held(self):
        w = self.welded
        if w is None:
            raise Refused("no welded mesh")
        return w["verts"], w["faces"], w["face_rgb"], w["vrgb"]

    def smooth_held(self):
        if self.smoothed is None:
            raise Refused("no smoothed mesh")
        return self.smoothed

    def decimate_held(self):
        if self.decimated is None:
            raise Refused("no decimated mesh")
        return self.decimated

    def refined_held(self):
        if self.refined is None:
            raise Refused("no refined mesh")
        return self.refined[:5]

    def render_held(self):
        if self.rendered is None:
            raise Refused("no render")
        return tuple(self.rendered)

    def _visible(self):
        # the colour list of an arvx_color_visible: gone with the list, and after a plain
        # arvx_color or arvx_colors_upload filled it anew
        if self.colors is None or self.visible is None or self.visible[0] is not self.colors:
            raise Refused("no visible colour result")
        return self.visible

    def surface_visible(self):
        return self._visible()[1]

    def view_depth(self, view):
        return self._visible()[2][view]


class HostModel:
    """The reference's Model: RGBA per voxel (src/Model.h:93-163) and the seen bits."""

    def __init__(self, scene, state0=None):
        self.sc = scene
        self.N = scene.X * scene.Y * scene.Z
        self.rgba = np.tile(MODEL_COLOR, (self.N, 1))
        self.seen = np.zeros(self.N, bool)
        if state0 is not None:  # what test_host.cpp's loader does: set() zero, see()
            st0 = np.asarray(state0, np.uint8).reshape(-1)
            self.rgba[(st0 & OCC) == 0] = 0
            self.seen |= (st0 & SEEN) != 0

    def flat(self, x, y, z):
        return x + self.sc.X * (y + self.sc.Y * z)

    def set(self, x, y, z, v):
        self.rgba[self.flat(x, y, z)] = np.asarray(v, np.float32)

    def see(self, x, y, z):
        self.seen[self.flat(x, y, z)] = True

    def state(self):
        return ((self.rgba[:, 3] != 0) * OCC | self.seen * SEEN).astype(np.uint8)

    def _carved(self, st):
        """src/VoxelCarving.cpp:52: a carved voxel becomes (0, 0, 0, 0); the others keep their
        colour."""
        st = st.reshape(-1)
        gone = (st & OCC) == 0
        self.rgba[gone] = 0
        self.seen = (st & SEEN) != 0

    def carve(self, first=0, count=None):
        sc = self.sc
        count = len(sc.M) - first if count is None else count
        v = slice(first, first + count)
        self._carved(sc.oracle.carve(sc.X, sc.Y, sc.Z, sc.s, sc.M[v], sc.masks[v], state=self.state()))

    def fast_carve(self):
        sc = self.sc
        self._carved(sc.oracle.fast_carve(sc.X, sc.Y, sc.Z, sc.s, sc.M, sc.masks, state=self.state()))

    def color(self, mode):
        sc = self.sc
        self.rgba = sc.oracle.color(sc.X, sc.Y, sc.Z, sc.s, sc.M, sc.campos, sc.images, mode, self.rgba)

    def handle_unseen(self):
        self.rgba[~self.seen] = UNSEEN_COLOR

    def closure(self, k):
        sc = self.sc
        self.rgba = closure_any_kernel(self.rgba, sc.X, sc.Y, sc.Z, k)


def replay(model, target, ops, check):
    """Run `ops` -- tuples (name, *args) -- on `model` (a CtxModel) and `target` (the same
    methods on the device).  A call the model refuses must be refused by the target (it raises
    Refused too) and the other way round; where the model's call returns something (the counts of
    photo_carve, components, keep_components and morph) the target's call returns the same;
    observations ("obs", name, *args) are compared by check(name, want, got, step).  Returns the
    number of steps run."""
    for step, op in enumerate(ops):
        name, args = op[0], op[1:]
        if name == "obs":
            oname, oargs = args[0], args[1:]
            try:
                want = ("ok", getattr(model, oname)(*oargs))
            except Refused as e:
                want = ("refused", str(e))
            try:
                got = ("ok", getattr(target, oname)(*oargs))
            except Refused as e:
                got = ("refused", str(e))
            assert want[0] == got[0], (step, oname, want[0], got[0], want[1] if want[0] == "refused"
                                       else got[1])
            if want[0] == "ok":
                check(oname, want[1], got[1], step)
            continue
        args = model.resolve(name, args)
        want_ret = got_ret = None
        try:
            want_ret = getattr(model, name)(*args)
            want = "ok"
        except Refused:
            want = "refused"
        try:
            got_ret = getattr(target, name)(*args)
            got = "ok"
        except Refused:
            got = "refused"
        assert want == got, (step, name, f"model: {want}", f"device: {got}")
        if want == "ok" and want_ret is not None:
            assert got_ret == want_ret, (step, name, f"model returns {want_ret}", f"device returns {got_ret}")
    return len(ops)
