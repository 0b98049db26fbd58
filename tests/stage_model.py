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
says they live, and their downloads are refused before and after.  Not restated: arvx_render*, the
smoothed and decimated meshes, arvx_color_visible and arvx_ctx_set_projection_assoc."""
import numpy as np

from tests import components, distance, mesh_weld, occ_codec, photo_carve, vote_carve

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

    def mc_cells(self):
        sc = self.sc
        occ = np.zeros((self.N, 4), np.float32)
        occ[:, 3] = self.st & OCC
        return sc.oracle.mc_cells(sc.X, sc.Y, sc.Z, occ)

    def mc_model(self, apply_unseen):
        """The model the meshes are built from: the state's occupancy in export_model's colours."""
        self._flag_ok(apply_unseen)
        m = self._model(apply_unseen)
        m[(self.st & OCC) == 0] = 0
        return m

    def mc_mesh(self, apply_unseen):
        sc = self.sc
        return sc.oracle.mc_mesh(sc.X, sc.Y, sc.Z, self.mc_model(apply_unseen))

    def mc_mesh_welded(self, apply_unseen):
        return mesh_weld.weld(*self.mc_mesh(apply_unseen))


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
