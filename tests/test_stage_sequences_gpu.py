"""Orders of calls on one whole-grid context against tests/stage_model.CtxModel: every
intermediate observation bit for bit, every refusal (ARVX_ERR_STATE) where arvx.h says so.

The device keeps caches between calls -- the lazy coarse-tile codes, the colour pass's bit planes,
the state packets, the colour / closure lists, the paint plane, the carve's tile summaries -- and a
fixed carve -> colour -> handleUnseen -> closure chain on a fresh context never asks whether they
are still valid for the next call.  Random sequences do, and the pinned ones keep the cases that
once went wrong (or were found by reading the code) from coming back.

A second generator and a second set of pinned sequences (random_stage_ops, STAGE_PINNED) mix the
stages beyond the reference's pipeline into those orders: the vote carve, photo-consistency carving,
arvx_components_keep and the four ops of arvx_morph replace the state by hand-written need_rec / drop
code of their own, and the vote counts, the components' labelling and the distance field are three
more results whose lifetime the context has to get right.  The counts the state-changing calls
return are compared as well.  tests/test_stage_model_cpu.py checks, without a GPU, that the generator
gives every new stage something to do and that the old generator's sequences are what they were.

A third generator and a third set (random_mesh_ops, MESH_PINNED) bring in the products: the cell list,
the unwelded, welded, smoothed, decimated and refined meshes, the render and the visible colour pass.
Each is built by one call and downloaded by another that builds nothing, at once, behind a call that
must keep it, or behind a call that replaces the state: the meshes are snapshots whose lifetimes are
hand-written flags in five entry points, they share device buffers with each other and with the
stages (the cell list, the triangle offsets, the chunk counts of every compaction, the CSRs behind
the smoothing, the depth buffers of arvx_color_visible and arvx_photo_carve), and a product
downloaded after other calls have run is the only observation that shows whether one of them wrote
over it."""
import ctypes

import numpy as np
import pytest

from tests import stage_model as sm

pytestmark = pytest.mark.gpu

# the lazy form (Y, Z multiples of 8, several coarse tiles) and the packet form (X % 32 == 0),
# odd sizes, a row longer than one 64-bit word
GRIDS = [(128, 64, 64), (64, 24, 16), (21, 13, 11), (130, 16, 12)]
NV = 8  # views of a scene


class Device:
    """The C-ABI through capi.Context with the method names of CtxModel; ARVX_ERR_STATE ->
    sm.Refused."""

    def __init__(self, arvx, sc, lib_path=None):
        self.arvx, self.sc = arvx, sc
        self.ctx = arvx.Context(sc.X, sc.Y, sc.Z, sc.s, lib_path=lib_path)
        self.views = None
        self.ncomp = 0  # components of the last components()
        # the sizes the device gave for the products it holds (what their downloads fill)
        self.mesh_t = 0
        self.nweld = (0, 0)
        self.nref = (0, 0)
        lib, vp = self.ctx._lib, ctypes.c_void_p
        lib.arvx_mc_mesh_download.argtypes = [vp, vp, vp]
        lib.arvx_mc_mesh_download_faces.argtypes = [vp, vp, vp]
        lib.arvx_mc_mesh_welded_download.argtypes = [vp, vp, vp, vp]

    def close(self):
        self.ctx.close()

    def _call(self, fn, *a):
        try:
            return fn(*a)
        except self.arvx.ArvxError as e:
            if e.code == 3:
                raise sm.Refused(str(e))
            raise

    def set_views(self, lo, hi):
        sc = self.sc
        self._call(self.ctx.set_views, sc.M[lo:hi], sc.masks[lo:hi], sc.campos[lo:hi])
        self.views = (lo, hi)

    def set_images(self):
        if self.views is None:
            # (capi's set_images checks the images against the views' sizes, which it does not have
            # yet: the library is asked itself, and answers before it looks at an image)
            ctx, im = self.ctx, self.sc.images
            ptrs = (ctypes.c_void_p * len(im))(*[im[i].ctypes.data for i in range(len(im))])
            return self._call(lambda: ctx._ck(ctx._lib.arvx_set_images(ctx._h, ptrs, im.shape[2] * 3)))
        lo, hi = self.views
        self._call(self.ctx.set_images, self.sc.images[lo:hi])

    def carve(self, first=0, count=None):
        if count is None and first == 0:
            return self._call(self.ctx.carve)
        return self._call(self.ctx.carve_views, first, count)

    def fast_carve(self):
        self._call(self.ctx.fast_carve)

    def color(self, mode):
        self._call(self.ctx.color, mode)

    def upload_colors(self, index, rgb):
        self._call(self.ctx.upload_colors, index, rgb)

    def handle_unseen(self):
        self._call(self.ctx.handle_unseen)

    def closure(self, k, apply_unseen):
        self._call(self.ctx.closure, k, bool(apply_unseen), False)

    def upload_state(self, state):
        self._call(self.ctx.upload_state, state)

    def upload_planes(self, occ, seen):
        self._call(self.ctx.upload_planes, occ, seen)

    def reset(self):
        self._call(self.ctx.reset)

    def download_state(self):
        return self._call(self.ctx.download_state).reshape(-1)

    def download_planes(self):
        return self._call(self.ctx.download_planes)

    def download_packets(self):
        n, _ = self.ctx.packet_geometry()
        occ, seen, on, sn = self._call(self.ctx.download_packets)
        return sm.decode_packet(occ, n, on), sm.decode_packet(seen, n, sn)

    def export_model(self, apply_unseen):
        return self._call(self.ctx.export_model, bool(apply_unseen))

    def surface(self):
        return self._call(self.ctx.surface)

    def closure_list(self):
        return self._call(self.ctx.closure_download)

    def mc_cells(self):
        return self._call(self.ctx.mc_cells)

    def mc_mesh(self, apply_unseen):
        verts, rgb = self._call(self.ctx.mc_mesh, bool(apply_unseen))
        self.mesh_t = len(rgb)
        return verts, rgb

    def mc_mesh_welded(self, apply_unseen):
        verts, faces, rgb = self._call(self.ctx.mc_mesh_welded, bool(apply_unseen))
        self.nweld = (len(verts), len(faces))
        return verts, faces, rgb

    # ---- the products: builds (the call alone) and downloads (the *_download entry point alone) ----
    def _raw(self, name, *a):
        ctx = self.ctx
        return self._call(lambda: ctx._ck(getattr(ctx._lib, name)(ctx._h, *a)))

    def mc_cells_build(self):
        n = ctypes.c_int64()
        self._raw("arvx_mc_cells", ctypes.byref(n))
        return int(n.value)

    def mc_mesh_build(self, apply_unseen):
        self.mesh_t = self._call(self.ctx.mc_mesh_count, bool(apply_unseen))
        return self.mesh_t

    def weld(self, apply_unseen):
        self.nweld = self._call(self.ctx.mc_mesh_welded_count, bool(apply_unseen))
        return self.nweld

    def smooth(self, iterations, lam, mu):
        self._call(self.ctx.mc_mesh_smooth, iterations, lam, mu, False)

    def decimate(self, cell, source):
        return self._call(self.ctx.mc_mesh_decimate, cell, source, False)

    def refine(self, bisections, apply_unseen):
        self.nref = self._call(self.ctx.mc_mesh_refined_count, bisections, bool(apply_unseen))
        return self.nref

    def render(self, M, W, H, background):
        self._call(self.ctx.render, M, W, H, background, False)

    def render_view(self, view):
        self._call(self.ctx.render_view, view, False)

    def render_agreement(self, view):
        return self._call(self.ctx.render_agreement, view)

    def color_visible(self, mode, tol_voxels):
        self._call(self.ctx.color_visible, mode, float(np.float32(tol_voxels) * self.sc.s))

    def mc_cells_list(self):
        """arvx_mc_cells_download alone.  The list is the last cell walk's, and only arvx_mc_cells says how
        long it is -- the mesh calls that run the walk themselves return other counts -- so the buffer
        has the bound of arvx.h, a row per cell of [-1, X) x [-1, Y) x [-1, Z), and the rows the call
        left untouched are counted off its end."""
        sc, untouched = self.sc, np.iinfo(np.int32).min
        cells = np.full(((sc.X + 1) * (sc.Y + 1) * (sc.Z + 1), 4), untouched, np.int32)
        self._raw("arvx_mc_cells_download", cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        n = int(np.count_nonzero(cells[:, 3] != untouched))
        assert (cells[n:] == untouched).all()
        return cells[:n]

    def mc_mesh_held(self):
        """Both forms of the download; the face records must say what the plain form says."""
        T = self.mesh_t
        verts, rgb = np.empty((max(3 * T, 1), 3), np.float32), np.empty((max(T, 1), 3), np.uint32)
        v2, faces = np.empty_like(verts), np.empty((max(T, 1), 6), np.uint32)
        self._raw("arvx_mc_mesh_download", verts.ctypes.data, rgb.ctypes.data)
        self._raw("arvx_mc_mesh_download_faces", v2.ctypes.data, faces.ctypes.data)
        verts, rgb, v2, faces = verts[:3 * T], rgb[:T], v2[:3 * T], faces[:T]
        assert equal(v2, verts) and np.array_equal(faces[:, 3:], rgb)
        assert np.array_equal(faces[:, :3].reshape(-1), np.arange(3 * T, dtype=np.uint32))
        return verts, rgb

    def welded_held(self):
        V, T = self.nweld
        verts, rec, vrgb = np.empty((V, 3), np.float32), np.empty((T, 6), np.uint32), np.empty((V, 3), np.float32)
        self._raw("arvx_mc_mesh_welded_download", verts.ctypes.data, rec.ctypes.data, vrgb.ctypes.data)
        return verts, np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 3:]), vrgb

    def smooth_held(self):
        V = self.nweld[0]
        verts, normals = np.empty((V, 3), np.float32), np.empty((V, 3), np.float32)
        self._raw("arvx_mc_mesh_smooth_download", verts.ctypes.data, normals.ctypes.data)
        return verts, normals

    def decimate_held(self):
        return self._call(self.ctx.mc_mesh_decimate_download)

    def refined_held(self):
        Vr, T = self.nref
        out = (np.empty((Vr, 3), np.float32), np.empty((T, 6), np.uint32), np.empty((Vr, 3), np.float32),
               np.empty((Vr, 4), np.int32), np.empty(Vr, np.int32))
        self._raw("arvx_mc_mesh_refined_download", *[a.ctypes.data for a in out])
        return out

    def render_held(self):
        return self._call(self.ctx.render_download)

    def surface_visible(self):
        n = ctypes.c_int64()
        self._raw("arvx_surface_count", ctypes.byref(n))
        out = np.empty(max(n.value, 1), np.int32)
        self._raw("arvx_surface_visible_download", out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        return out[:n.value]

    def view_depth(self, view):
        """arvx_view_depth_download alone (capi's wrapper takes the size from views it may not have yet)."""
        out = np.empty(self.sc.masks.shape[1:3], np.float32)
        self._raw("arvx_view_depth_download", int(view), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        return out

    def fallbacks(self):
        return int(self.ctx.stats()["host_total_fallbacks"])

    # ---- the stages beyond the reference's pipeline ----
    def carve_votes(self, max_misses, counts):
        self._call(self.ctx.carve_votes, max_misses, bool(counts))

    def photo_carve(self, max_std, min_views, tol_voxels, max_iterations):
        tol = float(np.float32(tol_voxels) * self.sc.s)
        return self._call(self.ctx.photo_carve, max_std, min_views, tol, max_iterations)

    def components(self, connectivity):
        labels, _ = self._call(self.ctx.components, connectivity)
        self.ncomp = len(labels)
        return self.ncomp

    def keep_components(self, connectivity, min_voxels, largest):
        return self._call(self.ctx.keep_components, min_voxels, bool(largest), connectivity)

    def distance(self, border_occupied):
        """arvx_distance alone: distance_field downloads."""
        flags = self.arvx.DISTANCE_BORDER_OCCUPIED if border_occupied else 0
        self._call(lambda: self.ctx._ck(self.ctx._lib.arvx_distance(self.ctx._h, flags)))

    def morph(self, op, radius_sq):
        return self._call(self.ctx.morph, op, radius_sq)

    def votes(self):
        return self._call(self.ctx.votes)

    def component_table(self):
        """arvx_components_download alone, no relabelling: the table of the last components() (a
        table has at most a label per voxel: room for that, whatever the library hands out)."""
        ctx = self.ctx
        lab, size = np.full(ctx.nvox, -1, np.int32), np.full(ctx.nvox, -1, np.int32)
        self._call(lambda: ctx._ck(ctx._lib.arvx_components_download(ctx._h, lab.ctypes.data, size.ctypes.data)))
        return lab[:self.ncomp], size[:self.ncomp]

    def component_labels(self):
        return self._call(self.ctx.component_labels)

    def distance_field(self):
        """arvx_distance_download alone, no rebuild."""
        ctx = self.ctx
        out = np.empty(ctx.nvox, np.int32)
        self._call(lambda: ctx._ck(ctx._lib.arvx_distance_download(ctx._h, out.ctypes.data)))
        return out


def packet_grid(X, Y):
    return X % 32 == 0 and (X * Y) % 64 == 0


OBS = ["download_state", "download_planes", "download_packets", "export_model", "surface",
       "closure_list", "mc_cells", "mc_mesh", "mc_mesh_welded"]


def random_ops(seed, X, Y):
    rng = np.random.default_rng(1000 + seed)
    ops = []
    if rng.random() < 0.9:
        ops.append(("set_views", 0, NV))
        if rng.random() < 0.85:
            ops.append(("set_images",))
    kinds = ["carve", "carve_views", "fast_carve", "set_views", "set_images", "color", "upload_colors",
             "handle_unseen", "closure", "upload_state", "upload_planes", "reset", "obs"]
    p = np.array([18, 6, 4, 3, 4, 12, 4, 12, 14, 4, 3, 3, 13], float)
    obs = [o for o in OBS if o != "download_packets" or packet_grid(X, Y)]
    for _ in range(int(rng.integers(6, 13))):
        k = kinds[rng.choice(len(kinds), p=p / p.sum())]
        if k == "carve":
            ops.append(("carve",))
        elif k == "carve_views":
            f = int(rng.integers(0, 3))  # (every view set has at least 3 views)
            ops.append(("carve", f, int(rng.integers(1, 4 - f))))
        elif k == "set_views":
            lo = int(rng.integers(0, 3))
            ops.append(("set_views", lo, int(rng.integers(lo + 3, NV + 1))))
        elif k == "color":
            ops.append(("color", int(rng.integers(0, 2))))
        elif k == "closure":
            ops.append(("closure", int(rng.choice([1, 3, 3, 5])), int(rng.integers(0, 2))))
        elif k in ("upload_state", "upload_planes", "upload_colors"):
            ops.append((k, int(rng.integers(0, 1 << 30))))
        elif k == "obs":
            o = obs[rng.integers(len(obs))]
            ops.append(("obs", o, int(rng.integers(0, 2))) if o in ("export_model", "mc_mesh", "mc_mesh_welded")
                       else ("obs", o))
        else:
            ops.append((k,))
    ops.append(("obs", "export_model", int(rng.integers(0, 2))))
    ops.append(("obs", "download_state"))
    return ops


# ---- sequences over the stages beyond the reference's pipeline ---------------------------------

STAGE_OBS = ["votes", "component_table", "component_labels", "distance_field"]
STAGE_GRIDS = GRIDS
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
INF = float("inf")


def random_stage_ops(seed, X, Y):
    """The kinds of random_ops at reduced weight, plus the vote carve, photo carving, the components,
    the distance field and the morphology, their arguments from the edges of their ranges.  A sequence
    opens with something that leaves the later stages material (two of the grids carve down to
    next to nothing under all views).  A stage that leaves a result is often asked for it, at once or
    after one of the calls that must keep it (keeper), so that a result is also seen to survive them.
    On the 128 x 64 x 64 grid a sequence gets two photo sweeps in all: a photo carve drawn there is cut
    to what is left of them, and once none is left it TURNS INTO A KEEP (so max_iterations 4 does not
    occur on that grid in the random set; the pinned sequences ask for it there)."""
    rng = np.random.default_rng(7000 + seed)
    pick = lambda values: values[int(rng.integers(len(values)))]

    def votes():
        return ("carve_votes", pick([0, 1, 2, NV, 65535]), int(rng.random() < 0.6))

    # The restatement of a photo sweep over the surface of an uploaded noise state is the one slow step
    # on the host, 0.15 s on the 128 x 64 x 64 grid: the budget keeps a case within three times the
    # slowest of test_random_sequence.
    sweeps_left = 2 if X * Y >= 8192 else 1 << 30

    def photo():
        nonlocal sweeps_left
        max_iterations = min(pick([1, 2, 4]), sweeps_left)
        if max_iterations == 0:
            return keep()
        sweeps_left -= max_iterations
        return ("photo_carve", pick([0.0, 20.0, 60.0, INF]), int(rng.integers(1, 4)), pick([0.0, 1.0, 2.0, INF]),
                max_iterations)

    def keep():
        return ("keep_components", pick([6, 26]), pick([1, 2, 10, 100]), int(rng.random() < 0.4))

    def morph():
        return ("morph", pick([ERODE, DILATE, OPEN, CLOSE]), pick([0, 1, 2, 3, 9]))

    def keeper(result):
        """A call that keeps `result` ("votes", "labelling" or "field"), per arvx.h."""
        calls = [("set_images",), ("color", int(rng.integers(0, 2))), ("upload_colors", int(rng.integers(0, 1 << 30)))]
        if result != "votes":
            calls.append(("set_views", 1, NV))
        if result != "labelling":
            calls.append(("components", pick([6, 26])))
        if result != "field":
            calls.append(("distance", int(rng.integers(0, 2))))
        return pick(calls)

    def ask(result, names, p):
        """With probability p an observation of `result`, half of the time behind a keeper."""
        if rng.random() < p:
            if rng.random() < 0.5:
                ops.append(keeper(result))
            ops.append(("obs", pick(names)))

    ops = []
    if rng.random() < 0.95:
        ops.append(("set_views", 0, NV))
        if rng.random() < 0.9:
            ops.append(("set_images",))
    opening = rng.random()
    if opening < 0.3:
        ops.append(("carve",))
    elif opening < 0.65:
        ops.append(("upload_state", int(rng.integers(0, 1 << 30))))
    elif opening < 0.85:
        ops.append(("carve_votes", pick([1, 2]), int(rng.random() < 0.6)))
    kinds = ["carve", "carve_views", "fast_carve", "set_views", "set_images", "color", "upload_colors",
             "handle_unseen", "closure", "upload_state", "upload_planes", "reset", "obs",
             "carve_votes", "photo_carve", "components", "keep_components", "distance", "morph", "stage_obs"]
    p = np.array([5, 2, 1, 3, 3, 5, 2, 6, 7, 5, 2, 1, 5,
                  8, 7, 6, 8, 5, 12, 10], float)
    obs = [o for o in OBS if o != "download_packets" or packet_grid(X, Y)]
    for _ in range(int(rng.integers(7, 13))):
        k = kinds[rng.choice(len(kinds), p=p / p.sum())]
        if k == "carve_views":
            f = int(rng.integers(0, 3))
            ops.append(("carve", f, int(rng.integers(1, 4 - f))))
        elif k == "set_views":
            lo = int(rng.integers(0, 3))
            ops.append(("set_views", lo, int(rng.integers(lo + 3, NV + 1))))
        elif k == "color":
            ops.append(("color", int(rng.integers(0, 2))))
        elif k == "closure":
            ops.append(("closure", pick([1, 3, 3, 5]), int(rng.integers(0, 2))))
            if rng.random() < 0.3:  # (the fills lose their list: photo carve, keep and morph are refused)
                ops.append(pick([("handle_unseen",), ("set_images",), ("color", 0)]))
        elif k == "upload_state":
            ops.append((k, int(rng.integers(0, 1 << 30)), int(rng.random() < 0.3)))
        elif k in ("upload_planes", "upload_colors"):
            ops.append((k, int(rng.integers(0, 1 << 30))))
        elif k == "obs":
            o = pick(obs)
            ops.append(("obs", o, int(rng.integers(0, 2))) if o in ("export_model", "mc_mesh", "mc_mesh_welded")
                       else ("obs", o))
        elif k == "carve_votes":
            ops.append(votes())
            if ops[-1][2]:
                ask("votes", ["votes"], 0.6)
        elif k == "photo_carve":
            ops.append(photo())
        elif k == "components":
            ops.append(("components", pick([6, 26])))
            ask("labelling", ["component_table", "component_labels"], 0.5)
        elif k == "keep_components":
            ops.append(keep())
        elif k == "distance":
            ops.append(("distance", int(rng.integers(0, 2))))
            ask("field", ["distance_field"], 0.5)
        elif k == "morph":
            ops.append(morph())
        elif k == "stage_obs":
            ops.append(("obs", pick(STAGE_OBS)))
        else:
            ops.append((k,))
    ops.append(("obs", "download_state"))
    ops.append(("obs", "export_model", int(rng.integers(0, 2))))
    return ops


# ---- sequences over the products: meshes, render, visible colour --------------------------------

MESH_OBS = ["mc_cells_list", "mc_mesh_held", "welded_held", "smooth_held", "decimate_held", "refined_held",
            "render_held", "surface_visible", "view_depth"]
LATTICE, SMOOTHED = 0, 1


def random_mesh_ops(seed, X, Y):
    """The kinds of random_stage_ops at reduced weight, plus the builds of the products and ask(): a
    download of a product at once, behind a call that must keep it, or behind a call that replaces the
    state (the meshes then still deliver what they held, the render is refused).

    The host-side restatements set the budget.  On the 128 x 64 x 64 grid a surface of an uploaded noise
    state has 200 000 vertices (8 s for one smooth, 2 s for one refine), a fresh or barely carved model a
    box of 40 000: a sequence there builds a mesh or runs arvx_color_visible only while the state is
    SMALL -- a carve or a tight vote carve under at least six views has run since the last upload or
    reset -- and has units left of a budget that the slow builds draw on (smooth 2, the first on a welded
    mesh 3; refine 2; decimate and color_visible 1).  A build drawn otherwise TURNS INTO a render of the
    held mesh or into a reset, and the old observations that weld or mesh at once into download_state.
    That keeps a case within three times the slowest of test_random_sequence, as random_stage_ops'
    photo budget does."""
    rng = np.random.default_rng(13000 + seed)
    pick = lambda values: values[int(rng.integers(len(values)))]
    big = X * Y >= 8192
    budget = 6 if big else 1 << 30
    small = not big          # (the other grids: any state is small enough)
    nviews = 0
    csr = False              # the held welded mesh has been smoothed (its CSRs exist)
    sweeps_left = 2 if big else 1 << 30
    ops = []

    def emit(op):
        nonlocal small, nviews
        ops.append(op)
        if not big:
            return
        if op[0] == "set_views":
            nviews = op[2] - op[1]
        elif op[0] in ("upload_state", "upload_planes", "reset"):
            small = False
        elif (op == ("carve",) or op[0] == "carve_votes" and op[1] <= 1) and nviews >= 6:
            small = True

    def render():
        return pick([("render", int(rng.integers(0, 4)), int(rng.integers(0, 2)), pick([None, int(rng.integers(0, 99))])),
                     ("render_view", int(rng.integers(0, 3))), ("render_agreement", int(rng.integers(0, 3)))])

    def build(op, cost=0):
        """The build, or what it turns into where the host could not follow."""
        nonlocal budget, csr
        if op[0] == "smooth" and not csr:
            cost += 1
        if small and budget >= cost:
            budget -= cost
            if op[0] == "weld":
                csr = False
            elif op[0] == "smooth":
                csr = True
            emit(op)
            return True
        emit(render() if rng.random() < 0.7 else ("reset",))
        return False

    def smooth():
        return ("smooth", pick([0, 1, 1, 2, 3]), pick([0.5, 0.33]), pick([-0.53, 0.0]))

    def keeper(product):
        """A call that must keep `product`, per arvx.h."""
        if product == "visible":
            return pick([("handle_unseen",), ("components", pick([6, 26])), ("distance", int(rng.integers(0, 2))),
                         ("render_view", int(rng.integers(0, 3))), ("mc_cells_build",)])
        calls = [("set_images",), ("color", int(rng.integers(0, 2))), ("upload_colors", int(rng.integers(0, 1 << 30))),
                 ("set_views", 1, NV), ("handle_unseen",), ("components", pick([6, 26])),
                 ("distance", int(rng.integers(0, 2)))]
        if product != "cells":
            calls.append(("mc_cells_build",))
        if product == "render":
            calls.append(("decimate", pick([1, 2, 3]), LATTICE))
        elif product in ("welded", "smoothed", "decimated"):
            calls.append(render())
        return pick(calls)

    def replacer():
        """A call that replaces the state (and does not put the 128 x 64 x 64 grid's noise there)."""
        f = int(rng.integers(0, 3))
        return pick([("carve", f, int(rng.integers(1, 4 - f))), ("morph", pick([ERODE, DILATE, OPEN, CLOSE]), pick([1, 2, 3])),
                     ("keep_components", pick([6, 26]), pick([2, 10]), int(rng.random() < 0.4)),
                     ("carve_votes", pick([0, 1, 2]), 0), ("handle_unseen",)])

    def ask(product, names, p=0.75):
        if rng.random() < p:
            how = rng.random()
            if how < 0.3:
                emit(keeper(product))
            elif how < 0.7:
                emit(replacer())
            o = pick(names)
            emit(("obs", o, int(rng.integers(0, 3))) if o == "view_depth" else ("obs", o))

    if rng.random() < 0.95:
        emit(("set_views", 0, NV))
        if rng.random() < 0.9:
            emit(("set_images",))
    opening = rng.random()
    if big:
        emit(("carve",) if opening < 0.7 else ("carve_votes", 1, 0) if opening < 0.85 else
             ("upload_state", int(rng.integers(0, 1 << 30))))
    elif opening < 0.5:
        emit(("upload_state", int(rng.integers(0, 1 << 30))))
    elif opening < 0.9:
        f = int(rng.integers(0, 3))
        emit(("carve", f, int(rng.integers(1, 3))))
    kinds = ["carve", "carve_views", "fast_carve", "set_views", "set_images", "color", "upload_colors",
             "handle_unseen", "closure", "upload_state", "upload_planes", "reset", "obs",
             "carve_votes", "photo_carve", "components", "keep_components", "distance", "morph",
             "cells", "mesh", "weld", "smooth", "decimate", "refine", "render", "color_visible", "mesh_obs"]
    p = np.array([3, 2, 1, 2, 2, 3, 1, 3, 4, 2, 1, 1, 3,
                  2, 2, 1, 2, 1, 3,
                  3, 3, 12, 5, 5, 7, 6, 7, 8], float)
    obs = [o for o in OBS if o != "download_packets" or packet_grid(X, Y)]
    for _ in range(int(rng.integers(7, 13))):
        k = kinds[rng.choice(len(kinds), p=p / p.sum())]
        if k == "carve_views":
            f = int(rng.integers(0, 3))
            emit(("carve", f, int(rng.integers(1, 4 - f))))
        elif k == "set_views":
            lo = int(rng.integers(0, 3))
            emit(("set_views", lo, int(rng.integers(lo + 3, NV + 1))))
        elif k == "color":
            emit(("color", int(rng.integers(0, 2))))
        elif k == "closure":
            emit(("closure", pick([1, 3, 3, 5]), int(rng.integers(0, 2))))
        elif k == "upload_state":
            emit((k, int(rng.integers(0, 1 << 30)), int(rng.random() < 0.3)))
        elif k in ("upload_planes", "upload_colors"):
            emit((k, int(rng.integers(0, 1 << 30))))
        elif k == "obs":
            o = pick(obs)
            if o in ("mc_mesh", "mc_mesh_welded") and not small:
                o = "download_state"
            if o == "mc_mesh_welded":
                csr = False
            emit(("obs", o, int(rng.integers(0, 2))) if o in ("export_model", "mc_mesh", "mc_mesh_welded")
                 else ("obs", o))
        elif k == "carve_votes":
            emit(("carve_votes", pick([0, 1, 2, NV]), 0))
        elif k == "photo_carve":
            it = min(pick([1, 2]), sweeps_left)
            sweeps_left -= it
            emit(("photo_carve", pick([20.0, 60.0, INF]), int(rng.integers(1, 4)), pick([0.0, 1.0, INF]), it) if it
                 else ("keep_components", 6, 2, 0))
        elif k == "components":
            emit(("components", pick([6, 26])))
        elif k == "keep_components":
            emit(("keep_components", pick([6, 26]), pick([1, 2, 10, 100]), int(rng.random() < 0.4)))
        elif k == "distance":
            emit(("distance", int(rng.integers(0, 2))))
        elif k == "morph":
            emit(("morph", pick([ERODE, DILATE, OPEN, CLOSE]), pick([0, 1, 2, 3, 9])))
        elif k == "cells":
            emit(("mc_cells_build",))
            ask("cells", ["mc_cells_list"])
        elif k == "mesh":
            if build(("mc_mesh_build", int(rng.integers(0, 2)))):
                ask("mesh", ["mc_mesh_held"])
        elif k == "weld":
            if build(("weld", int(rng.integers(0, 2)))):
                ask("welded", ["welded_held"], 0.5)
                if rng.random() < 0.6 and build(smooth(), 2):
                    ask("smoothed", ["smooth_held"], 0.5)
                    if rng.random() < 0.5 and build(smooth(), 2):
                        ask("smoothed", ["smooth_held", "welded_held"])
                if rng.random() < 0.6 and build(("decimate", pick([1, 2, 3, 7]), pick([LATTICE, SMOOTHED, SMOOTHED])), 1):
                    ask("decimated", ["decimate_held"])
                if rng.random() < 0.5:
                    emit(render())
                    ask("render", ["render_held"])
        elif k == "smooth":
            if build(smooth(), 2):
                ask("smoothed", ["smooth_held"])
        elif k == "decimate":
            if build(("decimate", pick([1, 2, 4, 64]), pick([LATTICE, SMOOTHED])), 1):
                ask("decimated", ["decimate_held", "smooth_held", "welded_held"])
        elif k == "refine":
            if build(("refine", pick([0, 1, 6, 6, 10]), int(rng.integers(0, 2))), 2):
                ask("refined", ["refined_held"])
        elif k == "render":
            emit(render())
            ask("render", ["render_held"], 0.9)
        elif k == "color_visible":
            if build(("color_visible", int(rng.integers(0, 2)), pick([0.0, 1.0, 2.0, INF])), 1):
                if rng.random() < 0.3:
                    emit(pick([("color", 1), ("upload_colors", int(rng.integers(0, 1 << 30)))]))
                elif rng.random() < 0.5:
                    emit(keeper("visible"))
                emit(pick([("obs", "surface_visible"), ("obs", "view_depth", int(rng.integers(0, 3))), ("obs", "surface")]))
        elif k == "mesh_obs":
            o = pick(MESH_OBS)
            emit(("obs", o, int(rng.integers(0, 3))) if o == "view_depth" else ("obs", o))
        else:
            emit((k,))
    emit(("obs", pick(["welded_held", "refined_held", "decimate_held", "render_held"])))
    emit(("obs", "download_state"))
    return ops


def equal(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 or b.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    return a.shape == b.shape and np.array_equal(a, b)


def run(arvx, sc, ops, label, lib_path=None, no_fallbacks=False):
    model = sm.CtxModel(sc)
    dev = Device(arvx, sc, lib_path)

    def check(name, want, got, step):
        if not equal(want, got):
            detail = ""
            if name in ("download_state", "export_model"):
                w, g = np.asarray(want).reshape(len(want), -1), np.asarray(got).reshape(len(got), -1)
                bad = np.flatnonzero((w != g).any(axis=1))
                detail = f" -- {len(bad)} voxels differ, first {bad[:5].tolist()}: want {w[bad[:3]].tolist()} got {g[bad[:3]].tolist()}"
            raise AssertionError(f"{label}: {name} differs at step {step}{detail}\n  ops: {ops[:step + 1]}")

    try:
        sm.replay(model, dev, ops, check)
        if no_fallbacks:  # (no list total had to be fetched from the device by the host)
            assert dev.fallbacks() == 0, f"{label}: host_total_fallbacks {dev.fallbacks()}"
    except AssertionError as e:
        if str(e).startswith(label):
            raise
        raise AssertionError(f"{label}: {e}\n  ops: {ops}") from None
    finally:
        dev.close()


@pytest.fixture(scope="module")
def scenes_by_grid(oracle):
    return {g: sm.make_scene(oracle, *g, seed=sum(g)) for g in GRIDS}


SEEDS = [(GRIDS[i % len(GRIDS)], i) for i in range(48)]


@pytest.mark.parametrize("grid,seed", SEEDS, ids=[f"{g[0]}x{g[1]}x{g[2]}-s{s}" for g, s in SEEDS])
def test_random_sequence(arvx, scenes_by_grid, grid, seed):
    sc = scenes_by_grid[grid]
    run(arvx, sc, random_ops(seed, grid[0], grid[1]), f"seed {seed} grid {grid}")


STAGE_SEEDS = [(STAGE_GRIDS[i % len(STAGE_GRIDS)], i) for i in range(48)]


@pytest.mark.parametrize("grid,seed", STAGE_SEEDS, ids=[f"{g[0]}x{g[1]}x{g[2]}-s{s}" for g, s in STAGE_SEEDS])
def test_random_stage_sequence(arvx, scenes_by_grid, grid, seed):
    sc = scenes_by_grid[grid]
    run(arvx, sc, random_stage_ops(seed, grid[0], grid[1]), f"stage seed {seed} grid {grid}")


MESH_SEEDS = [(GRIDS[i % len(GRIDS)], i) for i in range(48)]


@pytest.mark.parametrize("grid,seed", MESH_SEEDS, ids=[f"{g[0]}x{g[1]}x{g[2]}-s{s}" for g, s in MESH_SEEDS])
def test_random_mesh_sequence(arvx, scenes_by_grid, grid, seed):
    sc = scenes_by_grid[grid]
    run(arvx, sc, random_mesh_ops(seed, grid[0], grid[1]), f"mesh seed {seed} grid {grid}", no_fallbacks=True)


# ---- pinned sequences ----------------------------------------------------------------------

PINNED = {
    # Model::handleUnseen / a second closure on the lazy state: arvx_closure refuses a state that
    # holds an earlier closure's fills (its list is gone after handle_unseen / set_images)
    "closure_unseen_closure": [("set_views", 0, NV), ("set_images",), ("carve",), ("color", 1),
                               ("closure", 3, 1), ("obs", "closure_list"), ("handle_unseen",),
                               ("closure", 3, 1), ("obs", "export_model", 1), ("obs", "download_state")],
    "closure_images_color_closure": [("set_views", 0, NV), ("set_images",), ("carve",), ("closure", 3, 0),
                                     ("set_images",), ("color", 0), ("closure", 3, 0),
                                     ("obs", "export_model", 0), ("obs", "mc_cells")],
    # ... and so are the calls that return the fills' colours; occupancy and the colour pass stay
    "closure_unseen_outputs": [("set_views", 0, NV), ("set_images",), ("carve", 0, 3), ("closure", 3, 0),
                               ("handle_unseen",), ("obs", "mc_cells"), ("obs", "export_model", 1),
                               ("obs", "mc_mesh", 1), ("obs", "mc_mesh_welded", 0), ("color", 1),
                               ("obs", "surface"), ("obs", "download_state")],
    # ... while a carve replaces the state: a second closure is defined again
    "closure_carve_closure": [("set_views", 0, NV), ("set_images",), ("carve",), ("closure", 5, 1),
                              ("carve", 0, 2), ("closure", 3, 1), ("obs", "closure_list"),
                              ("obs", "export_model", 1)],
    # cstate_tiles (what earlier carves settled) across handleUnseen
    "carve_unseen_carve": [("set_views", 0, 4), ("carve",), ("handle_unseen",), ("set_views", 2, NV),
                           ("carve",), ("obs", "download_state"), ("obs", "download_planes")],
    # the closure starting from the colour pass's planes after handleUnseen
    "color_unseen_closure": [("set_views", 0, NV), ("set_images",), ("carve",), ("color", 1),
                             ("handle_unseen",), ("closure", 3, 0), ("obs", "closure_list"),
                             ("obs", "export_model", 0), ("obs", "mc_mesh", 0)],
    # the packet cache across a closure and handleUnseen
    "packets_closure_unseen": [("set_views", 0, NV), ("carve",), ("closure", 3, 0),
                               ("obs", "download_packets"), ("handle_unseen",), ("obs", "download_packets"),
                               ("obs", "download_state")],
    # bit2 on empty voxels (arvx_state_upload): kept, and the paint wins in export and closure
    "empty_paint_closure": [("upload_state", 11, 1), ("obs", "download_state"), ("obs", "export_model", 0),
                            ("closure", 3, 0), ("obs", "closure_list"), ("obs", "export_model", 0),
                            ("obs", "download_state")],
    # the paint plane's lifetime: uploaded, dropped by the carve
    "paint_carve_closure": [("set_views", 0, NV), ("set_images",), ("upload_state", 7),
                            ("obs", "download_state"), ("carve",), ("closure", 3, 0),
                            ("obs", "export_model", 0), ("obs", "download_state")],
}


@pytest.mark.parametrize("name", sorted(PINNED))
@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]], ids=["lazy", "packets"])
def test_pinned_sequence(arvx, scenes_by_grid, name, grid):
    run(arvx, scenes_by_grid[grid], PINNED[name], f"pinned {name} grid {grid}")


# ---- pinned sequences over the stages beyond the reference's pipeline -------------------------

VIEWS = [("set_views", 0, NV), ("set_images",)]
STATE3 = [("obs", "component_table"), ("obs", "component_labels"), ("obs", "distance_field")]


def _on_lazy_state(stage):
    """A carve of a fresh model leaves most coarse tiles as their code only; the stage has to end that
    lazy state (every form the state downloads in shows it), and the carve under other views that
    follows must neither trust a tile the stage changed nor miss the voxels it added."""
    return [("set_views", 0, 4), ("set_images",), ("carve",), stage, ("obs", "download_state"),
            ("obs", "download_planes"), ("obs", "download_packets"), ("obs", "mc_cells"),
            ("set_views", 2, NV), ("carve",), ("obs", "download_state")]


# Every view but 2 and 3 sees the whole grid, so after most carves handleUnseen has nothing to
# occupy.  View 2 alone leaves a quarter of the grid never seen (and carves nothing there); an erosion
# then empties part of it, and that part is what handleUnseen brings back.
UNSEEN_EMPTY = VIEWS + [("carve", 2, 1), ("morph", ERODE, 9)]


def _photo_after_unseen(max_std, max_iterations):
    """The colour pass's planes, handed on by handleUnseen (planes_unseen), meet the photo loop's own
    plane rebuild; the closure then starts from whatever planes are left."""
    return UNSEEN_EMPTY + [("color", 1), ("handle_unseen",), ("photo_carve", max_std, 3, 1.0, max_iterations),
                           ("obs", "download_state"), ("closure", 3, 0), ("obs", "closure_list"),
                           ("obs", "export_model", 0), ("obs", "mc_cells")]


STAGE_PINNED = {
    # (a vote carve under the views of the carve before it can empty nothing: it runs under six others,
    # two of them new, and the last carve runs under all eight)
    "lazy_votes": [("set_views", 0, 4), ("set_images",), ("carve",), ("set_views", 2, NV), ("carve_votes", 1, 1),
                   ("obs", "votes"), ("obs", "download_state"), ("obs", "download_planes"),
                   ("obs", "download_packets"), ("obs", "mc_cells"), ("set_views", 0, NV), ("carve",),
                   ("obs", "download_state")],
    "lazy_photo": _on_lazy_state(("photo_carve", 20.0, 2, 1.0, 2)),
    "lazy_keep": _on_lazy_state(("keep_components", 6, 10, 0)),
    "lazy_erode": _on_lazy_state(("morph", ERODE, 2)),
    "lazy_dilate": _on_lazy_state(("morph", DILATE, 3)),  # (the second carve looks at the new voxels)
    "lazy_open": _on_lazy_state(("morph", OPEN, 1)),
    "lazy_close": _on_lazy_state(("morph", CLOSE, 9)),    # (as for DILATE)
    # a closure's fills whose list handleUnseen dropped: the three stages that would have to know the
    # fills' colours are refused and change nothing; after a carve each is accepted
    "fills_without_list": VIEWS + [("carve", 0, 3), ("closure", 3, 0), ("handle_unseen",),
                                   ("photo_carve", 20.0, 1, 1.0, 1), ("keep_components", 6, 2, 0),
                                   ("morph", DILATE, 1), ("morph", ERODE, 1), ("obs", "download_state"),
                                   ("carve", 0, 3), ("photo_carve", 20.0, 1, 1.0, 1), ("keep_components", 6, 2, 0),
                                   ("morph", DILATE, 1), ("obs", "download_state"), ("obs", "export_model", 0)],
    # ... while the list is there a keep is accepted; it drops the list and the mark of the fills, which
    # are plain occupancy from then on: a second closure is defined again
    "fills_with_list_keep": VIEWS + [("carve", 0, 3), ("color", 0), ("closure", 3, 0), ("keep_components", 26, 2, 0),
                                     ("obs", "closure_list"), ("obs", "surface"), ("closure", 3, 0),
                                     ("obs", "closure_list"), ("obs", "export_model", 0)],
    # ... also where the closure ran on the lazy state and wrote out only the coarse tiles it filled into:
    # the keep / the dilation then writes out the rest, and must leave the filled tiles as they are
    "lazy_closure_keep_closure": VIEWS + [("carve",), ("closure", 3, 0), ("keep_components", 6, 100, 0),
                                          ("obs", "download_state"), ("closure", 3, 0), ("obs", "closure_list"),
                                          ("obs", "export_model", 0), ("obs", "mc_cells")],
    "lazy_closure_dilate": VIEWS + [("carve",), ("closure", 3, 1), ("morph", DILATE, 1), ("obs", "download_state"),
                                    ("obs", "download_planes"), ("obs", "export_model", 1)],
    # the labelling and the field read a lazy state as it is (they change nothing, so they do not end it),
    # before and after handleUnseen on it
    "lazy_components_distance": VIEWS + [("carve",), ("components", 6)] + STATE3[:2] + [
        ("distance", 0), ("obs", "distance_field"), ("handle_unseen",), ("components", 26), ("distance", 1)]
        + STATE3 + [("obs", "download_state")],
    # the paint plane (bit2, on empty voxels too) goes with a vote carve, a keep and a morph that change no
    # voxel: no bit2 in the bytes, no UNSEEN_COLOR in the model
    "paint_dropped_without_a_change": [("set_views", 0, NV), ("upload_state", 11, 1), ("carve_votes", 65535, 0),
                                       ("obs", "download_state"), ("obs", "export_model", 0),
                                       ("upload_state", 12, 1), ("keep_components", 6, 1, 0),
                                       ("obs", "download_state"), ("obs", "export_model", 0),
                                       ("upload_state", 13, 1), ("morph", ERODE, 0),
                                       ("obs", "download_state"), ("obs", "export_model", 0),
                                       ("upload_state", 14, 1), ("morph", CLOSE, 0),
                                       ("obs", "download_state"), ("obs", "export_model", 0)],
    # the vote counts: kept by what replaces neither the state nor the views ...
    "votes_lifetime": VIEWS + [("carve_votes", 1, 1), ("obs", "votes"), ("set_images",), ("color", 1),
                               ("upload_colors", 5), ("components", 6), ("distance", 0), ("obs", "votes"),
                               # ... dropped by new views, handleUnseen, the closure, a vote carve without counts
                               ("set_views", 0, NV), ("obs", "votes"),
                               ("carve_votes", 1, 1), ("handle_unseen",), ("obs", "votes"),
                               ("carve_votes", 2, 1), ("obs", "votes"), ("closure", 3, 0), ("obs", "votes"),
                               ("carve_votes", 2, 1), ("obs", "votes"), ("carve_votes", 2, 0), ("obs", "votes")],
    # the labelling and the field: kept by the colour calls, new images, new views and each other's
    # build ...
    # build (the field a labelling built after it, the labelling a field built after it): all three
    # downloads after every one of those calls, before anything is built again ...
    "labelling_field_lifetime": VIEWS + [("carve", 0, 3), ("distance", 1), ("components", 26)] + STATE3 + [
        ("color", 0)] + STATE3 + [("upload_colors", 6)] + STATE3 + [("set_images",)] + STATE3 + [
        ("set_views", 1, NV)] + STATE3 + [("distance", 0)] + STATE3 + [("components", 6)] + STATE3 + [
        # ... dropped by handleUnseen and by the closure.  arvx.h: "the labelling of arvx_components
        # lives until the next call that replaces the state: carve, vote carve, fast carve, photo carve,
        # arvx_handle_unseen, closure, state upload, reset, ..." -- the list names the call, not what
        # it fills: a closure of kernel size 1, which fills nothing, drops both as well
        ("handle_unseen",)] + STATE3 + [
        ("components", 6), ("distance", 0), ("closure", 1, 0), ("obs", "closure_list")] + STATE3 + [
        ("carve", 0, 2), ("components", 6), ("distance", 0), ("closure", 3, 0)] + STATE3 + [
        # a keep leaves no labelling (not even its own), a morph no field
        ("components", 26), ("keep_components", 26, 1, 0), ("obs", "component_table"),
        ("obs", "component_labels"), ("distance", 0), ("morph", OPEN, 0), ("obs", "distance_field")],
    # what handleUnseen occupies and what a closure fills is occupied for the components, the field
    # and the keep
    "unseen_components_distance_keep": UNSEEN_EMPTY + [("handle_unseen",), ("components", 6)] + STATE3[:2] + [
        ("distance", 0), ("obs", "distance_field"), ("keep_components", 6, 10, 1), ("obs", "download_state"),
        ("obs", "mc_cells")],
    "closure_components_distance": VIEWS + [("carve",), ("color", 1), ("closure", 3, 1), ("components", 26)]
                                   + STATE3[:2] + [("distance", 0), ("obs", "distance_field"),
                                                   ("obs", "export_model", 1)],
    # max_iterations 1 stops while voxels are still being removed, 4 stops on an empty sweep
    "color_unseen_photo_closure_1": _photo_after_unseen(60.0, 1),
    "color_unseen_photo_closure_4": _photo_after_unseen(140.0, 4),
}


@pytest.mark.parametrize("name", sorted(STAGE_PINNED))
@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]], ids=["lazy", "packets"])
def test_pinned_stage_sequence(arvx, scenes_by_grid, name, grid):
    run(arvx, scenes_by_grid[grid], STAGE_PINNED[name], f"pinned {name} grid {grid}")


# ---- pinned sequences over the products ---------------------------------------------------------

# state A: the model carved under views 0 and 1; state B: carved under views 2 and 3 as well.  (A carve
# under all views leaves next to nothing on the packet grid.)
A = VIEWS + [("carve", 0, 2)]
TO_B = [("carve", 2, 2)]
R = ("render", 1, 1, 5)    # a camera that is no view, an image size that is not the views', a background
R2 = ("render", 2, 0, None)
SMOOTH = ("smooth", 1, 0.5, -0.53)
HELD3 = [("obs", "welded_held"), ("obs", "smooth_held"), ("obs", "decimate_held")]
HELD = [("obs", "mc_cells_list"), ("obs", "mc_mesh_held")] + HELD3 + [("obs", "refined_held"), ("obs", "render_held")]
EMPTY = ("morph", ERODE, 1 << 20)  # (no voxel is further than that from the grid's border: nothing is left)


def _each(calls, then):
    return [op for call in calls for op in [call] + then]


def _mesh_on_lazy_state(stages, held):
    """As _on_lazy_state: the builds read a lazy state (they change nothing, so they do not end it), and
    what they built is still there after the carve under other views that follows."""
    return [("set_views", 0, 4), ("set_images",), ("carve",)] + stages + held + [
        ("obs", "download_state"), ("obs", "download_packets"), ("set_views", 2, NV), ("carve",),
        ("obs", "download_state")] + held


MESH_PINNED = {
    # The welded mesh and what was made of it are snapshots: after a carve under other views the three
    # downloads still give the old mesh; the render -- it shows the state the mesh was built from -- is
    # gone.  A new render, smooth and decimate act on the old mesh (with the colours it was built with:
    # the colour list went with the carve), and only a new weld ends the three products made of it.
    "weld_outlives_its_state": A + [("color", 1), ("weld", 0), SMOOTH, ("decimate", 2, SMOOTHED), R,
                                    ("obs", "render_held")] + TO_B + HELD3 + [
        ("obs", "render_held"), ("render_view", 0), ("obs", "render_held"), ("smooth", 1, 0.5, -0.53),
        ("obs", "smooth_held"), ("decimate", 3, SMOOTHED), ("obs", "decimate_held"), ("weld", 0),
        ("obs", "smooth_held"), ("obs", "decimate_held"), ("obs", "render_held"), ("obs", "welded_held")],
    # The render's lifetime (arvx.h, the render's last paragraph), in two halves.  Kept by every call that
    # replaces no occupied or seen bit and by arvx_handle_unseen and arvx_closure, each followed by a
    # download with nothing rebuilt ...
    "render_lifetime_kept": A + [("color", 1), ("weld", 0), R] + _each(
        [("color", 0), ("upload_colors", 3), ("color_visible", 1, 1.0), ("set_images",), ("set_views", 1, NV),
         ("set_images",), ("handle_unseen",), ("closure", 3, 0), ("components", 6), ("distance", 0),
         ("mc_cells_build",), ("mc_mesh_build", 0), ("refine", 2, 0), SMOOTH, ("decimate", 2, LATTICE)],
        [("obs", "render_held")]),
    # ... dropped by every call that replaces the state the mesh was built from, each from a fresh
    # render of the held mesh: the keep and the four morph ops as well, which arvx.h did not name
    # before these sequences (the library dropped the render, the paragraph was behind it), and by a
    # new weld
    "render_lifetime_dropped": A + [("weld", 0)] + _each(
        [("carve", 2, 1), ("carve_votes", 2, 0), ("fast_carve",), ("photo_carve", INF, 1, 1.0, 1),
         ("keep_components", 6, 1, 0), ("morph", ERODE, 0), ("morph", DILATE, 1), ("morph", OPEN, 1),
         ("morph", CLOSE, 0), ("upload_state", 5), ("upload_planes", 6), ("reset",), ("weld", 0)],
        [("obs", "render_held"), R2, ("obs", "render_held")]),
    # The smoothing's CSRs are built at the first smooth after a weld from the weld's rank and index
    # buffers: reused by the next smooths, built anew for a mesh of other V and T ...
    "smooth_csr_follows_the_weld": A + [("weld", 0), ("smooth", 1, 0.5, -0.53), ("obs", "smooth_held"),
                                        ("smooth", 10, 0.5, -0.53), ("obs", "smooth_held"), ("smooth", 0, 0.5, -0.53),
                                        ("obs", "smooth_held")] + TO_B + [
        ("weld", 0), SMOOTH, ("obs", "smooth_held"), ("obs", "welded_held")],
    # ... nothing to build for an empty mesh (which smooths, decimates and renders to nothing: the
    # background), and built again for the mesh after it
    "smooth_csr_after_an_empty_mesh": A + [("weld", 0), SMOOTH, EMPTY, ("weld", 0), SMOOTH, ("obs", "smooth_held"),
                                           ("decimate", 2, SMOOTHED), ("obs", "decimate_held"), R, ("obs", "render_held"),
                                           ("obs", "welded_held"), ("reset",), ("carve", 0, 2), ("weld", 0), SMOOTH,
                                           ("obs", "smooth_held"), ("decimate", 2, SMOOTHED), ("obs", "decimate_held")],
    # ARVX_DECIMATE_SMOOTHED needs a smoothed mesh ON THIS welded mesh: refused before any smooth and after
    # a new weld (which also ends the old decimated mesh), accepted in between; after smooth(0) -- the
    # positions are the lattice's -- both sources give the same mesh.
    "decimate_sources": A + [("weld", 0), ("decimate", 2, SMOOTHED), ("obs", "decimate_held"), SMOOTH,
                             ("decimate", 2, SMOOTHED), ("obs", "decimate_held")] + TO_B + [
        ("weld", 0), ("decimate", 2, SMOOTHED), ("obs", "decimate_held"), ("smooth", 0, 0.5, -0.53),
        ("decimate", 3, LATTICE), ("obs", "decimate_held"), ("decimate", 3, SMOOTHED), ("obs", "decimate_held")],
    # The refined mesh is a snapshot of the state AND the views at its call.  The model is carved under
    # five of the eight views and refined under all of them: the edges those five explain are
    # silhouette edges, the ones whose occupied end another view would have carved are not.  New views, a
    # carve, colours, a closure: the download stays what it was.  Fills whose list is gone refuse a new
    # refine, and the old mesh stays.
    "refined_is_a_snapshot": VIEWS + [("carve", 0, 5), ("refine", 6, 0), ("obs", "refined_held"), ("set_views", 2, NV),
                                      ("obs", "refined_held"), ("set_images",), ("carve",), ("obs", "refined_held"),
                                      ("color", 1), ("obs", "refined_held"), ("closure", 3, 0), ("obs", "refined_held"),
                                      ("handle_unseen",), ("refine", 6, 0), ("obs", "refined_held"),
                                      ("obs", "mc_cells_list")],
    # ... and without views: plain midpoints (B = 0) need none, a bisection does
    "refined_without_views": [("refine", 6, 0), ("obs", "refined_held"), ("refine", 0, 0), ("obs", "refined_held"),
                              ("refine", 6, 0), ("obs", "refined_held")],
    # A closure computed with one apply_unseen refuses the three builds with the other, and a refused
    # build leaves every product as it was (arvx_mc_mesh_welded clears four flags once it is past its
    # refusals).
    "refusals_leave_the_products": A + [("color", 1), ("mc_cells_build",), ("mc_mesh_build", 0), ("weld", 0), SMOOTH,
                                        ("decimate", 2, SMOOTHED), ("refine", 2, 0), R, ("closure", 3, 0),
                                        ("weld", 1), ("mc_mesh_build", 1), ("refine", 2, 1)] + HELD,
    # Every compaction hands the chunk counts on through two buffers that take turns, and the refined
    # mesh's edge plane is the one that is longer than the voxel planes: refine, colour, closure, weld,
    # components, decimate, refine, colour, with every held product and list downloaded after each.
    "compactions_take_turns": A + _each(
        [("refine", 2, 0), ("color", 1), ("closure", 3, 0), ("weld", 0), ("components", 6), ("decimate", 2, LATTICE),
         ("refine", 3, 0), ("color", 0)],
        HELD + [("obs", "surface"), ("obs", "closure_list"), ("obs", "component_table")]),
    # arvx_color_visible fills the colour list with the colour list's lifetime: handleUnseen and the
    # closure keep the two downloads, export, weld and render take its colours, a plain colour pass or a
    # colour upload ends them; a photo carve writes the depth buffers it shares, and a new pass follows.
    "visible_colour_lifetime": A + [("color_visible", 1, 1.0), ("obs", "surface"), ("obs", "surface_visible")] + [
        ("obs", "view_depth", v) for v in range(NV)] + [
        ("handle_unseen",), ("obs", "surface_visible"), ("obs", "view_depth", 3), ("closure", 3, 1),
        ("obs", "surface_visible"), ("obs", "view_depth", 0), ("obs", "export_model", 1), ("weld", 1),
        ("obs", "welded_held"), ("render_view", 0), ("obs", "render_held"), ("color", 1), ("obs", "surface_visible"),
        ("obs", "view_depth", 0), ("carve", 2, 1), ("color_visible", 0, 0.0), ("obs", "view_depth", 1),
        ("upload_colors", 4), ("obs", "surface_visible"), ("obs", "view_depth", 1),
        ("photo_carve", 20.0, 2, 1.0, 2), ("obs", "view_depth", 1), ("color_visible", 0, INF), ("obs", "surface"),
        ("obs", "surface_visible"), ("obs", "view_depth", 1)],
    # The cell list is the last cell walk's, whichever entry point ran it; a state change keeps it.
    "cells_follow_the_last_mesh": A + [("mc_cells_build",)] + TO_B + [
        ("obs", "mc_cells_list"), ("weld", 0), ("obs", "mc_cells_list"), ("morph", ERODE, 1), ("obs", "mc_cells_list"),
        ("refine", 0, 0), ("obs", "mc_cells_list"), ("morph", DILATE, 2), ("mc_mesh_build", 0),
        ("obs", "mc_cells_list"), ("obs", "mc_mesh_held"), EMPTY, ("mc_cells_build",), ("obs", "mc_cells_list"),
        ("obs", "mc_mesh_held")],
    "lazy_weld_smooth_decimate_render": _mesh_on_lazy_state(
        [("weld", 0), SMOOTH, ("decimate", 2, SMOOTHED), R], HELD3 + [("obs", "mc_cells_list")]),
    "lazy_refine": _mesh_on_lazy_state([("refine", 4, 0)], [("obs", "refined_held"), ("obs", "mc_cells_list")]),
}


@pytest.mark.parametrize("name", sorted(MESH_PINNED))
@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]], ids=["lazy", "packets"])
def test_pinned_mesh_sequence(arvx, scenes_by_grid, name, grid):
    run(arvx, scenes_by_grid[grid], MESH_PINNED[name], f"pinned {name} grid {grid}", no_fallbacks=True)
