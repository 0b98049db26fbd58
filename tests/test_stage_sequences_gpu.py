"""Orders of calls on one whole-grid context against tests/stage_model.CtxModel: every
intermediate observation bit for bit, every refusal (ARVX_ERR_STATE) where arvx.h says so.

The device keeps caches between calls -- the lazy coarse-tile codes, the colour pass's bit planes,
the state packets, the colour / closure lists, the paint plane, the carve's tile summaries -- and a
fixed carve -> colour -> handleUnseen -> closure chain on a fresh context never asks whether they
are still valid for the next call.  Random sequences do, and the pinned ones keep the cases that
once went wrong (or were found by reading the code) from coming back."""
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
        lo, hi = self.views if self.views else (0, NV)
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
        return self._call(self.ctx.mc_mesh, bool(apply_unseen))

    def mc_mesh_welded(self, apply_unseen):
        return self._call(self.ctx.mc_mesh_welded, bool(apply_unseen))


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


def equal(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 or b.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    return a.shape == b.shape and np.array_equal(a, b)


def run(arvx, sc, ops, label, lib_path=None):
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
