"""The reference state machines of tests/stage_model.py checked against the oracle: no GPU."""
import numpy as np
import pytest

from tests import stage_model as sm


@pytest.mark.parametrize("dims", [(21, 13, 11), (64, 24, 16), (130, 10, 7)])
def test_closure_any_kernel_3_is_the_oracles(oracle, dims):
    X, Y, Z = dims
    sc = sm.make_scene(oracle, X, Y, Z, seed=3)
    st = oracle.carve(X, Y, Z, sc.s, sc.M[:3], sc.masks[:3])
    model = oracle.color(X, Y, Z, sc.s, sc.M, sc.campos, sc.images, 1, oracle.model_from_state(st))
    model = oracle.handle_unseen(sm.random_state(4, X, Y, Z, paint=False) & 2 | st.reshape(-1), model)
    want = oracle.closure(X, Y, Z, model)
    got = sm.closure_any_kernel(model, X, Y, Z, 3)
    assert (want[:, 3] != model[:, 3]).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(sm.closure_any_kernel(model, X, Y, Z, 1), model)


@pytest.mark.parametrize("dims", [(21, 13, 11), (64, 24, 16)])
def test_host_model_carve_and_handle_unseen_are_the_oracles(oracle, dims):
    X, Y, Z = dims
    sc = sm.make_scene(oracle, X, Y, Z, seed=5)
    st0 = sm.random_state(9, X, Y, Z, paint=False)
    h = sm.HostModel(sc, st0)
    h.carve(0, 3)
    st = oracle.carve(X, Y, Z, sc.s, sc.M[:3], sc.masks[:3], state=st0)
    assert np.array_equal(h.state(), st.reshape(-1))
    assert np.array_equal(h.rgba, oracle.model_from_state(st))
    h.color(0)
    coloured = oracle.color(X, Y, Z, sc.s, sc.M, sc.campos, sc.images, 0, oracle.model_from_state(st))
    assert np.array_equal(h.rgba, coloured)
    h.handle_unseen()
    assert np.array_equal(h.rgba, oracle.handle_unseen(st, coloured))
    # a second carve keeps the colours (and the paint) of the voxels it leaves
    h.carve()
    st2 = oracle.carve(X, Y, Z, sc.s, sc.M, sc.masks, state=h.state() | 0)
    kept = (st2.reshape(-1) & 1) != 0
    assert np.array_equal(h.rgba[kept], oracle.handle_unseen(st, coloured)[kept])
    assert not h.rgba[~kept].any()


def test_ctx_model_export_and_closure_rules(oracle):
    """CtxModel's own bookkeeping: a carve drops the lists and the paint, handleUnseen only the
    closure's, and a second closure is refused until the state is replaced."""
    X, Y, Z = 21, 13, 11
    sc = sm.make_scene(oracle, X, Y, Z, seed=7)
    m = sm.CtxModel(sc)
    m.set_views(0, 8)
    m.set_images()
    m.carve()
    m.color(1)
    idx, rgb = m.surface()
    assert len(idx) > 0
    want = oracle.color(X, Y, Z, sc.s, sc.M, sc.campos, sc.images, 1, oracle.model_from_state(m.st))
    assert np.array_equal(m.export_model(0), want)
    st = m.st.copy()
    m.closure(3, 1)
    assert np.array_equal(m.export_model(1), oracle.closure(X, Y, Z, oracle.handle_unseen(st, want)))
    with pytest.raises(sm.Refused):
        m.export_model(0)
    m.handle_unseen()
    with pytest.raises(sm.Refused):
        m.closure_list()
    with pytest.raises(sm.Refused):  # (the fills' colours are gone)
        m.export_model(1)
    with pytest.raises(sm.Refused):
        m.closure(3, 1)
    m.upload_state(sm.random_state(1, X, Y, Z))
    with pytest.raises(sm.Refused):
        m.surface()
    assert (m.download_state() & 4).any()
    m.closure(3, 0)
    m.carve()
    assert not (m.download_state() & 4).any()


# ---- the stages beyond the reference's pipeline ------------------------------------------------

STAGE_DIMS = [(21, 13, 11), (64, 24, 16)]


def _uploaded(oracle, dims, seed=21):
    """A CtxModel with views and images on a random_state upload, and the bytes of that state."""
    X, Y, Z = dims
    sc = sm.make_scene(oracle, X, Y, Z, seed=seed)
    m = sm.CtxModel(sc)
    m.set_views(1, 7)
    m.set_images()
    st0 = sm.random_state(seed + 1, X, Y, Z, empty_paint=True)
    m.upload_state(st0)
    assert (st0 & 4).any() and ((st0 & 3) == 0).any() and ((st0 & 3) == 1).any()
    return sc, m, st0 & 3


@pytest.mark.parametrize("dims", STAGE_DIMS)
def test_ctx_model_carve_votes_is_the_restatement(oracle, dims):
    from tests import vote_carve
    sc, m, st0 = _uploaded(oracle, dims)
    v = slice(1, 7)
    for max_misses, counts in ((1, True), (0, False)):
        before = m.st.copy()
        want, votes = vote_carve.carve_votes(oracle, *dims, sc.s, sc.M[v], sc.masks[v], max_misses, state=before)
        assert m.carve_votes(max_misses, counts) is None
        assert np.array_equal(m.st, want)
        if counts:
            bg, inside = m.votes()
            assert np.array_equal(bg, votes.background) and np.array_equal(inside, votes.inside)
            assert (want != before).any() and bg.max() > 1
    # max_misses = 0 is the plain carve
    assert np.array_equal(m.st, oracle.carve(*dims, sc.s, sc.M[v], sc.masks[v], state=st0).reshape(-1))


@pytest.mark.parametrize("dims", STAGE_DIMS)
def test_ctx_model_photo_carve_is_the_restatement(oracle, dims):
    from tests import photo_carve
    sc, m, st0 = _uploaded(oracle, dims)
    v = slice(1, 7)
    for max_std, min_views, tol_voxels, iters in ((60.0, 2, 1.0, 2), (20.0, 1, 0.0, 1), (0.0, 3, float("inf"), 4)):
        before = m.st.copy()
        want = photo_carve.photo_carve(*dims, sc.s, sc.M[v], sc.images[v], before, max_std, min_views,
                                       np.float32(tol_voxels) * sc.s, iters)
        assert m.photo_carve(max_std, min_views, tol_voxels, iters) == (want.iterations, want.removed)
        assert np.array_equal(m.st, want.state)
        assert want.removed > 0
    assert m.photo_carve(float("inf"), 1, 1.0, 4) == (1, 0)


@pytest.mark.parametrize("dims", STAGE_DIMS)
def test_ctx_model_components_are_the_restatement(oracle, dims):
    from tests import components
    sc, m, st0 = _uploaded(oracle, dims)
    for conn in (6, 26):
        vl = components.labels(st0, dims, conn)
        lab, size = components.table(vl)
        assert m.components(conn) == len(lab) >= 2
        assert np.array_equal(m.component_labels(), vl)
        got = m.component_table()
        assert np.array_equal(got[0], lab) and np.array_equal(got[1], size)
        assert np.array_equal(m.st, st0)  # (nothing changes)
    for conn, min_voxels, largest in ((6, 10, False), (26, 1, True)):
        m.upload_state(st0)
        before = m.st.copy()
        want, kept, removed = components.keep(before, dims, conn, min_voxels, largest)
        assert m.keep_components(conn, min_voxels, largest) == (kept, removed)
        assert removed > 0 and np.array_equal(m.st, want)


@pytest.mark.parametrize("dims", STAGE_DIMS)
def test_ctx_model_distance_and_morph_are_the_restatement(oracle, dims):
    from tests import distance
    sc, m, st0 = _uploaded(oracle, dims)
    for border in (False, True):
        assert m.distance(border) is None
        assert np.array_equal(m.distance_field(), distance.signed_sq(st0, dims, border))
        assert np.array_equal(m.st, st0)
    for op, radius_sq in ((distance.OPEN, 1), (distance.CLOSE, 2), (distance.DILATE, 3), (distance.ERODE, 9),
                          (distance.DILATE, 0)):
        before = m.st.copy()
        want, removed, added = distance.morph(before, dims, op, radius_sq)
        assert m.morph(op, radius_sq) == (removed, added)
        assert np.array_equal(m.st, want)
        assert (removed + added > 0) == (radius_sq > 0)


def _refused(fn, *args):
    with pytest.raises(sm.Refused):
        fn(*args)


def _results(m):
    """Which of (vote counts, labelling -- both of its downloads --, field) the model delivers."""
    out = []
    for obs in (m.votes, m.component_table, m.component_labels, m.distance_field):
        try:
            obs()
            out.append(True)
        except sm.Refused:
            out.append(False)
    assert out[1] == out[2]
    return out[0], out[1], out[3]


def test_ctx_model_stage_result_lifetimes(oracle):
    """The vote counts, the labelling and the field, call by call as arvx.h has it (arvx_carve_votes:
    ARVX_VOTES_COUNTS; arvx_components: "The labelling of arvx_components lives until ..."; arvx_distance:
    "lives exactly as long as the labelling")."""
    X, Y, Z = 21, 13, 11
    sc = sm.make_scene(oracle, X, Y, Z, seed=7)
    m = sm.CtxModel(sc)
    assert _results(m) == (False, False, False)
    _refused(m.carve_votes, 1, True)  # no views
    m.set_views(0, 8)
    _refused(m.photo_carve, 20.0, 1, 1.0, 1)  # no images
    m.set_images()

    def build():
        m.upload_state(sm.random_state(3, X, Y, Z))
        m.carve_votes(2, True)
        m.components(6)
        m.distance(False)
        assert _results(m) == (True, True, True)

    build()  # ... and the builds keep each other's results
    m.components(26)
    m.distance(True)
    assert _results(m) == (True, True, True)
    # the calls that replace neither the state nor the views keep all three
    m.set_images()
    assert _results(m) == (True, True, True)
    m.color(1)
    assert _results(m) == (True, True, True)
    m.upload_colors(*m.resolve("upload_colors", (5,)))
    assert _results(m) == (True, True, True)
    # new views: the counts are sums over the views, the other two describe the occupancy alone
    m.set_views(2, 8)
    assert _results(m) == (False, True, True)
    m.set_images()
    # handleUnseen and the closure -- one that fills nothing too: arvx.h lists the call -- drop all three
    build()
    m.handle_unseen()
    assert _results(m) == (False, False, False)
    build()
    m.closure(1, 0)
    assert len(m.closure_list()[0]) == 0 and _results(m) == (False, False, False)
    build()
    m.closure(3, 0)
    assert len(m.closure_list()[0]) > 0 and _results(m) == (False, False, False)
    # every call that replaces the state drops all three, the new stages among them: a vote carve
    # without counts leaves none, a keep no labelling, a morph no field
    for call in (lambda: m.carve(), lambda: m.carve(0, 2), lambda: m.fast_carve(), lambda: m.reset(),
                 lambda: m.upload_state(sm.random_state(4, X, Y, Z)),
                 lambda: m.upload_planes(*m.resolve("upload_planes", (4,))),
                 lambda: m.carve_votes(1, False), lambda: m.photo_carve(float("inf"), 1, 1.0, 1),
                 lambda: m.keep_components(6, 1, False), lambda: m.morph(0, 0), lambda: m.morph(1, 0),
                 lambda: m.morph(2, 0), lambda: m.morph(3, 0)):
        build()
        call()
        assert _results(m) == (False, False, False)
    build()
    m.carve_votes(1, True)
    assert _results(m) == (True, False, False)


STAGE_CALLS = {"carve_votes": (65535, False), "photo_carve": (float("inf"), 1, 1.0, 1),
               "keep_components": (6, 1, False), "erode": (0, 0), "dilate": (1, 0), "open": (2, 0), "close": (3, 0)}


def _stage(m, name):
    return getattr(m, name if name in ("carve_votes", "photo_carve", "keep_components") else "morph")(*STAGE_CALLS[name])


@pytest.mark.parametrize("name", sorted(STAGE_CALLS))
def test_ctx_model_stage_drops_and_fills(oracle, name):
    """Each state-changing stage, with arguments under which it changes no voxel: the paint plane,
    the colour list, the closure's list and the mark of its fills go all the same; all but the vote
    carve are refused on fills whose list is gone and change nothing then."""
    X, Y, Z = 21, 13, 11
    sc = sm.make_scene(oracle, X, Y, Z, seed=7)
    m = sm.CtxModel(sc)
    m.set_views(0, 8)
    m.set_images()
    m.upload_state(sm.random_state(1, X, Y, Z, empty_paint=True))
    m.color(0)
    m.closure(3, 0)
    assert (m.download_state() & 4).any() and len(m.surface()[0]) and len(m.closure_list()[0]) and m.fills
    occ = m.st & 1
    _stage(m, name)
    assert np.array_equal(m.st & 1, occ)                   # no voxel changed (the fills are occupancy now)
    assert not (m.download_state() & 4).any()              # the paint plane
    assert not (m.export_model(0)[:, :3] == sm.UNSEEN_COLOR[:3]).all(axis=1).any()
    _refused(m.surface)                                    # the colour list
    _refused(m.closure_list)                               # the closure's list
    assert not m.fills
    m.closure(3, 0)                                        # ... so a second closure is defined again
    # the fills without their list
    m.handle_unseen()
    _refused(m.closure_list)
    before = m.download_state()
    if name == "carve_votes":
        _stage(m, name)  # (a carve: never refused for the fills, and it ends them)
        m.export_model(0)
    else:
        _refused(_stage, m, name)
        assert np.array_equal(m.download_state(), before) and m.fills
        _refused(m.export_model, 0)
        m.carve()
        _stage(m, name)
    if name != "carve_votes":
        assert not m.fills  # (refused while they were there, accepted after the carve)


# ---- the sequences tests/test_stage_sequences_gpu.py replays on the device --------------------

def test_old_random_sequences_are_unchanged():
    """random_ops over SEEDS: the 48 op lists of the commit before the stage generator was added
    (sha256 of their repr, computed with that commit's code)."""
    import hashlib
    from tests import test_stage_sequences_gpu as seq
    assert len(seq.SEEDS) == 48
    lists = [seq.random_ops(s, g[0], g[1]) for g, s in seq.SEEDS]
    assert hashlib.sha256(repr(lists).encode()).hexdigest() == \
        "e2063ccc71fbc231a2277e8e4d36edba876b06701891f58b48c0ec13f0b4539b"


def test_random_stage_sequences_census(oracle):
    """The model alone over every sequence of random_stage_ops: the new stages must have something to
    do and the new results must be both delivered and refused, or the device test compares nothing.
    Conditions on the generator's weights, arguments and seeds, not measurements: each at least 5
    times over the 48 sequences.  (The four grids of GRIDS are enough: uploads and tolerant vote carves
    give the two grids that carve down to nothing their material.)"""
    from collections import Counter
    from tests import test_stage_sequences_gpu as seq
    scenes = {g: sm.make_scene(oracle, *g, seed=sum(g)) for g in seq.STAGE_GRIDS}
    n = Counter()
    morph = {0: "erode", 1: "dilate", 2: "open", 3: "close"}
    for grid, seed in seq.STAGE_SEEDS:
        ops = seq.random_stage_ops(seed, grid[0], grid[1])
        assert ops[-2] == ("obs", "download_state") and ops[-1][:2] == ("obs", "export_model")
        m = sm.CtxModel(scenes[grid])
        for op in ops:
            name, args = op[0], op[1:]
            if name == "obs":
                if args[0] not in seq.STAGE_OBS:
                    continue  # (the old observations change nothing in the model)
                # (whether the field is there, not the field: its restatement is the slow one)
                delivered = (m.field is not None) if args[0] == "distance_field" else None
                if delivered is None:
                    try:
                        getattr(m, args[0])()
                        delivered = True
                    except sm.Refused:
                        delivered = False
                n[args[0], "delivered" if delivered else "refused"] += 1
                continue
            occ = m.st & 1
            try:
                ret = getattr(m, name)(*m.resolve(name, args))
            except sm.Refused:
                continue
            changed = int((occ != (m.st & 1)).sum())
            if name == "carve_votes":
                n["vote carve empties"] += changed > 0
            elif name == "photo_carve":
                assert ret[1] == changed
                n["photo carve removes"] += changed > 0
            elif name == "keep_components":
                assert ret[1] == changed
                n["keep removes"] += changed > 0
            elif name == "morph":
                assert sum(ret) == changed
                n[morph[args[0]], "changes"] += changed > 0
            elif name == "components":
                n["two components"] += ret >= 2
    print(sorted(n.items(), key=str))
    wanted = ["vote carve empties", "photo carve removes", "keep removes", "two components"]
    wanted += [(op, "changes") for op in morph.values()]
    wanted += [(obs, how) for obs in seq.STAGE_OBS for how in ("delivered", "refused")]
    assert {k: n[k] for k in wanted if n[k] < 5} == {}


@pytest.mark.parametrize("grid", ["lazy", "packets"])
def test_pinned_stage_sequences_do_what_they_say(oracle, grid):
    """STAGE_PINNED on the model alone, on both of its grids: the refusals, the lifetimes and the
    effects a sequence is there for happen in it.  A change of make_scene that left a closure nothing
    to fill, handleUnseen nothing to occupy or a stage nothing to remove would otherwise empty the
    device test without failing it."""
    from tests import photo_carve
    from tests import test_stage_sequences_gpu as seq
    refused = {"fills_with_list_keep": [6, 7], "fills_without_list": [5, 6, 7, 8],
               "labelling_field_lifetime": [33, 34, 35, 40, 41, 42, 47, 48, 49, 52, 53, 56],
               "votes_lifetime": [11, 14, 18, 22]}
    dims = seq.GRIDS[0] if grid == "lazy" else seq.GRIDS[1]
    sc = sm.make_scene(oracle, *dims, seed=sum(dims))
    for name, ops in seq.STAGE_PINNED.items():
        m = sm.CtxModel(sc)
        got, changed, ret = [], {}, {}
        for step, op in enumerate(ops):
            occ = m.st & 1
            try:
                if op[0] == "obs":
                    getattr(m, op[1])(*op[2:])
                    continue
                ret[step] = getattr(m, op[0])(*m.resolve(op[0], op[1:]))
            except sm.Refused:
                got.append(step)
                continue
            changed[step] = int((occ != (m.st & 1)).sum())
            if op[0] == "closure" and op[1] >= 3:
                assert changed[step] > 0, (name, step, "the closure fills nothing")
            if op[0] == "photo_carve" and name == "color_unseen_photo_closure_1":
                # stopped by max_iterations while voxels were still being removed
                more = photo_carve.photo_carve(*dims, sc.s, sc.M, sc.images, m.st & 3, op[1], op[2],
                                               np.float32(op[3]) * sc.s, 1)
                assert ret[step][0] == 1 and ret[step][1] > 0 and more.removed > 0, (name, ret[step])
            if op[0] == "photo_carve" and name == "color_unseen_photo_closure_4":
                assert 1 < ret[step][0] < 4 and ret[step][1] > 0, (name, ret[step])  # stopped by an empty sweep
        assert got == refused.get(name, []), name
        assert all(ops[s][0] == "obs" or name == "fills_without_list" for s in got)
        where = lambda opname: [s for s, op in enumerate(ops) if op[0] == opname and s in changed]
        if ops[:len(seq.UNSEEN_EMPTY)] == seq.UNSEEN_EMPTY:
            assert all(changed[s] > 0 for s in where("handle_unseen")), (name, "handleUnseen occupies nothing")
        # (lazy_closure_keep_closure: the closed model of the lazy grid is one component; its keep is
        # there to write out the tiles the closure left as codes, not to remove anything)
        if name.startswith("lazy_") and name not in ("lazy_components_distance", "lazy_closure_keep_closure"):
            # the stage on the lazy state changes voxels, and so does the carve under other views after it
            stage = [s for s in changed if ops[s][0] in ("carve_votes", "photo_carve", "keep_components", "morph")]
            assert stage and all(changed[s] > 0 for s in stage), (name, changed)
            if "closure" not in name:
                assert changed[where("carve")[-1]] > 0, name
        if name == "fills_without_list":  # (once accepted, each of the three does something)
            assert all(changed[s] > 0 for s in changed if s > 9), (name, changed)
        if name == "unseen_components_distance_keep":
            assert ret[where("components")[0]] >= 2 and changed[where("keep_components")[0]] > 0


# ---- the products: meshes, render, visible colour ----------------------------------------------

def _bits_equal(a, b):
    from tests.test_stage_sequences_gpu import equal
    return equal(a, b)


@pytest.mark.parametrize("dims", STAGE_DIMS)
def test_ctx_model_products_are_the_restatements(oracle, dims):
    """Each build of CtxModel against its stage's own restatement applied by hand to the state, the
    views and the colours of the moment."""
    from tests import mesh_decimate, mesh_refine, mesh_smooth, mesh_weld, visibility
    from tests import render as rnd
    X, Y, Z = dims
    sc, m, st0 = _uploaded(oracle, dims)
    v = slice(1, 7)
    # the visible colour pass fills the colour list
    m.color_visible(1, 1.0)
    base = oracle.model_from_state(st0)
    vis = visibility.color_visible(X, Y, Z, sc.s, sc.M[v], sc.campos[v], sc.images[v], 1, base, np.float32(1.0) * sc.s)
    idx, rgb = m.surface()
    assert len(idx) > 0 and np.array_equal(idx, vis.index[vis.has]) and _bits_equal(rgb, vis.rgba[idx, :3])
    assert np.array_equal(m.surface_visible(), vis.views[vis.has]) and 0 < (m.surface_visible() > 0).mean() < 1
    assert all(_bits_equal(m.view_depth(k), vis.zbuf[k]) for k in range(6))
    assert (vis.rgba[idx, :3] != oracle.color(X, Y, Z, sc.s, sc.M[v], sc.campos[v], sc.images[v], 1, base)[idx, :3]).any()
    model = m.export_model(1)
    model[(st0 & 1) == 0] = 0  # (the meshes take the occupied voxels in export_model's colours)
    # cells, unwelded and welded mesh
    occ = np.zeros((X * Y * Z, 4), np.float32)
    occ[:, 3] = st0 & 1
    assert m.mc_cells_build() == len(oracle.mc_cells(X, Y, Z, occ)) > 0
    assert np.array_equal(m.mc_cells_list(), oracle.mc_cells(X, Y, Z, occ))
    verts, frgb = oracle.mc_mesh(X, Y, Z, model)
    assert m.mc_mesh_build(1) == len(frgb) > 0 and _bits_equal(m.mc_mesh_held(), (verts, frgb))
    wv, wf, wrgb = mesh_weld.weld(verts, frgb)
    assert m.weld(1) == (len(wv), len(wf))
    index = mesh_weld.lattice_index(wv, X, Y)
    vrgb = model[index, :3]
    assert _bits_equal(m.welded_held(), (wv, wf, wrgb, vrgb))
    assert len(np.unique(vrgb, axis=0)) > 3  # (the pass's colours, the paint and MODEL_COLOR)
    # smoothing (twice: the second from the kept structures), decimation from both sources
    for iterations, lam, mu in ((2, 0.5, -0.53), (1, 0.33, 0.0)):
        m.smooth(iterations, lam, mu)
        want = mesh_smooth.smooth(wv, wf, iterations, lam, mu)
        assert _bits_equal(m.smooth_held(), want) and (want[0] != wv).any()
    records = np.concatenate([wf, wrgb], axis=1)
    for cell, source in ((2, 0), (3, 1)):
        d = mesh_decimate.decimate(wv, records, cell, want[0] if source else None, vrgb)
        assert m.decimate(cell, source) == (len(d["verts"]), len(d["records"]))
        assert 0 < len(d["verts"]) < len(wv)
        assert _bits_equal(m.decimate_held(), (d["verts"], d["records"], d["rgb"], d["members"], d["map"]))
    # the refined mesh under the views of the moment
    r = mesh_refine.refine((st0 & 1).astype(bool).reshape(Z, Y, X), sc.s, sc.M[v], sc.masks[v], 6,
                           rgb=model[:, :3].reshape(Z, Y, X, 3))
    assert m.refine(6, 1) == (len(r["verts"]), len(r["faces"]))
    got = m.refined_held()
    assert _bits_equal(got[0], r["verts"]) and np.array_equal(got[1][:, :3], r["faces"])
    assert np.array_equal(got[1][:, 3:], r["face_rgb"]) and np.array_equal(got[1][:, 3:], frgb)
    assert _bits_equal(got[2], r["vertex_rgb"]) and np.array_equal(got[3], r["edges"]) and np.array_equal(got[4], r["cut"])
    assert 0 < r["silhouette"].mean() < 1
    # the renders: a camera of its own on both sizes, with and without a background; a view; the agreement
    for cam, size, bg in ((0, 0, None), (3, 1, 9)):
        M, W, H, back = m.resolve("render", (cam, size, bg))
        assert (W, H) == m.RENDER_SIZES[size] and not any(np.array_equal(M, Mv) for Mv in sc.M)
        m.render(M, W, H, back)
        want = rnd.render(M, sc.s, index, vrgb, X, Y, W, H, back)
        assert _bits_equal(m.render_held(), tuple(want)) and (want.id >= 0).any() and (want.id < 0).any()
        assert bg is None or (want.bgr[want.id < 0] == back[want.id < 0]).all()
    assert m.RENDER_SIZES[1] != sc.masks.shape[2:0:-1] == m.RENDER_SIZES[0]
    m.render_view(2)
    want = rnd.render(sc.M[3], sc.s, index, vrgb, X, Y, sc.masks.shape[2], sc.masks.shape[1])
    assert _bits_equal(m.render_held(), tuple(want))
    assert m.render_agreement(4) == rnd.agreement(
        rnd.render(sc.M[5], sc.s, index, vrgb, X, Y, sc.masks.shape[2], sc.masks.shape[1]).id, sc.masks[5])


def _held(m):
    """Which products the model delivers: cells, welded, smoothed, decimated, refined, render, visible."""
    out = []
    for obs in (m.mc_cells_list, m.welded_held, m.smooth_held, m.decimate_held, m.refined_held, m.render_held,
                m.surface_visible):
        try:
            obs()
            out.append(True)
        except sm.Refused:
            out.append(False)
    try:
        m.view_depth(0)
        assert out[-1]
    except sm.Refused:
        assert not out[-1]
    return tuple(out)


def test_ctx_model_product_lifetimes(oracle):
    """The products call by call as arvx.h has it: arvx_mc_cells ("The list is a snapshot ..."), arvx_mc_mesh,
    arvx_mc_mesh_welded ("It lives until the next arvx_mc_mesh_welded ..."), arvx_mc_mesh_smooth, arvx_mc_mesh_decimate
    ("lives until the next arvx_mc_mesh_decimate or the next arvx_mc_mesh_welded"), arvx_mc_mesh_refined ("a snapshot of the
    state and the views"), the render's last paragraph and arvx_color_visible ("with the same lifetime")."""
    X, Y, Z = 21, 13, 11
    sc = sm.make_scene(oracle, X, Y, Z, seed=7)
    m = sm.CtxModel(sc)
    assert _held(m) == (False,) * 7 and len(m.mc_mesh_held()[1]) == 0
    for call in (lambda: m.smooth(1, 0.5, -0.53), lambda: m.decimate(2, 0), lambda: m.render_view(0),
                 lambda: m.render(*m.resolve("render", (0, 0, None))), lambda: m.refine(1, 0),
                 lambda: m.color_visible(0, 1.0)):
        _refused(call)  # no welded mesh, no views
    assert m.refine(0, 0)[0] > 0  # (B = 0 needs no views)
    m.set_views(0, 8)
    m.set_images()
    ALL = (True,) * 7

    def build():
        m.upload_state(sm.random_state(3, X, Y, Z))
        m.color_visible(1, 1.0)
        m.mc_mesh_build(0)
        m.weld(0)
        m.smooth(1, 0.5, -0.53)
        m.decimate(2, 1)
        m.refine(2, 0)
        m.render_view(1)
        assert _held(m) == ALL
        return [m.mc_cells_list(), m.mc_mesh_held(), m.welded_held(), m.smooth_held(), m.decimate_held(),
                m.refined_held()]

    def same(snapshot):
        now = [m.mc_cells_list(), m.mc_mesh_held(), m.welded_held(), m.smooth_held(), m.decimate_held(), m.refined_held()]
        return all(_bits_equal(a, b) for a, b in zip(snapshot, now))

    # kept by everything that replaces no bit of the state; the colour calls end the visible result only
    snap = build()
    for call, visible in ((lambda: m.components(6), True), (lambda: m.distance(0), True), (lambda: m.handle_unseen(), True),
                          (lambda: m.closure(3, 0), True), (lambda: m.color(1), False),
                          (lambda: m.upload_colors(*m.resolve("upload_colors", (5,))), False),
                          (lambda: m.set_images(), False), (lambda: m.set_views(1, 8), False)):
        call()
        assert _held(m) == ALL[:6] + (visible,) and same(snap)
    m.set_images()
    # every call that replaces the state ends the render and the visible result and nothing else; the
    # meshes and the cell list are still those of the state before
    for call in (lambda: m.carve(), lambda: m.carve(0, 2), lambda: m.fast_carve(), lambda: m.reset(),
                 lambda: m.upload_state(sm.random_state(4, X, Y, Z)),
                 lambda: m.upload_planes(*m.resolve("upload_planes", (4,))),
                 lambda: m.carve_votes(1, False), lambda: m.photo_carve(float("inf"), 1, 1.0, 1),
                 lambda: m.keep_components(6, 1, False), lambda: m.morph(0, 0), lambda: m.morph(1, 0),
                 lambda: m.morph(2, 0), lambda: m.morph(3, 0)):
        snap = build()
        call()
        assert _held(m) == (True, True, True, True, True, False, False) and same(snap)
        m.render_view(0)  # (the held mesh is still there to be drawn)
        assert _held(m)[5]
    # a new weld ends what was made of the old one; the unwelded and the refined mesh stay
    snap = build()
    m.carve(0, 2)
    m.weld(0)
    assert _held(m) == (True, True, False, False, True, False, False)
    assert _bits_equal(snap[1], m.mc_mesh_held()) and _bits_equal(snap[5], m.refined_held())
    assert not _bits_equal(snap[2], m.welded_held()) and not _bits_equal(snap[0], m.mc_cells_list())
    _refused(m.decimate, 2, 1)  # no smoothed mesh on this welded mesh
    m.decimate(2, 0)
    m.smooth(0, 0.5, -0.53)
    lattice = m.decimate_held()
    m.decimate(2, 1)
    assert _bits_equal(lattice, m.decimate_held())
    # each mesh call runs the cell walk; the other products do not care
    for k, call in enumerate((lambda: m.mc_mesh_build(0), lambda: m.refine(0, 0), lambda: m.weld(0),
                              lambda: m.mc_cells_build())):
        m.upload_state(sm.random_state(30 + k, X, Y, Z))
        before = m.mc_cells_list()
        call()
        assert len(m.mc_cells_list()) > 0 and not np.array_equal(before, m.mc_cells_list())
    # refusals leave everything: the other apply_unseen after a closure, fills without their list
    snap = build()
    m.closure(3, 1)
    for call in (lambda: m.weld(0), lambda: m.mc_mesh_build(0), lambda: m.refine(2, 0)):
        _refused(call)
        assert _held(m) == ALL and same(snap)
    m.handle_unseen()  # (the list goes, the fills stay)
    for call in (lambda: m.weld(1), lambda: m.mc_mesh_build(1), lambda: m.refine(2, 1)):
        _refused(call)
        assert _held(m) == ALL and same(snap)


def test_old_random_stage_sequences_are_unchanged():
    """random_stage_ops over STAGE_SEEDS: the 48 op lists of the commit before the mesh generator was added
    (sha256 of their repr, computed with that commit's code)."""
    import hashlib
    from tests import test_stage_sequences_gpu as seq
    assert len(seq.STAGE_SEEDS) == 48
    lists = [seq.random_stage_ops(s, g[0], g[1]) for g, s in seq.STAGE_SEEDS]
    assert hashlib.sha256(repr(lists).encode()).hexdigest() == \
        "da7c07e2556f99d9c4b410e65769f870992d326127f54421c24e1a6adad3c0c1"


def _replay_on_model(sc, ops, at=None):
    """ops on a fresh CtxModel -> (the model, the refused steps, what each accepted call returned);
    at(step, op, model) is called before each step."""
    m = sm.CtxModel(sc)
    refused, ret = [], {}
    for step, op in enumerate(ops):
        if at is not None:
            at(step, op, m)
        try:
            if op[0] == "obs":
                getattr(m, op[1])(*op[2:])
            else:
                ret[step] = getattr(m, op[0])(*m.resolve(op[0], op[1:]))
        except sm.Refused:
            refused.append(step)
    return m, refused, ret


@pytest.mark.parametrize("grid", ["lazy", "packets"])
def test_pinned_mesh_sequences_do_what_they_say(oracle, grid):
    """MESH_PINNED on the model alone, on both of its grids: what is refused where, that a held product
    is NOT what a fresh build would give once the state has moved on (or the device test could not
    tell a snapshot from a rebuild), and that the meshes have something in them."""
    import copy
    from tests import test_stage_sequences_gpu as seq
    refused = {"weld_outlives_its_state": [13, 21, 22, 23],
               "render_lifetime_dropped": list(range(5, 57, 4)),
               "decimate_sources": [4, 5, 11, 12],
               "refined_is_a_snapshot": [15],
               "refined_without_views": [0, 1, 4],
               "refusals_leave_the_products": [12, 13, 14],
               "visible_colour_lifetime": [26, 27, 32, 33, 35]}
    # (sequence, step of a held download, the build a rebuild would have made): they differ
    moved = [("weld_outlives_its_state", 10, ("weld", 0)), ("weld_outlives_its_state", 11, ("smooth", 1, 0.5, -0.53)),
             ("refined_is_a_snapshot", 6, ("refine", 6, 0)), ("refined_is_a_snapshot", 9, ("refine", 6, 0)),
             ("refined_is_a_snapshot", 11, ("refine", 6, 0)), ("refined_is_a_snapshot", 13, ("refine", 6, 0)),
             ("cells_follow_the_last_mesh", 5, ("mc_cells_build",)), ("cells_follow_the_last_mesh", 9, ("mc_cells_build",)),
             ("refusals_leave_the_products", 15, ("mc_cells_build",)),
             ("lazy_weld_smooth_decimate_render", 16, ("weld", 0)), ("lazy_refine", 11, ("refine", 4, 0))]
    dims = seq.GRIDS[0] if grid == "lazy" else seq.GRIDS[1]
    sc = sm.make_scene(oracle, *dims, seed=sum(dims))
    for name, ops in seq.MESH_PINNED.items():
        differs = {}

        def at(step, op, m):
            for n, s, build in moved:
                if n == name and s == step:
                    assert op[0] == "obs", (name, step, op)
                    held = getattr(m, op[1])()
                    fresh = copy.copy(m)
                    if build[0] == "smooth":  # (on a weld of the state as it is now)
                        fresh.weld(0)
                    getattr(fresh, build[0])(*build[1:])
                    differs[step] = not _bits_equal(held, getattr(fresh, op[1])())

        m, got, ret = _replay_on_model(sc, ops, at)
        if name == "compactions_take_turns":  # (every download, before its build and after)
            assert all(ops[s][0] == "obs" for s in got) and 20 < len(got) < 40, (name, got)
        else:
            assert got == refused.get(name, []), (name, got)
        assert all(differs.values()) and len(differs) == sum(n == name for n, _, _ in moved), (name, differs)
        for step, r in ret.items():  # every weld but the empty ones, every refine, every decimate builds something
            after_empty = seq.EMPTY in ops[:step] and ("reset",) not in ops[ops.index(seq.EMPTY):step]
            if ops[step][0] in ("weld", "refine", "decimate", "mc_mesh_build", "mc_cells_build") and not after_empty:
                assert min(r) > 0 if isinstance(r, tuple) else r > 0, (name, step, ops[step], r)
            if ops[step][0] in ("weld", "decimate", "mc_cells_build") and after_empty:
                assert r == (0, 0) or r == 0, (name, step, r)
        if name == "refined_is_a_snapshot":
            sil = m.refined[5]
            assert len(sil) > 100 and 0.05 <= sil.mean() <= 0.95, (name, len(sil), sil.mean())
        if name == "smooth_csr_follows_the_weld":  # (weld B has another V and T)
            welds = [ret[s] for s in ret if ops[s][0] == "weld"]
            assert welds[0][0] != welds[1][0] and welds[0][1] != welds[1][1], welds
        if name == "decimate_sources":  # (after smooth(0) both sources give the same mesh)
            assert ret[14] == ret[16] and ops[14][:2] == ops[16][:2] == ("decimate", 3)
        if name == "smooth_csr_after_an_empty_mesh":
            empty = [s for s in ret if ops[s] == ("weld", 0) and ret[s] == (0, 0)]
            assert len(empty) == 1 and ret[max(s for s in ret if ops[s] == ("weld", 0))][0] > 0


REPLACES_BITS = ("carve", "fast_carve", "carve_votes", "photo_carve", "keep_components", "morph", "upload_state",
                 "upload_planes", "reset", "handle_unseen", "closure")


def mesh_census(scenes):
    """The model alone over the 48 sequences of random_mesh_ops -> Counter of SEQUENCES in which a thing
    happens (downloads are counted one by one where the name says so)."""
    from collections import Counter
    from tests import test_stage_sequences_gpu as seq
    n = Counter()
    for grid, seed in seq.MESH_SEEDS:
        ops = seq.random_mesh_ops(seed, grid[0], grid[1])
        m = sm.CtxModel(scenes[grid])
        here = Counter()
        replaced_at = weld_at = -1
        smooths = 0        # smooths of the held, non-empty welded mesh
        rendered = False   # a render has been built in this sequence
        for step, op in enumerate(ops):
            name, args = op[0], op[1:]
            try:
                if name == "obs":
                    getattr(m, args[0])(*args[1:])
                    ret = None
                else:
                    ret = getattr(m, name)(*m.resolve(name, args))
            except sm.Refused:
                if name == "decimate" and args[1] == 1 and m.welded is not None:
                    here["decimate SMOOTHED refused"] += 1
                if op == ("obs", "render_held") and rendered:
                    here["render downloads refused after a drop"] += 1
                if op == ("obs", "surface_visible"):
                    here["surface_visible refused"] += 1
                continue
            if name in REPLACES_BITS:
                replaced_at = step
            welded = name == "weld" or op[:2] == ("obs", "mc_mesh_welded")
            if welded:
                weld_at, smooths = step, 0
                here["weld a non-empty mesh"] += len(m.welded["verts"]) > 0
            if op[:2] in (("obs", "welded_held"), ("obs", "smooth_held"), ("obs", "decimate_held")):
                here["download a mesh after the state was replaced"] += replaced_at > weld_at and len(m.welded["verts"]) > 0
            if name == "smooth" and len(m.welded["verts"]) > 0:
                smooths += 1
                here["smooth a non-empty mesh"] += 1
                here["smooth it twice"] += smooths == 2
            if name == "decimate" and args[1] == 1:
                here["decimate SMOOTHED"] += 1
            if name in ("render", "render_view", "render_agreement"):
                rendered = True
            if op == ("obs", "render_held"):
                here["render downloads delivered"] += 1
            if name == "refine" and ret[0] > 100:
                here["refined > 100 vertices"] += 1
                here["refined with both edge classes"] += bool(m.refined[5].any() and not m.refined[5].all())
            if op == ("obs", "surface_visible"):
                here["surface_visible delivered"] += 1
        for k, c in here.items():
            per_download = k.startswith("render downloads") or k.startswith("surface_visible") or k.startswith("decimate")
            n[k] += c if per_download else c > 0
    return n


MESH_CENSUS = {"weld a non-empty mesh": 12, "download a mesh after the state was replaced": 8,
               "smooth a non-empty mesh": 6, "smooth it twice": 3, "decimate SMOOTHED": 4,
               "decimate SMOOTHED refused": 3, "render downloads delivered": 6,
               "render downloads refused after a drop": 6, "refined > 100 vertices": 5,
               "refined with both edge classes": 2, "surface_visible delivered": 5, "surface_visible refused": 3}


def test_random_mesh_sequences_census(oracle):
    """Conditions on random_mesh_ops' weights, arguments and seeds, on the model alone: the builds have
    something to build and the held products are both delivered and refused, or the device test
    compares nothing.  A miss is mended in the generator, not here."""
    from tests import test_stage_sequences_gpu as seq
    scenes = {g: sm.make_scene(oracle, *g, seed=sum(g)) for g in seq.GRIDS}
    n = mesh_census(scenes)
    print(sorted(n.items()))
    assert {k: (n[k], least) for k, least in MESH_CENSUS.items() if n[k] < least} == {}
