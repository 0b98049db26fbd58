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
