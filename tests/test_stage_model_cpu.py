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
