"""The oracle (oracle/arvx_oracle.c, tests/stage_model.py) against the reference program's OWN
code: oracle/_ref/arvx_ref is the reference's Model.cpp, VoxelCarving.cpp, ColorReconstruction.cpp,
Postprocessing3d.cpp and MarchingCubes.cpp compiled against functional stand-ins for OpenCV and
Eigen (oracle/ref_standins/) and run on the cases of tests/ref_program.py.  Every comparison is bit
for bit (floats through view(uint32), OFF files as bytes).  K and Rt are taken as the binary
derived them (its pose dump), so the stand-ins' Rodrigues and inv cancel out; the stand-ins'
gemm / norm arithmetic is the oracle's own statement and stays unpinned."""
import functools

import numpy as np
import pytest

from tests import ref_program as rp
from tests.stage_model import closure_any_kernel

VIEW_CASES = {"A": rp.case_A, "B": rp.case_B, "C1": lambda: rp.case_C((1, 1, 1)),
              "C234": lambda: rp.case_C((2, 3, 4)), "D": rp.case_D, "T": rp.case_T}


@functools.lru_cache(maxsize=None)
def case(name):
    return (VIEW_CASES.get(name) or rp.FIXTURE_CASES[name])()


def pre(c):
    return [("load_model",)] if "model" in c else []


@functools.lru_cache(maxsize=None)
def chain_run(name, mode):
    return rp.run(case(name), pre(case(name)) + rp.chain(mode))


@functools.lru_cache(maxsize=None)
def fast_run(name):
    return rp.run(case(name), pre(case(name)) + [("fastCarve",), ("dump", "fast")])


def start_state(c):
    X, Y, Z = c["dims"]
    st = np.ones(X * Y * Z, np.uint8)
    if "model" in c:
        st = rp.state_of(*c["model"])
    return st.reshape(Z, Y, X)


def views(oracle, c, res):
    """(M, campos) from the K and Rt the binary itself derived."""
    M = oracle.compose(res["K32"], res["Rt"])
    return M, np.ascontiguousarray(res["Rt"][:, :, 3])


def assert_model(got, want_rgba, want_state, what):
    rgba, seen = got
    st = rp.state_of(rgba, seen)
    want_state = np.asarray(want_state).reshape(-1)
    bad = np.flatnonzero(st != want_state)
    assert len(bad) == 0, f"{what}: {len(bad)} states differ, first voxel {bad[0]}: " \
                          f"reference {st[bad[0]]} oracle {want_state[bad[0]]}"
    bad = np.flatnonzero((rp.bits(rgba) != rp.bits(want_rgba)).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} colours differ, first voxel {bad[0]}: " \
                          f"reference {rgba[bad[0]]} oracle {np.asarray(want_rgba)[bad[0]]}"


def oracle_chain(oracle, c, res, mode):
    """The oracle's carve -> colour -> handleUnseen -> closure on the same inputs."""
    X, Y, Z = c["dims"]
    M, campos = views(oracle, c, res)
    st = oracle.carve(X, Y, Z, c["s"], M, c["masks"], state=start_state(c), threads=1)
    carved = oracle.model_from_state(st)
    coloured = oracle.color(X, Y, Z, c["s"], M, campos, c["images"], {"closest": 0, "avg": 1}[mode], carved)
    unseen = oracle.handle_unseen(st, coloured)
    closed = oracle.closure(X, Y, Z, unseen)
    return st, carved, coloured, unseen, closed


@pytest.mark.parametrize("name", list(VIEW_CASES))
def test_carve(oracle, name):
    c, res = case(name), chain_run(name, "closest")
    st, carved, *_ = oracle_chain(oracle, c, res, "closest")
    assert_model(res["carve"], carved, st, f"carve {name}")
    if name in ("A", "B"):
        assert (st == 3).any() and (st == 2).any()
    assert "LOG - VC: carving complete." in res["log"]


@pytest.mark.parametrize("name", list(VIEW_CASES))
def test_fast_carve(oracle, name):
    c, res = case(name), fast_run(name)
    X, Y, Z = c["dims"]
    M, _ = views(oracle, c, res)
    st = oracle.fast_carve(X, Y, Z, c["s"], M, c["masks"], state=start_state(c))
    assert_model(res["fast"], oracle.model_from_state(st), st, f"fastCarve {name}")
    if name == "D":  # the wall held the flood back, the hole let it through
        s3 = st.reshape(Z, Y, X)
        assert (s3[:, :, 8] == 3).sum() == 16 * 16 - 1 and s3[5, 9, 8] == 2
        assert (s3[:, :, 9:] == 2).any()  # (reached through the hole alone)


@pytest.mark.parametrize("mode", ["closest", "avg"])
@pytest.mark.parametrize("name", list(VIEW_CASES))
def test_colour_unseen_closure(oracle, name, mode):
    c, res = case(name), chain_run(name, mode)
    st, carved, coloured, unseen, closed = oracle_chain(oracle, c, res, mode)
    assert_model(res[mode], coloured, st, f"{mode} {name}")
    assert_model(res[mode + "_unseen"], unseen, rp.state_of(unseen, st.reshape(-1) & 2), f"{mode} unseen {name}")
    assert_model(res[mode + "_closed"], closed, rp.state_of(closed, st.reshape(-1) & 2), f"{mode} closed {name}")
    if name in ("A", "B"):
        assert (rp.bits(coloured) != rp.bits(carved)).any()
        assert ((closed[:, 3] != 0) & (unseen[:, 3] == 0)).any()
        if name == "B":
            assert (~res[mode][1]).any()  # some voxels no view sees: handleUnseen paints them


@pytest.mark.parametrize("ksize", [3, 5, 7])
def test_closure_kernels(oracle, ksize):
    c = case("E")
    X, Y, Z = c["dims"]
    rgba, seen = rp.run(c, [("load_model",), ("dump", "in"), ("closure", ksize), ("dump", "out")])["out"]
    want = closure_any_kernel(c["model"][0], X, Y, Z, ksize)
    assert_model((rgba, seen), want, rp.state_of(want, seen), f"closure {ksize}")
    filled = (want[:, 3] != 0) & (c["model"][0][:, 3] == 0)
    assert filled.any() and len(np.unique(want[filled, 0])) > 10  # means, not one colour
    if ksize == 3:
        assert np.array_equal(rp.bits(oracle.closure(X, Y, Z, c["model"][0])), rp.bits(rgba))


def off_of(oracle, c, rgba):
    X, Y, Z = c["dims"]
    verts, rgb = oracle.mc_mesh(X, Y, Z, rgba, rp.MC_THRESHOLD)
    return oracle.off_text(verts, rgb, np.float32(rp.MC_SCALE) * c["s"], rp.MC_SHIFT).encode()


@pytest.mark.parametrize("name", ["F3", "F5"])
def test_marching_cubes_off_bytes(oracle, name):
    c = case(name)
    res = rp.run(c, [("load_model",), ("dump", "loaded"), ("mc", "mesh")])
    assert np.array_equal(rp.bits(res["loaded"][0]), rp.bits(c["model"][0]))  # setters / getters
    assert res["mesh"] == off_of(oracle, c, c["model"][0])
    assert res["mesh"].count(b"\n3 ") > 100


def test_marching_cubes_of_the_closed_sphere(oracle):
    c = case("A")
    res = rp.run(c, rp.chain("avg") + [("mc", "mesh")])
    assert res["mesh"] == off_of(oracle, c, res["avg_closed"][0])
    assert res["mesh"].count(b"\n3 ") > 100


def test_depth_tie_precondition(oracle):
    """In T both views give every voxel the same depth, bit for bit, and different pixels: the
    closest colour there is the FIRST view's (strict `<`), and taking the last one instead would
    change the model."""
    c, res = case("T"), chain_run("T", "closest")
    X, Y, Z = c["dims"]
    M, campos = views(oracle, c, res)
    assert np.array_equal(rp.bits(campos[0]), rp.bits(campos[1]))
    st = rp.state_of(*res["carve"])
    assert (st == 3).all()  # nothing carved, everything seen
    first_wins = last_wins = 0
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                px = [oracle.project(M[v], c["s"], x, y, z, 32, 24) for v in (0, 1)]
                if None in px:
                    continue
                bgr = [c["images"][v, px[v][1], px[v][0]] for v in (0, 1)]
                got = res["closest"][0][x + X * (y + Y * z)]
                if np.array_equal(got, rp.MODEL_COLOR):
                    continue  # an inner voxel: not coloured
                first_wins += np.array_equal(got[:3], bgr[0][::-1].astype(np.float32))
                last_wins += np.array_equal(got[:3], bgr[1][::-1].astype(np.float32))
    assert first_wins > 100 and last_wins < first_wins // 20


def test_inside_camera_precondition(oracle):
    """In B at least 1 % of the voxels have a2 <= 0 for the camera inside the grid, some have
    a2 == 0, and that view alone carves at least one voxel behind it (through the mirrored pixel)."""
    c, res = case("B"), chain_run("B", "closest")
    X, Y, Z = c["dims"]
    M, _ = views(oracle, c, res)
    v = rp.B_INSIDE
    a2 = np.array([[[oracle.project_raw(M[v], c["s"], x, y, z)[2] for x in range(X)] for y in range(Y)]
                   for z in range(Z)])
    assert (a2 <= 0).mean() >= 0.01 and (a2 == 0).any() and (a2 < 0).any()
    alone = oracle.carve(X, Y, Z, c["s"], M[v:v + 1], c["masks"][v:v + 1], threads=1)
    assert ((alone == 2) & (a2 < 0)).any(), "no voxel behind the inside camera is carved"
    assert ((alone & 2) == 0)[a2 == 0].all()  # depth 0: no pixel, not seen
    both = oracle.carve(X, Y, Z, c["s"], M, c["masks"], threads=1)
    assert np.array_equal(rp.state_of(*res["carve"]), both.reshape(-1))


@pytest.mark.parametrize("assoc,variant", [(1, "assoc_left"), (0, "assoc_right")])
def test_both_groupings(oracle, assoc, variant):
    c = case("B")
    X, Y, Z = c["dims"]
    res = rp.run(c, [("carve",), ("dump", "carve"), ("avg",), ("dump", "avg")], assoc=assoc)
    M, campos = views(oracle, c, res)
    with oracle.variant(variant):
        assert oracle.assoc() == assoc
        st = oracle.carve(X, Y, Z, c["s"], M, c["masks"], threads=1)
        model = oracle.color(X, Y, Z, c["s"], M, campos, c["images"], 1, oracle.model_from_state(st))
    assert_model(res["carve"], oracle.model_from_state(st), st, variant)
    assert_model(res["avg"], model, st, variant + " avg")


@pytest.mark.parametrize("name", list(rp.FIXTURE_CASES))
def test_fixture_is_what_the_binary_writes(name):
    """tests/golden/ref_<name>.npz (tools/make_ref_fixtures.py) regenerated from the live binary:
    a stale fixture fails here."""
    rp.binary()
    live = rp.record(case(name))
    z = np.load(rp.fixture_path(name))
    assert sorted(z.files) == sorted(live)
    for k in z.files:
        a, b = z[k], np.asarray(live[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name}: {k}"
