"""The welded marching-cubes mesh without a GPU: the numpy restatement of its definition
(tests/mesh_weld.py) on the oracle's meshes of the reference's own models, and arvx::weldMesh
(include/arvx/marching_cubes.hpp, compiled with g++) against the restatement.

On the reference's 1.off model the distinct vertices are the 5 704 occupied voxels with an empty
6-neighbour (tests/test_mc_off.py): the welded vertex list must be exactly that list, in
Model::flatten order, and unwelding must give the oracle's triangles back."""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_weld as mw
from tests.test_mc_off import coloured_model, off1, off23, random_coloured_model, state_of  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_weld(verts, rgb):
    """weld() satisfies the definition: distinct vertices, ascending (z, y, x), faces that
    unweld to the input, colours unchanged."""
    wv, faces, frgb = mw.weld(verts, rgb)
    key = wv[:, ::-1].astype(np.float64)
    assert all(tuple(a) < tuple(b) for a, b in zip(key[:-1], key[1:]))  # strictly ascending
    assert faces.shape == (len(rgb), 3) and faces.dtype == np.uint32
    assert len(faces) == 0 or faces.max() < len(wv)
    assert np.array_equal(mw.unweld(wv, faces), verts)
    assert np.array_equal(frgb, rgb)
    return wv, faces, frgb


def test_weld_of_1_off_is_the_surface_voxels(oracle, off1):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    verts, rgb = oracle.mc_mesh(X, Y, Z, oracle.model_from_state(state_of(off1["occ"])))
    wv, faces, _ = check_weld(verts, rgb)
    assert np.array_equal(mw.lattice_index(wv, X, Y), off1["surface_index"]) and len(wv) == 5704
    assert np.array_equal(mw.surface_voxels(off1["occ"]), off1["surface_index"])
    # snapping leaves degenerate triangles, and they stay
    assert len(faces) == off1["nf"]
    assert ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])).any()


@pytest.mark.parametrize("name", ["2", "3"])
def test_weld_of_2_off_and_3_off(oracle, off1, off23, name):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    verts, rgb = oracle.mc_mesh(X, Y, Z, coloured_model(oracle, off1, off23["vox_rgb" + name]))
    wv, faces, frgb = check_weld(verts, rgb)
    assert np.array_equal(mw.lattice_index(wv, X, Y), off1["surface_index"])
    assert np.array_equal(frgb.astype(np.uint8), off23["face_rgb" + name])


@pytest.mark.parametrize("fractional,threshold", [(False, 0.5), (True, 0.5), (True, 0.3)])
def test_weld_of_oracle_meshes(oracle, fractional, threshold):
    rng = np.random.default_rng(41 + fractional)
    for dims in [(6, 5, 4), (9, 9, 9), (3, 1, 2), (17, 11, 13)]:
        X, Y, Z = dims
        rgba = random_coloured_model(rng, X, Y, Z, fractional)
        verts, rgb = oracle.mc_mesh(X, Y, Z, rgba, threshold)
        wv, _, _ = check_weld(verts, rgb)
        if not fractional:  # snapped: the vertices are the surface voxels
            occ = (rgba[:, 3] != 0).reshape(Z, Y, X)
            assert np.array_equal(mw.lattice_index(wv, X, Y), mw.surface_voxels(occ)), dims
        else:
            assert len(verts) == 0 or len(wv) < len(verts)


def test_weld_restatement_on_a_handmade_mesh():
    """Float comparison, (z, y, x) order and degenerate triangles on a mesh small enough to
    check by hand."""
    verts = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1],
                        [0, 0, 1], [-0.0, 1, 0], [0.5, 0, 0],
                        [0.5, 0, 0], [0.5, 0, 0], [1, 0, 0]])
    wv, faces, _ = mw.weld(verts, np.uint32([[1, 2, 3], [4, 5, 6], [7, 8, 9]]))
    assert np.array_equal(wv, np.float32([[0.5, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]))
    assert np.array_equal(faces, np.uint32([[1, 2, 3], [3, 2, 0], [0, 0, 1]]))


@pytest.fixture(scope="module")
def weld_bin():
    from ar_voxel_project_amd import build
    return build.build_weld_host_test()


def cpp_weld(weld_bin, tmp_path, verts, rgb, off=None):
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int64(len(rgb)).tobytes())
        f.write(np.ascontiguousarray(verts, np.float32).tobytes())
        f.write(np.ascontiguousarray(rgb, np.uint32).tobytes())
    r = subprocess.run([weld_bin, src, out] + ([off] if off else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    b = open(out, "rb").read()
    nv, nt = np.frombuffer(b[:16], np.int64)
    wv = np.frombuffer(b[16:16 + 12 * nv], np.float32).reshape(-1, 3)
    rec = np.frombuffer(b[16 + 12 * nv:], np.uint32).reshape(-1, 6)
    assert len(rec) == nt
    return wv, rec[:, :3], rec[:, 3:]


def parse_off(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "OFF"
    nv, nf, _ = (int(a) for a in lines[1].split())
    v = np.array([ln.split() for ln in lines[2:2 + nv]], np.float32).reshape(-1, 3)
    f = np.array([ln.split() for ln in lines[2 + nv:2 + nv + nf]], np.int64).reshape(-1, 7)
    assert (f[:, 0] == 3).all() and lines[2 + nv + nf:] == [""]
    return v, f[:, 1:4], f[:, 4:]


def test_cpp_weld_mesh_agrees_with_the_restatement(weld_bin, oracle, off1, off23, tmp_path):  # noqa: F811
    X, Y, Z = off1["X"], off1["Y"], off1["Z"]
    meshes = [oracle.mc_mesh(X, Y, Z, oracle.model_from_state(state_of(off1["occ"]))),
              oracle.mc_mesh(X, Y, Z, coloured_model(oracle, off1, off23["vox_rgb2"]))]
    rng = np.random.default_rng(43)
    for fractional, threshold in [(False, 0.5), (True, 0.5), (True, 0.3)]:
        for dims in [(9, 9, 9), (17, 11, 13)]:
            meshes.append(oracle.mc_mesh(*dims, random_coloured_model(rng, *dims, fractional), threshold))
    meshes.append((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)))  # empty
    for k, (verts, rgb) in enumerate(meshes):
        want = mw.weld(verts, rgb)
        off = str(tmp_path / f"w{k}.off")
        got = cpp_weld(weld_bin, tmp_path, verts, rgb, off)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), k
        # WriteMesh writes the shared vertices as a valid OFF: the same mesh, values as %g
        ov, of, orgb = parse_off(off)
        assert np.array_equal(of, want[1]) and np.array_equal(orgb, want[2])
        assert np.array_equal(ov, np.float32(["%g" % x for x in want[0].ravel()]).reshape(-1, 3))
