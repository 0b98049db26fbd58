"""The inputs and the yardstick of tests/test_mesh_relax_gpu.py, checked without a GPU: the fan builder's
stated degrees against tests/mesh_smooth.py, that restatement's invariance under duplicated and
reversed faces, and tests/mesh_relax.py's CSR form of it against mesh_smooth itself, bit for bit."""
import numpy as np
import pytest

from tests import mesh_relax as mr
from tests import mesh_smooth as ms

F32 = np.float32


@pytest.fixture(scope="module")
def mesh():
    # (a hub below, at and above the CSR form's row classes as the tests below set them, isolated vertices)
    return mr.fans([1, 2, 3, 7, 8, 9, 40, 150], isolated=3, seed=5)


def test_fans_have_the_stated_degrees(mesh):
    verts, faces, degree = mesh
    assert len(verts) == sum(K + 1 for K in [1, 2, 3, 7, 8, 9, 40, 150]) + 3
    assert len(faces) == 2 * sum([1, 2, 3, 7, 8, 9, 40, 150])
    nbr, deg = ms.neighbours(len(verts), faces)
    assert np.array_equal(deg, degree)
    assert sorted(degree[degree > 3].tolist()) == [7, 8, 9, 40, 150] and (degree == 0).sum() == 3
    assert ((np.diff(nbr, axis=1) > 0) | (nbr[:, 1:] < 0)).all()  # (ascending, each once, then the padding)
    # the renumbering is no identity and the faces are not in fan order: ascending is not arrival order
    hubs = np.nonzero(degree == 150)[0]
    first = faces[(faces == hubs[0]).any(axis=1)][:, 1]
    assert (np.diff(first) < 0).any() and (np.diff(first) > 0).any()
    # every face is there with both windings
    key = {tuple(f) for f in faces.tolist()}
    assert all((a, c, b) in key for a, b, c in key)
    assert mr.neighbours(len(verts), faces)[1].tolist() == degree.tolist()


def test_restatement_is_invariant_under_duplicated_and_reversed_faces(mesh):
    """Positions depend on N(i) alone: a face given twice, or with the other winding, changes none."""
    verts, faces, _ = mesh
    once = faces[(faces[:, 1] < faces[:, 2]) | (faces[:, 1] == faces[:, 2])]  # (one winding of each face)
    assert 0 < len(once) < len(faces)
    want = ms.taubin(verts, once, 3)
    for other in (faces, np.concatenate([once, once]), once[:, [0, 2, 1]], once[::-1]):
        assert np.array_equal(mr.bits(ms.taubin(verts, other, 3)), mr.bits(want))
    assert not np.array_equal(want, verts)


@pytest.mark.parametrize("cap", [1, 8, 64, 1000])
@pytest.mark.parametrize("iterations", [0, 1, 3])
def test_csr_form_equals_mesh_smooth(mesh, cap, iterations):
    """tests/mesh_relax.py's smooth() -- rows above `cap` summed on their own -- is mesh_smooth.smooth()."""
    verts, faces, degree = mesh
    q, n = ms.smooth(verts, faces, iterations, 0.5, -0.53)
    q2, n2, d2 = mr.smooth(verts, faces, iterations, 0.5, -0.53, cap=cap)
    assert np.array_equal(mr.bits(q2), mr.bits(q)) and np.array_equal(mr.bits(n2), mr.bits(n))
    assert np.array_equal(d2, degree)
    assert np.array_equal(q2[degree == 0], verts[degree == 0]) and not n2[degree == 0].any()


def test_csr_form_on_degenerate_and_one_sided_faces():
    """Repeated corners, a face three times, faces with one winding only (normals that do not cancel)."""
    rng = np.random.default_rng(2)
    verts = rng.uniform(-4, 4, (12, 3)).astype(F32)
    faces = np.array([[0, 0, 0], [1, 1, 2], [3, 4, 3], [5, 6, 6], [7, 8, 9], [7, 8, 9], [7, 8, 9], [9, 10, 7],
                      [2, 5, 8], [0, 3, 10]], np.int64)
    for it in (0, 2):
        q, n = ms.smooth(verts, faces, it, 0.33, -0.34)
        q2, n2, d2 = mr.smooth(verts, faces, it, 0.33, -0.34, cap=2)
        assert np.array_equal(mr.bits(q2), mr.bits(q)) and np.array_equal(mr.bits(n2), mr.bits(n))
        assert np.array_equal(d2, ms.neighbours(12, faces)[1]) and d2[11] == 0 and n2[7].any()
    v0, f0, d0 = mr.fans([], isolated=2)
    assert len(v0) == 2 and len(f0) == 0 and not d0.any()
    q, n, d = mr.smooth(v0, f0, 3)
    assert np.array_equal(q, v0) and not n.any() and not d.any()
