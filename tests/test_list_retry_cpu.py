"""The reach of tests/test_list_retry_gpu.py: every list of its scene is longer than the room a fresh
context gives it.  The rule is restated from DESIGN 4.4 (tests/list_retry.py, first_capacity), the
lengths are counted on the CPU from the oracle's and the numpy restatements' results.  A condition,
not a measurement: a fresh context cannot hold any of these lists in one attempt."""
import pytest

from tests import list_retry as lr


@pytest.fixture(scope="module")
def want(oracle):
    return lr.references(oracle, lr.scene())


@pytest.fixture(scope="module")
def counted(want):
    return lr.lengths(lr.scene(), want)


def test_first_capacity_rule():
    caps = lr.first_capacities()
    assert caps == dict(surface=17099, fills=17099, cells=17099, triangles=34198, vertices=17099,
                        cut_edges=51297)
    # the bound on the minimum only matters for tiny grids: 8 voxels have room for 8, cells for more
    assert lr.first_capacity(8) == 8 and lr.first_capacity(8, 8 + 1e6) == 4128


@pytest.mark.parametrize("name", ["surface", "fills", "cells", "triangles", "vertices", "cut_edges"])
def test_every_list_outgrows_a_fresh_context(counted, name):
    cap = lr.first_capacities()[name]
    print(f"{name}: {counted[name]} entries, room for {cap}")
    assert counted[name] > cap


def test_photo_carve_reference_removes_voxels(want):
    """The photo carve's reference run is no fixed point: both of its iterations remove voxels, so
    the device's first (truncated) attempt of each must leave the state alone to match it."""
    photo = want.photo
    assert photo.iterations == lr.PHOTO["iterations"] and all(len(w) > 0 for w in photo.sweeps)
