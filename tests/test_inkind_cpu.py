"""
CPU: the host side of the index and data-kind layer (xugrid_amd/inkind.py) -- ``as_index`` on host indexers, the host paths of
``Index``, ``data_facet`` over one grid and over partitions, and the kind rule.  Nothing here needs a device.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from xugrid_amd import inkind
from xugrid_amd.inkind import Index, as_index, data_facet, result_kind

N = 5


def stub(n_node=4, n_edge=4, n_face=2):
    return SimpleNamespace(n_node=n_node, n_edge=n_edge, n_face=n_face, node_dimension="nodes", edge_dimension="edges",
                           face_dimension="faces")


# ---- as_index -------------------------------------------------------------------------------------------------------------------
def test_as_index_accepts_ids_masks_and_nothing():
    index = as_index([3, 0, 4], N)
    assert index.n == 3 and index.host.dtype == np.int64 and index.host.tolist() == [3, 0, 4]
    assert index.dev is None and index.like is None
    mask = as_index(np.array([True, False, False, True, True]), N)
    assert mask.host.dtype == np.int64 and mask.host.tolist() == [0, 3, 4]
    empty = as_index([], N)
    assert empty.n == 0 and empty.host.dtype == np.int64
    assert as_index(index, N) is index


def test_as_index_refusals():
    with pytest.raises(ValueError, match="1d"):
        as_index(np.zeros((2, 2), dtype=np.int64), N)
    with pytest.raises(ValueError, match="larger than dimension size"):
        as_index(np.arange(6), N)
    with pytest.raises(ValueError, match="bool index"):
        as_index(np.ones(4, dtype=bool), N)
    with pytest.raises(TypeError):
        as_index(np.array([0.0, 1.0]), N)
    for outside in ([0, 5], [2, -1]):  # nothing wraps around
        with pytest.raises(IndexError, match="outside"):
            as_index(outside, N)
    with pytest.raises(ValueError) as error:
        as_index([1, 2, 1], N)
    assert str(error.value) == inkind.REPEATED


# ---- Index on the host ----------------------------------------------------------------------------------------------------------
def test_index_host_paths():
    ids = np.array([2, 0, 1], dtype=np.int64)
    index = Index(host=ids)
    assert index.emit(None, to_numpy=True) is ids and index.numpy() is ids
    assert Index.wrap(ids).host is ids and Index.wrap(index) is index
    assert np.array_equal(Index.arange(3).numpy(), [0, 1, 2]) and Index.arange(3).numpy().dtype == np.int64
    assert Index.arange(0).n == 0


def test_index_same_on_the_host():
    a = Index(host=np.array([0, 1, 2], dtype=np.int64))
    assert Index.same(a, Index(host=np.array([0, 1, 2], dtype=np.int64)))
    assert not Index.same(a, Index(host=np.array([0, 2, 1], dtype=np.int64)))  # a permutation is another index
    assert not Index.same(a, Index(host=np.array([0, 1], dtype=np.int64)))
    assert Index.same(Index.arange(0), Index(host=np.zeros(0, dtype=np.int64)))


# ---- data_facet -----------------------------------------------------------------------------------------------------------------
def test_facet_names():
    assert inkind.facet_names(stub()) == {"nodes": "node", "edges": "edge", "faces": "face"}
    network = SimpleNamespace(n_node=3, n_edge=2, node_dimension="nodes", edge_dimension="edges")
    assert inkind.facet_names(network) == {"nodes": "node", "edges": "edge"}


def test_data_facet_of_one_grid():
    grid = stub()
    assert data_facet(grid, np.zeros((3, 2))) == "face"
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):  # nodes and edges both fit
        data_facet(grid, np.zeros((3, 4)))
    assert data_facet(grid, np.zeros((3, 4)), dim="edges") == "edge"
    assert data_facet(grid, np.zeros((3, 4)), dim="nodes") == "node"
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):  # the named dimension has another size
        data_facet(grid, np.zeros((3, 4)), dim="faces")
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):  # no facet fits
        data_facet(grid, np.zeros((3, 7)))
    with pytest.raises(ValueError, match="not a UGRID dimension"):
        data_facet(grid, np.zeros((3, 4)), dim="layer")
    with pytest.raises(ValueError, match=r"shape \(\.\.\., n\)"):
        data_facet(grid, np.float64(1.0))


def test_data_facet_of_partitions():
    grids = [stub(4, 5, 2), stub(6, 7, 3)]
    assert data_facet(grids, [np.zeros((3, 2)), np.zeros((3, 3))]) == "face"
    assert data_facet(grids, [np.zeros(5), np.zeros(7)], dim="edges") == "edge"
    with pytest.raises(ValueError, match="one array per partition"):
        data_facet(grids, [np.zeros((3, 2))])
    with pytest.raises(ValueError, match="same leading dimensions"):
        data_facet(grids, [np.zeros((3, 2)), np.zeros((2, 3))])
    with pytest.raises(ValueError, match="same leading dimensions"):
        data_facet(grids, [np.zeros((3, 2)), np.float64(0.0)])
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):  # faces in the first partition, nothing in the second
        data_facet(grids, [np.zeros((3, 2)), np.zeros((3, 2))])
    with pytest.raises(ValueError, match="not a UGRID dimension"):
        data_facet(grids, [np.zeros((3, 2)), np.zeros((3, 3))], dim="layer")


# ---- the kind rule --------------------------------------------------------------------------------------------------------------
def test_result_kind():
    assert result_kind(stub()) == (None, True)  # no ``_device_resident``: a host-array class
    assert result_kind(SimpleNamespace(_device_resident=False), None) == (None, True)
    assert result_kind(SimpleNamespace(_device_resident=True)) == (None, False)
    assert result_kind([SimpleNamespace(_device_resident=False), SimpleNamespace(_device_resident=True)], None) == (None, False)
    like = object()
    assert result_kind(stub(), None, like) == (like, False)
