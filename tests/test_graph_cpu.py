"""CPU tests of the yardsticks themselves (tests/graph_cases.py): the numpy restatement of the binary iteration against the
reference's known answers and scipy.ndimage, and the claimed component numbering against scipy.sparse.csgraph."""
import numpy as np
import pytest
from scipy import ndimage, sparse
from scipy.sparse import csgraph

import graph_cases as gc
from network_cases import raster_quads
from xugrid_amd import connectivity

T, F = True, False


def test_chain_erosion_known_answers():
    con = gc.chain(5)
    a = np.full(5, True)
    assert gc.binary_iterate(con, a, False).all()
    exterior = np.array([0, 4])
    assert np.array_equal(gc.binary_iterate(con, a, False, exterior=exterior), [F, T, T, T, F])
    assert a.all()  # no mutation
    assert not gc.binary_iterate(con, a, False, iterations=3, exterior=exterior).any()
    mask = np.array([F, F, F, T, T])
    assert np.array_equal(gc.binary_iterate(con, a, False, iterations=3, mask=mask, exterior=exterior), mask)
    a = np.array([F, T, T, T, F])
    assert np.array_equal(gc.binary_iterate(con, a, False), [F, F, T, F, F])


def test_chain_dilation_known_answers():
    con = gc.chain(5)
    a = np.full(5, False)
    assert not gc.binary_iterate(con, a, True).any()
    exterior = np.array([0, 4])
    assert not gc.binary_iterate(con, a, True, exterior=exterior).any()
    assert np.array_equal(gc.binary_iterate(con, a, True, exterior=exterior, border_value=True), [T, F, F, F, T])
    assert not a.any()  # no mutation
    assert gc.binary_iterate(con, a, True, iterations=3, exterior=exterior, border_value=True).all()
    mask = np.array([F, F, F, T, T])
    assert np.array_equal(gc.binary_iterate(con, a, True, iterations=3, mask=mask, exterior=exterior, border_value=True), ~mask)
    a = np.array([F, F, T, F, F])
    assert np.array_equal(gc.binary_iterate(con, a, True), [F, T, T, T, F])


def raster_case():
    """9 x 7 quad raster: face adjacency, border cells, a random field (ny, nx)."""
    nx, ny = 9, 7
    _, faces = raster_quads(np.arange(nx + 1.0), np.arange(ny + 1.0))
    topo = gc.host_topology(faces, (nx + 1) * (ny + 1))
    border = np.zeros((ny, nx), dtype=bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    field = np.random.default_rng(11).random((ny, nx)) < 0.45
    return topo["face_face"], np.nonzero(border.ravel())[0], field


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("border_value", [False, True])
def test_raster_dilation_agrees_with_ndimage(iterations, border_value):
    """Dilation: a False border changes nothing in either; a True border makes scipy's outside cells True, which after ONE step
    turns every border cell True -- the restatement's ``exterior`` rule -- and later steps only look inside the raster, where
    scipy's outside (True) can add nothing the border cells, already True, do not add."""
    conn, exterior, field = raster_case()
    got = gc.binary_iterate(conn, field.ravel(), True, iterations, exterior=exterior, border_value=border_value)
    exp = ndimage.binary_dilation(field, iterations=iterations, border_value=int(border_value))
    assert np.array_equal(got.reshape(field.shape), exp)


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("border_value", [False, True])
def test_raster_erosion_agrees_with_ndimage(iterations, border_value):
    """Erosion: with a False border scipy's outside cells erode every border cell in the first step, as ``exterior`` does;
    with a True border the outside never erodes anything and ``exterior`` is not used (border_value != value)."""
    conn, exterior, field = raster_case()
    got = gc.binary_iterate(conn, field.ravel(), False, iterations, exterior=exterior, border_value=border_value)
    exp = ndimage.binary_erosion(field, iterations=iterations, border_value=int(border_value))
    assert np.array_equal(got.reshape(field.shape), exp)


def random_symmetric_graph(n=400, n_edges=300, seed=3):
    """A sparse symmetric graph with isolated nodes (fewer edges than nodes)."""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, n_edges), rng.integers(0, n, n_edges)
    keep = i != j
    i, j = i[keep], j[keep]
    m = sparse.coo_matrix((np.ones(2 * i.size), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    m.data[:] = 1.0
    return m


def graphs():
    xy, faces = gc.disconnected()
    topo = gc.host_topology(faces, len(xy))
    yield topo["face_face"]
    yield topo["node_node"]
    yield random_symmetric_graph()


def test_component_numbering_is_scipys():
    """Rank of the smallest member == scipy's numbering (scipy labels components in the order it first meets them while
    walking the nodes upwards, i.e. in the order of their smallest members)."""
    for conn in graphs():
        n_comp, exp = csgraph.connected_components(conn, directed=False)
        got = gc.component_numbers(gc.smallest_member_labels(conn))
        assert np.array_equal(got, exp)
        assert got.max() + 1 == n_comp
    assert connectivity.FILL_VALUE == -1
