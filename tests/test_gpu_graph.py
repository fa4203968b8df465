"""
GPU (-m gpu): graph operations on the device (xugrid_amd/graph.py, Ugrid2d.connected_components / binary_dilation /
binary_erosion): the reference's known answers on the chain, everything else against the numpy restatement of
tests/graph_cases.py and scipy.sparse.csgraph with ``array_equal``.
"""
import numpy as np
import pytest
from scipy.sparse import csgraph

import graph_cases as gc
from graph_cases import device_grid
import xugrid_amd as xa
from network_cases import raster_quads
from xugrid_amd import graph

pytestmark = pytest.mark.gpu

T, F = True, False


def test_chain_known_answers():
    con = gc.chain(5)
    exterior, mask = np.array([0, 4]), np.array([F, F, F, T, T])
    a = np.full(5, True)
    assert graph.binary_erosion(con, a).all()
    assert np.array_equal(graph.binary_erosion(con, a, exterior=exterior), [F, T, T, T, F])
    assert a.all()  # no mutation
    assert not graph.binary_erosion(con, a, exterior=exterior, iterations=3).any()
    assert np.array_equal(graph.binary_erosion(con, a, exterior=exterior, iterations=3, mask=mask), mask)
    assert np.array_equal(graph.binary_erosion(con, np.array([F, T, T, T, F])), [F, F, T, F, F])
    a = np.full(5, False)
    assert not graph.binary_dilation(con, a).any()
    assert not graph.binary_dilation(con, a, exterior=exterior).any()
    assert np.array_equal(graph.binary_dilation(con, a, exterior=exterior, border_value=True), [T, F, F, F, T])
    assert not a.any()
    assert graph.binary_dilation(con, a, exterior=exterior, iterations=3, border_value=True).all()
    assert np.array_equal(graph.binary_dilation(con, a, exterior=exterior, iterations=3, mask=mask, border_value=True), ~mask)
    out = graph.binary_dilation(con, np.array([F, F, T, F, F]))
    assert out.dtype == np.bool_ and np.array_equal(out, [F, T, T, T, F])
    assert np.array_equal(xa.connected_components(con), np.zeros(5, dtype=np.int64))


def grids(xy, faces):
    """The same mesh as a host-built grid and as a device grid."""
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces), device_grid(xy, faces)


def expected(host, data, value, iterations, mask, border_value):
    return gc.binary_iterate(host.face_face_connectivity, data, value, iterations, mask, host.exterior_faces, border_value)


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("border_value", [False, True])
def test_raster(iterations, border_value):
    xy, faces = raster_quads(np.arange(10.0), np.arange(8.0))
    field = np.random.default_rng(11).random(len(faces)) < 0.45
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    border = np.zeros((7, 9), dtype=bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    assert np.array_equal(host.exterior_faces, np.nonzero(border.ravel())[0])
    for grid in grids(xy, faces):
        assert np.array_equal(grid.binary_dilation(field, iterations, border_value=border_value),
                              expected(host, field, True, iterations, None, border_value))
        assert np.array_equal(grid.binary_erosion(field, iterations, border_value=border_value),
                              expected(host, field, False, iterations, None, border_value))


_BIG = {}


def big():
    if not _BIG:
        xy, faces = gc.big_triangles()
        host, dev = grids(xy, faces)
        rng = np.random.default_rng(2)
        _BIG.update(host=host, dev=dev, field=rng.random(len(faces)) < 0.3, mask=rng.random(len(faces)) < 0.1)
    return _BIG["host"], _BIG["dev"], _BIG["field"], _BIG["mask"]


@pytest.mark.parametrize("iterations", [1, 2, 7])
@pytest.mark.parametrize("border_value", [False, True])
def test_40k_triangles_with_mask(iterations, border_value):
    host, dev, field, mask = big()
    before = field.copy()
    for value, method in ((True, dev.binary_dilation), (False, dev.binary_erosion)):
        got = method(field, iterations, mask=mask, border_value=border_value)
        assert np.array_equal(got, expected(host, field, value, iterations, mask, border_value))
    assert np.array_equal(field, before)  # the input is unchanged


def test_stacked_slices_equal_single_calls():
    host, dev, field, mask = big()
    rng = np.random.default_rng(8)
    stack = np.stack([field, ~field, rng.random(field.size) < 0.5])
    out = dev.binary_dilation(stack, 2, mask=mask, border_value=True)
    assert out.shape == stack.shape and out.dtype == np.bool_
    for k in range(3):
        assert np.array_equal(out[k], dev.binary_dilation(stack[k], 2, mask=mask, border_value=True))
    out2 = dev.binary_erosion(stack.reshape(3, 1, -1), 3)
    assert out2.shape == (3, 1, field.size)
    for k in range(3):
        assert np.array_equal(out2[k, 0], dev.binary_erosion(stack[k], 3))


def test_argument_errors():
    host, dev, field, mask = big()
    with pytest.raises(ValueError, match="iterations"):
        dev.binary_dilation(field, iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        graph.binary_erosion(gc.chain(5), np.full(5, True), iterations=0)
    with pytest.raises(TypeError, match="bool"):
        dev.binary_dilation(field.astype(np.float64))
    with pytest.raises(TypeError, match="bool"):
        graph.binary_dilation(gc.chain(5), np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match="shape"):
        dev.binary_erosion(field[:-1])


_STRIP = {}


def strip_grid():
    if not _STRIP:
        xy, faces = gc.strip(3000)
        _STRIP["grid"] = device_grid(xy, faces)
    return _STRIP["grid"]


def test_strip_dilation_travels_one_cell_per_iteration():
    grid = strip_grid()
    seed = np.zeros(3000, dtype=bool)
    seed[0] = True
    assert grid.binary_dilation(seed, iterations=2999).all()
    out = grid.binary_dilation(seed, iterations=2998)
    assert out[:-1].all() and not out[-1]


def assert_components(grid, host):
    for dim, conn in (("face", host.face_face_connectivity), ("node", host.node_node_connectivity)):
        got = grid.connected_components(dim)
        assert got.dtype == np.int64 and np.array_equal(got, csgraph.connected_components(conn, directed=False)[1])


def test_components_disconnected_mesh():
    xy, faces = gc.disconnected()
    host, dev = grids(xy, faces)
    assert_components(dev, host)
    assert_components(host, host)
    assert dev.connected_components().max() == 2  # two patches and the isolated triangle


def test_components_strip():
    xy, faces = gc.strip(3000)
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert_components(strip_grid(), host)
    assert not strip_grid().connected_components().any()


def test_components_permuted_40k():
    xy, faces = gc.big_permuted()
    host, dev = grids(xy, faces)
    assert_components(dev, host)
