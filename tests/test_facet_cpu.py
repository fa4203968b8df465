"""
CPU: what the facet mapping (xugrid_amd/facet.py: to_node / to_edge / to_face) rests on that needs no device -- the numpy
restatement of tests/facet_cases.py against hand-computed answers, node -> edge being the node_node CSR under another name,
the sequential reduction against numpy's nan-reducers within the derived reordering bound, and the argument errors.
"""
import numpy as np
import pytest

import facet_cases as fc
import graph_cases as gc
import xugrid_amd as xa
from xugrid_amd import connectivity

NAN = np.nan


def _tables():
    xy, faces = fc.two_triangles()
    return fc.host_tables(faces, len(xy))


def test_tables_of_the_two_triangle_mesh():
    t = _tables()
    assert np.array_equal(t[("edge", "node")], [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]])
    assert np.array_equal(t[("face", "edge")], [[0, 2, 1], [3, 4, 2]])
    assert np.array_equal(t[("edge", "face")], [[0, -1], [0, -1], [0, 1], [1, -1], [1, -1]])
    assert np.array_equal(t[("node", "face")], [[0, -1], [0, 1], [0, 1], [1, -1]])
    assert np.array_equal(t[("node", "edge")], [[0, 1, -1], [0, 2, 3], [1, 2, 4], [3, 4, -1]])


def test_restatement_gives_the_hand_computed_answers():
    t = _tables()
    eq = lambda a, b: np.array_equal(a, np.asarray(b, dtype=float), equal_nan=True)  # noqa: E731
    face = np.array([10.0, 20.0])
    assert eq(fc.raw(t[("node", "face")], face), [[10, NAN], [10, 20], [10, 20], [20, NAN]])
    node = np.array([1.0, 2.0, 3.0, 4.0])
    assert eq(fc.raw(t[("edge", "node")], node), [[1, 2], [1, 3], [2, 3], [2, 4], [3, 4]])
    edge = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert eq(fc.raw(t[("face", "edge")], edge), [[1, 3, 2], [4, 5, 3]])
    assert eq(fc.raw(t[("node", "edge")], edge)[0], [1, 2, NAN])
    for reduce in (fc.reduce_sequential, fc.reduce_numpy):
        assert eq(reduce(t[("node", "face")], face, "mean"), [10, 15, 15, 20])
        assert eq(reduce(t[("edge", "face")], face, "mean"), [10, 10, 15, 20, 20])
        assert eq(reduce(t[("face", "node")], node, "mean"), [2, 3])
        assert eq(reduce(t[("face", "edge")], edge, "sum"), [6, 12])
        assert eq(reduce(t[("node", "edge")], edge, "max"), [2, 4, 5, 5])
        assert eq(reduce(t[("node", "edge")], edge, "min"), [1, 1, 2, 4])
        holed = np.array([NAN, 20.0])
        assert eq(reduce(t[("node", "face")], holed, "mean"), [NAN, 20, 20, 20])
        assert eq(reduce(t[("node", "face")], holed, "sum"), [0, 20, 20, 20])
        assert eq(reduce(t[("node", "face")], holed, "min"), [NAN, 20, 20, 20])
    # leading dims are kept
    stack = np.stack([face, 2 * face]).reshape(2, 1, 2)
    assert fc.raw(t[("node", "face")], stack).shape == (2, 1, 4, 2)
    assert eq(fc.reduce_sequential(t[("node", "face")], stack, "mean")[1, 0], [20, 30, 30, 40])


def test_dense_pads_to_the_asked_width():
    csr = connectivity.invert_dense_to_sparse(np.array([[0, 1, 2], [1, 3, 2]]), n_rows=6)
    assert np.array_equal(fc.dense(csr), [[0, -1], [0, 1], [0, 1], [1, -1], [-1, -1], [-1, -1]])
    assert fc.dense(csr, 3).shape == (6, 3) and (fc.dense(csr, 3)[:, 2] == -1).all()


@pytest.mark.parametrize("mesh", ["disconnected", "hubs", "big_permuted"])
def test_node_node_data_is_node_edge(mesh):
    """Rows of node_node have ascending neighbours; edges are numbered by (lower, higher) node, so its data -- the edge ids
    -- are exactly the node -> edge inversion of edge_node, row pointers included."""
    xy, faces = getattr(gc, mesh)()
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    node_node, node_edge = grid.node_node_connectivity, grid.node_edge_connectivity
    assert node_edge.shape == (grid.n_node, grid.n_edge)
    assert np.array_equal(node_node.indptr, node_edge.indptr)
    assert np.array_equal(node_node.data, node_edge.indices)
    assert (np.diff(node_edge.indices)[np.diff(np.repeat(np.arange(grid.n_node), np.diff(node_edge.indptr))) == 0] > 0).all()


@pytest.mark.parametrize("mesh", ["disconnected", "hubs", "fan"])
def test_sequential_reduction_is_within_the_reordering_bound_of_numpy(mesh):
    xy, faces = getattr(gc, mesh)()
    tables = fc.host_tables(faces, len(xy))
    n = fc.sizes(tables)
    for (target, source), table in tables.items():
        data = fc.field(n[source], seed=3)
        for how in fc.REDUCERS:
            seq, ref = fc.reduce_sequential(table, data, how), fc.reduce_numpy(table, data, how)
            assert np.array_equal(np.isnan(seq), np.isnan(ref)), (target, source, how)
            if how in ("min", "max") or table.shape[1] <= 2:
                assert np.array_equal(seq, ref, equal_nan=True), (target, source, how)
                continue
            bound, has_inf = fc.reorder_bound(table, data, how)
            assert np.array_equal(seq[has_inf], ref[has_inf], equal_nan=True)
            fin = ~has_inf & ~np.isnan(ref)
            with np.errstate(invalid="ignore"):
                diff = np.abs(seq - ref)
            assert (diff[fin] <= bound[fin]).all(), (target, source, how)


# ---- argument errors: none of them needs a device
def _grid2d():
    xy, faces = fc.two_triangles()
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


def _grid1d():
    xy, edges = fc.y_network()
    return xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)


def test_same_facet_is_refused():
    grid = _grid2d()
    with pytest.raises(ValueError, match="No conversion needed, data is already node-associated."):
        grid.to_node(np.zeros(4), dim="node")
    with pytest.raises(ValueError, match="No conversion needed, data is already face-associated."):
        grid.to_face(np.zeros(2), dim=grid.face_dimension)
    with pytest.raises(ValueError, match="No conversion needed, data is already edge-associated."):
        _grid1d().to_edge(np.zeros(10), dim="edge")


def test_unknown_reduce_lists_the_four():
    with pytest.raises(ValueError, match="mean, sum, min, max"):
        _grid2d().to_node(np.zeros(2), reduce="median")


def test_dim_none_needs_one_matching_facet():
    # one quad has 4 nodes and 4 edges: data of 4 entries going to the faces fits both
    quad = xa.Ugrid2d(np.array([0.0, 1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0, 1.0]), -1, np.array([[0, 1, 2, 3]]))
    assert quad.n_node == 4 and quad.n_edge == 4
    with pytest.raises(ValueError, match="dim"):
        quad.to_face(np.zeros(4))
    grid = _grid2d()
    with pytest.raises(ValueError, match=r"expected sizes 5 \(edge\), 2 \(face\)"):
        grid.to_node(np.zeros(7))
    with pytest.raises(ValueError, match=r"expected sizes 11 \(node\)"):
        _grid1d().to_edge(np.zeros(10))  # (edge data: the only other facet has 11)


def test_a_network_has_no_faces():
    with pytest.raises(ValueError, match="Cannot map to face for a Ugrid1d topology."):
        _grid1d().to_face(np.zeros(10))
    with pytest.raises(ValueError, match="Cannot map to face for a Ugrid1d topology."):
        _grid1d().facet_width("face", "node")


def test_host_widths():
    grid = _grid2d()
    widths = {(t, s): grid.facet_width(t, s) for t, s in fc.DIRECTIONS}
    assert widths == {("node", "face"): 2, ("node", "edge"): 3, ("edge", "node"): 2, ("edge", "face"): 2, ("face", "node"): 3,
                      ("face", "edge"): 3}
    net = _grid1d()
    assert net.facet_width("node", "edge") == 3 and net.facet_width("edge", "node") == 2
