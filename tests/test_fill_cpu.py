"""
CPU: the host side of the fills -- adjacency matrices against the reference's construction, argument validation before
any device call, the KDTree distance rule the nearest fill follows, and the test helper's known answer.
"""
import numpy as np
import pytest
from scipy import sparse
from scipy.spatial import KDTree

import xugrid_amd as xa
from fill_cases import (chain, mixed_faces, reference_face_face, reference_laplace, reference_node_node,
                        reference_weights)


def assert_same_csr(a, b):
    a, b = a.tocsr(), b.tocsr()
    a.sort_indices()
    b.sort_indices()
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.indptr, b.indptr)
    np.testing.assert_array_equal(a.indices, b.indices)
    np.testing.assert_allclose(a.data, b.data, rtol=1e-15, atol=0)


def grids():
    xy, faces = mixed_faces()
    yield xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces), xy, faces
    rxy, rfaces = xa.meshgen.quad_mesh(np.linspace(0.0, 4.0, 6), np.linspace(0.0, 3.0, 5))
    yield xa.Ugrid2d(rxy[:, 0], rxy[:, 1], -1, rfaces), rxy, rfaces


@pytest.mark.parametrize("case", [0, 1])
def test_connectivity_matrices_match_reference_construction(case):
    grid, xy, faces = list(grids())[case]
    ff = grid.face_face_connectivity
    assert_same_csr(ff, reference_face_face(faces))
    assert np.all(np.diff(ff.indices[ff.indptr[0]:ff.indptr[1]]) > 0)
    assert_same_csr(grid.get_connectivity_matrix("face", xy_weights=False), reference_face_face(faces))
    nn = reference_node_node(faces, xy.shape[0])
    assert_same_csr(grid.node_node_connectivity, nn)
    assert_same_csr(grid.get_connectivity_matrix(grid.node_dimension, xy_weights=False), nn)
    weighted = grid.get_connectivity_matrix("node", xy_weights=True)
    expected = nn.copy()
    expected.data = reference_weights(nn, xy)
    assert_same_csr(weighted, expected)


def test_ugrid1d_connectivity():
    xy = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [3.0, 3.0], [4.0, 4.0]])
    grid = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, np.array([[0, 1], [1, 2], [3, 4]]))
    conn = grid.get_connectivity_matrix("node", xy_weights=False)
    np.testing.assert_array_equal(conn.indptr, [0, 1, 3, 4, 5, 6])
    np.testing.assert_array_equal(conn.indices, [1, 0, 2, 1, 4, 3])
    np.testing.assert_array_equal(conn.data, [0, 0, 1, 1, 2, 2])


def test_validation_before_any_device_call():
    with pytest.raises(ValueError, match="connectivity is not a square matrix"):
        xa.laplace_interpolate(np.ones(3), sparse.csr_matrix((3, 4)), np.zeros(3, dtype=int), False)
    with pytest.raises(ValueError, match=r"expected data of shape \(5,\)"):
        xa.laplace_interpolate(np.ones(4), chain(5), np.zeros(5, dtype=int), False)
    with pytest.raises(ValueError, match="ILU0"):
        xa.laplace_interpolate(np.ones(5), chain(5), np.zeros(5, dtype=int), False, delta=0.1)
    grid, _, _ = next(grids())
    with pytest.raises(ValueError, match='"abc" is not a valid interpolator.'):
        grid.interpolate_na(np.ones(grid.n_face), method="abc")
    with pytest.raises(ValueError, match="Laplace interpolation along edges is not allowed."):
        grid.laplace_interpolate(np.ones(grid.n_edge), dim="edge")
    with pytest.raises(ValueError, match="ILU0"):
        grid.laplace_interpolate(np.ones(grid.n_face), relax=0.5)
    with pytest.raises(ValueError, match="Expected one of"):
        grid.laplace_interpolate(np.ones(grid.n_face), dim="nope")
    line = xa.Ugrid1d(np.arange(3.0), np.zeros(3), -1, np.array([[0, 1], [1, 2]]))
    with pytest.raises(ValueError, match="Laplace interpolation along edges is not allowed."):
        line.laplace_interpolate(np.ones(2), dim="edge")
    with pytest.raises(ValueError, match='"abc" is not a valid interpolator.'):
        line.interpolate_na(np.ones(2), method="abc")


def test_kdtree_upper_bound_is_strict():
    """The nearest fill keeps NaN at exactly max_distance: KDTree.query(distance_upper_bound=d) does the same."""
    xy = np.array([[0.0, 0.0], [0.5, 0.0], [3.0, 4.0]])
    tree = KDTree(xy[[0]])
    d, j = tree.query(xy[1:], distance_upper_bound=0.5)
    assert np.isinf(d[0]) and j[0] == 1
    d, j = tree.query(xy[1:], distance_upper_bound=np.nextafter(0.5, 1.0))
    assert d[0] == 0.5 and j[0] == 0
    d, j = tree.query(xy[[2]], distance_upper_bound=5.0)
    assert np.isinf(d[0])


def test_helper_reproduces_reference_chain():
    data = np.array([1.0, np.nan, np.nan, np.nan, 5.0])
    np.testing.assert_allclose(reference_laplace(data, chain(5), False), np.arange(1.0, 6.0))
