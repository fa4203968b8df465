"""
CPU: the host side of the fills -- adjacency matrices against the reference's construction, argument validation before
any device call, the KDTree distance rule the nearest fill follows, and the test helper's known answer.
"""
import numpy as np
import pytest
from scipy import sparse
from scipy.spatial import KDTree

import xugrid_amd as xa
from fill_cases import (brute_nearest, chain, kdtree_nearest, mixed_faces, reference_cg, reference_face_face,
                        reference_laplace, reference_nearest, reference_node_node, reference_weights, scaled_system)


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


# ---- the host references the device fills are compared with (tests/test_gpu_fill_edges.py)
@pytest.mark.parametrize("max_distance", [np.inf, 0.02])
def test_brute_nearest_equals_kdtree_without_ties(max_distance):
    rng = np.random.default_rng(5)
    xy = rng.random((3000, 2))
    data = rng.normal(size=3000)
    data[rng.random(3000) < 0.4] = np.nan
    data[np.hypot(xy[:, 0] - 0.3, xy[:, 1] - 0.6) < 0.15] = np.nan
    src = brute_nearest(xy, data, max_distance, chunk=64)  # several chunks
    expected, _ = reference_nearest(xy, data, max_distance)
    out = np.where(src >= 0, data[np.maximum(src, 0)], np.nan)
    assert np.array_equal(out, expected, equal_nan=True)
    valid = ~np.isnan(data)
    np.testing.assert_array_equal(src[valid], np.nonzero(valid)[0])
    if np.isinf(max_distance):
        np.testing.assert_array_equal(kdtree_nearest(xy, data), src)
    else:
        assert (src == -1).any()


def test_brute_nearest_ties_and_strict_bound():
    xy = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 0.0], [1.0, 1.0], [1.0, -1.0], [5.0, 5.0], [2.0, 0.0]])
    data = np.array([10.0, 11.0, np.nan, np.nan, 12.0, np.nan, np.nan])
    # point 2 is 1 from 0, 1 and 4: the lowest index, 0; point 3 is sqrt(2) from 0 and 1 and 2 from 4: 0; point 5 is
    # nearest to 1; point 6 coincides with 1 (distance 0)
    np.testing.assert_array_equal(brute_nearest(xy, data), [0, 1, 0, 0, 4, 1, 1])
    np.testing.assert_array_equal(kdtree_nearest(xy, data), [0, 1, 0, 0, 4, 1, 1])
    # strictly below max_distance: at exactly 1.0 point 2 stays empty, just above it fills
    np.testing.assert_array_equal(brute_nearest(xy, data, 1.0), [0, 1, -1, -1, 4, -1, 1])
    np.testing.assert_array_equal(brute_nearest(xy, data, np.nextafter(1.0, 2.0)), [0, 1, 0, -1, 4, -1, 1])
    np.testing.assert_array_equal(brute_nearest(xy, data, 0.0), [0, 1, -1, -1, 4, -1, -1])
    assert (brute_nearest(xy, np.full(7, np.nan)) == -1).all()


def cg_case():
    xy, faces = xa.meshgen.triangle_mesh(300, 0)
    c = xy[faces].mean(axis=1)  # triangles: the centroid is the vertex mean
    data = np.sin(3 * c[:, 0]) + np.cos(2 * c[:, 1])
    data[np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) < 0.3] = np.nan
    conn = reference_face_face(faces)
    conn.data = reference_weights(conn, c)
    labels = sparse.csgraph.connected_components(conn)[1]
    return scaled_system(data, conn, labels, True)


@pytest.mark.parametrize("maxiter", [0, 1, 2, 5, 24, 25, 1000])
def test_reference_cg_equals_scipy(maxiter):
    from scipy.sparse.linalg import cg

    A, b, _, _ = cg_case()
    iterates, info, norms, tol = reference_cg(A, b, atol=1e-4, rtol=0.0, maxiter=maxiter)
    x, sinfo = cg(A, b, atol=1e-4, rtol=0.0, maxiter=maxiter)
    assert info == sinfo
    np.testing.assert_allclose(iterates[-1], x, rtol=0.0, atol=1e-12)
    if maxiter == 0:  # scipy returns x0 = 0 with info 0; so does the device (k_cg_start)
        assert info == 0 and len(iterates) == 1 and not x.any()
    elif info == 0:
        assert norms[-1] < tol and all(r >= tol for r in norms[:-1]) and len(iterates) == len(norms)
    else:
        assert info == maxiter and len(iterates) == maxiter + 1 and len(norms) == maxiter
    if maxiter == 1000:
        assert info == 0 and 25 < len(iterates) - 1 < 1000


def test_reference_cg_zero_rhs():
    A, b, _, _ = cg_case()
    iterates, info, norms, _ = reference_cg(A, np.zeros_like(b), atol=1e-4, rtol=0.0, maxiter=10)
    assert info == 0 and len(iterates) == 1 and not iterates[0].any() and norms == []
