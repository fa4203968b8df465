"""
Expected values of the fills, computed on the host with scipy inside the tests (the product never imports this): the
reference's Laplace system (xugrid/ugrid/interpolate.py:286-329) solved by ``spsolve``, its adjacency construction
(ugrid/connectivity.py:487-531) written out edge by edge, and ``scipy.spatial.KDTree`` for the nearest fill.
"""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph
from scipy.sparse.linalg import spsolve
from scipy.spatial import KDTree


def scaled_system(data, conn, labels, use_weights):
    """-> (A_scaled, rhs_scaled, scale, unknown) built as the reference builds them."""
    isnull = np.isnan(data)
    all_null = np.ones(labels.max() + 1, dtype=bool)
    np.logical_and.at(all_null, labels, isnull)
    all_null = all_null[labels]
    known = ~isnull & ~all_null
    unknown = isnull & ~all_null
    W = conn.astype(np.float64, copy=True)
    if not use_weights:
        W.data[:] = 1.0
    D = np.asarray(W.sum(axis=1)).ravel()
    L = sparse.diags(D) - W
    A = L[unknown][:, unknown]
    rhs = -L[unknown][:, known].dot(data[known])
    diag = A.diagonal().copy()
    diag[diag <= 0.0] = 1e-10 * abs(diag).mean()
    scale = 1.0 / np.sqrt(diag)
    S = sparse.diags(scale)
    return (S @ A @ S).tocsr(), scale * rhs, scale, unknown


def reference_laplace(data, conn, use_weights, labels=None):
    if labels is None:
        labels = csgraph.connected_components(conn)[1]
    A, b, scale, unknown = scaled_system(data, conn, labels, use_weights)
    out = data.copy()
    if unknown.any():
        out[unknown] = scale * np.atleast_1d(spsolve(A.tocsc(), b))
    return out


def scaled_residual(filled, data, conn, use_weights):
    """||A_s y - b_s|| of a fill, y = filled[U] / scale: what the CG stopping rule measures."""
    labels = csgraph.connected_components(conn)[1]
    A, b, scale, unknown = scaled_system(data, conn, labels, use_weights)
    return float(np.linalg.norm(A @ (filled[unknown] / scale) - b))


def edges_of_faces(faces):
    """Unique undirected edges (lexicographic (lo, hi)) and, per edge, its faces in ascending order."""
    pairs = {}
    for f, row in enumerate(faces):
        ring = [v for v in row if v >= 0]
        for a, b in zip(ring, ring[1:] + ring[:1]):
            if a != b:
                pairs.setdefault((min(a, b), max(a, b)), set()).add(f)
    keys = sorted(pairs)
    return keys, [sorted(pairs[k]) for k in keys]


def reference_face_face(faces):
    keys, owners = edges_of_faces(faces)
    rows, cols, data = [], [], []
    for e, fs in enumerate(owners):
        if len(fs) == 2:
            rows += [fs[0], fs[1]]
            cols += [fs[1], fs[0]]
            data += [e, e]
    n = len(faces)
    return sparse.coo_matrix((data, (rows, cols)), shape=(n, n)).tocsr()


def reference_node_node(faces, n_node):
    keys, _ = edges_of_faces(faces)
    rows = [a for a, b in keys] + [b for a, b in keys]
    cols = [b for a, b in keys] + [a for a, b in keys]
    data = list(range(len(keys))) * 2
    return sparse.coo_matrix((data, (rows, cols)), shape=(n_node, n_node)).tocsr()


def reference_weights(conn, xy):
    coo = conn.tocoo()
    d = np.linalg.norm(xy[coo.col] - xy[coo.row], axis=1)
    return d.mean() / d


def reference_nearest(xy, data, max_distance=np.inf):
    """KDTree fill of one slice: null entries take the nearest valid value strictly closer than max_distance."""
    out = data.copy()
    valid = ~np.isnan(data)
    tree = KDTree(xy[valid])
    d, j = tree.query(xy[~valid], distance_upper_bound=max_distance)
    found = np.isfinite(d)
    vals = np.full(d.shape, np.nan)
    vals[found] = data[valid][j[found]]
    out[~valid] = vals
    return out, d


def chain(n=5):
    """The reference's test_interpolate.py chain: nodes 0..n-1 joined in a line, weights 1."""
    i = np.arange(n - 1)
    return sparse.coo_matrix((np.ones(2 * (n - 1)), (np.r_[i, i + 1], np.r_[i + 1, i])), shape=(n, n)).tocsr()


def mixed_faces():
    """A small mixed triangle / quad mesh (3 x 2 node lattice plus a fan), -1 filled."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 1.0], [1.0, 2.0], [2.6, 0.5]])
    faces = np.array([[0, 1, 4, 3], [1, 2, 5, 4], [3, 4, 6, -1], [4, 5, 6, -1], [2, 7, 5, -1]])
    return xy, faces
