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


def brute_nearest(xy, data, max_distance=np.inf, chunk=2048):
    """Source index per point of the nearest fill of one slice, or -1: every valid point is its own source; a null point
    takes the valid point of smallest squared distance ``dx*dx + dy*dy`` in float64 -- the kernel's own arithmetic (no
    fused multiply-add), so decisions are bit-identical -- kept strictly below ``max_distance**2``, lowest index among
    equal distances."""
    xy = np.asarray(xy, dtype=np.float64)
    valid = ~np.isnan(data)
    src = np.where(valid, np.arange(len(data)), -1)
    vidx = np.nonzero(valid)[0]
    null = np.nonzero(~valid)[0]
    if vidx.size == 0 or null.size == 0:
        return src
    md2 = max_distance * max_distance
    vx, vy = xy[vidx, 0], xy[vidx, 1]
    step = max(1, chunk * 4096 // max(vidx.size, 1))  # ~8M distances per chunk
    for c0 in range(0, null.size, step):
        rows = null[c0:c0 + step]
        dx = vx[None, :] - xy[rows, 0][:, None]
        dy = vy[None, :] - xy[rows, 1][:, None]
        d2 = dx * dx + dy * dy
        j = np.argmin(d2, axis=1)  # the first of equal minima: the lowest index (vidx is ascending)
        best = d2[np.arange(rows.size), j]
        src[rows] = np.where(best < md2, vidx[j], -1)
    return src


def kdtree_nearest(xy, data):
    """``brute_nearest`` (no distance bound) for point sets too large for brute force: the KDTree distance, the candidates
    in a ball slightly wider than it, then the kernel's squared distance and the lowest index among the closest."""
    xy = np.asarray(xy, dtype=np.float64)
    valid = ~np.isnan(data)
    src = np.where(valid, np.arange(len(data)), -1)
    vidx = np.nonzero(valid)[0]
    null = np.nonzero(~valid)[0]
    if vidx.size == 0 or null.size == 0:
        return src
    tree = KDTree(xy[vidx])
    d, _ = tree.query(xy[null])
    balls = tree.query_ball_point(xy[null], d * (1.0 + 1e-9) + 1e-300)
    for i, cand in zip(null, balls):
        j = vidx[np.sort(np.asarray(cand, dtype=np.int64))]
        dx = xy[j, 0] - xy[i, 0]
        dy = xy[j, 1] - xy[i, 1]
        d2 = dx * dx + dy * dy
        src[i] = j[np.argmin(d2)]
    return src


def reference_cg(A, b, atol=0.0, rtol=1e-5, maxiter=None):
    """scipy 1.15's ``sparse.linalg.cg`` loop without a preconditioner, restated so every iterate is kept: x0 = 0;
    ``||r|| < max(atol, rtol ||b||)`` is tested at the top of each pass; a loop that runs out reports ``maxiter``.
    -> (iterates [x_0, x_1, ...], info, residual norms at the tests made, tolerance).  ``info`` 0 is convergence and
    ``len(iterates) - 1`` the iteration count either way."""
    b = np.asarray(b, dtype=np.float64)
    bnrm2 = np.linalg.norm(b)
    tol = max(float(atol), float(rtol) * float(bnrm2))
    x = np.zeros_like(b)
    iterates, norms = [x.copy()], []
    if bnrm2 == 0:
        return iterates, 0, norms, tol
    if maxiter is None:
        maxiter = 10 * len(b)
    r = b.copy()
    rho_prev, p = None, None
    for iteration in range(maxiter):
        norms.append(np.linalg.norm(r))
        if norms[-1] < tol:
            return iterates, 0, norms, tol
        rho_cur = np.dot(r, r)
        if iteration > 0:
            p = p * (rho_cur / rho_prev) + r
        else:
            p = r.copy()
        q = A @ p
        alpha = rho_cur / np.dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        rho_prev = rho_cur
        iterates.append(x.copy())
    return iterates, maxiter, norms, tol
