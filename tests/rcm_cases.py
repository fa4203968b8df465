"""Yardsticks and fixtures of the renumbering tests (test_rcm_cpu.py, test_gpu_rcm.py): numpy / scipy only.

``sequential`` is the loop of ``scipy.sparse.csgraph.reverse_cuthill_mckee`` (symmetric mode) restated with a STABLE argsort of
the degrees; scipy's own argsort is numpy's default, unstable one, so scipy may seed a component at any of several unvisited
vertices of equal least degree.  ``level_form`` is the level-synchronous rule the device kernels follow (include/xugrid_amd.h:
xr_graph_rcm_dev).  ``seed_ties`` counts the seed choices at which scipy's answer depends on its tie order."""
import numpy as np
from scipy import sparse
from scipy.spatial import Delaunay


def canonical(A):
    """CSR with ascending columns and no repeated entries."""
    A = sparse.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def degrees(A):
    """scipy's ``_node_degrees``: the row length, plus one where the row has a diagonal entry."""
    A = canonical(A)
    return np.diff(A.indptr) + _has_diagonal(A)


def _has_diagonal(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    out = np.zeros(A.shape[0], dtype=np.int64)
    out[rows[A.indices == rows]] = 1  # (a stored diagonal entry counts whatever its value)
    return out


def _bfs(A, seeds_in_order, on_seed=None):
    """scipy's loop over the given seed order -> the order before its reversal."""
    A = canonical(A)
    n = A.shape[0]
    indptr, indices = A.indptr, A.indices
    degree = degrees(A)
    visited = np.zeros(n, dtype=bool)
    order = []
    for seed in seeds_in_order:
        if visited[seed]:
            continue
        if on_seed is not None:
            on_seed(seed, visited, degree)
        visited[seed] = True
        order.append(seed)
        level_start, level_end = len(order) - 1, len(order)
        while level_start < level_end:
            for ii in range(level_start, level_end):
                i = order[ii]
                new = []
                for j in indices[indptr[i]:indptr[i + 1]]:
                    if not visited[j]:
                        visited[j] = True
                        new.append(j)
                new.sort(key=lambda j: degree[j])  # (stable, as scipy's insertion sort of the one row's new entries)
                order.extend(new)
            level_start, level_end = level_end, len(order)
    return np.array(order, dtype=np.int64).reshape(-1)


def sequential(A):
    """scipy's routine with ``np.argsort(degree, kind="stable")``."""
    return _bfs(A, np.argsort(degrees(A), kind="stable"))[::-1].copy()


def seed_ties(A):
    """Seed choices of ``sequential`` at which more than one unvisited vertex has the least degree (0: scipy's answer does
    not depend on how its argsort orders equal degrees)."""
    ties = []

    def on_seed(seed, visited, degree):
        open_degrees = degree[~visited]
        ties.append(int((open_degrees == open_degrees.min()).sum()) > 1)

    _bfs(A, np.argsort(degrees(A), kind="stable"), on_seed)
    return int(sum(ties))


def level_form(A):
    """-> (order, widths).  Seeds in (degree, id) order; each unvisited neighbour j of level L takes as parent the smallest
    position in the order among its neighbours in level L; level L + 1 is the claimed vertices sorted by (parent position,
    degree[j], j); a seed is a level of one; the order is reversed at the end.  ``widths``: the size of every level."""
    A = canonical(A)
    n = A.shape[0]
    indptr, indices = A.indptr, A.indices
    degree = degrees(A)
    seeds = np.lexsort((np.arange(n), degree))
    pos = np.full(n, -1, dtype=np.int64)
    order = np.empty(n, dtype=np.int64)
    placed, cursor, widths = 0, 0, []
    while placed < n:
        while pos[seeds[cursor]] >= 0:
            cursor += 1
        level = seeds[cursor:cursor + 1]
        while level.size:
            order[placed:placed + level.size] = level
            pos[level] = np.arange(placed, placed + level.size)
            placed += level.size
            widths.append(int(level.size))
            lengths = indptr[level + 1] - indptr[level]
            offsets = np.arange(lengths.sum()) - np.repeat(np.cumsum(lengths) - lengths, lengths)
            cols = indices[np.repeat(indptr[level], lengths) + offsets]
            parents = np.repeat(pos[level], lengths)
            free = pos[cols] < 0
            cols, parents = cols[free], parents[free]
            parent = np.full(n, n, dtype=np.int64)
            np.minimum.at(parent, cols, parents)
            claimed = np.unique(cols)
            level = claimed[np.lexsort((claimed, degree[claimed], parent[claimed]))]
    return order[::-1].copy(), widths


# ---- fixtures
def face_graph(faces):
    """The face-face adjacency (one entry per pair of faces sharing an edge) of a dense face table with -1 fill, as canonical
    CSR with unit data."""
    faces = np.asarray(faces, dtype=np.int64)
    n_face, m = faces.shape
    valid = faces >= 0
    count = valid.sum(axis=1)
    slot = np.arange(m)[None, :]
    successor = np.take_along_axis(faces, np.where(slot + 1 < count[:, None], slot + 1, 0), axis=1)
    a, b, f = faces[valid], successor[valid], np.repeat(np.arange(n_face), count)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    by = np.lexsort((f, hi, lo))
    lo, hi, f = lo[by], hi[by], f[by]
    same = (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])
    r, c = f[:-1][same], f[1:][same]
    A = sparse.coo_matrix((np.ones(2 * r.size), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n_face, n_face))
    A = canonical(A)
    A.data[:] = 1.0
    return A


def delaunay(n_points, seed=0):
    """Delaunay triangles of uniform random points in the unit square -> (node_xy, faces), faces counter-clockwise."""
    xy = np.random.default_rng(seed).random((n_points, 2))
    faces = Delaunay(xy).simplices.astype(np.int64)
    u, v = xy[faces[:, 1]] - xy[faces[:, 0]], xy[faces[:, 2]] - xy[faces[:, 0]]
    clockwise = (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]) < 0
    faces[clockwise] = faces[clockwise][:, ::-1]
    return xy, faces


def with_ear(xy, faces):
    """One more triangle on a hull edge (the last face, on a new node outside the hull): its degree is 1."""
    faces = np.asarray(faces, dtype=np.int64)
    tri = faces[:, :3]
    a, b = tri.ravel(), np.roll(tri, -1, axis=1).ravel()
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * len(xy) + hi
    uniq, first, counts = np.unique(key, return_index=True, return_counts=True)
    at = first[counts == 1][0]  # a hull edge, as the face at // 3 walks it
    p, q = xy[a[at]], xy[b[at]]
    out = np.array([q[1] - p[1], p[0] - q[0]])  # (the right of a counter-clockwise face's edge points outward)
    apex = 0.5 * (p + q) + 0.5 * out
    ear = np.full((1, faces.shape[1]), -1, dtype=np.int64)
    ear[0, :3] = [b[at], a[at], len(xy)]
    return np.vstack([xy, apex]), np.vstack([faces, ear])


def isolated_triangles(count, x0=10.0):
    """``count`` triangles that share nothing -> (node_xy, faces)."""
    k = np.arange(count, dtype=np.float64)
    xy = np.column_stack([x0 + 2.0 * np.repeat(k, 3) + np.tile([0.0, 1.0, 0.0], count), np.tile([0.0, 0.0, 1.0], count)])
    return xy, np.arange(3 * count, dtype=np.int64).reshape(count, 3)


def join(*meshes):
    """Meshes side by side in one table (no shared nodes), faces in the order given."""
    xys, tables, base = [], [], 0
    for xy, faces in meshes:
        xys.append(xy)
        tables.append(np.where(faces >= 0, faces + base, -1))
        base += len(xy)
    return np.vstack(xys), np.vstack(tables)


def hub_graph(n_leaves, tails=(), diagonal=()):
    """A star: vertex 0 joined to the leaves 1 .. n_leaves.  ``tails``: (leaf, length) pairs, a chain of ``length`` further
    vertices hung on that leaf (the leaf's degree becomes 2).  ``diagonal``: vertices that get a diagonal entry."""
    rows, cols = [np.zeros(n_leaves, dtype=np.int64)], [np.arange(1, n_leaves + 1)]
    n = n_leaves + 1
    for leaf, length in tails:
        chain = np.concatenate([[leaf], np.arange(n, n + length)])
        rows.append(chain[:-1])
        cols.append(chain[1:])
        n += length
    r, c = np.concatenate(rows), np.concatenate(cols)
    d = np.asarray(diagonal, dtype=np.int64)
    A = sparse.coo_matrix((np.ones(2 * r.size + d.size), (np.concatenate([r, c, d]), np.concatenate([c, r, d]))), shape=(n, n))
    return canonical(A)
