"""
Host-side (numpy) mesh algebra needed around the hot path -- the subset of
xugrid/ugrid/connectivity.py used by the regridders: polygon closing
(:372-382), dense connectivity inversion (:325-333), unique edges (:419-457) and the raster
bounds helper of xugrid/conversion.py:272-282.  Face areas and centroids are computed on the
device (xugrid_amd/csrc/xr_mesh_front.hip, xr_mesh_derived.hip), not here.
Also the adjacency matrices of the fills (xugrid/ugrid/connectivity.py:487-531): face -> face through shared edges and
node -> node along edges, both symmetric scipy CSR whose data is the id of the connecting edge.
"""
import numpy as np
from scipy import sparse

IntDType = np.intp
FILL_VALUE = -1


def bounds1d_to_vertices(bounds):
    """(n, 2) monotonic cell bounds -> n + 1 vertices in the bounds' own direction."""
    diff = np.diff(bounds, axis=0)
    if (diff >= 0.0).all():
        return np.concatenate((bounds[:, 0], bounds[-1:, 1]))
    if (diff <= 0.0).all():
        return np.concatenate((bounds[:, 1], bounds[-1:, 0]))
    raise ValueError("Bounds are not monotonic ascending or monotonic descending")


def close_polygons(face_node_connectivity):
    """Append node 0 and replace every fill slot by node 0; also return the fill mask."""
    n, m = face_node_connectivity.shape
    closed = np.full((n, m + 1), FILL_VALUE, dtype=IntDType)
    closed[:, :-1] = face_node_connectivity
    isfill = closed == FILL_VALUE
    first = np.broadcast_to(face_node_connectivity[:, :1], closed.shape)
    closed = np.where(isfill, first, closed)
    return closed, isfill


def _dense_to_coo(conn):
    n, m = conn.shape
    i = np.repeat(np.arange(n, dtype=IntDType), m)
    j = conn.ravel()
    valid = j != FILL_VALUE
    return i[valid], j[valid]


def invert_dense_to_sparse(conn, n_rows=None):
    """(a -> b) dense table with -1 fill  ->  scipy CSR of (b -> a), sorted column indices."""
    i, j = _dense_to_coo(conn)
    n_b = int(j.max()) + 1 if j.size else 0
    if n_rows is not None:
        n_b = max(n_b, n_rows)
    mat = sparse.coo_matrix((i, (j, i)), shape=(n_b, conn.shape[0])).tocsr()
    mat.sort_indices()
    return mat


def to_dense(mat):
    """scipy CSR -> dense table with -1 fill, entries in column order."""
    n = mat.shape[0]
    counts = np.diff(mat.indptr)
    m = int(counts.max()) if n else 0
    dense = np.full((n, m), FILL_VALUE, dtype=IntDType)
    rows = np.repeat(np.arange(n), counts)
    cols = np.arange(mat.indices.size) - np.repeat(mat.indptr[:-1], counts)
    dense[rows, cols] = mat.indices
    return dense


def invert_dense(conn):
    return to_dense(invert_dense_to_sparse(conn))


def edge_connectivity(face_node_connectivity):
    """
    Unique undirected edges of the faces.

    Returns ``edge_node_connectivity`` (n_edge, 2) with sorted node pairs in lexicographic
    order and ``face_edge_connectivity`` (n_face, n_max_node) with -1 fill.
    """
    n_face, n_max = face_node_connectivity.shape
    closed, isfill = close_polygons(face_node_connectivity)
    a = closed[:, :-1].ravel()
    b = closed[:, 1:].ravel()
    valid = a != b  # fill slots close onto node 0 -> self edges
    lo = np.minimum(a[valid], b[valid])
    hi = np.maximum(a[valid], b[valid])
    # unique undirected edges through ONE 1-D sort: key = lo * n_node + hi orders the edges
    # lexicographically, exactly like np.unique(pairs, axis=0) but ~10x faster
    n_node = int(max(lo.max(initial=-1), hi.max(initial=-1))) + 1
    key, inverse = np.unique(lo.astype(np.int64) * n_node + hi.astype(np.int64), return_inverse=True)
    edges = np.column_stack([key // max(n_node, 1), key % max(n_node, 1)])
    face_edges = np.full((n_face, n_max), FILL_VALUE, dtype=IntDType)
    face_edges.ravel()[np.nonzero(valid)[0]] = inverse.ravel()
    # compact each row to the left so that fill values trail
    order = np.argsort(face_edges == FILL_VALUE, axis=1, kind="stable")
    face_edges = np.take_along_axis(face_edges, order, axis=1)
    return edges.astype(IntDType), face_edges


def _symmetric_csr(a, b, edge, n):
    """Entries (a, b) and (b, a) with data ``edge`` -> (n, n) CSR, sorted columns, duplicates summed (coo -> csr)."""
    rows = np.concatenate([a, b])
    cols = np.concatenate([b, a])
    data = np.concatenate([edge, edge])
    return sparse.coo_matrix((data, (rows, cols)), shape=(n, n)).tocsr()


def face_face_connectivity(edge_face_connectivity, n_face):
    """Faces that share an edge; data = the shared edge's id."""
    if edge_face_connectivity.shape[1] < 2:  # (the table is as wide as the busiest edge: no edge is shared)
        return sparse.csr_matrix((n_face, n_face), dtype=IntDType)
    inner = edge_face_connectivity[:, 1] != FILL_VALUE
    edge = np.nonzero(inner)[0].astype(IntDType)
    return _symmetric_csr(edge_face_connectivity[inner, 0], edge_face_connectivity[inner, 1], edge, n_face)


def node_node_connectivity(edge_node_connectivity, n_node):
    """Nodes joined by an edge; data = the edge's id."""
    edge = np.arange(len(edge_node_connectivity), dtype=IntDType)
    return _symmetric_csr(edge_node_connectivity[:, 0], edge_node_connectivity[:, 1], edge, n_node)


def edge_edge_connectivity(edge_node_connectivity, node_edge_connectivity):
    """Edges that share a node (xugrid/ugrid/connectivity.py:534-551): row i holds every OTHER edge at either node of edge i,
    columns ascending; data = the shared node (coo -> csr sums the nodes where two edges share both)."""
    n_edge = len(edge_node_connectivity)
    node = np.asarray(edge_node_connectivity).ravel()  # the two nodes of edge 0, of edge 1, ...
    ptr = node_edge_connectivity.indptr
    count = (ptr[1:] - ptr[:-1])[node]  # edges at each of them
    # ... and which: the node -> edge rows ptr[node] .. ptr[node] + count, one after the other
    at = np.repeat(ptr[node] - (np.cumsum(count) - count), count) + np.arange(count.sum())
    other = node_edge_connectivity.indices[at]
    own = np.repeat(np.arange(n_edge, dtype=IntDType), count.reshape(-1, 2).sum(axis=1))
    shared = np.repeat(node, count)
    keep = own != other
    return sparse.coo_matrix((shared[keep], (own[keep], other[keep])), shape=(n_edge, n_edge)).tocsr()


def index_like_device(xy_a, xy_b, tolerance=0.0):
    """``index_like`` (xugrid/ugrid/connectivity.py:38-61) through the device key table: the index that turns ``xy_a`` into
    ``xy_b``.  See ``xugrid_amd.partition.index_like_device`` (imported on use: that module needs the engine)."""
    from .partition import index_like_device as run

    return run(xy_a, xy_b, tolerance)
