"""
Cases and yardsticks of the network fill (Ugrid1d.interpolate_na(metric="network"), Ugrid1d.network_distance), shared by
tests/test_netfill_cpu.py and tests/test_gpu_netfill.py.  numpy and scipy only.

``reference_graph`` / ``reference_fill`` restate what xugrid/ugrid/ugrid1d.py ``_nearest_interpolate`` does (pinned to the
reference's own output by tests/golden/netfill_known.json); ``fixed_point`` restates the contract of ``xr_graph_nearest_dev``
in include/xugrid_amd.h.  One deliberate difference: the reference builds its node graph without a shape, so unused nodes at
the end of the node table shrink it (and its fill then fails on the size mismatch); here every graph has one row per node.
"""
import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import dijkstra


# ---- yardsticks ---------------------------------------------------------------------------------------------------------------
def edge_length(xy, edges):
    d = xy[edges[:, 1]] - xy[edges[:, 0]]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def edge_edge_connectivity(edges, n_node):
    """Row i: every other edge at either node of edge i; data = the shared node."""
    n_edge = len(edges)
    node_edge = sparse.coo_matrix((np.repeat(np.arange(n_edge), 2), (edges.ravel(), np.repeat(np.arange(n_edge), 2))),
                                  shape=(n_node, n_edge)).tocsr()
    node_edge.sort_indices()
    own, other, shared = [], [], []
    for e, (a, b) in enumerate(edges):
        for v in (a, b):
            row = node_edge.indices[node_edge.indptr[v]:node_edge.indptr[v + 1]]
            row = row[row != e]
            own.append(np.full(row.size, e)), other.append(row), shared.append(np.full(row.size, v))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)  # noqa: E731
    return sparse.coo_matrix((cat(shared), (cat(own), cat(other))), shape=(n_edge, n_edge)).tocsr()


def reference_graph(xy, edges, facet):
    """scipy CSR of the distances along the network: between nodes the length of the joining edge (a coo of the edge ids made
    into a csr, then ``edge_length[data]``), between edges half of the two lengths (``edge_edge_connectivity`` made into a coo,
    then ``0.5 * (L[row] + L[col])``)."""
    n_node, n_edge = len(xy), len(edges)
    length = edge_length(xy, edges)
    if facet == "node":
        i, j, e = edges[:, 0], edges[:, 1], np.arange(n_edge)
        graph = sparse.coo_matrix((np.concatenate([e, e]), (np.concatenate([i, j]), np.concatenate([j, i]))),
                                  shape=(n_node, n_node)).tocsr()
        return sparse.csr_matrix((length[graph.data], graph.indices, graph.indptr), shape=graph.shape)
    coo = edge_edge_connectivity(edges, n_node).tocoo()
    return sparse.csr_matrix((0.5 * (length[coo.row] + length[coo.col]), (coo.row, coo.col)), shape=(n_edge, n_edge))


def csr_arrays(graph):
    """(indptr, indices, data) with ascending columns per row, as the device keeps them."""
    graph = graph.copy()
    graph.sort_indices()
    return graph.indptr.astype(np.int64), graph.indices.astype(np.int64), graph.data.astype(np.float64)


def reference_fill(data, graph, max_distance=None):
    """A NaN takes the value of the source scipy's multi-source dijkstra names for it; unreached entries stay NaN."""
    isnull = np.isnan(data)
    if isnull.all():
        raise ValueError("All values are NA.")
    limit = np.inf if max_distance is None else max_distance
    _, _, index = dijkstra(csgraph=graph, indices=np.flatnonzero(~isnull), return_predecessors=True, limit=limit, min_only=True)
    found = index != -9999
    out = data.copy()
    out[found] = data[index[found]]
    return out


def reference_nearest(graph, is_source, max_distance=None):
    """(distance, source) of scipy's multi-source dijkstra, inf / -1 where unreached."""
    limit = np.inf if max_distance is None else max_distance
    distance, _, source = dijkstra(csgraph=graph, indices=np.flatnonzero(is_source), return_predecessors=True, limit=limit,
                                   min_only=True)
    return distance, np.where(source == -9999, -1, source).astype(np.int64)


def fixed_point(graph, is_source, limit=np.inf):
    """The contract of xr_graph_nearest_dev as a plain relaxation: every round each vertex takes the lexicographic minimum of
    its own (d, s) and of (d_u + w, s_u) over its entries with d_u + w <= limit, until nothing changes.  -> (d, s), inf / -1."""
    indptr, indices, w = csr_arrays(graph)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    none = n  # (sorts behind every id)
    d = np.where(is_source, 0.0, np.inf)
    s = np.where(is_source, np.arange(n), none)
    while True:
        c = d[indices] + w
        ok = np.isfinite(d[indices]) & (c <= limit)
        r, c, sc = rows[ok], c[ok], s[indices][ok]
        order = np.lexsort((sc, c, r))
        r, c, sc = r[order], c[order], sc[order]
        first = np.ones(r.size, dtype=bool)
        first[1:] = r[1:] != r[:-1]
        r, c, sc = r[first], c[first], sc[first]
        better = (c < d[r]) | ((c == d[r]) & (sc < s[r]))
        if not better.any():
            break
        d[r[better]], s[r[better]] = c[better], sc[better]
    return d, np.where(s == none, -1, s).astype(np.int64)


# ---- networks: (xy float64 (n_node, 2), edges int64 (n_edge, 2)) -----------------------------------------------------------------
def single_edge():
    return np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([[1, 0]], dtype=np.int64)


def chain(n_node, seed=0):
    """A path with irregular spacing (no two sums of lengths tie)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(0.5, 1.5, n_node))
    xy = np.column_stack([x, 0.1 * np.sin(x)])
    return xy, np.column_stack([np.arange(n_node - 1), np.arange(1, n_node)]).astype(np.int64)


def random_network(n_node=2000, extra=0.1, seed=1):
    """A random tree (node i hangs on a random earlier node) plus ``extra * n_node`` further edges; nodes in the unit square, the
    node numbering, the edge order and the edges' directions shuffled."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n_node, 2))
    pairs = {(int(rng.integers(0, i)), i) for i in range(1, n_node)}
    while len(pairs) < n_node - 1 + int(extra * n_node):
        a, b = sorted(int(v) for v in rng.integers(0, n_node, 2))
        if a != b:
            pairs.add((a, b))
    edges = np.array(sorted(pairs), dtype=np.int64)
    edges = rng.permutation(n_node)[edges]
    edges = edges[rng.permutation(len(edges))]
    flip = rng.random(len(edges)) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    return xy, np.ascontiguousarray(edges)


def unused_nodes():
    """A random network whose node table also holds nodes no edge names: some in the middle, some at the end."""
    xy, edges = random_network(300, 0.1, seed=2)
    rng = np.random.default_rng(3)
    xy = np.concatenate([xy, rng.random((40, 2))])
    # nodes 100 .. 119 and 320 .. 339 are the unused ones: the used ids above 99 move up by 20
    edges = np.where(edges >= 100, edges + 20, edges)
    return xy, edges


def hub(degree, seed=4):
    """One node with ``degree`` spokes, each spoke two edges long; the hub is not node 0 and the edges are shuffled."""
    rng = np.random.default_rng(seed)
    angle = np.sort(rng.uniform(0.0, 2.0 * np.pi, degree))
    radius = rng.uniform(1.0, 2.0, degree)
    inner = np.column_stack([radius * np.cos(angle), radius * np.sin(angle)])
    xy = np.concatenate([inner[:5], [[0.0, 0.0]], inner[5:], 2.0 * inner])  # the hub is node 5
    first = np.concatenate([np.arange(5), np.arange(6, degree + 1)])
    edges = np.concatenate([np.column_stack([np.full(degree, 5), first]), np.column_stack([first, degree + 1 + np.arange(degree)])])
    edges = edges[rng.permutation(len(edges))]
    return xy, np.ascontiguousarray(edges, dtype=np.int64)


def coincident():
    """Nodes 1 and 2 lie on each other, joined by an edge of length zero."""
    xy = np.array([[0.0, 0.0], [1.0, 0.5], [1.0, 0.5], [2.5, 0.25], [1.0, 2.0]])
    return xy, np.array([[0, 1], [2, 1], [2, 3], [4, 1]], dtype=np.int64)


def hairpin():
    """Two parallel branches 0.3 apart, joined at x = 10.  Branch A: nodes 0 .. 101 at y = 0, its far end at x = -0.2, then
    x = 0, 0.1, .. 10; branch B: nodes 102 .. 202 at y = 0.3 from its far end at x = 0 to x = 10.  -> (xy, edges, far end of A,
    far end of B, nodes of A, nodes of B).  Along the network every node is nearer to its own branch's far end (the joint of A:
    10.2 against 10.3); in the plane the nodes of A beyond x = 0.125 are nearer to B's far end."""
    xa = np.concatenate([[-0.2], np.arange(101) * 0.1])
    xb = np.arange(101) * 0.1
    xy = np.concatenate([np.column_stack([xa, np.zeros(102)]), np.column_stack([xb, np.full(101, 0.3)])])
    a, b = np.arange(102), 102 + np.arange(101)
    edges = np.concatenate([np.column_stack([a[:-1], a[1:]]), np.column_stack([b[:-1], b[1:]]), [[a[-1], b[-1]]]])
    return xy, edges.astype(np.int64), 0, 102, a, b


def unit_path(n_node=9):
    xy = np.column_stack([np.arange(n_node, dtype=np.float64), np.zeros(n_node)])
    return xy, np.column_stack([np.arange(n_node - 1), np.arange(1, n_node)]).astype(np.int64)


def dyadic_path():
    """Lengths 0.5, 0.25, 0.5, 0.25, ..: every distance from node 0 is exact in binary."""
    x = np.concatenate([[0.0], np.cumsum(np.tile([0.5, 0.25], 4))])
    return np.column_stack([x, np.zeros(x.size)]), np.column_stack([np.arange(8), np.arange(1, 9)]).astype(np.int64)


def two_components():
    """A chain of 40 nodes and, apart from it, a chain of 25."""
    xy1, e1 = chain(40, seed=5)
    xy2, e2 = chain(25, seed=6)
    return np.concatenate([xy1, xy2 + [0.0, 50.0]]), np.concatenate([e1, e2 + 40])


def n_of(xy, edges, facet):
    return len(xy) if facet == "node" else len(edges)


def masked_data(n, valid_fraction, seed):
    """Distinct values (the value names its source), NaN but for ``valid_fraction`` of the entries."""
    rng = np.random.default_rng(seed)
    data = 1000.0 + np.arange(n, dtype=np.float64)
    data[rng.random(n) >= valid_fraction] = np.nan
    if np.isnan(data).all():
        data[0] = 1000.0
    return data


SLICE_LIMIT = 0.7


def slice_data(n):
    """Three slices with three masks, the middle one without NaN (edge data of ``random_network``, filled within SLICE_LIMIT)."""
    return np.stack([masked_data(n, 0.05, seed=20), 1000.0 + np.arange(n), masked_data(n, 0.5, seed=21)])


def distance_case(xy, edges, facet, max_distance):
    """Sources of the network_distance tests (the mask of the "sparse" fill cases) -> (mask, the ids in descending order,
    scipy's distance, scipy's source)."""
    mask = ~np.isnan(masked_data(n_of(xy, edges, facet), 0.05, seed=12))
    return (mask, np.flatnonzero(mask)[::-1].copy()) + reference_nearest(reference_graph(xy, edges, facet), mask, max_distance)


# name -> (network, valid fraction, max_distance): the tie-free cases of the comparison with scipy.  The limited ones leave
# some entries NaN (checked by the CPU test).
FILL_CASES = {
    "sparse": (random_network, 0.05, None),
    "sparse_limited": (random_network, 0.05, 0.6),
    "dense": (random_network, 0.30, None),
    "dense_limited": (random_network, 0.30, 0.4),
}

# the small cases tests/golden/gen_netfill.py runs through the reference itself
KNOWN_CASES = {
    "tree40": (lambda: random_network(40, 0.1, seed=7), 0.2, None),
    "tree40_limited": (lambda: random_network(40, 0.1, seed=7), 0.2, 0.6),
    "chain30": (lambda: chain(30, seed=8), 0.1, None),
    "hub12": (lambda: hub(12, seed=9), 0.15, None),
}
