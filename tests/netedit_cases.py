"""
Cases and yardsticks of the network edits (Ugrid1d.topology_subset / isel / sel / clip_box / remove_self_loops / merge_partitions /
reindex_like / refine_by_vertices), shared by tests/test_netedit_cpu.py, tests/test_gpu_netedit.py and
tests/netedit_worker_gpu.py.  numpy only.

The ``*_ref`` functions restate what xugrid/ugrid/ugrid1d.py:603-663, :574-601, :714-738, :770-876 and
xugrid/ugrid/partitioning.py:81-116, :137-148 do (pinned to the reference's own output by tests/golden/netedit_known.json).  The
locate step of the refinement, ``EdgeCellTree2d.locate_points`` in the reference, is the brute-force point-to-segment rule of
include/xugrid_amd.h (``locate_ref``).  Two deliberate differences: ``remove_self_loops_ref`` keeps exactly the nodes the kept edges
use (the reference's ``bincount`` mask can be shorter than ``n_node``), and ``merge_ref`` finds equal nodes with ``==`` on doubles, so a
row with NaN equals nothing.
"""
import hashlib

import numpy as np

from netfill_cases import chain, coincident, hub, random_network, single_edge, two_components, unused_nodes  # noqa: F401


# ---- yardsticks -----------------------------------------------------------------------------------------------------------------
def subset_ref(xy, edges, index):
    """-> (xy, edges, node_index) of edges[index]."""
    sub = edges[index]
    node_index = np.unique(sub.ravel())
    return xy[node_index], np.searchsorted(node_index, sub).astype(np.int64).reshape(-1, 2), node_index.astype(np.int64)


def edges_of_nodes_ref(edges, n_node, node_index):
    flag = np.zeros(n_node, dtype=bool)
    flag[node_index] = True
    return np.flatnonzero(flag[edges].any(axis=1)).astype(np.int64)


def box_edges_ref(xy, edges, xmin, ymin, xmax, ymax):
    mid = 0.5 * (xy[edges[:, 0]] + xy[edges[:, 1]])
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((mid[:, 0] >= xmin) & (mid[:, 0] < xmax) & (mid[:, 1] >= ymin) & (mid[:, 1] < ymax)).astype(np.int64)


def remove_self_loops_ref(xy, edges):
    """-> (xy, edges, node_index, edge_index)."""
    edge_index = np.flatnonzero(edges[:, 0] != edges[:, 1]).astype(np.int64)
    return subset_ref(xy, edges, edge_index) + (edge_index,)


def first_occurrence(rows):
    """-> (index of the first row of every set of equal rows, ascending; inverse into those) with == on doubles."""
    seen, index, inverse = {}, [], np.empty(len(rows), dtype=np.int64)
    for i, (x, y) in enumerate(rows.tolist()):
        key = (x + 0.0, y + 0.0)  # (-0.0 + 0.0 is +0.0)
        if x != x or y != y:
            key = ("nan", i)
        if key not in seen:
            seen[key] = len(index)
            index.append(i)
        inverse[i] = seen[key]
    return np.array(index, dtype=np.int64), inverse


def merge_ref(parts):
    """parts: [(xy, edges)] -> dict(xy, edges, node_inverse, node_index [per part], edge_index [per part])."""
    node_off = np.cumsum([0] + [len(xy) for xy, _ in parts])
    edge_off = np.cumsum([0] + [len(e) for _, e in parts])
    all_xy = np.concatenate([xy for xy, _ in parts])
    index, inverse = first_occurrence(all_xy)
    gathered = np.concatenate([inverse[e + off] for (_, e), off in zip(parts, node_off)]).reshape(-1, 2)
    _, first = np.unique(np.sort(gathered, axis=1), axis=0, return_index=True)
    first.sort()
    split = lambda ids, off: [part - o for part, o in zip(np.split(ids, np.searchsorted(ids, off[1:-1])), off)]  # noqa: E731
    return dict(xy=all_xy[index], edges=gathered[first], node_inverse=inverse, node_index=split(index, node_off),
                edge_index=split(first.astype(np.int64), edge_off))


def point_segment(p, a, b):
    """Distance of points p (n, 2) to the closed segments (a, b) (n, 2), the rule of xr_network_refine_dev, in its order of
    operations."""
    ux, uy, vx, vy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], p[:, 0] - a[:, 0], p[:, 1] - a[:, 1]
    len2, dot = ux * ux + uy * uy, vx * ux + vy * uy
    wx, wy = p[:, 0] - b[:, 0], p[:, 1] - b[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        between = np.abs(ux * vy - uy * vx) / np.sqrt(len2)
        return np.where(dot <= 0.0, np.sqrt(vx * vx + vy * vy), np.where(dot >= len2, np.sqrt(wx * wx + wy * wy), between))


def locate_ref(xy, edges, vertices, tolerance):
    """The lowest edge within ``tolerance`` of every vertex, -1 for none: all pairs."""
    out = np.full(len(vertices), -1, dtype=np.int64)
    a, b = xy[edges[:, 0]], xy[edges[:, 1]]
    for v, p in enumerate(vertices):
        with np.errstate(invalid="ignore"):
            hit = np.flatnonzero(point_segment(np.broadcast_to(p, a.shape), a, b) <= tolerance)
        if hit.size:
            out[v] = hit[0]
    return out


def refine_ref(xy, edges, vertices, tolerance, edge_index=None):
    """ugrid1d.py:824-876 -> dict(xy, edges, node_index, parent_edge); ``edge_index``: the located edges when known."""
    n_node, n_edge = len(xy), len(edges)
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    if edge_index is None:
        edge_index = locate_ref(xy, edges, vertices, tolerance)
    if (edge_index == -1).any():
        raise ValueError(f"The following vertices are not located on any edge:\n{vertices[edge_index == -1]}")
    combined = np.concatenate((xy, vertices))
    _, index, inverse = np.unique(combined, return_index=True, return_inverse=True, axis=0)
    not_duplicated = index[inverse.ravel()][n_node:] >= n_node
    new_vertices, edge_index = vertices[not_duplicated], edge_index[not_duplicated]
    d = new_vertices - xy[edges[edge_index, 0]]
    distance = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    repeats = np.bincount(np.concatenate((np.arange(n_edge), edge_index)), minlength=n_edge)
    new_edges = np.repeat(edges, repeats, axis=0)
    order = np.lexsort((distance, edge_index))
    node_index = np.arange(n_node, n_node + len(edge_index))[order]
    i = np.arange(len(new_edges))
    ends = np.cumsum(repeats)
    new_edges[i > np.repeat(ends - repeats, repeats), 0] = node_index
    new_edges[i < np.repeat(ends, repeats) - 1, 1] = node_index
    return dict(xy=np.concatenate((xy, new_vertices)), edges=new_edges.astype(np.int64), node_index=node_index.astype(np.int64),
                parent_edge=np.repeat(np.arange(n_edge), repeats).astype(np.int64))


# ---- refine cases: name -> (xy, edges, vertices, tolerance, every vertex lies EXACTLY on an edge) -----------------------------------
def known():
    """The reference's own test_ugrid1d_refine_by_vertices."""
    xy = np.array([[0.0, 0.0], [5.0, 5.0], [10.0, 5.0], [15.0, 0.0], [15.0, 10.0]])
    edges = np.array([[0, 1], [1, 2], [2, 3], [2, 4]], dtype=np.int64)
    vertices = np.array([[7.5, 5.0], [12.5, 2.5], [12.5, 7.5], [1.0, 1.0], [4.0, 4.0]])
    return xy, edges, vertices


KNOWN_EDGES = [[0, 8], [8, 9], [9, 1], [1, 5], [5, 2], [2, 6], [6, 3], [2, 7], [7, 4]]
KNOWN_NODE_INDEX = [8, 9, 5, 6, 7]


def _known_offset():
    xy, edges, vertices = known()
    return xy, edges, vertices + [0.01, 0.0], 0.01, False


def _junction():
    xy, edges, vertices = known()
    return xy, edges, np.concatenate([vertices[:2], xy[2:3], vertices[2:], xy[:1]]), 0.0, True


def _twins():
    xy, edges, vertices = known()
    return xy, edges, np.concatenate([vertices, [[2.5, 2.5], [7.5, 5.0], [2.5, 2.5]]]), 0.0, True


def _reversed():
    xy = np.array([[8.0, 1.0], [0.0, 1.0], [8.0, 9.0]])
    edges = np.array([[0, 1], [2, 0]], dtype=np.int64)  # (right to left, top to bottom)
    return xy, edges, np.array([[1.0, 1.0], [8.0, 2.0], [6.0, 1.0], [8.0, 7.5], [3.0, 1.0]]), 0.0, True


def _long_row():
    rng = np.random.default_rng(30)
    x = rng.permutation(np.arange(1, 4096))[:2999].astype(np.float64)
    x = np.concatenate([x, x[1234:1235]])
    x = x[rng.permutation(3000)]
    xy = np.array([[0.0, 0.0], [4096.0, 0.0], [0.0, 8.0]])
    return xy, np.array([[2, 0], [0, 1]], dtype=np.int64), np.column_stack([x, np.zeros(3000)]), 0.0, True


def _chain2049():
    rng = np.random.default_rng(31)
    x = 2.0 * np.arange(2050)
    xy = np.column_stack([x, np.zeros(2050)])
    edges = np.column_stack([np.arange(2049), np.arange(1, 2050)]).astype(np.int64)
    vertices = np.column_stack([x[:-1] + 1.0, np.zeros(2049)])[rng.permutation(2049)]
    return xy, edges, vertices, 0.0, True


def _diagonal(length, step_x, step_y):
    """2000 short horizontal edges on rows y = step_y * j + 0.25 and, in the middle of the table, one edge (0, 0) - (length, length)
    that crosses every row of the vertex grid; the ``length`` vertices (k + 0.5, k + 0.5) lie on the long one.  The device bins the
    vertices in ``grid_rows`` rows of cells: an edge of more than 8 rows is walked by its whole wave, a row per lane, and beyond 64
    rows every lane walks more than one."""
    rng = np.random.default_rng(32)
    i, j = np.meshgrid(np.arange(50), np.arange(40), indexing="ij")
    left = np.column_stack([step_x * i.ravel(), step_y * j.ravel() + 0.25]).astype(np.float64)
    xy = np.concatenate([left, left + [1.0, 0.0], [[0.0, 0.0], [float(length), float(length)]]])
    short = np.column_stack([np.arange(2000), 2000 + np.arange(2000)])
    edges = np.concatenate([short[:1000], [[4000, 4001]], short[1000:]]).astype(np.int64)
    k = rng.permutation(length).astype(np.float64)
    return xy, edges, np.column_stack([k + 0.5, k + 0.5]), 0.0, True


def grid_rows(vertices):
    """(nx, ny) of the cell grid the device bins ``vertices`` in (size_grid of csrc/xr_sample.hip restated: about two vertices per
    cell of their bounding box)."""
    n = len(vertices)
    w, ht = np.ptp(vertices[:, 0]), np.ptp(vertices[:, 1])
    target = max(1.0, n / 2.0)
    cell = np.sqrt(max(w * ht, 0.0) / target)
    if not cell > 0.0:
        cell = max(max(w, ht) / target, 0.0)
    if not cell > 0.0 or not np.isfinite(cell):
        cell = 1.0
    nx, ny = min(int(w / cell) + 1, 1 << 15), min(int(ht / cell) + 1, 1 << 15)
    while nx * ny > 4 * n + 16:
        cell *= 1.5
        nx, ny = int(w / cell) + 1, int(ht / cell) + 1
    return nx, ny


def _two_edges():
    """Vertices within the tolerance of two parallel edges; edge 0 is the upper one.  The second vertex is nearer to edge 1."""
    xy = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 0.5], [4.0, 0.5]])
    edges = np.array([[2, 3], [0, 1]], dtype=np.int64)
    return xy, edges, np.array([[2.0, 0.25], [1.0, 0.125]]), 0.5, False


def _rows32_33():
    """Rows of 32 vertices, the longest a vertex ranks by counting, and of 33, the shortest a block sorts; each with a pair of
    equal vertices."""
    rng = np.random.default_rng(33)
    xy = np.array([[0.0, 0.0], [64.0, 0.0], [64.0, 64.0]])
    edges = np.array([[0, 1], [2, 1]], dtype=np.int64)
    x = rng.permutation(np.arange(1, 64))[:31].astype(np.float64)
    y = rng.permutation(np.arange(1, 64))[:32].astype(np.float64)
    vertices = np.concatenate([np.column_stack([np.append(x, x[7]), np.zeros(32)]), np.column_stack([np.full(33, 64.0), np.append(y, y[5])])])
    return xy, edges, vertices[rng.permutation(65)], 0.0, True


REFINE_CASES = {
    "known": lambda: known() + (0.0, True),
    "known_offset": _known_offset,
    "junction": _junction,
    "twins": _twins,
    "none": lambda: known()[:2] + (np.zeros((0, 2)), 0.0, True),
    "reversed": _reversed,
    "long_row": _long_row,
    "chain2049": _chain2049,
    "diagonal": lambda: _diagonal(300, 6.0, 7.5),  # 13 rows of cells: a row per lane
    "diagonal_wide": lambda: _diagonal(9000, 180.0, 225.0),  # 68 rows: lanes 0 .. 3 walk two rows each
    "two_edges": _two_edges,
    "rows32_33": _rows32_33,
}


# ---- merge cases: name -> [(xy, edges)] ------------------------------------------------------------------------------------------
def int_chain(n_node, spacing=1.0):
    x = spacing * np.arange(n_node)
    return np.column_stack([x, np.zeros(n_node)]), np.column_stack([np.arange(n_node - 1), np.arange(1, n_node)]).astype(np.int64)


def _overlapping(n_node, n_part=3, overlap=5):
    """A chain cut into overlapping parts; the later parts hold their edges reversed and in reversed order."""
    xy, edges = chain(n_node, seed=40)
    cuts = np.linspace(0, len(edges), n_part + 1).astype(int)
    parts = []
    for p in range(n_part):
        lo, hi = max(cuts[p] - (overlap if p else 0), 0), cuts[p + 1]
        sub_xy, sub_edges, _ = subset_ref(xy, edges, np.arange(lo, hi))
        if p:
            sub_edges = sub_edges[::-1, ::-1].copy()
        parts.append((sub_xy, sub_edges))
    return parts


def _coincident_inside():
    xy, edges = coincident()
    return [(xy, edges), (xy[[3, 4, 1]] + 0.0, np.array([[0, 2], [2, 1]], dtype=np.int64))]


def _zeros():
    a = (np.array([[0.0, 0.0], [1.0, -0.0], [2.0, 0.0]]), np.array([[0, 1], [1, 2]], dtype=np.int64))
    b = (np.array([[1.0, 0.0], [-0.0, -0.0], [3.0, 0.0]]), np.array([[1, 0], [0, 2]], dtype=np.int64))
    return [a, b]


def _nan_node():
    a = (np.array([[0.0, 0.0], [np.nan, 1.0], [1.0, 0.0]]), np.array([[0, 1], [0, 2]], dtype=np.int64))
    b = (np.array([[np.nan, 1.0], [0.0, 0.0], [1.0, 0.0]]), np.array([[1, 0], [1, 2]], dtype=np.int64))
    return [a, b]


MERGE_CASES = {
    "overlapping": lambda: _overlapping(60),
    "coincident_inside": _coincident_inside,
    "zeros": _zeros,
    "nan_node": _nan_node,
    "parts2049": lambda: _overlapping(3 * 2049 - 10, overlap=5),
}

# ---- subset cases the goldens pin: name -> (network, index) -------------------------------------------------------------------------
SUBSET_CASES = {
    "tree_permuted": lambda: random_network(40, 0.1, seed=7) + (np.random.default_rng(41).permutation(43)[:20],),
    "hub_every_other": lambda: hub(12, seed=9) + (np.arange(0, 24, 2),),
    "unused": lambda: unused_nodes() + (np.random.default_rng(42).permutation(329)[:100],),
}


def self_loops():
    """Loops at the first, a middle and the last edge; node 6 is used only by a loop."""
    xy = np.column_stack([np.arange(8.0), np.zeros(8)])
    edges = np.array([[0, 0], [0, 1], [1, 2], [6, 6], [2, 3], [3, 4], [4, 5], [5, 7], [7, 7]], dtype=np.int64)
    return xy, edges


# ---- comparing with the goldens ---------------------------------------------------------------------------------------------------
DIGEST_FROM = 300  # rows: a larger array is stored as shape, dtype and SHA-256


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64 if np.asarray(a).dtype.kind == "f" else np.int64)
    return {"shape": list(a.shape), "dtype": a.dtype.name, "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def equals_known(a, known_value):
    """``a`` against a golden entry: a nested list (NaN equals NaN) or a digest."""
    if isinstance(known_value, dict):
        return digest(a) == known_value
    a = np.asarray(a)
    expected = np.asarray(known_value, dtype=np.float64 if a.dtype.kind == "f" else np.int64).reshape(a.shape if a.size == 0 else np.shape(known_value))
    return a.shape == expected.shape and np.array_equal(a, expected, equal_nan=a.dtype.kind == "f")
