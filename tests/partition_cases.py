"""
Yardsticks and cases of the merge tests (tests/test_partition_cpu.py, tests/test_gpu_partition.py): numpy restatements of
``merge_partitions`` (nodes, faces, derived edges), ``labels_to_indices`` and ``index_like``, written from the rule (DESIGN
section 15) with ``np.unique(axis=0, return_index=True, return_inverse=True)``, a row sort and ``np.searchsorted``, and pinned to
what the reference's own functions return in tests/golden/partition_known.json; the partitions the tests run on.
"""
import json
import os

import numpy as np

import subset_cases as sc
from xugrid_amd import connectivity, meshgen

HERE = os.path.dirname(os.path.abspath(__file__))


def known():
    with open(os.path.join(HERE, "golden", "partition_known.json")) as f:
        return json.load(f)


# ---- restatements ---------------------------------------------------------------------------------------------------------
def _split(first, slices):
    """Ascending kept ids of a concatenation -> per segment, local."""
    cuts = np.searchsorted(first, slices[1:-1])
    return [(part - off).astype(np.int64) for part, off in zip(np.split(first, cuts), slices)]


def merge_nodes(parts):
    """-> (xy_merged, node_indexes, node_inverse): rows equal as doubles are one node (np.unique(axis=0): -0.0 == 0.0, a NaN row
    equals nothing), the first occurrence is kept and kept nodes keep the concatenation order."""
    xy_all = np.concatenate([np.asarray(xy, dtype=np.float64).reshape(-1, 2) for xy, _ in parts])
    slices = np.cumsum([0] + [len(xy) for xy, _ in parts])
    _, first, inverse = np.unique(xy_all, axis=0, return_index=True, return_inverse=True)
    kept = np.sort(first)
    node_inverse = np.searchsorted(kept, first[inverse.ravel()]).astype(np.int64)
    return xy_all[kept], _split(kept, slices), node_inverse


def widened_faces(parts, node_inverse):
    m = max([f.shape[1] for _, f in parts] + [1])
    offsets = np.cumsum([0] + [len(xy) for xy, _ in parts])
    rows = []
    for (xy, faces), off in zip(parts, offsets):
        wide = np.full((len(faces), m), -1, dtype=np.int64)
        valid = faces != -1
        wide[:, : faces.shape[1]][valid] = node_inverse[faces[valid] + off]
        rows.append(wide)
    return np.concatenate(rows).reshape(-1, m)


def merge_rows(rows, slices):
    """First occurrence of every row up to the order inside the row -> (kept ids ascending, per-segment local ids)."""
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64), _split(np.zeros(0, dtype=np.int64), slices)
    _, first = np.unique(np.sort(rows, axis=1), axis=0, return_index=True)
    kept = np.sort(first)
    return kept, _split(kept, slices)


def host_edges(faces):
    if len(faces) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return connectivity.edge_connectivity(np.asarray(faces, dtype=np.intp))[0].astype(np.int64)


def merge(parts):
    """The whole yardstick -> dict(xy, faces, node_indexes, node_inverse, face_indexes, edge_indexes, edge_positions, edges)."""
    parts = [(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(f, dtype=np.int64)) for xy, f in parts]
    xy, node_indexes, node_inverse = merge_nodes(parts)
    rows = widened_faces(parts, node_inverse)
    kept, face_indexes = merge_rows(rows, np.cumsum([0] + [len(f) for _, f in parts]))
    faces = rows[kept]
    # edges: every grid derives its own, numbered lexicographically by (lower, higher) node
    offsets = np.cumsum([0] + [len(p[0]) for p in parts])
    tables = [host_edges(f) for _, f in parts]
    edge_rows = np.sort(np.concatenate([node_inverse[t + off] for t, off in zip(tables, offsets)]).reshape(-1, 2), axis=1)
    edge_slices = np.cumsum([0] + [len(t) for t in tables])
    edge_kept, edge_indexes = merge_rows(edge_rows, edge_slices)
    edges = host_edges(faces)
    width = max(len(xy), 1)
    position = np.searchsorted(edges[:, 0] * width + edges[:, 1], edge_rows[edge_kept, 0] * width + edge_rows[edge_kept, 1])
    assert np.array_equal(edges[position], edge_rows[edge_kept])  # every kept edge is an edge of the merged grid
    cuts = np.searchsorted(edge_kept, edge_slices[1:-1])
    return dict(xy=xy, faces=faces, node_indexes=node_indexes, node_inverse=node_inverse, face_indexes=face_indexes,
                edge_indexes=edge_indexes, edge_positions=[p.astype(np.int64) for p in np.split(position, cuts)], edges=edges,
                edge_slices=edge_slices)


def merge_data(expected, data, facet):
    """The merged (K, n) float64 data: kept values concatenated (nodes, faces) or scattered to their edge (edges)."""
    data = [np.asarray(d, dtype=np.float64) for d in data]
    if facet != "edge":
        return np.concatenate([d[..., i] for d, i in zip(data, expected[f"{facet}_indexes"])], axis=-1)
    out = np.full(data[0].shape[:-1] + (len(expected["edges"]),), np.nan)
    for d, i, pos in zip(data, expected["edge_indexes"], expected["edge_positions"]):
        out[..., pos] = d[..., i]
    return out


def labels_to_indices(labels):
    labels = np.asarray(labels)
    return [np.nonzero(labels == l)[0].astype(np.int64) for l in range(int(labels.max()) + 1 if labels.size else 0)]


def like_keys(xy, tolerance):
    xy = np.asarray(xy, dtype=np.float64)
    return xy + 0.0 if tolerance == 0.0 else np.rint(xy / tolerance) + 0.0


def index_like(xy_a, xy_b, tolerance):
    """index[i] = the row of a whose key is the key of row i of b; unique keys and equal key sets are required."""
    xy_a, xy_b = np.asarray(xy_a, dtype=np.float64), np.asarray(xy_b, dtype=np.float64)
    if xy_a.shape != xy_b.shape:
        raise ValueError("coordinates do not match in shape")
    ka, kb = like_keys(xy_a, tolerance), like_keys(xy_b, tolerance)
    ua, first_a = np.unique(ka, axis=0, return_index=True)
    ub = np.unique(kb, axis=0)
    if len(ua) != len(ka) or len(ub) != len(kb) or not np.array_equal(ua, ub):
        raise ValueError("coordinates are not identical after sorting")
    # rows of the sorted unique keys: position of every key of b among them (lexicographic: x first, then y)
    order_b = np.lexsort((kb[:, 1], kb[:, 0]))
    index = np.empty(len(kb), dtype=np.int64)
    index[order_b] = first_a
    if not (np.abs(xy_a[index] - xy_b) <= tolerance).all():
        raise ValueError("coordinates are not identical after sorting")
    return index


def like_inside_deviation(xy_a, xy_b, tolerance):
    """Unique keys on both sides and equal key sets: where the key pairing and the reference's sorted pairing agree."""
    ka, kb = like_keys(xy_a, tolerance), like_keys(xy_b, tolerance)
    ua, ub = np.unique(ka, axis=0), np.unique(kb, axis=0)
    return len(ua) == len(ka) and len(ub) == len(kb) and np.array_equal(ua, ub)


# ---- partitions: name -> list of (node_xy, faces) ------------------------------------------------------------------------------
def cut(xy, faces, ids):
    xy_sub, faces_sub, _, _ = sc.topology_subset(xy, faces, np.asarray(ids, dtype=np.int64))
    return xy_sub, faces_sub


def quads(nx, ny):
    return meshgen.quad_mesh(np.arange(nx + 1.0), np.arange(ny + 1.0))


def halo_blocks(xy, faces, n_block):
    """Contiguous blocks of face ids, each with the faces that touch one of its nodes."""
    n = len(faces)
    labels = np.minimum(np.arange(n) * n_block // n, n_block - 1)
    out = []
    for l in range(n_block):
        own = np.nonzero(labels == l)[0]
        nodes = np.unique(faces[own])
        out.append(sc.faces_of_nodes(faces, nodes[nodes != -1]))
    return out


def anchor():
    xy, faces = quads(3, 2)
    return [cut(xy, faces, [0, 1, 2, 3]), cut(xy, faces, [5, 4, 3, 2])]


def mixed36_halo3():
    xy, faces = sc.mesh("mixed36")
    blocks = halo_blocks(xy, faces, 3)
    return [cut(xy, faces, blocks[k]) for k in (2, 0, 1)]


def tri3_quad4():
    """The triangles of the mixed mesh in a 3-wide table, then every face whose id is odd in the 4-wide one."""
    xy, faces = sc.mesh("mixed36")
    tri_xy, tri_faces = cut(xy, faces, np.nonzero((faces == -1).any(axis=1))[0])
    return [(tri_xy, np.ascontiguousarray(tri_faces[:, :3])), cut(xy, faces, np.arange(1, len(faces), 2))]


def rotated_reversed():
    """Face 1 of the first grid comes again rotated, reversed and (a triangle) with its fill in the table; only the first stays."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [2.0, 0.5]])
    first = np.array([[0, 1, 2, 3], [1, 4, 2, -1]])
    second = np.array([[2, 3, 0, 1], [3, 2, 1, 0], [2, 1, 4, -1], [4, 2, 1, -1]])
    return [(xy, first), (xy[::-1].copy(), np.where(second == -1, -1, 4 - second))]


def disjoint():
    xy, faces = quads(3, 2)
    return [(xy, faces), (xy + np.array([10.0, 0.0]), faces[::-1].copy())]


def all_duplicate():
    xy, faces = sc.mesh("mixed36")
    return [cut(xy, faces, np.arange(len(faces))[::-1]), cut(xy, faces, [7, 3, 11]), cut(xy, faces, [0, 1])]


def with_empty():
    xy, faces = quads(3, 2)
    empty = (np.zeros((0, 2)), np.zeros((0, 4), dtype=np.int64))
    return [cut(xy, faces, [0, 1, 2]), empty, cut(xy, faces, [2, 3, 4, 5])]


def signed_zero():
    """The seam of two quads lies on x = 0, written 0.0 on one side and -0.0 on the other; y = -0.0 on one node too."""
    left = np.array([[-1.0, -0.0], [0.0, 0.0], [0.0, 1.0], [-1.0, 1.0]])
    right = np.array([[-0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [-0.0, 1.0]])
    face = np.array([[0, 1, 2, 3]])
    return [(left, face), (right, face)]


def nan_nodes():
    """Both grids hold a node with a NaN coordinate "at the same place": it equals nothing, so it stays two nodes."""
    a = np.array([[0.0, 0.0], [1.0, 0.0], [np.nan, 1.0], [0.0, 1.0]])
    b = np.array([[1.0, 0.0], [2.0, 0.0], [2.0, 1.0], [np.nan, 1.0]])
    face = np.array([[0, 1, 2, 3]])
    return [(a, face), (b, face)]


def mixed2049_halo4():
    xy, faces = sc.mesh("mixed2049")
    return [cut(xy, faces, ids) for ids in halo_blocks(xy, faces, 4)]


PARTITIONS = {
    "anchor": anchor,
    "mixed36_halo3": mixed36_halo3,
    "tri3_quad4": tri3_quad4,
    "rotated_reversed": rotated_reversed,
    "disjoint": disjoint,
    "all_duplicate": all_duplicate,
    "with_empty": with_empty,
    "signed_zero": signed_zero,
    "nan_nodes": nan_nodes,
    "mixed2049_halo4": mixed2049_halo4,
}
SLACK_CASES = ("anchor", "mixed36_halo3", "mixed2049_halo4")
GOLDEN_CASES = tuple(n for n in PARTITIONS if n != "mixed2049_halo4")  # (recorded from the reference; the large one is not)
_MADE, _EXPECTED = {}, {}


def partitions(name):
    if name not in _MADE:
        _MADE[name] = [(np.ascontiguousarray(xy, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64))
                       for xy, f in PARTITIONS[name]()]
    return _MADE[name]


def expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = merge(partitions(name))
    return _EXPECTED[name]


# ---- index_like cases: name -> (xy_a, xy_b, tolerance) -----------------------------------------------------------------------
def like_cases():
    xy, faces = sc.mesh("mixed36")
    rng = np.random.default_rng(17)
    tolerance = 2.0 ** -10
    lattice = np.rint(xy / (64 * tolerance)) * (64 * tolerance)  # multiples of the tolerance, far apart
    order = rng.permutation(len(xy))
    jitter = (rng.random(xy.shape) - 0.5) * (tolerance / 2)      # |jitter| <= tolerance / 4
    return {
        "known_exact": (np.array([[3.0, 3.0], [1.0, 1.0], [2.0, 2.0], [0.0, 0.0]]),
                        np.array([[0.0, 0.0], [1.0, 1.0], [3.0, 3.0], [2.0, 2.0]]), 0.0),
        "known_tolerance": (np.array([[3.0, 3.0001], [1.0, 1.0], [2.0, 2.0], [-0.0001, 0.0]]),
                            np.array([[0.0, 0.0], [1.0, 1.0], [3.0, 3.0], [2.0, 2.0]]), 0.001),
        "permuted": (xy, xy[order], 0.0),
        "jitter": (lattice + jitter, lattice[order], tolerance),
    }


# ---- assertions shared by tests/test_gpu_partition.py and tests/partition_worker_gpu.py ---------------------------------------
def to_numpy(a):
    return sc.to_numpy(a)


def same_bits(a, b):
    """Equal bit for bit: NaN equals NaN, -0.0 does not equal 0.0."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def assert_merged(merged, e):
    assert merged.n_node == len(e["xy"]) and merged.n_face == len(e["faces"])
    assert merged.n_max_node_per_face == e["faces"].shape[1]
    assert np.array_equal(merged.face_node_connectivity, e["faces"])
    assert same_bits(merged.node_coordinates, e["xy"])


def assert_index_lists(grid, indexes, e, kind_of=None):
    assert set(indexes) == {grid.node_dimension, grid.edge_dimension, grid.face_dimension}
    for dim, key in ((grid.node_dimension, "node_indexes"), (grid.edge_dimension, "edge_indexes"), (grid.face_dimension, "face_indexes")):
        got = indexes[dim]
        assert len(got) == len(e[key]), dim
        for g, want in zip(got, e[key]):
            if kind_of is not None:
                assert isinstance(g, kind_of), (dim, type(g))
            g = to_numpy(g)
            assert g.dtype == np.int64 and np.array_equal(g, want), (dim, g, want)

