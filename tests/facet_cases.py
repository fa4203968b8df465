"""Shared cases and numpy yardsticks of the facet-mapping tests (test_facet_cpu.py, test_gpu_facet.py): the numpy restatement of
the reference's ``_to_facet`` (xugrid/core/dataarray_accessor.py:300-344: ``obj.isel(indexer).where(indexer != -1)``) and of the
reduction that follows it, the host route's six dense tables, and the small meshes.  Not a test file."""
import warnings

import numpy as np

from xugrid_amd import connectivity

EPS = np.finfo(np.float64).eps
REDUCERS = ("mean", "sum", "min", "max")
DIRECTIONS = (("node", "face"), ("node", "edge"), ("edge", "node"), ("edge", "face"), ("face", "node"), ("face", "edge"))


# ---- the restatement
def raw(table, data):
    """``data (..., n_source)``, dense ``table (n_target, w)`` with -1 -> ``(..., n_target, w)``, NaN where the table is -1."""
    table = np.asarray(table)
    data = np.asarray(data, dtype=np.float64)
    return np.where(table >= 0, data[..., np.maximum(table, 0)], np.nan)


def reduce_sequential(table, data, how):
    """The specified order: a loop over the table's columns with np.add / np.fmin / np.fmax on whole columns, NaN
    contributors passed over; mean = that sum divided once by the count.  No contributor: NaN, 0.0 for the sum."""
    table = np.asarray(table)
    data = np.asarray(data, dtype=np.float64)
    shape = data.shape[:-1] + (table.shape[0],)
    summing = how in ("mean", "sum")
    acc = np.zeros(shape) if summing else np.full(shape, np.nan)
    count = np.zeros(shape)
    with np.errstate(invalid="ignore"):  # (inf + -inf in a row is NaN, on purpose)
        for j in range(table.shape[1]):
            x = np.where(table[:, j] >= 0, data[..., np.maximum(table[:, j], 0)], np.nan)
            valid = ~np.isnan(x)
            if summing:
                acc = np.where(valid, np.add(acc, x), acc)
                count += valid
            elif how == "min":
                acc = np.fmin(acc, x)
            elif how == "max":
                acc = np.fmax(acc, x)
            else:
                raise ValueError(how)
        if how == "mean":
            acc = np.where(count > 0, acc / np.maximum(count, 1), np.nan)
    return acc


def reduce_numpy(table, data, how):
    """What the reference's ``.mean("nmax")`` and its kin compute: numpy's nan-reducers over the raw form."""
    r = raw(table, data)
    if r.shape[-1] == 0:
        return np.zeros(r.shape[:-1]) if how == "sum" else np.full(r.shape[:-1], np.nan)
    fn = {"mean": np.nanmean, "sum": np.nansum, "min": np.nanmin, "max": np.nanmax}[how]
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)  # (all-NaN rows)
        return fn(r, axis=-1)


def reorder_bound(table, data, how):
    """Worst case of reordering a row's sum: ``(w_row - 1) * eps * sum(|valid contributors|)``, divided by their number for
    the mean (each order is within ``(w_row - 1) * eps / 2 * sum|x|`` of the exact sum).  ``w_row``: the row's entries.
    -> (bound, rows that hold an infinity: compared for equality instead)."""
    r = raw(table, data)
    w_row = (np.asarray(table) >= 0).sum(axis=1)
    with np.errstate(invalid="ignore"):
        total = np.nansum(np.abs(r), axis=-1)
        has_inf = np.isinf(r).any(axis=-1)
        bound = np.maximum(w_row - 1, 0) * EPS * np.where(has_inf, 0.0, total)
    if how == "mean":
        bound = bound / np.maximum((~np.isnan(r)).sum(axis=-1), 1)
    return bound, has_inf


def dense(csr, width=None):
    """scipy CSR -> the dense table with -1 fill, entries in column order, ``width`` columns (default: the widest row)."""
    counts = np.diff(csr.indptr)
    w = int(counts.max()) if counts.size else 0
    width = w if width is None else width
    assert width >= w
    out = np.full((csr.shape[0], width), -1, dtype=np.int64)
    rows = np.repeat(np.arange(csr.shape[0]), counts)
    cols = np.arange(csr.indices.size) - np.repeat(csr.indptr[:-1], counts)
    out[rows, cols] = csr.indices
    return out


def host_tables(faces, n_node):
    """The host route's six tables in dense form: (target, source) -> int64 ``(n_target, w)``."""
    faces = np.asarray(faces, dtype=np.int64)
    edge_node, face_edge = connectivity.edge_connectivity(faces)
    return {
        ("face", "node"): faces,
        ("face", "edge"): face_edge,
        ("edge", "node"): edge_node,
        ("edge", "face"): connectivity.invert_dense(face_edge),
        ("node", "face"): dense(connectivity.invert_dense_to_sparse(faces, n_rows=n_node)),
        ("node", "edge"): dense(connectivity.invert_dense_to_sparse(edge_node, n_rows=n_node)),
    }


def network_tables(edge_node, n_node):
    edge_node = np.asarray(edge_node, dtype=np.int64)
    return {
        ("edge", "node"): edge_node,
        ("node", "edge"): dense(connectivity.invert_dense_to_sparse(edge_node, n_rows=n_node)),
    }


def sizes(tables):
    """facet -> its size, from the tables."""
    return {"node": len(tables[("node", "edge")]), "edge": len(tables[("edge", "node")]),
            **({"face": len(tables[("face", "node")])} if ("face", "node") in tables else {})}


# ---- data
def field(n, K=3, seed=0, dtype=np.float64):
    """``(K, n)`` seeded values of mixed sign and magnitude, about 10 % NaN; the last slice also holds +-inf and +-0.0."""
    rng = np.random.default_rng(seed + 31 * n)
    a = rng.standard_normal((K, n)) * 10.0 ** rng.integers(-3, 4, size=(K, n))
    a[rng.random((K, n)) < 0.1] = np.nan
    if n >= 4:
        special = rng.permutation(n)[: min(n, 8)]
        a[-1, special] = np.resize([np.inf, -np.inf, 0.0, -0.0], special.size)
    return a.astype(dtype)


# ---- meshes
def two_triangles():
    """The hand-checked mesh: nodes 0..3, faces [[0,1,2],[1,3,2]]; edges (0,1),(0,2),(1,2),(1,3),(2,3)."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    return xy, np.array([[0, 1, 2], [1, 3, 2]])


def three_on_one_edge():
    """Three triangles sharing the edge (0, 1): non-manifold, the device topology keeps nothing."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0], [0.5, -1.0], [1.5, 1.0]])
    return xy, np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4]])


def y_network():
    """A Y of 10 edges: three arms of 3, 3 and 4 edges meeting in node 0 -> (node_xy, edge_node)."""
    edges, xy, nxt = [], [[0.0, 0.0]], 1
    for arm, (dx, dy, length) in enumerate([(1.0, 1.0, 3), (-1.0, 1.0, 3), (0.0, -1.0, 4)]):
        prev = 0
        for step in range(1, length + 1):
            xy.append([dx * step, dy * step])
            edges.append([prev, nxt] if (arm + step) % 2 else [nxt, prev])  # (either direction)
            prev, nxt = nxt, nxt + 1
    return np.array(xy), np.array(edges)
