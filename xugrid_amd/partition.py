"""
The join half of the partition workflow (xugrid/ugrid/partitioning.py:16-148, ``Ugrid2d.merge_partitions`` ugrid2d.py,
``Ugrid2d.reindex_like`` :1574-1617, ``connectivity.index_like`` connectivity.py:38-61) on arrays.  Kernels in
``csrc/xr_merge.hip``; DESIGN section 15.

``merge_partitions`` joins grids into one: nodes that compare equal as doubles become one node (first occurrence kept, bit for
bit), faces with the same node set become one face (first occurrence kept, slot order as given); the merged grid derives its
own edges.  ``labels_to_indices`` / ``partition_by_label`` cut a grid by integer face labels; ``reindex_like`` /
``index_like_device`` match two grids' coordinates.  ``label_partitions`` makes such labels: ``n_part`` balanced parts of a graph
by the deterministic rule of include/xugrid_amd.h (xr_graph_partition_dev; kernels in ``csrc/xr_partlabel.hip``, DESIGN section
22) where the reference asks METIS.  "Which rows are equal and which came first" is answered by a key table
in HBM, never by a sort; the table always runs on the device.

Kinds of result, as ``subset``: host grids give a host ``Ugrid2d`` and numpy int64 indexes; any device-resident grid in the list
gives a ``DeviceUgrid2d`` and ``DeviceArray`` indexes; torch data or labels give torch results.  The edge arithmetic runs on
the device when every grid in the list is device-resident with a manifold topology, in numpy otherwise.
"""
import operator

import numpy as np

from . import engine, netedit, subset
from .inkind import (Index, concat_last_axis, data_facet, device_topologies, first_torch, host_edge_node, int64_dev, result_kind,
                     xy_dev)
from .ugrid1d import Ugrid1d

FACETS = ("node", "edge", "face")
ZERO = "Cannot merge partitions: zero partitions provided."
NOT_IDENTICAL = "coordinates are not identical after sorting"


# ---- labels ---------------------------------------------------------------------------------------------------------------
def labels_to_indices(labels):
    """partitioning.py:16-27: ``[0, 1, 0, 2, 2] -> [[0, 2], [1], [3, 4]]`` -- ``max + 1`` ascending int64 index arrays, an
    empty one for a label that does not occur.  numpy labels give numpy arrays, device labels device arrays of their kind."""
    dev, like, n = int64_dev(labels, "labels")
    ids = _label_indices(dev, like, n)
    return ids if like is not None else [Index(dev=i).numpy() for i in ids]


def _label_indices(dev, like, n):
    """-> per label ``0 .. max`` the ascending ids that carry it: int64 device arrays of the kind of ``like``."""
    ptr = engine.device_array_info(dev)[0]
    lo, hi = engine.labels_range(ptr, n)
    if lo < 0:
        raise ValueError("labels must be non-negative")
    return engine.labels_order(ptr, n, hi + 1, like)


def partition_by_label(grid, labels, data=None):
    """partitioning.py:71-76 on arrays: one ``topology_subset(index, return_index=True)`` result ``(grid, indexes)`` per label
    ``0 .. max``; with ``data`` ``(..., n)`` on one facet each entry is ``(grid, indexes, data[..., indexes[facet]])``."""
    dev, like, n = int64_dev(labels, "labels", grid.n_face)
    facet = data_facet(grid, data) if data is not None else None
    out = []
    for ids in _label_indices(dev, like, n):
        entry = subset.topology_subset(grid, Index(dev=ids, like=like), return_index=True)
        if data is not None:
            by = Index.wrap(entry[1][getattr(grid, f"{facet}_dimension")])
            entry += (by.gather(data, getattr(grid, f"n_{facet}")),)
        out.append(entry)
    return out


# ---- making labels -------------------------------------------------------------------------------------------------------------
PART_MAX_ROUNDS = 16  # PL_MAX_ROUNDS, csrc/xr_partlabel.hip: refinement rounds at most
PART_EPS = (3, 100)  # PL_EPS_NUM / PL_EPS_DEN: a part may weigh 1.03 sum(weights) / n_part
DEVICE_WEIGHT_LIMIT = 2**31 - 1  # what ``engine.labels_range`` clamps to: a device weight must stay below it
last_info = None  # {"rounds", "moves", "cut_seed", "cut"} of the last labelling (tests and profiles read it; None: nothing ran)


def check_n_part(n_part, n):
    n_part = operator.index(n_part)
    if n_part < 1:
        raise ValueError(f"n_part must be at least 1, received: {n_part}")
    if n > 0 and n_part > n:
        raise ValueError(f"n_part must be at most the number of elements ({n}), received: {n_part}")
    return n_part


def check_weights(weights, n, n_part):
    """ugridbase.py:1508-1526 with its three messages, and ``100 * n_part * sum(weights)`` within int64 -> the weights as
    ``int64_dev`` gives them, or ``(None, None, n)`` for none.  Host weights are checked without a device; device weights
    through ``engine.labels_range`` (their sum is checked by the library)."""
    total = n
    if weights is not None:
        info = None if isinstance(weights, (list, tuple)) else engine.device_array_info(weights)
        a = np.asarray(weights) if info is None else None
        shape, dtype = (a.shape, a.dtype) if info is None else info[1:]
        if tuple(shape) != (n,):
            raise ValueError(f"Wrong shape on weights. Expected a 1D array with {n} elements, received array with shape: {tuple(shape)}")
        if not np.issubdtype(dtype, np.integer):
            raise TypeError(f"Wrong type on weights. Expected an integer array, received: {dtype}")
        if info is None:
            if np.any(a < 0):
                raise ValueError("Wrong values on weights. Weights should be greater or equal to zero.")
            if 100.0 * n_part * float(np.sum(a, dtype=np.float64)) >= 2.0**63:  # (the exact sum below cannot wrap behind this)
                raise ValueError(f"100 * n_part * sum(weights) does not fit in int64 (n_part {n_part})")
            total = int(np.sum(a, dtype=np.int64)) or n  # (all zero: all ones)
    if 100 * n_part * total > np.iinfo(np.int64).max:
        raise ValueError(f"100 * n_part * sum(weights) does not fit in int64 (n_part {n_part}, sum {total})")
    if weights is None or n == 0:
        return None, (weights if weights is not None and info is not None else None), n
    dev, like, _ = int64_dev(weights, "weights", n)
    if like is not None:
        lo, hi = engine.labels_range(engine.device_array_info(dev)[0], n)
        if lo < 0:
            raise ValueError("Wrong values on weights. Weights should be greater or equal to zero.")
        if hi >= DEVICE_WEIGHT_LIMIT:
            raise ValueError(f"Wrong values on weights. Weights in device memory should be smaller than {DEVICE_WEIGHT_LIMIT}.")
    return dev, like, n


def graph_labels(n, make_graph, coordinates, n_part, weights=None, device_out=False):
    """The labels of ``label_partitions`` for the ``n`` vertices of ``make_graph()`` (a ``fill.DeviceGraph``) at
    ``coordinates()`` ``(n, 2)`` (host or device float64); everything is validated before either is made.  Kinds: device
    ``weights`` give labels of their kind, else ``device_out`` a ``DeviceArray``, else int64 numpy."""
    global last_info
    n_part = check_n_part(n_part, n)
    w, like, _ = check_weights(weights, n, n_part)
    to_numpy = like is None and not device_out
    labels, ptr = (np.empty(n, dtype=np.int64), None) if to_numpy and n == 0 else engine.empty_like_device(like, (n,), np.int64)
    if n == 0:
        return labels
    keep, xy_ptr, shape = xy_dev(coordinates(), "coordinates")
    if tuple(shape) != (n, 2):
        raise ValueError(f"expected coordinates of shape ({n}, 2), received: {tuple(shape)}")
    graph = make_graph()  # (held until the call is back: the handle dies with its owner)
    info = engine.graph_partition_dev(graph._h, xy_ptr, engine.device_array_info(w)[0] if w is not None else None, n_part, ptr)
    last_info = dict(zip(("rounds", "moves", "cut_seed", "cut"), info))
    return Index(dev=labels).emit(like, to_numpy)


def canonical_graph(connectivity):
    """The ``DeviceGraph`` of a scipy matrix with repeated entries summed and ascending columns."""
    from .fill import DeviceGraph

    csr = connectivity.tocsr().copy()  # (the caller's matrix keeps its repeated entries)
    csr.sum_duplicates()
    csr.sort_indices()
    return DeviceGraph(csr)


def label_partitions(connectivity, coordinates, n_part, weights=None):
    """``n_part`` balanced parts of the symmetric scipy CSR ``connectivity`` ``(n, n)`` whose vertices lie at ``coordinates``
    ``(n, 2)``: int64 labels ``(n,)`` by the rule of xr_graph_partition_dev -- a Hilbert-curve split of the integer
    ``weights`` (default: all ones), then rounds of cut-lowering moves within a 3 % imbalance.  Repeated entries are summed
    and indices sorted first; the diagonal is ignored.  numpy in -> numpy out, device weights in -> labels of their kind."""
    from .fill import _check_square

    n = _check_square(connectivity)
    return graph_labels(n, lambda: canonical_graph(connectivity), lambda: coordinates, n_part, weights)


# ---- merge ----------------------------------------------------------------------------------------------------------------
def _edges_numpy(grids, merged, merge):
    """The kept edges and their ids in the merged grid over the host tables (partitioning.py:137-148 on derived edges)."""
    inverse = merge.node_inverse().download()
    offsets = np.cumsum([0] + [g.n_node for g in grids])
    tables = [host_edge_node(g) for g in grids]
    slices = np.cumsum([0] + [len(t) for t in tables])
    rows = np.sort(np.concatenate([inverse[t + off] for t, off in zip(tables, offsets)]).reshape(-1, 2), axis=1)
    n_merged = max(merged.n_node, 1)
    keys = rows[:, 0] * n_merged + rows[:, 1]
    _, first = np.unique(keys, return_index=True)
    first.sort()
    merged_edges = host_edge_node(merged)
    position = np.searchsorted(merged_edges[:, 0] * n_merged + merged_edges[:, 1], keys[first])
    cuts = np.searchsorted(first, slices[1:-1])
    return ([Index(host=(part - off).astype(np.int64)) for part, off in zip(np.split(first, cuts), slices)],
            [Index(host=p.astype(np.int64)) for p in np.split(position, cuts)], slices)


def merge_partitions(grids, return_index=False, data=None, dim=None):
    """See ``Ugrid2d.merge_partitions``; a list of ``Ugrid1d`` goes to ``netedit.merge_partitions``, a mixed one raises
    ``TypeError`` (partitioning.py:151-158)."""
    grids = list(grids)
    if any(isinstance(g, Ugrid1d) for g in grids):
        return netedit.merge_partitions(grids, return_index, data, dim)
    if len(grids) == 0:
        raise ValueError(ZERO)
    if data is not None:
        data = list(data)
    facet = data_facet(grids, data, dim) if data is not None else None
    host = grids[0]
    lead = next((g for g in grids if g._device_resident), host)
    like, to_numpy = result_kind(grids, first_torch(data) if data is not None else None)
    parts = range(len(grids))

    if len(grids) == 1:  # (partitioning.py: one partition is the grid itself)
        merged, merge = host, None
    else:
        merge = engine.DeviceMerge([g.device_mesh for g in grids])
        merged = lead._grid_from_mesh(merge.take_mesh())
        merged.name = host.name
    out = [merged]
    need = set(FACETS) if return_index else ({facet} if facet else set())
    indexes, positions, edge_slices = {}, None, None
    if merge is None:
        indexes = {f: [Index.arange(getattr(host, f"n_{f}"))] for f in need}
        positions = indexes.get("edge")
        edge_slices = np.array([0, host.n_edge]) if "edge" in need else None
    else:
        for f in need - {"edge"}:
            indexes[f] = [Index(dev=merge.index(f, p, like)) for p in parts]
        if "edge" in need:
            topologies = device_topologies(grids, merged)
            if topologies is not None:
                merge.add_edges(topologies[:-1], topologies[-1])
                indexes["edge"] = [Index(dev=merge.index("edge", p, like)) for p in parts]
                positions = [Index(dev=merge.index("edge", p, like, position=True)) for p in parts]
                edge_slices = np.cumsum([0] + [t.n_edge for t in topologies[:-1]])
            else:
                indexes["edge"], positions, edge_slices = _edges_numpy(grids, merged, merge)
    if return_index:
        out.append({getattr(host, f"{f}_dimension"): [i.emit(like, to_numpy) for i in indexes[f]] for f in FACETS})
    if data is not None:
        sizes = [getattr(g, f"n_{facet}") for g in grids]
        cat, total = concat_last_axis(data, sizes)
        if facet == "edge":
            source = np.full(merged.n_edge, -1, dtype=np.int64)
            for p, (idx, pos) in enumerate(zip(indexes["edge"], positions)):
                source[pos.numpy()] = idx.numpy() + edge_slices[p]
            source = Index(host=source)
        elif merge is None:
            source = indexes[facet][0]
        else:
            source = Index(dev=merge.index(facet, -1, like))
        out.append(source.gather(cat, total))
    return out[0] if len(out) == 1 else tuple(out)


# ---- matching coordinates ---------------------------------------------------------------------------------------------------
def index_like_device(xy_a, xy_b, tolerance=0.0):
    """connectivity.py:38-61 through the key table: ``index[i]`` is the row of ``xy_a`` that equals row ``i`` of ``xy_b``, so
    ``xy_a[index]`` is ``xy_b``.  The key is the coordinate pair, or ``rint(xy / tolerance)`` for a non-zero tolerance; after
    matching every pair must lie within the tolerance on both axes.  Keys that repeat inside either input, and rows without a
    partner, raise ``ValueError("coordinates are not identical after sorting")`` (the reference pairs by sorted position and
    accepts some of those: DESIGN section 7).  numpy in -> numpy out; a device array in -> an int64 device array."""
    keep_a, ptr_a, shape_a = xy_dev(xy_a, "coordinates")
    keep_b, ptr_b, shape_b = xy_dev(xy_b, "coordinates")
    if shape_a != shape_b:
        raise ValueError("coordinates do not match in shape")
    if len(shape_a) != 2 or shape_a[1] != 2:
        raise ValueError(f"expected (n, 2) coordinates, received shape {shape_a}")
    like = first_torch([xy_a, xy_b])
    index, repeats, misses = engine.index_like_dev(ptr_a, ptr_b, shape_a[0], abs(float(tolerance)), like)
    if repeats or misses:
        raise ValueError(NOT_IDENTICAL)
    host = engine.device_array_info(xy_a) is None and engine.device_array_info(xy_b) is None
    return Index(dev=index).numpy() if host else index


def _facet_coordinates(grid, facet):
    if facet == "node":
        return grid.node_coordinates
    if facet == "edge":
        return grid._edge_points()
    return grid.centroids


def reindex_like(grid, other, data, dim=None, tolerance=0.0):
    """See ``Ugrid2d.reindex_like`` / ``Ugrid1d.reindex_like``."""
    if isinstance(grid, Ugrid1d):
        return netedit.reindex_like(grid, other, data, dim, tolerance)
    facet = data_facet(grid, data, dim)
    index = Index.wrap(index_like_device(_facet_coordinates(grid, facet), _facet_coordinates(other, facet), tolerance))
    return index.gather(data, getattr(grid, f"n_{facet}"))
