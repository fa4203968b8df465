"""
The join half of the partition workflow (xugrid/ugrid/partitioning.py:16-148, ``Ugrid2d.merge_partitions`` ugrid2d.py,
``Ugrid2d.reindex_like`` :1574-1617, ``connectivity.index_like`` connectivity.py:38-61) on arrays.  Kernels in
``csrc/xr_merge.hip``; DESIGN section 15.

``merge_partitions`` joins grids into one: nodes that compare equal as doubles become one node (first occurrence kept, bit for
bit), faces with the same node set become one face (first occurrence kept, slot order as given); the merged grid derives its
own edges.  ``labels_to_indices`` / ``partition_by_label`` cut a grid by integer face labels; ``reindex_like`` /
``index_like_device`` match two grids' coordinates.  "Which rows are equal and which came first" is answered by a key table
in HBM, never by a sort; the table always runs on the device.

Kinds of result, as ``subset``: host grids give a host ``Ugrid2d`` and numpy int64 indexes; any device-resident grid in the list
gives a ``DeviceUgrid2d`` and ``DeviceArray`` indexes; torch data or labels give torch results.  The edge arithmetic runs on
the device when every grid in the list is device-resident with a manifold topology, in numpy otherwise.
"""
import numpy as np

from . import engine, netedit, sample, subset
from .subset import FACETS
from .ugrid1d import Ugrid1d

ZERO = "Cannot merge partitions: zero partitions provided."
NOT_IDENTICAL = "coordinates are not identical after sorting"


def _first_torch(items):
    return next((x for x in items if x is not None and engine.is_torch(x)), None)


def _emit(dev, to_numpy):
    return engine.download(dev).astype(np.int64, copy=False) if to_numpy else dev


# ---- labels ---------------------------------------------------------------------------------------------------------------
def _labels_dev(labels, n=None):
    """-> (int64 device array, like): 1-D integer labels from the host or the device."""
    info = engine.device_array_info(labels) if not isinstance(labels, (list, tuple)) else None
    if info is not None:
        _, shape, dtype = info
        if dtype.kind != "i":
            raise TypeError("labels must have integer dtype")
        dev = labels
        if dtype != np.int64:
            if not engine.is_torch(labels):
                raise TypeError("integer device labels must be int64")
            dev = labels.long()
        engine.sync_producer(labels)
        like = labels
    else:
        a = np.asarray(labels)
        shape = a.shape
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("labels must have integer dtype")
        dev, like = engine.DeviceArray.from_host(np.ascontiguousarray(a, dtype=np.int64)), None
    if len(shape) != 1:
        raise ValueError("labels must be 1-D")
    if n is not None and shape[0] != n:
        raise ValueError(f"labels must have the length of the face dimension {n}, received: {shape[0]}")
    return dev, like, int(shape[0])


def labels_to_indices(labels):
    """partitioning.py:16-27: ``[0, 1, 0, 2, 2] -> [[0, 2], [1], [3, 4]]`` -- ``max + 1`` ascending int64 index arrays, an
    empty one for a label that does not occur.  numpy labels give numpy arrays, device labels device arrays of their kind."""
    dev, like, n = _labels_dev(labels)
    return _label_indices(dev, like, n, to_numpy=like is None)


def _label_indices(dev, like, n, to_numpy):
    ptr = engine.device_array_info(dev)[0]
    lo, hi = engine.labels_range(ptr, n)
    if lo < 0:
        raise ValueError("labels must be non-negative")
    return [_emit(ids, to_numpy) for ids in engine.labels_order(ptr, n, hi + 1, like)]


def partition_by_label(grid, labels, data=None):
    """partitioning.py:71-76 on arrays: one ``topology_subset(index, return_index=True)`` result ``(grid, indexes)`` per label
    ``0 .. max``; with ``data`` ``(..., n)`` on one facet each entry is ``(grid, indexes, data[..., indexes[facet]])``."""
    dev, like, n = _labels_dev(labels, grid.n_face)
    to_numpy = like is None and not grid._device_resident
    facet = subset._data_facet(grid, data) if data is not None else None
    dims = {"node": grid.node_dimension, "edge": grid.edge_dimension, "face": grid.face_dimension}
    out = []
    for index in _label_indices(dev, like, n, to_numpy):
        sub, indexes = subset.topology_subset(grid, index, return_index=True)
        if data is None:
            out.append((sub, indexes))
            continue
        by = indexes[dims[facet]]
        if engine.device_array_info(data) is None:
            by = by if isinstance(by, np.ndarray) else engine.download(by)
        elif isinstance(by, np.ndarray):
            by = engine.upload_like(by, data)
        out.append((sub, indexes, sample.gather_points(data, getattr(grid, f"n_{facet}"), by)))
    return out


# ---- merge ----------------------------------------------------------------------------------------------------------------
def _host_edge_node(grid):
    if grid.n_face == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return np.asarray(grid.edge_node_connectivity, dtype=np.int64).reshape(-1, 2)


def _edges_numpy(grids, merged, merge):
    """The kept edges and their ids in the merged grid over the host tables (partitioning.py:137-148 on derived edges)."""
    inverse = merge.node_inverse().download()
    offsets = np.cumsum([0] + [g.n_node for g in grids])
    tables = [_host_edge_node(g) for g in grids]
    slices = np.cumsum([0] + [len(t) for t in tables])
    rows = np.sort(np.concatenate([inverse[t + off] for t, off in zip(tables, offsets)]).reshape(-1, 2), axis=1)
    n_merged = max(merged.n_node, 1)
    keys = rows[:, 0] * n_merged + rows[:, 1]
    _, first = np.unique(keys, return_index=True)
    first.sort()
    merged_edges = _host_edge_node(merged)
    position = np.searchsorted(merged_edges[:, 0] * n_merged + merged_edges[:, 1], keys[first])
    cuts = np.searchsorted(first, slices[1:-1])
    return ([(part - off).astype(np.int64) for part, off in zip(np.split(first, cuts), slices)],
            [p.astype(np.int64) for p in np.split(position, cuts)], slices)


def _device_topologies(grids, merged):
    """The grids' device topologies when the edge arithmetic may run on them, else None."""
    if not all(g._device_resident and g.n_face > 0 for g in list(grids) + [merged]):
        return None
    topologies = [g.device_topology() for g in list(grids) + [merged]]
    return topologies if all(t.manifold for t in topologies) else None


def _merge_facet(grids, data, dim):
    if len(data) != len(grids):
        raise ValueError(f"data must hold one array per partition: {len(grids)} partitions, {len(data)} arrays")
    shapes = []
    for d in data:
        info = engine.device_array_info(d)
        shapes.append(tuple(info[1]) if info is not None else np.shape(d))
    if any(len(s) == 0 for s in shapes) or len({s[:-1] for s in shapes}) != 1:
        raise ValueError("data must have shape (..., n) with the same leading dimensions in every partition")
    if dim is not None:
        names = {grids[0].node_dimension: "node", grids[0].edge_dimension: "edge", grids[0].face_dimension: "face"}
        if dim not in names:
            raise ValueError(f"dim {dim!r} is not a UGRID dimension, expected one of {set(names)}")
        candidates = (names[dim],)
    else:
        candidates = FACETS
    fits = [f for f in candidates if all(s[-1] == getattr(g, f"n_{f}") for s, g in zip(shapes, grids))]
    if len(fits) != 1:
        raise ValueError(f"the last dimension of every data array must be the size of exactly one UGRID dimension of its "
                         f"partition, it fits: {fits}")
    return fits[0]


def _concat(data, sizes):
    """The partitions' data side by side along the last axis -> (array of one kind, total)."""
    total = int(sum(sizes))
    infos = [engine.device_array_info(d) for d in data]
    if all(i is None for i in infos):
        arrays = [np.asarray(d) for d in data]
        dtype = np.float32 if all(a.dtype == np.float32 for a in arrays) else np.float64
        return np.concatenate([a.astype(dtype, copy=False) for a in arrays], axis=-1), total
    if any(i is None for i in infos):
        raise TypeError("the partitions' data must be all host arrays or all device arrays")
    torch_like = _first_torch(data)
    if torch_like is not None:
        import torch

        return torch.cat([d if d.dtype in (torch.float32, torch.float64) else d.double() for d in data], dim=-1).contiguous(), total
    if len({i[2] for i in infos}) != 1:
        raise TypeError("the partitions' device data must have one dtype")
    lead = infos[0][1][:-1]
    K = int(np.prod(lead, dtype=np.int64))
    flat = [d.reshape(K, s) if hasattr(d, "reshape") else d for d, s in zip(data, sizes)]
    return engine.concat_last_axis_dev(flat).reshape(*lead, total), total


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
    facet = _merge_facet(grids, data, dim) if data is not None else None
    host = grids[0]
    lead = next((g for g in grids if g._device_resident), host)
    like = _first_torch(data) if data is not None else None
    to_numpy = like is None and not lead._device_resident
    dims = {"node": host.node_dimension, "edge": host.edge_dimension, "face": host.face_dimension}

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
        for f in need:
            indexes[f] = [np.arange(getattr(host, f"n_{f}"), dtype=np.int64)]
        positions = indexes.get("edge")
        edge_slices = np.array([0, host.n_edge]) if "edge" in need else None
    else:
        for f in need - {"edge"}:
            indexes[f] = [merge.index(f, p, like) for p in range(len(grids))]
        if "edge" in need:
            topologies = _device_topologies(grids, merged)
            if topologies is not None:
                merge.add_edges(topologies[:-1], topologies[-1])
                indexes["edge"] = [merge.index("edge", p, like) for p in range(len(grids))]
                positions = [merge.index("edge", p, like, position=True) for p in range(len(grids))]
                edge_slices = np.cumsum([0] + [t.n_edge for t in topologies[:-1]])
            else:
                indexes["edge"], positions, edge_slices = _edges_numpy(grids, merged, merge)
    if return_index:
        def emit(a):
            if isinstance(a, np.ndarray):
                return a if to_numpy else engine.upload_like(a, like)
            return _emit(a, to_numpy)

        out.append({dims[f]: [emit(a) for a in indexes[f]] for f in FACETS})
    if data is not None:
        sizes = [getattr(g, f"n_{facet}") for g in grids]
        cat, total = _concat(data, sizes)
        if facet == "edge":
            source = np.full(merged.n_edge, -1, dtype=np.int64)
            for p, (idx, pos) in enumerate(zip(indexes["edge"], positions)):
                idx, pos = (a if isinstance(a, np.ndarray) else engine.download(a) for a in (idx, pos))
                source[pos] = idx + edge_slices[p]
        elif merge is None:
            source = indexes[facet][0]
        else:
            source = merge.index(facet, -1, like)
        if engine.device_array_info(cat) is None:
            source = source if isinstance(source, np.ndarray) else engine.download(source)
        elif isinstance(source, np.ndarray):
            source = engine.upload_like(source, cat)
        out.append(sample.gather_points(cat, total, source))
    return out[0] if len(out) == 1 else tuple(out)


# ---- matching coordinates ---------------------------------------------------------------------------------------------------
def _xy_dev(xy):
    info = engine.device_array_info(xy)
    if info is not None:
        ptr, shape, dtype = info
        if dtype != np.float64:
            raise TypeError("device coordinates must be float64")
        engine.sync_producer(xy)
        return xy, ptr, tuple(shape)
    a = np.ascontiguousarray(xy, dtype=np.float64)
    dev = engine.DeviceArray.from_host(a)
    return dev, dev.ptr, a.shape


def index_like_device(xy_a, xy_b, tolerance=0.0):
    """connectivity.py:38-61 through the key table: ``index[i]`` is the row of ``xy_a`` that equals row ``i`` of ``xy_b``, so
    ``xy_a[index]`` is ``xy_b``.  The key is the coordinate pair, or ``rint(xy / tolerance)`` for a non-zero tolerance; after
    matching every pair must lie within the tolerance on both axes.  Keys that repeat inside either input, and rows without a
    partner, raise ``ValueError("coordinates are not identical after sorting")`` (the reference pairs by sorted position and
    accepts some of those: DESIGN section 7).  numpy in -> numpy out; a device array in -> an int64 device array."""
    keep_a, ptr_a, shape_a = _xy_dev(xy_a)
    keep_b, ptr_b, shape_b = _xy_dev(xy_b)
    if shape_a != shape_b:
        raise ValueError("coordinates do not match in shape")
    if len(shape_a) != 2 or shape_a[1] != 2:
        raise ValueError(f"expected (n, 2) coordinates, received shape {shape_a}")
    like = _first_torch([xy_a, xy_b])
    index, repeats, misses = engine.index_like_dev(ptr_a, ptr_b, shape_a[0], abs(float(tolerance)), like)
    if repeats or misses:
        raise ValueError(NOT_IDENTICAL)
    host = engine.device_array_info(xy_a) is None and engine.device_array_info(xy_b) is None
    return engine.download(index).astype(np.int64, copy=False) if host else index


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
    if dim is not None:
        names = {grid.node_dimension: "node", grid.edge_dimension: "edge", grid.face_dimension: "face"}
        if dim not in names:
            raise ValueError(f"dim {dim!r} is not a UGRID dimension, expected one of {set(names)}")
        facet = names[dim]
    else:
        facet = subset._data_facet(grid, data)
    index = index_like_device(_facet_coordinates(grid, facet), _facet_coordinates(other, facet), tolerance)
    if engine.device_array_info(data) is None:
        index = index if isinstance(index, np.ndarray) else engine.download(index)
    elif isinstance(index, np.ndarray):
        index = engine.upload_like(index, data)
    return sample.gather_points(data, getattr(grid, f"n_{facet}"), index)
