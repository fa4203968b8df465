"""
Editing networks: ``topology_subset`` / ``isel`` / ``sel`` / ``clip_box`` / ``remove_self_loops`` / ``refine_by_vertices`` of
``Ugrid1d`` (xugrid/ugrid/ugrid1d.py:574-672, :714-738, :770-876; the index rules of ugridbase.py:42-78 and :703-720) and its
part of the partition workflow (``merge_partitions``, partitioning.py:81-116 and :137-148; ``reindex_like``) on arrays.
Kernels in ``csrc/xr_netedit.hip``; DESIGN section 18.

Every edit runs on the device: the grid's ``node_xy`` and ``edges`` are uploaded once and kept with its other caches
(``Ugrid1d.drop_device_caches`` releases them).  ``Ugrid1d`` is a host-array class, so every result is a host ``Ugrid1d`` that
carries the parent's ``name``.  Indexers, indexes and ``data`` follow ``subset.py``: 1-D integer ids (unique, any order) or a
bool mask of the dimension's length, from the host or the device; device indexers give device indexes of their kind back,
host ones numpy int64.  ``data`` ``(..., n)``: numpy in -> numpy out, a device array in -> a float64 device array out.
"""
import numpy as np

from . import engine, sample, subset
from .engine import DeviceNetEdit
from .subset import Index, _raise_problems, _same, as_index

FACETS = ("node", "edge")
ZERO = "Cannot merge partitions: zero partitions provided."
OFF_EDGE = "The following vertices are not located on any edge:\n"
DEFAULT_TOLERANCE = 1e-9  # times the larger side of the node bounding box


def _ugrid1d():
    from .ugrid1d import Ugrid1d

    return Ugrid1d


def device_arrays(grid):
    """-> (node_xy float64 (n_node, 2), edges int64 (n_edge, 2)) as ``DeviceArray``: uploaded on first use, kept on the grid."""
    cache = grid.__dict__.get("_netedit_cache")
    if cache is None:
        cache = grid.__dict__["_netedit_cache"] = (
            engine.DeviceArray.from_host(np.ascontiguousarray(grid.node_coordinates, dtype=np.float64).reshape(-1, 2)),
            engine.DeviceArray.from_host(np.ascontiguousarray(grid.edge_node_connectivity, dtype=np.int64).reshape(-1, 2)),
        )
    return cache


def _network_args(grid):
    xy, edges = device_arrays(grid)
    return xy.ptr, grid.n_node, edges.ptr, grid.n_edge


def _grid_from(grid, net):
    xy, edges = net.node_xy().download(), net.edges().download()
    return _ugrid1d()(xy[:, 0], xy[:, 1], grid.fill_value, edges, name=grid.name)


def _arange(n):
    return Index(host=np.arange(n, dtype=np.int64))


def _dims(grid):
    return {grid.node_dimension: "node", grid.edge_dimension: "edge"}


def _data_facet(grid, data, dim=None):
    """The facet ``data`` ``(..., n)`` lies on; ``dim`` names it where ``n_node == n_edge`` (a ring) leaves it open."""
    info = engine.device_array_info(data)
    shape = info[1] if info is not None else np.shape(data)
    if len(shape) == 0:
        raise ValueError("data must have shape (..., n) with n the size of one UGRID dimension")
    candidates = FACETS
    if dim is not None:
        if dim not in _dims(grid):
            raise ValueError(f"dim {dim!r} is not a UGRID dimension, expected one of {set(_dims(grid))}")
        candidates = (_dims(grid)[dim],)
    fits = [f for f in candidates if getattr(grid, f"n_{f}") == shape[-1]]
    if len(fits) != 1:
        raise ValueError(f"the last dimension of data ({shape[-1]}) must be the size of exactly one of the UGRID dimensions, "
                         f"it fits: {fits}")
    return fits[0]


def _gather(data, n, index):
    """``data[..., index]`` with ``index`` an ``Index``: on the side ``data`` is on."""
    by = index.device() if engine.device_array_info(data) is not None else index.numpy()
    return sample.gather_points(data, n, by)


def _cut(grid, edge_index, want_node=False, keep_identity=True):
    """-> (sub-grid, or ``grid`` itself for the identity when ``keep_identity``; node Index or None)."""
    xy_ptr, n_node, edges_ptr, n_edge = _network_args(grid)
    net, identity, problems = DeviceNetEdit.subset(xy_ptr, n_node, edges_ptr, n_edge, edge_index.ptr() if edge_index.n else 0, edge_index.n,
                                                   keep_identity)
    _raise_problems(problems, n_edge)
    if identity:
        return grid, (_arange(n_node) if want_node else None)
    return _grid_from(grid, net), (Index(dev=net.node_index(edge_index.like)) if want_node else None)


def _emit(grid, like, node_index, edge_index):
    to_numpy = like is None
    return {grid.node_dimension: node_index.emit(like, to_numpy), grid.edge_dimension: edge_index.emit(like, to_numpy)}


def topology_subset(grid, edge_index, return_index=False):
    """ugrid1d.py:603-663 on arrays: see ``Ugrid1d.topology_subset``."""
    index = as_index(edge_index, grid.n_edge, checked=False)
    sub, node_index = _cut(grid, index, return_index)
    if not return_index:
        return sub
    return sub, _emit(grid, index.like, node_index, index)


def _edges_of(grid, facet, index):
    """The edge index a node selection stands for: ``np.unique(node_edge_connectivity[node_index].data)``."""
    if facet == "edge":
        return index
    _, n_node, edges_ptr, n_edge = _network_args(grid)
    found = engine.network_index("edges_of_nodes", engine.vp(edges_ptr), n_edge, n_node, engine.vp(index.ptr() if index.n else 0), index.n)
    return Index(dev=found.to_dev(index.like), like=index.like)


def _finish(grid, sub, final, like, return_index, data, dim=None):
    out = [sub]
    if return_index:
        out.append(_emit(grid, like, final["node"], final["edge"]))
    if data is not None:
        facet = _data_facet(grid, data, dim)
        out.append(_gather(data, getattr(grid, f"n_{facet}"), final[facet]))
    return out[0] if len(out) == 1 else tuple(out)


def isel(grid, indexers=None, return_index=False, data=None, dim=None, **indexers_kwargs):
    """ugridbase.py:703-720 with ugrid1d.py:603-663 on arrays: see ``Ugrid1d.isel``."""
    if indexers is not None and indexers_kwargs:
        raise ValueError("cannot specify both keyword and positional arguments to .isel")
    indexers = dict(indexers if indexers is not None else indexers_kwargs)
    dims = _dims(grid)
    invalid = set(indexers) - set(dims)
    if invalid:
        raise ValueError(f"Dimensions {invalid} do not exist. Expected one of {set(dims)}")
    if not indexers:
        raise ValueError("isel needs an indexer for at least one UGRID dimension")
    if data is not None:
        _data_facet(grid, data, dim)
    data_dim = dim
    given = {dim: as_index(v, getattr(grid, f"n_{dims[dim]}")) for dim, v in indexers.items()}
    edge_index = {dim: _edges_of(grid, dims[dim], index) for dim, index in given.items()}
    # pre-check: every dimension must stand for the same edges
    dim, index = edge_index.popitem()
    for check_dim, check_index in edge_index.items():
        if not _same(index, check_index):
            raise ValueError(f"UGRID dimensions do not align: {dim} versus {check_dim}")
    sub, node_index = _cut(grid, index, True)
    final = {"node": node_index, "edge": index}
    # post-check: a node selection must be exactly the nodes of the edges it stands for
    for dim, indexer in given.items():
        if dims[dim] == "node" and not _same(indexer, node_index):
            raise ValueError(f"This subset selection of UGRID dimension {dim} results in an invalid topology ")
    like = next((i.like for i in given.values() if i.like is not None), None)
    return _finish(grid, sub, final, like, return_index, data, data_dim)


def _bounds(indexer):
    """ugrid1d.py:564-572; a ``None`` bound is unbounded on that side (an addition: DESIGN section 7)."""
    if indexer is None:
        indexer = slice(None, None)
    if not isinstance(indexer, slice):
        raise ValueError("Ugrid1d only supports slice indexing")
    if indexer.step is not None:
        raise ValueError("Ugrid1d does not support steps in slices")
    start = -np.inf if indexer.start is None else float(indexer.start)
    stop = np.inf if indexer.stop is None else float(indexer.stop)
    if start >= stop:
        raise ValueError("slice start should be smaller than slice stop")
    return start, stop


def sel(grid, x=None, y=None, data=None, return_index=False, dim=None):
    """ugrid1d.py:574-601 on arrays: see ``Ugrid1d.sel``."""
    xmin, xmax = _bounds(x)
    ymin, ymax = _bounds(y)
    if data is not None:
        _data_facet(grid, data, dim)
    xy_ptr, n_node, edges_ptr, n_edge = _network_args(grid)
    found = engine.network_index("box_edges", engine.vp(xy_ptr), n_node, engine.vp(edges_ptr), n_edge, xmin, ymin, xmax, ymax)
    index = Index(dev=found.to_dev())
    sub, node_index = _cut(grid, index, return_index or data is not None)
    return _finish(grid, sub, {"node": node_index, "edge": index}, None, return_index, data, dim)


def clip_box(grid, xmin, ymin, xmax, ymax):
    """ugrid1d.py:665-672."""
    return sel(grid, x=slice(xmin, xmax), y=slice(ymin, ymax))


def remove_self_loops(grid, return_index=False):
    """ugrid1d.py:714-738: see ``Ugrid1d.remove_self_loops``."""
    _, _, edges_ptr, n_edge = _network_args(grid)
    index = Index(dev=engine.network_index("nonloop_edges", engine.vp(edges_ptr), n_edge).to_dev())
    sub, node_index = _cut(grid, index, return_index, keep_identity=False)
    if not return_index:
        return sub
    return sub, _emit(grid, None, node_index, index)


# ---- partitions -----------------------------------------------------------------------------------------------------------------
def _merge_facet(grids, data, dim):
    if len(data) != len(grids):
        raise ValueError(f"data must hold one array per partition: {len(grids)} partitions, {len(data)} arrays")
    shapes = []
    for d in data:
        info = engine.device_array_info(d)
        shapes.append(tuple(info[1]) if info is not None else np.shape(d))
    if any(len(s) == 0 for s in shapes) or len({s[:-1] for s in shapes}) != 1:
        raise ValueError("data must have shape (..., n) with the same leading dimensions in every partition")
    candidates = FACETS
    if dim is not None:
        names = _dims(grids[0])
        if dim not in names:
            raise ValueError(f"dim {dim!r} is not a UGRID dimension, expected one of {set(names)}")
        candidates = (names[dim],)
    fits = [f for f in candidates if all(s[-1] == getattr(g, f"n_{f}") for s, g in zip(shapes, grids))]
    if len(fits) != 1:
        raise ValueError(f"the last dimension of every data array must be the size of exactly one UGRID dimension of its "
                         f"partition, it fits: {fits}")
    return fits[0]


def merge_partitions(grids, return_index=False, data=None, dim=None):
    """partitioning.py:81-116, :137-148 on arrays: see ``Ugrid1d.merge_partitions``."""
    from . import partition

    grids = list(grids)
    if len(grids) == 0:
        raise ValueError(ZERO)
    if not all(isinstance(g, _ugrid1d()) for g in grids):
        raise TypeError(f"All partition topologies should be of the same type, received: {sorted({type(g).__name__ for g in grids})}")
    if data is not None:
        data = list(data)
    facet = _merge_facet(grids, data, dim) if data is not None else None
    host = grids[0]
    like = partition._first_torch(data) if data is not None else None
    to_numpy = like is None
    P = len(grids)
    if P == 1:  # (partitioning.py: one partition is the grid itself)
        merged = host
        indexes = {"node": [np.arange(host.n_node, dtype=np.int64)], "edge": [np.arange(host.n_edge, dtype=np.int64)]}
    else:
        args = [_network_args(g) for g in grids]
        net = DeviceNetEdit.merge([a[0] for a in args], [a[1] for a in args], [a[2] for a in args], [a[3] for a in args])
        merged = _grid_from(host, net)
        need = set(FACETS) if return_index else ({facet} if facet else set())
        indexes = {f: [engine.download(net.part_index(FACETS.index(f), p)).astype(np.int64, copy=False) for p in range(P)] for f in need}
    out = [merged]
    if return_index:
        emit = (lambda a: a) if to_numpy else (lambda a: engine.upload_like(a, like))
        out.append({getattr(host, f"{f}_dimension"): [emit(a) for a in indexes[f]] for f in FACETS})
    if data is not None:
        sizes = [getattr(g, f"n_{facet}") for g in grids]
        cat, total = partition._concat(data, sizes)
        offsets = np.cumsum([0] + sizes)
        source = np.concatenate([idx + off for idx, off in zip(indexes[facet], offsets)])
        if engine.device_array_info(cat) is not None:
            source = engine.upload_like(source, cat)
        out.append(sample.gather_points(cat, total, source))
    return out[0] if len(out) == 1 else tuple(out)


def reindex_like(grid, other, data, dim=None, tolerance=0.0):
    """See ``Ugrid1d.reindex_like``: nodes are matched by their coordinates, edges by their midpoints."""
    from . import partition

    if not isinstance(other, _ugrid1d()):
        raise TypeError(f"Expected Ugrid1d, received: {type(other).__name__}")
    if dim is not None:
        names = _dims(grid)
        if dim not in names:
            raise ValueError(f"dim {dim!r} is not a UGRID dimension, expected one of {set(names)}")
        facet = names[dim]
    else:
        facet = _data_facet(grid, data)
    coordinates = (lambda g: g.node_coordinates) if facet == "node" else (lambda g: g.edge_coordinates)
    index = partition.index_like_device(coordinates(grid), coordinates(other), tolerance)
    if engine.device_array_info(data) is not None:
        index = engine.upload_like(index, data)
    return sample.gather_points(data, getattr(grid, f"n_{facet}"), index)


# ---- refinement -----------------------------------------------------------------------------------------------------------------
def default_tolerance(grid):
    if grid.n_node == 0:
        return 0.0
    xmin, ymin, xmax, ymax = grid.bounds
    return DEFAULT_TOLERANCE * max(xmax - xmin, ymax - ymin)


def refine_by_vertices(grid, vertices, return_index=False, tolerance=None, data=None):
    """ugrid1d.py:770-876 on arrays: see ``Ugrid1d.refine_by_vertices``."""
    if tolerance is not None and not float(tolerance) >= 0.0:
        raise ValueError(f"tolerance must be non-negative, received: {tolerance}")
    if data is not None:  # (only edge data has a meaning here: the edge dimension wins where both sizes fit, a ring for one)
        info = engine.device_array_info(data)
        shape = info[1] if info is not None else np.shape(data)
        if len(shape) == 0 or shape[-1] != grid.n_edge:
            if len(shape) and shape[-1] == grid.n_node:
                raise ValueError("node data cannot be carried across a refinement: the new nodes have no value")
            raise ValueError(f"data must have shape (..., n_edge) with n_edge = {grid.n_edge}")
    tolerance = default_tolerance(grid) if tolerance is None else float(tolerance)
    info = engine.device_array_info(vertices) if not isinstance(vertices, (list, tuple)) else None
    if info is not None:
        ptr, shape, dtype = info
        if dtype != np.float64:
            raise TypeError("device vertices must be float64")
        engine.sync_producer(vertices)
        keep, like = vertices, vertices
    else:
        host = np.ascontiguousarray(vertices, dtype=np.float64)
        shape = host.shape
        keep, like = engine.DeviceArray.from_host(host.reshape(-1, 2)) if host.size else None, None
        ptr = keep.ptr if keep is not None else 0
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"expected (n, 2) vertices, received shape {tuple(shape)}")
    net, n_off = DeviceNetEdit.refine(*_network_args(grid), ptr, shape[0], tolerance)
    if n_off:
        xy = np.asarray(engine.download(vertices) if info is not None else vertices, dtype=np.float64).reshape(-1, 2)
        raise ValueError(f"{OFF_EDGE}{xy[net.off_edge()]}")
    out = [_grid_from(grid, net)]
    if return_index:
        node_index = net.node_index(like)
        out.append(node_index if like is not None else engine.download(node_index).astype(np.int64, copy=False))
    if data is not None:
        out.append(_gather(data, grid.n_edge, Index(dev=net.parent_edge(data if engine.is_torch(data) else None))))
    return out[0] if len(out) == 1 else tuple(out)
