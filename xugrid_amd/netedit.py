"""
Editing networks: ``topology_subset`` / ``isel`` / ``sel`` / ``clip_box`` / ``remove_self_loops`` / ``refine_by_vertices`` of
``Ugrid1d`` (xugrid/ugrid/ugrid1d.py:574-672, :714-738, :770-876; the index rules of ugridbase.py:42-78 and :703-720) and its
part of the partition workflow (``merge_partitions``, partitioning.py:81-116 and :137-148; ``reindex_like``) on arrays.
Kernels in ``csrc/xr_netedit.hip``; DESIGN section 18.

Every edit runs on the device: the grid's ``node_xy`` and ``edges`` are uploaded once and kept with its other caches
(``Ugrid1d.drop_device_caches`` releases them).  ``Ugrid1d`` is a host-array class, so every result is a host ``Ugrid1d`` that
carries the parent's ``name``.  Indexers, indexes and ``data`` follow ``inkind.py``: 1-D integer ids (unique, any order) or a
bool mask of the dimension's length, from the host or the device; device indexers give device indexes of their kind back,
host ones numpy int64.  ``data`` ``(..., n)``: numpy in -> numpy out, a device array in -> a float64 device array out.
"""
import numpy as np

from . import engine
from .engine import DeviceNetEdit
from .inkind import (Index, as_index, check_aligned, concat_last_axis, data_facet, facet_names, first_torch, parse_indexers,
                     raise_problems, result_kind, xy_dev)

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


def _cut(grid, edge_index, want_node=False, keep_identity=True):
    """-> (sub-grid, or ``grid`` itself for the identity when ``keep_identity``; node Index or None)."""
    xy_ptr, n_node, edges_ptr, n_edge = _network_args(grid)
    net, identity, problems = DeviceNetEdit.subset(xy_ptr, n_node, edges_ptr, n_edge, edge_index.ptr() if edge_index.n else 0, edge_index.n,
                                                   keep_identity)
    raise_problems(problems, n_edge)
    if identity:
        return grid, (Index.arange(n_node) if want_node else None)
    return _grid_from(grid, net), (Index(dev=net.node_index(edge_index.like)) if want_node else None)


def _emit(grid, like, node_index, edge_index):
    like, to_numpy = result_kind(grid, like)
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


def _finish(grid, sub, final, like, return_index, data, facet):
    out = [sub]
    if return_index:
        out.append(_emit(grid, like, final["node"], final["edge"]))
    if data is not None:
        out.append(final[facet].gather(data, getattr(grid, f"n_{facet}")))
    return out[0] if len(out) == 1 else tuple(out)


def isel(grid, indexers=None, return_index=False, data=None, dim=None, **indexers_kwargs):
    """ugridbase.py:703-720 with ugrid1d.py:603-663 on arrays: see ``Ugrid1d.isel``."""
    facet = data_facet(grid, data, dim) if data is not None else None
    given = parse_indexers(grid, indexers, indexers_kwargs)
    dims = facet_names(grid)
    # pre-check: every dimension must stand for the same edges
    index = check_aligned({d: _edges_of(grid, dims[d], i) for d, i in given.items()})
    sub, node_index = _cut(grid, index, True)
    # post-check: a node selection must be exactly the nodes of the edges it stands for
    for d, indexer in given.items():
        if dims[d] == "node" and not Index.same(indexer, node_index):
            raise ValueError(f"This subset selection of UGRID dimension {d} results in an invalid topology ")
    like = next((i.like for i in given.values() if i.like is not None), None)
    return _finish(grid, sub, {"node": node_index, "edge": index}, like, return_index, data, facet)


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
    facet = data_facet(grid, data, dim) if data is not None else None
    xy_ptr, n_node, edges_ptr, n_edge = _network_args(grid)
    found = engine.network_index("box_edges", engine.vp(xy_ptr), n_node, engine.vp(edges_ptr), n_edge, xmin, ymin, xmax, ymax)
    index = Index(dev=found.to_dev())
    sub, node_index = _cut(grid, index, return_index or data is not None)
    return _finish(grid, sub, {"node": node_index, "edge": index}, None, return_index, data, facet)


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
def merge_partitions(grids, return_index=False, data=None, dim=None):
    """partitioning.py:81-116, :137-148 on arrays: see ``Ugrid1d.merge_partitions``."""
    grids = list(grids)
    if len(grids) == 0:
        raise ValueError(ZERO)
    if not all(isinstance(g, _ugrid1d()) for g in grids):
        raise TypeError(f"All partition topologies should be of the same type, received: {sorted({type(g).__name__ for g in grids})}")
    if data is not None:
        data = list(data)
    facet = data_facet(grids, data, dim) if data is not None else None
    host = grids[0]
    like, to_numpy = result_kind(grids, first_torch(data) if data is not None else None)
    P = len(grids)
    if P == 1:  # (partitioning.py: one partition is the grid itself)
        merged = host
        indexes = {f: [Index.arange(getattr(host, f"n_{f}"))] for f in FACETS}
    else:
        args = [_network_args(g) for g in grids]
        net = DeviceNetEdit.merge([a[0] for a in args], [a[1] for a in args], [a[2] for a in args], [a[3] for a in args])
        merged = _grid_from(host, net)
        need = set(FACETS) if return_index else ({facet} if facet else set())
        indexes = {f: [Index(dev=net.part_index(FACETS.index(f), p)) for p in range(P)] for f in need}
    out = [merged]
    if return_index:
        out.append({getattr(host, f"{f}_dimension"): [i.emit(like, to_numpy) for i in indexes[f]] for f in FACETS})
    if data is not None:
        sizes = [getattr(g, f"n_{facet}") for g in grids]
        cat, total = concat_last_axis(data, sizes)
        offsets = np.cumsum([0] + sizes)
        source = Index(host=np.concatenate([i.numpy() + off for i, off in zip(indexes[facet], offsets)]))
        out.append(source.gather(cat, total))
    return out[0] if len(out) == 1 else tuple(out)


def reindex_like(grid, other, data, dim=None, tolerance=0.0):
    """See ``Ugrid1d.reindex_like``: nodes are matched by their coordinates, edges by their midpoints."""
    from .partition import index_like_device

    if not isinstance(other, _ugrid1d()):
        raise TypeError(f"Expected Ugrid1d, received: {type(other).__name__}")
    facet = data_facet(grid, data, dim)
    coordinates = (lambda g: g.node_coordinates) if facet == "node" else (lambda g: g.edge_coordinates)
    index = Index.wrap(index_like_device(coordinates(grid), coordinates(other), tolerance))
    return index.gather(data, getattr(grid, f"n_{facet}"))


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
    on_device = engine.device_array_info(vertices) is not None
    keep, ptr, shape = xy_dev(vertices, "vertices")
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"expected (n, 2) vertices, received shape {tuple(shape)}")
    net, n_off = DeviceNetEdit.refine(*_network_args(grid), ptr if shape[0] else 0, shape[0], tolerance)
    if n_off:
        xy = np.asarray(engine.download(vertices) if on_device else vertices, dtype=np.float64).reshape(-1, 2)
        raise ValueError(f"{OFF_EDGE}{xy[net.off_edge()]}")
    out = [_grid_from(grid, net)]
    if return_index:
        like, to_numpy = result_kind(grid, vertices if on_device else None)
        out.append(Index(dev=net.node_index(like)).emit(like, to_numpy))
    if data is not None:
        out.append(Index(dev=net.parent_edge(data if engine.is_torch(data) else None)).gather(data, grid.n_edge))
    return out[0] if len(out) == 1 else tuple(out)
