"""
Periodic grids: ``Ugrid2d.to_periodic`` (xugrid/ugrid/ugrid2d.py:1392-1462) and ``Ugrid2d.to_nonperiodic`` (:1464-1572) on
arrays.  Kernels in ``csrc/xr_periodic.hip``; DESIGN section 16.

``to_periodic`` folds the right column of nodes (``x`` close to the largest ``x``) onto the left one: in a working copy every
right node gets ``x = xmin``, rows that then compare equal as doubles become one node (first occurrence kept, kept nodes keep
their order and their ORIGINAL coordinates), faces go through the node map with their fill slots left at ``-1``.
``to_nonperiodic(xmax)`` cuts the seam open again: the nodes a face reaches across more than half the domain are appended as
``(xmax, y)`` and those slots name the copies.  Both return a new grid; the input grid is never modified.

Each also knows, per UGRID dimension, the GATHER index that aligns data of the old grid with the new one:
``data_new = data[..., index]`` on all three facets.  The grids derive their edges, so the edge index is in the new grid's own
edge numbering: after ``to_periodic`` ``index[e]`` is the lowest old edge that became new edge ``e``; after ``to_nonperiodic``
the old edge whose node pair new edge ``e`` maps back to.

Kinds of result, as ``subset`` and ``partition``: a host grid gives a host ``Ugrid2d`` and numpy int64 indexes, a
device-resident grid a ``DeviceUgrid2d`` and ``DeviceArray`` indexes; torch data gives torch results.  The mesh is always
converted on the device.  The edge arithmetic runs on the device for device-resident grids with manifold topologies, in numpy
over the host tables otherwise.
"""
import numpy as np

from . import engine
from .inkind import Index, data_facet, device_topologies, host_edge_node, result_kind

FACETS = ("node", "edge", "face")

Y_MISMATCH = "y-coordinates of the left and right boundaries do not match"
NO_COUNTERPART = ("Cannot map edge-associated data onto the non-periodic grid:\n"
                  "the new grid has edges with no counterpart in the periodic grid,\n"
                  "which suggests a degenerate periodic topology.\n"
                  "Please file an issue at: github.com/deltares/xugrid/issues")


def _edges_numpy(grid, new, handle):
    """The edge index over the host tables (both grids' derived edges are (lower, higher) rows in lexicographic order)."""
    old_edges, new_edges = host_edge_node(grid), host_edge_node(new)
    if len(new_edges) == 0:
        return np.zeros(0, dtype=np.int64)
    width = max(grid.n_node, new.n_node, 1)
    if handle.wrapped:  # the old edges through the node map; of the old edges of one new pair the first is the lowest
        rows = np.sort(handle.node_inverse().download()[old_edges], axis=1)
        keys, source = np.unique(rows[:, 0] * width + rows[:, 1], return_index=True)
        wanted = new_edges[:, 0] * width + new_edges[:, 1]
    else:  # the new edges through the node index, looked up among the old ones
        keys, source = old_edges[:, 0] * width + old_edges[:, 1], np.arange(len(old_edges), dtype=np.int64)
        rows = np.sort(handle.index("node").download()[new_edges], axis=1)
        wanted = rows[:, 0] * width + rows[:, 1]
    position = np.clip(np.searchsorted(keys, wanted), 0, max(len(keys) - 1, 0))
    if len(keys) == 0 or not np.array_equal(keys[position], wanted):
        raise ValueError(NO_COUNTERPART)
    return source[position].astype(np.int64)


def _edge_index(grid, new, handle, like):
    """-> the edge ``Index``: from the device topologies, or from the host route."""
    topologies = device_topologies([grid], new)
    if topologies is None:
        return Index(host=_edges_numpy(grid, new, handle))
    if handle.add_edges(topologies[0], topologies[1]):
        raise ValueError(NO_COUNTERPART)
    return Index(dev=handle.index("edge", like))


def _convert(grid, handle, data, facet, return_index):
    like, to_numpy = result_kind(grid, data if data is not None and engine.is_torch(data) else None)
    new = grid._grid_from_mesh(handle.take_mesh())
    out = [new]
    need = set(FACETS) if return_index else ({facet} if facet else set())
    indexes = {f: (_edge_index(grid, new, handle, like) if f == "edge" else Index(dev=handle.index(f, like))) for f in need}
    if return_index:
        out.append({getattr(grid, f"{f}_dimension"): indexes[f].emit(like, to_numpy) for f in FACETS})
    if data is not None:
        out.append(indexes[facet].gather(data, getattr(grid, f"n_{facet}")))
    return out[0] if len(out) == 1 else tuple(out)


def to_periodic(grid, data=None, dim=None, return_index=False):
    """See ``Ugrid2d.to_periodic``."""
    facet = data_facet(grid, data, dim) if data is not None else None  # (before any work is done)
    handle, _ = engine.DevicePeriodic.wrap(grid.device_mesh)
    if handle is None:
        raise ValueError(Y_MISMATCH)
    return _convert(grid, handle, data, facet, return_index)


def to_nonperiodic(grid, xmax, data=None, dim=None, return_index=False):
    """See ``Ugrid2d.to_nonperiodic``."""
    facet = data_facet(grid, data, dim) if data is not None else None
    return _convert(grid, engine.DevicePeriodic.unwrap(grid.device_mesh, float(xmax)), data, facet, return_index)
