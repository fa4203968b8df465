"""
Snapping lines to the edges of a mesh on the device: ``create_snap_to_grid_dataframe`` (xugrid/ugrid/snapping.py:367-493) and
``snap_to_grid`` (:496-552) on arrays.  Kernels in ``csrc/xr_snapgrid.hip``; DESIGN section 21.

``lines = (coords (n, 2), line_offsets (n_line + 1)[, values (n_line,) or (K, n_line)])``, the layout of
``burn_vector_geometry``: a segment joins consecutive vertices of one line, a line of 0 or 1 vertices has none (INTEGRATION.md
has the lines that turn a GeoDataFrame into them).  The array contract is ``burn.py``'s: numpy in -> numpy out; if ``coords`` is
a device array (a torch tensor on the GPU, ``__cuda_array_interface__``) every result is a device array of that kind and only
sizes cross PCIe.  Inputs are never modified.

The rule is the reference's, stage by stage: the vertices snap onto the grid's nodes (``snap_to_nodes`` with
``tiebreaker="nearest"``; the lowest id among equidistant nodes, where the reference's choice is arbitrary); every segment is
cut into its pieces per face (the clipper of ``CellTree2d.intersect_edges``); a piece snaps to an interior edge of its face
iff, widened by ``tolerance * max(|Ux|, |Uy|)`` at both ends, it separates the centroids of the two faces beside the edge
(``snap_to_edges``, :255-325).  Every such (piece, edge) is a row of the frame.

Row order: by segment, then face ascending, then edge ascending.  The reference's rows are ordered by segment too, but within
one segment they follow the traversal order of numba_celltree, which cannot be restated; ``CellTree2d.intersect_edges``
normalises that order to face ascending and so does this module.  ``snap_to_grid`` does not depend on it except between rows of
EQUAL length on one edge, and those come from one line whenever they come from one segment.
"""
import numpy as np

from . import burn, engine
from .engine import DeviceSnapGrid

COLUMNS = ("line_index", "edge_index", "x0", "y0", "x1", "y1", "length")


class _Values:
    """The optional third array of ``lines``: float64 ``(n_line,)`` or ``(K, n_line)`` on the host or the device."""

    def __init__(self, array, n_line):
        info = engine.device_array_info(array)
        if info is not None:
            if info[2] != np.float64:
                if not engine.is_torch(array):
                    raise TypeError(f"line values on the device must be float64, received {info[2]}")
                import torch

                array = array.to(torch.float64)
                info = engine.device_array_info(array)
            engine.sync_producer(array)
            self.shape, self.keep, self._ptr, self.host = tuple(info[1]), array, info[0], None
        else:
            self.host = np.ascontiguousarray(array, dtype=np.float64)
            self.shape, self.keep = self.host.shape, None
        if len(self.shape) not in (1, 2):
            raise ValueError(f"line values: expected an array of shape (n_line,) or (K, n_line), received shape {self.shape}")
        if self.shape[-1] != n_line:
            raise ValueError(f"lines: {self.shape[-1]} values for {n_line} geometries")
        self.K = self.shape[0] if len(self.shape) == 2 else 1

    @property
    def ptr(self):
        if self.keep is None:
            self.keep = engine.DeviceArray.from_host(self.host)
            self._ptr = self.keep.ptr
        return self._ptr


def _line_args(lines):
    parts = burn._parts(lines, 2, "lines")
    coords = burn._coords(parts[0], "line")
    offsets = burn._offsets(parts[1], "line_offsets", coords.n)
    values = _Values(parts[2], offsets.n - 1) if len(parts) == 3 else None
    return coords, offsets, values


def _snapgrid(lines, grid, max_snap_distance, tolerance, reduce):
    from .ugrid2d import Ugrid2d

    if not isinstance(grid, Ugrid2d):
        raise TypeError(f"Expected Ugrid2d, received: {type(grid).__name__}")
    # every argument is checked before the first launch
    coords, offsets, values = _line_args(lines)
    if not float(max_snap_distance) >= 0.0:
        raise ValueError(f"max_snap_distance must be non-negative, received: {max_snap_distance}")
    tolerance = float(tolerance)
    if tolerance != tolerance:
        raise ValueError("tolerance must be a number")
    topology = grid.device_topology()
    if not topology.manifold:
        raise ValueError("snap_to_grid needs a grid whose edges have at most two faces")
    node_index = grid._nearest_index("node") if grid.n_node else None
    made = DeviceSnapGrid(grid.device_mesh, topology, node_index, coords.ptr, coords.n, offsets.ptr, offsets.n - 1, max_snap_distance,
                          tolerance, reduce)
    return made, coords.device, values


def _out(device_like, array):
    return array if device_like is not None else array.download()


def create_snap_to_grid_dataframe(lines, grid, max_snap_distance, tolerance=1e-12):
    """snapping.py:367-493 on arrays -> a dict with one array per column of the reference's frame: ``line_index`` and
    ``edge_index`` int64, ``x0``, ``y0``, ``x1``, ``y1`` (the piece inside its face, as the clipper leaves it) and ``length``
    float64.  ``length`` is the SQUARED length of the piece, as in the reference (:491).  ``pandas.DataFrame(frame)`` is the
    reference's frame up to the order of the rows within one segment: see the module docstring."""
    made, like, _ = _snapgrid(lines, grid, max_snap_distance, tolerance, reduce=False)
    return {name: _out(like, made.column(what, like)) for what, name in enumerate(COLUMNS)}


def snap_to_grid(lines, grid, max_snap_distance):
    """snapping.py:496-552 on arrays -> ``(line_index, edges, edge_lines[, values])``.

    ``line_index`` float64 ``(n_edge,)``: per edge the line snapped to it, NaN for none (the reference's ``uds["line_index"]``).
    ``edges`` int64 ``(n_snapped,)`` ascending and ``edge_lines``, the winning line of each: the index pair of the reference's
    GeoDataFrame.  With ``values`` in ``lines`` a fourth result, float64 ``(n_edge,)`` or ``(K, n_edge)``: the values of the
    winning lines, NaN for edges without one (the reference's per-column variables).

    Among the rows of one edge the greatest ``length`` wins, the first in row order among equal ones (``groupby.idxmax``)."""
    made, like, values = _snapgrid(lines, grid, max_snap_distance, 1e-12, reduce=True)
    out = (_out(like, made.line_index(like)), _out(like, made.edges(like)), _out(like, made.edge_lines(like)))
    if values is None:
        return out
    gathered = made.values(values.ptr, values.K, like)
    if len(values.shape) == 1:
        gathered = gathered.reshape(made.n_edge)
    return out + (_out(like, gathered),)
