"""
Meshes from cell geometry, built on the device: sorted unique coordinate rows (``np.unique(axis=0)``), CF cell bounds
``(N, M, 4)`` (``conversion.bounds2d_to_topology2d``, xugrid/conversion.py:297-354), curvilinear lattices from intervals or
centres (``infer_interval_breaks`` :171-199, ``Ugrid2d.from_structured_intervals2d`` / ``from_structured``), polygons and
lines as coordinate arrays (``polygons_to_faces`` :82-117, ``linestrings_to_edges`` :70-79) and the way back.  Kernels in
``csrc/xr_geometry.hip``; DESIGN section 24.

Inputs are host numpy arrays or device arrays (torch tensors on the GPU, ``__cuda_array_interface__``, ``DeviceArray``); with
device inputs nothing of mesh size crosses PCIe -- counts and problem words do.  Grids come back device-resident
(``DeviceUgrid2d.from_device_mesh``), networks as the host ``Ugrid1d`` that ``netedit.py`` returns.  Plain arrays follow the
kind rule of ``polygonize``: numpy in -> numpy out, a device array in -> device arrays of its kind.

Polygons are ``(coords (V, 2), ring_offsets)`` or the ``(coords, ring_offsets, polygon_offsets[, values])`` tuple that
``polygonize`` returns and ``burn_vector_geometry`` takes; lines are ``(coords (V, 2), line_offsets)``.
"""
import ctypes
import warnings

import numpy as np

from . import _lib, engine
from ._lib import check
from .engine import DeviceMesh, vp
from .inkind import int64_dev, xy_dev

NOT_MONOTONIC = "The input coordinate is not monotonic."
INVALID_FACES = ("A UGRID2D face requires at least three unique non-collinear vertices.\n"
                 "Your structured bounds contain {} invalid faces.\n"
                 "These will be omitted from the Ugrid2d topology.")


def _like(values):
    """The device array the results take their kind from, None for host input."""
    return values if not isinstance(values, (list, tuple)) and engine.device_array_info(values) is not None else None


def _emit(outputs, like):
    """Device arrays as the caller gets them: as they are for device input, downloaded for host input."""
    return [a if like is not None else engine.download(a) for a in outputs]


def _grid(handle, name):
    from .ugrid2d import DeviceUgrid2d

    return DeviceUgrid2d.from_device_mesh(DeviceMesh._from_handle(handle), name)


def _nonfinite(count, what):
    if count:
        raise ValueError(f"{what} hold {count} row(s) with a NaN or infinite coordinate")


# ---- sorted unique rows ---------------------------------------------------------------------------------------------------------
class DeviceUnique(engine.CopyHandle):
    """``xr_unique_xy``: the sorted unique rows of one coordinate array in HBM, with its counts."""

    _destroy = "xr_unique_xy_destroy"
    _copy_dev = "xr_unique_xy_copy_dev"
    XY, INDEX, INVERSE = 0, 1, 2

    def __init__(self, handle):
        self._h = handle
        sizes = (ctypes.c_int64 * 5)()
        check(_lib.load().xr_unique_xy_info(handle, sizes))
        self.n, self.n_unique, self.n_nonfinite, self.passes_run, self.passes_skipped = (int(v) for v in sizes)

    @classmethod
    def of(cls, ptr, n):
        handle = ctypes.c_void_p()
        check(_lib.load().xr_unique_xy_dev(vp(ptr), int(n), ctypes.byref(handle)))
        return cls(handle)

    def xy(self, like=None):
        return self._copy(self.XY, (self.n_unique, 2), np.float64, like)

    def index(self, like=None):
        return self._copy(self.INDEX, (self.n_unique,), np.int64, like)

    def inverse(self, like=None):
        return self._copy(self.INVERSE, (self.n,), np.int64, like)


def _rows(xy, what):
    keep, ptr, shape = xy_dev(xy, what)
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"expected an (n, 2) array of coordinates, received shape {tuple(shape)}")
    return keep, ptr, int(shape[0])


def unique_xy(xy, return_index=False, return_inverse=False):
    """``np.unique(xy, axis=0, return_index=..., return_inverse=...)`` for float64 rows ``(n, 2)``: two rows are one when both
    coordinates compare ``==`` (so ``-0.0 == 0.0``), the kept bits are those of the first occurrence, the unique rows ascend by
    ``x``, then ``y``.  A NaN or infinite coordinate raises ``ValueError``."""
    keep, ptr, n = _rows(xy, "xy")
    like = _like(xy)
    unique = DeviceUnique.of(ptr, n)
    _nonfinite(unique.n_nonfinite, "xy")
    out = [unique.xy(like)]
    if return_index:
        out.append(unique.index(like))
    if return_inverse:
        out.append(unique.inverse(like))
    out = _emit(out, like)
    return out[0] if len(out) == 1 else tuple(out)


# ---- (N, M, 4) bounds -----------------------------------------------------------------------------------------------------------
def bounds_mesh(x_bounds, y_bounds, name="mesh2d"):
    """-> (grid, index, counts): the device grid of ``(N, M, 4)`` bounds, the bool ``(N * M,)`` device array of the cells that
    became faces (a torch tensor for torch bounds, else a ``DeviceArray``) and ``xr_mesh_from_bounds_dev``'s four counts."""
    x_keep, x_ptr, x_shape = xy_dev(x_bounds, "bounds")
    y_keep, y_ptr, y_shape = xy_dev(y_bounds, "bounds")
    if tuple(x_shape) != tuple(y_shape):
        raise ValueError(f"Bounds shapes do not match: {tuple(x_shape)} versus {tuple(y_shape)}")
    if len(x_shape) != 3 or x_shape[2] != 4:
        raise ValueError(f"Expected (N, M, 4) bounds, received shape {tuple(x_shape)}")
    like = _like(x_bounds)
    n_cell = int(x_shape[0]) * int(x_shape[1])
    if engine.is_torch(like):
        import torch

        index = torch.empty((n_cell,), dtype=torch.uint8, device=like.device)
        index_ptr = int(index.data_ptr())
    else:
        index = engine.DeviceArray((n_cell,), np.bool_)  # (the kernel writes bytes 0 / 1)
        index_ptr = index.ptr
    handle, counts = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
    check(_lib.load().xr_mesh_from_bounds_dev(vp(x_ptr), vp(y_ptr), n_cell, ctypes.byref(handle), vp(index_ptr), counts))
    return _grid(handle, name), (index.bool() if engine.is_torch(like) else index), [int(v) for v in counts]


def from_bounds(x_bounds, y_bounds, name="mesh2d", return_index=False):
    """See ``Ugrid2d.from_structured_bounds`` with ``(N, M, 4)`` bounds."""
    grid, index, counts = bounds_mesh(x_bounds, y_bounds, name)
    if counts[1]:
        warnings.warn(INVALID_FACES.format(counts[1]), UserWarning, stacklevel=3)
    if not return_index:
        return grid
    return grid, (index if _like(x_bounds) is not None else index.download())


# ---- lattices -------------------------------------------------------------------------------------------------------------------
def _coord2d(values, what):
    keep, ptr, shape = xy_dev(values, what)
    return keep, ptr, tuple(int(n) for n in shape)


def interval_breaks(coord, axis=0, check_monotonic=False):
    """``conversion.infer_interval_breaks`` on a 1-D or 2-D float64 array, host or device -> a ``DeviceArray`` with one more
    element along ``axis``."""
    keep, ptr, shape = _coord2d(coord, "coord")
    if len(shape) not in (1, 2) or axis not in range(len(shape)):
        raise ValueError(f"coord must be 1-D or 2-D with axis inside it, received shape {shape} and axis {axis}")
    if 0 in shape:
        raise ValueError("coord must not be empty")
    rows, cols = (shape[0], 1) if len(shape) == 1 else shape
    out_shape = tuple(n + (k == axis) for k, n in enumerate(shape))
    out = engine.DeviceArray(out_shape, np.float64)
    problems = (ctypes.c_int64 * 2)()
    check(_lib.load().xr_interval_breaks_dev(vp(ptr), rows, cols, 0 if len(shape) == 1 else axis, vp(out.ptr), problems))
    if check_monotonic and problems[0] and problems[1]:
        raise ValueError(NOT_MONOTONIC)
    return out


def from_intervals2d(x_intervals, y_intervals, name="mesh2d"):
    """See ``Ugrid2d.from_structured_intervals2d``."""
    x_keep, x_ptr, x_shape = _coord2d(x_intervals, "intervals")
    y_keep, y_ptr, y_shape = _coord2d(y_intervals, "intervals")
    if len(x_shape) != 2 or len(y_shape) != 2:
        raise ValueError("Dimensions of intervals must be 2D.")
    if x_shape != y_shape:
        raise ValueError(f"Interval shapes must match. Found: x_intervals: {x_shape}, versus y_intervals: {y_shape}")
    ny, nx = x_shape[0] - 1, x_shape[1] - 1
    if ny < 1 or nx < 1:
        raise ValueError(f"intervals must hold at least one cell per axis, received shape {x_shape}")
    handle = ctypes.c_void_p()
    check(_lib.load().xr_mesh_from_intervals_dev(vp(x_ptr), vp(y_ptr), ny, nx, ctypes.byref(handle)))
    return _grid(handle, name)


def _host1d(values, what):
    a = engine.download(values) if engine.device_array_info(values) is not None else np.asarray(values, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{what} must be 1-D, received shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float64)


def from_intervals1d(x_intervals, y_intervals, name="mesh2d"):
    """See ``Ugrid2d.from_structured_intervals1d``: the rectilinear device mesh of the two vertex arrays (axis-sized)."""
    from .ugrid2d import RectilinearUgrid2d

    return RectilinearUgrid2d(_host1d(x_intervals, "x_intervals"), _host1d(y_intervals, "y_intervals"), name)


def _ndim(values):
    info = None if isinstance(values, (list, tuple)) else engine.device_array_info(values)
    return len(info[1]) if info is not None else np.ndim(values)


def from_structured(x, y, name="mesh2d"):
    """See ``Ugrid2d.from_structured``."""
    ndim = _ndim(x)
    if ndim == 1:
        for axis_name, coord in (("x", x), ("y", y)):
            if _host1d(coord, axis_name).size == 1:
                raise ValueError(f"Cannot derive spacing of 1-sized coordinate: {axis_name} \n"
                                 f"Assign a d{axis_name} variable with spacing instead.")
        xv = interval_breaks(x, 0, check_monotonic=True).download()
        yv = interval_breaks(y, 0, check_monotonic=True).download()
        return from_intervals1d(xv, yv, name)
    if ndim != 2:
        raise ValueError(f"x and y must be 1D or 2D. Found: {ndim}")
    if _coord2d(x, "x")[2] != _coord2d(y, "y")[2]:
        raise ValueError(f"x and y must have the same shape, received {_coord2d(x, 'x')[2]} versus {_coord2d(y, 'y')[2]}")
    xv = interval_breaks(interval_breaks(x, 1, check_monotonic=True), 0)
    yv = interval_breaks(interval_breaks(y, 1), 0, check_monotonic=True)
    return from_intervals2d(xv, yv, name)


# ---- polygons and lines -----------------------------------------------------------------------------------------------------------
HOLE = "Cannot make faces of polygons with holes: {} polygon(s) do not hold exactly one ring"
OPEN = "{} ring(s) are not closed: the last vertex must equal the first"
SHORT = "{} ring(s) have fewer than four vertices (a closed triangle has four)"
OFFSETS = "the offsets must ascend from 0 to the number of vertices"


def _offsets(values, what):
    dev, _, n = int64_dev(values, what)
    if n < 1:
        raise ValueError(f"{what} must hold at least one offset")
    return dev, engine.device_array_info(dev)[0], n - 1


def from_polygons(polygons, name="mesh2d"):
    """See ``Ugrid2d.from_polygons``."""
    if not isinstance(polygons, (tuple, list)) or len(polygons) not in (2, 3, 4):
        raise TypeError("polygons must be (coords, ring_offsets) or (coords, ring_offsets, polygon_offsets[, values])")
    keep, ptr, n_vertex = _rows(polygons[0], "coords")
    ring_keep, ring_ptr, n_ring = _offsets(polygons[1], "ring_offsets")
    poly_keep, poly_ptr, n_poly = _offsets(polygons[2], "polygon_offsets") if len(polygons) > 2 else (None, 0, 0)
    handle, problems = ctypes.c_void_p(), (ctypes.c_int64 * 5)()
    check(_lib.load().xr_mesh_from_rings_dev(vp(ptr), n_vertex, vp(ring_ptr), n_ring, vp(poly_ptr), n_poly, ctypes.byref(handle), problems))
    n_short, n_open, n_offsets, n_holes, n_nonfinite = (int(v) for v in problems)
    if n_offsets:
        raise ValueError(OFFSETS)
    for count, message in ((n_holes, HOLE), (n_short, SHORT), (n_open, OPEN)):
        if count:
            raise ValueError(message.format(count))
    _nonfinite(n_nonfinite, "coords")
    return _grid(handle, name)


def to_polygons(grid):
    """See ``Ugrid2d.to_polygons``."""
    mesh = grid.device_mesh
    ring_offsets, polygon_offsets = (engine.DeviceArray((mesh.n_face + 1,), np.int64) for _ in range(2))
    n_vertex = ctypes.c_int64()
    check(_lib.load().xr_mesh_ring_offsets_dev(mesh._h, vp(ring_offsets.ptr), vp(polygon_offsets.ptr), ctypes.byref(n_vertex)))
    coords = engine.DeviceArray((n_vertex.value, 2), np.float64)
    check(_lib.load().xr_mesh_ring_coords_dev(mesh._h, vp(ring_offsets.ptr), n_vertex.value, vp(coords.ptr)))
    out = (coords, ring_offsets, polygon_offsets)
    return out if getattr(grid, "_device_resident", False) else tuple(a.download() for a in out)


def from_lines(lines, name="network1d"):
    """See ``Ugrid1d.from_lines``."""
    from .ugrid1d import FILL_VALUE, Ugrid1d

    if not isinstance(lines, (tuple, list)) or len(lines) != 2:
        raise TypeError("lines must be (coords, line_offsets)")
    keep, ptr, n_vertex = _rows(lines[0], "coords")
    off_keep, off_ptr, n_line = _offsets(lines[1], "line_offsets")
    edges = engine.DeviceArray((max(n_vertex - 1, 0), 2), np.int64)
    handle, counts = ctypes.c_void_p(), (ctypes.c_int64 * 3)()
    check(_lib.load().xr_lines_to_network_dev(vp(ptr), n_vertex, vp(off_ptr), n_line, ctypes.byref(handle), vp(edges.ptr), counts))
    if counts[1]:
        raise ValueError(OFFSETS)
    nodes = DeviceUnique(handle)
    _nonfinite(int(counts[2]), "coords")
    xy = nodes.xy().download()
    return Ugrid1d(xy[:, 0], xy[:, 1], FILL_VALUE, edges.download()[: int(counts[0])], name=name)


def to_lines(grid):
    """See ``Ugrid1d.to_lines``."""
    edges = np.asarray(grid.edge_node_connectivity, dtype=np.int64).reshape(-1, 2)
    return grid.node_coordinates.reshape(-1, 2)[edges.ravel()], np.arange(0, 2 * len(edges) + 1, 2, dtype=np.int64)


def bounding_polygon(grid):
    """See ``Ugrid2d.bounding_polygon``."""
    from .polygonize import polygonize

    coords, ring_offsets, polygon_offsets, _ = (engine.download(a) if not isinstance(a, np.ndarray) else a
                                                for a in polygonize(grid, np.zeros(grid.n_face, dtype=np.float64)))
    if len(polygon_offsets) < 2:
        return np.zeros((0, 2), dtype=np.float64), np.zeros(1, dtype=np.int64)
    best, best_area = 0, -np.inf
    for p in range(len(polygon_offsets) - 1):  # (a handful: the connected parts of the grid)
        first, last = ring_offsets[polygon_offsets[p]], ring_offsets[polygon_offsets[p + 1]]
        xy = coords[first:last]
        area = (xy[:, 0].max() - xy[:, 0].min()) * (xy[:, 1].max() - xy[:, 1].min())
        if area > best_area:
            best, best_area = p, area
    rings = ring_offsets[polygon_offsets[best]: polygon_offsets[best + 1] + 1]
    return coords[rings[0]: rings[-1]].copy(), (rings - rings[0]).astype(np.int64)
