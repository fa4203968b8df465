"""
Reading mesh data at points and along lines on the device: ``sel_points`` / ``sel`` / ``intersect_line`` /
``intersect_linestring`` (xugrid/ugrid/ugridbase.py:1125-1506) and ``locate_nearest_node`` / ``_edge`` / ``_face``
(ugridbase.py:1261-1303, ugrid2d.py:1007-1027).  Kernels in ``csrc/xr_sample.hip``; the containment search
(``locate_points``) and the line clipping (``CellTree2d.intersect_edges``) are the grid's existing ones.

The array contract is ``fill.py``'s: ``data`` is ``(..., n)`` and the leading dims are K slices; numpy in -> numpy out; a
device array in (torch tensor on the GPU, ``__cuda_array_interface__``) -> a float64 device array of the same kind, the
data never crossing PCIe (the query points, the indices and the few thousand pieces of a section do).  float32 data is read
as it is; the values come back as float64, as ``regrid`` gives them.  The input is never modified.

Where the reference returns an xarray object with coordinates, the functions here return small named tuples of arrays.
"""
import ctypes
import warnings
from collections import namedtuple

import numpy as np

from . import _lib, engine
from ._lib import XR_F32, XR_F64, check
from .engine import vp
from .fill import resolve_dim

PointSelection = namedtuple("PointSelection", ["values", "index", "x", "y"])
LineSelection = namedtuple("LineSelection", ["values", "face_index", "x", "y", "s"])
BoxSelection = namedtuple("BoxSelection", ["values", "face_index"])
BoxGridSelection = namedtuple("BoxGridSelection", ["values", "face_index", "grid"])

FACETS = ("node", "edge", "face")
_MESH_FACET_IDS = {"node": 0, "face": 2}  # include/xugrid_amd.h: XR_FACET_NODE, XR_FACET_FACE


class NearestIndex(engine.Handle):
    """Nearest-neighbour index over a fixed set of points in HBM (include/xugrid_amd.h: xr_nn): the device counterpart
    of the reference's ``scipy.spatial.KDTree`` per facet.  The handle keeps its own copy of the coordinates."""

    _destroy = "xr_nn_destroy"

    def __init__(self, handle):
        self._h = handle
        n, n_cell = ctypes.c_int64(), ctypes.c_int64()
        check(_lib.load().xr_nn_info(handle, ctypes.byref(n), ctypes.byref(n_cell)))
        self.n, self.n_cell = n.value, n_cell.value

    @classmethod
    def from_points(cls, xy):
        """``xy``: float64 ``(n, 2)``, a host array or a device array."""
        info = engine.device_array_info(xy)
        if info is None:
            xy = engine.DeviceArray.from_host(engine._as_xy(xy))
            info = engine.device_array_info(xy)
        else:
            engine.sync_producer(xy)
        ptr, shape, dtype = info
        if len(shape) != 2 or shape[1] != 2 or dtype != np.float64:
            raise ValueError("expected a float64 (n, 2) array of coordinates")
        handle = ctypes.c_void_p()
        check(_lib.load().xr_nn_create_dev(vp(ptr), shape[0], ctypes.byref(handle)))
        return cls(handle)

    @classmethod
    def from_mesh(cls, device_mesh, facet):
        """Over the nodes or the face centroids of a ``DeviceMesh``, read where they are (no host copy)."""
        handle = ctypes.c_void_p()
        check(_lib.load().xr_nn_create_mesh(device_mesh._h, _MESH_FACET_IDS[facet], ctypes.byref(handle)))
        return cls(handle)

    def query(self, points, max_distance=np.inf):
        """Id of the nearest indexed point per query point ``(n_point, 2)``, -1 for none: strictly closer than
        ``max_distance``, the lowest id among equidistant points, -1 for a NaN query.  Host points -> numpy integers;
        device points -> an int64 device array of the same kind."""
        max_distance = np.inf if max_distance is None else float(max_distance)
        if not max_distance >= 0.0:
            raise ValueError("max_distance must be non-negative")
        info = engine.device_array_info(points)
        if info is not None:
            ptr, shape, dtype = info
            if len(shape) != 2 or shape[1] != 2 or dtype != np.float64:
                raise ValueError("expected a float64 (n_point, 2) array of points")
            engine.sync_producer(points)
            out, out_ptr = engine.empty_like_device(points, (shape[0],), np.int64)
            check(_lib.load().xr_nn_query_dev(self._h, vp(ptr), shape[0], max_distance, vp(out_ptr)))
            return out
        pts = engine._as_xy(points)
        src = engine.DeviceArray.from_host(pts)
        dst = engine.DeviceArray((pts.shape[0],), np.int64)
        check(_lib.load().xr_nn_query_dev(self._h, vp(src.ptr), pts.shape[0], max_distance, vp(dst.ptr)))
        return dst.download().astype(engine.IntDType, copy=False)


class GridSample:
    """The nearest-neighbour indices of one grid, one per facet, built on first use and kept."""

    def __init__(self):
        self.indices = {}

    def index(self, facet, make):
        if facet not in self.indices:
            self.indices[facet] = make()
        return self.indices[facet]


def _as_data(data, n):
    """-> (kind, array, dtype id, K, shape): 'device' (a contiguous float64 / float32 device array) or 'host' (numpy)."""
    info = engine.device_array_info(data)
    if info is not None:
        ptr, shape, dtype = info
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            if not engine.is_torch(data):
                raise TypeError(f"device data must be float64 or float32, received {dtype}")
            data = data.double()
            ptr, shape, dtype = engine.device_array_info(data)
        kind, a = "device", data
    else:
        a = np.asarray(data)
        if a.dtype != np.float32:
            a = a.astype(np.float64, copy=False)
        a = np.ascontiguousarray(a)
        kind, shape, dtype = "host", a.shape, a.dtype
    if len(shape) == 0 or shape[-1] != n:
        raise ValueError(f"expected data of shape (..., {n}), received: {tuple(shape)}")
    K = int(np.prod(shape[:-1], dtype=np.int64))
    return kind, a, (XR_F32 if dtype == np.float32 else XR_F64), K, tuple(shape)


def gather_points(data, n, index, fill_value=np.nan):
    """``out[..., p] = data[..., index[p]]``, ``fill_value`` where ``index[p] < 0`` (include/xugrid_amd.h:
    xr_gather_points_dev).  ``index``: integers ``(n_point,)`` on the host or an int64 device array; an index ``>= n``
    raises.  The result is of ``data``'s kind."""
    kind, a, dtype_id, K, shape = _as_data(data, n)
    idx_info = engine.device_array_info(index)
    if idx_info is None:
        keep = engine.DeviceArray.from_host(np.ascontiguousarray(index, dtype=np.int64).reshape(-1))
        idx_ptr, n_point = keep.ptr, keep.shape[0]
    else:
        idx_ptr, idx_shape, idx_dtype = idx_info
        if len(idx_shape) != 1 or idx_dtype != np.int64:
            raise ValueError("a device index must be a 1-D int64 array")
        engine.sync_producer(index)
        n_point = idx_shape[0]
    out_shape = shape[:-1] + (n_point,)
    fill_value = float(fill_value)
    if kind == "device":
        engine.sync_producer(a)
        out, out_ptr = engine.empty_like_device(a, out_shape)
        check(_lib.load().xr_gather_points_dev(vp(engine.device_array_info(a)[0]), dtype_id, K, n, vp(idx_ptr), n_point,
                                               fill_value, vp(out_ptr)))
        return out
    src = engine.DeviceArray.from_host(a)
    dst = engine.DeviceArray(out_shape)
    check(_lib.load().xr_gather_points_dev(vp(src.ptr), dtype_id, K, n, vp(idx_ptr), n_point, fill_value, vp(dst.ptr)))
    return dst.download()


def section_arrays(pieces, piece_segment, segments, like=None):
    """Midpoints ``(n, 2)`` and distance along the line ``s (n,)`` of the pieces ``(n, 2, 2)`` cut from the line's
    ``segments (m, 2, 2)`` (``piece_segment``: the segment of each piece), computed on the device
    (include/xugrid_amd.h: xr_section_coords_dev).  Host arrays in; numpy out, or torch tensors on ``like``'s device."""
    pieces = np.ascontiguousarray(pieces, dtype=np.float64).reshape(-1, 2, 2)
    seg_of = np.ascontiguousarray(piece_segment, dtype=np.int64).reshape(-1)
    segments = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 2, 2)
    n = pieces.shape[0]
    if seg_of.shape[0] != n:
        raise ValueError("one segment id per piece expected")
    d_pieces, d_seg_of, d_segments = (engine.DeviceArray.from_host(a) for a in (pieces, seg_of, segments))
    if like is not None and engine.is_torch(like):
        mid, mid_ptr = engine.empty_like_device(like, (n, 2))
        s, s_ptr = engine.empty_like_device(like, (n,))
    else:
        mid, s = engine.DeviceArray((n, 2)), engine.DeviceArray((n,))
        mid_ptr, s_ptr = mid.ptr, s.ptr
    check(_lib.load().xr_section_coords_dev(vp(d_pieces.ptr), vp(d_seg_of.ptr), n, vp(d_segments.ptr), segments.shape[0],
                                            vp(mid_ptr), vp(s_ptr)))
    if isinstance(mid, engine.DeviceArray):
        return mid.download(), s.download()
    return mid, s


# ---- the grid methods (Ugrid2d delegates here) --------------------------------------------------------------------------------
def _scalar_fill(fill_value):
    if callable(fill_value) or np.ndim(fill_value) != 0:
        raise TypeError("fill_value must be a scalar (callables and arrays are not supported)")
    return float(fill_value)


def sel_points(grid, data, x, y, dim=None, method=None, out_of_bounds="warn", fill_value=np.nan, tolerance=None):
    """ugridbase.py:1125-1259 on arrays: see ``Ugrid2d.sel_points``."""
    method_options = (None, "nearest")
    if method not in method_options:
        raise ValueError(f"method must be one of {method_options}, received: {method}")
    bounds_options = ("warn", "raise", "ignore", "drop")
    if out_of_bounds not in bounds_options:
        raise ValueError(f"out_of_bounds must be one of {', '.join(bounds_options)}, received: {out_of_bounds}")
    fill_value = _scalar_fill(fill_value)
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    y = np.atleast_1d(np.asarray(y, dtype=np.float64))
    if x.shape != y.shape:
        raise ValueError("shape of x does not match shape of y")
    if x.ndim != 1:
        raise ValueError("x and y must be 1d")
    facet = resolve_dim(grid, dim, FACETS)
    xy = np.column_stack([x, y])

    # containment decides which points are in bounds, whatever the data's facet
    core = np.asarray(grid.locate_points(xy, tolerance))
    valid = core != -1
    kept = np.arange(x.size, dtype=engine.IntDType)
    mask_invalid = False
    if not valid.all():
        msg = "Not all points are located on the topology."
        if out_of_bounds == "raise":
            raise ValueError(msg)
        if out_of_bounds == "drop":
            core, xy, kept = core[valid], xy[valid], kept[valid]
        else:
            if out_of_bounds == "warn":
                warnings.warn(msg, UserWarning, stacklevel=3)
            mask_invalid = True
    if facet == "face" and method is None:
        indexer = core
    else:
        indexer = np.asarray(grid._locate_nearest(facet, xy))
        if mask_invalid:
            indexer = np.where(valid, indexer, -1)
    values = gather_points(data, getattr(grid, f"n_{facet}"), indexer, fill_value)
    return PointSelection(values, kept, xy[:, 0].copy(), xy[:, 1].copy())


def _as_linestring(xy):
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 2:
        raise ValueError(f"expected an (n_vertex, 2) array of at least two vertices, received shape {xy.shape}")
    return np.stack((xy[:-1], xy[1:]), axis=1)


def _section(grid, data, segments):
    """The faces ``segments (m, 2, 2)`` cross, ordered by the distance along the line."""
    segment_index, face_index, pieces = grid.intersect_edges(segments)
    mid, s = section_arrays(pieces, segment_index, segments, like=data)
    if isinstance(s, np.ndarray):
        order = np.argsort(s, kind="stable")
        face_index, mid, s = np.asarray(face_index)[order], mid[order], s[order]
    else:  # (torch data: the section stays on its device)
        import torch

        s, order = torch.sort(s, stable=True)
        face_index = torch.as_tensor(np.ascontiguousarray(face_index, dtype=np.int64), device=s.device)[order]
        mid = mid[order]
    values = gather_points(data, grid.n_face, face_index)
    return LineSelection(values, face_index, mid[:, 0], mid[:, 1], s)


def intersect_line(grid, data, start, end):
    if (len(start) != 2) or (len(end) != 2):
        raise ValueError("Start and end coordinate pairs must have length two")
    return _section(grid, data, np.array([[start, end]], dtype=np.float64))


def intersect_linestring(grid, data, xy):
    return _section(grid, data, _as_linestring(xy))


def locate_bounding_box(grid, xmin, ymin, xmax, ymax):
    c = grid.centroids
    return np.nonzero((c[:, 0] >= xmin) & (c[:, 0] < xmax) & (c[:, 1] >= ymin) & (c[:, 1] < ymax))[0]


def validate_indexer(indexer):
    """ugrid2d.py:1290-1320: a slice (with a step: the points it enumerates) or a 1-D array of coordinates."""
    if isinstance(indexer, slice):
        s = indexer
        if s.start is not None and s.stop is not None:
            if s.start >= s.stop:
                raise ValueError(f"slice stop should be larger than slice start, received: start: {s.start}, stop: {s.stop}")
            if s.step is not None:
                indexer = np.arange(s.start, s.stop, s.step)
        elif s.step is not None:
            raise ValueError("step should be None if slice start or stop is None")
        return indexer
    if not isinstance(indexer, (list, np.ndarray, int, float, np.integer, np.floating)):
        raise TypeError(
            f"Invalid indexer type: {type(indexer).__name__}, allowed types: integer, float, list, numpy array"
        )
    indexer = np.atleast_1d(indexer)
    if indexer.ndim > 1:
        raise ValueError("index should be 0d or 1d")
    return indexer


def sel_kind(x, y):
    """Which selection a pair of validated indexers asks for (ugridbase.py:1492-1505): 'box', 'yline' (x a slice, y one
    value), 'xline' or 'points'."""
    xs, ys = isinstance(x, slice), isinstance(y, slice)
    if xs and ys:
        return "box"
    if xs and isinstance(y, np.ndarray):
        return "yline"
    if isinstance(x, np.ndarray) and ys:
        return "xline"
    if isinstance(x, np.ndarray) and isinstance(y, np.ndarray):
        return "points"
    raise TypeError(f"Invalid indexer types: {type(x).__name__}, and {type(y).__name__}")


def _bound(value, default):
    return default if value is None else value


def sel(grid, data, x=None, y=None, dim=None, return_grid=False):
    """ugridbase.py:1462-1506 on arrays: see ``Ugrid2d.sel``."""
    x = validate_indexer(slice(None, None) if x is None else x)
    y = validate_indexer(slice(None, None) if y is None else y)
    kind = sel_kind(x, y)
    if return_grid and kind != "box":
        raise ValueError("return_grid needs a box selection (two slices without step): points and lines select no sub-grid")
    if kind == "points":
        yy, xx = (a.ravel() for a in np.meshgrid(y, x, indexing="ij"))
        return sel_points(grid, data, xx, yy, dim=dim)
    if resolve_dim(grid, dim, FACETS) != "face":
        raise ValueError("line and box selections take data on the faces")
    if kind == "yline":
        if y.size != 1:
            raise ValueError("If x is a slice without steps, y should be a single value")
        xmin, _, xmax, _ = grid.bounds
        return intersect_line(grid, data, (_bound(x.start, xmin), y[0]), (_bound(x.stop, xmax), y[0]))
    if kind == "xline":
        if x.size != 1:
            raise ValueError("If y is a slice without steps, x should be a single value")
        _, ymin, _, ymax = grid.bounds
        return intersect_line(grid, data, (x[0], _bound(y.start, ymin)), (x[0], _bound(y.stop, ymax)))
    xmin, ymin, xmax, ymax = grid.bounds
    face_index = grid.locate_bounding_box(_bound(x.start, xmin), _bound(y.start, ymin), _bound(x.stop, xmax),
                                          _bound(y.stop, ymax))
    values = gather_points(data, grid.n_face, face_index)
    if return_grid:  # (the face index alone: no edge topology is built for it)
        return BoxGridSelection(values, face_index, grid.topology_subset(face_index))
    return BoxSelection(values, face_index)
