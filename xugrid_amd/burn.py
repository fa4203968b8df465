"""
Writing vector geometry into the faces of a mesh on the device: ``burn_vector_geometry`` and ``_locate_polygon``
(xugrid/ugrid/burn.py:57-262).  Kernels in ``csrc/xr_burn.hip``; lines and ``all_touched`` reuse the segment clipper of
``CellTree2d.intersect_edges``, points the containment search of ``locate_points``.

Geometry comes in as plain arrays, in the layout ``shapely.to_ragged_array`` produces (INTEGRATION.md has the few lines that
turn a GeoDataFrame into them; nothing here imports shapely):

* ``polygons = (coords (n, 2), ring_offsets (n_ring + 1), polygon_offsets (n_polygon + 1)[, values (n_polygon)])``: the first
  ring of a polygon is its exterior, the others are holes; rings are cyclic, so closed (first == last) and open rings
  both work;
* ``lines = (coords, line_offsets (n_line + 1)[, values (n_line)])``: a segment joins consecutive vertices of one line;
* ``points = (coords[, values (n_point)])``.

Missing values mean 1.0 (the reference's ``column=None``).  The array contract is ``fill.py``'s and ``sample.py``'s: numpy in
-> numpy out; if any coordinate array is a device array (a torch tensor on the GPU, ``__cuda_array_interface__``) the result
is a float64 device array of that kind and neither coordinates nor result cross PCIe.  Inputs are never modified.

Semantics: a face is in a polygon iff its centroid passes the point-in-face rule of ``locate_points``
(within the mesh's default tolerance of a segment, or an odd crossing number) over ALL ring segments of the polygon;
``all_touched`` adds the faces in which a ring segment has a piece of positive length.  Polygons, then lines, then points;
within a kind the highest index wins, as in the reference's sequential loop.  A point outside the mesh burns nothing.
"""
import numpy as np

from . import _lib, engine
from ._lib import check
from .engine import vp


class _Arg:
    """One input array on the device: ``ptr``, ``shape``; ``keep`` holds what must outlive the calls; ``device`` is the
    caller's own array if it came as a device array."""

    def __init__(self, array, dtype, what, ndim):
        info = engine.device_array_info(array)
        self.device = None
        if info is not None:
            ptr, shape, got = info
            if got != np.dtype(dtype):
                if not engine.is_torch(array):
                    raise TypeError(f"{what} on the device must be {np.dtype(dtype).name}, received {got}")
                import torch

                array = array.to(getattr(torch, np.dtype(dtype).name))
                ptr, shape, got = engine.device_array_info(array)
            engine.sync_producer(array)
            self.device, self.keep, self._ptr, self.shape, self.host = array, array, ptr, tuple(shape), None
        else:
            a = np.asarray(array)
            if np.dtype(dtype).kind == "i" and a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{what} must be integers, received {a.dtype}")
            a = np.ascontiguousarray(a, dtype=dtype)
            self.host, self.shape, self.keep = a, a.shape, None  # (uploaded on first use: validation comes first)
        if len(self.shape) != ndim or (ndim == 2 and self.shape[1] != 2):
            expected = "(n, 2)" if ndim == 2 else "(n,)"
            raise ValueError(f"{what}: expected an array of shape {expected}, received shape {self.shape}")
        self.n = self.shape[0]

    @property
    def ptr(self):
        if self.keep is None:
            self.keep = engine.DeviceArray.from_host(self.host)
            self._ptr = self.keep.ptr
        return self._ptr


def _coords(array, what):
    arg = _Arg(array, np.float64, f"{what} coordinates", 2)
    if arg.host is not None and not np.isfinite(arg.host).all():
        raise ValueError(f"{what} coordinates must be finite")
    return arg


def _offsets(array, what, total):
    """Offsets into ``total`` items: start at 0, end at ``total``, never decrease (host arrays are checked here, device
    arrays by the library before anything is read through them)."""
    arg = _Arg(array, np.int64, what, 1)
    if arg.n < 1:
        raise ValueError(f"{what} must hold at least one entry (a single 0 for no geometry)")
    if arg.host is not None:
        o = arg.host
        if o[0] != 0 or o[-1] != total or (np.diff(o) < 0).any():
            raise ValueError(f"{what} must start at 0, end at {total} and never decrease")
    return arg


def _values(parts, n_fixed, count, what):
    if len(parts) == n_fixed:
        return None
    arg = _Arg(parts[n_fixed], np.float64, f"{what} values", 1)
    if arg.n != count:
        raise ValueError(f"{what}: {arg.n} values for {count} geometries")
    return arg


def _parts(parts, n_fixed, what):
    if isinstance(parts, np.ndarray) or engine.device_array_info(parts) is not None:
        parts = (parts,)
    parts = tuple(parts)
    if not n_fixed <= len(parts) <= n_fixed + 1:
        raise ValueError(f"{what}: expected {n_fixed} arrays and optionally the values, received {len(parts)}")
    return parts


def _mesh(like):
    mesh = getattr(like, "device_mesh", None)
    if mesh is None:
        raise TypeError(f"like must be a Ugrid2d, received: {type(like).__name__}")
    return mesh


def _polygon_args(polygons):
    parts = _parts(polygons, 3, "polygons")
    coords = _coords(parts[0], "polygon")
    ring_offsets = _offsets(parts[1], "ring_offsets", coords.n)
    polygon_offsets = _offsets(parts[2], "polygon_offsets", ring_offsets.n - 1)
    return coords, ring_offsets, polygon_offsets, _values(parts, 3, polygon_offsets.n - 1, "polygons")


def _polygon_winner(mesh, coords, ring_offsets, polygon_offsets, all_touched, winner_ptr):
    check(_lib.load().xr_burn_polygons_dev(mesh._h, vp(coords.ptr), coords.n, vp(ring_offsets.ptr), ring_offsets.n - 1,
                                           vp(polygon_offsets.ptr), polygon_offsets.n - 1, int(bool(all_touched)),
                                           vp(winner_ptr)))


def polygon_winner(like, coords, ring_offsets, polygon_offsets, all_touched=False):
    """Per face the highest index of a polygon that covers it, -1 for none (include/xugrid_amd.h: xr_burn_polygons_dev):
    what ``burn_vector_geometry`` looks the polygon values up with.  Host arrays -> numpy integers; device coordinates ->
    an int32 device array of their kind."""
    mesh = _mesh(like)
    coords, ring_offsets, polygon_offsets, _ = _polygon_args((coords, ring_offsets, polygon_offsets))
    if coords.device is not None:
        out, out_ptr = engine.empty_like_device(coords.device, (like.n_face,), np.int32)
        _polygon_winner(mesh, coords, ring_offsets, polygon_offsets, all_touched, out_ptr)
        return out
    out = engine.DeviceArray((like.n_face,), np.int32)
    _polygon_winner(mesh, coords, ring_offsets, polygon_offsets, all_touched, out.ptr)
    return out.download().astype(engine.IntDType)


def locate_polygon(like, exterior, interiors=(), all_touched=False):
    """The reference's ``_locate_polygon`` (burn.py:59-112): the sorted indices of the faces one polygon covers.
    ``exterior`` and every entry of ``interiors`` are ``(n, 2)`` host arrays of ring vertices, closed or open."""
    rings = [np.asarray(exterior, dtype=np.float64).reshape(-1, 2)]
    rings += [np.asarray(ring, dtype=np.float64).reshape(-1, 2) for ring in interiors]
    ring_offsets = np.concatenate(([0], np.cumsum([len(ring) for ring in rings]))).astype(np.int64)
    winner = polygon_winner(like, np.concatenate(rings), ring_offsets, np.array([0, len(rings)], dtype=np.int64), all_touched)
    return np.nonzero(winner >= 0)[0].astype(engine.IntDType)


def burn_vector_geometry(like, *, polygons=None, lines=None, points=None, fill=np.nan, all_touched=False):
    """xugrid.burn_vector_geometry (burn.py:184-262) on arrays -> float64 ``(n_face,)``: see the module docstring."""
    mesh = _mesh(like)
    n_face = like.n_face
    fill = float(fill)
    # every argument is checked before the first launch
    v_polygon = v_line = v_point = None
    coordinate_arrays = []
    if polygons is not None:
        polygon_xy, ring_offsets, polygon_offsets, v_polygon = _polygon_args(polygons)
        coordinate_arrays.append(polygon_xy)
    if lines is not None:
        parts = _parts(lines, 2, "lines")
        line_xy = _coords(parts[0], "line")
        line_offsets = _offsets(parts[1], "line_offsets", line_xy.n)
        v_line = _values(parts, 2, line_offsets.n - 1, "lines")
        coordinate_arrays.append(line_xy)
    if points is not None:
        parts = _parts(points, 1, "points")
        point_xy = _coords(parts[0], "point")
        v_point = _values(parts, 1, point_xy.n, "points")
        coordinate_arrays.append(point_xy)
    device_like = next((a.device for a in coordinate_arrays if a.device is not None), None)

    lib = _lib.load()
    w_polygon = w_line = w_point = None  # (no geometry of a kind: no launch of that kind)
    if polygons is not None and polygon_offsets.n - 1 > 0 and n_face > 0:
        w_polygon = engine.DeviceArray((n_face,), np.int32)
        _polygon_winner(mesh, polygon_xy, ring_offsets, polygon_offsets, all_touched, w_polygon.ptr)
    if lines is not None and line_offsets.n - 1 > 0 and n_face > 0:
        w_line = engine.DeviceArray((n_face,), np.int32)
        check(lib.xr_burn_lines_dev(mesh._h, vp(line_xy.ptr), line_xy.n, vp(line_offsets.ptr), line_offsets.n - 1,
                                    vp(w_line.ptr)))
    if points is not None and point_xy.n > 0 and n_face > 0:
        w_point = engine.DeviceArray((n_face,), np.int32)
        check(lib.xr_burn_points_dev(mesh._h, vp(point_xy.ptr), point_xy.n, vp(w_point.ptr)))

    def ptr(arg):
        return vp(arg.ptr) if arg is not None else None

    def combine(out_ptr):
        check(lib.xr_burn_combine_dev(n_face, ptr(w_polygon), ptr(v_polygon), ptr(w_line), ptr(v_line), ptr(w_point),
                                      ptr(v_point), fill, vp(out_ptr)))

    if device_like is not None:
        out, out_ptr = engine.empty_like_device(device_like, (n_face,))
        combine(out_ptr)
        return out
    out = engine.DeviceArray((n_face,))
    combine(out.ptr)
    return out.download()
