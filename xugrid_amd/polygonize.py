"""
Regions of equal face value as polygon rings, traced on the device: ``polygonize`` (xugrid.polygonize,
xugrid/ugrid/polygonize.py).  Kernels in ``csrc/xr_polygonize.hip``; they read the grid's edge topology (``DeviceTopology``)
where it is.

The result is plain arrays in the layout of ``shapely.to_ragged_array`` -- exactly the ``polygons=`` argument of
``burn_vector_geometry`` (INTEGRATION.md has the two lines that make a GeoDataFrame of them; nothing here imports shapely):

* ``coords (n_vertex, 2)`` float64, ``ring_offsets (n_ring + 1)`` int64, ``polygon_offsets (n_polygon + 1)`` int64,
  ``values (n_polygon,)`` float64 and, with ``return_index``, ``face_polygon (n_face,)`` int64: the polygon of every face, -1
  for a NaN face.  Rings are closed (first vertex == last).  No data or all NaN: no polygon, ``coords`` of shape ``(0, 2)``,
  offsets ``[0]``.

Semantics: NaN faces belong to no polygon; a region is a maximal set of faces with ``==`` values joined
through shared edges (not through a node alone); regions are numbered by their smallest face, polygon ``p`` is region ``p``,
``values[p]`` the value of that face.  Every region is ONE polygon: its exterior ring first, then its holes ascending by
leader -- the boundary half-edge of smallest (face, slot), at whose start node every ring also begins.  Where a region touches
itself at a node a ring passes through that node more than once (the reference keeps only the piece of largest bounding box
there and loses area).

The array contract is ``burn.py``'s and ``fill.py``'s: numpy in (float32, float64, int32, int64) -> numpy out; a device array
in (torch tensor on the GPU or ``__cuda_array_interface__``; float64, float32 or int32) -> device arrays of the same kind out,
and nothing of the size of the mesh crosses PCIe.  The input is never modified.
"""
import ctypes

import numpy as np

from . import _lib, engine
from ._lib import check
from .engine import vp

_DTYPE_IDS = {np.dtype(np.float64): _lib.XR_F64, np.dtype(np.float32): _lib.XR_F32, np.dtype(np.int32): _lib.XR_I32}


def _check_shape(shape, n_face):
    if tuple(shape) != (n_face,):
        raise ValueError(f"Cannot polygonize non-face dimensions. Expected only ({n_face},), but received {tuple(shape)}.")


def host_data(data, n_face):
    """Host face data -> float64 ``(n_face,)``; every argument error that needs no device is raised here."""
    a = np.asarray(data)
    _check_shape(a.shape, n_face)
    if a.dtype not in (np.float64, np.float32, np.int32, np.int64):
        raise TypeError(f"data must be float64, float32, int32 or int64, received {a.dtype}")
    out = np.ascontiguousarray(a, dtype=np.float64)
    if a.dtype == np.int64 and a.size:
        # (2^63 rounds to a float64 that no int64 holds: compare in float64 first, cast back only what fits)
        fits = np.abs(out) < 2.0**63
        if not fits.all() or not np.array_equal(out.astype(np.int64), a):
            raise ValueError("int64 data holds values that float64 cannot represent exactly")
    return out


class DevicePolygons(engine.Handle):
    """``xr_polygons``: the result of one call in HBM, with its counts."""

    _destroy = "xr_polygons_destroy"

    def __init__(self, topology, data_ptr, dtype_id):
        handle = ctypes.c_void_p()
        check(_lib.load().xr_polygonize_dev(topology._h, vp(data_ptr), dtype_id, ctypes.byref(handle)))
        self._h = handle
        v = [ctypes.c_int64() for _ in range(6)]
        check(_lib.load().xr_polygons_info(handle, *(ctypes.byref(x) for x in v[:5])))
        check(_lib.load().xr_polygons_readbacks(handle, ctypes.byref(v[5])))
        self.n_polygon, self.n_ring, self.n_vertex, self.n_halfedge, self.label_rounds, self.readbacks = (x.value for x in v)
        self.n_face = topology.n_face

    def shapes(self):
        return (((self.n_vertex, 2), np.float64), ((self.n_ring + 1,), np.int64), ((self.n_polygon + 1,), np.int64),
                ((self.n_polygon,), np.float64), ((self.n_face,), np.int64))

    def copy_to(self, pointers):
        check(_lib.load().xr_polygons_copy_dev(self._h, *(vp(p) for p in pointers)))


def polygonize_device(like, data):
    """-> the ``DevicePolygons`` of ``data`` on the grid ``like`` (counts, ``label_rounds``) and the device array kind of the
    input (None: host data)."""
    get_topology = getattr(like, "device_topology", None)
    if get_topology is None:
        raise TypeError(f"like must be a Ugrid2d, received: {type(like).__name__}")
    n_face = like.n_face
    info = engine.device_array_info(data)
    if info is None:
        keep = host_data(data, n_face)
        dtype_id = _lib.XR_F64
    else:
        _check_shape(info[1], n_face)
        if info[2] not in _DTYPE_IDS:
            raise TypeError(f"data on the device must be float64, float32 or int32, received {info[2]}")
        dtype_id = _DTYPE_IDS[info[2]]
    topology = get_topology()
    if not topology.manifold:
        raise ValueError(f"Cannot polygonize a non-manifold mesh: {topology.n_nonmanifold} edges have more than two faces")
    if info is None:
        keep = engine.DeviceArray.from_host(keep)
        ptr = keep.ptr
    else:
        engine.sync_producer(data)
        ptr = info[0]
    return DevicePolygons(topology, ptr, dtype_id), (data if info is not None else None)


def polygonize(like, data, return_index=False):
    """xugrid.polygonize on arrays -> ``(coords, ring_offsets, polygon_offsets, values[, face_polygon])``: see the module
    docstring."""
    result, device_like = polygonize_device(like, data)
    shapes = result.shapes()
    if not return_index:
        shapes = shapes[:4]
    if device_like is not None:
        made = [engine.empty_like_device(device_like, shape, dtype) for shape, dtype in shapes]
        result.copy_to([ptr for _, ptr in made] + [None] * (5 - len(made)))
        return tuple(out for out, _ in made)
    arrays = [engine.DeviceArray(shape, dtype) for shape, dtype in shapes]
    result.copy_to([a.ptr for a in arrays] + [None] * (5 - len(arrays)))
    return tuple(a.download() for a in arrays)
