"""
Layered (3-D) overlap regridding: a 2-D grid plus ``top`` and ``bottom`` of every layer in every cell -- the layered
subsurface models the reference's half-written ``StructuredGrid3d`` / ``ExplicitStructuredGrid3d``
(xugrid/regrid/structured.py, regridder.py:88-91) were meant for.

The weight of (target layer lt, target cell j) <- (source layer ls, source cell i) is the 2-D overlap weight of (j, i)
times the vertical overlap ``min(top_s, top_t) - max(bottom_s, bottom_t)`` where that is positive (DESIGN section 25:
NaN bounds and ``top <= bottom`` mean "no such layer here", nothing is assumed about the order of the layers).  The 2-D
weights are the ones ``OverlapRegridder`` / ``RelativeOverlapRegridder`` build for the pair; the 3-D matrix is made from
them on the device (``xr_csr_layered``, csrc/xr_layered.hip) and is a weight matrix like any other: every reducer, the
many-variable apply, ``regrid_adjoint``, autograd and the persistence layer are the inherited ones.

Data is ``(..., n_layer, n_face)`` (``(..., n_layer, ny, nx)`` on a raster), C-contiguous: flat ids ``layer * n_face + face``.
"""
import ctypes
from typing import Union

import numpy as np

from .. import _lib, engine
from .._lib import check
from ..reduce import Method
from ..ugrid2d import Ugrid2d
from .regridder import BaseRegridder, OverlapRegridder, RelativeOverlapRegridder, setup_grid
from .structured import StructuredGrid2d

__all__ = ["LayeredGrid", "LayeredOverlapRegridder", "LayeredRelativeOverlapRegridder", "overlap_1d_nd"]


def _bounds_array(value, name):
    """-> (array as given: numpy float64 or a float64 device array, its shape)"""
    info = engine.device_array_info(value)
    if info is not None:
        if info[2] != np.dtype(np.float64):
            raise TypeError(f"{name}: device arrays must be float64, received {info[2]}")
        return value, tuple(info[1])
    array = np.ascontiguousarray(value, dtype=np.float64)
    return array, array.shape


def _device_pointer(array, keep):
    """The device pointer of ``array``; a numpy array is uploaded once and kept alive in ``keep``."""
    info = engine.device_array_info(array)
    if info is None:
        array = engine.DeviceArray.from_host(array)
        info = engine.device_array_info(array)
    else:
        engine.sync_producer(array)
    keep.append(array)
    return info[0]


class LayeredGrid:
    """
    A 2-D grid (``Ugrid2d``, ``Raster`` or a regridder grid) with ``n_layer`` layers: ``top`` and ``bottom`` of shape
    ``(n_layer, n_face)`` (rasters also ``(n_layer, ny, nx)``), or ``(n_layer,)`` for the same layering in every cell (kept as
    it is, not expanded).  numpy arrays, or float64 arrays on the device (torch / ``__cuda_array_interface__``).  A NaN
    bound, or ``top <= bottom``, says that the layer does not exist in that cell; layers may come in any order.
    """

    layered = True  # (regridder.setup_grid passes such a grid through)

    def __init__(self, grid, top, bottom):
        self.base = setup_grid(grid)
        self.top, top_shape = _bounds_array(top, "top")
        self.bottom, bottom_shape = _bounds_array(bottom, "bottom")
        if len(top_shape) < 1:
            raise ValueError("top must have a leading layer dimension")
        self.n_layer = int(top_shape[0])
        allowed = {(self.n_layer,) + tuple(self.base.shape), (self.n_layer, self.base.size)}
        if top_shape != (self.n_layer,) and top_shape not in allowed:
            raise ValueError(
                f"top: shape {top_shape} does not fit the grid: (n_layer,) or (n_layer, {self.base.size}) expected"
                + (f" or (n_layer, {', '.join(str(n) for n in self.base.shape)})" if self.base.ndim > 1 else "")
            )
        if bottom_shape != top_shape:
            raise ValueError(f"bottom: shape {bottom_shape} differs from the shape of top, {top_shape}")
        self.uniform = len(top_shape) == 1

    @property
    def ndim(self):
        return self.base.ndim + 1

    @property
    def dims(self):
        return ("layer",) + tuple(self.base.dims)

    @property
    def shape(self):
        return (self.n_layer,) + tuple(self.base.shape)

    @property
    def size(self):
        return self.n_layer * self.base.size

    @property
    def coords(self):
        return self.base.coords

    def to_dataset(self, name: str):
        ds = self.base.to_dataset(name)
        ds[name + "_type"] = "Layered" + ds[name + "_type"]
        ds[name + "_top"] = self.top if isinstance(self.top, np.ndarray) else engine.download(self.top)
        ds[name + "_bottom"] = self.bottom if isinstance(self.bottom, np.ndarray) else engine.download(self.bottom)
        return ds

    @staticmethod
    def from_dataset(dataset, name: str, kind: str):
        if kind == "LayeredUnstructuredGrid2d":
            base = setup_grid(Ugrid2d.from_dataset(dataset, name))
        else:
            base = StructuredGrid2d.from_dataset(dataset, name)
        return LayeredGrid(base, np.asarray(dataset[name + "_top"]), np.asarray(dataset[name + "_bottom"]))


def _layered_weights(weights2d, source: LayeredGrid, target: LayeredGrid, relative: bool) -> "engine.DeviceCSR":
    """The 3-D matrix of ``weights2d`` (the device weights of the 2-D pair) and the two layerings."""
    if isinstance(weights2d, engine.DeviceOuter):
        weights2d = weights2d.csr()
    if weights2d.n != target.base.size or weights2d.m != source.base.size:
        raise ValueError(
            f"the 2-D weights are {weights2d.n} x {weights2d.m}, the grids have {target.base.size} and {source.base.size} cells"
        )
    return weights2d.layered(source.top, source.bottom, target.top, target.bottom, relative)


class _Layered:
    """What the two layered regridders add to their 2-D bases: the grids are ``LayeredGrid``s, the weights come from the 2-D
    regridder of the pair.  Everything else -- ``regrid``, ``regrid_adjoint``, ``weights``, ``to_dataset`` / ``from_weights``,
    ``to_file`` / ``from_file``, the reducers -- is inherited."""

    _BASE2D = None
    _RELATIVE = False

    def __init__(self, source: LayeredGrid, target: LayeredGrid, method: Union[str, Method, None] = None):
        for name, grid in (("source", source), ("target", target)):
            if not isinstance(grid, LayeredGrid):
                raise TypeError(f"{name}: LayeredGrid expected, received {type(grid).__name__}")
        self._build(self._BASE2D(source.base, target.base), source, target)
        self._setup_regrid(self._DEFAULT_METHOD if method is None else method)

    def _build(self, regridder2d, source, target):
        self._source, self._target = source, target
        self._weights = None
        self._device_weights = _layered_weights(regridder2d._ensure_device_weights(), source, target, self._RELATIVE)

    def _compute_weights(self, source, target, tolerance=None):  # (the constructor above builds them)
        raise NotImplementedError

    @classmethod
    def from_regridder(cls, regridder2d, top_source, bottom_source, top_target, bottom_target, method=None):
        """Reuse the 2-D weights ``regridder2d`` has built for another layering of the same pair of grids."""
        if not isinstance(regridder2d, cls._BASE2D) or isinstance(regridder2d, _Layered):
            raise TypeError(
                f"{cls.__name__}.from_regridder takes the 2-D weights of a {cls._BASE2D.__name__}, received "
                f"{type(regridder2d).__name__}"
            )
        instance = cls.__new__(cls)
        source = LayeredGrid(regridder2d._source, top_source, bottom_source)
        target = LayeredGrid(regridder2d._target, top_target, bottom_target)
        instance._build(regridder2d, source, target)
        instance._setup_regrid(cls._DEFAULT_METHOD if method is None else method)
        return instance

    @classmethod
    def from_weights(cls, weights, target, method=None):
        return super().from_weights(weights, target, cls._DEFAULT_METHOD if method is None else method)

    @staticmethod
    def _grid_from_dataset(dataset, name):
        kind = dataset[name + "_type"]
        kind = kind if isinstance(kind, str) else str(np.asarray(kind).item())
        if kind.startswith("Layered"):
            return LayeredGrid.from_dataset(dataset, name, kind)
        return BaseRegridder._grid_from_dataset(dataset, name)


class LayeredOverlapRegridder(_Layered, OverlapRegridder):
    """``OverlapRegridder`` between two ``LayeredGrid``s: weights = overlap area x overlap height (a volume); the methods of
    ``OverlapRegridder``."""

    _BASE2D = OverlapRegridder
    _RELATIVE = False
    _DEFAULT_METHOD = "mean"


class LayeredRelativeOverlapRegridder(_Layered, RelativeOverlapRegridder):
    """``RelativeOverlapRegridder`` between two ``LayeredGrid``s: weights = the share of the source voxel (share of the
    source cell's area x share of the source layer's height); ``first_order_conservative`` (default) and ``conductance``."""

    _BASE2D = RelativeOverlapRegridder
    _RELATIVE = True
    _DEFAULT_METHOD = "first_order_conservative"


def _checked(value, name, dtype, ndim):
    info = engine.device_array_info(value)
    if info is None:
        value = np.ascontiguousarray(value, dtype=dtype)
        shape = value.shape
    else:
        if info[2] != np.dtype(dtype):
            raise TypeError(f"{name}: device arrays must be {np.dtype(dtype).name}, received {info[2]}")
        shape = tuple(info[1])
    if len(shape) != ndim or (ndim == 3 and shape[2] != 2):
        raise ValueError(f"{name}: shape {('(n, n_layer, 2)' if ndim == 3 else '(o,)')} expected, received {tuple(shape)}")
    return value, shape


def overlap_1d_nd(source_bounds, target_bounds, source_index, target_index):
    """
    The reference's ``overlap_1d_nd`` (xugrid/regrid/overlap_1d.py:162-245) on the device: ``source_bounds (n, Ls, 2)`` and
    ``target_bounds (m, Lt, 2)`` hold (lower, upper) per column and layer, ``source_index`` / ``target_index`` ``(o,)`` name
    the column pairs.  -> ``(flat_source_index, flat_target_index, overlap)`` with ``column * n_layer + layer`` ids, ordered
    by pair, target layer, source layer -- the reference's arrays where it runs (NaN-free columns of positive thickness
    over a shared extent, one pair per target column), and the rule of DESIGN section 25 for any input: NaN layers, layers
    in any order, any number of pairs.  numpy in, numpy out; with a device array among the inputs the result stays there.
    """
    source_bounds, s_shape = _checked(source_bounds, "source_bounds", np.float64, 3)
    target_bounds, t_shape = _checked(target_bounds, "target_bounds", np.float64, 3)
    source_index, si_shape = _checked(source_index, "source_index", np.int64, 1)
    target_index, ti_shape = _checked(target_index, "target_index", np.int64, 1)
    if si_shape != ti_shape:
        raise ValueError(f"target_index: {ti_shape[0]} pairs, source_index names {si_shape[0]}")
    inputs = (source_bounds, target_bounds, source_index, target_index)
    like = next((a for a in inputs if not isinstance(a, np.ndarray)), None)
    keep = []
    sb, tb, si, ti = (engine.vp(_device_pointer(a, keep)) for a in inputs)
    lib = _lib.load()
    count = ctypes.c_int64()

    def call(capacity, s_out, t_out, w_out):
        check(lib.xr_overlap_1d_nd_dev(sb, s_shape[0], s_shape[1], tb, t_shape[0], t_shape[1], si, ti, si_shape[0], capacity,
                                       engine.vp(s_out), engine.vp(t_out), engine.vp(w_out), ctypes.byref(count)))

    call(0, 0, 0, 0)
    p = count.value
    s_out, s_ptr = engine.empty_like_device(like, (p,), np.int64)
    t_out, t_ptr = engine.empty_like_device(like, (p,), np.int64)
    w_out, w_ptr = engine.empty_like_device(like, (p,), np.float64)
    if p > 0:
        call(p, s_ptr, t_ptr, w_ptr)
    if like is None:
        return (s_out.download().astype(engine.IntDType, copy=False), t_out.download().astype(engine.IntDType, copy=False),
                w_out.download())
    return s_out, t_out, w_out
