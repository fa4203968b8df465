"""
Snapping points: ``snap_nodes`` (xugrid/ugrid/snapping.py:46-143) and ``snap_to_nodes`` (:146-219) on arrays, and the grid
methods built on them.  Kernels in ``csrc/xr_snap.hip``; DESIGN section 19.  ``snap_to_grid`` and its frame are in ``snapgrid.py``, which snaps the line
vertices through ``grid_snap_to_nodes``'s index.

``x`` and ``y`` (and ``to_x``, ``to_y``) are 1-D coordinate arrays of one length, both on the host or both on the device.  numpy in
-> numpy out; device arrays in (``DeviceArray``, torch tensors on the GPU, ``__cuda_array_interface__``, float64) -> device
arrays of the kind of ``x`` out, and only the few scalars of the call cross PCIe.  The inputs are never modified and no output
aliases them.  "Within the distance" is ``dx * dx + dy * dy <= d * d`` in float64, inclusive, as the reference's KD-tree tests
it.  A NaN or infinite coordinate raises ``ValueError`` ("data must be finite"), as scipy does.
"""
import ctypes

import numpy as np

from . import _lib, engine, sample
from ._lib import check
from .engine import DeviceSnap, vp

BAD_TIEBREAKER = 'Invalid tiebreaker: {}, should be one of {{None, "nearest"}} instead.'
TIES = "Ties detected: multiple options to snap to, given max distance: set a smaller tolerance or specify a tiebreaker."


class _Coords:
    """A pair of 1-D float64 coordinate arrays in HBM: two pointers, their length, and what the outputs should look like
    (``like``: the caller's device array, None for host input)."""

    def __init__(self, x, y, names=("x", "y")):
        infos = [engine.device_array_info(a) for a in (x, y)]
        if (infos[0] is None) != (infos[1] is None):
            raise TypeError(f"{names[0]} and {names[1]} must both be host arrays or both be device arrays")
        if infos[0] is not None:
            for (ptr, shape, dtype), name in zip(infos, names):
                if len(shape) != 1 or dtype != np.float64:
                    raise ValueError(f"device {name} must be a 1-D float64 array")
            if infos[0][1] != infos[1][1]:
                raise ValueError(f"shape of {names[0]} does not match shape of {names[1]}")
            engine.sync_producer(x)
            engine.sync_producer(y)
            self.n, self.like, self.keep = infos[0][1][0], x, (x, y)
            self.x_ptr, self.y_ptr = infos[0][0], infos[1][0]
        else:
            hx, hy = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
            if hx.ndim != 1 or hx.shape != hy.shape:
                raise ValueError(f"{names[0]} and {names[1]} must be 1-D arrays of one length, received shapes {hx.shape} and {hy.shape}")
            self.n, self.like = hx.shape[0], None
            self.keep = engine.DeviceArray.from_host(np.stack((hx, hy))) if self.n else None  # (2, n): one upload
            self.x_ptr = self.keep.ptr if self.n else 0
            self.y_ptr = self.x_ptr + 8 * self.n if self.n else 0
            self.host = (hx, hy)

    @property
    def on_device(self):
        return self.like is not None


def _snap_to(index, coords, max_distance, x_ptr, y_ptr, out_stride, index_ptr=0):
    """include/xugrid_amd.h: xr_nn_snap_dev -> the number of points with more than one candidate."""
    tied = ctypes.c_int64()
    check(_lib.load().xr_nn_snap_dev(index._h if index is not None else None, vp(coords.x_ptr), vp(coords.y_ptr), 1, coords.n,
                                     float(max_distance), vp(x_ptr), vp(y_ptr), out_stride, vp(index_ptr), ctypes.byref(tied)))
    return tied.value


def _pair_out(coords):
    """Fresh x and y outputs of the kind of the input -> (finish() -> (x, y), x pointer, y pointer)."""
    n = coords.n
    if coords.on_device:
        x, x_ptr = engine.empty_like_device(coords.like, (n,))
        y, y_ptr = engine.empty_like_device(coords.like, (n,))
        return (lambda: (x, y)), x_ptr, y_ptr
    both = engine.DeviceArray((2, n))
    return (lambda: tuple(both.download())), both.ptr, both.ptr + 8 * n


def _copies(coords):
    """Copies of coordinates that have been checked already (or are none): host arrays on the host, device arrays by the kernel,
    which copies every point when it is given no index."""
    if not coords.on_device:
        return coords.host[0].copy(), coords.host[1].copy()
    finish, x_ptr, y_ptr = _pair_out(coords)
    if coords.n:
        _snap_to(None, coords, 0.0, x_ptr, y_ptr, 1)
    return finish()


def _merge(coords, max_snap_distance):
    return DeviceSnap(coords.x_ptr, coords.y_ptr, 1, coords.n, max_snap_distance)


def snap_nodes(x, y, max_snap_distance):
    """snapping.py:86-143: nodes within ``max_snap_distance`` of each other are merged.  -> ``(inverse, x_snapped, y_snapped)``:
    ``inverse`` int64 ``(n,)`` is the new number of every old node (``inverse[connectivity]`` renumbers a connectivity), the
    snapped coordinates are those of the kept nodes in ascending old number, bit for bit.  ``inverse`` is None, with copies of
    ``x`` and ``y``, when no two nodes lie within the distance.  Node ``i`` is kept iff no lower-numbered kept node lies within
    the distance; every other node goes to the nearest kept node, the lowest number among equally near ones."""
    coords = _Coords(x, y)
    merged = _merge(coords, max_snap_distance)
    if merged.n_pair == 0:
        return (None,) + _copies(coords)
    if coords.on_device:
        return merged.inverse(coords.like), merged.x(coords.like), merged.y(coords.like)
    xy = merged.xy().download()
    return merged.inverse().download().astype(engine.IntDType, copy=False), xy[:, 0].copy(), xy[:, 1].copy()


def _to_index(to):
    """The nearest index over a pair of coordinate arrays, None for an empty one."""
    if to.n == 0:
        return None
    xy = engine.DeviceArray((to.n, 2))
    _snap_to(None, to, 0.0, xy.ptr, xy.ptr + 8, 2)  # (interleaves, and raises for NaN / infinity before an index is built)
    return sample.NearestIndex.from_points(xy)


def _check_tiebreaker(tiebreaker):
    if tiebreaker not in (None, "nearest"):
        raise ValueError(BAD_TIEBREAKER.format(tiebreaker))


def _snap_onto(index, coords, max_distance, tiebreaker, return_index):
    """``index`` None: an empty set of nodes, every point is copied."""
    if not float(max_distance) >= 0.0:
        raise ValueError(f"max_distance must be non-negative, received: {max_distance}")
    if coords.n == 0:
        out = _copies(coords)
        if not return_index:
            return out
        return out + ((engine.empty_like_device(coords.like, (0,), np.int64)[0] if coords.on_device else np.empty(0, dtype=engine.IntDType)),)
    finish, x_ptr, y_ptr = _pair_out(coords)
    ids = None
    if return_index:
        ids = engine.empty_like_device(coords.like, (coords.n,), np.int64)[0] if coords.on_device else engine.DeviceArray((coords.n,), np.int64)
    n_tied = _snap_to(index, coords, max_distance, x_ptr, y_ptr, 1, engine.device_array_info(ids)[0] if ids is not None else 0)
    if n_tied and tiebreaker is None:
        raise ValueError(TIES)
    out = finish()
    if not return_index:
        return out
    return out + ((ids if coords.on_device else ids.download().astype(engine.IntDType, copy=False)),)


def snap_to_nodes(x, y, to_x, to_y, max_distance, tiebreaker=None, return_index=False):
    """snapping.py:146-219: every point ``(x, y)`` with a node ``(to_x, to_y)`` within ``max_distance`` moves onto the nearest
    such node; the others are copied.  -> ``(x_snapped, y_snapped)``, with ``return_index`` (an addition) also the int64 id of
    the node taken, -1 for none.  A point with several nodes within the distance raises ``ValueError`` unless
    ``tiebreaker="nearest"``; among equidistant nodes the lowest id wins (the reference's choice there is arbitrary)."""
    _check_tiebreaker(tiebreaker)
    coords = _Coords(x, y)
    to = _Coords(to_x, to_y, ("to_x", "to_y"))
    return _snap_onto(_to_index(to), coords, max_distance, tiebreaker, return_index)


def grid_snap_to_nodes(grid, x, y, max_distance, tiebreaker=None, return_index=False):
    """``snap_to_nodes`` onto the grid's own nodes, through its cached nearest-neighbour index."""
    _check_tiebreaker(tiebreaker)
    coords = _Coords(x, y)
    return _snap_onto(grid._nearest_index("node") if grid.n_node else None, coords, max_distance, tiebreaker, return_index)


def network_snap_nodes(grid, max_snap_distance, return_index=False):
    """See ``Ugrid1d.snap_nodes``."""
    from . import netedit

    xy, edges = netedit.device_arrays(grid)
    merged = DeviceSnap(xy.ptr, xy.ptr + 8, 2, grid.n_node, max_snap_distance) if grid.n_node else None
    if merged is None or merged.n_pair == 0:
        return (grid, {grid.node_dimension: None}) if return_index else grid
    new_xy = merged.xy().download()
    new_edges = merged.relabel(edges.ptr, (grid.n_edge, 2)).download()
    out = type(grid)(new_xy[:, 0].copy(), new_xy[:, 1].copy(), grid.fill_value, new_edges, name=grid.name)
    if not return_index:
        return out
    return out, {grid.node_dimension: merged.inverse().download().astype(engine.IntDType, copy=False)}
