"""
Graph operations on a symmetric adjacency on the device: ``connected_components`` (scipy.sparse.csgraph's numbering) and the
binary morphology of xugrid/ugrid/connectivity.py:791-877 (``binary_dilation`` / ``binary_erosion``).  Kernels in
``csrc/xr_fill.hip`` (k_comp_*, k_binary_step); the functions here take a scipy CSR like ``fill.laplace_interpolate``, the
``Ugrid2d`` methods hand in the grid's device graph.  ``reverse_cuthill_mckee`` (kernels in ``csrc/xr_rcm.hip``) renumbers the
rows as ``scipy.sparse.csgraph.reverse_cuthill_mckee(..., symmetric_mode=True)`` does, with one stated difference: seeds are
taken in ``(degree, id)`` order, the stable sort, where scipy's unstable argsort picks among equal degrees as numpy's sort
kernel happens to (include/xugrid_amd.h: xr_graph_rcm_dev).

Binary iteration, restated: one iteration is a Jacobi step on a snapshot -- an entry becomes ``value`` (True for dilation,
False for erosion) iff a neighbour's old state differs from its own.  After every step the entries of ``mask`` are set to
``not value`` (sic: the reference writes ``output[mask] = not value``; reproduced).  After the first step
only, the ``exterior`` entries are set to ``value`` -- when ``border_value == value``, else ``exterior`` is ignored.
Deviation: ``iterations < 1`` raises ``ValueError`` (the reference silently runs one iteration).

bool numpy in -> bool numpy out; a device bool / uint8 array in (torch tensor on the GPU, ``__cuda_array_interface__``) -> a
device array of the same kind and dtype out.  ``input`` is ``(..., n)``: leading dims are independent slices.  The input is
never modified.
"""
import ctypes

import numpy as np

from . import _lib, engine
from ._lib import check
from .fill import MAX_SLICES, DeviceGraph, _check_square


def _bool_info(obj):
    """``engine.byte_array_info``; a device array of any other dtype raises."""
    info = engine.byte_array_info(obj)
    if info is None:
        try:
            other = engine.device_array_info(obj) is not None
        except (TypeError, ValueError):  # (a device array the engine takes nowhere)
            other = True
        if other:
            raise TypeError("input dtype should be bool")
    return info


def _flags(flags, n, what):
    """mask / exterior -> a uint8 (n,) device array (or None): bool arrays, index arrays (``exterior``) or device bytes."""
    if flags is None:
        return None
    info = _bool_info(flags)
    if info is not None:
        if info[1] != (n,):
            raise ValueError(f"expected {what} of shape ({n},), received: {info[1]}")
        engine.sync_producer(flags)
        return flags, info[0]
    a = np.asarray(flags)
    if a.dtype != np.bool_:  # indices, as the reference's `exterior`
        b = np.zeros(n, dtype=bool)
        b[a.astype(np.int64)] = True
        a = b
    if a.shape != (n,):
        raise ValueError(f"expected {what} of shape ({n},), received: {a.shape}")
    dev = engine.DeviceArray.from_host(a.view(np.uint8))
    return dev, dev.ptr


def binary_iterate(graph: DeviceGraph, input, value, iterations=1, mask=None, exterior=None, border_value=False):
    """The binary iteration of the module docstring over a ``DeviceGraph``."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"iterations must be at least 1, received: {iterations}")
    n = graph.n
    info = _bool_info(input)
    if info is None:
        a = np.asarray(input)
        if a.dtype != np.bool_:
            raise TypeError("input dtype should be bool")
        shape = a.shape
    else:
        shape = info[1]
    if len(shape) == 0 or shape[-1] != n:
        raise ValueError(f"expected input of shape (..., {n}), received: {tuple(shape)}")
    K = int(np.prod(shape[:-1], dtype=np.int64))
    mask_dev = _flags(mask, n, "mask")
    exterior_dev = _flags(exterior, n, "exterior") if bool(border_value) == bool(value) else None
    if info is None:
        if a.size == 0:
            return a.copy()
        src = engine.DeviceArray.from_host(np.ascontiguousarray(a).view(np.uint8))
        dst = engine.DeviceArray(shape, np.uint8)
        in_ptr, out_ptr, out = src.ptr, dst.ptr, None
    else:
        engine.sync_producer(input)
        in_ptr = info[0]
        if engine.is_torch(input):
            import torch

            out = torch.empty(shape, dtype=input.dtype, device=input.device)
            out_ptr = int(out.data_ptr())
        else:
            out = engine.DeviceArray(shape, np.bool_ if info[2] == "bool" else np.uint8)
            out_ptr = out.ptr
    lib = _lib.load()
    for k0 in range(0, K, MAX_SLICES):  # (slices are independent: the tiling changes no result)
        check(lib.xr_graph_binary_iterate_dev(
            graph._h, ctypes.c_void_p(in_ptr + k0 * n), ctypes.c_void_p(out_ptr + k0 * n), min(MAX_SLICES, K - k0), int(bool(value)),
            iterations, None if mask_dev is None else ctypes.c_void_p(mask_dev[1]),
            None if exterior_dev is None else ctypes.c_void_p(exterior_dev[1])))
    if info is None:
        return dst.download().view(np.bool_)
    return out


def components(graph: DeviceGraph):
    """int64 numpy ``(n,)`` component numbers 0 .. n_components-1 in the order of each component's smallest member (the
    numbering of ``scipy.sparse.csgraph.connected_components``)."""
    count = ctypes.c_int64()
    out = engine.DeviceArray((graph.n,), np.int64)
    check(_lib.load().xr_graph_components_dev(graph._h, ctypes.c_void_p(out.ptr), ctypes.byref(count)))
    return out.download()


RCM_BLOCK = 256  # RB, csrc/xr_rcm.hip: positions of a level one block of the level kernels takes per turn
RCM_GRID = 1024  # RCM_GRID, csrc/xr_rcm.hip: blocks of a level kernel at most (a wider level takes several turns)
last_levels = None  # breadth-first levels the last renumbering ran (tests and profiles read it)


def rcm_dev(graph: DeviceGraph):
    """The reverse Cuthill-McKee order of ``graph`` as an int64 ``DeviceArray`` ``(n,)``: new row ``i`` is old row ``order[i]``."""
    global last_levels
    levels = ctypes.c_int64()
    out = engine.DeviceArray((graph.n,), np.int64)
    check(_lib.load().xr_graph_rcm_dev(graph._h, ctypes.c_void_p(out.ptr), ctypes.byref(levels)))
    last_levels = levels.value
    return out


def rcm(graph: DeviceGraph):
    """``rcm_dev`` as int64 numpy ``(n,)``."""
    return rcm_dev(graph).download()


def _graph_of(connectivity):
    _check_square(connectivity)
    csr = connectivity.tocsr()
    csr.sort_indices()
    return DeviceGraph(csr)


def connected_components(connectivity):
    """Component number per row of the symmetric scipy CSR ``connectivity``, as ``scipy.sparse.csgraph.connected_components``."""
    return components(_graph_of(connectivity))


def reverse_cuthill_mckee(connectivity):
    """The permutation ``scipy.sparse.csgraph.reverse_cuthill_mckee(connectivity, symmetric_mode=True)`` gives for the symmetric
    scipy CSR ``connectivity``, its seeds taken in ``(degree, id)`` order (see the module docstring)."""
    _check_square(connectivity)
    csr = connectivity.tocsr().copy()  # (the caller's matrix keeps its repeated entries)
    csr.sum_duplicates()
    return rcm(_graph_of(csr))


def binary_dilation(connectivity, input, iterations=1, mask=None, exterior=None, border_value=False):
    """xugrid.ugrid.connectivity.binary_dilation on the device.  By default, does not dilate inward from the exterior."""
    return binary_iterate(_graph_of(connectivity), input, True, iterations, mask, exterior, border_value)


def binary_erosion(connectivity, input, iterations=1, mask=None, exterior=None, border_value=False):
    """xugrid.ugrid.connectivity.binary_erosion on the device.  By default, erodes inwards from the exterior."""
    return binary_iterate(_graph_of(connectivity), input, False, iterations, mask, exterior, border_value)
