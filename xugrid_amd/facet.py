"""
Moving data between the facets of a mesh on the device: ``to_node`` / ``to_edge`` / ``to_face``
(``UgridDataArray.ugrid.to_node`` and its kin, xugrid/core/dataarray_accessor.py:300-416, ``_to_facet``).  Kernels in
``csrc/xr_facet.hip``.

``data`` is ``(..., n_source)``; the table is ``{target}_{source}_connectivity`` in dense form
(``format_connectivity_as_dense``, ugridbase.py:224).  With ``reduce=None`` the result is ``(..., n_target, w)``:
``out[..., t, j] = data[..., table[t, j]]``, NaN where ``table[t, j] == -1`` -- what ``obj.isel(...).where(indexer != -1)``
gives.  ``reduce`` in ``"mean"``, ``"sum"``, ``"min"``, ``"max"`` is the reference's ``.mean(dim)`` and its kin over that new
dimension, fused: the result is ``(..., n_target)`` and no ``(..., w)`` intermediate exists.  NaN contributors are skipped; a
target without a valid contributor gets NaN, 0.0 for the sum; the sum runs in table column order, sequentially, in float64,
and the mean is that sum divided once by the count.

Two routes, one launcher: a grid whose edge topology is in HBM (``Ugrid2d.from_device_arrays``, manifold) maps through the
tables where they are; every other grid (host-built, rectilinear, non-manifold, ``Ugrid1d``) uploads its int32 tables once
and keeps them until ``drop_device_caches``.

Deviations from the reference: float32 in gives float64 out (the reference keeps float32); integer data is refused (the
reference promotes it through ``.where``); ``dim`` names the SOURCE facet, not a new dimension; the device grid's
``edge_face`` always has two columns.

The array contract is ``sample.py``'s: numpy in -> numpy out, a device array in -> a float64 device array of the same kind.
"""
import numpy as np

from . import _lib, connectivity, engine
from ._lib import check
from .engine import vp
from .fill import resolve_dim
from .sample import _as_data

FORM_IDS = {"mean": 0, "sum": 1, "min": 2, "max": 3, None: 4}  # include/xugrid_amd.h: XR_FACET_MEAN, _SUM, _MIN, _MAX, _RAW
REDUCERS = ("mean", "sum", "min", "max")


def grid_facets(grid):
    """The facets a grid has: a ``Ugrid1d`` has no faces."""
    return ("node", "edge", "face") if hasattr(grid, "n_face") else ("node", "edge")


def _last_size(data):
    info = engine.device_array_info(data)
    shape = info[1] if info is not None else np.shape(data)
    if len(shape) == 0:
        raise ValueError("expected data of shape (..., n), received a scalar")
    return int(shape[-1])


def resolve(grid, target, data, dim, reduce):
    """-> the source facet; every argument error that needs no device is raised here."""
    facets = grid_facets(grid)
    if target not in facets:
        raise ValueError(f"Cannot map to {target} for a {type(grid).__name__} topology.")
    if reduce not in FORM_IDS:
        raise ValueError(f"reduce must be None or one of {', '.join(REDUCERS)}; received: {reduce}")
    if dim is not None:
        source = resolve_dim(grid, dim, facets)
    else:
        n = _last_size(data)
        sizes = {f: getattr(grid, f"n_{f}") for f in facets if f != target}
        matches = [f for f, size in sizes.items() if size == n]
        if len(matches) > 1:
            raise ValueError(f"data of {n} entries fits {' and '.join(matches)} alike: name the source facet with dim")
        if not matches:
            expected = ", ".join(f"{size} ({f})" for f, size in sizes.items())
            raise ValueError(f"data of {n} entries fits no source facet: expected sizes {expected}")
        source = matches[0]
    if source == target:
        raise ValueError(f"No conversion needed, data is already {target}-associated.")
    return source


def _refuse_integers(data):
    info = engine.device_array_info(data)
    dtype = info[2] if info is not None else np.asarray(data).dtype
    if np.dtype(dtype).kind != "f":
        raise TypeError(f"data must be float64 or float32, received {dtype} (integer data is not promoted)")


# ---- the table route: int32 tables of the host connectivity, uploaded once per grid -------------------------------------------
def host_table(grid, target, source):
    """``{target}_{source}_connectivity`` of the host route -> (indptr or None, indices, width): dense ``(n_target, width)``
    with -1 fill, or CSR with ``width`` the widest row."""
    conn = getattr(grid, f"{target}_{source}_connectivity")
    if target == "node":  # scipy CSR
        indptr = np.asarray(conn.indptr)
        n_target = getattr(grid, "n_node")
        if indptr.size != n_target + 1:
            raise ValueError(f"node_{source}_connectivity has {indptr.size - 1} rows for {n_target} nodes")
        width = int(np.diff(indptr).max()) if n_target else 0
        return indptr, np.asarray(conn.indices), width
    conn = np.asarray(conn)
    return None, conn, int(conn.shape[1])


class _DeviceTable:
    def __init__(self, indptr, indices, width, n_target, n_source):
        for a in (indptr, indices):
            if a is not None and a.size and (a.max() > np.iinfo(np.int32).max):
                raise OverflowError("connectivity beyond 2^31 does not fit the int32 device tables")
        self.ptr = None if indptr is None else engine.DeviceArray.from_host(np.ascontiguousarray(indptr, dtype=np.int32))
        self.idx = engine.DeviceArray.from_host(np.ascontiguousarray(indices, dtype=np.int32).reshape(-1))
        self.width, self.n_target, self.n_source = width, n_target, n_source


def _device_table(grid, target, source):
    cache = grid.__dict__.setdefault("_facet_cache", {})
    key = (target, source)
    if key not in cache:
        indptr, indices, width = host_table(grid, target, source)
        cache[key] = _DeviceTable(indptr, indices, width, getattr(grid, f"n_{target}"), getattr(grid, f"n_{source}"))
    return cache[key]


def _topology(grid):
    """The grid's manifold ``DeviceTopology``, or None: the table route."""
    get = getattr(grid, "_fill_topology", None)
    return get() if get is not None else None


def facet_width(grid, target, source):
    """Width ``w`` of the ``(..., n_target, w)`` layout ``to_{target}`` gives for data on ``source``."""
    facets = grid_facets(grid)
    if target not in facets:
        raise ValueError(f"Cannot map to {target} for a {type(grid).__name__} topology.")
    source = resolve_dim(grid, source, facets)
    if source == target:
        raise ValueError(f"No conversion needed, data is already {target}-associated.")
    topology = _topology(grid)
    if topology is not None:
        return topology.facet_width(target, source)
    cache = grid.__dict__.get("_facet_cache", {})
    if (target, source) in cache:
        return cache[(target, source)].width
    return host_table(grid, target, source)[2]


def to_facet(grid, target, data, dim=None, reduce=None):
    """See ``Ugrid2d.to_node``."""
    source = resolve(grid, target, data, dim, reduce)
    _refuse_integers(data)
    n_source, n_target = getattr(grid, f"n_{source}"), getattr(grid, f"n_{target}")
    kind, a, dtype_id, K, shape = _as_data(data, n_source)
    form = FORM_IDS[reduce]
    topology = _topology(grid)
    if topology is not None:
        width = topology.facet_width(target, source)

        def run(in_ptr, out_ptr):
            topology.facet_map(target, source, form, in_ptr, dtype_id, K, out_ptr)
    else:
        table = _device_table(grid, target, source)
        width = table.width

        def run(in_ptr, out_ptr):
            check(_lib.load().xr_facet_map_dev(vp(table.ptr.ptr) if table.ptr is not None else None,
                                               vp(table.idx.ptr), table.n_target, table.width, table.n_source, form,
                                               vp(in_ptr), dtype_id, K, vp(out_ptr)))
    out_shape = shape[:-1] + ((n_target, width) if reduce is None else (n_target,))
    if kind == "device":
        engine.sync_producer(a)
        out, out_ptr = engine.empty_like_device(a, out_shape)
        run(engine.device_array_info(a)[0], out_ptr)
        return out
    src = engine.DeviceArray.from_host(a)
    dst = engine.DeviceArray(out_shape)
    run(src.ptr, dst.ptr)
    return dst.download()


def node_edge_connectivity(edge_node_connectivity, n_node):
    """node -> edge, scipy CSR over all nodes, edges ascending per row (ugridbase.py:866-878)."""
    return connectivity.invert_dense_to_sparse(np.asarray(edge_node_connectivity), n_rows=n_node)
