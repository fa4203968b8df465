"""
Filling the NaN entries of mesh data on the device: ``laplace_interpolate`` (xugrid/ugrid/interpolate.py:207-330) and the
nearest fill of ``UgridDataArrayAccessor.interpolate_na`` (xugrid/core/dataarray_accessor.py:761-886).  Kernels in
``csrc/xr_fill.hip``.  The nearest fill of a network along its edges (xugrid/ugrid/ugrid1d.py ``_nearest_interpolate``: a
multi-source dijkstra) is ``network_graph`` / ``network_fill`` / ``network_nearest``, kernels in ``csrc/xr_netfill.hip``.

Arrays in, arrays out, like ``Regridder.regrid``: ``data`` is ``(..., n)``; the leading dims are K slices filled
independently (the reference's ``apply_ufunc(vectorize=True)``).  K is unbounded: the kernels take at most 65 535 slices
per call (the launch grid's y dimension), so ``_run`` hands them consecutive tiles of the slices.  numpy in -> numpy out;
a device array in (torch tensor on the GPU, ``__cuda_array_interface__``) -> a float64 device array of the same kind,
nothing crossing PCIe but the per-slice status words.  The input is never modified.

Deviation: the reference preconditions CG with a sequential ILU0; the device runs unpreconditioned CG on
the same diagonally scaled system under scipy's stopping rule.  ``delta`` / ``relax`` (ILU0 knobs) are accepted at 0.0 only;
``direct_solve=True`` runs the device CG to ``rtol=1e-13, atol=0`` with ``maxiter = 10 n``.  ``maxiter`` counts device CG
iterations, which for a wide hole are more than the reference's preconditioned ones.
"""
import ctypes
import warnings

import numpy as np

from . import _lib, engine
from ._lib import check

CG_CHUNK = 24  # CG iterations enqueued between two reads of the slices' state
MAX_SLICES = 65535  # slices per kernel call (xr_fill.hip puts the slice on gridDim.y)
_STATUS_MAXITER, _STATUS_BREAKDOWN, _STATUS_NODATA = 1, 2, 3

# what the last fill reported per slice (tests and profiles read it: iteration counts of the device CG)
last_iterations = None
NET_CHUNK = 32  # rounds of the network nearest enqueued between two reads of the "changed" words
_NETWORK_FACET_IDS = {"node": 0, "edge": 1}  # include/xugrid_amd.h: XR_FACET_NODE, XR_FACET_EDGE
# rounds the last network fill / network nearest ran (the largest count of its tiles of slices; None: nothing ran)
last_rounds = None


class DeviceGraph(engine.Handle):
    """A symmetric adjacency in HBM (include/xugrid_amd.h: xr_graph): CSR structure, the weights, component labels."""

    _destroy = "xr_graph_destroy"

    def __init__(self, connectivity, labels=None, weights=None):
        lib = _lib.load()
        n, m = connectivity.shape
        indptr = np.ascontiguousarray(connectivity.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(connectivity.indices, dtype=np.int64)
        data = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int64)
        handle = ctypes.c_void_p()
        check(lib.xr_graph_from_csr(
            indptr.ctypes.data_as(ctypes.c_void_p), indices.ctypes.data_as(ctypes.c_void_p),
            None if data is None else data.ctypes.data_as(ctypes.c_void_p), n, indices.size,
            None if lab is None else lab.ctypes.data_as(ctypes.c_void_p), ctypes.byref(handle)))
        self._h = handle
        self.n, self.nnz, self.has_weights = n, indices.size, data is not None

    @classmethod
    def from_handle(cls, handle, has_weights):
        """Wrap an ``xr_graph`` made by the library (``DeviceTopology.graph``: nothing came from the host)."""
        self = object.__new__(cls)
        n, nnz = ctypes.c_int64(), ctypes.c_int64()
        check(_lib.load().xr_graph_info(handle, ctypes.byref(n), ctypes.byref(nnz)))
        self._h = handle
        self.n, self.nnz, self.has_weights = n.value, nnz.value, has_weights
        return self

    @classmethod
    def network(cls, node_xy, edges, facet):
        """The node graph (weights: the edge lengths) or the edge graph (half of the two edge lengths) of a network, built on
        the device from ``node_xy`` (n_node, 2) and ``edges`` (n_edge, 2) (include/xugrid_amd.h: xr_network_graph_dev)."""
        xy = engine.DeviceArray.from_host(np.ascontiguousarray(node_xy, dtype=np.float64).reshape(-1, 2))
        ed = engine.DeviceArray.from_host(np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2))
        handle, problems = ctypes.c_void_p(), (ctypes.c_int64 * 2)()
        check(_lib.load().xr_network_graph_dev(engine.vp(xy.ptr), xy.shape[0], engine.vp(ed.ptr), ed.shape[0],
                                               _NETWORK_FACET_IDS[facet], ctypes.byref(handle), problems))
        if problems[0] or problems[1]:
            raise ValueError(
                f"the network has {problems[0]} self-loops (edges from a node to itself) and {problems[1]} edges that repeat "
                "the node pair of an earlier edge; distances along the network need every node pair at most once"
            )
        return cls.from_handle(handle, True)

    def label_rounds(self):
        """Rounds of minimum-label propagation the component labelling took (0: the labels were given)."""
        rounds = ctypes.c_int64()
        check(_lib.load().xr_graph_label_rounds(self._h, ctypes.byref(rounds)))
        return rounds.value

    def download(self):
        """-> (indptr, indices, data) as numpy."""
        indptr, indices = np.empty(self.n + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int64)
        data = np.empty(self.nnz, dtype=np.float64)
        check(_lib.load().xr_graph_download(self._h, indptr.ctypes.data_as(ctypes.c_void_p), indices.ctypes.data_as(ctypes.c_void_p),
                                            data.ctypes.data_as(ctypes.c_void_p), None))
        return indptr, indices, data

    def labels(self):
        out = np.empty(self.n, dtype=np.int64)
        check(_lib.load().xr_graph_download(self._h, None, None, None, out.ctypes.data_as(ctypes.c_void_p)))
        return out


def _check_square(connectivity):
    n, m = connectivity.shape
    if n != m:
        raise ValueError(f"connectivity is not a square matrix: ({n}, {m})")
    return n


def _check_ilu_options(delta, relax):
    if delta != 0.0 or relax != 0.0:
        raise ValueError(
            "delta and relax tune the reference's ILU0 preconditioner; the device solver runs unpreconditioned CG on the "
            "same scaled system (no ILU0), so they must be 0.0"
        )


def _as_slices(data, n):
    """-> (kind, array, K, shape): kind 'device' (float64 contiguous device array) or 'host' (float64 numpy (K, n))."""
    info = engine.device_array_info(data)
    if info is not None:
        ptr, shape, dtype = info
        if dtype != np.float64:
            if engine.is_torch(data):
                data = data.double()
                ptr, shape, dtype = engine.device_array_info(data)
            else:
                raise TypeError(f"device data must be float64, received {dtype}")
        if len(shape) == 0 or shape[-1] != n:
            raise ValueError(f"expected data of shape (..., {n}), received: {shape}")
        K = int(np.prod(shape[:-1], dtype=np.int64))
        return "device", data, K, shape
    a = np.asarray(data, dtype=np.float64)
    if a.ndim == 0 or a.shape[-1] != n:
        raise ValueError(f"expected data of shape (..., {n}), received: {a.shape}")
    return "host", np.ascontiguousarray(a), int(np.prod(a.shape[:-1], dtype=np.int64)), a.shape


def _tiles(in_ptr, out_ptr, n, K, launch):
    """``launch(in_ptr, out_ptr, k)`` on consecutive tiles of at most MAX_SLICES slices (once, with k = 0, for K = 0).
    Every slice is filled independently of the others, so the tiling changes no result."""
    for k0 in range(0, max(K, 1), MAX_SLICES):
        offset = k0 * n * 8  # float64 (K, n)
        launch(in_ptr + offset, out_ptr + offset, min(MAX_SLICES, K - k0))


def _run(data, n, launch):
    """Move ``data`` to the device if it is not there, run ``launch(in_ptr, out_ptr, k)`` per tile of slices (``_tiles``),
    return the same kind."""
    kind, a, K, shape = _as_slices(data, n)
    if kind == "device":
        engine.sync_producer(a)
        out, out_ptr = engine.empty_like_device(a, shape)
        _tiles(engine.device_array_info(a)[0], out_ptr, n, K, launch)
        return out
    if a.size == 0:
        return a.copy()
    src = engine.DeviceArray.from_host(a)
    dst = engine.DeviceArray(a.shape)
    _tiles(src.ptr, dst.ptr, n, K, launch)
    return dst.download()


def laplace_fill(graph: DeviceGraph, data, use_weights, direct_solve=False, delta=0.0, relax=0.0, atol=1e-4, rtol=0.0,
                 maxiter=500):
    """Laplace fill of ``data`` (..., n) over ``graph`` (see the module docstring)."""
    global last_iterations
    _check_ilu_options(delta, relax)
    if use_weights and not graph.has_weights:
        raise ValueError("use_weights requires a connectivity with weights")
    n = graph.n
    if direct_solve:
        atol, rtol, maxiter = 0.0, 1e-13, 10 * max(n, 1)
    maxiter = int(maxiter)
    tiles = []  # (iterations, status) per tile of slices: checked together below, as for one call

    def launch(in_ptr, out_ptr, K):
        iters = np.zeros(K, dtype=np.int64)
        status = np.zeros(K, dtype=np.int32)
        check(_lib.load().xr_graph_laplace_fill_dev(
            graph._h, ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr), K, int(bool(use_weights)), float(atol),
            float(rtol), maxiter, CG_CHUNK, iters.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p)))
        tiles.append((iters, status))

    out = _run(data, n, launch)
    status = np.concatenate([s for _, s in tiles]) if tiles else np.zeros(0, dtype=np.int32)
    last_iterations = np.concatenate([i for i, _ in tiles]) if tiles else None
    if (status == _STATUS_NODATA).any():
        raise ValueError("data is fully nodata")
    if (status == _STATUS_BREAKDOWN).any():
        raise ValueError("conjugate gradient: illegal input or breakdown")
    if (status == _STATUS_MAXITER).any():
        warnings.warn(f"Failed to converge after {maxiter} iterations", UserWarning, stacklevel=3)
    return out


def nearest_fill(xy_dev: "engine.DeviceArray", data, max_distance=None):
    """Nearest fill of ``data`` (..., n) at the points ``xy_dev`` (a float64 (n, 2) device array)."""
    if max_distance is None:
        max_distance = np.inf
    max_distance = float(max_distance)
    if not max_distance >= 0.0:
        raise ValueError("max_distance must be non-negative")
    n = xy_dev.shape[0]

    def launch(in_ptr, out_ptr, K):
        check(_lib.load().xr_nearest_fill_dev(ctypes.c_void_p(xy_dev.ptr), n, ctypes.c_void_p(in_ptr),
                                              ctypes.c_void_p(out_ptr), K, max_distance))

    return _run(data, n, launch)


def _limit(max_distance):
    limit = np.inf if max_distance is None else float(max_distance)
    if not limit >= 0.0:
        raise ValueError("max_distance must be non-negative")
    return limit


def network_graph(grid, facet):
    """The device graph of ``grid`` (a ``Ugrid1d``) for ``facet`` "node" or "edge", built on first use and kept with the grid's
    other device caches (``DeviceGraph.network``)."""
    return grid._fill().network_graph(grid, facet)


def network_fill(graph: DeviceGraph, data, max_distance=None, chunk=None):
    """Nearest fill of ``data`` (..., n) along ``graph``: a NaN takes the value of the valid entry with the shortest path to
    it, of the lowest id among equidistant ones; entries farther than ``max_distance`` (inclusive, scipy's ``limit``) from
    every value, or in a component without one, stay NaN.  ``chunk``: rounds between two reads of the device's "changed"
    words (None: NET_CHUNK; no result depends on it)."""
    global last_rounds
    limit = _limit(max_distance)
    chunk = NET_CHUNK if chunk is None else int(chunk)
    rounds = []

    def launch(in_ptr, out_ptr, K):
        r = ctypes.c_int64()
        check(_lib.load().xr_graph_nearest_fill_dev(graph._h, engine.vp(in_ptr), engine.vp(out_ptr), K, limit, chunk,
                                                    ctypes.byref(r)))
        rounds.append(r.value)

    out = _run(data, graph.n, launch)
    last_rounds = max(rounds) if rounds else None
    return out


def network_nearest(graph: DeviceGraph, is_source, max_distance=None, chunk=None):
    """Per entry the distance along ``graph`` to the nearest source and that source's id: ``(distance (..., n) float64,
    source (..., n) int64)``, ``inf`` / ``-1`` where no source is within ``max_distance`` (inclusive).  ``is_source`` is a
    mask (..., n): a host array (anything non-zero is a source; numpy out) or a one-byte device array (torch ``bool`` /
    ``uint8`` -> torch tensors, another device array -> ``DeviceArray``).  The leading dims are slices, as in ``network_fill``."""
    global last_rounds
    limit = _limit(max_distance)
    chunk = NET_CHUNK if chunk is None else int(chunk)
    n = graph.n
    info = engine.byte_array_info(is_source)
    if info is not None:
        ptr, shape, _ = info
        like = is_source
        engine.sync_producer(is_source)
    else:
        mask = np.ascontiguousarray(np.asarray(is_source) != 0, dtype=np.uint8)
        shape = mask.shape
        uploaded = engine.DeviceArray.from_host(mask)  # (alive until the calls below have returned)
        ptr, like = uploaded.ptr, None
    if len(shape) == 0 or shape[-1] != n:
        raise ValueError(f"expected a mask of shape (..., {n}), received: {tuple(shape)}")
    K = int(np.prod(shape[:-1], dtype=np.int64))
    distance, d_ptr = engine.empty_like_device(like, shape)
    source, s_ptr = engine.empty_like_device(like, shape, np.int64)
    rounds = []
    for k0 in range(0, K, MAX_SLICES):
        r = ctypes.c_int64()
        check(_lib.load().xr_graph_nearest_dev(graph._h, engine.vp(ptr + k0 * n), min(MAX_SLICES, K - k0), limit, chunk,
                                               engine.vp(d_ptr + k0 * n * 8), engine.vp(s_ptr + k0 * n * 8), ctypes.byref(r)))
        rounds.append(r.value)
    last_rounds = max(rounds) if rounds else None
    if info is None:
        return distance.download(), source.download()
    return distance, source


def laplace_interpolate(data, connectivity, components_labels, use_weights, direct_solve=False, delta=0.0, relax=0.0,
                        atol=1e-4, rtol=0.0, maxiter=500):
    """xugrid.ugrid.interpolate.laplace_interpolate on the device: 1-D ``data`` (n,), scipy CSR ``connectivity`` (n, n)
    whose ``data`` are the weights when ``use_weights``, ``components_labels`` (n,) as scipy's ``connected_components``.
    The solver is the device CG of the module docstring (no ILU0; ``delta`` / ``relax`` must be 0.0)."""
    n = _check_square(connectivity)
    shape = engine.device_array_info(data)
    shape = shape[1] if shape is not None else np.shape(data)
    if tuple(shape) != (n,):
        raise ValueError(f"expected data of shape ({n},), received: {tuple(shape)}")
    _check_ilu_options(delta, relax)
    graph = DeviceGraph(connectivity, labels=components_labels, weights=connectivity.data if use_weights else None)
    return laplace_fill(graph, data, use_weights, direct_solve, delta, relax, atol, rtol, maxiter)


def connectivity_weights(connectivity, coordinates):
    """ugridbase.py:962-970: mean(d) / d of the distances between the connected points, in the matrix' entry order."""
    coo = connectivity.tocoo()
    d = coordinates[coo.col] - coordinates[coo.row]
    distance = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return distance.mean() / distance


class GridFill:
    """The fills of one grid: device graphs and point arrays per dimension, built on first use and kept."""

    def __init__(self):
        self.graphs = {}
        self.points = {}

    def graph(self, key, make_connectivity, coordinates, topology=None):
        """``topology``: a manifold ``DeviceTopology`` -- the graph is then made from it on the device (no scipy matrix, no
        host weights, no upload); otherwise from the host connectivity."""
        if key not in self.graphs:
            if topology is not None:
                self.graphs[key] = topology.graph(key)
            else:
                conn = make_connectivity()
                self.graphs[key] = DeviceGraph(conn, weights=connectivity_weights(conn, coordinates()))
        return self.graphs[key]

    def network_graph(self, grid, facet):
        """The shortest-path graph of a ``Ugrid1d`` (weights: lengths along the edges), under a key of its own: the Laplace
        graph of the same facet carries other weights."""
        key = ("network", facet)
        if key not in self.graphs:
            self.graphs[key] = DeviceGraph.network(grid.node_coordinates, grid.edge_node_connectivity, facet)
        return self.graphs[key]

    def xy(self, key, coordinates):
        if key not in self.points:
            xy = coordinates()  # (a DeviceArray where the points are in HBM already: the edge midpoints of a device topology)
            if not isinstance(xy, engine.DeviceArray):
                xy = engine.DeviceArray.from_host(np.ascontiguousarray(xy, dtype=np.float64))
            self.points[key] = xy
        return self.points[key]


def resolve_dim(grid, dim, facets):
    """'node' / 'edge' / 'face' or the grid's dimension name -> facet name."""
    names = {getattr(grid, f"{f}_dimension"): f for f in facets}
    if dim is None:
        dim = grid.core_dimension
    if dim in facets:
        return dim
    if dim in names:
        return names[dim]
    raise ValueError(f"Expected one of {sorted(list(names) + list(facets))}; got: {dim}")
