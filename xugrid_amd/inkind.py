"""
The index and data-kind layer under the mesh-editing modules (``subset``, ``netedit``, ``partition``, ``periodic``; DESIGN
section 14): what they all ask of an index or of ``data`` is answered here, once.

``Index``: int64 ids on the host, on the device or on both; a side is made from the other on first use and kept, so an index
crosses PCIe at most once each way.  ``emit`` hands it to the caller, ``gather`` reads ``data`` through it on the side the
data is on.  ``as_index`` makes one from an indexer (ugridbase.py:42-78).

The kind rule (``result_kind``): indexes come back as device arrays of the kind of the first device array the caller gave,
else as ``DeviceArray`` when a grid is device-resident, else as numpy int64.  ``data`` ``(..., n)``: numpy in -> numpy out, a
device array in -> a float64 device array of its kind (``sample.gather_points``).

``data_facet`` is the one place that decides which facet ``data`` lies on, for one grid or a list of partitions.
"""
import numpy as np

from . import engine, sample
from .facet import grid_facets

REPEATED = "index contains repeated values; only subsets will result in valid UGRID topology."


def raise_problems(problems, n):
    out_of_range, repeated = problems
    if out_of_range:
        raise IndexError(f"index contains {out_of_range} value(s) outside [0, {n}); negative values do not wrap around")
    if repeated:
        raise ValueError(REPEATED)


class Index:
    """One normalised indexer: ``n`` int64 ids, on the host (``host``), on the device (``dev``) or both; each side is made
    from the other on first use.  ``like``: the caller's device array when the indexer came as one."""

    def __init__(self, host=None, dev=None, like=None):
        self.host, self.dev, self.like = host, dev, like
        shape = host.shape if host is not None else getattr(dev, "shape", None) or engine.device_array_info(dev)[1]
        self.n = int(shape[0])

    @classmethod
    def wrap(cls, a, like=None):
        """An index that arrives as numpy or as a device array; an ``Index`` passes through."""
        if isinstance(a, Index):
            return a
        return cls(host=a, like=like) if isinstance(a, np.ndarray) else cls(dev=a, like=like)

    @classmethod
    def arange(cls, n):
        return cls(host=np.arange(n, dtype=np.int64))

    def numpy(self):
        if self.host is None:
            self.host = engine.download(self.dev).astype(np.int64, copy=False)
        return self.host

    def device(self, like=None):
        if self.dev is None:
            self.dev = engine.upload_like(self.host, like if like is not None else self.like)
        return self.dev

    def ptr(self):
        return engine.device_array_info(self.device())[0]

    def emit(self, like, to_numpy):
        """The index as the caller gets it: numpy, or a device array of the kind of ``like``."""
        if to_numpy:
            return self.numpy()
        if self.dev is None:
            self.dev = engine.upload_like(self.host, like)
        elif engine.is_torch(self.dev) != (like is not None and engine.is_torch(like)):
            return engine.upload_like(self.numpy(), like)
        return self.dev

    def gather(self, data, n, fill_value=np.nan):
        """``data[..., index]`` for ``data`` ``(..., n)``, on the side ``data`` is on; ``fill_value`` where an id is -1."""
        by = self.numpy() if engine.device_array_info(data) is None else self.device(data)
        return sample.gather_points(data, n, by, fill_value)

    @staticmethod
    def same(a, b):
        """pandas ``Index.equals`` on two indexes: the same ids in the same order."""
        if a.n != b.n:
            return False
        if a.n == 0:
            return True
        if a.host is not None and b.host is not None:
            return bool(np.array_equal(a.host, b.host))
        return engine.index_mismatch(a.ptr(), b.ptr(), a.n) == 0


# ---- what came in ---------------------------------------------------------------------------------------------------------------
def int64_dev(values, what, n=None):
    """-> (int64 device array, like, length): 1-D integers from the host (uploaded; ``like`` None) or from the device (a torch
    tensor of another width is cast; ``like`` is ``values``).  ``n``: the length they must have."""
    info = None if isinstance(values, (list, tuple)) else engine.device_array_info(values)
    a = np.asarray(values) if info is None else None
    shape, dtype = (a.shape, a.dtype) if info is None else info[1:]
    if dtype.kind not in "iu":
        raise TypeError(f"{what} must have integer dtype")
    dev = _int64_of(values, dtype, what) if info is not None else None
    if len(shape) != 1:
        raise ValueError(f"{what} must be 1-D")
    if n is not None and shape[0] != n:
        raise ValueError(f"{what} must have the length {n}, received: {shape[0]}")
    if info is None:
        return engine.DeviceArray.from_host(np.ascontiguousarray(a, dtype=np.int64)), None, int(shape[0])
    return dev, values, int(shape[0])


def _int64_of(values, dtype, what):
    """A device array of integers of ``dtype`` as an int64 one the engine may read: a torch tensor of another width is cast."""
    if dtype != np.int64 and not engine.is_torch(values):
        raise TypeError(f"integer device {what} must be int64")
    dev = values if dtype == np.int64 else values.long()
    engine.sync_producer(values)  # (after the cast: it runs on the producer's stream too)
    return dev


def xy_dev(values, what):
    """-> (device array, pointer, shape): float64 coordinates from the host (uploaded) or from the device."""
    info = engine.device_array_info(values)
    if info is not None:
        if info[2] != np.float64:
            raise TypeError(f"device {what} must be float64")
        engine.sync_producer(values)
        return values, info[0], tuple(info[1])
    a = np.ascontiguousarray(values, dtype=np.float64)
    dev = engine.DeviceArray.from_host(a)
    return dev, dev.ptr, a.shape


def as_index(index, n, checked=True):
    """ugridbase.py:42-78 (``as_pandas_index``) on arrays -> ``Index``: 1-D integer ids (unique, any order) or a bool mask of
    length ``n``.  Host indexers are checked here; device indexers are checked on the device (``checked``: now; else the
    caller's next kernel does it, ``DeviceMesh.subset``)."""
    if isinstance(index, Index):
        return index
    mask = engine.byte_array_info(index)
    if mask is not None:
        ptr, shape, _ = mask
        if len(shape) != 1:
            raise ValueError("index should be 1d")
        if shape[0] != n:
            raise ValueError(f"a bool index must have the dimension's size {n}, received: {shape[0]}")
        engine.sync_producer(index)
        return Index(dev=engine.DeviceIndex.from_mask(ptr, n).to_dev(index), like=index)
    info = None if isinstance(index, (list, tuple)) else engine.device_array_info(index)
    if info is not None:
        _, shape, dtype = info
        if len(shape) != 1:
            raise ValueError("index should be 1d")
        if shape[0] > n:
            raise ValueError(f"index size {shape[0]} is larger than dimension size: {n}")
        if dtype.kind != "i":
            raise TypeError(f"index should be bool or integer. Received: {dtype}")
        out = Index(dev=_int64_of(index, dtype, "index"), like=index)
        if checked:
            raise_problems(engine.index_check(out.ptr(), out.n, n), n)
        return out
    a = np.asarray(index)
    if a.ndim != 1:
        raise ValueError("index should be 1d")
    if a.size > n:
        raise ValueError(f"index size {a.size} is larger than dimension size: {n}")
    if a.dtype == np.bool_:
        if a.size != n:
            raise ValueError(f"a bool index must have the dimension's size {n}, received: {a.size}")
        return Index(host=np.nonzero(a)[0].astype(np.int64))
    if not np.issubdtype(a.dtype, np.integer) and not (a.size == 0 and isinstance(index, (list, tuple))):
        raise TypeError(f"index should be bool or integer. Received: {a.dtype}")
    a = a.astype(np.int64)
    out_of_range = int(((a < 0) | (a >= n)).sum())
    raise_problems((out_of_range, 0 if out_of_range else a.size - np.unique(a).size), n)
    return Index(host=a)


def parse_indexers(grid, indexers, indexers_kwargs):
    """The indexers of an ``isel`` -> ``{dimension name: Index}``, after the argument checks of ugridbase.py:703-720."""
    if indexers is not None and indexers_kwargs:
        raise ValueError("cannot specify both keyword and positional arguments to .isel")
    indexers = dict(indexers if indexers is not None else indexers_kwargs)
    names = facet_names(grid)
    invalid = set(indexers) - set(names)
    if invalid:
        raise ValueError(f"Dimensions {invalid} do not exist. Expected one of {set(names)}")
    if not indexers:
        raise ValueError("isel needs an indexer for at least one UGRID dimension")
    return {dim: as_index(v, getattr(grid, f"n_{names[dim]}")) for dim, v in indexers.items()}


def check_aligned(indexes):
    """The pre-check of ``isel``: ``{dimension name: Index}`` must hold the same ids under every name -> that ``Index``."""
    dim, index = indexes.popitem()
    for check_dim, check_index in indexes.items():
        if not Index.same(index, check_index):
            raise ValueError(f"UGRID dimensions do not align: {dim} versus {check_dim}")
    return index


# ---- facets and kinds -----------------------------------------------------------------------------------------------------------
def facet_names(grid):
    """``{dimension name: facet}`` for the facets the grid has."""
    return {getattr(grid, f"{f}_dimension"): f for f in grid_facets(grid)}


def data_facet(grids, data, dim=None):
    """The facet ``data`` ``(..., n)`` lies on: the one whose size is ``n``, among all facets or the one ``dim`` names (a
    ring, or equal counts, leave it open).  One grid and one array, or a list of partitions and a list with one array each:
    then every array must fit the facet in its own partition.  Needs no device."""
    if isinstance(grids, (list, tuple)):
        if len(data) != len(grids):
            raise ValueError(f"data must hold one array per partition: {len(grids)} partitions, {len(data)} arrays")
    else:
        grids, data = [grids], [data]
    shapes = []
    for d in data:
        info = engine.device_array_info(d)
        shapes.append(tuple(info[1]) if info is not None else np.shape(d))
    if any(len(s) == 0 for s in shapes) or len({s[:-1] for s in shapes}) != 1:
        raise ValueError("data must have shape (..., n) with n the size of one UGRID dimension, and the same leading dimensions "
                         "in every partition")
    names = facet_names(grids[0])
    candidates = tuple(names.values())
    if dim is not None:
        if dim not in names:
            raise ValueError(f"dim {dim!r} is not a UGRID dimension, expected one of {set(names)}")
        candidates = (names[dim],)
    fits = [f for f in candidates if all(s[-1] == getattr(g, f"n_{f}") for s, g in zip(shapes, grids))]
    if len(fits) != 1:
        raise ValueError(f"the last dimension of data ({', '.join(str(s[-1]) for s in shapes)}) must be the size of exactly one "
                         f"UGRID dimension of its grid, it fits: {fits}")
    return fits[0]


def result_kind(grids, *likes):
    """-> (like, to_numpy) for the indexes a call returns: ``like`` is the first device array among ``likes``."""
    grids = grids if isinstance(grids, (list, tuple)) else [grids]
    like = next((x for x in likes if x is not None), None)
    return like, (like is None and not any(getattr(g, "_device_resident", False) for g in grids))


def first_torch(items):
    return next((x for x in items if x is not None and engine.is_torch(x)), None)


# ---- partitions -----------------------------------------------------------------------------------------------------------------
def concat_last_axis(data, sizes):
    """The partitions' data side by side along the last axis -> (array of one kind, total)."""
    total = int(sum(sizes))
    infos = [engine.device_array_info(d) for d in data]
    if all(i is None for i in infos):
        arrays = [np.asarray(d) for d in data]
        dtype = np.float32 if all(a.dtype == np.float32 for a in arrays) else np.float64
        return np.concatenate([a.astype(dtype, copy=False) for a in arrays], axis=-1), total
    if any(i is None for i in infos):
        raise TypeError("the partitions' data must be all host arrays or all device arrays")
    if first_torch(data) is not None:
        import torch

        return torch.cat([d if d.dtype in (torch.float32, torch.float64) else d.double() for d in data], dim=-1).contiguous(), total
    if len({i[2] for i in infos}) != 1:
        raise TypeError("the partitions' device data must have one dtype")
    lead = infos[0][1][:-1]
    K = int(np.prod(lead, dtype=np.int64))
    flat = [d.reshape(K, s) if hasattr(d, "reshape") else d for d, s in zip(data, sizes)]
    return engine.concat_last_axis_dev(flat).reshape(*lead, total), total


def host_edge_node(grid):
    if grid.n_face == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return np.asarray(grid.edge_node_connectivity, dtype=np.int64).reshape(-1, 2)


def device_topologies(grids, new):
    """The device topologies of ``grids`` and of ``new`` (last) when the edge arithmetic may run on them, else None."""
    if not all(g._device_resident and g.n_face > 0 for g in list(grids) + [new]):
        return None
    topologies = [g.device_topology() for g in list(grids) + [new]]
    return topologies if all(t.manifold for t in topologies) else None
