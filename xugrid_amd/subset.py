"""
Sub-meshes: ``topology_subset`` / ``clip_box`` / ``isel`` of ``Ugrid2d`` (xugrid/ugrid/ugrid2d.py:1138-1288, the index rules of
ugridbase.py:42-78 and :703-720) on arrays.  Kernels in ``csrc/xr_subset.hip``; DESIGN section 14.

The mesh is always cut on the device (``DeviceMesh.subset``).  The index arithmetic around it -- a mask to an index, the faces of
a node or edge selection, the edge index of the result, the equality checks of ``isel`` -- runs on the device for grids whose
mesh lives in HBM (``from_device_arrays``, rectilinear) and in numpy for host grids and for grids whose topology is
non-manifold (the device topology keeps no edge tables for those).

Kinds of result, as ``triangulate``: a host grid gives a host grid, a device-resident grid a ``DeviceUgrid2d``.  Indexes are
int64: device arrays of the indexer's kind when an indexer is a device array (torch tensor, ``__cuda_array_interface__``);
otherwise numpy for a host grid and ``DeviceArray`` for a device-resident one.

Indexers are 1-D integer ids (unique, any order) or a bool mask of the dimension's length; a one-byte device array (torch
``bool`` / ``uint8``, typestr ``|b1`` / ``|u1``) is a mask.  Ids outside ``[0, n)`` raise ``IndexError`` -- negative ones too:
nothing wraps around.
"""
import numpy as np

from . import engine, sample

REPEATED = "index contains repeated values; only subsets will result in valid UGRID topology."
FACETS = ("node", "edge", "face")


def _raise_problems(problems, n):
    out_of_range, repeated = problems
    if out_of_range:
        raise IndexError(f"index contains {out_of_range} value(s) outside [0, {n}); negative values do not wrap around")
    if repeated:
        raise ValueError(REPEATED)


class Index:
    """One normalised indexer: ``n`` unique int64 ids, on the host (``host``), on the device (``dev``) or both; each side is
    made from the other on first use.  ``like``: the caller's device array when the indexer came as one."""

    def __init__(self, host=None, dev=None, like=None):
        self.host, self.dev, self.like = host, dev, like
        self.n = int(host.shape[0]) if host is not None else int(engine.device_array_info(dev)[1][0])

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
        if self.dev is not None and engine.is_torch(self.dev) == (like is not None and engine.is_torch(like)):
            return self.dev
        return engine.upload_like(self.numpy(), like)


def as_index(index, n, checked=True):
    """ugridbase.py:42-78 (``as_pandas_index``) on arrays -> ``Index``.  Host indexers are checked here; device indexers are
    checked on the device (``checked``: now; else the caller's next kernel does it, ``DeviceMesh.subset``)."""
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
        dev = index
        if dtype != np.int64:
            if not engine.is_torch(index):
                raise TypeError("an integer device index must be int64")
            dev = index.long()
        engine.sync_producer(index)
        out = Index(dev=dev, like=index)
        if checked:
            _raise_problems(engine.index_check(out.ptr(), out.n, n), n)
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
    _raise_problems((out_of_range, 0 if out_of_range else a.size - np.unique(a).size), n)
    return Index(host=a)


def _same(a, b):
    """pandas ``Index.equals`` on two indexes: the same ids in the same order."""
    if a.n != b.n:
        return False
    if a.n == 0:
        return True
    if a.host is not None and b.host is not None:
        return bool(np.array_equal(a.host, b.host))
    return engine.index_mismatch(a.ptr(), b.ptr(), a.n) == 0


def _device_topology(grid):
    """The grid's device topology when the index arithmetic may use it: device-resident grids with a manifold topology."""
    if not grid._device_resident:
        return None
    topology = grid.device_topology()
    return topology if topology.manifold else None


def _result_kind(grid, *indexes):
    """-> (like, to_numpy) for the indexes a call returns."""
    like = next((i.like for i in indexes if i.like is not None), None)
    return like, (like is None and not grid._device_resident)


def _arange(n):
    return Index(host=np.arange(n, dtype=np.int64))


def _cut(grid, face_index, want_node=False, want_edge=False):
    """-> (sub-grid or ``grid`` itself for the identity, node Index or None, edge Index or None)."""
    mesh, identity, problems = grid.device_mesh.subset(face_index.ptr(), face_index.n)
    _raise_problems(problems, grid.n_face)
    if identity:
        return grid, (_arange(grid.n_node) if want_node else None), (_arange(grid.n_edge) if want_edge else None)
    sub = grid._grid_from_mesh(mesh)
    node_index = Index(dev=mesh.subset_node_index_dev(face_index.like), like=None) if want_node else None
    edge_index = None
    if want_edge:
        topology = _device_topology(grid)
        if topology is not None:
            edge_index = Index(dev=topology.subset_edges(face_index.ptr(), face_index.n).to_dev(face_index.like))
        else:  # host grids and non-manifold topologies: numpy over the host tables
            edges = np.unique(np.asarray(grid.face_edge_connectivity)[face_index.numpy()].ravel())
            edge_index = Index(host=edges[edges != -1].astype(np.int64))
    return sub, node_index, edge_index


def topology_subset(grid, face_index, return_index=False):
    """ugrid2d.py:1138-1216 on arrays: see ``Ugrid2d.topology_subset``."""
    index = as_index(face_index, grid.n_face, checked=False)
    sub, node_index, edge_index = _cut(grid, index, return_index, return_index)
    if not return_index:
        return sub
    like, to_numpy = _result_kind(grid, index)
    return sub, {
        grid.node_dimension: node_index.emit(like, to_numpy),
        grid.edge_dimension: edge_index.emit(like, to_numpy),
        grid.face_dimension: index.emit(like, to_numpy),
    }


def clip_box(grid, xmin, ymin, xmax, ymax):
    """ugrid2d.py:1218-1226: the faces whose centroid lies in the half-open box; on a device-resident grid the box test runs
    on the device centroids."""
    if grid._device_resident:
        index = Index(dev=grid.device_mesh.box_faces(xmin, ymin, xmax, ymax).to_dev())
    else:
        index = Index(host=np.asarray(grid.locate_bounding_box(xmin, ymin, xmax, ymax), dtype=np.int64))
    return _cut(grid, index)[0]


def _faces_of(grid, facet, index):
    """The face index a node or edge selection stands for (ugrid2d.py:1262-1270)."""
    if facet == "face":
        return index
    if grid._device_resident and facet == "node":
        return Index(dev=grid.device_mesh.faces_of_nodes(index.ptr(), index.n).to_dev(index.like), like=index.like)
    topology = _device_topology(grid) if facet == "edge" else None
    if topology is not None:
        return Index(dev=topology.faces_of_edges(index.ptr(), index.n).to_dev(index.like), like=index.like)
    if facet == "node":
        faces = np.unique(grid.node_face_connectivity[index.numpy()].data)
    else:
        faces = np.unique(np.asarray(grid.edge_face_connectivity)[index.numpy()])
        faces = faces[faces != -1]
    return Index(host=faces.astype(np.int64), like=index.like)


def isel(grid, indexers=None, return_index=False, data=None, **indexers_kwargs):
    """ugrid2d.py:1228-1288 on arrays: see ``Ugrid2d.isel``."""
    if indexers is not None and indexers_kwargs:
        raise ValueError("cannot specify both keyword and positional arguments to .isel")
    indexers = dict(indexers if indexers is not None else indexers_kwargs)
    dims = {grid.node_dimension: "node", grid.edge_dimension: "edge", grid.face_dimension: "face"}
    invalid = set(indexers) - set(dims)
    if invalid:
        raise ValueError(f"Dimensions {invalid} do not exist. Expected one of {set(dims)}")
    if not indexers:
        raise ValueError("isel needs an indexer for at least one UGRID dimension")
    given = {dim: as_index(v, getattr(grid, f"n_{dims[dim]}")) for dim, v in indexers.items()}
    face_index = {dim: _faces_of(grid, dims[dim], index) for dim, index in given.items()}
    # pre-check: every dimension must stand for the same faces
    dim, index = face_index.popitem()
    for check_dim, check_index in face_index.items():
        if not _same(index, check_index):
            raise ValueError(f"UGRID dimensions do not align: {dim} versus {check_dim}")
    data_facet = None
    if data is not None:
        data_facet = _data_facet(grid, data)
    need = {dims[d] for d in given} | ({data_facet} if data_facet else set())
    want_node, want_edge = return_index or "node" in need, return_index or "edge" in need
    sub, node_index, edge_index = _cut(grid, index, want_node, want_edge)
    final = {"node": node_index, "edge": edge_index, "face": index}
    # post-check: a node or edge selection must be exactly the nodes or edges of the faces it stands for
    for dim, indexer in given.items():
        if dims[dim] != "face" and not _same(indexer, final[dims[dim]]):
            raise ValueError(f"This subset selection of UGRID dimension {dim} results in an invalid topology ")
    out = [sub]
    if return_index:
        like, to_numpy = _result_kind(grid, *given.values())
        out.append({d: final[f].emit(like, to_numpy) for d, f in dims.items()})
    if data is not None:
        gather = final[data_facet]
        by = gather.device() if engine.device_array_info(data) is not None else gather.numpy()
        out.append(sample.gather_points(data, getattr(grid, f"n_{data_facet}"), by))
    return out[0] if len(out) == 1 else tuple(out)


def _data_facet(grid, data):
    info = engine.device_array_info(data)
    shape = info[1] if info is not None else np.shape(data)
    if len(shape) == 0:
        raise ValueError("data must have shape (..., n) with n the size of one UGRID dimension")
    fits = [f for f in FACETS if getattr(grid, f"n_{f}") == shape[-1]]
    if len(fits) != 1:
        raise ValueError(f"the last dimension of data ({shape[-1]}) must be the size of exactly one of the UGRID dimensions, "
                         f"it fits: {fits}")
    return fits[0]
