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

from .inkind import Index, as_index, check_aligned, data_facet, facet_names, parse_indexers, raise_problems, result_kind


def _device_topology(grid):
    """The grid's device topology when the index arithmetic may use it: device-resident grids with a manifold topology."""
    if not grid._device_resident:
        return None
    topology = grid.device_topology()
    return topology if topology.manifold else None


def _cut(grid, face_index, want_node=False, want_edge=False):
    """-> (sub-grid or ``grid`` itself for the identity, node Index or None, edge Index or None)."""
    mesh, identity, problems = grid.device_mesh.subset(face_index.ptr(), face_index.n)
    raise_problems(problems, grid.n_face)
    if identity:
        return grid, (Index.arange(grid.n_node) if want_node else None), (Index.arange(grid.n_edge) if want_edge else None)
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
    like, to_numpy = result_kind(grid, index.like)
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
    given = parse_indexers(grid, indexers, indexers_kwargs)
    facet = data_facet(grid, data) if data is not None else None
    dims = facet_names(grid)
    # pre-check: every dimension must stand for the same faces
    index = check_aligned({dim: _faces_of(grid, dims[dim], index) for dim, index in given.items()})
    need = {dims[d] for d in given} | ({facet} if facet else set())
    want_node, want_edge = return_index or "node" in need, return_index or "edge" in need
    sub, node_index, edge_index = _cut(grid, index, want_node, want_edge)
    final = {"node": node_index, "edge": edge_index, "face": index}
    # post-check: a node or edge selection must be exactly the nodes or edges of the faces it stands for
    for dim, indexer in given.items():
        if dims[dim] != "face" and not Index.same(indexer, final[dims[dim]]):
            raise ValueError(f"This subset selection of UGRID dimension {dim} results in an invalid topology ")
    out = [sub]
    if return_index:
        like, to_numpy = result_kind(grid, *(i.like for i in given.values()))
        out.append({d: final[f].emit(like, to_numpy) for d, f in dims.items()})
    if data is not None:
        out.append(final[facet].gather(data, getattr(grid, f"n_{facet}")))
    return out[0] if len(out) == 1 else tuple(out)
