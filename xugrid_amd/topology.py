"""
The edge topology of a device mesh, built on the device (``csrc/xr_topology.hip``): unique edges, face -> edge, edge -> face, the
face and node adjacencies and the exterior flags, each equal element for element to what ``xugrid_amd/connectivity.py``
derives on the host from the same faces.  Nothing of the size of the mesh crosses PCIe unless one of the arrays is asked for
as numpy; the fills and graph operations read the topology where it is.
"""
import ctypes

import numpy as np
from scipy import sparse

from . import _lib, engine
from ._lib import check

_FACET_IDS = {"node": 0, "edge": 1, "face": 2}  # include/xugrid_amd.h: XR_FACET_NODE, XR_FACET_EDGE, XR_FACET_FACE

# slots of xr_topology_download, in argument order
_SLOTS = ("edge_node", "face_edge", "edge_face", "ff_indptr", "ff_indices", "ff_data", "nn_indptr", "nn_indices", "nn_data",
          "exterior_edge", "exterior_face")


class DeviceTopology(engine.Handle):
    """``xr_topology`` of a ``DeviceMesh`` (which it keeps alive).  ``n_nonmanifold`` > 0 -- an edge with more than two faces
    does not fit the two columns of ``edge_face_connectivity`` -- means the handle holds nothing: the caller takes the host
    route.  Arrays are downloaded lazily as int64 numpy and kept.

    The handle borrows the mesh; it copies none of it.  Its own arrays (edges, adjacencies, flags) depend on the faces alone
    and stay valid after ``DeviceMesh.invalidate()`` -- which ``drop_device_caches`` calls and which drops only what the mesh
    derives (centroids, areas, index), never ``faces_raw`` or the node coordinates.  A topology still held by the caller
    after that keeps answering: ``graph("face")`` has the mesh rebuild its centroids, at the cost of that rebuild.  The grid
    itself makes a new topology on next use."""

    _destroy = "xr_topology_destroy"

    def __init__(self, device_mesh):
        self._mesh = device_mesh
        handle = ctypes.c_void_p()
        check(_lib.load().xr_topology_create(device_mesh._h, ctypes.byref(handle)))
        self._h = handle
        v = [ctypes.c_int64() for _ in range(5)]
        check(_lib.load().xr_topology_info(handle, *(ctypes.byref(x) for x in v)))
        self.n_edge, self.n_exterior_edge, self.face_face_nnz, self.node_node_nnz, self.n_nonmanifold = (x.value for x in v)
        n_node, n_face, m = (ctypes.c_int64() for _ in range(3))
        check(_lib.load().xr_mesh_info(device_mesh._h, ctypes.byref(n_node), ctypes.byref(n_face), ctypes.byref(m)))
        self.n_node, self.n_face, self.n_max_node_per_face = n_node.value, n_face.value, m.value
        n_long = ctypes.c_int64()
        check(_lib.load().xr_topology_long_nodes(handle, ctypes.byref(n_long)))
        self.n_long_nodes = n_long.value  # nodes past 16 distinct neighbours: listed by the wave-per-node kernel
        self._host = {}
        self._edge_xy = None

    @property
    def manifold(self):
        return self.n_nonmanifold == 0

    # ---- lazy int64 downloads
    def _shape(self, slot):
        E, F, N = self.n_edge, self.n_face, self.n_node
        return {
            "edge_node": (E, 2), "face_edge": (F, self.n_max_node_per_face), "edge_face": (E, 2), "ff_indptr": (F + 1,),
            "ff_indices": (self.face_face_nnz,), "ff_data": (self.face_face_nnz,), "nn_indptr": (N + 1,),
            "nn_indices": (self.node_node_nnz,), "nn_data": (self.node_node_nnz,), "exterior_edge": (E,), "exterior_face": (F,),
        }[slot]

    def _get(self, *slots):
        missing = [s for s in slots if s not in self._host]
        if missing:
            arrays = {s: np.empty(self._shape(s), dtype=np.int64) for s in missing}
            args = [arrays[s].ctypes.data_as(ctypes.c_void_p) if s in arrays else None for s in _SLOTS]
            check(_lib.load().xr_topology_download(self._h, *args))
            self._host.update(arrays)
        return [self._host[s] for s in slots]

    @property
    def edge_node_connectivity(self):
        return self._get("edge_node")[0]

    @property
    def face_edge_connectivity(self):
        return self._get("face_edge")[0]

    @property
    def edge_face_connectivity(self):
        return self._get("edge_face")[0]

    @property
    def face_face_connectivity(self):
        """scipy CSR (n_face, n_face); data = the shared edge's id (a fresh matrix per call, like the host property)."""
        indptr, indices, data = self._get("ff_indptr", "ff_indices", "ff_data")
        return sparse.csr_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(self.n_face, self.n_face))

    @property
    def node_node_connectivity(self):
        indptr, indices, data = self._get("nn_indptr", "nn_indices", "nn_data")
        return sparse.csr_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(self.n_node, self.n_node))

    def _node_tables(self):
        """node -> face and node -> edge (``xr_topology_download_node_tables``): the row pointers first, they size the rest."""
        if "nf_indptr" not in self._host:
            N = self.n_node
            nf_indptr, ne_indptr = np.empty(N + 1, dtype=np.int64), np.empty(N + 1, dtype=np.int64)
            as_vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            check(_lib.load().xr_topology_download_node_tables(self._h, as_vp(nf_indptr), None, as_vp(ne_indptr), None))
            nf_indices, ne_indices = np.empty(nf_indptr[-1], dtype=np.int64), np.empty(ne_indptr[-1], dtype=np.int64)
            check(_lib.load().xr_topology_download_node_tables(self._h, None, as_vp(nf_indices), None, as_vp(ne_indices)))
            self._host.update(nf_indptr=nf_indptr, nf_indices=nf_indices, ne_indptr=ne_indptr, ne_indices=ne_indices)
        return [self._host[s] for s in ("nf_indptr", "nf_indices", "ne_indptr", "ne_indices")]

    @property
    def node_face_connectivity(self):
        """scipy CSR (n_node, n_face), faces ascending per row; data = the face id, as ``invert_dense_to_sparse`` leaves it."""
        indptr, indices, _, _ = self._node_tables()
        return sparse.csr_matrix((indices.copy(), indices.copy(), indptr.copy()), shape=(self.n_node, self.n_face))

    @property
    def node_edge_connectivity(self):
        """scipy CSR (n_node, n_edge), edges ascending per row: the node_node rows with the edge id as the column."""
        _, _, indptr, indices = self._node_tables()
        return sparse.csr_matrix((indices.copy(), indices.copy(), indptr.copy()), shape=(self.n_node, self.n_edge))

    @property
    def exterior_edges(self):
        return np.nonzero(self._get("exterior_edge")[0])[0]

    @property
    def exterior_faces(self):
        return np.nonzero(self._get("exterior_face")[0])[0]

    # ---- what stays in HBM
    def edge_coordinates_device(self):
        """Edge midpoints ``0.5 * (a + b)`` as a float64 ``(n_edge, 2)`` ``DeviceArray`` (kept)."""
        if self._edge_xy is None:
            xy = engine.DeviceArray((self.n_edge, 2))
            check(_lib.load().xr_topology_edge_xy_dev(self._h, ctypes.c_void_p(xy.ptr)))
            self._edge_xy = xy
        return self._edge_xy

    def exterior_face_flags_device(self):
        """uint8 ``(n_face,)`` ``DeviceArray``: 1 for a face with at least one exterior edge."""
        flags = engine.DeviceArray((self.n_face,), np.uint8)
        check(_lib.load().xr_topology_exterior_face_dev(self._h, ctypes.c_void_p(flags.ptr)))
        return flags

    def facet_width(self, target, source):
        """Width of ``{target}_{source}_connectivity`` in dense form: m, 2, or the widest row of a node table."""
        w = ctypes.c_int64()
        check(_lib.load().xr_topology_facet_width(self._h, _FACET_IDS[target], _FACET_IDS[source], ctypes.byref(w)))
        return w.value

    def facet_map(self, target, source, form, in_ptr, dtype_id, K, out_ptr):
        """``xr_topology_facet_map_dev`` on device pointers: the tables are read where they are."""
        check(_lib.load().xr_topology_facet_map_dev(self._h, _FACET_IDS[target], _FACET_IDS[source], form,
                                                    ctypes.c_void_p(int(in_ptr)), dtype_id, K, ctypes.c_void_p(int(out_ptr))))

    # ---- index arithmetic of sub-meshes (xugrid_amd/subset.py); manifold topologies only
    def faces_of_edges(self, edge_index_ptr, n):
        """The faces beside the edges ``edge_index`` (an int64 device pointer, ``n`` ids), ascending -> ``engine.DeviceIndex``."""
        handle = ctypes.c_void_p()
        check(_lib.load().xr_topology_faces_of_edges_dev(self._h, ctypes.c_void_p(int(edge_index_ptr)), int(n), ctypes.byref(handle)))
        return engine.DeviceIndex(handle)

    def subset_edges(self, face_index_ptr, n):
        """The edges of the faces ``face_index`` (an int64 device pointer, ``n`` ids), ascending -> ``engine.DeviceIndex``."""
        handle = ctypes.c_void_p()
        check(_lib.load().xr_topology_subset_edges_dev(self._h, ctypes.c_void_p(int(face_index_ptr)), int(n), ctypes.byref(handle)))
        return engine.DeviceIndex(handle)

    def graph(self, facet):
        """The fills' ``DeviceGraph`` of the faces or nodes: structure, ``mean(d) / d`` weights and component labels, all
        made on the device."""
        from .fill import DeviceGraph

        handle = ctypes.c_void_p()
        check(_lib.load().xr_graph_from_topology(self._h, _FACET_IDS[facet], ctypes.byref(handle)))
        return DeviceGraph.from_handle(handle, has_weights=True)
