"""
Minimal ``Ugrid2d``: exactly the slice of xugrid/ugrid/ugrid2d.py the regridding hot path touches
(SURVEY.md 2 row 11): the constructor's connectivity handling (:72-115), ``node_coordinates``
(ugridbase.py:576-579), ``area`` (:575-584), ``centroids`` (:544-559), ``celltree`` (:908-921),
``locate_points`` (ugridbase.py:1305-1323), ``compute_barycentric_weights`` (:1054-1078) and
``from_structured_bounds`` (:1894-1912, :1973-2034), and what later sections of DESIGN.md added (fills, sampling, facets,
derived meshes, sub-meshes: ``topology_subset`` / ``clip_box`` / ``isel``).  IO, plotting and partitioning are out of scope.
"""
import numpy as np

import ctypes

from . import _lib, connectivity, engine, facet, fill, geometry, graph, sample, snap
from .celltree import CellTree2d
from .engine import FloatDType, IntDType

FILL_VALUE = -1


def _node_table(node_x, node_y):
    """(n, 2) C-contiguous float64 table of the node coordinates: the layout the device wants, written once -- by the
    library's host threads when the inputs are float64 (any stride, e.g. the two columns of an (n, 2) array)."""
    x, y = np.asarray(node_x), np.asarray(node_y)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("node_x and node_y must be 1-D arrays of equal length")
    n = x.size
    if n >= 65536 and x.dtype == np.float64 and y.dtype == np.float64 and x.strides[0] % 8 == 0 and y.strides[0] % 8 == 0:
        out = np.empty((n, 2), dtype=np.float64)
        _lib.check(_lib.load().xr_host_interleave2(ctypes.c_void_p(x.ctypes.data), x.strides[0] // 8, ctypes.c_void_p(y.ctypes.data),
                                                   y.strides[0] // 8, n, ctypes.c_void_p(out.ctypes.data)))
        return out
    return np.column_stack([np.asarray(x, dtype=FloatDType), np.asarray(y, dtype=FloatDType)])


def _copy_connectivity(faces):
    """face_node_connectivity.copy() as IntDType (ugrid2d.py:94-96): a private copy the constructor may rewrite."""
    if faces.dtype == IntDType and faces.flags.c_contiguous and faces.nbytes >= (1 << 20):
        out = np.empty(faces.shape, dtype=IntDType)
        _lib.check(_lib.load().xr_host_copy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(faces.ctypes.data), faces.nbytes))
        return out
    return faces.astype(IntDType, copy=True)


class Ugrid2d:
    def __init__(self, node_x, node_y, fill_value, face_node_connectivity, name="mesh2d", start_index=0):
        # (n, 2) node table, contiguous: what node_coordinates returns and the device mesh uploads; node_x / node_y
        # (contiguous, as the reference keeps them, ugrid2d.py:86-87) are cut out of it on first use
        self._node_xy = _node_table(node_x, node_y)
        self._node_x = self._node_y = None
        if not isinstance(face_node_connectivity, np.ndarray):
            raise TypeError("face_node_connectivity should be an array of integers")
        faces = _copy_connectivity(face_node_connectivity)
        if faces.ndim != 2:
            raise ValueError("face_node_connectivity must be 2-D (n_face, n_max_node_per_face)")
        # fill -> -1 and 0-based, as ugrid2d.py:105-110
        if fill_value != FILL_VALUE or start_index != 0:
            is_fill = faces == fill_value
            if start_index != 0:
                faces[~is_fill] -= start_index
            if fill_value != FILL_VALUE:
                faces[is_fill] = FILL_VALUE
        self.face_node_connectivity = faces
        self.fill_value = FILL_VALUE
        self.start_index = 0
        self.name = name
        self._celltree = None
        self._voronoi_device_cache = None  # (UnstructuredGrid2d._voronoi_device)
        self._area = None
        self._centroids = None
        self._edge_node_connectivity = None
        self._face_edge_connectivity = None
        self._edge_face_connectivity = None
        self._node_face_connectivity = None

    @property
    def node_x(self):
        if self._node_x is None:
            self._node_x = np.ascontiguousarray(self._node_xy[:, 0])
        return self._node_x

    @property
    def node_y(self):
        if self._node_y is None:
            self._node_y = np.ascontiguousarray(self._node_xy[:, 1])
        return self._node_y

    # plain attributes in the reference (ugrid2d.py:86-87): assigning new coordinates is legal there.  Here the interleaved
    # buffer is what the device sees, so an assignment rebuilds it and drops everything derived from the old coordinates
    # that THIS grid holds.  Regridders and UnstructuredGrid2d wrappers already built from the grid keep the weights they
    # computed from the old coordinates, as in the reference: build new ones.
    @node_x.setter
    def node_x(self, value):
        self._set_node_axis(0, value)

    @node_y.setter
    def node_y(self, value):
        self._set_node_axis(1, value)

    def _set_node_axis(self, axis, value):
        value = np.asarray(value, dtype=np.float64)
        if value.shape != (self.n_node,):
            raise ValueError(f"expected {self.n_node} node coordinates, got shape {value.shape}")
        xy = np.array(self._node_xy)  # (a fresh buffer: the old one may be in use by a device upload or a caller's view)
        xy[:, axis] = value
        self._node_xy = xy
        self._node_x = self._node_y = None
        self._area = self._centroids = None
        self.drop_device_caches()

    # ---- sizes / names
    @property
    def n_node(self):
        return self._node_xy.shape[0]

    @property
    def n_face(self):
        return self.face_node_connectivity.shape[0]

    @property
    def n_max_node_per_face(self):
        return self.face_node_connectivity.shape[1]

    @property
    def face_dimension(self):
        return f"{self.name}_nFaces"

    @property
    def node_dimension(self):
        return f"{self.name}_nNodes"

    @property
    def edge_dimension(self):
        return f"{self.name}_nEdges"

    @property
    def core_dimension(self):
        return self.face_dimension

    @property
    def dims(self):
        return (self.face_dimension,)

    @property
    def node_coordinates(self):
        """(n_node, 2), a FRESH array per call as in the reference (``column_stack``, ugridbase.py:576-579): writing into it
        changes neither the grid nor its device copy -- assign ``node_x`` / ``node_y`` for that (the setters drop what was
        derived from the old coordinates).  Until round 5 this was a read-only view of the grid's own buffer; reference-style
        code that edits the returned array in place raised on it."""
        return self._node_xy.copy()

    @property
    def bounds(self):
        lo, hi = self._node_xy.min(axis=0), self._node_xy.max(axis=0)
        return (lo[0], lo[1], hi[0], hi[1])

    def node_coordinates_of(self, nodes):
        """(len(nodes), 2) coordinates of the given node ids."""
        return self._node_xy[nodes]

    # ---- device-backed geometry
    @property
    def celltree(self) -> CellTree2d:
        if self._celltree is None:
            self._celltree = CellTree2d(self._node_xy, self.face_node_connectivity, FILL_VALUE)
        return self._celltree

    def drop_device_caches(self):
        """Release what this grid keeps in HBM beyond its mesh: the celltree index and the cached centroidal Voronoi
        tessellation of the barycentric path (mesh, prepared arrays and index: several times ``n_face`` worth of memory that
        the engine's pool cannot reclaim while the grid is alive).  The next regridder on this grid rebuilds them."""
        self._celltree = None
        self._voronoi_device_cache = None
        self.__dict__.pop("_fill_cache", None)
        self.__dict__.pop("_sample_cache", None)
        self.__dict__.pop("_topology_cache", None)
        self.__dict__.pop("_facet_cache", None)
        self.__dict__.pop("_derive_cache", None)

    @property
    def device_mesh(self):
        return self.celltree.device_mesh

    @property
    def area(self):
        if self._area is None:
            self._area = self.device_mesh.area()
        return self._area

    @property
    def centroids(self):
        if self._centroids is None:
            self._centroids = self.device_mesh.centroids()
        return self._centroids

    def locate_points(self, points, tolerance=None):
        return self.celltree.locate_points(points, tolerance)

    def compute_barycentric_weights(self, points, tolerance=None):
        return self.celltree.compute_barycentric_weights(points, tolerance)

    # ---- point sampling with the same spatial index (ugrid2d.py:1080-1140)
    def rasterize_like(self, x, y):
        """Face index at every (y, x) raster node: -> (x, y, index (nrow, ncol)), -1 outside the grid."""
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        # (the y.size * x.size sample points are generated on the device from the two 1-D arrays)
        return x, y, self.device_mesh.locate_raster(x, y)

    def rasterize(self, resolution, bounds=None):
        """Sample the grid on a raster of cell centres generated from ``bounds`` (default: the node bounds)
        and ``resolution``; y runs from top to bottom."""
        if bounds is None:
            bounds = self.bounds
        xmin, ymin, xmax, ymax = bounds
        d = abs(resolution)
        xmin = np.floor(xmin / d) * d
        xmax = np.ceil(xmax / d) * d
        ymin = np.floor(ymin / d) * d
        ymax = np.ceil(ymax / d) * d
        x = np.arange(xmin + 0.5 * d, xmax, d)
        y = np.arange(ymax - 0.5 * d, ymin, -d)
        return self.rasterize_like(x, y)

    # ---- host-side connectivities (feed the Voronoi pre-step of BarycentricInterpolator)
    @property
    def edge_node_connectivity(self):
        if self._edge_node_connectivity is None:
            self._edge_node_connectivity, self._face_edge_connectivity = connectivity.edge_connectivity(
                self.face_node_connectivity
            )
        return self._edge_node_connectivity

    @property
    def face_edge_connectivity(self):
        if self._face_edge_connectivity is None:
            self.edge_node_connectivity
        return self._face_edge_connectivity

    @property
    def edge_face_connectivity(self):
        if self._edge_face_connectivity is None:
            self._edge_face_connectivity = connectivity.invert_dense(self.face_edge_connectivity)
        return self._edge_face_connectivity

    @property
    def node_face_connectivity(self):
        if self._node_face_connectivity is None:
            self._node_face_connectivity = connectivity.invert_dense_to_sparse(
                self.face_node_connectivity, n_rows=self.n_node
            )
        return self._node_face_connectivity

    @property
    def node_edge_connectivity(self):
        """node -> edge, scipy CSR over all nodes, edges ascending per row (ugridbase.py:866-878)."""
        return facet.node_edge_connectivity(self.edge_node_connectivity, self.n_node)

    @property
    def n_edge(self):
        return self.edge_node_connectivity.shape[0]

    @property
    def edge_coordinates(self):
        """(n_edge, 2) edge midpoints (ugridbase.py:606-609)."""
        xy = self.node_coordinates_of(self.edge_node_connectivity.ravel()).reshape(-1, 2, 2)
        return 0.5 * (xy[:, 0] + xy[:, 1])

    @property
    def face_face_connectivity(self):
        """Faces sharing an edge, scipy CSR; data = the shared edge's id (ugrid2d.py:680-698)."""
        return connectivity.face_face_connectivity(self.edge_face_connectivity, self.n_face)

    @property
    def node_node_connectivity(self):
        """Nodes joined by an edge, scipy CSR; data = the edge's id."""
        return connectivity.node_node_connectivity(self.edge_node_connectivity, self.n_node)

    def get_connectivity_matrix(self, dim, xy_weights):
        """ugrid2d.py:746-762: the face or node adjacency; with ``xy_weights`` its data are mean(d) / d of the centroid or
        node distances (ugridbase.py:962-970)."""
        facet = fill.resolve_dim(self, dim, ("node", "face"))
        conn = self.node_node_connectivity if facet == "node" else self.face_face_connectivity
        if xy_weights:
            conn.data = fill.connectivity_weights(conn, self._fill_coordinates(facet))
        return conn

    # ---- filling NaN entries on the device (xugrid_amd/fill.py)
    def _fill(self):
        cache = self.__dict__.get("_fill_cache")
        if cache is None:
            cache = self.__dict__["_fill_cache"] = fill.GridFill()
        return cache

    def _fill_coordinates(self, facet):
        if facet == "node":
            return self.node_coordinates
        if facet == "edge":
            return self._edge_points()
        return self.centroids

    def _edge_points(self):
        """Edge midpoints for the nearest fill and the nearest index: a host array here, a device array where the grid has
        its topology in HBM (DeviceUgrid2d)."""
        return self.edge_coordinates

    def _fill_topology(self):
        """The ``DeviceTopology`` the fill graphs are made from, or None: the host connectivity (host-built grids)."""
        return None

    def _graph(self, facet):
        """The device graph (structure, weights, component labels) of the faces or nodes, built on first use and kept."""
        conn = (lambda: self.node_node_connectivity) if facet == "node" else (lambda: self.face_face_connectivity)
        return self._fill().graph(facet, conn, lambda: self._fill_coordinates(facet), topology=self._fill_topology())

    # ---- the edge topology in HBM and the graph operations on it (xugrid_amd/topology.py, xugrid_amd/graph.py)
    def device_topology(self):
        """The grid's ``DeviceTopology``: edges and adjacencies built on the device from the device mesh (kept until
        ``drop_device_caches``)."""
        from .topology import DeviceTopology

        cache = self.__dict__.get("_topology_cache")
        if cache is None:
            cache = self.__dict__["_topology_cache"] = DeviceTopology(self.device_mesh)
        return cache

    @property
    def exterior_edges(self):
        """Ascending indices of the edges with one face only (ugrid2d.py:877-887)."""
        edge_face = self.edge_face_connectivity
        if edge_face.shape[1] < 2:  # (the host table is as wide as the busiest edge: no edge has two faces)
            return np.arange(edge_face.shape[0])
        return np.nonzero(edge_face[:, 1] == FILL_VALUE)[0]

    @property
    def exterior_faces(self):
        """Ascending indices of the faces with an unshared edge (ugrid2d.py:889-900)."""
        faces = self.edge_face_connectivity[self.exterior_edges].ravel()
        return np.unique(faces[faces != FILL_VALUE])

    def _exterior_face_flags(self):
        flags = np.zeros(self.n_face, dtype=bool)
        flags[self.exterior_faces] = True
        return flags

    def connected_components(self, dim=None):
        """int64 ``(n,)`` component number of every face (default) or node, numbered like
        ``scipy.sparse.csgraph.connected_components`` on the adjacency (dataarray_accessor.py:691-708); labelled on the device."""
        facet = fill.resolve_dim(self, dim, ("node", "face"))
        return graph.components(self._graph(facet))

    def reverse_cuthill_mckee(self, dimension=None, data=None, return_device=False):
        """The grid with its faces renumbered to reduce the bandwidth of ``face_face_connectivity`` (ugrid2d.py:1734-1756) ->
        ``(reordered_grid, reordering)``: a grid of this grid's kind with the same nodes (unused ones included) and the faces
        ``face_node_connectivity[reordering]``.  The order is ``scipy.sparse.csgraph.reverse_cuthill_mckee``'s with seeds taken
        in ``(degree, id)`` order (``graph.reverse_cuthill_mckee``), computed on the device; for a grid whose mesh lives in HBM
        the face table is gathered there too.  ``reordering``: int64 numpy, or with ``return_device`` on such a grid an int64
        device array (of ``data``'s kind when ``data`` is a device array).  ``dimension``: ``None`` or the face dimension
        (nodes are not renumbered), else ``ValueError``.  ``data`` ``(..., n_face)``: also returned, gathered along its last
        axis (numpy in -> numpy out, device array in -> float64 device array out)."""
        from .inkind import Index

        if dimension is not None and dimension != self.face_dimension:
            raise ValueError(f"reverse_cuthill_mckee renumbers {self.face_dimension} only, received: {dimension}")
        index = Index(dev=graph.rcm_dev(self._graph("face")))
        data_on_device = data is not None and engine.device_array_info(data) is not None
        if self._device_resident:
            grid = self._grid_from_mesh(self.device_mesh.reorder_faces(index.ptr()))
        else:
            grid = Ugrid2d(self.node_x, self.node_y, FILL_VALUE, self.face_node_connectivity[index.numpy()], name=self.name)
        out = [grid, index.emit(data if data_on_device else None, not (return_device and self._device_resident))]
        if data is not None:
            out.append(index.gather(data, self.n_face))
        return tuple(out)

    def _binary(self, data, value, iterations, mask, border_value):
        exterior = self._exterior_face_flags() if bool(border_value) == bool(value) else None
        return graph.binary_iterate(self._graph("face"), data, value, iterations, mask, exterior, border_value)

    def binary_dilation(self, data, iterations=1, mask=None, border_value=False):
        """Expand the True entries of the bool face data ``data`` (..., n_face) over the face adjacency, ``iterations`` times
        (dataarray_accessor.py:643-665); leading dims are independent slices.  ``mask`` (n_face,) and ``border_value`` as
        in the reference (xugrid_amd/graph.py).  numpy in -> numpy out, device bool / uint8 in -> the same kind out."""
        return self._binary(data, True, iterations, mask, border_value)

    def binary_erosion(self, data, iterations=1, mask=None, border_value=False):
        """Shrink the True entries of ``data`` (dataarray_accessor.py:667-689); see ``binary_dilation``."""
        return self._binary(data, False, iterations, mask, border_value)

    def laplace_interpolate(self, data, dim=None, xy_weights=True, direct_solve=False, delta=0.0, relax=0.0, rtol=0.0,
                            atol=1e-4, maxiter=500):
        """Fill the NaN entries of ``data`` (..., n) along ``dim`` (default: faces) by Laplace interpolation on the device
        (UgridDataArrayAccessor.laplace_interpolate, dataarray_accessor.py:805-886).  Unpreconditioned CG instead of the
        reference's ILU0-preconditioned one: ``delta`` / ``relax`` must be 0.0 and ``maxiter`` counts device iterations
        (xugrid_amd/fill.py).  numpy in -> numpy out, device array in -> float64 device array out."""
        facet = fill.resolve_dim(self, dim, ("node", "edge", "face"))
        if facet == "edge":
            raise ValueError("Laplace interpolation along edges is not allowed.")
        fill._check_ilu_options(delta, relax)
        return fill.laplace_fill(self._graph(facet), data, xy_weights, direct_solve, delta, relax, atol, rtol, maxiter)

    def interpolate_na(self, data, dim=None, method="nearest", max_distance=None):
        """Fill the NaN entries of ``data`` (..., n) along ``dim`` (default: faces) with the value of the nearest non-NaN
        entry closer than ``max_distance`` (UgridDataArrayAccessor.interpolate_na): face centroids, nodes or edge
        midpoints; among equidistant entries the lowest index wins."""
        if method != "nearest":
            raise ValueError(f'"{method}" is not a valid interpolator.')
        facet = fill.resolve_dim(self, dim, ("node", "edge", "face"))
        xy = self._fill().xy(facet, lambda: self._fill_coordinates(facet))
        return fill.nearest_fill(xy, data, max_distance)

    # ---- reading data at points and along lines on the device (xugrid_amd/sample.py)
    def _sample(self):
        cache = self.__dict__.get("_sample_cache")
        if cache is None:
            cache = self.__dict__["_sample_cache"] = sample.GridSample()
        return cache

    def _nearest_index(self, facet):
        """The nearest-neighbour index of a facet's points: nodes and face centroids are read from the device mesh where they
        are; edge midpoints come from ``edge_coordinates``."""
        if facet == "edge":
            return self._sample().index(facet, lambda: sample.NearestIndex.from_points(self._edge_points()))
        return self._sample().index(facet, lambda: sample.NearestIndex.from_mesh(self.device_mesh, facet))

    def _locate_nearest(self, facet, points, max_distance=np.inf):
        if facet not in sample.FACETS:
            raise ValueError(f"Expected facet as one of {sample.FACETS}, received: {facet}")
        return self._nearest_index(facet).query(points, max_distance)

    def locate_nearest_node(self, points, max_distance=np.inf):
        """Index of the nearest node per point ``(n_point, 2)``, -1 for none (ugridbase.py:1261-1281): strictly closer
        than ``max_distance`` as scipy's ``distance_upper_bound``; the lowest index among equidistant nodes.  Host points
        -> numpy; a float64 device array -> an int64 device array of the same kind."""
        return self._locate_nearest("node", points, max_distance)

    def locate_nearest_edge(self, points, max_distance=np.inf):
        """... the nearest edge midpoint (ugridbase.py:1283-1303).  On a host-built grid the edges are derived on the host
        (``connectivity.edge_connectivity``); a grid made by ``from_device_arrays`` takes them from its device topology."""
        return self._locate_nearest("edge", points, max_distance)

    def locate_nearest_face(self, points, max_distance=np.inf):
        """... the nearest face centroid (ugrid2d.py:1007-1027)."""
        return self._locate_nearest("face", points, max_distance)

    def snap_to_nodes(self, x, y, max_distance, tiebreaker=None, return_index=False):
        """``xugrid_amd.snap_to_nodes`` (snapping.py:146-219) with this grid's nodes as the targets, through its cached node
        index: the points ``(x, y)`` within ``max_distance`` of a node move onto the nearest one.  -> ``(x_snapped,
        y_snapped[, index])``; host arrays in -> numpy out, device arrays in -> device arrays out."""
        return snap.grid_snap_to_nodes(self, x, y, max_distance, tiebreaker, return_index)

    def snap_to_grid(self, lines, max_snap_distance):
        """``xugrid_amd.snap_to_grid`` (snapping.py:496-552) with this grid: the lines ``(coords, line_offsets[, values])`` snapped
        to its edges -> ``(line_index (n_edge,), edges, edge_lines[, values])``."""
        from . import snapgrid

        return snapgrid.snap_to_grid(lines, self, max_snap_distance)

    def intersect_edges(self, edges):
        """ugridbase.py:1325-1343: ``(edge_index, face_index, intersections (n, 2, 2))`` of segments ``(n_edge, 2, 2)``."""
        return self.celltree.intersect_edges(edges)

    def locate_bounding_box(self, xmin, ymin, xmax, ymax):
        """Indices of the faces whose centroid lies in the half-open box ``xmin <= x < xmax``, ``ymin <= y < ymax``
        (ugrid2d.py:1029-1052)."""
        return sample.locate_bounding_box(self, xmin, ymin, xmax, ymax)

    def sel_points(self, data, x, y, dim=None, method=None, out_of_bounds="warn", fill_value=np.nan, tolerance=None):
        """Values of ``data`` (..., n) along ``dim`` (default: faces) at the points ``(x[i], y[i])`` (ugridbase.py:1125-1259)
        -> ``(values (..., n_sel), index (n_sel,), x, y)``.  Containment (``locate_points`` with ``tolerance``) decides which
        points are in bounds.  Face data takes the containing face, or the nearest centroid with ``method="nearest"``; node
        and edge data always take the nearest entity.  ``out_of_bounds``: "raise", "warn" / "ignore" (``fill_value``, a
        scalar, at those points) or "drop" (``index`` then tells which of the caller's points remain).  numpy in -> numpy
        out, device array in -> float64 device array out; the gather runs on the device."""
        return sample.sel_points(self, data, x, y, dim, method, out_of_bounds, fill_value, tolerance)

    def sel(self, data, x=None, y=None, dim=None, return_grid=False):
        """Selection in x and y (ugridbase.py:1462-1506): scalars, lists, arrays or slices with a step give orthogonal points
        through ``sel_points``; a slice without step paired with one value gives a line across the grid's bounds
        (``intersect_line``); two slices give the faces whose centroid lies in the box, open ends taken from the grid's
        bounds -> ``(values (..., n_sel), face_index)``.  ``return_grid``: a box selection also returns the sub-grid of those
        faces, ``(values, face_index, grid)``, as the reference does; points and lines have none and raise ``ValueError``."""
        return sample.sel(self, data, x, y, dim, return_grid)

    def intersect_line(self, data, start, end):
        """Values of face data (..., n_face) in the faces the line from ``start`` to ``end`` crosses (ugridbase.py:1345-1378)
        -> ``(values (..., n_piece), face_index, x, y, s)`` ordered by ``s``, the distance of each piece's midpoint
        ``(x, y)`` from ``start``.  A torch tensor in gives tensors out."""
        return sample.intersect_line(self, data, start, end)

    def intersect_linestring(self, data, xy):
        """``intersect_line`` along the vertices ``xy (n_vertex, 2)`` (ugridbase.py:1412-1460; an array instead of a shapely
        geometry): ``s`` runs along the whole line."""
        return sample.intersect_linestring(self, data, xy)

    # ---- moving data between facets on the device (xugrid_amd/facet.py)
    def to_node(self, data, dim=None, reduce=None):
        """Face or edge data ``(..., n)`` at the nodes (dataarray_accessor.py:346-368): ``(..., n_node, w)`` with NaN where a
        node has fewer contributors, or ``(..., n_node)`` with ``reduce`` in "mean", "sum", "min", "max" (NaN skipped; the
        sum in table order).  ``dim`` names the source facet (default: the one whose size fits).  See xugrid_amd/facet.py."""
        return facet.to_facet(self, "node", data, dim, reduce)

    def to_edge(self, data, dim=None, reduce=None):
        """Node or face data at the edges (dataarray_accessor.py:370-392); see ``to_node``."""
        return facet.to_facet(self, "edge", data, dim, reduce)

    def to_face(self, data, dim=None, reduce=None):
        """Node or edge data at the faces (dataarray_accessor.py:394-416); see ``to_node``."""
        return facet.to_facet(self, "face", data, dim, reduce)

    def facet_width(self, target, source):
        """Width ``w`` of the ``(..., n_target, w)`` result ``to_{target}`` gives for ``source`` data without ``reduce``."""
        return facet.facet_width(self, target, source)

    # ---- face data -> polygons on the device (xugrid_amd/polygonize.py)
    def polygonize(self, data, return_index=False):
        """Regions of equal value of the face data ``data`` (n_face,) as polygons (xugrid.polygonize) ->
        ``(coords, ring_offsets, polygon_offsets, values)``, the ``polygons=`` argument of ``burn_vector_geometry``; with
        ``return_index`` also the polygon of every face (-1 for NaN).  numpy in -> numpy out, device array in -> device
        arrays of the same kind out.  See xugrid_amd/polygonize.py."""
        from .polygonize import polygonize  # (the package attribute of that name is this function, not the module)

        return polygonize(self, data, return_index)

    # ---- sub-meshes cut on the device (xugrid_amd/subset.py, csrc/xr_subset.hip)
    def topology_subset(self, face_index, return_index=False):
        """The grid of the faces ``face_index`` (ugrid2d.py:1138-1216): 1-D integer ids, unique and in any order, or a bool mask
        of length ``n_face``.  The faces keep the order given, the connectivity its width and the caller's vertex order; the
        nodes are the distinct nodes of those faces in ascending old id; coordinates are copied -> a grid of this grid's kind,
        or this grid itself when the selection is every face in order.  ``return_index``: also ``{node_dimension: node_index,
        edge_dimension: edge_index, face_dimension: face_index}``, int64 -- edge ``k`` of the sub-grid is edge
        ``edge_index[k]`` of this one.  Repeated ids raise ``ValueError``, ids outside ``[0, n_face)`` ``IndexError`` (negative
        ids too).  See xugrid_amd/subset.py for the kinds of the results."""
        from . import subset

        return subset.topology_subset(self, face_index, return_index)

    def clip_box(self, xmin, ymin, xmax, ymax):
        """``topology_subset`` of the faces whose centroid lies in the half-open box ``xmin <= x < xmax``, ``ymin <= y < ymax``
        (ugrid2d.py:1218-1226)."""
        from . import subset

        return subset.clip_box(self, xmin, ymin, xmax, ymax)

    def isel(self, indexers=None, return_index=False, data=None, **indexers_kwargs):
        """Selection by node, edge or face ids or masks, keyed by dimension name (ugrid2d.py:1228-1288).  A node selection
        stands for the faces touching any selected node, an edge selection for the faces beside any selected edge; several
        dimensions must stand for the same faces, and a node or edge selection must be exactly the nodes or edges of those
        faces, else ``ValueError``.  -> the sub-grid; with ``return_index`` also the three indexes; with ``data`` ``(..., n)``,
        ``n`` the size of exactly one dimension, also ``data`` gathered along that dimension's index (numpy in -> numpy out,
        device array in -> float64 device array out)."""
        from . import subset

        return subset.isel(self, indexers, return_index, data, **indexers_kwargs)

    # ---- joining and matching grids on the device (xugrid_amd/partition.py, csrc/xr_merge.hip)
    @staticmethod
    def merge_partitions(grids, return_index=False, data=None, dim=None):
        """The grids joined into one (ugrid2d.py ``merge_partitions``, partitioning.py:81-148): nodes whose coordinates compare
        equal as doubles become one node, faces with the same node set one face; of each the first occurrence is kept, in the
        order of the list -> the merged grid (one grid: that grid itself; none: ``ValueError``).  ``return_index``: also
        ``{node_dimension: [...], edge_dimension: [...], face_dimension: [...]}``, per partition the ascending local ids of
        the nodes, edges and faces it contributes.  ``data``: one array ``(..., n_p)`` per partition on one facet (found by
        its size, or named by ``dim``) -> also the merged ``(..., n_merged)`` float64 array.  See xugrid_amd/partition.py for
        the kinds of the results."""
        from . import partition

        return partition.merge_partitions(grids, return_index, data, dim)

    def partition_by_label(self, labels, data=None):
        """One ``topology_subset(index, return_index=True)`` result per label ``0 .. max(labels)`` of the 1-D integer face
        ``labels`` (partitioning.py:71-76); with ``data`` each entry also carries its selection of ``data``."""
        from . import partition

        return partition.partition_by_label(self, labels, data)

    def _partition_points(self):
        """The coordinates the part labels are made from: the centroids, in HBM where the grid lives there."""
        return self.device_mesh.centroids_dev() if self._device_resident else self.centroids

    def label_partitions(self, n_part, weights=None, return_device=False):
        """int64 ``(n_face,)`` labels ``0 .. n_part-1`` of ``n_part`` balanced, connected-leaning parts of the faces
        (ugridbase.py:1528-1571).  The reference asks METIS; here the labels follow the deterministic rule of
        include/xugrid_amd.h (xr_graph_partition_dev): the faces along the Hilbert curve of their centroids are cut into
        runs of equal weight, then at most 16 rounds of moves lower the edge cut of ``face_face_connectivity`` while every
        part stays within 3 % of its share.  ``weights``: integers ``(n_face,)`` >= 0 (default, or all zero: all ones);
        the reference's three errors for a wrong shape, dtype or sign, ``ValueError`` for ``n_part`` outside
        ``[1, n_face]``.  numpy int64 out; an ``engine.DeviceArray`` for a grid whose mesh lives in HBM or with
        ``return_device``; device weights (a torch tensor) give labels of their kind."""
        from . import partition

        return partition.graph_labels(self.n_face, lambda: self._graph("face"), self._partition_points, n_part, weights,
                                      return_device or self._device_resident)

    def partition(self, n_part, weights=None, return_index=False):
        """``label_partitions`` followed by ``partition_by_label`` (ugridbase.py:1573-1596): the list of the parts' grids, of
        this grid's kind, one per label ``0 .. max(labels)`` -- ``n_part`` of them whenever no weight exceeds
        ``sum(weights) / n_part``.  For a grid whose mesh lives in HBM the labels never leave it.  ``return_index``: the
        ``(grid, indexes)`` entries of ``partition_by_label`` instead."""
        entries = self.partition_by_label(self.label_partitions(n_part, weights, return_device=self._device_resident))
        return entries if return_index else [entry[0] for entry in entries]

    def reindex_like(self, other, data, dim=None, tolerance=0.0):
        """``data`` of this grid in the order of ``other`` (ugrid2d.py:1574-1617): the two grids hold the same nodes, edge
        midpoints or centroids -- those of ``data``'s facet, found by its size or named by ``dim`` -- in another order,
        equal, or within ``tolerance`` on both axes.  Raises ``ValueError`` when they do not match one to one."""
        from . import partition

        return partition.reindex_like(self, other, data, dim, tolerance)

    # ---- periodic grids converted on the device (xugrid_amd/periodic.py, csrc/xr_periodic.hip)
    def to_periodic(self, data=None, dim=None, return_index=False):
        """The grid with its rightmost nodes folded onto its leftmost ones (ugrid2d.py:1392-1462): nodes with ``x`` close to
        the grid's largest ``x`` (``np.isclose``) count as ``x = xmin``, nodes that then coincide become one, the first of them
        is kept with the coordinates it HAS (a right node that comes before its left twin keeps ``x = xmax``, as in the
        reference), faces are renumbered with their fill slots left at ``-1``.  The sorted ``y`` of the left and the right
        boundary must be ``np.allclose``, else ``ValueError``.  -> the periodic grid, of this grid's kind; ``return_index``:
        also ``{node_dimension: ..., edge_dimension: ..., face_dimension: ...}``, int64 gather indexes with
        ``data_new = data[..., index]``; ``data`` ``(..., n)`` on one facet (found by its size, or named by ``dim``): also that
        selection.  See xugrid_amd/periodic.py for the kinds of the results."""
        from . import periodic

        return periodic.to_periodic(self, data, dim, return_index)

    def to_nonperiodic(self, xmax, data=None, dim=None, return_index=False):
        """The periodic grid cut open at its seam (ugrid2d.py:1464-1572): a node that a face reaches across more than half the
        width of the grid is copied to ``(xmax, y)``, the copies are appended behind the grid's nodes in ascending order of
        their originals, and those face slots name the copies.  Returns as ``to_periodic``; edge data of an edge on the seam is
        repeated on both sides."""
        from . import periodic

        return periodic.to_nonperiodic(self, xmax, data, dim, return_index)

    # ---- meshes and per-face geometry derived on the device (csrc/xr_mesh_derived.hip: triangulation, circumcenters, perimeter,
    # face bounds; csrc/xr_voronoi.hip: the tessellations)
    _device_resident = False  # True: the mesh exists in HBM only; derived grids stay there and indices are device arrays

    def _derived(self, key, make):
        cache = self.__dict__.setdefault("_derive_cache", {})
        if key not in cache:
            cache[key] = make()
        return cache[key]

    def _grid_from_mesh(self, mesh):
        """A grid of this grid's kind around a mesh that was built on the device."""
        if self._device_resident:
            return DeviceUgrid2d.from_device_mesh(mesh, name=self.name)
        xy, faces = mesh.download()
        grid = Ugrid2d(xy[:, 0], xy[:, 1], FILL_VALUE, faces, name=self.name)
        grid._celltree = CellTree2d.from_device_mesh(mesh)  # (the mesh is in HBM already: no second upload)
        return grid

    def triangulate(self, return_index=False):
        """The fan triangulation of the grid (ugrid2d.py:1650-1662): every face of k nodes becomes the triangles
        ``(n0, n[t + 1], n[t + 2])``, in the caller's vertex order -> a grid of this grid's kind with the same nodes.
        ``return_index`` (not in the reference): also ``triangle_face_connectivity``, the face of every triangle -- numpy for
        a host grid, an int64 device array for a grid whose mesh lives in HBM."""
        triangles = self.device_mesh.triangulate()
        grid = self._grid_from_mesh(triangles)
        if not return_index:
            return grid
        index = triangles.triangle_face_dev()
        return grid, (index if self._device_resident else index.download().astype(IntDType, copy=False))

    @property
    def triangulation(self):
        """``((node_x, node_y, triangles), triangle_face_connectivity)`` as numpy (ugrid2d.py:857-875)."""

        def make():
            triangles = self.device_mesh.triangulate()
            faces = triangles.download()[1].astype(IntDType, copy=False)
            index = triangles.triangle_face_dev().download().astype(IntDType, copy=False)
            return (self.node_x, self.node_y, faces), index

        return self._derived("triangulation", make)

    def _tesselate_voronoi(self, generators, add_exterior, add_vertices, skip_concave):
        from .voronoi import voronoi_topology_device

        mesh, face_index, _ = voronoi_topology_device(self, add_exterior=add_exterior, add_vertices=add_vertices,
                                                      skip_concave=skip_concave, generators=generators)
        return mesh, face_index

    def tesselate_centroidal_voronoi(self, add_exterior=True, add_vertices=True, skip_concave=False):
        """The centroidal Voronoi tessellation of the grid (ugrid2d.py:1686-1708) -> a grid of this grid's kind.  Raises
        ``ValueError`` where the reference crashes (no node with three faces and ``add_exterior=False``) or yields cells of
        two corners."""
        return self._grid_from_mesh(self._tesselate_voronoi(None, add_exterior, add_vertices, skip_concave)[0])

    def tesselate_circumcenter_voronoi(self, add_exterior=True, add_vertices=True, skip_concave=False):
        """... with the circumcenters of the faces as generator points (ugrid2d.py:1710-1732); triangular grids only."""
        if self.n_max_node_per_face != 3:  # (before anything touches the device)
            raise NotImplementedError("Circumcenters are only supported for triangular grids")
        generators = self.device_mesh.circumcenters_dev()
        return self._grid_from_mesh(self._tesselate_voronoi(generators, add_exterior, add_vertices, skip_concave)[0])

    def _voronoi_topology_mesh(self):
        return self._derived("voronoi_mesh", lambda: self._tesselate_voronoi(None, True, False, False))

    @property
    def voronoi_topology(self):
        """``(vertices, faces, face_index)`` of the centroidal tessellation with ``add_exterior=True, add_vertices=False``
        as numpy (ugrid2d.py:810-833)."""

        def make():
            mesh, face_index = self._voronoi_topology_mesh()
            vertices, faces = mesh.download()
            return vertices, faces.astype(IntDType, copy=False), face_index

        return self._derived("voronoi_topology", make)

    @property
    def centroid_triangulation(self):
        """``((x, y, triangles), face_index)``: the triangle mesh over the face centroids (ugrid2d.py:835-855), the
        triangulation kernel run on the tessellation of ``voronoi_topology``."""

        def make():
            mesh, face_index = self._voronoi_topology_mesh()
            vertices, triangles = mesh.triangulate().download()
            return (vertices[:, 0].copy(), vertices[:, 1].copy(), triangles.astype(IntDType, copy=False)), face_index

        return self._derived("centroid_triangulation", make)

    @property
    def circumcenters(self):
        """(n_face, 2) circumcenter of every face; triangular grids only (ugrid2d.py:561-573)."""
        if self.n_max_node_per_face != 3:  # (before anything touches the device)
            raise NotImplementedError("Circumcenters are only supported for triangular grids")
        return self._derived("circumcenters", lambda: self.device_mesh.circumcenters_dev().download())

    @property
    def perimeter(self):
        """(n_face,) perimeter length of every face (ugrid2d.py:586-595)."""
        return self._derived("perimeter", lambda: self.device_mesh.perimeter_dev().download())

    @property
    def face_bounds(self):
        """(n_face, 4) ``minx, miny, maxx, maxy`` of every face (ugrid2d.py:597-619)."""
        return self._derived("face_bounds", lambda: self.device_mesh.face_bounds_dev().download())

    # ---- structured -> unstructured (raster cells become CCW quads)
    @staticmethod
    def _from_intervals_helper(node_x, node_y, nx, ny, name):
        # face id = row-major (y, x) in the bounds' own order; ugrid2d.py:1894-1912
        linear_index = np.arange(node_x.size, dtype=IntDType).reshape((ny + 1, nx + 1))
        face_nodes = np.empty((ny * nx, 4), dtype=IntDType)
        left, right = slice(None, -1), slice(1, None)
        lower, upper = slice(None, -1), slice(1, None)
        if node_x[1] < node_x[0]:
            left, right = right, left
        # NOTE: the reference tests `node_y[ny + 1] < node_y[0]` on the flattened vertex array
        # (ugrid2d.py:1906), which for nx > ny with descending y emits clockwise quads (SURVEY
        # appendix D).  Orientation does not matter downstream (the engine normalises every face
        # to CCW on the device), so the intended test -- first element of the second row -- is used.
        if node_y[nx + 1] < node_y[0]:
            lower, upper = upper, lower
        face_nodes[:, 0] = linear_index[lower, left].ravel()
        face_nodes[:, 1] = linear_index[lower, right].ravel()
        face_nodes[:, 2] = linear_index[upper, right].ravel()
        face_nodes[:, 3] = linear_index[upper, left].ravel()
        return Ugrid2d(node_x, node_y, FILL_VALUE, face_nodes, name=name)

    @staticmethod
    def from_structured_bounds(x_bounds, y_bounds, name="mesh2d", return_index=False):
        """(nx, 2) and (ny, 2) cell bounds -> quad mesh, or the (N, M, 4) corner arrays of a curvilinear grid (CF cell bounds,
        host or device arrays) -> a device-resident mesh of its valid cells; ugrid2d.py:1973-2034.  The corners of a cell may
        come in any order.  A cell with fewer than three distinct corners or no area is left out with a ``UserWarning`` that
        counts them; a cell with a NaN or infinite corner is left out too.  ``return_index``: also which cells became faces --
        ``slice(None, None)`` for 2-D bounds; for 3-D ones a bool ``(N * M,)`` array: numpy for host bounds, a torch tensor for torch
        bounds, a ``DeviceArray`` of dtype bool for other device arrays.  The mesh is
        built on the device (xugrid_amd/geometry.py)."""
        if geometry._ndim(x_bounds) == 3:
            return geometry.from_bounds(x_bounds, y_bounds, name, return_index)
        x_bounds = np.asarray(x_bounds, dtype=FloatDType)
        y_bounds = np.asarray(y_bounds, dtype=FloatDType)
        if x_bounds.ndim != 2 or y_bounds.ndim != 2:
            raise ValueError(f"Expected 2 dimensions on bounds, received: {x_bounds.ndim}")
        nx, ny = x_bounds.shape[0], y_bounds.shape[0]
        x = connectivity.bounds1d_to_vertices(x_bounds)
        y = connectivity.bounds1d_to_vertices(y_bounds)
        node_y, node_x = (a.ravel() for a in np.meshgrid(y, x, indexing="ij"))
        grid = Ugrid2d._from_intervals_helper(node_x, node_y, nx, ny, name)
        return (grid, slice(None, None)) if return_index else grid

    @staticmethod
    def from_structured_intervals1d(x_intervals, y_intervals, name="mesh2d"):
        """(M + 1,) and (N + 1,) interval values -> the rectilinear quad mesh, generated on the device; ugrid2d.py:1915-1938."""
        return geometry.from_intervals1d(x_intervals, y_intervals, name)

    @staticmethod
    def from_structured_intervals2d(x_intervals, y_intervals, name="mesh2d"):
        """(N + 1, M + 1) node coordinates of a curvilinear lattice (host or device arrays) -> a device-resident quad mesh,
        numbered and oriented as ``_from_intervals_helper`` does; ugrid2d.py:1941-1971."""
        return geometry.from_intervals2d(x_intervals, y_intervals, name)

    @staticmethod
    def from_structured(x, y, name="mesh2d"):
        """Cell CENTRE coordinates -> mesh; ugrid2d.py:2036-2150 on arrays.  1-D ``x`` (M,) and ``y`` (N,): the rectilinear mesh
        of the inferred breaks.  2-D ``x`` and ``y`` (N, M) of a rotated or curvilinear grid: breaks along axis 1, then axis 0
        (``infer_interval_breaks``), then ``from_structured_intervals2d``.  A non-monotonic coordinate raises ``ValueError``."""
        return geometry.from_structured(x, y, name)

    @staticmethod
    def from_polygons(polygons, name="mesh2d"):
        """Polygons as coordinate arrays -> mesh: ``from_shapely`` (ugrid2d.py:1867-1892, ``conversion.polygons_to_faces``)
        without shapely.  ``polygons``: ``(coords (V, 2), ring_offsets)`` or what ``polygonize`` returns.  Every ring loses its
        closing vertex, the nodes are the sorted unique vertices, faces keep ring and vertex order.  Holes, open rings and rings
        of fewer than four vertices raise ``ValueError``."""
        return geometry.from_polygons(polygons, name)

    def to_polygons(self):
        """-> ``(coords, ring_offsets, polygon_offsets)``: every face as one closed ring (``conversion.faces_to_polygons``),
        numpy for a host grid, ``DeviceArray`` for a device-resident one."""
        return geometry.to_polygons(self)

    def bounding_polygon(self):
        """-> ``(coords, ring_offsets)`` of the grid's outline, holes included: of the polygons ``polygonize`` traces for a
        constant field the one with the largest bounding box, the first among equals (ugrid2d.py:2192-2205)."""
        return geometry.bounding_polygon(self)

    @staticmethod
    def from_structured_bounds_device(x_bounds, y_bounds, name="mesh2d"):
        """``from_structured_bounds`` with the mesh generated on the device: only the two 1-D vertex arrays are
        uploaded; the host copies of the node and face arrays are made on first access (persistence, host
        connectivities), never for regridding."""
        x_bounds = np.asarray(x_bounds, dtype=FloatDType)
        y_bounds = np.asarray(y_bounds, dtype=FloatDType)
        if x_bounds.ndim != 2 or y_bounds.ndim != 2:
            raise ValueError(f"Expected 2 dimensions on bounds, received: {x_bounds.ndim}")
        return RectilinearUgrid2d(
            connectivity.bounds1d_to_vertices(x_bounds), connectivity.bounds1d_to_vertices(y_bounds), name
        )

    # ---- persistence (plain dict of arrays; xarray is optional and absent here)
    def to_dataset(self, prefix=None):
        name = prefix if prefix is not None else self.name
        return {
            f"{name}_node_x": self.node_x,
            f"{name}_node_y": self.node_y,
            f"{name}_face_nodes": self.face_node_connectivity,
        }

    @staticmethod
    def from_device_arrays(node_coordinates, face_node_connectivity, fill_value=FILL_VALUE, name="mesh2d"):
        """A grid whose arrays ALREADY live in HBM: ``node_coordinates`` float64 ``(n_node, 2)`` and ``face_node_connectivity``
        int64 / int32 ``(n_face, n_max_node_per_face)`` as torch tensors on the GPU or anything with ``__cuda_array_interface__``
        (cupy, numba, ``engine.DeviceArray``).  Nothing crosses PCIe: the device mesh is made from the pointers
        (xr_mesh_create_dev validates and copies), the host arrays of the base class are downloaded only if somebody reads
        them.  (The reference has host grids only, ugrid2d.py:72-110; this is how its classes reach data a GPU pipeline
        already holds.)"""
        return DeviceUgrid2d(node_coordinates, face_node_connectivity, fill_value, name)

    @staticmethod
    def from_dataset(dataset, name):
        return Ugrid2d(
            np.asarray(dataset[f"{name}_node_x"]),
            np.asarray(dataset[f"{name}_node_y"]),
            FILL_VALUE,
            np.asarray(dataset[f"{name}_face_nodes"]),
            name=name,
        )


class RectilinearUgrid2d(Ugrid2d):
    """The quads of a rectilinear grid (``Ugrid2d.from_structured_bounds``, ugrid2d.py:1973-2034) whose node and
    face arrays exist on the DEVICE only: ``xr_mesh_create_rectilinear`` generates them from the two 1-D vertex
    arrays.  The host arrays of the base class are materialised lazily, on the first access of ``node_x`` /
    ``node_y`` / ``face_node_connectivity`` (persistence, host-side connectivities)."""

    def __init__(self, x_vertices, y_vertices, name="mesh2d"):
        self._xv = np.ascontiguousarray(x_vertices, dtype=FloatDType)
        self._yv = np.ascontiguousarray(y_vertices, dtype=FloatDType)
        if self._xv.ndim != 1 or self._yv.ndim != 1 or self._xv.size < 2 or self._yv.size < 2:
            raise ValueError("a rectilinear grid needs at least one cell per axis")
        self._host = None
        self.fill_value = FILL_VALUE
        self.start_index = 0
        self.name = name
        self._celltree = None
        self._area = None
        self._centroids = None
        self._edge_node_connectivity = None
        self._face_edge_connectivity = None
        self._edge_face_connectivity = None
        self._node_face_connectivity = None

    _device_resident = True

    def _materialise(self):
        if self._host is None:
            node_y, node_x = (a.ravel() for a in np.meshgrid(self._yv, self._xv, indexing="ij"))
            self._host = Ugrid2d._from_intervals_helper(node_x, node_y, self._xv.size - 1, self._yv.size - 1, self.name)
        return self._host

    node_x = property(lambda self: self._materialise().node_x)
    node_y = property(lambda self: self._materialise().node_y)
    node_coordinates = property(lambda self: self._materialise().node_coordinates)
    _node_xy = property(lambda self: self._materialise()._node_xy)
    face_node_connectivity = property(lambda self: self._materialise().face_node_connectivity)

    @property
    def n_node(self):
        return self._xv.size * self._yv.size

    @property
    def n_face(self):
        return (self._xv.size - 1) * (self._yv.size - 1)

    @property
    def n_max_node_per_face(self):
        return 4

    @property
    def bounds(self):
        return (self._xv.min(), self._yv.min(), self._xv.max(), self._yv.max())

    def node_coordinates_of(self, nodes):
        nodes = np.asarray(nodes)
        j, i = np.divmod(nodes, self._xv.size)  # node id = j * (nx + 1) + i (meshgrid order)
        return np.column_stack([self._xv[i], self._yv[j]])

    @property
    def celltree(self) -> CellTree2d:
        if self._celltree is None:
            from .engine import DeviceMesh

            self._celltree = CellTree2d.from_device_mesh(DeviceMesh.from_rectilinear(self._xv, self._yv))
        return self._celltree


class DeviceUgrid2d(Ugrid2d):
    """``Ugrid2d.from_device_arrays``: the mesh exists on the device; host copies are made lazily (see RectilinearUgrid2d)."""

    def __init__(self, node_coordinates, face_node_connectivity, fill_value=FILL_VALUE, name="mesh2d"):
        from . import engine

        xy = engine.device_array_info(node_coordinates)
        faces = engine.device_array_info(face_node_connectivity)
        if xy is None or faces is None:
            raise TypeError("from_device_arrays expects device arrays (torch tensors on the GPU or __cuda_array_interface__)")
        (xy_ptr, xy_shape, xy_dtype), (f_ptr, f_shape, f_dtype) = xy, faces
        if len(xy_shape) != 2 or xy_shape[1] != 2 or xy_dtype != np.float64:
            raise ValueError("node_coordinates must be a float64 (n_node, 2) device array")
        if len(f_shape) != 2 or f_dtype not in (np.dtype(np.int64), np.dtype(np.int32)):
            raise ValueError("face_node_connectivity must be an int64 / int32 (n_face, n_max_node_per_face) device array")
        engine.sync_producer(node_coordinates)
        engine.sync_producer(face_node_connectivity)
        mesh = engine.DeviceMesh.from_device(xy_ptr, xy_shape[0], f_ptr, f_dtype.itemsize, f_shape[0], f_shape[1], fill_value)
        self._init_from_mesh(mesh, name)

    def _init_from_mesh(self, mesh, name):
        self._n_node, self._n_face, self._m = mesh.n_node, mesh.n_face, mesh.n_max_node
        self._host = None
        self.fill_value = FILL_VALUE
        self.start_index = 0
        self.name = name
        self._celltree = CellTree2d.from_device_mesh(mesh)
        self._voronoi_device_cache = None
        self._area = None
        self._centroids = None
        self._edge_node_connectivity = None
        self._face_edge_connectivity = None
        self._edge_face_connectivity = None
        self._node_face_connectivity = None

    _device_resident = True

    @classmethod
    def from_device_mesh(cls, mesh, name="mesh2d"):
        """A grid around an existing ``engine.DeviceMesh`` (one built on the device: a triangulation, a tessellation)."""
        self = cls.__new__(cls)
        self._init_from_mesh(mesh, name)
        return self

    def _materialise(self):
        if self._host is None:
            xy, faces = self._celltree.device_mesh.download()
            self._host = Ugrid2d(xy[:, 0], xy[:, 1], FILL_VALUE, faces, name=self.name)
        return self._host

    node_x = property(lambda self: self._materialise().node_x)
    node_y = property(lambda self: self._materialise().node_y)
    node_coordinates = property(lambda self: self._materialise().node_coordinates)
    _node_xy = property(lambda self: self._materialise()._node_xy)
    face_node_connectivity = property(lambda self: self._materialise().face_node_connectivity)
    n_node = property(lambda self: self._n_node)
    n_face = property(lambda self: self._n_face)
    n_max_node_per_face = property(lambda self: self._m)
    bounds = property(lambda self: self._materialise().bounds)

    def node_coordinates_of(self, nodes):
        return self._materialise().node_coordinates_of(nodes)

    @property
    def celltree(self) -> CellTree2d:
        return self._celltree

    def drop_device_caches(self):
        # (the device mesh IS this grid: its derived arrays and index go, the raw arrays stay)
        self._voronoi_device_cache = None
        self.__dict__.pop("_fill_cache", None)
        self.__dict__.pop("_sample_cache", None)
        self.__dict__.pop("_topology_cache", None)
        self.__dict__.pop("_facet_cache", None)
        self.__dict__.pop("_derive_cache", None)
        self._celltree.device_mesh.invalidate()

    # ---- edge connectivity from the device topology.  An edge with more than two faces does not fit its two-column tables: such
    # a grid takes the host route of the base class (download the mesh, numpy), exactly as before.
    def _fill_topology(self):
        topology = self.device_topology()
        return topology if topology.manifold else None

    def _from_topology(name):  # noqa: N805  (property factory, used in the class body only)
        def get(self):
            topology = self._fill_topology()
            if topology is None:
                return getattr(Ugrid2d, name).fget(self)
            return getattr(topology, name)

        return property(get, doc=getattr(Ugrid2d, name).__doc__)

    edge_node_connectivity = _from_topology("edge_node_connectivity")
    face_edge_connectivity = _from_topology("face_edge_connectivity")
    edge_face_connectivity = _from_topology("edge_face_connectivity")  # (always two columns; the host table has one when no edge is shared)
    face_face_connectivity = _from_topology("face_face_connectivity")
    node_node_connectivity = _from_topology("node_node_connectivity")
    node_face_connectivity = _from_topology("node_face_connectivity")  # (from the device: the mesh is not downloaded)
    node_edge_connectivity = _from_topology("node_edge_connectivity")
    exterior_edges = _from_topology("exterior_edges")
    exterior_faces = _from_topology("exterior_faces")
    del _from_topology

    @property
    def n_edge(self):
        topology = self._fill_topology()
        return topology.n_edge if topology is not None else Ugrid2d.n_edge.fget(self)

    @property
    def edge_coordinates(self):
        topology = self._fill_topology()
        if topology is None:
            return Ugrid2d.edge_coordinates.fget(self)
        return topology.edge_coordinates_device().download()

    def _edge_points(self):
        topology = self._fill_topology()
        return topology.edge_coordinates_device() if topology is not None else self.edge_coordinates

    def _exterior_face_flags(self):
        topology = self._fill_topology()
        return topology.exterior_face_flags_device() if topology is not None else Ugrid2d._exterior_face_flags(self)
