"""
``Ugrid1d``: a network of line segments -- the part of xugrid/ugrid/ugrid1d.py:65-111 and ugridbase.py the
NetworkGridder path reads: the constructor arguments ``(node_x, node_y, fill_value, edge_node_connectivity)``,
``n_node`` / ``n_edge``, ``node_coordinates``, ``edge_node_coordinates`` (ugridbase.py:611-614) and ``edge_length``
(:955-959), and the topology editing of xugrid_amd/netedit.py.  UGRID IO, CRS handling and the depth-first graph walks of the
reference class are outside (out of scope).
"""
import numpy as np

from . import connectivity, engine, facet, fill, netedit, sample, snap
from .engine import FloatDType, IntDType

FILL_VALUE = -1


class Ugrid1d:
    def __init__(self, node_x, node_y, fill_value, edge_node_connectivity, name="network1d", start_index=0):
        self.node_x = np.ascontiguousarray(node_x, dtype=FloatDType)
        self.node_y = np.ascontiguousarray(node_y, dtype=FloatDType)
        if self.node_x.ndim != 1 or self.node_x.shape != self.node_y.shape:
            raise ValueError("node_x and node_y must be 1-D arrays of equal length")
        self.fill_value = fill_value
        self.start_index = start_index
        edges = np.asarray(edge_node_connectivity)
        if edges.ndim != 2 or edges.shape[1] != 2:
            raise ValueError("edge_node_connectivity must have shape (n_edge, 2)")
        if not np.issubdtype(edges.dtype, np.integer):
            raise TypeError("edge_node_connectivity must be an integer array")
        edges = edges.astype(IntDType) - start_index
        if edges.size and (edges.min() < 0 or edges.max() >= self.node_x.size):
            raise ValueError("edge_node_connectivity refers to nodes that do not exist")
        self.edge_node_connectivity = np.ascontiguousarray(edges)
        self.name = name

    @staticmethod
    def from_lines(lines, name="network1d"):
        """Lines as coordinate arrays ``(coords (V, 2), line_offsets)`` -> network: ``conversion.linestrings_to_edges`` without
        shapely, on the device.  An edge joins every two consecutive vertices of a line; the nodes are the sorted unique
        vertices."""
        from . import geometry

        return geometry.from_lines(lines, name)

    def to_lines(self):
        """-> ``(coords (2 n_edge, 2), line_offsets)``: one two-vertex line per edge."""
        from . import geometry

        return geometry.to_lines(self)

    # ---- ugridbase.py:560-614, :955-959
    @property
    def n_node(self) -> int:
        return self.node_x.size

    @property
    def n_edge(self) -> int:
        return self.edge_node_connectivity.shape[0]

    @property
    def node_dimension(self):
        return f"{self.name}_nNodes"

    @property
    def edge_dimension(self):
        return f"{self.name}_nEdges"

    @property
    def core_dimension(self):
        return self.edge_dimension

    @property
    def dims(self):
        return (self.edge_dimension,)

    @property
    def node_coordinates(self):
        return np.column_stack([self.node_x, self.node_y])

    @property
    def edge_node_coordinates(self):
        """Node coordinates of every edge, shape ``(n_edge, 2, 2)``."""
        return self.node_coordinates[self.edge_node_connectivity]

    @property
    def edge_length(self):
        d = np.diff(self.edge_node_coordinates, axis=1)[:, 0, :]
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])

    @property
    def edge_coordinates(self):
        """(n_edge, 2) edge midpoints."""
        xy = self.edge_node_coordinates
        return 0.5 * (xy[:, 0] + xy[:, 1])

    @property
    def node_node_connectivity(self):
        """Nodes joined by an edge, scipy CSR; data = the edge's id."""
        return connectivity.node_node_connectivity(self.edge_node_connectivity, self.n_node)

    @property
    def node_edge_connectivity(self):
        """node -> edge, scipy CSR over all nodes, edges ascending per row (ugridbase.py:866-878)."""
        return facet.node_edge_connectivity(self.edge_node_connectivity, self.n_node)

    @property
    def edge_edge_connectivity(self):
        """Edges that share a node, scipy CSR (n_edge, n_edge), columns ascending; data = the shared node
        (connectivity.py:534-551)."""
        return connectivity.edge_edge_connectivity(self.edge_node_connectivity, self.node_edge_connectivity)

    # ---- moving data between nodes and edges on the device (xugrid_amd/facet.py; the Ugrid2d methods of the same name)
    def to_node(self, data, dim=None, reduce=None):
        """Edge data ``(..., n_edge)`` at the nodes: ``(..., n_node, w)``, or ``(..., n_node)`` with ``reduce``; see
        ``Ugrid2d.to_node``."""
        return facet.to_facet(self, "node", data, dim, reduce)

    def to_edge(self, data, dim=None, reduce=None):
        """Node data at the edges: ``(..., n_edge, 2)``, or ``(..., n_edge)`` with ``reduce``."""
        return facet.to_facet(self, "edge", data, dim, reduce)

    def to_face(self, data, dim=None, reduce=None):
        """A network has no faces: raises, as the reference's ``_to_facet`` does."""
        return facet.to_facet(self, "face", data, dim, reduce)

    def facet_width(self, target, source):
        """Width ``w`` of the ``(..., n_target, w)`` result of ``to_node`` / ``to_edge`` without ``reduce``."""
        return facet.facet_width(self, target, source)

    def get_connectivity_matrix(self, dim="node", xy_weights=True):
        """ugrid1d.py:334-345: the node adjacency; with ``xy_weights`` its data are mean(d) / d of the node distances."""
        facet = fill.resolve_dim(self, dim, ("node",))
        conn = self.node_node_connectivity
        if xy_weights:
            conn.data = fill.connectivity_weights(conn, self.node_coordinates)
        return conn

    # ---- filling NaN entries on the device (xugrid_amd/fill.py; the Ugrid2d methods of the same name)
    def _fill(self):
        cache = self.__dict__.get("_fill_cache")
        if cache is None:
            cache = self.__dict__["_fill_cache"] = fill.GridFill()
        return cache

    def laplace_interpolate(self, data, dim="node", xy_weights=True, direct_solve=False, delta=0.0, relax=0.0, rtol=0.0,
                            atol=1e-4, maxiter=500):
        """Laplace fill of node data (..., n_node) on the device; see ``Ugrid2d.laplace_interpolate``."""
        facet = fill.resolve_dim(self, dim, ("node", "edge"))
        if facet == "edge":
            raise ValueError("Laplace interpolation along edges is not allowed.")
        fill._check_ilu_options(delta, relax)
        graph = self._fill().graph("node", lambda: self.node_node_connectivity, lambda: self.node_coordinates)
        return fill.laplace_fill(graph, data, xy_weights, direct_solve, delta, relax, atol, rtol, maxiter)

    def interpolate_na(self, data, dim=None, method="nearest", max_distance=None, metric="euclidean"):
        """Nearest fill of node or edge data (default: edges).

        ``metric="euclidean"`` (the default): the nearest node or edge midpoint in the plane, strictly closer than
        ``max_distance``; see ``Ugrid2d.interpolate_na``.

        ``metric="network"``: the reference's rule for a ``Ugrid1d`` (ugrid1d.py ``_nearest_interpolate``) -- the nearest value
        measured ALONG the edges: between nodes the edge lengths, between edges half of the two edge lengths (midpoint to
        midpoint through the shared node).  Across a meander or between two parallel branches that is another reach than the
        Euclidean neighbour.  ``max_distance`` is INCLUSIVE here (scipy's dijkstra ``limit``): an entry at exactly that distance
        is filled.  Among equidistant values the one with the lowest id is taken.  Entries in a part of the network without any
        value stay NaN.  A network with self-loops or repeated edges raises ``ValueError``.

        ``max_distance=None`` is no limit; a negative one, or an unknown ``metric``, raises ``ValueError`` before the device is
        touched."""
        if method != "nearest":
            raise ValueError(f'"{method}" is not a valid interpolator.')
        if metric not in ("euclidean", "network"):
            raise ValueError(f'metric must be "euclidean" or "network", received: {metric!r}')
        fill._limit(max_distance)
        facet = fill.resolve_dim(self, dim, ("node", "edge"))
        if metric == "network":
            return fill.network_fill(fill.network_graph(self, facet), data, max_distance)
        coords = (lambda: self.node_coordinates) if facet == "node" else (lambda: self.edge_coordinates)
        return fill.nearest_fill(self._fill().xy(facet, coords), data, max_distance)

    def network_distance(self, sources, dim=None, max_distance=None):
        """Distance along the network to the nearest of ``sources`` (gauges, outlets) and which one it is:
        ``(distance (n,) float64, source_index (n,) int64)`` over the nodes or edges of ``dim`` (default: edges), ``inf`` / ``-1``
        where none is within ``max_distance`` (inclusive; None: no limit).  ``sources``: unique ids, or a bool mask of the
        dimension's length.  Host arrays in -> numpy out; torch tensors on the GPU in -> torch tensors out.  The metric and the
        tie rule are those of ``interpolate_na(metric="network")``."""
        fill._limit(max_distance)
        facet = fill.resolve_dim(self, dim, ("node", "edge"))
        n = self.n_node if facet == "node" else self.n_edge
        if engine.is_torch(sources) and getattr(sources, "is_cuda", False):
            import torch

            if sources.dtype == torch.bool:
                if tuple(sources.shape) != (n,):
                    raise ValueError(f"expected a mask of shape ({n},), received: {tuple(sources.shape)}")
                mask = sources.to(torch.uint8).contiguous()
            else:
                ids = sources.reshape(-1).long()
                if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
                    raise ValueError(f"sources must be ids in [0, {n})")
                if torch.unique(ids).numel() != ids.numel():
                    raise ValueError("sources must be unique ids")
                mask = torch.zeros(n, dtype=torch.uint8, device=sources.device)
                mask[ids] = 1
        else:
            a = np.asarray(sources.cpu() if engine.is_torch(sources) else sources)
            if a.dtype == np.bool_:
                if a.shape != (n,):
                    raise ValueError(f"expected a mask of shape ({n},), received: {a.shape}")
                mask = a
            else:
                if not np.issubdtype(a.dtype, np.integer):
                    raise TypeError("sources must be integer ids or a bool mask")
                ids = a.reshape(-1)
                if ids.size and (ids.min() < 0 or ids.max() >= n):
                    raise ValueError(f"sources must be ids in [0, {n})")
                if np.unique(ids).size != ids.size:
                    raise ValueError("sources must be unique ids")
                mask = np.zeros(n, dtype=np.bool_)
                mask[ids] = True
        return fill.network_nearest(fill.network_graph(self, facet), mask, max_distance)

    # ---- nearest node / edge on the device (xugrid_amd/sample.py; the Ugrid2d methods of the same name)
    def _nearest_index(self, facet):
        cache = self.__dict__.get("_sample_cache")
        if cache is None:
            cache = self.__dict__["_sample_cache"] = sample.GridSample()
        coords = (lambda: self.node_coordinates) if facet == "node" else (lambda: self.edge_coordinates)
        return cache.index(facet, lambda: sample.NearestIndex.from_points(coords()))

    def locate_nearest_node(self, points, max_distance=np.inf):
        """Index of the nearest node per point ``(n_point, 2)``, -1 for none (ugridbase.py:1261-1281); see
        ``Ugrid2d.locate_nearest_node``."""
        return self._nearest_index("node").query(points, max_distance)

    def locate_nearest_edge(self, points, max_distance=np.inf):
        """Index of the nearest edge midpoint per point, -1 for none (ugridbase.py:1283-1303)."""
        return self._nearest_index("edge").query(points, max_distance)

    # ---- editing the network on the device (xugrid_amd/netedit.py, csrc/xr_netedit.hip)
    def topology_subset(self, edge_index, return_index=False):
        """ugrid1d.py:603-663: the network of the edges ``edge_index`` (unique ids in any order, or a bool mask of length
        ``n_edge``; host or device) in the order given; its nodes are the end nodes of those edges in ascending old id.  Every
        edge in order gives the grid itself.  ``return_index``: also ``{node_dimension: .., edge_dimension: ..}``, int64 (numpy,
        or device arrays of the indexer's kind).  Ids outside ``[0, n_edge)`` raise ``IndexError`` (negative ones too),
        repeated ids ``ValueError``."""
        return netedit.topology_subset(self, edge_index, return_index)

    def isel(self, indexers=None, return_index=False, data=None, dim=None, **indexers_kwargs):
        """ugridbase.py:703-720: the sub-network of an indexer per UGRID dimension (node and / or edge).  A node indexer stands
        for the edges with at least one end in it; all indexers must stand for the same edges ("UGRID dimensions do not align")
        and a node indexer must be exactly the ascending nodes of the result ("results in an invalid topology").  ``data``
        ``(..., n)`` on one dimension comes back indexed alongside; ``dim`` names that dimension where ``n_node == n_edge`` (a
        ring) leaves it open.  -> grid [, indexes] [, data]."""
        return netedit.isel(self, indexers, return_index, data, dim, **indexers_kwargs)

    def sel(self, x=None, y=None, data=None, return_index=False, dim=None):
        """ugrid1d.py:574-601: the edges whose midpoint lies in the half-open box of two slices (no steps).  A ``None`` slice or
        bound is unbounded on that side (an addition).  -> grid [, indexes] [, data]."""
        return netedit.sel(self, x, y, data, return_index, dim)

    def clip_box(self, xmin, ymin, xmax, ymax):
        """ugrid1d.py:665-672: ``sel(x=slice(xmin, xmax), y=slice(ymin, ymax))``."""
        return netedit.clip_box(self, xmin, ymin, xmax, ymax)

    def remove_self_loops(self, return_index=False):
        """ugrid1d.py:714-738: the network without the edges that join a node to itself.  Always a NEW grid, whose nodes are
        exactly those the kept edges use.  ``return_index``: also the node and edge index."""
        return netedit.remove_self_loops(self, return_index)

    def label_partitions(self, n_part, weights=None, return_device=False):
        """int64 ``(n_edge,)`` labels ``0 .. n_part-1`` of ``n_part`` balanced parts of the edges, the core dimension
        (ugridbase.py:1528-1571): the rule of ``Ugrid2d.label_partitions`` on ``edge_edge_connectivity`` and the edge
        midpoints.  numpy out, an ``engine.DeviceArray`` with ``return_device``, device weights give labels of their kind."""
        from . import partition

        return partition.graph_labels(self.n_edge, lambda: partition.canonical_graph(self.edge_edge_connectivity),
                                      lambda: self.edge_coordinates, n_part, weights, return_device)

    def partition(self, n_part, weights=None):
        """ugridbase.py:1573-1596: ``topology_subset`` of the edges of every label of ``label_partitions``."""
        from . import partition

        return [self.topology_subset(ids) for ids in partition.labels_to_indices(self.label_partitions(n_part, weights))]

    @staticmethod
    def merge_partitions(grids, return_index=False, data=None, dim=None):
        """partitioning.py:81-116, :137-148: the networks joined into one.  Nodes whose coordinates compare equal as doubles are
        one node (first occurrence kept, bit for bit, in concatenation order); edges with the same (lower, higher) node pair are
        one edge (first occurrence kept with its orientation).  One grid gives that grid itself.  ``return_index``: per
        dimension a list with every partition's ascending local ids of its kept nodes / edges; ``data``: one array
        ``(..., n_p)`` per partition on one dimension -> the merged data.  -> grid [, indexes] [, data]."""
        return netedit.merge_partitions(grids, return_index, data, dim)

    def reindex_like(self, other, data, dim=None, tolerance=0.0):
        """``data`` ``(..., n)`` of this grid in the node or edge order of ``other``, the same network numbered differently:
        nodes are matched by their coordinates, edges by their midpoints (``partition.index_like_device``); a mismatch raises
        ``ValueError``."""
        return netedit.reindex_like(self, other, data, dim, tolerance)

    def refine_by_vertices(self, vertices, return_index=False, tolerance=None, data=None):
        """ugrid1d.py:770-876: every vertex ``(n, 2)`` (host or float64 device array) becomes a node of the edge it lies on, the
        edge is split there.  A vertex lies on an edge when its distance to the closed segment is ``<= tolerance`` (None:
        ``1e-9`` times the larger side of the node bounding box; the lowest edge id wins); a vertex on no edge raises
        ``ValueError`` listing those vertices.  Vertices that equal an existing node are dropped, vertices that equal one
        another are all inserted.  New nodes follow the old ones in the order given, unprojected.  ``return_index``: the new
        ids ordered by edge, then distance from the edge's first node.  ``data``: edge data ``(..., n_edge)`` repeated onto the
        new edges (an addition; node data raises ``ValueError``).  -> grid [, node_index] [, data]."""
        return netedit.refine_by_vertices(self, vertices, return_index, tolerance, data)

    # ---- snapping (xugrid_amd/snap.py, csrc/xr_snap.hip)
    def snap_to_nodes(self, x, y, max_distance, tiebreaker=None, return_index=False):
        """``xugrid_amd.snap_to_nodes`` (snapping.py:146-219) with this network's nodes as the targets, through its cached
        node index; see ``Ugrid2d.snap_to_nodes``."""
        return snap.grid_snap_to_nodes(self, x, y, max_distance, tiebreaker, return_index)

    def snap_nodes(self, max_snap_distance, return_index=False):
        """``xugrid_amd.snap_nodes`` (snapping.py:86-143) on this network's nodes: nodes within ``max_snap_distance`` of each
        other become one node and ``edge_node_connectivity`` is ``inverse[edges]``, gathered on the device.  Every edge is
        kept, so edges may become self-loops (``remove_self_loops`` drops them) or repeat one another.  The grid itself comes
        back when no two nodes lie within the distance.  ``return_index``: also ``{node_dimension: inverse}``, int64
        ``(n_node,)`` the new id of every old node, None for the identity."""
        return snap.network_snap_nodes(self, max_snap_distance, return_index)

    def drop_device_caches(self):
        """Release what this grid keeps in HBM: the fills' graphs (the network graphs of ``metric="network"`` among them) and
        point arrays, the nearest-neighbour indices (built from the coordinates as they were on first use) and the copy of the
        nodes and edges the edits read."""
        self.__dict__.pop("_netedit_cache", None)
        self.__dict__.pop("_fill_cache", None)
        self.__dict__.pop("_sample_cache", None)
        self.__dict__.pop("_facet_cache", None)

    @property
    def bounds(self):
        return float(self.node_x.min()), float(self.node_y.min()), float(self.node_x.max()), float(self.node_y.max())

    def __eq__(self, other):
        return (
            isinstance(other, Ugrid1d)
            and np.array_equal(self.node_x, other.node_x)
            and np.array_equal(self.node_y, other.node_y)
            and np.array_equal(self.edge_node_connectivity, other.edge_node_connectivity)
        )

    __hash__ = None

    # ---- persistence (plain dict of arrays, as Ugrid2d.to_dataset)
    def to_dataset(self, prefix=None):
        name = prefix if prefix is not None else self.name
        return {
            f"{name}_node_x": self.node_x,
            f"{name}_node_y": self.node_y,
            f"{name}_edge_nodes": self.edge_node_connectivity,
        }

    @staticmethod
    def from_dataset(dataset, name):
        return Ugrid1d(
            np.asarray(dataset[f"{name}_node_x"]),
            np.asarray(dataset[f"{name}_node_y"]),
            FILL_VALUE,
            np.asarray(dataset[f"{name}_edge_nodes"]),
            name=name,
        )
