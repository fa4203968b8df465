/*
 * xugrid_amd.h -- C ABI of the MI355X-native regridding engine (libxugrid_amd.so).
 *
 * This is the drop-in boundary for ONE hot path of Deltares/xugrid 0.15.3: regridding weight
 * construction + sparse weight x data apply.  xugrid has no FFI of its own;
 * the path sits behind three Python seams, and every entry point below names the seam it
 * replaces (paths relative to the reference tree):
 *
 *   seam 1  the tree object returned by Ugrid2d.celltree        xugrid/ugrid/ugrid2d.py:908-921
 *           (external numba_celltree.CellTree2d) and its methods
 *             .intersect_faces(vertices, faces, fill_value)     xugrid/regrid/unstructured.py:124-132
 *             .locate_points(points, tolerance)                 xugrid/regrid/unstructured.py:139,189
 *             .compute_barycentric_weights(points, tolerance)   xugrid/ugrid/ugrid2d.py:1078
 *   seam 2  the apply callable  self._regrid(source(K,S), A, size)  xugrid/regrid/regridder.py:41-67,
 *           looked up at :124-141, invoked at :187; COO variant :400-409
 *   seam 3  MatrixCSR.from_triplet(target, source, w, n, m)     xugrid/regrid/regridder.py:433-435,
 *           xugrid/core/sparse.py:61-78,119-127
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns an int
 *     status: 0 = ok, < 0 = error (message via xr_last_error(), thread-local).  No exception or
 *     abort crosses the boundary.
 *   - Host arrays are caller-owned numpy-style buffers: float64 coordinates/weights, int64
 *     indices (np.intp, xugrid/constants.py:10), fill value -1 after ingestion.
 *     On the device the engine keeps int32 connectivity/indices and float64 geometry.
 *   - Functions with the suffix _dev take DEVICE pointers (HBM addresses on the current device,
 *     e.g. torch tensor .data_ptr()) and do no host transfer; they run on the engine stream and
 *     synchronise it before returning unless stated otherwise.
 *   - Handles (xr_mesh, xr_csr) own HBM; they are not tied to a host thread.  Re-entrancy (dask calls
 *     the apply seam from several threads, regridder.py:177-185): the apply entry points
 *     xr_apply_csr[_dev], which only READ a weight matrix, run concurrently, each calling thread on a
 *     HIP stream of its own; every other entry point (building or mutating a handle, and the
 *     partial-state entries of the multi-GPU split, one thread per process by design) is exclusive:
 *     callable from any thread, serialised inside the library.
 *   - There is NO CPU fallback: without a HIP device every compute entry point fails with
 *     XR_ERR_NO_DEVICE.
 */
#ifndef XUGRID_AMD_H
#define XUGRID_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XR_OK 0
#define XR_ERR_INVALID (-1)   /* bad argument (maps to ValueError/TypeError on the Python side) */
#define XR_ERR_NO_DEVICE (-2) /* no HIP device / HIP runtime error at init */
#define XR_ERR_HIP (-3)       /* HIP runtime error during a call */
#define XR_ERR_LIMIT (-4)     /* size limit exceeded (int32 index range, max vertices per face) */

/* Reducer ids.  Names and semantics: xugrid/regrid/reduce.py:16-272. */
#define XR_MEAN 0
#define XR_HARMONIC_MEAN 1
#define XR_GEOMETRIC_MEAN 2
#define XR_SUM 3
#define XR_MINIMUM 4
#define XR_MAXIMUM 5
#define XR_MODE 6
#define XR_PERCENTILE 7 /* + percentile argument; median = 50 */
#define XR_FIRST_ORDER_CONSERVATIVE 8 /* = conductance */
#define XR_MAX_OVERLAP 9
/* Not a reduce.py reducer: the value of the row's LAST entry, NaN included, weights ignored -- the COO scatter
 * of CentroidLocatorRegridder._regrid (xugrid/regrid/regridder.py:400-409: out[k, row] = source[k, col], later
 * entries overwrite earlier ones) expressed on CSR rows, so that locator weights stay in HBM too. */
#define XR_SELECT 10

/* Source data dtypes accepted by the apply seam (output is always float64, regridder.py:44). */
#define XR_F64 0
#define XR_F32 1
#define XR_I32 2 /* int32 face data of xr_polygonize_dev only */

#define XR_MAX_FACE_NODES 32 /* numba_celltree MAX_N_VERTEX */

typedef struct xr_mesh xr_mesh; /* device-resident Ugrid2d face topology + spatial index */
typedef struct xr_csr xr_csr;   /* device-resident MatrixCSR weights */
typedef struct xr_outer xr_outer; /* separable (rectilinear) weights in factored form */

/* ---- engine ---------------------------------------------------------------------------- */
const char *xr_last_error(void);
/* Number of HIP devices (0 if none / no runtime). */
int xr_device_count(int *count);
/* Bind the engine (this process) to one device; creates the engine stream.  One process per
 * GPU is the multi-GPU model (torch.distributed ranks call this with LOCAL_RANK).  Calling any
 * compute entry point before xr_init implies xr_init(0). */
int xr_init(int device);
int xr_current_device(int *device);
/* Release cached HBM held by the engine's block pool. */
int xr_trim_pool(void);
int xr_version(void);
/* Share a HIP stream with the caller (e.g. PyTorch's current stream, `torch.cuda.current_stream().cuda_stream`;
 * the null stream is a valid handle): with external != 0 every kernel, copy and event of the engine goes to
 * `hip_stream`, so device work of caller and engine is ordered without host synchronisation, and with
 * async_dev != 0 the *_dev entry points return as soon as their kernels are enqueued.  external == 0 restores the
 * engine's own stream.  The multi-GPU layer uses this between its kernels and the RCCL collectives. */
int xr_set_stream(void *hip_stream, int external, int async_dev);
/* Asynchronous mode on the engine's OWN stream (on != 0): the *_dev entry points, xr_overlap_apply_dev and
 * xr_mesh_invalidate return with their kernels still in flight; results are complete after xr_dev_sync() or any call that
 * returns data to the host.  All work then stays on the one engine stream (no per-thread lanes): calls from several host
 * threads are safe but take turns -- each is enqueued whole before the next starts -- instead of running on streams of their
 * own (the same holds after xr_set_stream).  For pipelines that keep their data on the device and issue many calls back to
 * back (a time loop; bench.py's step). */
int xr_set_async(int on);
/* Run-time options of the library -- the switches tests and measurement scripts flip (no reference interface: xugrid has no
 * such knobs).  None changes a result, except "apply_contract" (documented there).  Names and meanings: DESIGN.md section 8 /
 * xugrid_amd/csrc/xr_internal.h (enum Option); the value an option starts with is read ONCE from the environment variable
 * XR_<NAME IN CAPITALS> when the library is first used.  Unknown names are an error (XR_ERR_INVALID).  The calls are
 * thread-safe; an option changed while another thread is inside a call takes effect for that call or the next. */
int xr_set_option(const char *name, int64_t value);
int xr_get_option(const char *name, int64_t *value);
/* Host-only helpers of the Python layer (no device, usable without one): the copies xugrid's constructors make
 * (Ugrid2d.__init__, xugrid/ugrid/ugrid2d.py:86-96: contiguous node_x / node_y, face_node_connectivity.copy()) done by the
 * library's host thread pool.  xr_host_interleave2: out_xy[i] = (x[i * x_stride], y[i * y_stride]), strides in elements. */
int xr_host_copy(void *dst, const void *src, int64_t bytes);
int xr_host_interleave2(const double *x, int64_t x_stride, const double *y, int64_t y_stride, int64_t n, double *out_xy);

/* ---- seam 1: mesh handle = CellTree2d(vertices, faces, fill_value) --------------------- */
/* ugrid2d.py:915-921.  node_xy: float64[n_node,2] (node_coordinates, ugridbase.py:576-579);
 * faces: int32 or int64 [n_face, n_max_node] dense face_node_connectivity with `fill_value`
 * in unused slots (faces_itemsize = 4 or 8).  Uploads the raw arrays only; the derived state
 * (CCW-normalised connectivity, per-face length/bbox/area, spatial index) is built on the
 * device lazily by the first call that needs it, or explicitly by xr_mesh_prepare /
 * xr_mesh_build_index. */
int xr_mesh_create(const double *node_xy, int64_t n_node, const void *faces, int faces_itemsize,
                   int64_t n_face, int64_t n_max_node, int64_t fill_value, xr_mesh **out);
/* The same from arrays that are ALREADY in HBM of the engine's device (a multi-GPU rank that cut its shard out of the
 * replicated mesh on the device, xugrid_amd/distributed.py; any pipeline that produced the mesh there).  node_xy_dev:
 * float64[n_node,2]; faces_dev: int32 or int64 [n_face, n_max_node].  Both are COPIED (the handle owns its arrays; the
 * copy of the connectivity is the same fill -> -1 / narrowing / validation pass xr_mesh_create runs).  The caller's arrays
 * must be complete in the engine's stream order (xr_set_stream: the caller's own stream) or on the host's view
 * (after a device synchronisation). */
int xr_mesh_create_dev(const double *node_xy_dev, int64_t n_node, const void *faces_dev, int faces_itemsize,
                       int64_t n_face, int64_t n_max_node, int64_t fill_value, xr_mesh **out);
/* The quad mesh of a rectilinear grid, generated on the device: Ugrid2d.from_structured_bounds ->
 * _from_intervals_helper (xugrid/ugrid/ugrid2d.py:1973-2034, :1894-1912), which is how a raster enters the polygon
 * path when the other grid is unstructured (StructuredGrid2d.convert_to, regrid/structured.py:489-501).
 * x_vertices float64[nx + 1], y_vertices float64[ny + 1]: the cell edges in the raster's own order (ascending or
 * descending).  Nodes in meshgrid order (node id = j * (nx + 1) + i), face id = j * nx + i, corners
 * counter-clockwise for ascending axes.  Only the two 1-D arrays cross PCIe. */
int xr_mesh_create_rectilinear(const double *x_vertices, int64_t nx, const double *y_vertices, int64_t ny,
                               xr_mesh **out);
int xr_mesh_destroy(xr_mesh *mesh);
int xr_mesh_info(const xr_mesh *mesh, int64_t *n_node, int64_t *n_face, int64_t *n_max_node);
/* HBM currently held by the handle (raw arrays, prepared arrays, query order, tree index).  Vertex blocks of meshes with
 * more than 4 nodes per face are stored flat with offsets (sum of the real polygon lengths, not n_face * n_max_node). */
int xr_mesh_device_bytes(const xr_mesh *mesh, int64_t *bytes);
/* Per-face preparation on the device: fill->-1, polygon length, CCW normalisation, bbox, area. */
int xr_mesh_prepare(xr_mesh *mesh);
/* Spatial index over the faces of this mesh (the "tree" side): hierarchical uniform grid. */
int xr_mesh_build_index(xr_mesh *mesh);
/* Drop all derived state (prepare + index + the face centroids a locate / barycentric call left on the mesh -- the
 * reference caches Ugrid2d.centroids on the grid the same way); used by benchmarks to time the whole path. */
int xr_mesh_invalidate(xr_mesh *mesh);
/* Face areas, connectivity.area (xugrid/ugrid/connectivity.py:615-633) -> float64[n_face]. */
int xr_mesh_area(xr_mesh *mesh, double *area_out);
/* Face centroids, connectivity.centroids (connectivity.py:636-664) -> float64[n_face,2]. */
int xr_mesh_centroids(xr_mesh *mesh, double *centroids_out);
/* ... the same values into device memory float64[n_face,2] (a copy of the array the mesh keeps). */
int xr_mesh_centroids_dev(xr_mesh *mesh, double *out_dev);
/* CCW-normalised connectivity as held on the device -> int64[n_face, n_max_node]. */
int xr_mesh_faces(xr_mesh *mesh, int64_t *faces_out);
/* The arrays the handle was created from: node_xy float64[n_node, 2] and the connectivity int64[n_face, m] in
 * the caller's vertex order, fill -1 (either pointer may be NULL).  Mainly for meshes that were built on the
 * device (xr_voronoi_mesh). */
int xr_mesh_download(xr_mesh *mesh, double *node_xy_out, int64_t *faces_out);
/* ---- meshes and per-face quantities derived from a mesh, all in the caller's vertex order -----------------------------
 * Fan triangulation (connectivity.triangulate, connectivity.py:704-788; Ugrid2d.triangulate, ugrid2d.py:1650-1662): a new
 * device-resident mesh with the same node coordinates (copied device to device: the handle owns its arrays) whose faces are
 * the triangles (n0, n[t + 1], n[t + 2]), t = 0 .. k - 3, of every face of k nodes, in face order.  A mesh of
 * n_max_node == 3 gives a copy.  XR_ERR_LIMIT when 3 * n_triangle leaves the int32 range.
 * xr_mesh_triangle_face_dev: the source face of every triangle, repeat(arange(n_face), k - 2) -> int64[n_triangle] in device
 * memory; only for a mesh made by xr_mesh_triangulate. */
int xr_mesh_triangulate(xr_mesh *mesh, xr_mesh **out);
int xr_mesh_triangle_face_dev(const xr_mesh *triangles, int64_t *index_dev);
/* Circumcenters of a triangle mesh, connectivity.circumcenters (connectivity.py:667-701), evaluated operation for operation
 * -> float64[n_face, 2] in device memory.  XR_ERR_INVALID unless n_max_node == 3. */
int xr_mesh_circumcenters_dev(xr_mesh *mesh, double *out_dev);
/* connectivity.perimeter (connectivity.py:600-612), the edge lengths summed in slot order -> float64[n_face] in device memory. */
int xr_mesh_perimeter_dev(xr_mesh *mesh, double *out_dev);
/* Ugrid2d.face_bounds (ugrid2d.py:597-619): (min x, min y, max x, max y) over the real nodes -> float64[n_face, 4] in device memory. */
int xr_mesh_face_bounds_dev(xr_mesh *mesh, double *out_dev);

/* CellTree2d.intersect_faces (unstructured.py:124-132) + relative normalisation (:133-134)
 * + MatrixCSR.from_triplet (regridder.py:433-435): all (query face, tree face) pairs with
 * intersection area > 0, as a CSR matrix with one row per QUERY (= regridding target) face,
 * columns = TREE (= source) faces sorted ascending within a row, data = overlap area, or
 * area / tree-face area if relative != 0.  The result stays in HBM.
 * As in numba_celltree a pair only counts if the two faces' exact bounding boxes overlap strictly and the separating-axis
 * test does not separate them: faces that merely touch (a mesh against itself, meshes sharing nodes) give no entry even
 * where the clip's floating-point result is a sliver of rounding dust. */
int xr_overlap(xr_mesh *tree, xr_mesh *query, int relative, xr_csr **out);
/* Statistics of the last xr_overlap on this tree: bbox candidate pairs tested by the clipper. */
int xr_overlap_stats(const xr_mesh *tree, int64_t *n_candidates);
/* Weights AND their first use in one call: OverlapRegridder(source, target, method).regrid(data) -- constructor
 * (regridder.py:505-512 -> _compute_weights :428-436) followed by regrid (:212-262 -> _regrid :41-67).  Same results as
 * xr_overlap + xr_apply_csr_dev; the matrix is returned for further applies.  For one variable and a streaming reducer the
 * apply is enqueued before the host has read the sizes of the matrix back, so the build's one host round trip hides behind
 * the apply kernel instead of separating the two.  source_dev (K, S) / out_dev (K, T) are device pointers. */
int xr_overlap_apply_dev(xr_mesh *tree, xr_mesh *query, int relative, int method, double percentile,
                         const void *source_dev, int source_dtype, int64_t K, double *out_dev, xr_csr **out);

/* CellTree2d.locate_points(points, tolerance) (unstructured.py:139,189; ugridbase.py:1323).
 * points float64[n,2] -> face index int64[n], -1 = not found.  tolerance < 0 selects the
 * default 1e-12 x max bbox diagonal (ugridbase.py:1165-1170).  A point within tolerance of an
 * edge shared by several faces is assigned to the LOWEST face index. */
int xr_locate_points(xr_mesh *mesh, const double *points, int64_t n, double tolerance,
                     int64_t *face_index_out);
/* Ugrid2d.rasterize_like (xugrid/ugrid/ugrid2d.py:1080-1100): locate_points on the nodes of a raster given by its
 * two 1-D coordinate arrays; the ny * nx points are generated on the device (point j * nx + i = (x[i], y[j])),
 * face_index_out int64[ny * nx]. */
int xr_locate_raster(xr_mesh *mesh, const double *x, int64_t nx, const double *y, int64_t ny,
                     double tolerance, int64_t *face_index_out);
/* CellTree2d.compute_barycentric_weights(points, tolerance) (ugrid2d.py:1054-1078).
 * -> face index int64[n] and float64[n, n_max_node] generalized barycentric weights
 * (all zero, face -1 when outside). */
int xr_barycentric(xr_mesh *mesh, const double *points, int64_t n, double tolerance,
                   int64_t *face_index_out, double *weights_out);

/* replace_interpolated_weights(vertices, faces, face_index, weights, node_to_node_map, node_index_threshold)
 * (xugrid/regrid/unstructured.py:17-57) as a stand-alone call: the device kernel xr_barycentric_csr runs inside its
 * pipeline, on caller-owned arrays.  vertices float64[n_vertex, 2]; faces int64[n_face, m] (-1 fill behind the
 * corners); face_index int64[n] (-1 = point in no cell: row untouched); weights float64[n, m] row-major, updated
 * IN PLACE as the reference does; node_to_node_map int64[n_map, 2]; node_index_threshold = n_vertex - n_map. */
int xr_replace_interpolated_weights(const double *vertices, int64_t n_vertex, const int64_t *faces, int64_t n_face,
                                    int64_t m, const int64_t *face_index, double *weights, int64_t n,
                                    const int64_t *node_to_node_map, int64_t n_map);

/* UnstructuredGrid2d.locate_centroids (xugrid/regrid/unstructured.py:137-144) + MatrixCOO.from_triplet
 * (regridder.py:386-398) without leaving the device: one row per query point holding (face containing it, 1.0),
 * no entry when the point is in no face.  Query points: `points` float64[n, 2] (query == NULL) or the face
 * centroids of the mesh `query` (points == NULL).  Apply with XR_SELECT. */
int xr_locate_csr(xr_mesh *tree, xr_mesh *query, const double *points, int64_t n, double tolerance,
                  xr_csr **out);

/* The whole of UnstructuredGrid2d.barycentric after the Voronoi pre-step (xugrid/regrid/unstructured.py:166-201),
 * assembled on the device: compute_barycentric_weights of the query points in the centroidal Voronoi mesh
 * `voronoi` (ugrid2d.py:1054-1078), replace_interpolated_weights (unstructured.py:17-57) for the synthetic exterior
 * vertices (the last n_extra Voronoi vertices; node_to_node_map int64[n_extra, 2]), zero rows for points outside
 * `source` (locate_points == -1 with the default tolerance, :188-190), weights > 0 only (:191-198), Voronoi
 * vertices mapped to source faces through vertex_face int64[n_vertex] (node_to_face_index).  The query points are
 * either `points` float64[n, 2] (query == NULL) or the face centroids of the mesh `query` (points == NULL; computed
 * on the device, nothing crosses PCIe).  Result: MatrixCSR.from_triplet(target, source, weights) (regridder.py:634-636)
 * with n rows (points) and source->n_face columns, entries of a row in Voronoi-vertex slot order. */
int xr_barycentric_csr(xr_mesh *voronoi, xr_mesh *source, xr_mesh *query, const double *points,
                       int64_t n, double tolerance, const int64_t *vertex_face,
                       const int64_t *node_to_node_map, int64_t n_extra, xr_csr **out);
/* the same with vertex_face given only for the vertices >= n_identity (vertex v < n_identity, a face centroid,
 * belongs to source face v): spares the host an O(n) array and its upload.
 * The weight of slot j of a cell is paired with vertex j of the cell in the CALLER's vertex order, exactly as the
 * reference does (unstructured.py:175,193) -- also in xr_barycentric_csr above.  tree_order = 1 (opt-in, NOT the
 * reference's result): paired with vertex j in the TREE's own counter-clockwise-normalised order, the order the
 * weights were computed in.  The two differ only for cells the tree stores reversed (clockwise cells, or concave
 * exterior cells that start at a reflex corner). */
int xr_barycentric_csr_tail(xr_mesh *voronoi, xr_mesh *source, xr_mesh *query, const double *points, int64_t n,
                            double tolerance, int64_t n_identity, const int64_t *vertex_face_tail,
                            const int64_t *node_to_node_map, int64_t n_extra, int tree_order, xr_csr **out);

/* The source-side half of UnstructuredGrid2d.barycentric -- the query points (points, or the face centroids of `query`,
 * unstructured.py:147) and `grid.locate_points(points) == -1` with the default tolerance (:188-190) -- as a device-resident
 * handle whose kernels run on the engine's side stream: they need nothing of the Voronoi tessellation, so they run beside
 * the (latency-bound) kernels of the Voronoi pre-step instead of behind them (1M faces / 4M points: construction 3.3 -> 2.96
 * ms).  Since round 5 they are DEFERRED: enqueued not by this call but by whichever call needs them or has the device idle
 * next -- xr_voronoi_create / xr_voronoi_mesh_auto where their host round trips begin, xr_barycentric_csr_points at the
 * latest.  LIFETIME: the handle keeps raw pointers to `source` and `query`; both meshes must stay alive until
 * xr_barycentric_csr_points has consumed the handle or xr_points_destroy has released it.  xr_mesh_invalidate and
 * xr_mesh_destroy of either mesh launch the deferred kernels first (they read the arrays as they are at that moment), so a
 * mesh that is invalidated or destroyed in between is safe, a handle used AFTER its source was destroyed is not.
 * xr_barycentric_csr_points is xr_barycentric_csr_tail on such a handle; it joins the side stream before it reads the flags. */
typedef struct xr_points xr_points;
int xr_locate_flags_begin(xr_mesh *source, xr_mesh *query, const double *points, int64_t n, xr_points **out);
int xr_points_destroy(xr_points *points);
int xr_barycentric_csr_points(xr_mesh *voronoi, xr_mesh *source, xr_points *points, double tolerance, int64_t n_identity,
                              const int64_t *vertex_face_tail, const int64_t *node_to_node_map, int64_t n_extra,
                              int tree_order, xr_csr **out);

/* ---- Voronoi pre-step of BarycentricInterpolator (xugrid/ugrid/voronoi.py:330-458 as called from
 * xugrid/regrid/unstructured.py:151-165: add_exterior, add_vertices, skip_concave) ---------------------
 * xr_voronoi_create does the O(n) part on the device: the node -> face inversion
 * (ugrid2d.py:700-713, connectivity.py:247-259), the exterior edges (the only part of edge_node_connectivity /
 * edge_face_connectivity the Voronoi step reads, voronoi.py:77-97; ugrid2d.py:497-509, :661-677) and the cells
 * of all nodes that touch no exterior edge: the centroids of the surrounding faces ordered counter-clockwise
 * about the node (voronoi.py:355-372).  The cells of the boundary nodes (projections on the exterior edges, one extra
 * corner per boundary node, the convexity choice: voronoi.py:59-327) are O(boundary) work on a few KB the device gathers:
 * done by the library itself in native host code (xr_voronoi_mesh_auto; a dozen dependent sorts / scans over a few thousand
 * items take tens of microseconds there, as device kernels each would be a launch and a round trip) or by the caller
 * (xr_voronoi_boundary -> xr_voronoi_mesh).  The Voronoi tessellation is assembled as a device-resident mesh:
 *   vertices = [face centroids ; extra_xy]      cells = [interior nodes ascending ; boundary_cells]. */
typedef struct xr_voronoi xr_voronoi;
int xr_voronoi_create(xr_mesh *mesh, xr_voronoi **out); /* `mesh` must outlive the handle */
/* The same builder for every flag set of voronoi_topology (voronoi.py:330-458) and any generator points: generators_dev
 * float64[n_face, 2] in device memory (copied), NULL = the face centroids.  xr_voronoi_create = (1, 1, 1, NULL).
 *   skip_concave = 0   the true boundary node always replaces the substitute corner (no area comparison)
 *   add_vertices = 0   no extra corner per boundary node: the tail holds projections only, the interpolation map is empty
 *   add_exterior = 0   cells for every node with at least three faces, boundary nodes included, and no boundary part; the
 *                      vertices are the generator points some cell uses, ascending by face (xr_voronoi_vertex_info: their
 *                      number and the largest used face id); XR_ERR_INVALID when no node has three faces
 * xr_voronoi_vertex_info: generator points at the head of the vertex array (n_face with the exterior) and the largest face
 * id among them. */
int xr_voronoi_create_flags(xr_mesh *mesh, int add_exterior, int add_vertices, int skip_concave, const double *generators_dev,
                            xr_voronoi **out);
int xr_voronoi_vertex_info(const xr_voronoi *v, int64_t *n_generator_vertex, int64_t *max_used_face);
int xr_voronoi_info(const xr_voronoi *v, int64_t *n_node, int64_t *nnz, int64_t *n_exterior_edge,
                    int64_t *n_interior_cell, int64_t *max_interior_degree);
/* node_face_connectivity as CSR (indptr int64[n_node+1], indices int64[nnz], faces ascending per node), the
 * exterior edges in lexicographic order (edge_nodes int64[n_edge, 2] = (lower, higher node id), edge_face
 * int64[n_edge]) and, optionally, the face centroids float64[n_face, 2]. */
/* (A handle built with add_exterior = 0 keeps only the generator points its cells use: `centroids` must be NULL there.) */
int xr_voronoi_download(const xr_voronoi *v, int64_t *indptr, int64_t *indices, int64_t *edge_nodes,
                        int64_t *edge_face, double *centroids);
/* The same information restricted to what the O(boundary) host part reads -- nothing of size O(n) crosses PCIe:
 * the boundary nodes (end points of exterior edges, ascending), their rows of node_face_connectivity as a small
 * CSR (row_ptr int64[n_boundary_node + 1], faces int64[n_boundary_entry]) with the centroid of every listed face
 * (face_xy float64[n_boundary_entry, 2]), the exterior edges as above and the centroid of each edge's face. */
int xr_voronoi_boundary_info(xr_voronoi *v, int64_t *n_boundary_node, int64_t *n_boundary_entry);
int xr_voronoi_boundary(xr_voronoi *v, int64_t *nodes, int64_t *row_ptr, int64_t *faces, double *face_xy,
                        int64_t *edge_nodes, int64_t *edge_face, double *edge_face_xy);
/* extra_xy float64[n_extra_vertex, 2]: projections and substitute vertices (ids n_face ...);
 * boundary_cells int64[n_boundary_cell, n_max_boundary], -1 padded, counter-clockwise. */
int xr_voronoi_mesh(const xr_voronoi *v, const double *extra_xy, int64_t n_extra_vertex,
                    const int64_t *boundary_cells, int64_t n_boundary_cell, int64_t n_max_boundary,
                    xr_mesh **out);
/* The whole pre-step in one call: boundary cells by the library, assembly on the device.  n_tail = vertices added behind
 * the n_face centroids, n_map = rows of the interpolation map (voronoi.py:interpolation_map); xr_voronoi_tail copies
 * tail_face_index int64[n_tail] (source face of every added vertex, -1 for the per-node extra corners) and
 * interpolation_map int64[n_map, 2] (global vertex ids).  xr_voronoi_boundary_cells[_info]: the boundary cells themselves
 * (extra_xy float64[n_extra_vertex, 2], cells int64[n_cell, n_max], -1 padded) as xr_voronoi_mesh expects them. */
int xr_voronoi_mesh_auto(xr_voronoi *v, xr_mesh **out, int64_t *n_tail, int64_t *n_map);
int xr_voronoi_tail(xr_voronoi *v, int64_t *tail_face_index, int64_t *interpolation_map);
int xr_voronoi_boundary_cells_info(xr_voronoi *v, int64_t *n_extra_vertex, int64_t *n_cell, int64_t *n_max);
int xr_voronoi_boundary_cells(xr_voronoi *v, double *extra_xy, int64_t *cells);
int xr_voronoi_destroy(xr_voronoi *v);

/* ---- seam 3: MatrixCSR handle ----------------------------------------------------------- */
int xr_csr_info(const xr_csr *csr, int64_t *n, int64_t *m, int64_t *nnz);
/* Copy out as the reference's MatrixCSR fields (core/sparse.py:81-137): data float64[nnz],
 * indices int64[nnz], indptr int64[n+1]. */
int xr_csr_download(const xr_csr *csr, double *data, int64_t *indices, int64_t *indptr);
/* Build a device CSR from host MatrixCSR fields (from_weights / from_dataset path,
 * regridder.py:299-312,334-348). */
int xr_csr_upload(const double *data, const int64_t *indices, const int64_t *indptr, int64_t n,
                  int64_t m, int64_t nnz, xr_csr **out);
/* MatrixCSR.from_triplet(row, col, data, n, m): rows must be non-decreasing
 * (core/sparse.py:65); indptr = [0, cumsum(bincount(row, minlength=n))] computed on device. */
int xr_csr_from_triplet(const int64_t *row, const int64_t *col, const double *data, int64_t nnz,
                        int64_t n, int64_t m, xr_csr **out);
/* Separable (rectilinear) weights: StructuredGrid2d.broadcast_sorted (xugrid/regrid/structured.py:503-531 =
 * utils.broadcast, regrid/utils.py:17-36, followed by an argsort on the target index) for the per-axis
 * triplets of StructuredGrid1d.overlap / linear_weights (structured.py:335-356, :379-403).  Each axis is a
 * small sparse matrix in CSR form: indptr int64[n_target+1], source index int64[nnz] (ascending within a
 * row) and weight float64[nnz].  The result is the CSR of their outer product: row jt * n_target_x + it holds
 * the entries (source_y * n_source_x + source_x, weight_y * weight_x), ordered by column id, assembled on the
 * device without a sort. */
int xr_csr_from_outer(const int64_t *indptr_y, const int64_t *source_y, const double *weight_y,
                      int64_t n_target_y, int64_t n_source_y, const int64_t *indptr_x,
                      const int64_t *source_x, const double *weight_x, int64_t n_target_x,
                      int64_t n_source_x, xr_csr **out);
/* The same separable weights kept in FACTORED form (the two per-axis sparse matrices, a few hundred KB for
 * 4000 x 4000 grids) instead of their P_y * P_x product: xr_apply_outer reduces each target cell by walking its
 * c_y x c_x entries in the order of the product's CSR row (= the order of the reference's loop,
 * xugrid/regrid/structured.py:503-601 -> regrid/reduce.py), forming every weight w_y * w_x on the fly, so rows of
 * ANY length are reduced sequentially and bit-identically to the reference, and the apply reads the source data
 * once instead of the 12 bytes per entry of a stored matrix.  mode / percentiles (which need a row's values side by
 * side) and xr_outer_csr materialise the product once and keep it inside the handle. */
int xr_outer_create(const int64_t *indptr_y, const int64_t *source_y, const double *weight_y,
                    int64_t n_target_y, int64_t n_source_y, const int64_t *indptr_x,
                    const int64_t *source_x, const double *weight_x, int64_t n_target_x,
                    int64_t n_source_x, xr_outer **out);
int xr_outer_info(const xr_outer *outer, int64_t *n, int64_t *m, int64_t *nnz);
/* borrowed handle of the materialised product (owned by `outer`; do not destroy) */
int xr_outer_csr(xr_outer *outer, const xr_csr **out);
int xr_outer_destroy(xr_outer *outer);
/* Layered grids: a 2-D grid plus top / bottom of every layer in every cell (float64, layer-major: value of layer l in cell
 * c at [l * n_cell + c] with column stride 1; column stride 0: arrays of n_layer values, the same layering in every cell,
 * not expanded).  From the 2-D weights `w2d` (rows = target cells j, entries (i, w) in the caller's ids and in the order
 * xr_csr_download returns them, whatever order the handle stores) the 3-D matrix: one entry for every entry of w2d and
 * every layer pair (lt, ls) with
 *     dz = min(top_s[ls, i], top_t[lt, j]) - max(bottom_s[ls, i], bottom_t[lt, j]) > 0
 * -- a NaN bound or top <= bottom: no such layer in that cell; layers that only touch: nothing; any layer order.  Row
 * lt * n_target + j, column ls * n_source + i, so data is (..., n_layer, n_cell) on both sides.  A row keeps w2d's order of
 * i, ls ascending within one i.  Weight w * dz; relative != 0: w * (dz / (top_s[ls, i] - bottom_s[ls, i])), the share of the
 * source voxel's height -- single IEEE operations in that order.  The result is an independent matrix like any other
 * (applies, adjoint, download); rows of more than 32 entries are listed for the cooperative reducers.  XR_ERR_LIMIT,
 * before anything is launched, where n_layer_t * nnz(w2d), n_layer_t * n_target or n_layer_s * n_source leave the int32
 * range; the number of entries is known behind the count pass and checked there.
 * xr_csr_layered takes host arrays and uploads them; xr_csr_layered_dev takes device pointers. */
int xr_csr_layered(const xr_csr *w2d, const double *top_s, const double *bottom_s, int64_t n_layer_s, int64_t col_stride_s,
                   const double *top_t, const double *bottom_t, int64_t n_layer_t, int64_t col_stride_t, int relative,
                   xr_csr **out);
int xr_csr_layered_dev(const xr_csr *w2d, const double *top_s_dev, const double *bottom_s_dev, int64_t n_layer_s,
                       int64_t col_stride_s, const double *top_t_dev, const double *bottom_t_dev, int64_t n_layer_t,
                       int64_t col_stride_t, int relative, xr_csr **out);
/* The vertical building block on its own, with the signature and the ids of the reference's overlap_1d_nd
 * (xugrid/regrid/overlap_1d.py:162-245): source_bounds float64 (n, n_layer_s, 2) and target_bounds (m, n_layer_t, 2) hold
 * (lower, upper) per column and layer, source_index / target_index int64 (o,) name the column pairs -- any o, every id
 * checked (XR_ERR_INVALID).  Result: the triplets (source column * n_layer_s + ls, target column * n_layer_t + lt, dz) of
 * the rule above in the order pair k, then lt, then ls.  *n_out = their number p; they are written (int64, int64,
 * float64, device pointers) only when capacity >= p: call with capacity 0 for the size, then again. */
int xr_overlap_1d_nd_dev(const double *source_bounds_dev, int64_t n, int64_t n_layer_s, const double *target_bounds_dev,
                         int64_t m, int64_t n_layer_t, const int64_t *source_index_dev, const int64_t *target_index_dev,
                         int64_t o, int64_t capacity, int64_t *source_out_dev, int64_t *target_out_dev,
                         double *overlap_out_dev, int64_t *n_out);
/* NetworkGridder weights (xugrid/regrid/gridder.py:66-73 through UnstructuredGrid2d.intersection_length,
 * xugrid/regrid/unstructured.py:203-215): replaces numba_celltree's
 *     celltree.intersect_edges(edge_coords) -> (edge_index, face_index, intersections[n, 2, 2]),
 * the length = norm(diff(intersections)) that follows, the argsort by face and MatrixCSR.from_triplet.
 * edge_xy: (n_edge, 2, 2) float64 end-point coordinates (Ugrid1d.edge_node_coordinates).  Result: rows = faces of
 * `tree`, columns = edge ids (ascending within a row), data = length of the piece of the edge inside the face
 * (Cyrus-Beck clip against the convex, CCW-normalised face); only pieces of positive length are entries, so an
 * edge that merely touches a face corner or runs outside along its boundary adds nothing.  Applied with
 * xr_apply_csr like any other weights (source variables live on the EDGES).  `relative` lengths are not offered:
 * the reference never requests them (gridder.py:49) and its formula indexes the edge lengths by face id (:213-214). */
int xr_edge_length_csr(xr_mesh *tree, const double *edge_xy, int64_t n_edge, xr_csr **out);
/* ... with the end points already in HBM (edge_xy_dev: float64 [n_edge][2][2], a device pointer): no upload -- the device part
 * of the call above on its own (a third of which is the PCIe transfer of 32 bytes per edge). */
int xr_edge_length_csr_dev(xr_mesh *tree, const double *edge_xy_dev, int64_t n_edge, xr_csr **out);
/* The third return value of intersect_edges for the entries of such a matrix: intersections float64[nnz, 2, 2]
 * (begin and end point of every piece, along the direction of its edge), in the entry order of the CSR. */
int xr_edge_pieces(xr_mesh *tree, const xr_csr *csr, const double *edge_xy, int64_t n_edge,
                   double *intersections);
/* Optional locality hint for matrices that were uploaded (xr_csr_upload / xr_csr_from_triplet, i.e. the
 * from_weights path): one small integer per row such that rows with equal keys are spatial neighbours (e.g. the
 * Morton code of a coarse cell holding the target face's centroid).  With many source variables (K >= 8) the apply
 * regroups the STORED rows by key once -- results and xr_csr_download are unaffected.  xr_overlap attaches such
 * keys itself (runs of 16 consecutive target ids share a key, so that a variable's outputs leave in 128-byte pieces);
 * keys given for such a matrix are per CALLER row and replace that grouping -- worth it with xr_csr_output_stored_order,
 * where the output no longer cares about the caller's numbering and every row can go to its own tile. */
int xr_csr_set_row_keys(xr_csr *csr, const int64_t *keys, int64_t key_range);
/* The same for the COLUMNS (source cells): one small integer per column such that columns with equal keys are spatial
 * neighbours.  The columns are renumbered once by key (stable), so that the source values a block of target rows
 * gathers are neighbours in memory whatever the caller's cell numbering (a qhull-numbered mesh: half the fetched bytes
 * were unused).  Entry order inside the rows is untouched -- reducers add in the same order, results are bit-identical
 * -- and xr_csr_download returns the caller's column ids.  The source block handed to the apply entry points is either
 * in the caller's cell order (default: one gather pass per call puts it in the stored order) or, after
 * xr_csr_expect_permuted(csr, 1), already in the stored order: source_permuted[k][j] = source[k][order[j]] with
 * order = xr_csr_col_order (int64[m]) -- for data that stays on the device across many applies, or producers that can
 * write in that order. */
int xr_csr_set_col_keys(xr_csr *csr, const int64_t *keys, int64_t key_range);
int xr_csr_col_order(const xr_csr *csr, int64_t *order_out);
int xr_csr_expect_permuted(xr_csr *csr, int permuted);
/* The mirror image for the OUTPUT: after xr_csr_output_stored_order(csr, 1) the applies write stored row r to out[k, r]
 * (fully coalesced whatever the caller's numbering) instead of out[k, row_order[r]]; xr_csr_row_order returns the permutation
 * (stored row r = caller's row order[r]; K_hint is ignored and kept for binary compatibility).  The regrouping of the rows
 * into 2-D tiles -- otherwise deferred to the first apply with 8 or more variables -- is part of the stored order: both calls
 * settle it at once, and from xr_csr_output_stored_order(csr, 1) on the order is FROZEN: xr_csr_set_row_keys refuses
 * (XR_ERR_INVALID) until the stored-order output is switched off again, so no apply can ever write rows in a permutation
 * the caller has not read.  With columns AND rows in the engine's order a pipeline that keeps its blocks on the device pays
 * the caller's numbering once, not per apply. */
int xr_csr_output_stored_order(xr_csr *csr, int stored);
int xr_csr_row_order(const xr_csr *csr, int64_t K_hint, int64_t *order_out);
/* The STORED rows of more than 32 entries, which the applies reduce cooperatively, as the matrix' builder listed them (in no
 * particular order): *n_out = their number, the first min(*n_out, capacity) of them -> rows_out.  For inspection and tests. */
int xr_csr_long_rows(const xr_csr *csr, int64_t capacity, int64_t *rows_out, int64_t *n_out);
int xr_csr_destroy(xr_csr *csr);

/* ---- seam 2: apply ---------------------------------------------------------------------- */
/* make_regrid(func)._regrid(source, A, size), regridder.py:41-67.
 * source: (K, S) row-major, S = csr.m, dtype XR_F64 / XR_F32; out: float64 (K, T), T = csr.n,
 * NaN for empty rows.  `percentile` is used by XR_PERCENTILE only (0..100, reduce.py:241-243). */
int xr_apply_csr(const xr_csr *csr, int method, double percentile, const void *source,
                 int source_dtype, int64_t K, double *out);
int xr_apply_csr_dev(const xr_csr *csr, int method, double percentile, const void *source_dev,
                     int source_dtype, int64_t K, double *out_dev);
/* the same two calls on factored separable weights (xr_outer_create) */
int xr_apply_outer(xr_outer *outer, int method, double percentile, const void *source,
                   int source_dtype, int64_t K, double *out);
int xr_apply_outer_dev(xr_outer *outer, int method, double percentile, const void *source_dev,
                       int source_dtype, int64_t K, double *out_dev);
/* ---- the adjoint of the apply: target-side quantities (gradients, residuals, sensitivities) back onto the source ------
 * For the reducers that are linear in the source values for a fixed NaN pattern -- XR_MEAN, XR_SUM,
 * XR_FIRST_ORDER_CONSERVATIVE, XR_SELECT; every other id is XR_ERR_INVALID -- with W the T x S matrix in the ids the applies
 * use (entries e = (i, j, w) at storage position p), v the forward input (K, S), g (K, T) float64:
 *     valid(k, e) = !isnan(v[k, j]);   Wsum[k, i] = sum of w over the valid entries of row i, by the forward's own row walk
 *     row i is live for k when Wsum[k, i] != 0 (XR_SELECT: when it is not empty)
 *     r[k, i] = g[k, i] / Wsum[k, i] (XR_MEAN), g[k, i] (the others)
 *     coefficient of e: w (XR_MEAN, XR_FIRST_ORDER_CONSERVATIVE), 1 (XR_SUM), 1 on the row's last entry else 0 (XR_SELECT)
 *     out[k, j] = sum of r[k, i] * coefficient(e) over the entries of column j whose row is live, in ascending (i, p) order;
 *                 +0.0 for an empty sum and wherever v[k, j] is NaN (XR_SELECT ignores NaN: its forward copies them)
 * A row that is not live contributes nothing whatever g holds there; on live rows plain IEEE arithmetic applies.  Columns of
 * more than 32 entries are summed by a wave, of more than 2048 by a block, in a fixed order: no floating-point atomics, the
 * same bits on every call.  source == NULL: no NaN in the source.  out: float64 (K, S).
 * The first call transposes the weights on the device and keeps the result inside the handle (12 bytes per entry + 4 per
 * column and listed long column; xr_csr_drop_transpose releases it, the next call rebuilds it).  xr_csr_transpose returns that
 * structure as an independent S x T matrix: rows = the columns of `csr` in the caller's ids, entries in ascending (i, p).
 * A matrix whose source blocks arrive pre-permuted (xr_csr_expect_permuted) is XR_ERR_INVALID. */
int xr_csr_transpose(const xr_csr *csr, xr_csr **out);
int xr_csr_drop_transpose(xr_csr *csr);
int xr_apply_csr_adjoint(const xr_csr *csr, int method, const void *source, int source_dtype, const double *grad,
                         int64_t K, double *out);
int xr_apply_csr_adjoint_dev(const xr_csr *csr, int method, const void *source_dev, int source_dtype,
                             const double *grad_dev, int64_t K, double *out_dev);
/* ... on factored separable weights: through the materialised CSR the handle keeps (xr_outer_csr) */
int xr_apply_outer_adjoint_dev(xr_outer *outer, int method, const void *source_dev, int source_dtype,
                               const double *grad_dev, int64_t K, double *out_dev);
/* CentroidLocatorRegridder._regrid, regridder.py:400-409: out[k,row[i]] = source[k,col[i]],
 * NaN elsewhere.  rows must be unique (they are target indices of located centroids). */
int xr_apply_coo(const int64_t *row, const int64_t *col, int64_t nnz, int64_t T,
                 const void *source, int source_dtype, int64_t K, int64_t S, double *out);

/* ---- multi-GPU set-up: which source faces are mine, which targets can they reach ------------------
 * The reference has no multi-device path (its only parallel loop is the dask map of regridder.py:167-185); SURVEY 8(e) shards
 * the SOURCE faces over the ranks and replicates the target.  xr_shard_plan_dev evaluates the partition rule on the rank's
 * device from the replicated raw meshes (float64 [N, 2] coordinates, int64 [F, m] connectivity with -1 fill, device pointers):
 *   mode 0 "hash"      owner = face id mod world (the north star's wording)
 *   mode 1 "morton"    cells of a 1024 x 1024 raster over the source centroids, ordered along the Morton curve, cut into
 *                      `world` stretches of equal face COUNT (owner per cell: floor(faces in front of the cell * world / S))
 *   mode 2 "balanced"  the same cut by estimated WORK, round(4096 (1 + 4 n_tgt / n_src)) per source face from a coarse raster
 *                      both meshes are counted into
 * and keeps the target faces whose box touches the 128 x 128 occupancy raster of the rank's own source faces.  A face without
 * a valid node (all -1) has the centroid (0, 0) and no box: it enters no bounds and the occupancy raster on neither side, but as
 * a source face it still has a cell (its (0, 0) clamped into the other faces' bounds), work and an owner.  Integer
 * arithmetic decides every owner, so all ranks agree without communication.  Outputs: ascending global ids (device arrays of
 * capacity n_src_face / n_tgt_face), their counts, optionally the owner of every source face (int32 [n_src_face]). */
int xr_shard_plan_dev(const double *src_xy_dev, const int64_t *src_faces_dev, int64_t n_src_face, int src_m,
                      const double *tgt_xy_dev, const int64_t *tgt_faces_dev, int64_t n_tgt_face, int tgt_m, int world, int rank,
                      int mode, int64_t *local_faces_dev, int64_t *n_local_faces, int64_t *local_targets_dev,
                      int64_t *n_local_targets, int32_t *owner_dev);

/* Multi-GPU (source faces sharded over ranks).  For EVERY reducer that decomposes over source shards
 * (xugrid/regrid/reduce.py:16-123, 206-222) each rank reduces the entries of its own columns to a few partial STATE components per (target, variable),
 * the ranks combine the components element-wise with ONE collective (sum, or max for minimum / maximum), the owner of a
 * target finalises.  Components (v = value, w = weight; "valid" = v not NaN):
 *   XR_MEAN, XR_FIRST_ORDER_CONSERVATIVE   [sum w v, sum w]                     over valid          -> c0 / c1 resp. c0
 *   XR_SUM                                 [sum v,   sum w]                     over valid          -> c0
 *   XR_HARMONIC_MEAN                       [sum w,   sum w / v]                 valid, v != 0, w > 0 -> c0 / c1
 *   XR_GEOMETRIC_MEAN                      [sum w (ALL entries), sum w ln v, sum w (v > 0, w > 0), #(v < 0)]
 *                                                                                                     -> exp(c1 / c2)
 *   XR_MINIMUM / XR_MAXIMUM                [max(-v) resp. max v, max w]         over valid (combine with MAX)
 * with NaN where the reference returns NaN (zero weight sum, a negative value under the geometric mean ...).
 * xr_partial_components(method) -> number of components (0: the reducer needs whole rows: mode, percentiles,
 * max_overlap), xr_partial_combine_is_max(method) -> 1 if the collective is MAX.
 * Layouts: planes float64 [C, K, T] (dense exchange) or rows float64 [T, C * K] (sparse exchange, component-major
 * inside a row); t runs over the CALLER's row order of the matrix. */
int xr_partial_components(int method);
int xr_partial_combine_is_max(int method);
int xr_apply_partial_dev(const xr_csr *csr, int method, const void *source_dev, int source_dtype, int64_t K,
                         double *out_dev, int rows_layout);
/* Weight build + partial state of ONE call: what a rank of the sharded regridder does per rebuild (xugrid/regrid/regridder.py:386-398
 * + the per-target reduction of :41-67 restricted to the rank's columns).  As xr_overlap_apply_dev: for K = 1 the partial-state
 * kernel is enqueued before the host has read the matrix' sizes back, so the one host round trip of the build hides behind it. */
int xr_overlap_partial_dev(xr_mesh *tree, xr_mesh *query, int relative, int method, const void *source_dev, int source_dtype,
                           int64_t K, double *out_dev, int rows_layout, xr_csr **out);
/* identity element of the combine step in the same layouts (buffers of targets a rank has no weight for) */
int xr_partial_fill_identity_dev(int method, double *planes_dev, int64_t K, int64_t T);
/* out_dev float64 [K, T] from combined planes [C, K, T] */
int xr_finalize_partial_dev(int method, const double *planes_dev, int64_t K, int64_t T, double *out_dev);
/* owner side of the sparse exchange in one launch: rows_dev float64 [R, C * K] received partial rows; target t of this
 * rank's slice combines rows order_dev[indptr_dev[t] .. indptr_dev[t+1]) in that (sender) order and is finalised:
 * out_dev float64 [K, n_targets]. */
int xr_reduce_partial_rows_dev(int method, const double *rows_dev, const int64_t *indptr_dev, const int64_t *order_dev,
                               int64_t n_targets, int64_t K, double *out_dev);

/* ---- filling NaN entries (xugrid UgridDataArrayAccessor.laplace_interpolate / interpolate_na) ------------------- */
/* A symmetric adjacency on the device: CSR from the host (int64 indptr [n+1], indices [nnz] ascending per row), weights
 * `data` [nnz] (NULL: none; the fill then runs with unit weights only) and connected-component labels [n] (NULL: computed
 * on the device -- the smallest node id of each component, by minimum-label propagation to a fixed point). */
typedef struct xr_graph xr_graph;
int xr_graph_from_csr(const int64_t *indptr, const int64_t *indices, const double *data, int64_t n, int64_t nnz,
                      const int64_t *labels, xr_graph **out);
int xr_graph_info(const xr_graph *graph, int64_t *n, int64_t *nnz);
/* any pointer may be NULL; indptr [n+1], indices [nnz], data [nnz], labels [n] */
int xr_graph_download(const xr_graph *graph, int64_t *indptr, int64_t *indices, double *data, int64_t *labels);
int xr_graph_destroy(xr_graph *graph);
/* Laplace fill of K slices in_dev float64 [K, n] -> out_dev [K, n] (device pointers; in_dev is not modified): unpreconditioned
 * CG on the diagonally scaled system of xugrid/ugrid/interpolate.py:286-329 with scipy's stopping rule (||r|| < max(atol,
 * rtol ||b||) before every iteration, x0 = 0), all slices together; the host reads the slices' state every `chunk`
 * iterations (<= 0: default).  Per slice: iterations_out [K] and status_out [K] = XR_FILL_*.  Slices without NaN are copied. */
#define XR_FILL_CONVERGED 0
#define XR_FILL_MAXITER 1   /* the last iterate after maxiter iterations */
#define XR_FILL_BREAKDOWN 2 /* p.Ap <= 0 or not finite */
#define XR_FILL_NODATA 3    /* the slice holds no value at all */
int xr_graph_laplace_fill_dev(const xr_graph *graph, const double *in_dev, double *out_dev, int64_t K, int use_weights,
                              double atol, double rtol, int64_t maxiter, int64_t chunk, int64_t *iterations_out,
                              int *status_out);
/* nearest fill: null entries of in_dev [K, n] take the value of the nearest non-null entry (points xy_dev float64 [n, 2],
 * Euclidean distance strictly below max_distance (INFINITY: no limit), lowest index among equidistant ones); the rest stays
 * NaN.  XR_ERR_INVALID "All values are NA." for a slice without any value. */
int xr_nearest_fill_dev(const double *xy_dev, int64_t n, const double *in_dev, double *out_dev, int64_t K, double max_distance);

/* ---- edge topology of a device mesh (xugrid_amd/connectivity.py: edge_connectivity, invert_dense, face_face_connectivity,
 * node_node_connectivity) built where the mesh is, from its faces_raw; every array in the caller's numbering and equal,
 * element for element, to what the host route gives for the same faces:
 *   edge_node [n_edge, 2]  unique undirected edges (lower, higher node), lexicographic; the edge id is the rank
 *   face_edge [n_face, m]  edge of slot k (node k -> its successor, the last node closing onto node 0), valid entries
 *                          compacted to the left, -1 trailing; a slot whose two nodes are equal is no edge
 *   edge_face [n_edge, 2]  the faces of each edge ascending, -1 in column 1 for an exterior edge
 *   face_face CSR          one entry per pair of faces sharing an edge, columns ascending, data = the edge id (the SUM of
 *                          the ids where two faces share several edges, as scipy's coo -> csr)
 *   node_node CSR          over all n_node nodes (unused nodes: empty rows), columns ascending, data = the edge id
 *   exterior_edge [n_edge], exterior_face [n_face]  flags (a face with at least one exterior edge)
 * An edge with more than two faces does not fit two columns: the builder counts those (n_nonmanifold), keeps nothing else
 * when there are any and still returns XR_OK; every other call on such a handle but xr_topology_info / _destroy is
 * XR_ERR_INVALID.  `mesh` must outlive the handle. */
typedef struct xr_topology xr_topology;
int xr_topology_create(xr_mesh *mesh, xr_topology **out);
/* any pointer may be NULL */
int xr_topology_info(const xr_topology *topology, int64_t *n_edge, int64_t *n_exterior_edge, int64_t *face_face_nnz,
                     int64_t *node_node_nnz, int64_t *n_nonmanifold);
/* nodes with more distinct neighbours than the per-thread list holds (16): those the wave-per-node kernel listed */
int xr_topology_long_nodes(const xr_topology *topology, int64_t *n_long_nodes);
/* int64 outputs, any pointer may be NULL: edge_node [n_edge*2], face_edge [n_face*m], edge_face [n_edge*2], ff_indptr
 * [n_face+1], ff_indices / ff_data [face_face_nnz], nn_indptr [n_node+1], nn_indices / nn_data [node_node_nnz],
 * exterior_edge [n_edge], exterior_face [n_face] (0 / 1) */
int xr_topology_download(const xr_topology *topology, int64_t *edge_node, int64_t *face_edge, int64_t *edge_face,
                         int64_t *ff_indptr, int64_t *ff_indices, int64_t *ff_data, int64_t *nn_indptr, int64_t *nn_indices,
                         int64_t *nn_data, int64_t *exterior_edge, int64_t *exterior_face);
/* edge midpoints 0.5 * (a + b) into xy_dev float64 [n_edge, 2] (a device pointer) */
int xr_topology_edge_xy_dev(const xr_topology *topology, double *xy_dev);
/* exterior_face as uint8 [n_face] into a device buffer (the `exterior` argument of xr_graph_binary_iterate_dev) */
int xr_topology_exterior_face_dev(const xr_topology *topology, uint8_t *flags_dev);
int xr_topology_destroy(xr_topology *topology);
/* node -> face and node -> edge as CSR over all n_node nodes (connectivity.invert_dense_to_sparse of face_node and of
 * edge_node; unused nodes: empty rows), int64 outputs, any pointer may be NULL: nf_indptr [n_node+1], nf_indices
 * [nf_indptr[n_node]] faces ascending per row, ne_indptr [n_node+1], ne_indices [node_node_nnz] edges ascending per row.
 * node -> edge is the node_node CSR under another name: its rows have ascending neighbours, and edges are numbered
 * lexicographically by (lower, higher) node, so its data -- the edge ids -- ascend too.  A face that names a node twice
 * appears twice in that node's row (the host route's coo -> csr merges the two). */
int xr_topology_download_node_tables(const xr_topology *topology, int64_t *nf_indptr, int64_t *nf_indices, int64_t *ne_indptr,
                                     int64_t *ne_indices);
/* The xr_graph of the faces (facet 2, XR_FACET_FACE below) or nodes (0, XR_FACET_NODE) straight from the device CSR: component labels by the
 * label kernels, weights mean(d) / d (ugridbase.py:962-970) with d the distance between the connected face centroids or
 * nodes; the mean is a fixed-order sum of block partials (the same bits on every run). */
int xr_graph_from_topology(const xr_topology *topology, int facet, xr_graph **out);
/* rounds of minimum-label propagation the component labelling of this graph took (0: labels given by the caller) */
int xr_graph_label_rounds(const xr_graph *graph, int64_t *rounds);

/* ---- graph operations (xugrid connected_components / binary_dilation / binary_erosion) --------------------------- */
/* labels_dev int64 [n] (a device pointer): components numbered 0 .. n_components-1 in the order of their smallest member,
 * which is the numbering of scipy.sparse.csgraph.connected_components */
int xr_graph_components_dev(const xr_graph *graph, int64_t *labels_dev, int64_t *n_components);
/* `iterations` (>= 1) Jacobi steps of xugrid/ugrid/connectivity.py _binary_iterate on K slices in_dev uint8 [K, n] ->
 * out_dev [K, n] (in_dev is not modified): an entry becomes `value` iff a neighbour's old state differs from its own; then
 * entries flagged in mask_dev uint8 [n] (or NULL) are set to !value (sic: the reference's `output[mask] = not value`);
 * after the FIRST step only, entries flagged in exterior_dev uint8 [n] (or NULL) are set to `value`. */
int xr_graph_binary_iterate_dev(const xr_graph *graph, const uint8_t *in_dev, uint8_t *out_dev, int64_t K, int value,
                                int64_t iterations, const uint8_t *mask_dev, const uint8_t *exterior_dev);

/* ---- renumbering (scipy.sparse.csgraph.reverse_cuthill_mckee, symmetric_mode=True; xugrid Ugrid2d.reverse_cuthill_mckee) ---- */
/* order_dev int64 [n] (a device pointer): the permutation in scipy's reversed order, new row i = old row order_dev[i].
 * The graph must be symmetric with ascending columns; an entry that repeats a column of its row counts in the degree (as in scipy)
 * and is otherwise ignored.
 * degree = entries of the row, plus one where the row holds its diagonal entry (scipy's count; the diagonal is never visited).
 * scipy's routine is a sequential breadth-first search: the seed is the first unvisited vertex in the order of ascending
 * degree; each visited row appends its unvisited neighbours in stored column order; the new entries of that one row are then
 * insertion-sorted by degree (stable); a new seed follows whenever a component is exhausted; the order is reversed at the end.
 * The engine runs it level by level: each unvisited neighbour j of level L takes as parent the smallest position in the order
 * among its neighbours in level L, and level L + 1 is the claimed vertices sorted by (parent position, degree[j], j) -- equal to
 * the sequential search element for element.  The claim is an integer minimum: the result is the same on every run.
 * The engine's rule: seeds are taken in (degree, id) order, which is the stable sort.  Everything else follows scipy.  scipy
 * takes its seeds from numpy's default, unstable argsort of the degrees: which of several unvisited vertices of equal least
 * degree it picks depends on numpy's sort kernel.  Where scipy's answer does not depend on its tie order, the engine equals
 * scipy exactly.  Elsewhere it equals the restatement (the same loop with a stable argsort).
 * levels_out (or NULL): the breadth-first levels run, every seed being a level of one.  The host reads one word per chunk of
 * levels, not per level; no kernel waits for another block. */
int xr_graph_rcm_dev(const xr_graph *graph, int64_t *order_dev, int64_t *levels_out);

/* ---- balanced part labels (xugrid Ugrid2d.label_partitions / partition, ugridbase.py:1508-1596) --------------------------- */
/* labels_dev int64 [n] (a device pointer): a label in [0, n_part) for every vertex of the symmetric graph (ascending columns;
 * the diagonal is ignored), from xy_dev float64 [n, 2] and weights_dev int64 [n], all >= 0 (NULL, or all zero: all ones).
 * 1 <= n_part <= n, and 100 * n_part * sum(weights) must fit in int64.  The reference hands the graph to METIS, whose
 * labels are not a function of its input that can be written down; the engine follows this rule (numpy: tests/partlabel_cases.py).
 * With P = n_part, w the weights, T = sum(w):
 * 1. Key.  lo, hi = the bounds of xy per axis, side = max(hi_x - lo_x, hi_y - lo_y); the cell of a coordinate v on its axis is
 *    floor((v - lo) * (65536.0 / max(side, 1e-300))) clamped to [0, 65535] (two IEEE operations, not contracted); the key is
 *    the 32-bit Hilbert index of (cx, cy): d = 0; for s = 32768, 16384 .. 1: rx = (x & s) > 0, ry = (y & s) > 0,
 *    d += s * s * ((3 * rx) ^ ry); if ry == 0: (if rx == 1: x = 65535 - x, y = 65535 - y), swap x and y.
 * 2. Seed.  order = the vertices by (key, id) ascending; before(v) = the sum of w over the vertices in front of v in order;
 *    label = min(P - 1, before(v) * P / T) in integers.
 * 3. Refinement.  L = max(ceil(T / P), floor(103 T / (100 P))), Lmin = min(floor(T / P), ceil(97 T / (100 P))); at most 16
 *    synchronous rounds on a snapshot of the labels, none when P == 1 or floor(T / P) == 0.  In a round, for every vertex v
 *    with label a: its neighbours (the entries of its row other than v) are counted per label; b = the label other than a with
 *    the largest count, the smallest such label on a tie; gain = count[b] - count[a]; v is a candidate when gain > 0, and a
 *    mover unless a neighbour is a candidate that comes first by (gain descending, id ascending) -- movers are an
 *    independent set, so an accepted move lowers the edge cut by exactly its gain.  With W the parts' weights at the start
 *    of the round: the movers into b, ranked by (gain descending, id ascending), pass the destination budget while the sum of
 *    w over the movers into b ranked up to and including them is <= L - W[b]; the movers out of a, ranked the same way, pass
 *    the source budget while that sum is <= W[a] - Lmin (both sums include movers that fail the other budget).  Movers that
 *    pass both take label b.  A round that accepts nothing is the last.
 * Every decision is integer arithmetic or an order-independent minimum / maximum: the labels are the same on every run.
 * What holds: the edge cut never rises from round to round, and part weights that start within [Lmin, L] stay there.
 * info (or NULL) int64[4]: rounds run (a last round without a move counts), moves accepted, edge cut of the seed, edge cut of
 * the result.  State stays in HBM; the host reads the control words once per four rounds; no kernel waits for another block. */
int xr_graph_partition_dev(const xr_graph *graph, const double *xy_dev, const int64_t *weights_dev, int64_t n_part,
                           int64_t *labels_dev, int64_t *info);
/* A new mesh with the nodes of `mesh` (all of them, used or not, coordinates copied) and the face table
 * faces[order_dev[i], :] (order_dev int64 [n_face], a device pointer; an id outside [0, n_face) is XR_ERR_INVALID). */
int xr_mesh_reorder_faces_dev(const xr_mesh *mesh, const int64_t *order_dev, xr_mesh **out);

/* ---- filling NaN entries of a network along its edges (xugrid Ugrid1d._nearest_interpolate: multi-source dijkstra) ---- */
/* The graph of a network (node_xy_dev float64 [n_node, 2], edges_dev int64 [n_edge, 2], device pointers) for the nearest calls below.
 * facet XR_FACET_NODE: the reference's node_node_connectivity over ALL n_node nodes (unused nodes: empty rows), columns ascending,
 *   data = length of the joining edge.
 * facet XR_FACET_EDGE: the reference's edge_edge_connectivity (every OTHER edge sharing a node, each once, columns ascending),
 *   data = 0.5 * (length[i] + length[j]).
 * length = sqrt(dx*dx + dy*dy), uncontracted (the unit is compiled with the Makefile's -ffp-contract=off like the rest).
 * problems[0] = self-loops (a == b), problems[1] = edges repeating an earlier edge's node pair in either orientation.
 * With any problem *out is NULL and the call is still XR_OK.  nnz >= 2^31 is XR_ERR_LIMIT.  Labels by the existing label kernels.
 * An edge that names a node outside [0, n_node) is XR_ERR_INVALID.  (XR_FACET_* are defined further down.) */
int xr_network_graph_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, int facet,
                         xr_graph **out, int64_t *problems);
/* Per slice k and vertex v the state is (d, s).  Sources start at (0.0, v); every other vertex starts at (inf, none).
 * The result is the fixed point of
 *     (d_v, s_v) = lexicographic min of the start value and, over the CSR entries (v, u, w), of (fl(d_u + w), s_u),
 *                  keeping only candidates with fl(d_u + w) <= limit.
 * limit is inclusive, as scipy's; INFINITY means none.
 * is_source_dev uint8 [K,n]; distance_dev float64 [K,n] (inf where unreached), source_dev int64 [K,n] (-1 where unreached); either
 * may be NULL.
 * The host reads one "changed" word per `chunk` rounds (<= 0: default), as the CG does.  rounds_out gets the rounds run (the one that
 * found nothing to change included).
 * The graph must carry weights, all finite and >= 0.  Zero weights are allowed.
 * The rounds are pulls whose results go to a second buffer, a block sweeping its own vertices several times within a round (DESIGN
 * section 17): no state is read while it is written, the same bits on every run.  A vertex takes the minimum of its previous state
 * and the candidates, so states only decrease and the rounds end; the distances are Dijkstra's bits, the source is the lowest id
 * among equidistant ones. */
int xr_graph_nearest_dev(const xr_graph *graph, const uint8_t *is_source_dev, int64_t K, double limit, int64_t chunk,
                         double *distance_dev, int64_t *source_dev, int64_t *rounds_out);
/* Sources are the non-NaN entries of in_dev [K,n].  out = in where valid, in[s_v] where reached, NaN elsewhere.
 * A slice without NaN is copied.  A slice without any value is XR_ERR_INVALID "All values are NA.", as xr_nearest_fill_dev. */
int xr_graph_nearest_fill_dev(const xr_graph *graph, const double *in_dev, double *out_dev, int64_t K, double limit,
                              int64_t chunk, int64_t *rounds_out);

/* ---- moving data between the facets of a mesh (xugrid UgridDataArray.ugrid.to_node / to_edge / to_face,
 * core/dataarray_accessor.py:300-416) ------------------------------------------------------------------------------- */
/* The table is {target}_{source}_connectivity, int32: dense [n_target, width] with -1 fill (face_node, face_edge, edge_node,
 * edge_face) or CSR with `width` the widest row (node_face, node_edge).  in_dev [K, n_source] of dtype XR_F64 / XR_F32 (widened
 * to float64 first), never modified.
 *   XR_FACET_RAW   out_dev float64 [K, n_target, width]: out[k, t, j] = in[k, table[t, j]], NaN where the table has no entry
 *                  (obj.isel(indexer).where(indexer != -1))
 *   XR_FACET_MEAN / _SUM / _MIN / _MAX   out_dev float64 [K, n_target]: the reference's .mean(dim) and its kin over that new
 *                  dimension, without the [.., width] intermediate.  NaN contributors are skipped (xarray's skipna); a target
 *                  without a valid contributor gets NaN, 0.0 for the sum.  The sum runs over the row's entries in table order,
 *                  sequentially, in float64, and the mean is that sum divided once by the count: the same bits on every run.
 * Before anything is read through an index the table is checked once per call: an index >= n_source, row pointers that do
 * not start at 0 or decrease, or a row longer than `width` is XR_ERR_INVALID.  Rows may have any length.
 * Option "facet_tile" = 1 keeps one slice per lane instead of eight (measurement switch; no result depends on it). */
#define XR_FACET_MEAN 0
#define XR_FACET_SUM 1
#define XR_FACET_MIN 2
#define XR_FACET_MAX 3
#define XR_FACET_RAW 4
/* ... through the tables of a topology where they are; target / source: XR_FACET_NODE (0), XR_FACET_EDGE (1), XR_FACET_FACE
 * (2), different from each other.  edge_face always has two columns here (the host table has one when no edge is shared). */
int xr_topology_facet_map_dev(xr_topology *topology, int target, int source, int form, const void *in_dev, int dtype, int64_t K,
                              double *out_dev);
/* `width` of that table: m for the face tables, 2 for the edge tables, the widest row for the node tables (one reduction over
 * the row pointers on first request, then kept) */
int xr_topology_facet_width(xr_topology *topology, int target, int source, int64_t *width);
/* ... through the caller's int32 device tables: ptr_dev NULL -> idx_dev is dense [n_target, width]; else CSR, ptr_dev
 * [n_target+1], idx_dev [ptr[n_target]], `width` at least the widest row.  The route of host-built grids, rectilinear grids,
 * non-manifold device grids and Ugrid1d. */
int xr_facet_map_dev(const int32_t *ptr_dev, const int32_t *idx_dev, int64_t n_target, int64_t width, int64_t n_source, int form,
                     const void *in_dev, int dtype, int64_t K, double *out_dev);

/* ---- sampling mesh data at points and along lines (xugrid sel_points / sel / intersect_line / locate_nearest_*) ---- */
/* Nearest-neighbour index over n fixed points xy_dev float64 [n, 2] (a device pointer): what Ugrid2d.node_kdtree /
 * edge_kdtree / face_kdtree are in the reference (scipy KDTree, xugrid/ugrid/ugridbase.py:1113-1123, ugrid2d.py:902-906).
 * A uniform grid of about two points per cell; the handle keeps its own copy of the coordinates in cell order, so the
 * caller's array may go.  n = 0 is XR_ERR_INVALID. */
typedef struct xr_nn xr_nn;
int xr_nn_create_dev(const double *xy_dev, int64_t n, xr_nn **out);
/* ... over the nodes or the face centroids (connectivity.centroids) of a mesh, straight from its device arrays: the index
 * of a grid made by Ugrid2d.from_device_arrays needs no host copy of the mesh. */
#define XR_FACET_NODE 0
#define XR_FACET_EDGE 1
#define XR_FACET_FACE 2
int xr_nn_create_mesh(xr_mesh *mesh, int facet, xr_nn **out);
int xr_nn_info(const xr_nn *index, int64_t *n, int64_t *n_cell);
int xr_nn_destroy(xr_nn *index);
/* KDTree.query(points, distance_upper_bound=max_distance) as locate_nearest_node / _edge / _face call it
 * (ugridbase.py:1261-1303, ugrid2d.py:1007-1027): query_xy_dev float64 [n_query, 2] -> index_out_dev int64 [n_query], the id
 * of the nearest indexed point or -1.  Squared distance dx * dx + dy * dy in float64; a point counts only STRICTLY below
 * max_distance (scipy's rule; INFINITY: no limit); the lowest id wins among equidistant points (scipy's choice there is
 * arbitrary); a query with a NaN coordinate gets -1. */
int xr_nn_query_dev(const xr_nn *index, const double *query_xy_dev, int64_t n_query, double max_distance,
                    int64_t *index_out_dev);
/* obj.isel(points).where(valid, fill_value) of sel_points (ugridbase.py:1240-1258) for K slices: in_dev [K, n] of dtype
 * XR_F64 / XR_F32, index_dev int64 [n_point] -> out_dev float64 [K, n_point], out[k, p] = in[k, index[p]], fill_value where
 * index[p] < 0.  An index >= n is XR_ERR_INVALID (checked once per call, before anything is read through it). */
int xr_gather_points_dev(const void *in_dev, int dtype, int64_t K, int64_t n, const int64_t *index_dev, int64_t n_point,
                         double fill_value, double *out_dev);
/* Coordinates of a line section (intersect_linestring, ugridbase.py:1438-1452; section_coordinates_2d,
 * selection_utils.py:27-32): pieces_dev float64 [n_piece, 2, 2] as xr_edge_pieces returns them, piece_segment_dev int64
 * [n_piece] the segment each piece was cut from, segment_xy_dev float64 [n_segment, 2, 2] the line's segments in order.
 * mid = 0.5 (p0 + p1) -> mid_xy_out_dev [n_piece, 2]; s = |mid - start of the segment| + summed length of the segments in
 * front of it -> s_out_dev [n_piece].  All pointers are device pointers; the caller orders the pieces by s. */
int xr_section_coords_dev(const double *pieces_dev, const int64_t *piece_segment_dev, int64_t n_piece,
                          const double *segment_xy_dev, int64_t n_segment, double *mid_xy_out_dev, double *s_out_dev);

/* ---- burning vector geometry into the faces of a mesh (xugrid.burn_vector_geometry, xugrid/ugrid/burn.py) ---------------- */
/* All pointers are device pointers; coordinates float64 [n, 2], offsets int64.  A winner array int32 [n_face] holds per face
 * the HIGHEST id of a geometry that covers it (the reference's sequential loop: later geometries overwrite earlier ones),
 * -1 for none.  Offsets must start at 0, end at the count they index and never decrease (XR_ERR_INVALID).
 * xr_burn_polygons_dev (_locate_polygon / _burn_polygons, burn.py:59-137): the layout of shapely.to_ragged_array -- ring r
 * holds the vertices [ring_offsets[r], ring_offsets[r + 1]), polygon g the rings [polygon_offsets[g], polygon_offsets[g + 1]),
 * the first its exterior, the others holes; rings are cyclic, closed (first == last) or open.  Face f is in polygon g iff its
 * centroid (connectivity.centroids) passes the per-segment rule of xr_locate_points with the mesh's default tolerance --
 * within tolerance of a segment, or an odd number of crossings -- over all ring segments of g.  all_touched != 0 adds every
 * face in which a ring segment of g has a piece of positive length (the rule of xr_edge_length_csr), unless the segment
 * lies exactly on the line of one of the face's edges (a border drawn along a mesh line touches neither neighbour, as in
 * the reference).  No triangulation.
 * Option "burn_strips" (> 0) forces the number of strips of the segment index; no result depends on it.  XR_ERR_LIMIT when
 * the strips would list 2^31 segments or more. */
int xr_burn_polygons_dev(xr_mesh *mesh, const double *coords_dev, int64_t n_vertex, const int64_t *ring_offsets_dev,
                         int64_t n_ring, const int64_t *polygon_offsets_dev, int64_t n_polygon, int all_touched,
                         int32_t *winner_dev);
/* _burn_lines (burn.py:153-181): line l joins the consecutive vertices [line_offsets[l], line_offsets[l + 1]); a face is
 * covered where a segment has a piece of positive length in it. */
int xr_burn_lines_dev(xr_mesh *mesh, const double *coords_dev, int64_t n_vertex, const int64_t *line_offsets_dev, int64_t n_line,
                      int32_t *winner_dev);
/* _burn_points (burn.py:140-150): the face xr_locate_points finds with the default tolerance.  A point in no face burns
 * nothing (the reference writes it into the LAST face through the index -1). */
int xr_burn_points_dev(xr_mesh *mesh, const double *coords_dev, int64_t n_point, int32_t *winner_dev);
/* out[f] = value of the point winner, else of the line winner, else of the polygon winner, else fill (burn.py:253-260:
 * polygons, then lines, then points).  A NULL winner array: no geometry of that kind; NULL values: 1.0 (column=None). */
int xr_burn_combine_dev(int64_t n_face, const int32_t *polygon_winner_dev, const double *polygon_values_dev,
                        const int32_t *line_winner_dev, const double *line_values_dev, const int32_t *point_winner_dev,
                        const double *point_values_dev, double fill, double *out_dev);

/* ---- polygonizing face data (xugrid.polygonize, xugrid/ugrid/polygonize.py) ---------------------------------------------- */
/* Regions of equal value -> polygon rings, in the layout xr_burn_polygons_dev reads (shapely.to_ragged_array).  data_dev
 * [n_face] of dtype XR_F64 / XR_F32 / XR_I32 (a device pointer, never written).  NaN faces belong to no polygon.  A region is a
 * maximal set of valid faces with == values joined through shared edges; regions are numbered by the rank of their smallest
 * face, polygon p IS region p and values[p] the value of that face.  Every region is one polygon: its exterior ring (the ring
 * of positive shoelace sum) first, then its holes ascending by leader, the half-edge of smallest (face, slot), where every
 * ring also starts; rings are closed (first vertex == last).  A ring passes more than once through a node at which its region
 * touches itself.  XR_ERR_INVALID: a non-manifold mesh, a face with data whose shoelace sum is zero or not finite
 * ("degenerate face"), or rings that do not close ("internal error").  All-NaN data gives zero polygons and offsets [0]. */
typedef struct xr_polygons xr_polygons;
int xr_polygonize_dev(xr_topology *topology, const void *data_dev, int dtype, xr_polygons **out);
/* n_vertex = n_halfedge + n_ring; label_rounds: hook launches of the region labelling (the last one changes nothing) */
int xr_polygons_info(const xr_polygons *p, int64_t *n_polygon, int64_t *n_ring, int64_t *n_vertex, int64_t *n_halfedge,
                     int64_t *label_rounds);
/* device-to-host transfers the call waited for (label_rounds + 9; the ring table is three of them) */
int xr_polygons_readbacks(const xr_polygons *p, int64_t *readbacks);
/* coords float64 [n_vertex, 2], ring_offsets int64 [n_ring + 1], polygon_offsets int64 [n_polygon + 1], values float64
 * [n_polygon], face_polygon int64 [n_face] (-1 for a NaN face) into the caller's device arrays */
int xr_polygons_copy_dev(const xr_polygons *p, double *coords_dev, int64_t *ring_offsets_dev, int64_t *polygon_offsets_dev,
                         double *values_dev, int64_t *face_polygon_dev);   /* any pointer may be NULL */
int xr_polygons_destroy(xr_polygons *p);

/* ---- sub-meshes (Ugrid2d.topology_subset, ugrid2d.py:1138-1216; clip_box :1218-1226; isel :1228-1288) ----------------------
 * xr_mesh_subset_dev: a NEW device-resident mesh of the faces face_index_dev int64[n] (device memory; ids unique, any order):
 *   - its faces are faces[index] in the order given; the table keeps its width n_max_node, the caller's vertex order and -1
 *     in the unused slots, even when every kept face is shorter;
 *   - its nodes are the distinct nodes of those faces in ascending old id, renumbered by their dense rank (np.unique, then
 *     connectivity.renumber); the coordinates are copied, so they are bit-identical to the source's.
 * problems[0]: ids outside [0, n_face) (negative ones included: nothing wraps), problems[1]: ids that repeat an earlier one.
 * If either is non-zero *out is NULL and the call still returns XR_OK: the caller words the exception.  Nothing is read
 * through an id before it has been compared with its range.  *is_identity = 1 (and *out NULL) when the selection is every
 * face in order: the caller keeps the mesh it has.  n == 0 gives the empty mesh (0 faces, 0 nodes) without a launch.
 * XR_ERR_INVALID: n > n_face; XR_ERR_LIMIT: n * n_max_node leaves the int32 range.  One synchronising read-back per call (the
 * number of kept nodes and the three status words in one copy).
 * xr_mesh_subset_node_index_dev: the old id of every node of such a mesh, ascending -> int64[n_node] in device memory;
 * XR_ERR_INVALID for a mesh that xr_mesh_subset_dev did not make. */
int xr_mesh_subset_dev(xr_mesh *mesh, const int64_t *face_index_dev, int64_t n, xr_mesh **out, int *is_identity, int64_t *problems);
int xr_mesh_subset_node_index_dev(const xr_mesh *subset, int64_t *index_dev);
/* The same two counts for any index int64[n] into a dimension of `size` entries (the node and edge indexers of isel), and the
 * number of i with a[i] != b[i] (isel's pre- and post-check, pandas Index.equals on arrays of one length). */
int xr_index_check_dev(const int64_t *index_dev, int64_t n, int64_t size, int64_t *problems);
int xr_index_mismatch_dev(const int64_t *a_dev, const int64_t *b_dev, int64_t n, int64_t *count);
/* An ascending index made on the device: flags int32[n] -> exclusive scan -> compaction, one read-back (its length).  The
 * handle owns int32 ids; xr_index_copy_dev widens them into the caller's int64[n] device array.
 *   xr_index_from_mask_dev          nonzero of a one-byte mask uint8[n]
 *   xr_mesh_box_faces_dev           Ugrid2d.locate_bounding_box (ugrid2d.py:1029-1052) on the mesh's device centroids: the faces
 *                                   with xmin <= x < xmax and ymin <= y < ymax, exactly these four comparisons (a NaN centroid
 *                                   is outside)
 *   xr_mesh_faces_of_nodes_dev      the faces with at least one of the nodes node_index_dev[n] (unique of
 *                                   node_face_connectivity[node_index].data); ids out of range select nothing
 *   xr_topology_faces_of_edges_dev  the faces in either column of edge_face_connectivity[edge_index], without the fill
 *   xr_topology_subset_edges_dev    the distinct ids of face_edge_connectivity[face_index], without the fill: since edges are
 *                                   numbered lexicographically by (lower, higher) node and the node renumbering is monotone,
 *                                   edge k of the sub-mesh IS old edge index[k]
 * The two topology calls return XR_ERR_INVALID for a non-manifold topology (it keeps no tables: the caller takes the host
 * route). */
typedef struct xr_index xr_index;
int xr_index_from_mask_dev(const uint8_t *mask_dev, int64_t n, xr_index **out);
int xr_mesh_box_faces_dev(xr_mesh *mesh, double xmin, double ymin, double xmax, double ymax, xr_index **out);
int xr_mesh_faces_of_nodes_dev(xr_mesh *mesh, const int64_t *node_index_dev, int64_t n, xr_index **out);
int xr_topology_faces_of_edges_dev(const xr_topology *topology, const int64_t *edge_index_dev, int64_t n, xr_index **out);
int xr_topology_subset_edges_dev(const xr_topology *topology, const int64_t *face_index_dev, int64_t n, xr_index **out);
int xr_index_info(const xr_index *index, int64_t *n);
int xr_index_copy_dev(const xr_index *index, int64_t *out_dev);
int xr_index_destroy(xr_index *index);

/* ---- joining meshes (Ugrid2d.merge_partitions, partitioning.py:81-148), matching point sets (connectivity.index_like,
 * connectivity.py:38-61), splitting by label (partitioning.py:16-27); xr_merge.hip, DESIGN section 15 -------------------------
 * All of it rests on one primitive, an open-addressing key table in HBM that finds the FIRST row of every set of equal rows
 * (insert with atomicCAS / atomicMin, look-up in a second launch; option merge_table_slack = 1 gives it the smallest legal
 * capacity).  No sort.
 *
 * xr_merge_meshes_dev: the meshes parts[0 .. n_part) joined into one.
 *   nodes  the partitions' node_xy concatenated in the order given; two nodes are one when both coordinates compare equal as
 *          doubles (-0.0 == 0.0; a row holding NaN equals nothing, not even itself); the first occurrence is kept, bit for
 *          bit, and kept nodes keep their concatenation order.
 *   faces  every table widened to m = max n_max_node with -1, real slots mapped to merged node ids; two faces are one when
 *          their rows are equal after sorting each row, the -1 taking part; the first occurrence is kept with its slot order.
 * The handle owns the merged mesh (xr_merge_take_mesh hands it out once; the caller destroys it with xr_mesh_destroy), the
 * merged id of every concatenated node (xr_merge_node_inverse_copy_dev, int64[sum n_node]) and the kept rows per partition.
 * One synchronising read-back per call: both scans at the 2 (n_part + 1) partition boundaries in one copy.
 * XR_ERR_LIMIT: the concatenated nodes or face slots leave the int32 range.
 *
 * xr_merge_edges_dev: the same question for the partitions' DERIVED edges (their xr_topology, all manifold): an edge is kept
 * when its merged (lower, higher) node pair occurs at no earlier edge of the concatenation; `merged` is the topology of the
 * merged mesh, in whose node -> node CSR (data = edge id) every kept edge's own id there is looked up.  One read-back.
 *
 * xr_merge_index_info / xr_merge_index_copy_dev: facet 0 nodes, 1 edges (after xr_merge_edges_dev), 2 faces.  part >= 0: the
 * ascending LOCAL ids of that partition's kept rows; part == -1: all kept rows as ids into the concatenation.  position != 0
 * (edges only): instead the merged mesh's own edge id of each of those kept edges. */
typedef struct xr_merge xr_merge;
int xr_merge_meshes_dev(xr_mesh *const *parts, int64_t n_part, xr_merge **out);
int xr_merge_edges_dev(xr_merge *merge, const xr_topology *const *parts, int64_t n_part, const xr_topology *merged);
int xr_merge_info(const xr_merge *merge, int64_t *n_part, int64_t *n_node_all, int64_t *n_face_all);
int xr_merge_take_mesh(xr_merge *merge, xr_mesh **mesh);
int xr_merge_index_info(const xr_merge *merge, int facet, int64_t part, int64_t *n);
int xr_merge_index_copy_dev(const xr_merge *merge, int facet, int64_t part, int position, int64_t *out_dev);
int xr_merge_node_inverse_copy_dev(const xr_merge *merge, int64_t *out_dev);
int xr_merge_destroy(xr_merge *merge);
/* index_out_dev[i] = the row j of a float64[n, 2] whose key equals the key of row i of b (-1: none, or the pair differs by
 * more than `tolerance` on an axis).  Key: the coordinate pair (tolerance == 0) or rint(xy / tolerance).  problems[0]: keys
 * that repeat inside a or inside b; problems[1]: rows of b without a partner.  The caller words the errors; one read-back. */
int xr_index_like_dev(const double *a_dev, const double *b_dev, int64_t n, double tolerance, int64_t *index_out_dev, int64_t *problems);
/* labels int64[n] in device memory: their range (clamped to [-1, INT32_MAX]; n == 0: 0, -1), then the ids grouped by label
 * 0 .. n_label - 1 and ascending inside a label -- flags per label laid out label-major, ONE exclusive scan, a placement
 * without atomics; bounds[n_label + 1] (host): where each label's ids start.  One read-back each.  XR_ERR_LIMIT: n * n_label
 * leaves the int32 range. */
typedef struct xr_label_order xr_label_order;
int xr_labels_range_dev(const int64_t *labels_dev, int64_t n, int64_t *min_label, int64_t *max_label);
int xr_labels_order_dev(const int64_t *labels_dev, int64_t n, int64_t n_label, xr_label_order **out, int64_t *bounds);
int xr_label_order_copy_dev(const xr_label_order *order, int64_t first, int64_t count, int64_t *out_dev);
int xr_label_order_destroy(xr_label_order *order);
/* `rows` rows of src_row_bytes each into rows of dst_row_bytes (>= src_row_bytes), device to device: a column block of a wider
 * array (the concatenation of the partitions' data along the last axis) */
int xr_dev_copy_columns(void *dst_dev, int64_t dst_row_bytes, const void *src_dev, int64_t src_row_bytes, int64_t rows);

/* ---- periodic meshes (Ugrid2d.to_periodic, ugrid2d.py:1392-1462; to_nonperiodic, :1464-1572); xr_periodic.hip, DESIGN section
 * 16.  Both make a NEW device mesh and keep, per UGRID dimension, the GATHER index that aligns data of the old mesh with the
 * new one (data_new = data[..., index]).  The input mesh is only read.  XR_ERR_INVALID: a mesh without nodes.
 *
 * xr_periodic_wrap_dev: the right column folded onto the left one.
 *   xmin / xmax   smallest / largest node x (every node counts, used by a face or not)
 *   boundary      |x - xmax| <= 1e-8 + 1e-5 |xmax| is a right node, the same with xmin a left node (np.isclose).  The y of both
 *                 sets are read back and sorted on the host; they must have one length and agree pair by pair within
 *                 |l - r| <= 1e-8 + 1e-5 |r| (np.allclose).  Otherwise *out is NULL, problems[0] = 1 for different lengths,
 *                 problems[1] = pairs apart, and the call still returns XR_OK: the caller words the exception.
 *   nodes         in a working copy every right node has x = xmin; rows of it that compare equal as doubles are one node (the
 *                 key table of xr_merge_meshes_dev).  The first occurrence is kept, kept nodes keep their order and their
 *                 ORIGINAL coordinates, bit for bit: a right node that comes before its left twin keeps x = xmax.
 *   faces         every real slot through the old -> new node map; a fill slot stays -1.
 * Read-backs: the bounds, the two boundary counts, the boundary y, the number of kept nodes.
 *
 * xr_periodic_unwrap_dev: the seam cut open again.  half = 0.5 (xright - xleft) of the node bounds; slot (f, k) is periodic when
 * (max x over the real slots of f) - x > half; the distinct nodes of periodic slots, ascending, are appended as (xmax, y) and
 * the periodic slots name the copies.  Old nodes keep their ids and coordinates.  Read-backs: the bounds, the number of new nodes.
 *
 * xr_periodic_edges_dev: the edge index, for the DERIVED edges of both meshes (their xr_topology, both manifold).  After a wrap
 * index[e] is the lowest old edge whose node pair, through the node map, is new edge e; after an unwrap the old edge of the pair
 * (map(a), map(b)) of new edge e.  *misses: new edges without an old one (the index is then not handed out).  One read-back.
 *
 * xr_periodic_info: n_index[3], the length of the node / edge / face index (edge: -1 before xr_periodic_edges_dev).
 * xr_periodic_index_copy_dev: facet 0 nodes, 1 edges, 2 faces (0 .. n_face - 1) -> int64 in device memory.
 * xr_periodic_node_inverse_copy_dev (after a wrap only): the new id of every old node, int64[n_node of the old mesh]. */
typedef struct xr_periodic xr_periodic;
int xr_periodic_wrap_dev(xr_mesh *mesh, xr_periodic **out, int64_t *problems);
int xr_periodic_unwrap_dev(xr_mesh *mesh, double xmax, xr_periodic **out);
int xr_periodic_edges_dev(xr_periodic *periodic, const xr_topology *old_topology, const xr_topology *new_topology, int64_t *misses);
int xr_periodic_info(const xr_periodic *periodic, int64_t *n_index);
int xr_periodic_take_mesh(xr_periodic *periodic, xr_mesh **mesh);
int xr_periodic_index_copy_dev(const xr_periodic *periodic, int facet, int64_t *out_dev);
int xr_periodic_node_inverse_copy_dev(const xr_periodic *periodic, int64_t *out_dev);
int xr_periodic_destroy(xr_periodic *periodic);

/* ---- editing networks (Ugrid1d.topology_subset, ugrid1d.py:603-663; sel / clip_box :574-601, :665-672; remove_self_loops
 * :714-738; merge_partitions, partitioning.py:81-116, :137-148; refine_by_vertices, ugrid1d.py:770-876); xr_netedit.hip, DESIGN
 * section 18.  A network is two arrays of the caller in DEVICE memory, node_xy float64[n_node, 2] and edges int64[n_edge, 2];
 * every pointer argument below is device memory except the per-partition arrays of xr_network_merge_dev, which are host arrays
 * (of device pointers and of sizes).  The inputs are only read.  Ids are int32 inside the library: XR_ERR_LIMIT when a count
 * leaves that range.  Nothing is read through an id before it has been compared with its range; an edge that names a node
 * outside [0, n_node) is never followed and fails the call with XR_ERR_INVALID.  Every call makes an xr_netedit handle that
 * owns its results in HBM; xr_netedit_info / xr_netedit_copy_dev read them.
 *
 * xr_network_subset_dev: the network of the edges edge_index_dev int64[n] (ids unique, any order):
 *   - its edges are edges[index] in the order given, with their orientation;
 *   - its nodes are the distinct end nodes of those edges in ascending old id, renumbered by their dense rank (np.unique, then
 *     connectivity.renumber); the coordinates are copied bit for bit.  XR_NET_NODE_INDEX: that ascending node index.
 * problems[0]: ids outside [0, n_edge) (negative ones included: nothing wraps), problems[1]: ids that repeat an earlier one.
 * If either is non-zero *out is NULL and the call still returns XR_OK: the caller words the exception.  *is_identity = 1 (and
 * *out NULL) when the selection is every edge in order; with is_identity == NULL that selection is cut like any other (its unused
 * nodes go: remove_self_loops).  n == 0 gives the empty network without a launch.  XR_ERR_INVALID:
 * n > n_edge.  One synchronising read-back (the number of kept nodes and the four status words in one copy).
 *
 * Ascending edge indexes (xr_index: flags -> exclusive scan -> compaction, one read-back each, its length):
 *   xr_network_edges_of_nodes_dev  the edges with at least one end among node_index_dev[n] (np.unique of
 *                                  node_edge_connectivity[node_index].data); ids out of range select nothing
 *   xr_network_box_edges_dev       the edges whose midpoint 0.5 * (a + b), per coordinate, satisfies xmin <= x < xmax and
 *                                  ymin <= y < ymax: exactly these four comparisons, so a NaN midpoint is outside
 *   xr_network_nonloop_edges_dev   the edges with a != b (compared as ids, in range or not)
 *
 * xr_network_merge_dev: the networks 0 .. n_part - 1 joined into one.
 *   nodes  the rule of xr_merge_meshes_dev: the partitions' node_xy concatenated in the order given; two nodes are one when both
 *          coordinates compare equal as doubles (-0.0 == 0.0; a row holding NaN equals nothing, not even itself); the first
 *          occurrence is kept, bit for bit, and kept nodes keep their concatenation order.
 *   edges  the partitions' GIVEN edges mapped to merged node ids; two edges are one when their (lower, higher) pairs are equal;
 *          the first occurrence is kept with its own orientation, kept edges keep their concatenation order.
 * XR_NET_NODE_INVERSE: the merged id of every concatenated node; xr_netedit_part_*: per partition the ascending LOCAL ids of its
 * kept nodes (facet 0) and kept edges (facet 1).  One synchronising read-back: both scans at the 2 (n_part + 1) partition
 * boundaries and the count of bad edges in one copy.
 *
 * xr_network_refine_dev: every vertex float64[n_vertex, 2] becomes a node of the edge it lies on.
 *   locate  vertex p lies on edge (a, b) when its distance to the closed segment is <= tolerance (>= 0): with u = b - a and
 *           v = p - a, the distance is |v| when u.v <= 0 (a zero-length edge is its point), |p - b| when u.v >= u.u, else
 *           |u x v| / |u| -- the projection clamped to the segment, in uncontracted double arithmetic.  Among several such edges
 *           the LOWEST edge id wins (atomicMin, read in the next launch).  A NaN coordinate is on no edge.  The search is not
 *           all-pairs: the vertices are binned in the cell grid of xr_nn and every edge visits the cells its tolerance-inflated
 *           segment passes.  If some vertex is on no edge, *n_off_edge is their number, the handle holds ONLY the mask
 *           (XR_NET_OFF_EDGE, uint8[n_vertex]) and the call returns XR_OK: the caller words the exception.
 *   drop    a vertex is kept iff the first row of [nodes; vertices] with its coordinates (the key table's equality, as above) is a
 *           vertex: vertices that equal a node are dropped, vertices that equal one another are all kept.
 *   order   kept vertices by edge, then by sqrt(dx * dx + dy * dy) from the edge's FIRST node, then by their position among the
 *           kept vertices (np.lexsort((distance, edge_index)), stable).
 *   emit    node_xy = [nodes; kept vertices in the order given], copied bit for bit (never projected onto the edge); old edge e
 *           becomes 1 + count[e] consecutive edges first -> v1 -> v2 .. -> last.  XR_NET_NODE_INDEX: int64[kept] the new ids in
 *           that order; XR_NET_PARENT_EDGE: int64[n_edge of the result] the old edge of every new edge.
 * Read-backs: the extent of the vertices (the cell grid), the count of vertices on no edge, the numbers of kept vertices and of
 * long rows in one copy;  without vertices only the last, and the count of edges with a node out of range.
 *
 * xr_netedit_info: sizes[7] = n_node, n_edge of the result (-1, -1 without one), the lengths of XR_NET_NODE_INDEX,
 * XR_NET_PARENT_EDGE, XR_NET_NODE_INVERSE, the number of partitions, the length of XR_NET_OFF_EDGE.
 * xr_netedit_copy_dev: `what` into the caller's device array: float64[n_node, 2], int64[n_edge, 2], int64[..] or the uint8 mask. */
typedef struct xr_netedit xr_netedit;
enum { XR_NET_NODE_XY = 0, XR_NET_EDGES = 1, XR_NET_NODE_INDEX = 2, XR_NET_PARENT_EDGE = 3, XR_NET_NODE_INVERSE = 4, XR_NET_OFF_EDGE = 5 };
int xr_network_subset_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, const int64_t *edge_index_dev,
                          int64_t n, xr_netedit **out, int *is_identity, int64_t *problems);
int xr_network_edges_of_nodes_dev(const int64_t *edges_dev, int64_t n_edge, int64_t n_node, const int64_t *node_index_dev, int64_t n,
                                  xr_index **out);
int xr_network_box_edges_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, double xmin, double ymin,
                             double xmax, double ymax, xr_index **out);
int xr_network_nonloop_edges_dev(const int64_t *edges_dev, int64_t n_edge, xr_index **out);
int xr_network_merge_dev(const double *const *node_xy_dev, const int64_t *n_node, const int64_t *const *edges_dev, const int64_t *n_edge,
                         int64_t n_part, xr_netedit **out);
int xr_network_refine_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, const double *vertices_dev,
                          int64_t n_vertex, double tolerance, xr_netedit **out, int64_t *n_off_edge);
int xr_netedit_info(const xr_netedit *net, int64_t *sizes);
int xr_netedit_copy_dev(const xr_netedit *net, int what, void *out_dev);
int xr_netedit_part_info(const xr_netedit *net, int facet, int64_t part, int64_t *n);
int xr_netedit_part_copy_dev(const xr_netedit *net, int facet, int64_t part, int64_t *out_dev);
int xr_netedit_destroy(xr_netedit *net);

/* ---- snapping points (xugrid.snap_nodes, xugrid/ugrid/snapping.py:46-143; snap_to_nodes, :146-219); xr_snap.hip, DESIGN section
 * 19.  Every pointer argument is device memory and the inputs are only read.  Coordinates come as two pointers and one stride in
 * elements: stride 1 for separate x and y arrays, (xy, xy + 1, 2) for an interleaved float64[n, 2] array.  "Within the distance"
 * is dx * dx + dy * dy <= max_distance * max_distance in uncontracted float64, INCLUSIVE (the test of the KD-tree's
 * sparse_distance_matrix), so max_distance = 0 still pairs coincident points.  A NaN or infinite coordinate is XR_ERR_INVALID
 * ("data must be finite", as cKDTree raises); a negative or NaN max_distance is XR_ERR_INVALID.
 *
 * xr_snap_nodes_dev: nodes within the distance of each other are merged (snapping.py:86-143).
 *   adjacency  every point's neighbours within the distance, itself excluded, as CSR, with the ROUNDED square root of each squared
 *              distance (what the reference's distance matrix holds).  More than 2^31 - 1 entries is XR_ERR_INVALID.
 *   targets    point i is a target iff no lower-numbered target lies within the distance (the greedy loop of :66-81 taken as what
 *              it computes: the lexicographically first maximal independent set).  Decided in rounds: undecided -> snapped when a
 *              lower-numbered neighbour is a target, -> target when every lower-numbered neighbour is snapped; XR_SNAP_SWEEPS
 *              bounded passes over a point's row per launch; the host reads one pair of status words every few launches.
 *   assign     a point that is not a target goes to the target among its neighbours with the smallest stored distance, the lowest
 *              id on equal distances (:77: overwritten only when strictly closer, targets met in ascending order).
 *   result     np.unique(visited, return_inverse=True) of :140: XR_SNAP_INDEX the kept points ascending, XR_SNAP_INVERSE the rank
 *              of the kept point every point went to, the kept coordinates copied bit for bit.
 * xr_snap_info: n_kept; n_pair, the number of adjacency entries -- 0 means nothing lies within the distance (the reference then
 * returns None and copies), the handle holds no arrays and xr_snap_copy_dev / xr_snap_relabel_dev are XR_ERR_INVALID; rounds, the
 * number of the last launch that decided a point.  n = 0 gives n_pair = 0 without a launch.
 * xr_snap_copy_dev: XR_SNAP_INVERSE int64[n], XR_SNAP_INDEX int64[n_kept], XR_SNAP_XY float64[n_kept, 2], XR_SNAP_X / XR_SNAP_Y
 * float64[n_kept].  xr_snap_relabel_dev: out[k] = inverse[ids[k]] for int64 ids[count] (a connectivity); an id outside [0, n) is
 * XR_ERR_INVALID, checked before anything is read through it.
 *
 * xr_nn_snap_dev: points move onto the nearest point of an xr_nn index within the distance (snapping.py:146-219); to_index NULL
 * stands for an empty set.  Per point: the indexed points within the distance are counted; with at least one, the output
 * coordinates are those of the one with the smallest squared distance, the LOWEST id on equal squares (the reference's choice
 * between distinct equidistant points follows its tree and is arbitrary), and index_out_dev (optional, int64[n]) is its id; with
 * none the point is copied and the id is -1.  *n_tied: points with more than one indexed point within the distance (the
 * reference raises for them without a tiebreaker; with "nearest" it takes what is computed here).  The indexed points are
 * checked for NaN / infinity on every call. */
typedef struct xr_snap xr_snap;
#define XR_SNAP_SWEEPS 4
enum { XR_SNAP_INVERSE = 0, XR_SNAP_INDEX = 1, XR_SNAP_XY = 2, XR_SNAP_X = 3, XR_SNAP_Y = 4 };
int xr_snap_nodes_dev(const double *x_dev, const double *y_dev, int64_t stride, int64_t n, double max_distance, xr_snap **out);
int xr_snap_info(const xr_snap *snap, int64_t *n_kept, int64_t *n_pair, int64_t *rounds);
int xr_snap_copy_dev(const xr_snap *snap, int what, void *out_dev);
int xr_snap_relabel_dev(const xr_snap *snap, const int64_t *ids_dev, int64_t count, int64_t *out_dev);
int xr_snap_destroy(xr_snap *snap);
int xr_nn_snap_dev(const xr_nn *to_index, const double *x_dev, const double *y_dev, int64_t stride, int64_t n, double max_distance,
                   double *x_out_dev, double *y_out_dev, int64_t out_stride, int64_t *index_out_dev, int64_t *n_tied);

/* ---- snapping lines to mesh edges (xugrid.create_snap_to_grid_dataframe and snap_to_grid, xugrid/ugrid/snapping.py:255-552);
 * xr_snapgrid.hip, DESIGN section 21.  Every pointer argument is device memory and the inputs are only read.
 *
 * xr_snapgrid_create_dev: coords_dev float64[n_vertex, 2] and line_offsets_dev int64[n_line + 1] (start at 0, end at n_vertex,
 * never decrease: checked on the device, XR_ERR_INVALID otherwise) are the vertices of n_line lines; `topology` is the
 * xr_topology of `mesh` (manifold), `node_index` the xr_nn over the mesh's nodes.
 *   snap      every vertex moves onto the nearest node within max_snap_distance (xr_nn_snap_dev, lowest id among equidistant ones)
 *   segments  segment i joins vertex i to the next vertex of its line, the last vertex of a line to itself (no piece)
 *   pieces    the entries of xr_edge_length_csr_dev, their end points recomputed with the arithmetic of xr_edge_pieces
 *   rows      snap_to_edges (:289-325) per piece: widened by tolerance * max(|Ux|, |Uy|) along sign(U), strict left_of, exterior
 *             edges skipped, a face's edges in ascending id; one row per (piece, edge) that passes
 *   order     rows by segment, then face, then edge (within a segment the reference's order is that of its tree traversal)
 *   reduce    (reduce != 0) per edge the row of greatest length, the first in row order among equal ones
 * A NaN or infinite coordinate is XR_ERR_INVALID ("data must be finite"); n_vertex, the number of pieces or of rows >= 2^30 is
 * XR_ERR_LIMIT.
 * xr_snapgrid_copy_dev: the frame's columns XR_SNAPGRID_LINE / _EDGE int64[n_row], _X0 / _Y0 / _X1 / _Y1 / _LENGTH float64[n_row]
 * (the un-widened piece and its SQUARED length, :491); of a reduced handle also XR_SNAPGRID_LINE_INDEX float64[n_edge] (the
 * winning line, NaN for none), XR_SNAPGRID_EDGES int64[n_snapped] (the edges with a line, ascending) and XR_SNAPGRID_EDGE_LINES
 * int64[n_snapped] (their lines).  xr_snapgrid_values_dev: out_dev float64[K, n_edge] = values_dev[K, n_line] of every edge's
 * winning line, NaN for none. */
typedef struct xr_snapgrid xr_snapgrid;
enum {
    XR_SNAPGRID_LINE = 0, XR_SNAPGRID_EDGE = 1, XR_SNAPGRID_X0 = 2, XR_SNAPGRID_Y0 = 3, XR_SNAPGRID_X1 = 4, XR_SNAPGRID_Y1 = 5,
    XR_SNAPGRID_LENGTH = 6, XR_SNAPGRID_LINE_INDEX = 7, XR_SNAPGRID_EDGES = 8, XR_SNAPGRID_EDGE_LINES = 9
};
int xr_snapgrid_create_dev(xr_mesh *mesh, const xr_topology *topology, const xr_nn *node_index, const double *coords_dev,
                           int64_t n_vertex, const int64_t *line_offsets_dev, int64_t n_line, double max_snap_distance,
                           double tolerance, int reduce, xr_snapgrid **out);
int xr_snapgrid_info(const xr_snapgrid *snapgrid, int64_t *n_piece, int64_t *n_row, int64_t *n_snapped);
int xr_snapgrid_copy_dev(const xr_snapgrid *snapgrid, int what, void *out_dev);
int xr_snapgrid_values_dev(const xr_snapgrid *snapgrid, const double *values_dev, int64_t K, double *out_dev);
int xr_snapgrid_destroy(xr_snapgrid *snapgrid);

/* ---- meshes from cell geometry: sorted unique rows, CF cell bounds, lattices, rings and lines; xr_geometry.hip, DESIGN
 * section 24.  Every pointer argument whose name ends in _dev is device memory; inputs are only read.
 *
 * xr_unique_xy_dev: np.unique of xy_dev float64[n, 2] along axis 0 with return_index and return_inverse.  Two rows are one
 * when both coordinates compare == as doubles (-0.0 == 0.0); the kept bits are those of the first such row in input order; the
 * unique rows ascend by x, then by y, with < on doubles.  index[u] is the input position of the kept row, inverse[i] the
 * sorted rank of row i's key.  Rows with a NaN or an infinity are counted: with any, the handle holds the count only and the
 * caller words the error.  The key table of xr_merge_meshes_dev finds the first occurrences; they are sorted by a stable LSD
 * radix sort, one byte per pass, over the order-preserving images of the coordinates; passes whose byte is equal in all
 * keys are skipped.  XR_ERR_LIMIT: n >= 2^30.
 * xr_unique_xy_info: sizes[5] = n, n_unique, rows with a non-finite coordinate, sort passes run, sort passes skipped.
 * xr_unique_xy_copy_dev: what 0 the unique rows float64[n_unique, 2], 1 index int64[n_unique], 2 inverse int64[n]. */
typedef struct xr_unique_xy xr_unique_xy;
int xr_unique_xy_dev(const double *xy_dev, int64_t n, xr_unique_xy **out);
int xr_unique_xy_info(const xr_unique_xy *unique, int64_t *sizes);
int xr_unique_xy_copy_dev(const xr_unique_xy *unique, int what, void *out_dev);
int xr_unique_xy_destroy(xr_unique_xy *unique);

/* xr_mesh_from_bounds_dev: conversion.bounds2d_to_topology2d (conversion.py:297-354) on x_dev / y_dev float64[n_cell, 4], the
 * four corners of every cell in any order.  Per cell: the corners sorted by x, then y; n_unique = corners that differ from
 * their cyclic predecessor; valid = n_unique >= 3 and quad_area > 0 (the fan from the first sorted corner, |.| per triangle).
 * index_out_dev uint8[n_cell] (bytes 0 / 1) = valid and all eight coordinates finite.  The cells of the index, in order, become the faces:
 * their corners ordered by atan2 about the mean corner (a corner at its sorted predecessor's angle goes last, ties keep the
 * sorted order), numbered by the rule of xr_unique_xy_dev; the last slot of a face with n_unique == 3 is -1.
 * counts[4] = faces, cells that are not valid (NaN cells included: the reference's warning), sort passes run / skipped.
 * The caller destroys the mesh with xr_mesh_destroy.  XR_ERR_LIMIT: n_cell >= 2^28 (the corner rows reach the limit of xr_unique_xy_dev). */
int xr_mesh_from_bounds_dev(const double *x_dev, const double *y_dev, int64_t n_cell, xr_mesh **out, uint8_t *index_out_dev, int64_t *counts);

/* xr_interval_breaks_dev: conversion.infer_interval_breaks (conversion.py:171-199) of coord_dev float64[rows, cols] along axis
 * 0 (out_dev float64[rows + 1, cols]) or 1 (float64[rows, cols + 1]): first - half the first step, every element but the last
 * + half its step, last + half the last step; a line of one element gives it twice.  problems[2] = 1 when some neighbour pair
 * along the axis does not ascend / does not descend (a NaN does neither), else 0: the coordinate is monotonic when either is 0.
 * xr_mesh_from_intervals_dev: the lattice of x_dev / y_dev float64[ny + 1, nx + 1] node coordinates as a mesh: node id = row *
 * (nx + 1) + column, face id = row * nx + column, quads (lower left, lower right, upper right, upper left) where left and
 * right swap when x[0, 1] < x[0, 0], lower and upper when y[1, 0] < y[0, 0]. */
int xr_interval_breaks_dev(const double *coord_dev, int64_t rows, int64_t cols, int axis, double *out_dev, int64_t *problems);
int xr_mesh_from_intervals_dev(const double *x_dev, const double *y_dev, int64_t ny, int64_t nx, xr_mesh **out);

/* xr_mesh_from_rings_dev: conversion.polygons_to_faces (conversion.py:82-117) on closed rings: coords_dev float64[n_vertex, 2],
 * ring_off_dev int64[n_ring + 1]; poly_off_dev int64[n_poly + 1] or NULL (n_poly 0).  Every ring loses its closing vertex, the
 * nodes are the sorted unique vertices (xr_unique_xy_dev), face r is ring r's vertices in order, n_max_node the longest ring,
 * -1 behind shorter ones; without rings an empty mesh of width 3.  problems[5] = rings of fewer than four vertices, rings
 * whose last vertex is not == the first, offsets that do not ascend from 0 to n_vertex, polygons that do not hold exactly
 * one ring (holes), vertices with a non-finite coordinate; with any, *out is NULL and the caller words the error.
 * xr_mesh_ring_offsets_dev / xr_mesh_ring_coords_dev: the way back (conversion.faces_to_polygons): ring f is face f's nodes in
 * order and its first node again (a face without a node: an empty ring).  The first writes ring_off_out_dev int64[n_face + 1], poly_off_out_dev int64[n_face + 1] = 0 .. n_face
 * (one ring per polygon; NULL: not wanted) and *n_vertex, the second
 * coords_out_dev float64[n_vertex, 2] for those offsets. */
int xr_mesh_from_rings_dev(const double *coords_dev, int64_t n_vertex, const int64_t *ring_off_dev, int64_t n_ring, const int64_t *poly_off_dev,
                           int64_t n_poly, xr_mesh **out, int64_t *problems);
int xr_mesh_ring_offsets_dev(const xr_mesh *mesh, int64_t *ring_off_out_dev, int64_t *poly_off_out_dev, int64_t *n_vertex);
int xr_mesh_ring_coords_dev(const xr_mesh *mesh, const int64_t *ring_off_dev, int64_t n_vertex, double *coords_out_dev);

/* xr_lines_to_network_dev: conversion.linestrings_to_edges (conversion.py:70-79): coords_dev float64[n_vertex, 2],
 * line_off_dev int64[n_line + 1].  The nodes are the sorted unique vertices (*nodes_out: rows 0 of xr_unique_xy_copy_dev), an
 * edge joins every two consecutive vertices of one line, in order (a repeated vertex gives a self loop, a line of one vertex
 * no edge): edges_out_dev int64[max(n_vertex - 1, 0), 2], of which the first counts[0] rows are written.  counts[1] = offsets
 * that do not ascend from 0 to n_vertex (then *nodes_out is NULL), counts[2] = vertices with a non-finite coordinate. */
int xr_lines_to_network_dev(const double *coords_dev, int64_t n_vertex, const int64_t *line_off_dev, int64_t n_line, xr_unique_xy **nodes_out,
                            int64_t *edges_out_dev, int64_t *counts);

/* ---- raw HBM helpers for hosts that do not bring their own allocator -------------------- */
int xr_dev_alloc(int64_t bytes, void **ptr_out);
int xr_dev_free(void *ptr);
int xr_dev_upload(void *dst_dev, const void *src_host, int64_t bytes);
int xr_dev_download(void *dst_host, const void *src_dev, int64_t bytes);
int xr_dev_sync(void);

/* ---- in-library kernel timing (HIP events on the engine stream) -------------------------- */
/* When enabled every kernel launch is bracketed by hipEvents on the engine stream; durations
 * are accumulated per kernel name. */
int xr_prof_enable(int on);
int xr_prof_reset(void);
/* Number of distinct kernels recorded since the last reset. */
int xr_prof_count(int *count);
/* i-th record: name (copied, NUL-terminated, at most name_cap bytes), launches, total ms. */
int xr_prof_get(int i, char *name, int name_cap, int64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* XUGRID_AMD_H */
