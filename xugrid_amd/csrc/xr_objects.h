// xr_objects.h -- the device-resident handle types behind the C ABI that more than one unit reads.
#pragma once
#include <memory>
#include <vector>

#include "xr_geom.h"
#include "xr_internal.h"

// Device-resident face topology + derived per-face data.  A mesh IS its raw upload; everything else hangs off it in stages, one
// small struct per lifetime (layout: xr_geom.h).  Every stage lists its buffers once, in bytes() and release():
//   raw      what the caller uploaded (node_xy, faces_raw) + where the mesh came from
//   stats    the eight statistics of the faces and their way to the host (MeshStatsBox)
//   prep     per-face arrays in the CALLER's face order (fxy, len, bbox, area)
//   qo       the same arrays permuted into a spatially coherent order (Morton order of coarse
//            cells) -- used when the mesh is the QUERY (regridding target) side
//   index    the same arrays permuted into grid-cell order + cell_start -- used when the mesh is
//            the TREE (regridding source) side
//   centroids, bary   caches other units keep on the mesh
namespace xr {
struct StatsTail; // the hand-off words a statistics kernel gets (xr_mesh.h)

struct MeshRaw {
    int64_t n_node = 0, n_face = 0;
    int m = 0; // n_max_node_per_face
    DevBuf<double> node_xy;    // [n_node*2]
    DevBuf<int32_t> faces_raw; // [n_face*m] caller's vertex order, fill -> -1
    // kept when this mesh is the fan triangulation of another (xr_mesh_triangulate): the source face of every triangle
    DevBuf<int32_t> tri_face; // [n_face]
    bool is_triangulation = false;
    // kept when this mesh was cut out of another (xr_mesh_subset_dev, xr_subset.hip): the source node of every node, ascending
    DevBuf<int32_t> sub_node; // [n_node]
    bool is_subset = false;
    size_t bytes() const { return node_xy.bytes() + faces_raw.bytes() + tri_face.bytes() + sub_node.bytes(); }
};

// The statistics of a mesh and their hand-off.  The reduction (a kernel's last block, or k_reduce_stats behind it) deposits them
// in the device copy and in pinned host memory and stores the launch's sequence number behind them; the host polls that word,
// or waits on the event recorded behind k_reduce_stats, so kernels queued later (the other mesh's prepare) keep the GPU busy
// meanwhile.  One launch goes begin() -> kernel -> enqueued(); read() brings the values to h[] (xr_mesh_front.hip).
struct MeshStatsBox {
    DevBuf<double> dev;            // [8] device copy
    double h[stat::N_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0}; // host values, indexed by stat::Slot (xr_geom.h)
    double *host = nullptr;        // [9] pinned: the statistics + the sequence word the publishing block stores last
    hipEvent_t event = nullptr;
    DevBuf<unsigned> done;         // blocks that have delivered their partial (zero at rest; stats_tail, xr_mesh_front.hip)
    double seq = 0.0;              // sequence number of the last statistics launch (what host[8] must show)
    bool launched = false;         // a statistics kernel has run for the mesh as it is (the mesh is "prepared")
    bool event_pending = false;    // a reduction kernel + event were enqueued for the last launch (fallback of the poll)
    bool polled = false;           // the statistics of the last launch arrive through the sequence word (no event recorded)
    bool valid = false;            // h[] holds the last launch's values
    bool sampled = false; // h[stat::SUM_EXTENT..MAX_DIAGONAL] come from a sample of the faces: enough to size a grid, NOT for the default tolerance
    ~MeshStatsBox() { // (not copyable: DevBuf)
        if (host) (void)hipHostFree(host);
        if (event) (void)hipEventDestroy(event);
    }
    size_t bytes() const { return dev.bytes(); }
    void release() { // (`sampled` describes the last launch and is overwritten by the next; the counters stay, zero at rest)
        launched = valid = false;
        dev.release();
    }
    StatsTail begin(double *partials, int64_t nb); // next sequence number; the pinned page and the counters on first use
    void enqueued(const double *partials, int64_t nb, const StatsTail &tail, bool on_side); // behind the kernel: k_reduce_stats where its last block does not reduce
    void read(); // wait for the last launch's values
};

struct MeshPrepared { // caller's face order
    bool has_attrs = false; // len / bbox / fxy filled (prepared as a query)
    bool fxy_valid = false;
    bool area_valid = false;
    DevBuf<double> fxy;      // [n_face*m*2] CCW-normalised vertex coordinates per face (only if fxy_valid:
                             // needed when the mesh is a query kept in the caller's numbering)
    DevBuf<int32_t> fxy_off; // [n_face+1] only for ragged() meshes: fxy is flat, face f starts at vertex fxy_off[f]
    DevBuf<uint8_t> len;     // [n_face]
    DevBuf<double> bbox;     // [n_face*4] xmin,xmax,ymin,ymax; ragged() meshes only (dense ones: query_face_box, xr_geom.h)
    DevBuf<double> area;     // [n_face]   connectivity.area on the caller's vertex order (mesh_area, on demand)
    size_t bytes() const { return fxy.bytes() + fxy_off.bytes() + len.bytes() + bbox.bytes() + area.bytes(); }
    void release() {
        has_attrs = fxy_valid = area_valid = false;
        fxy.release(), fxy_off.release(), len.release(), bbox.release(), area.release();
    }
};

// If the caller's face numbering is already spatially coherent (mean distance between consecutive faces <= a few face
// extents) the caller's order IS the query order: no permutation, no copies (identity); xr_mesh::qo_*() hide the difference.
struct MeshQueryOrder {
    bool ready = false;
    bool identity = false;
    DevBuf<int32_t> perm; // [n_face] position -> caller's face id
    DevBuf<double> fxy;   // [n_face*m*2], ragged(): [sum len * 2]
    DevBuf<int32_t> off;  // [n_face+1] ragged() only
    DevBuf<uint8_t> len;  // [n_face]
    DevBuf<double> bbox;  // [n_face*4] ragged() only
    size_t bytes() const { return perm.bytes() + fxy.bytes() + off.bytes() + len.bytes() + bbox.bytes(); }
    void release() {
        ready = identity = false;
        perm.release(), fxy.release(), off.release(), len.release(), bbox.release();
    }
};

struct MeshIndex { // tree index (records in grid-cell order)
    // records of padding behind rec_bb: the record walks (k_search, k_edge_walk) issue several unclamped loads at once, and the
    // ones beyond a run's end -- masked afterwards -- must stay inside the array
    static constexpr int REC_BB_PAD = 8;
    bool ready = false;
    GridParams grid{};
    DevBuf<int32_t> cell_start; // [n_cells+1]
    DevBuf<float> rec_bb;       // [(n_face + REC_BB_PAD)*4] conservative f32 bbox relative to the grid origin
    DevBuf<int32_t> rec_face;   // [n_face]   record -> caller's face id
    DevBuf<double> rec_fxy;     // [n_face*m*2], ragged(): [sum len * 2]
    DevBuf<int32_t> rec_off;    // [n_face+1] ragged() only
    DevBuf<uint8_t> rec_len;    // [n_face]
    size_t bytes() const {
        return cell_start.bytes() + rec_bb.bytes() + rec_face.bytes() + rec_fxy.bytes() + rec_off.bytes() + rec_len.bytes();
    }
    void release() {
        ready = false;
        cell_start.release(), rec_bb.release(), rec_face.release(), rec_fxy.release(), rec_off.release(), rec_len.release();
    }
};

// connectivity.centroids, on demand (mesh_centroids_shared); kept like the reference's cached Ugrid2d.centroids until the mesh
// is invalidated
struct MeshCentroids {
    std::shared_ptr<DevBuf<double>> dev; // [n_face*2]
    hipEvent_t event = nullptr;   // recorded behind the kernel that filled dev, on `stream`: a user on another stream
    hipStream_t stream = nullptr; // (the handles' kernels run on the side stream) waits for it
    MeshCentroids() = default;
    MeshCentroids(const MeshCentroids &) = delete;
    MeshCentroids &operator=(const MeshCentroids &) = delete;
    ~MeshCentroids() {
        if (event) (void)hipEventDestroy(event);
    }
    size_t bytes() const { return dev ? dev->bytes() : 0; }
    void release() { dev.reset(); } // (a handle that shares them keeps them)
};

// Kept by the barycentric construction when this mesh is a Voronoi tessellation (xr_locate.hip:barycentric_csr, its only
// reader): the vertex -> face table with the interpolation map behind it, and the flags of the cells that hold a substitute
// vertex -- a second interpolator on a cached tessellation uploads and recomputes nothing (its first kernel then runs BESIDE the
// source-side locate pass instead of behind a copy).  Describes the raw mesh: xr_mesh_invalidate keeps it, and
// xr_mesh_device_bytes has never counted it.
struct MeshBaryCache {
    std::vector<int64_t> ids_host; // what was uploaded (tail of the vertex table, then the map)
    DevBuf<int64_t> ids;           // [n_node + 2 n_extra + 1]
    int64_t n_identity = -1, n_extra = -1;
    DevBuf<uint8_t> cell_flag;     // [n_face], valid for n_extra
    bool flag_valid = false;
};
} // namespace xr

struct xr_mesh : xr::MeshRaw {
    xr::MeshStatsBox stats;
    xr::MeshPrepared prep;
    xr::MeshQueryOrder qo;
    xr::MeshIndex index;
    xr::MeshCentroids centroids;
    xr::MeshBaryCache bary;
    int64_t last_candidates = 0;

    // vertex blocks flat + offsets instead of dense [n_face][m] (xr_geom.h)
    bool ragged() const { return m > xr::DENSE_MAX_NODES; }
    const int32_t *caller_off() const { return ragged() ? prep.fxy_off.get() : nullptr; }
    const int32_t *record_off() const { return ragged() ? index.rec_off.get() : nullptr; }
    const int32_t *qo_off() const { return !ragged() ? nullptr : qo.identity ? prep.fxy_off.get() : qo.off.get(); }
    const double *qo_fxy() const { return qo.identity ? prep.fxy.get() : qo.fxy.get(); }
    const uint8_t *qo_len() const { return qo.identity ? prep.len.get() : qo.len.get(); }
    const double *qo_bbox() const { return qo.identity ? prep.bbox.get() : qo.bbox.get(); } // nullptr for dense meshes
    const int32_t *qo_perm() const { return qo.identity ? nullptr : qo.perm.get(); } // nullptr = identity
};

// Rows with more entries than this are not walked by one thread but reduced cooperatively in the apply kernels:
// by one wave each up to XR_APPLY_WAVE_ROW entries, by a whole block beyond.  (Cooperative = fixed butterfly
// order: deterministic, ~1e-15 from the sequential order of the reference loop.)
static constexpr int XR_APPLY_LONG_ROW = 32;
static constexpr int XR_APPLY_WAVE_ROW = 2048;

// Device-resident MatrixCSR (xugrid/core/sparse.py:81-137), int32 structure + float64 data.  A matrix IS its three arrays;
// everything else hangs off it in stages, one small struct per lifetime (as xr_mesh above), each listing its buffers once:
//   stored   the order the rows are stored in, when it is not the caller's
//   longs    the list of the long rows (the cooperative kernels of the applies)
//   tiling   row keys waiting for the many-variable apply to regroup the stored rows
//   cols     the renumbering of the columns
//   plan     the apply plan of the many-variable kernels (lazily built cache)
//   tr       the transposed weights of the adjoint apply (lazily built cache)
// Which cache goes stale on which event: xr_csr::rows_regrouped(), xr_csr::keys_changed().
namespace xr {
// Rows may be STORED in a spatially coherent order instead of the caller's: stored row r is the
// caller's row row_order[r] (weights built by xr_overlap: the query mesh's query order).  The
// apply kernels scatter their outputs through it; xr_csr_download un-permutes.
struct CsrStoredOrder {
    DevBuf<int32_t> row_order; // [n]
    bool has_row_order = false;
    bool output_stored = false; // applies write row r of the STORED order to out[k, r] (xr_csr_output_stored_order)
    void release() {
        has_row_order = false;
        row_order.release();
    }
};

// stored rows with more than XR_APPLY_LONG_ROW entries (reduced by one wave or block each in the apply)
struct CsrLongRows {
    DevBuf<int32_t> rows;     // [<= n]
    DevBuf<int32_t> n_dev;    // [1] device-side count (matrices of the fused build: TAIL_WORDS = 4 words, indexed by TailWord --
                              // the count, the gate of an apply enqueued behind the build, n_big, p_regular; xr_overlap_tail.h)
    int64_t max_row_len = -1; // entries of the longest row if the builder reported it (-1: unknown)
    bool any = false;         // the list is not empty: the applies launch the long rows' kernels
    // in front of the kernel that lists the rows: room for `capacity` of them and `words` control words, the count ([0]) zero
    void begin(size_t capacity, int words = 1) {
        rows.alloc(capacity);
        n_dev.alloc((size_t)words);
        XR_HIP(hipMemsetAsync(n_dev.get(), 0, sizeof(int32_t), launch_stream()));
    }
    // behind it: `count` rows were listed (negative: the caller does not know -- read from the device)
    void end(int64_t count = -1) { any = (count >= 0 ? count : (int64_t)read_scalar(n_dev.get())) > 0; }
    void release() {
        any = false;
        max_row_len = -1;
        rows.release(), n_dev.release();
    }
};

// Coarse Morton key per STORED row (tile of ~12 target extents).  Set by xr_overlap when the rows are kept
// in the caller's order, or by xr_csr_set_row_keys; consumed once by the many-variable apply, which regroups
// the stored rows into compact 2-D tiles (xr_csr.hip: ensure_tiled) and then drops the keys.
struct CsrTiling {
    DevBuf<int32_t> key;   // [n]
    bool pending = false;
    int64_t key_range = 0; // keys are in [0, key_range)
    void release() {
        pending = false;
        key.release();
    }
};

// Columns renumbered by a spatial key (xr_csr_set_col_keys): stored column j is the caller's column col_of[j].
// The apply gathers the caller's source block into the stored order first unless the caller says it already is.
struct CsrColumns {
    DevBuf<int32_t> col_of; // [m]
    bool permuted = false;
    bool source_permuted = false;
    void release() {
        permuted = false;
        col_of.release();
    }
};

// "apply plan" for many source variables (built lazily, xr_apply_plan.hip: ensure_plan): per block of 256 stored
// rows the sorted list of DISTINCT column ids and, per entry, its 16-bit position in that list
struct CsrPlan {
    bool ready = false;
    bool merged = false;           // the lists are per GROUP of row blocks (k_plan_build<PLAN_GROUP>), not per block
    DevBuf<int32_t> unplanned;     // blocks the plan could not take (handled by the direct kernel)
    int n_unplanned = 0;
    int lmax = 0;                  // entries of the largest planned block, rounded up to 256 (LDS stage of the apply)
    DevBuf<int32_t> ucol;          // [n_blocks * PLAN_UMAX]
    DevBuf<int32_t> nuniq;         // [n_blocks], -1 = block not planned (falls back to direct gathers)
    DevBuf<uint16_t> loc;          // [nnz]
    void release() {
        ready = false;
        unplanned.release(), ucol.release(), nuniq.release(), loc.release();
    }
};

// the transposed weights of the adjoint apply (built lazily, xr_adjoint.hip: ensure_transposed), in the ids the applies
// use -- caller's columns, output rows -- with a copy of every weight: per column the entries in ascending (row, storage
// position).  Built in the caller's row ids, no re-layout of the stored matrix touches them; built in stored positions
// (output_stored), the row tiling invalidates them (xr_csr::rows_regrouped) and the next adjoint rebuilds them
struct CsrTransposed {
    bool ready = false;
    bool output_stored = false; // the row ids are stored positions (the matrix delivered in stored order when this was built)
    DevBuf<int32_t> indptr;     // [m+1]
    DevBuf<uint32_t> row;       // [nnz] row id; bit 31: the entry is the last of its row (what XR_SELECT copies)
    DevBuf<double> w;           // [nnz]
    DevBuf<int32_t> long_cols;  // [n_long] columns with more than XR_APPLY_LONG_ROW entries, ascending
    int64_t n_long = 0, max_len = 0;
    void release() {
        ready = output_stored = false;
        indptr.release(), row.release(), w.release(), long_cols.release();
        n_long = max_len = 0;
    }
};
} // namespace xr

struct xr_csr {
    int64_t n = 0, m = 0, nnz = 0;
    xr::DevBuf<int32_t> indptr;    // [n+1]
    xr::DevBuf<int32_t> indices;   // [nnz]
    xr::DevBuf<double> data;       // [nnz]
    xr::CsrStoredOrder stored;
    xr::CsrLongRows longs;
    xr::CsrTiling tiling;
    xr::CsrColumns cols;
    xr::CsrPlan plan;
    xr::CsrTransposed tr;

    // The two events that make a lazily built cache stale.  (A stale cache keeps its buffers until it is rebuilt.)
    // The stored rows were regrouped (ensure_tiled): the plan indexes stored rows; so does a transpose built in stored
    // positions -- one built in the caller's ids is untouched.
    void rows_regrouped() {
        plan.ready = false;
        if (tr.output_stored) tr.ready = false;
    }
    // The tiling keys or the column ids changed (xr_csr_set_row_keys, xr_csr_set_col_keys): the plan is rebuilt; the
    // transpose is left as it is.
    void keys_changed() { plan.ready = false; }
};

// Separable (rectilinear) weights kept as the two per-axis sparse matrices (xugrid/regrid/structured.py:503-601): the
// P = P_y * P_x entries of their outer product are never stored unless somebody asks for the CSR.
struct xr_outer {
    int64_t nty = 0, nsy = 0, ntx = 0, nsx = 0, Py = 0, Px = 0;
    xr::DevBuf<int32_t> ipy, ipx; // [nt + 1]
    xr::DevBuf<int32_t> sy, sx;   // [P] source index per entry (ascending within a row)
    xr::DevBuf<double> wy, wx;    // [P]
    xr::DevBuf<int32_t> tx;       // [Px] x-target owning each x-entry (CSR assembly)
    int64_t max_cy = 0, max_cx = 0;
    xr_csr *csr = nullptr;        // materialised on demand (mode / percentiles, downloads)
    ~xr_outer() { delete csr; }
};

// A symmetric adjacency in HBM (xr_fill.hip: the Laplace fill and the graph operations; xr_netfill.hip: the network graphs and
// the shortest-path nearest).
struct xr_graph {
    int64_t n = 0, nnz = 0;
    xr::DevBuf<int32_t> indptr;  // [n+1]
    xr::DevBuf<int32_t> indices; // [nnz] ascending per row
    xr::DevBuf<double> data;     // [nnz] weights (1.0 when the caller gave none)
    xr::DevBuf<int32_t> labels;  // [n] connected component: the smallest node id of the component
    bool has_data = false;
    int64_t label_rounds = 0; // rounds of k_label_round the labelling took (0: labels given by the caller)
};

namespace xr {
void label_components(xr_graph *g); // labels = the smallest member id of every component (xr_fill.hip)
// a mesh handle with its sizes set and node_xy / faces_raw allocated, for the caller to fill (xr_mesh.hip)
Building<xr_mesh> new_raw_mesh(int64_t n_node, int64_t n_face, int m, OnFailure rule = OnFailure::FreeOnly);
void mesh_prepare_pair(xr_mesh *tree, xr_mesh *query); // the front of a weight build: both preparations, in one launch where it can be
void mesh_prepare(xr_mesh *mesh, bool want_fxy = true, bool stats_on_side = false, bool allow_sampled = false); // stats_on_side: the reduction of the
    // statistics (only the HOST reads them) leaves the main stream: kernels queued behind the prepare pass do not wait for it
const double *mesh_area(xr_mesh *mesh); // connectivity.area in the caller's face order (computed on first use)
void mesh_face_coords(xr_mesh *mesh); // make sure the caller-order vertex blocks exist
void mesh_query_order(xr_mesh *mesh);
void mesh_build_index(xr_mesh *mesh);
void flush_pending_points(); // launch the deferred source-side kernels of pending xr_points handles (xr_locate.hip)
void flush_pending_points_of(const xr_mesh *mesh); // ... if one of them reads `mesh`, before its arrays are released
void mesh_read_stats(xr_mesh *mesh, bool need_exact = false); // need_exact: statistics over ALL faces (sampled ones are redone)
void mesh_centroids_dev(xr_mesh *mesh, double *cxy_dev);    // connectivity.centroids into device memory [n_face*2]
std::shared_ptr<xr::DevBuf<double>> mesh_centroids_shared(xr_mesh *mesh); // ... computed once per mesh, shared with the callers
// locate_points on device-resident points (xr_locate.hip); tolerance < 0: the mesh's default.  The mesh must have faces.  -> the tolerance used
double locate_points_dev(xr_mesh *mesh, const double *pts_dev, int64_t n, double tolerance, int64_t *out_dev);
void mesh_faces_ccw_dev(xr_mesh *mesh, int64_t *faces_dev, bool caller_order = false); // CCW-normalised (or the caller's) connectivity [n_face*m]
} // namespace xr
