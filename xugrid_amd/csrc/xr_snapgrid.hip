// xr_snapgrid.hip -- snapping lines to the edges of a mesh on the device: create_snap_to_grid_dataframe and snap_to_grid
// (xugrid/ugrid/snapping.py:255-552).  DESIGN section 21.
//
// The reference snaps the line vertices to the nodes, cuts every segment into its pieces per face (celltree.intersect_edges),
// and then, piece by piece, asks of every interior edge of the piece's face whether the piece separates the two centroids on
// either side of it (snap_to_edges, :289-325).  Every (piece, edge) that passes is a row of the frame; snap_to_grid keeps, per
// edge, the row whose piece is longest (groupby("edge_index").idxmax(): the first of equal ones).
//
// Here: vertices through xr_nn_snap_dev (xr_snap.hip), pieces through xr_edge_length_csr_dev (xr_edges.hip) and the clip of
// xr_edge_clip.h -- the pieces k_edge_pieces writes, bit for bit --, centroids from the buffer the mesh shares with everybody
// (mesh_centroids_shared), edges from the device topology.  New in this unit:
//   rows     one lane per CSR entry, twice (count, scan, fill): piece, separation test in the reference's operation order (no
//            contraction: the unit is built with -ffp-contract=off like every other), edges in ascending id;
//   order    the CSR is face-major, the frame segment-major: rows are bucketed by segment (histogram from the count pass, scan,
//            scatter through a cursor) and every bucket is sorted by the row's position in the CSR walk -- within one segment that
//            position ascends with (face, edge), so the frame is ordered by (segment, face, edge) whatever order the lanes ran in;
//   reduce   atomicMax of the bits of `length` per edge (non-negative doubles order like their bit patterns), then atomicMin of
//            the frame row among the rows that hold the maximum.  No floating-point accumulation anywhere.
// Segment i joins vertex i to the next vertex of its line; the last vertex of a line is joined to itself (zero length: no
// piece), so segment ids ascend exactly like the reference's compacted ones (lines_as_edges, :232-237).
#include <climits>
#include <cmath>

#include "xr_edge_clip.h"
#include "xr_index.h"
#include "xr_objects.h"
#include "xr_prims.h"
#include "xr_topology.h"

namespace xr {

static constexpr int SG = 256;          // threads per block
static constexpr int SG_SORT_SMALL = 16; // buckets up to this many rows are insertion-sorted by one lane
static constexpr int SG_TOTALS = 64, SG_TOTAL_STRIDE = 16; // the row count is summed into 64 words, a 128-byte line apart

// flag = 1 unless off[0] == 0, off[n_off - 1] == total and off never decreases
__global__ void __launch_bounds__(SG)
k_sg_check_offsets(const int64_t *__restrict__ off, int64_t n_off, int64_t total, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * SG + threadIdx.x;
    bool bad = false;
    if (i < n_off) {
        const int64_t v = off[i];
        bad = (i == 0 && v != 0) || (i == n_off - 1 && v != total) || (i > 0 && v < off[i - 1]);
    }
    wave_flag(bad, flag);
}

// seg[i] = (vertex i, next vertex of its line or vertex i itself), seg_line[i] = the line of vertex i: the last r with
// off[r] <= i (off ascending, off[0] = 0 <= i < off[n_line]; empty lines share an offset and are passed over)
__global__ void __launch_bounds__(SG)
k_sg_segments(const double2 *__restrict__ xy, int64_t n_vertex, const int64_t *__restrict__ off, int64_t n_line,
              double4 *__restrict__ seg, int32_t *__restrict__ seg_line) {
    const int64_t i = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (i >= n_vertex) return;
    int64_t lo = 0, hi = n_line;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const int64_t nxt = i + 1 < off[lo + 1] ? i + 1 : i;
    const double2 a = xy[i], b = xy[nxt];
    seg[i] = make_double4(a.x, a.y, b.x, b.y);
    seg_line[i] = (int32_t)lo;
}

// snapping.py:241-244: whether a lies left of U anchored at p.  Strict.
__device__ __forceinline__ bool left_of(P2 a, P2 p, double ux, double uy) { return ux * (a.y - p.y) > uy * (a.x - p.x); }
// np.sign: 0 for both zeros
__device__ __forceinline__ double sign0(double v) { return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : 0.0; }

// snap_to_edges (:296-306): the piece c -> d widened by tolerance * max(|Ux|, |Uy|) at both ends, along sign(U)
struct Widened {
    P2 p, q;
    double ux, uy;
    bool any; // false: U == 0, the piece is passed over
};
__device__ __forceinline__ Widened widen_piece(P2 c, P2 d, double tolerance) {
    Widened w;
    const double ux = d.x - c.x, uy = d.y - c.y;
    w.any = !(ux == 0.0 && uy == 0.0);
    const double signx = sign0(ux), signy = sign0(uy);
    const double increase = tolerance * fmax(fabs(ux), fabs(uy));
    w.p = P2{c.x - signx * increase, c.y - signy * increase};
    w.q = P2{d.x + signx * increase, d.y + signy * increase};
    w.ux = w.q.x - w.p.x, w.uy = w.q.y - w.p.y;
    return w;
}
// (:316-320): the piece separates the centroid a of its face from the centroid b across an edge
__device__ __forceinline__ bool separates(const Widened &w, P2 a, bool a_left, P2 b) {
    if (left_of(b, w.p, w.ux, w.uy) == a_left) return false;
    const double vx = b.x - a.x, vy = b.y - a.y;
    return left_of(w.p, a, vx, vy) != left_of(w.q, a, vx, vy);
}

// The interior edges of one face in ascending id (connectivity.to_sparse sorts a face's edges) with the centroid across each:
// gathered ONCE per face and used for every piece of its row.  edge[k] = -1: no edge in this slot, or an exterior one.
template <int MC> struct FaceSides {
    int32_t edge[MC];
    P2 b[MC];
};
template <int MC>
__device__ __forceinline__ FaceSides<MC> load_sides(int32_t f, const int32_t *__restrict__ slots, const int2 *__restrict__ edge_face,
                                                    const double2 *__restrict__ centroid) {
    int32_t e[MC];
#pragma unroll
    for (int j = 0; j < MC; j++) e[j] = slots[j] < 0 ? INT32_MAX : slots[j];
#pragma unroll
    for (int i = 0; i < MC - 1; i++) {
#pragma unroll
        for (int j = 0; j < MC - 1 - i; j++) {
            const int32_t lo = min(e[j], e[j + 1]), hi = max(e[j], e[j + 1]);
            e[j] = lo, e[j + 1] = hi;
        }
    }
    FaceSides<MC> s;
#pragma unroll
    for (int k = 0; k < MC; k++) {
        const bool has = e[k] != INT32_MAX && (k == 0 || e[k] != e[k - 1]);
        const int2 ff = has ? edge_face[e[k]] : make_int2(-1, -1);
        const int32_t other = ff.y == f ? ff.x : ff.y;
        const double2 cb = centroid[other >= 0 ? other : f];
        s.edge[k] = has && other >= 0 ? e[k] : -1;
        s.b[k] = P2{cb.x, cb.y};
    }
    return s;
}

// snap_to_edges (:289-325) for ONE piece c -> d inside a face with centroid a: emit(edge) for every edge that passes, in
// ascending edge id.  -> their number.
template <int MC, typename Emit>
__device__ __forceinline__ int piece_rows(P2 a, const FaceSides<MC> &s, P2 c, P2 d, double tolerance, Emit &&emit) {
    const Widened w = widen_piece(c, d, tolerance);
    if (!w.any) return 0;
    const bool a_left = left_of(a, w.p, w.ux, w.uy);
    int n = 0;
#pragma unroll
    for (int k = 0; k < MC; k++) {
        if (s.edge[k] >= 0 && separates(w, a, a_left, s.b[k])) {
            emit(s.edge[k]);
            n++;
        }
    }
    return n;
}

// ... for faces of any width: the edges are picked from the face's slots in ascending id, piece by piece (at most m rounds of
// m slots)
template <typename Emit>
__device__ __forceinline__ int piece_rows_any(int32_t f, P2 a, P2 c, P2 d, double tolerance, const double2 *__restrict__ centroid,
                                              const int32_t *__restrict__ slots, int m, const int2 *__restrict__ edge_face, Emit &&emit) {
    const Widened w = widen_piece(c, d, tolerance);
    if (!w.any) return 0;
    const bool a_left = left_of(a, w.p, w.ux, w.uy);
    int n = 0;
    int32_t last = -1;
    for (int k = 0; k < m; k++) {
        int32_t e = INT32_MAX;
        for (int j = 0; j < m; j++) {
            const int32_t v = slots[j];
            if (v > last && v < e) e = v;
        }
        if (e == INT32_MAX) break; // (the -1 padding of a short face never exceeds `last`)
        last = e;
        const int2 ff = edge_face[e];
        const int32_t other = ff.y == f ? ff.x : ff.y;
        if (other < 0) continue; // exterior
        const double2 cb = centroid[other];
        if (separates(w, a, a_left, P2{cb.x, cb.y})) {
            emit(e);
            n++;
        }
    }
    return n;
}

// entry_face[p] = the face (row) of CSR entry p: one lane per face writes its row's entries
__global__ void __launch_bounds__(SG)
k_sg_entry_face(const int32_t *__restrict__ indptr, int64_t n_face, int32_t *__restrict__ entry_face) {
    const int64_t f = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (f >= n_face) return;
    for (int32_t p = indptr[f], p1 = indptr[f + 1]; p < p1; p++) entry_face[p] = (int32_t)f;
}

// One lane per CSR entry p = (face, segment); the entries of a face are neighbours, so a wave gathers the vertices, edges and
// centroids of a dozen faces, not of 64.  FILL = false: count[p] = rows of the entry, seg_hist[segment] += them, the words of `total` += them.
// FILL = true: the rows go to row_off[p] ..., in ascending edge id, and into the bucket of their segment through its cursor (the
// bucket is sorted afterwards: k_sg_bucket_sort); an entry without rows is passed over before anything of it is fetched.
// MC = 3 / 4: meshes of that width keep the face's sides in registers; MC = 0: any width.
template <bool FILL, int MC>
__global__ void __launch_bounds__(SG)
k_sg_rows(const int32_t *__restrict__ entry_face, const int32_t *__restrict__ indices, int64_t n_entry, const double *__restrict__ fxy,
          const uint8_t *__restrict__ len, const int32_t *__restrict__ off, int m_mesh, const double4 *__restrict__ seg,
          const double2 *__restrict__ centroid, const int32_t *__restrict__ face_edge, int m, const int2 *__restrict__ edge_face,
          double tolerance, int32_t *__restrict__ count, int32_t *__restrict__ seg_hist, unsigned long long *__restrict__ total,
          const int32_t *__restrict__ row_off, const int32_t *__restrict__ bucket_start, int32_t *__restrict__ cursor,
          int32_t *__restrict__ u_seg, int32_t *__restrict__ u_edge, double4 *__restrict__ u_xy, int32_t *__restrict__ order,
          int64_t n_row) {
    const int64_t p = (int64_t)blockIdx.x * SG + threadIdx.x;
    unsigned long long mine = 0;
    bool live = p < n_entry;
    int32_t r = 0, r1 = 0;
    if constexpr (FILL) {
        if (live) r = row_off[p], r1 = row_off[p + 1];
        live = r < r1;
    }
    if (live) {
        const int32_t f = entry_face[p], s = indices[p];
        const double4 ab = seg[s];
        const double2 ca = centroid[f];
        const P2 a{ca.x, ca.y};
        const int32_t *slots = face_edge + (int64_t)f * m;
        P2 c{NAN, NAN}, d{NAN, NAN};
        cyrus_beck_length(fxy + 2 * face_vertex_base(off, f, m_mesh), len[f], P2{ab.x, ab.y}, P2{ab.z, ab.w}, &c, &d);
        auto rows_of = [&](auto &&emit) {
            if constexpr (MC > 0) return piece_rows<MC>(a, load_sides<MC>(f, slots, edge_face, centroid), c, d, tolerance, emit);
            else return piece_rows_any(f, a, c, d, tolerance, centroid, slots, m, edge_face, emit);
        };
        if constexpr (!FILL) {
            const int n = rows_of([](int32_t) {});
            count[p] = n;
            if (n) atomicAdd(&seg_hist[s], n);
            mine = (unsigned long long)n;
        } else {
            rows_of([&](int32_t e) {
                if (r < r1 && r < n_row) { // (what the count pass found: the two passes run the same arithmetic)
                    u_seg[r] = s;
                    u_edge[r] = e;
                    u_xy[r] = make_double4(c.x, c.y, d.x, d.y);
                    const int32_t at = bucket_start[s] + atomicAdd(&cursor[s], 1);
                    if (at < bucket_start[s + 1]) order[at] = r;
                    r++;
                }
            });
        }
    }
    if constexpr (!FILL) {
        mine = wave_reduce<OpSum>(mine);
        // (one word for all waves is one atomic at a time: 88 000 waves on it were four fifths of this kernel)
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&total[(blockIdx.x % SG_TOTALS) * SG_TOTAL_STRIDE], mine);
    }
}

// One lane per segment: its bucket of `order` ascending.  Short buckets here; the others are listed for k_sg_bucket_sort_big.
__global__ void __launch_bounds__(SG)
k_sg_bucket_sort(const int32_t *__restrict__ bucket_start, int64_t n_seg, int32_t *__restrict__ order, int32_t *__restrict__ long_list,
                 int32_t *__restrict__ n_long) {
    const int64_t s = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (s >= n_seg) return;
    const int32_t b = bucket_start[s], n = bucket_start[s + 1] - b;
    if (n > SG_SORT_SMALL) {
        long_list[atomicAdd(n_long, 1)] = (int32_t)s;
        return;
    }
    int32_t *row = order + b;
    for (int i = 1; i < n; i++) {
        const int32_t key = row[i];
        int j = i - 1;
        while (j >= 0 && row[j] > key) {
            row[j + 1] = row[j];
            j--;
        }
        row[j + 1] = key;
    }
}

// one block per listed bucket (a segment that crosses many faces): the bitonic network of xr_prims.h in global memory, any length
__global__ void __launch_bounds__(SG)
k_sg_bucket_sort_big(const int32_t *__restrict__ bucket_start, int32_t *__restrict__ order, const int32_t *__restrict__ long_list,
                     const int32_t *__restrict__ n_long) {
    const int n = *n_long;
    for (int i = blockIdx.x; i < n; i += gridDim.x) { // (block-uniform)
        const int32_t s = long_list[i], b = bucket_start[s];
        block_sort_ascending<SG>(order + b, (int64_t)(bucket_start[s + 1] - b));
    }
}

// frame row j = CSR-walk row order[j]: line, edge, the un-widened piece and its SQUARED length (snapping.py:491)
__global__ void __launch_bounds__(SG)
k_sg_gather(const int32_t *__restrict__ order, int64_t n_row, const int32_t *__restrict__ u_seg, const int32_t *__restrict__ u_edge,
            const double4 *__restrict__ u_xy, const int32_t *__restrict__ seg_line, int32_t *__restrict__ row_line,
            int32_t *__restrict__ row_edge, double *__restrict__ columns /* [5][n_row]: x0, y0, x1, y1, length */) {
    const int64_t j = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (j >= n_row) return;
    const int32_t r = order[j];
    const double4 v = u_xy[r];
    row_line[j] = seg_line[u_seg[r]];
    row_edge[j] = u_edge[r];
    columns[j] = v.x;
    columns[n_row + j] = v.y;
    columns[2 * n_row + j] = v.z;
    columns[3 * n_row + j] = v.w;
    const double dx = v.z - v.x, dy = v.w - v.y;
    columns[4 * n_row + j] = dx * dx + dy * dy;
}

// best[edge] = max over its rows of the bits of length (lengths are >= +0: their order is that of their bit patterns)
__global__ void __launch_bounds__(SG)
k_sg_longest(const int32_t *__restrict__ row_edge, const double *__restrict__ length, int64_t n_row, unsigned long long *__restrict__ best) {
    const int64_t j = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (j < n_row) atomicMax(&best[row_edge[j]], (unsigned long long)__double_as_longlong(length[j]));
}

// first[edge] = the lowest frame row among those of maximal length
__global__ void __launch_bounds__(SG)
k_sg_first(const int32_t *__restrict__ row_edge, const double *__restrict__ length, int64_t n_row,
           const unsigned long long *__restrict__ best, int32_t *__restrict__ first) {
    const int64_t j = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (j >= n_row) return;
    const int32_t e = row_edge[j];
    if ((unsigned long long)__double_as_longlong(length[j]) == best[e]) atomicMin(&first[e], (int32_t)j);
}

// edge_line[e] = line of the winning row, -1 for an edge without rows; flag[e] = 1 for the others
__global__ void __launch_bounds__(SG)
k_sg_winner(const int32_t *__restrict__ first, const int32_t *__restrict__ row_line, int64_t n_edge, int32_t *__restrict__ edge_line,
            int32_t *__restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (e >= n_edge) return;
    const int32_t j = first[e];
    edge_line[e] = j == INT32_MAX ? -1 : row_line[j];
    flag[e] = j != INT32_MAX;
}

// out[e] = the line as a float, NaN for none (the reference's uds["line_index"])
__global__ void __launch_bounds__(SG) k_sg_line_index(const int32_t *__restrict__ edge_line, int64_t n_edge, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (e < n_edge) out[e] = edge_line[e] < 0 ? NAN : (double)edge_line[e];
}

// out[k] = edge_line[ids[k]]
__global__ void __launch_bounds__(SG)
k_sg_edge_lines(const int32_t *__restrict__ edge_line, const int32_t *__restrict__ ids, int64_t n, int64_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (k < n) out[k] = edge_line[ids[k]];
}

// out[k][e] = values[k][line of e], NaN for an edge without a line
__global__ void __launch_bounds__(SG)
k_sg_values(const int32_t *__restrict__ edge_line, int64_t n_edge, const double *__restrict__ values, int64_t n_line, int64_t K,
            double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * SG + threadIdx.x;
    if (e >= n_edge) return;
    const int32_t l = edge_line[e];
    for (int64_t k = 0; k < K; k++) out[k * n_edge + e] = l < 0 ? NAN : values[k * n_line + l];
}

} // namespace xr

// The frame of one create_snap_to_grid_dataframe and, when asked for, its reduction (include/xugrid_amd.h)
struct xr_snapgrid {
    int64_t n_line = 0, n_edge = 0, n_piece = 0, n_row = 0;
    bool reduced = false;
    xr::DevBuf<int32_t> row_line, row_edge; // [n_row] in frame order
    xr::DevBuf<double> columns;             // [5][n_row] x0, y0, x1, y1, length
    xr::DevBuf<int32_t> edge_line;          // [n_edge] the winning line, -1 for none
    std::unique_ptr<xr_index> snapped;      // the edges with a line, ascending
};

using namespace xr;

namespace {

void snapgrid_build(xr_snapgrid *h, xr_mesh *mesh, const xr_topology *topology, const xr_nn *node_index, const double *coords_dev,
                    int64_t n_vertex, const int64_t *line_off, int64_t n_line, double max_snap_distance, double tolerance, bool reduce) {
    const int64_t F = mesh->n_face, E = topology->n_edge;
    h->n_line = n_line, h->n_edge = E;
    if (n_line > 0) {
        DevBuf<int32_t> flag(1);
        fill_i32(flag.get(), 0, 1);
        XR_LAUNCH("snapgrid_check_offsets", k_sg_check_offsets, dim3(div_up(n_line + 1, SG)), dim3(SG), 0, line_off, n_line + 1, n_vertex,
                  flag.get());
        XR_REQUIRE(read_scalar(flag.get()) == 0, XR_ERR_INVALID, "line_offsets must start at 0, end at %lld and never decrease",
                   (long long)n_vertex);
    } else {
        XR_REQUIRE(n_vertex == 0, XR_ERR_INVALID, "line_offsets must start at 0, end at %lld and never decrease", (long long)n_vertex);
    }
    std::unique_ptr<xr_csr> csr;
    DevBuf<double4> seg;
    DevBuf<int32_t> seg_line;
    if (n_vertex > 0 && F > 0 && E > 0) {
        // 1. vertices onto nodes (copies of node coordinates), 2. segments
        DevBuf<double> snapped((size_t)n_vertex * 2);
        const int rc = xr_nn_snap_dev(node_index, coords_dev, coords_dev + 1, 2, n_vertex, max_snap_distance, snapped.get(),
                                      snapped.get() + 1, 2, nullptr, nullptr);
        if (rc != XR_OK) throw Failure{rc};
        seg.alloc((size_t)n_vertex), seg_line.alloc((size_t)n_vertex);
        XR_LAUNCH("snapgrid_segments", k_sg_segments, dim3(div_up(n_vertex, SG)), dim3(SG), 0,
                  reinterpret_cast<const double2 *>(snapped.get()), n_vertex, line_off, n_line, seg.get(), seg_line.get());
        // 3. pieces: the faces x segments matrix of the clipper
        xr_csr *made = nullptr;
        const int rc2 = xr_edge_length_csr_dev(mesh, reinterpret_cast<const double *>(seg.get()), n_vertex, &made);
        if (rc2 != XR_OK) throw Failure{rc2};
        csr.reset(made);
        h->n_piece = csr->nnz;
    }
    if (h->n_piece > 0) {
        XR_REQUIRE(h->n_piece < ((int64_t)1 << 30), XR_ERR_LIMIT, "xr_snapgrid_create_dev: too many pieces");
        mesh_prepare(mesh, true);
        mesh_face_coords(mesh);
        const auto centroids = mesh_centroids_shared(mesh);
        const int64_t P = h->n_piece, S = n_vertex;
        // 4. rows: count, scan, fill
        DevBuf<int32_t> count((size_t)P), row_off((size_t)P + 1), seg_hist((size_t)S), bucket_start((size_t)S + 1), entry_face((size_t)P);
        XR_LAUNCH("snapgrid_rows_faces", k_sg_entry_face, dim3(div_up(F, SG)), dim3(SG), 0, csr->indptr.get(), F, entry_face.get());
        DevBuf<unsigned long long> total_dev((size_t)SG_TOTALS * SG_TOTAL_STRIDE);
        fill_i32(seg_hist.get(), 0, S);
        fill_i32(reinterpret_cast<int32_t *>(total_dev.get()), 0, 2 * SG_TOTALS * SG_TOTAL_STRIDE);
        auto rows = [&](auto fill, int32_t *cursor, int32_t *u_seg, int32_t *u_edge, double4 *u_xy, int32_t *order, int64_t n_row) {
            with_nodes_per_face(topology->m, [&](auto mc) {
                XR_LAUNCH(fill() ? "snapgrid_rows_fill" : "snapgrid_rows_count", (k_sg_rows<fill(), mc()>), dim3(div_up(P, SG)), dim3(SG),
                          0, entry_face.get(), csr->indices.get(), P, mesh->prep.fxy.get(), mesh->prep.len.get(), mesh->caller_off(), mesh->m,
                          seg.get(), reinterpret_cast<const double2 *>(centroids->get()), topology->face_edge.get(), topology->m,
                          reinterpret_cast<const int2 *>(topology->edge_face.get()), tolerance, count.get(), seg_hist.get(),
                          total_dev.get(), row_off.get(), bucket_start.get(), cursor, u_seg, u_edge, u_xy, order, n_row);
            });
        };
        rows(std::false_type(), nullptr, nullptr, nullptr, nullptr, nullptr, 0);
        unsigned long long totals[SG_TOTALS * SG_TOTAL_STRIDE], total = 0;
        d2h(totals, total_dev.get(), sizeof(totals));
        for (int i = 0; i < SG_TOTALS; i++) total += totals[i * SG_TOTAL_STRIDE];
        XR_REQUIRE(total < (1ull << 30), XR_ERR_LIMIT, "xr_snapgrid_create_dev: too many rows");
        const int64_t R = (int64_t)total;
        h->n_row = R;
        if (R > 0) {
            exclusive_scan_i32(count.get(), row_off.get(), P);
            exclusive_scan_i32(seg_hist.get(), bucket_start.get(), S);
            DevBuf<int32_t> u_seg((size_t)R), u_edge((size_t)R), order((size_t)R), cursor((size_t)S);
            DevBuf<double4> u_xy((size_t)R);
            fill_i32(cursor.get(), 0, S);
            rows(std::true_type(), cursor.get(), u_seg.get(), u_edge.get(), u_xy.get(), order.get(), R);
            // 5. order: every bucket ascending
            DevBuf<int32_t> long_list((size_t)(R / (SG_SORT_SMALL + 1) + 1)), n_long(1);
            fill_i32(n_long.get(), 0, 1);
            XR_LAUNCH("snapgrid_order", k_sg_bucket_sort, dim3(div_up(S, SG)), dim3(SG), 0, bucket_start.get(), S, order.get(),
                      long_list.get(), n_long.get());
            XR_LAUNCH("snapgrid_order_big", k_sg_bucket_sort_big, dim3(engine().num_cu * 2), dim3(SG), 0, bucket_start.get(), order.get(),
                      long_list.get(), n_long.get());
            h->row_line.alloc((size_t)R), h->row_edge.alloc((size_t)R), h->columns.alloc((size_t)R * 5);
            XR_LAUNCH("snapgrid_gather", k_sg_gather, dim3(div_up(R, SG)), dim3(SG), 0, order.get(), R, u_seg.get(), u_edge.get(),
                      u_xy.get(), seg_line.get(), h->row_line.get(), h->row_edge.get(), h->columns.get());
            stream_sync(); // (the scratch goes back to the pool behind its readers)
        }
    }
    if (reduce) {
        // 6. per edge the first row of greatest length
        h->reduced = true;
        h->edge_line.alloc((size_t)E);
        if (E > 0) {
            const int64_t R = h->n_row;
            DevBuf<unsigned long long> best((size_t)E);
            DevBuf<int32_t> first((size_t)E), flag((size_t)E);
            fill_i32(reinterpret_cast<int32_t *>(best.get()), 0, 2 * E);
            fill_i32(first.get(), INT32_MAX, E);
            if (R > 0) {
                const double *length = h->columns.get() + 4 * R;
                XR_LAUNCH("snapgrid_longest", k_sg_longest, dim3(div_up(R, SG)), dim3(SG), 0, h->row_edge.get(), length, R, best.get());
                XR_LAUNCH("snapgrid_first", k_sg_first, dim3(div_up(R, SG)), dim3(SG), 0, h->row_edge.get(), length, R, best.get(),
                          first.get());
            }
            XR_LAUNCH("snapgrid_winner", k_sg_winner, dim3(div_up(E, SG)), dim3(SG), 0, first.get(), h->row_line.get(), E,
                      h->edge_line.get(), flag.get());
            h->snapped.reset(index_from_flags(flag.get(), E));
        } else {
            h->snapped.reset(index_from_flags(nullptr, 0));
        }
    }
    stream_sync(); // (the matrix and the segments go back to the pool behind their readers)
}

} // namespace

extern "C" {

int xr_snapgrid_create_dev(xr_mesh *mesh, const xr_topology *topology, const xr_nn *node_index, const double *coords_dev,
                           int64_t n_vertex, const int64_t *line_offsets_dev, int64_t n_line, double max_snap_distance,
                           double tolerance, int reduce, xr_snapgrid **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && topology && out, XR_ERR_INVALID, "xr_snapgrid_create_dev: NULL argument");
    XR_REQUIRE(topology->mesh == mesh, XR_ERR_INVALID, "xr_snapgrid_create_dev: the topology does not belong to this mesh");
    XR_REQUIRE(topology->n_nonmanifold == 0, XR_ERR_INVALID, "xr_snapgrid_create_dev: an edge of the mesh has more than two faces");
    XR_REQUIRE(n_vertex >= 0 && n_line >= 0, XR_ERR_INVALID, "xr_snapgrid_create_dev: negative size");
    XR_REQUIRE(n_vertex < ((int64_t)1 << 30) && n_line < INT32_MAX, XR_ERR_LIMIT, "xr_snapgrid_create_dev: too many vertices or lines");
    XR_REQUIRE((coords_dev || n_vertex == 0) && line_offsets_dev, XR_ERR_INVALID, "xr_snapgrid_create_dev: NULL argument");
    XR_REQUIRE(node_index || mesh->n_node == 0 || n_vertex == 0, XR_ERR_INVALID, "xr_snapgrid_create_dev: the node index is missing");
    XR_REQUIRE(max_snap_distance >= 0.0, XR_ERR_INVALID, "xr_snapgrid_create_dev: max_snap_distance must be non-negative");
    XR_REQUIRE(tolerance == tolerance, XR_ERR_INVALID, "xr_snapgrid_create_dev: tolerance is NaN");
    Building<xr_snapgrid> h(OnFailure::WaitFirst);
    snapgrid_build(h.get(), mesh, topology, node_index, coords_dev, n_vertex, line_offsets_dev, n_line, max_snap_distance, tolerance,
                   reduce != 0);
    dev_call_done();
    *out = h.release();
    XR_API_END
}

int xr_snapgrid_info(const xr_snapgrid *h, int64_t *n_piece, int64_t *n_row, int64_t *n_snapped) {
    XR_API_BEGIN
    XR_REQUIRE(h, XR_ERR_INVALID, "xr_snapgrid_info: NULL handle");
    if (n_piece) *n_piece = h->n_piece;
    if (n_row) *n_row = h->n_row;
    if (n_snapped) *n_snapped = h->snapped ? h->snapped->n : 0;
    XR_API_END
}

int xr_snapgrid_copy_dev(const xr_snapgrid *h, int what, void *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(h && what >= XR_SNAPGRID_LINE && what <= XR_SNAPGRID_EDGE_LINES, XR_ERR_INVALID, "xr_snapgrid_copy_dev: bad argument");
    const int64_t R = h->n_row, E = h->n_edge;
    if (what <= XR_SNAPGRID_LENGTH) {
        XR_REQUIRE(out_dev || R == 0, XR_ERR_INVALID, "xr_snapgrid_copy_dev: NULL argument");
        if (R > 0) {
            if (what == XR_SNAPGRID_LINE) widen_dev(h->row_line.get(), R, static_cast<int64_t *>(out_dev));
            else if (what == XR_SNAPGRID_EDGE) widen_dev(h->row_edge.get(), R, static_cast<int64_t *>(out_dev));
            else
                XR_HIP(hipMemcpyAsync(out_dev, h->columns.get() + (int64_t)(what - XR_SNAPGRID_X0) * R, sizeof(double) * (size_t)R,
                                      hipMemcpyDeviceToDevice, launch_stream()));
        }
    } else {
        XR_REQUIRE(h->reduced, XR_ERR_INVALID, "xr_snapgrid_copy_dev: the handle was made without the reduction");
        const int64_t n = what == XR_SNAPGRID_LINE_INDEX ? E : h->snapped->n;
        XR_REQUIRE(out_dev || n == 0, XR_ERR_INVALID, "xr_snapgrid_copy_dev: NULL argument");
        if (n > 0) {
            if (what == XR_SNAPGRID_LINE_INDEX)
                XR_LAUNCH("snapgrid_line_index", k_sg_line_index, dim3(div_up(E, SG)), dim3(SG), 0, h->edge_line.get(), E,
                          static_cast<double *>(out_dev));
            else if (what == XR_SNAPGRID_EDGES) widen_dev(h->snapped->ids.get(), n, static_cast<int64_t *>(out_dev));
            else
                XR_LAUNCH("snapgrid_edge_lines", k_sg_edge_lines, dim3(div_up(n, SG)), dim3(SG), 0, h->edge_line.get(),
                          h->snapped->ids.get(), n, static_cast<int64_t *>(out_dev));
        }
    }
    dev_call_done();
    XR_API_END
}

int xr_snapgrid_values_dev(const xr_snapgrid *h, const double *values_dev, int64_t K, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(h && K >= 0, XR_ERR_INVALID, "xr_snapgrid_values_dev: bad argument");
    XR_REQUIRE(h->reduced, XR_ERR_INVALID, "xr_snapgrid_values_dev: the handle was made without the reduction");
    if (K > 0 && h->n_edge > 0) {
        XR_REQUIRE(out_dev && (values_dev || h->n_line == 0), XR_ERR_INVALID, "xr_snapgrid_values_dev: NULL argument");
        XR_LAUNCH("snapgrid_values", k_sg_values, dim3(div_up(h->n_edge, SG)), dim3(SG), 0, h->edge_line.get(), h->n_edge, values_dev,
                  h->n_line, K, out_dev);
    }
    dev_call_done();
    XR_API_END
}

int xr_snapgrid_destroy(xr_snapgrid *h) {
    XR_API_BEGIN
    if (h) {
        release_point();
        delete h;
    }
    XR_API_END
}

} // extern "C"
