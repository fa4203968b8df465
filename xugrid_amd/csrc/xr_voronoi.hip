// xr_voronoi.hip -- the O(n) part of the centroidal Voronoi pre-step of BarycentricInterpolator on the
// device.
//
// Replaces, for the call made at xugrid/regrid/unstructured.py:151-165
// (voronoi_topology(..., add_exterior=True, add_vertices=True, skip_concave=True)):
//   * Ugrid2d.node_face_connectivity (ugrid/ugrid2d.py:700-713 -> connectivity.invert_dense_to_sparse,
//     ugrid/connectivity.py:247-259)                      -> node -> faces CSR by counting sort
//   * Ugrid2d.edge_node_connectivity / edge_face_connectivity (ugrid2d.py:497-509, :661-677 ->
//     connectivity.edge_connectivity, connectivity.py:419-457) -- of which the Voronoi step only uses
//     the EXTERIOR edges (voronoi.py:77-97)               -> exterior half-edges found through the CSR
//   * the interior cells: centroids of the faces around every node that touches no exterior edge,
//     ordered counter-clockwise about the node (voronoi.py:355-372: lexsort((arctan2, node)))
//   * the assembly of the dense, -1 padded cell table and of the vertex array into a device-resident mesh
// The cells of nodes ON the boundary (projections on exterior edges, substitute vertices, convexity
// choice: voronoi.py:59-327) are O(boundary) host work on a few KB the device gathers (xr_voronoi_boundary.h); they are
// handed back in as a small table.
// The same builder serves the public tessellations (ugrid2d.py:1664-1732): any flag set of voronoi_topology and any
// generator points (xr_voronoi_create_flags).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include <cstring>

#include "xr_node_faces.h"
#include "xr_objects.h"
#include "xr_prims.h"
#include "xr_voronoi_boundary.h"

struct xr_voronoi {
    xr_mesh *mesh = nullptr; // borrowed: the caller keeps the source mesh alive
    int64_t n_node = 0, n_face = 0, nnz = 0;
    // what is built (voronoi.py:330-458): add_exterior closes the cells of the boundary nodes; without it every node with at
    // least three faces gets an open-ended cell of generator points only, and the vertices are compacted to the points used
    bool add_exterior = true, add_vertices = true, skip_concave = true;
    xr::DevBuf<int32_t> vertex_rank; // [n_face+1] !add_exterior: exclusive scan of "some cell uses this generator point"
    int64_t n_used = 0, max_used = -1; // !add_exterior: points used, the largest used face id
    xr::DevBuf<int32_t> indptr;    // [n_node+1]
    xr::DevBuf<int32_t> faces_asc; // [nnz] faces around each node, ascending (scipy CSR order)
    xr::DevBuf<int32_t> faces_ccw; // [nnz] interior nodes: counter-clockwise about the node
    xr::DevBuf<uint8_t> interior;  // [n_node] 1 = has faces and touches no exterior edge
    xr::DevBuf<int32_t> cell_rank; // [n_node+1] exclusive scan of `interior`
    xr::DevBuf<double> centroids;  // [n_face*2] the generator points: face centroids, or what the caller handed in
    int64_t n_interior = 0;
    int max_degree = 0, min_degree = 0; // over interior nodes
    std::vector<int64_t> edge_lo, edge_hi, edge_face; // exterior edges, lexicographic (lo, hi)
    // the rows of the boundary nodes (what the O(boundary) host part reads), gathered on first request
    bool boundary_ready = false;
    std::vector<int64_t> b_nodes, b_ptr, b_faces; // ascending node ids, CSR offsets, faces ascending per node
    std::vector<double> b_face_xy, b_edge_face_xy; // centroid of every listed face / of every exterior edge's face
    std::vector<double> b_node_xy;                 // coordinates of the boundary nodes
    // the cells of the boundary nodes (voronoi_boundary_cells: native O(boundary) host part)
    bool cells_ready = false;
    std::vector<double> c_extra_xy;   // vertices added behind the n_face centroids: kept projections, then one per boundary node
    std::vector<int64_t> c_cells;     // [c_n_cell][c_m] global vertex ids, -1 padded, counter-clockwise
    int64_t c_n_cell = 0, c_m = 0;
    std::vector<int64_t> c_tail;      // source face of every added vertex (-1: the per-node extras)
    std::vector<int64_t> c_interp;    // [n_extra][2] the two projection vertex ids an extra corner sits between
};

namespace xr {

__device__ __forceinline__ int face_len(const int32_t *__restrict__ face, int m) {
    int n = m;
    for (int i = m - 1; i >= 3; i--)
        if (face[i] < 0) n = i;
    return n;
}

// One thread per half-edge (face f, slot j): a -> b.  The edge is exterior iff no OTHER face around node a
// has a and b as ring neighbours (either direction).  Exterior edges are appended (unordered).
__global__ void __launch_bounds__(256)
k_vor_exterior(const int32_t *__restrict__ faces, int64_t n_face, int m, const int32_t *__restrict__ indptr,
               const int32_t *__restrict__ rows, uint8_t *__restrict__ on_boundary, int32_t *__restrict__ n_edges,
               int32_t *__restrict__ e_all /* (lo, hi, face) per exterior edge: one download */) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_face * m) return;
    const int64_t f = i / m;
    const int j = (int)(i - f * m);
    const int32_t *face = faces + f * m;
    const int n = face_len(face, m);
    if (j >= n) return;
    const int a = face[j], b = face[j + 1 == n ? 0 : j + 1]; // (wrap by compare: `% n` with a run-time n is an integer division)
    if (a == b) return;
    bool shared = false;
    if (m == 3) {
        // triangles: any two nodes of a face are ring neighbours, so the edge is shared iff a face other than f is in the rows
        // of BOTH nodes -- a merge of two short ascending rows (k_vor_sort_rows ran before), contiguous reads, instead of a
        // gather of every neighbouring face's node list
        int ia = indptr[a], ib = indptr[b];
        const int ea = indptr[a + 1], eb = indptr[b + 1];
        constexpr int ROW_REG = 8; // (a Delaunay node has ~6 faces)
        if (ea - ia <= ROW_REG && eb - ib <= ROW_REG) {
            // both rows in registers with ONE round of independent loads, then the intersection by all pairs: the merge below is a
            // chain of ~10 dependent pairs of loads per half-edge (the kernel waited on memory for 57 % of its wave cycles)
            int ra[ROW_REG], rb[ROW_REG];
#pragma unroll
            for (int u = 0; u < ROW_REG; u++) ra[u] = ia + u < ea ? rows[ia + u] : -1;
#pragma unroll
            for (int u = 0; u < ROW_REG; u++) rb[u] = ib + u < eb ? rows[ib + u] : -2;
#pragma unroll
            for (int u = 0; u < ROW_REG; u++) {
                bool in_b = false;
#pragma unroll
                for (int w = 0; w < ROW_REG; w++) in_b = in_b || ra[u] == rb[w];
                shared = shared || (in_b && ra[u] != (int)f);
            }
        } else
        while (ia < ea && ib < eb) {
            const int ga = rows[ia], gb = rows[ib];
            if (ga == gb) {
                if (ga != f) {
                    shared = true;
                    break;
                }
                ia++;
                ib++;
            } else if (ga < gb) {
                ia++;
            } else {
                ib++;
            }
        }
    } else
    for (int r = indptr[a]; r < indptr[a + 1] && !shared; r++) {
        const int g = rows[r];
        if (g == f) continue;
        const int32_t *other = faces + (int64_t)g * m;
        const int k = face_len(other, m);
        for (int t = 0; t < k; t++) {
            if (other[t] != a) continue;
            if (other[t + 1 == k ? 0 : t + 1] == b || other[t == 0 ? k - 1 : t - 1] == b) shared = true;
        }
    }
    if (shared) return;
    on_boundary[a] = 1;
    on_boundary[b] = 1;
    const int at = atomicAdd(n_edges, 1);
    e_all[3 * (int64_t)at] = a < b ? a : b;
    e_all[3 * (int64_t)at + 1] = a < b ? b : a;
    e_all[3 * (int64_t)at + 2] = (int32_t)f;
}

__global__ void k_vor_init_counters(int32_t *__restrict__ c) {
    if (threadIdx.x < 8) c[threadIdx.x] = threadIdx.x == 1 ? INT32_MAX : 0;
}
__global__ void k_vor_totals(const int32_t *__restrict__ n_interior, const int32_t *__restrict__ nnz, int32_t *__restrict__ c) {
    if (threadIdx.x == 0) {
        c[3] = *n_interior;
        c[4] = *nnz;
    }
}

// angle class of a direction in arctan2's order (-pi, pi]: 0: dy < 0, 1: dy == 0 & dx >= 0, 2: dy > 0,
// 3: dy == 0 & dx < 0
__device__ __forceinline__ int angle_class(double dx, double dy) {
    if (dy < 0) return 0;
    if (dy > 0) return 2;
    return dx < 0 ? 3 : 1;
}

// true iff direction a comes strictly before direction b in arctan2 order
__device__ __forceinline__ bool angle_less(double ax, double ay, double bx, double by) {
    const int ca = angle_class(ax, ay), cb = angle_class(bx, by);
    if (ca != cb) return ca < cb;
    if (ca == 1 || ca == 3) return false; // same ray
    return ax * by - ay * bx > 0;
}

// Interior nodes: order the surrounding face centroids counter-clockwise about the node (stable on ties:
// ascending face id, as lexsort).  Also flags the node and records the degree range.
// The row -- face ids and centroid offsets -- is gathered ONCE into the thread's LDS column (independent loads, four in
// flight) and insertion-sorted there: the same insertions and comparisons, in the same order, as the sort in global memory
// this replaces, whose every step was a load that depended on the store before it and re-gathered a centroid through L2
// (0.35 ms for 0.5M nodes; PMC: 164 MB written for 12 MB of rows).  Rows longer than VOR_CAP keep that path.
static constexpr int VOR_BLOCK = 128, VOR_CAP = 16;

__global__ void __launch_bounds__(VOR_BLOCK)
k_vor_interior(const double *__restrict__ node_xy, const double *__restrict__ cxy,
               const int32_t *__restrict__ indptr, const int32_t *__restrict__ rows_asc,
               const uint8_t *__restrict__ on_boundary, int64_t n_node, int32_t *__restrict__ rows_ccw,
               uint8_t *__restrict__ interior, int32_t *__restrict__ flag32, int32_t *__restrict__ deg_minmax,
               int all_nodes /* 1: add_exterior = False -- every node with at least three faces, boundary nodes included */) {
    __shared__ double2 sh_d[VOR_CAP][VOR_BLOCK];
    __shared__ int32_t sh_k[VOR_CAP][VOR_BLOCK];
    const int t = threadIdx.x;
    const int64_t v = (int64_t)blockIdx.x * VOR_BLOCK + t;
    const bool in_range = v < n_node;
    const int s = in_range ? indptr[v] : 0, e = in_range ? indptr[v + 1] : 0;
    const bool ok = in_range && (all_nodes ? e - s >= 3 : e > s && !on_boundary[v]);
    // degree range: reduced over the wave, and an atomic only when it improves what the word already holds -- one
    // atomicMin + one atomicMax per NODE on the same two words cost 0.13 ms of the kernel's 0.23 (A/B without them: 0.097)
    {
        int dmin = ok ? e - s : INT32_MAX, dmax = ok ? e - s : 0;
        dmin = wave_reduce<OpMin>(dmin), dmax = wave_reduce<OpMax>(dmax);
        if ((t & 63) == 0) {
            if (dmin < __hip_atomic_load(&deg_minmax[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&deg_minmax[0], dmin);
            if (dmax > __hip_atomic_load(&deg_minmax[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&deg_minmax[1], dmax);
        }
    }
    if (!in_range) return;
    interior[v] = ok;
    flag32[v] = ok;
    if (!ok) {
        for (int i = s; i < e; i++) rows_ccw[i] = rows_asc[i];
        return;
    }
    const P2 p = load_p2(node_xy, (int)v);
    const int deg = e - s;
    if (deg <= VOR_CAP) {
        for (int i0 = 0; i0 < deg; i0 += 8) { // (eight at a time: the typical row of six in ONE pair of dependent round trips)
            int key[8];
            P2 c[8];
#pragma unroll
            for (int u = 0; u < 8; u++) key[u] = rows_asc[s + (i0 + u < deg ? i0 + u : deg - 1)];
#pragma unroll
            for (int u = 0; u < 8; u++) c[u] = load_p2(cxy, key[u]);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (i0 + u < deg) {
                    sh_k[i0 + u][t] = key[u];
                    sh_d[i0 + u][t] = make_double2(c[u].x - p.x, c[u].y - p.y);
                }
            }
        }
        for (int i = 1; i < deg; i++) { // insertion sort of the thread's own column (no other thread touches it)
            const int key = sh_k[i][t];
            const double2 k = sh_d[i][t];
            int j = i - 1;
            while (j >= 0) {
                const double2 d = sh_d[j][t];
                if (!angle_less(k.x, k.y, d.x, d.y)) break;
                sh_d[j + 1][t] = d;
                sh_k[j + 1][t] = sh_k[j][t];
                j--;
            }
            sh_d[j + 1][t] = k;
            sh_k[j + 1][t] = key;
        }
        for (int i = 0; i < deg; i++) rows_ccw[s + i] = sh_k[i][t];
        return;
    }
    for (int i = s; i < e; i++) { // long rows: insertion sort in global memory
        const int key = rows_asc[i];
        const P2 c = load_p2(cxy, key);
        const double kx = c.x - p.x, ky = c.y - p.y;
        int j = i - 1;
        while (j >= s) {
            const P2 d = load_p2(cxy, rows_ccw[j]);
            if (!angle_less(kx, ky, d.x - p.x, d.y - p.y)) break;
            rows_ccw[j + 1] = rows_ccw[j];
            j--;
        }
        rows_ccw[j + 1] = key;
    }
}

// one thread per SLOT of the cell table (the lanes of a wave write consecutive words; a thread per node wrote its own
// 4 m bytes -- 64 partial lines per store instruction: 0.135 ms for a 44 MB table)
__global__ void __launch_bounds__(256)
k_vor_cells(const int32_t *__restrict__ indptr, const int32_t *__restrict__ rows_ccw,
            const uint8_t *__restrict__ interior, const int32_t *__restrict__ cell_rank, int64_t n_node, int m,
            int32_t *__restrict__ cells, const int32_t *__restrict__ vertex_rank /* nullptr: vertex id = face id */) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_node * m) return;
    const int64_t v = i / m;
    const int j = (int)(i - v * m);
    if (!interior[v]) return;
    const int s = indptr[v], n = indptr[v + 1] - s;
    int c = j < n ? rows_ccw[s + j] : -1;
    if (vertex_rank && c >= 0) c = vertex_rank[c];
    cells[(int64_t)cell_rank[v] * m + j] = c;
}

// add_exterior = False: the generator points some cell uses (a face is used iff one of its nodes has at least three faces),
// then -- behind the scan of the flags -- their coordinates in ascending face order and the largest used face id
__global__ void __launch_bounds__(256)
k_vor_used(const int32_t *__restrict__ faces, int64_t n_face, int m, const int32_t *__restrict__ indptr,
           int32_t *__restrict__ used) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int u = 0;
    for (int j = 0; j < m; j++) {
        const int a = faces[f * m + j];
        if (a >= 0 && indptr[a + 1] - indptr[a] >= 3) u = 1;
    }
    used[f] = u;
}

__global__ void __launch_bounds__(256)
k_vor_compact(const double *__restrict__ cxy, const int32_t *__restrict__ rank, int64_t n_face, double *__restrict__ out_xy,
              int32_t *__restrict__ max_used) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const int r = rank[f];
    if (rank[f + 1] == r) return; // not used
    reinterpret_cast<double2 *>(out_xy)[r] = reinterpret_cast<const double2 *>(cxy)[f];
    if (r + 1 == rank[n_face]) *max_used = (int32_t)f;
}

__global__ void __launch_bounds__(256)
k_vor_boundary_cells(const int32_t *__restrict__ table, int64_t n_rows, int mb, int m, int32_t *__restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * m) return;
    const int64_t r = i / m;
    const int j = (int)(i - r * m);
    cells[i] = j < mb ? table[r * mb + j] : -1;
}

// everything the host needs about the boundary except the rows themselves, in ONE launch: per boundary node its degree and
// coordinates, per exterior edge the centroid of its face.  `in` = [nodes (nb) | edge faces (ne)]; `out` (8-byte words) =
// [degree (nb, int64) | node xy (2 nb) | edge-face xy (2 ne)]
__global__ void __launch_bounds__(256)
k_vor_boundary_info(const int32_t *__restrict__ indptr, const double *__restrict__ node_xy, const double *__restrict__ centroids,
                    const int64_t *__restrict__ in, int64_t nb, int64_t ne, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double *out_d = reinterpret_cast<double *>(out);
    if (i < nb) {
        const int64_t v = in[i];
        out[i] = indptr[v + 1] - indptr[v];
        out_d[nb + 2 * i] = node_xy[2 * v];
        out_d[nb + 2 * i + 1] = node_xy[2 * v + 1];
    }
    if (i < ne) {
        const int64_t f = in[nb + i];
        out_d[3 * nb + 2 * i] = centroids[2 * f];
        out_d[3 * nb + 2 * i + 1] = centroids[2 * f + 1];
    }
}

// exclusive scan of the degrees by one block (a few thousand boundary nodes): ptr[0..n].  256 threads, a wave per SIMD: a block
// of 1024 threads needs four free wave slots on every SIMD of ONE CU, and beside a kernel that fills the device (the locate pass of
// a barycentric construction runs on the side stream during this phase) it waited 200 us for them.
__global__ void __launch_bounds__(256) k_vor_scan_deg(const int64_t *__restrict__ deg, int64_t n, int64_t *__restrict__ ptr) {
    constexpr int NT = 256;
    __shared__ long long sh[NT];
    const int t = threadIdx.x;
    const int64_t chunk = (n + NT - 1) / NT, i0 = (int64_t)t * chunk < n ? (int64_t)t * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
    long long sum = 0;
    for (int64_t i = i0; i < i1; i++) sum += deg[i];
    sh[t] = sum;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const long long add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    long long run = sh[t] - sum; // exclusive prefix of this thread's chunk
    for (int64_t i = i0; i < i1; i++) {
        ptr[i] = run;
        run += deg[i];
    }
    if (t == NT - 1) ptr[n] = sh[NT - 1];
}

// rows of the boundary nodes: `out` (8-byte words) = [faces (total, int64) | their centroids (2 total)]
__global__ void k_vor_row_gather(const int32_t *__restrict__ indptr, const int32_t *__restrict__ faces_asc,
                                 const double *__restrict__ centroids, const int64_t *__restrict__ nodes,
                                 const int64_t *__restrict__ ptr, int64_t n, int64_t total, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double *xy = reinterpret_cast<double *>(out) + total;
    const int s = indptr[nodes[i]], e = indptr[nodes[i] + 1];
    for (int r = s; r < e; r++) {
        const int f = faces_asc[r];
        const int64_t o = ptr[i] + (r - s);
        out[o] = f;
        xy[2 * o] = centroids[2 * f];
        xy[2 * o + 1] = centroids[2 * f + 1];
    }
}

// Three host <-> device round trips (one upload, two downloads of packed buffers) instead of the nine single-array copies
// this used to make: each is a stream synchronisation, ~20 us with the device idle in between.
static void voronoi_boundary(xr_voronoi *v) {
    if (v->boundary_ready) return;
    std::vector<int64_t> nodes(v->edge_lo);
    nodes.insert(nodes.end(), v->edge_hi.begin(), v->edge_hi.end());
    std::sort(nodes.begin(), nodes.end());
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    const int64_t nb = (int64_t)nodes.size(), ne = (int64_t)v->edge_face.size();
    v->b_nodes = nodes;
    v->b_ptr.assign((size_t)nb + 1, 0);
    v->b_faces.clear();
    v->b_face_xy.clear();
    v->b_edge_face_xy.assign((size_t)ne * 2, 0.0);
    v->b_node_xy.assign((size_t)nb * 2, 0.0);
    if (nb + ne > 0) {
        std::vector<int64_t> in(nodes);
        in.insert(in.end(), v->edge_face.begin(), v->edge_face.end());
        DevBuf<int64_t> d_in((size_t)(nb + ne)), d_info((size_t)(3 * nb + 2 * ne)), d_ptr((size_t)nb + 1);
        h2d(d_in.get(), in.data(), sizeof(int64_t) * (size_t)(nb + ne));
        XR_LAUNCH("vor_boundary_info", k_vor_boundary_info, dim3(div_up(std::max(nb, ne), 256)), dim3(256), 0, v->indptr.get(),
                  v->mesh->node_xy.get(), v->centroids.get(), d_in.get(), nb, ne, d_info.get());
        if (nb > 0) XR_LAUNCH("vor_scan_deg", k_vor_scan_deg, dim3(1), dim3(256), 0, d_info.get(), nb, d_ptr.get());
        std::vector<int64_t> info((size_t)(3 * nb + 2 * ne));
        d2h(info.data(), d_info.get(), sizeof(int64_t) * info.size());
        for (int64_t i = 0; i < nb; i++) v->b_ptr[(size_t)i + 1] = v->b_ptr[(size_t)i] + info[(size_t)i];
        if (nb > 0) memcpy(v->b_node_xy.data(), info.data() + nb, sizeof(double) * 2 * (size_t)nb);
        if (ne > 0) memcpy(v->b_edge_face_xy.data(), info.data() + 3 * nb, sizeof(double) * 2 * (size_t)ne);
        const int64_t total = v->b_ptr[(size_t)nb];
        v->b_faces.resize((size_t)total);
        v->b_face_xy.resize((size_t)total * 2);
        if (total > 0) {
            DevBuf<int64_t> d_rows((size_t)(3 * total));
            XR_LAUNCH("vor_row_gather", k_vor_row_gather, dim3(div_up(nb, 256)), dim3(256), 0, v->indptr.get(),
                      v->faces_asc.get(), v->centroids.get(), d_in.get(), d_ptr.get(), nb, total, d_rows.get());
            std::vector<int64_t> rows((size_t)(3 * total));
            d2h(rows.data(), d_rows.get(), sizeof(int64_t) * rows.size());
            memcpy(v->b_faces.data(), rows.data(), sizeof(int64_t) * (size_t)total);
            memcpy(v->b_face_xy.data(), rows.data() + total, sizeof(double) * 2 * (size_t)total);
        }
    }
    v->boundary_ready = true;
}


// The cells of the boundary nodes (voronoi.py:59-327): native host code on the few KB voronoi_boundary() gathered; the
// computation itself is plain C++ in xr_voronoi_boundary.h (also built stand-alone under the host sanitizers).
static void voronoi_boundary_cells(xr_voronoi *v) {
    if (v->cells_ready) return;
    voronoi_boundary(v);
    // (the boundary rows are on the host now; whatever device work is waiting for a good moment -- the source-side half of a
    // barycentric construction -- goes out here, and runs while the host builds the boundary cells below)
    flush_pending_points();
    VoronoiBoundaryIn in;
    in.n_face = v->n_face;
    in.nb = (int64_t)v->b_nodes.size();
    in.ne = (int64_t)v->edge_face.size();
    in.nodes = v->b_nodes.data();
    in.row_ptr = v->b_ptr.data();
    in.faces = v->b_faces.data();
    in.face_xy = v->b_face_xy.data();
    in.node_xy = v->b_node_xy.data();
    in.edge_lo = v->edge_lo.data();
    in.edge_hi = v->edge_hi.data();
    in.edge_face = v->edge_face.data();
    in.edge_face_xy = v->b_edge_face_xy.data();
    in.add_vertices = v->add_vertices;
    in.skip_concave = v->skip_concave;
    VoronoiBoundaryOut out;
    const int status = xr::voronoi_boundary_cells(in, out);
    XR_REQUIRE(status != VORONOI_BOUNDARY_ID_RANGE, XR_ERR_LIMIT, "voronoi: vertex ids exceed the int32 range");
    XR_REQUIRE(status != VORONOI_BOUNDARY_CELL_CORNERS, XR_ERR_LIMIT, "voronoi: a boundary cell has %lld corners", (long long)out.m);
    if (option(OPT_DEBUG) & 4)
        fprintf(stderr, "[voronoi] records %lld: set-up %.3f, sort %.3f, cells + convexity %.3f ms\n", (long long)out.n_record,
                out.ms_setup, out.ms_sort, out.ms_cells);
    v->c_extra_xy = std::move(out.extra_xy);
    v->c_cells = std::move(out.cells);
    v->c_n_cell = out.n_cell;
    v->c_m = out.m;
    v->c_tail = std::move(out.tail);
    v->c_interp = std::move(out.interp);
    v->cells_ready = true;
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_voronoi_create(xr_mesh *mesh, xr_voronoi **out) { return xr_voronoi_create_flags(mesh, 1, 1, 1, nullptr, out); }

int xr_voronoi_create_flags(xr_mesh *mesh, int add_exterior, int add_vertices, int skip_concave, const double *generators_dev,
                            xr_voronoi **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out, XR_ERR_INVALID, "xr_voronoi_create: NULL argument");
    Building<xr_voronoi> v(generators_dev ? OnFailure::WaitFirst : OnFailure::FreeOnly);
    v->add_exterior = add_exterior != 0; v->add_vertices = add_vertices != 0; v->skip_concave = skip_concave != 0;
    const int64_t N = mesh->n_node, F = mesh->n_face;
    const int m = mesh->m;
    const int64_t total = F * m;
    v->mesh = mesh; v->n_node = N; v->n_face = F;
    DevBuf<int32_t> count_cursor(2 * ((size_t)N + 1)); // (histogram and scatter cursors: one buffer, one fill)
    int32_t *const count = count_cursor.get(), *const cursor = count_cursor.get() + N + 1;
    v->indptr.alloc((size_t)N + 1);
    fill_i32(count_cursor.get(), 0, 2 * (N + 1));
    if (total > 0)
        XR_LAUNCH("vor_count", k_vor_count, dim3(div_up(total, VOR_SLOTS)), dim3(256), 0, mesh->faces_raw.get(), total, count);
    exclusive_scan_i32(count, v->indptr.get(), N);
    // (sized by the slot count, an upper bound of the entries: their number is read at the end with the other counters --
    // the whole construction has TWO host round trips, counters and exterior edges, instead of seven)
    v->faces_asc.alloc((size_t)std::max<int64_t>(total, 1));
    v->faces_ccw.alloc((size_t)std::max<int64_t>(total, 1));
    v->interior.alloc((size_t)N);
    v->cell_rank.alloc((size_t)N + 1);
    v->centroids.alloc((size_t)F * 2);
    DevBuf<uint8_t> on_boundary((size_t)N);
    DevBuf<int32_t> flag32((size_t)N), counters(8), e_all((size_t)std::max<int64_t>(3 * total, 1));
    XR_HIP(hipMemsetAsync(on_boundary.get(), 0, (size_t)(N > 0 ? N : 1), launch_stream()));
    // counters: [0] exterior edges, [1] min / [2] max interior degree, [3] interior nodes, [4] entries of the node -> face rows
    XR_LAUNCH("vor_init", k_vor_init_counters, dim3(1), dim3(64), 0, counters.get());
    if (total > 0) {
        XR_LAUNCH("vor_scatter", k_vor_scatter, dim3(div_up(total, VOR_SLOTS)), dim3(256), 0, mesh->faces_raw.get(), total, m,
                  v->indptr.get(), cursor, v->faces_asc.get());
        XR_LAUNCH("vor_sort_rows", k_vor_sort_rows, dim3(div_up(N, 256)), dim3(256), 0, v->indptr.get(), N,
                  v->faces_asc.get());
        if (v->add_exterior) // (without it no cell is closed along the boundary: nothing reads the exterior edges)
            XR_LAUNCH("vor_exterior", k_vor_exterior, dim3(div_up(total, 256)), dim3(256), 0, mesh->faces_raw.get(), F, m,
                      v->indptr.get(), v->faces_asc.get(), on_boundary.get(), counters.get(), e_all.get());
    }
    if (generators_dev) {
        if (F > 0)
            XR_HIP(hipMemcpyAsync(v->centroids.get(), generators_dev, sizeof(double) * 2 * (size_t)F, hipMemcpyDeviceToDevice,
                                  launch_stream()));
    } else {
        mesh_centroids_dev(mesh, v->centroids.get());
    }
    if (N > 0)
        XR_LAUNCH("vor_interior", k_vor_interior, dim3(div_up(N, VOR_BLOCK)), dim3(VOR_BLOCK), 0, mesh->node_xy.get(),
                  v->centroids.get(), v->indptr.get(), v->faces_asc.get(), on_boundary.get(), N, v->faces_ccw.get(),
                  v->interior.get(), flag32.get(), counters.get() + 1, v->add_exterior ? 0 : 1);
    exclusive_scan_i32(flag32.get(), v->cell_rank.get(), N);
    XR_LAUNCH("vor_totals", k_vor_totals, dim3(1), dim3(64), 0, v->cell_rank.get() + N, v->indptr.get() + N, counters.get());
    // (every kernel of the O(n) part is enqueued; from here on the host reads counters and lists back -- the device idles for
    // most of the next 0.2-0.3 ms.  A pending source-side locate pass of a barycentric construction goes out here.)
    flush_pending_points();
    int32_t h[8];
    d2h(h, counters.get(), sizeof(h));
    v->n_interior = h[3];
    v->nnz = h[4];
    v->min_degree = v->n_interior > 0 ? h[1] : 0;
    v->max_degree = h[2];
    const int64_t ne = h[0];
    std::vector<int32_t> lo((size_t)ne), hi((size_t)ne), fc((size_t)ne);
    if (ne > 0) {
        std::vector<int32_t> all((size_t)(3 * ne));
        d2h(all.data(), e_all.get(), sizeof(int32_t) * all.size());
        for (int64_t i = 0; i < ne; i++) {
            lo[(size_t)i] = all[3 * (size_t)i];
            hi[(size_t)i] = all[3 * (size_t)i + 1];
            fc[(size_t)i] = all[3 * (size_t)i + 2];
        }
    }
    std::vector<int64_t> order((size_t)ne);
    for (int64_t i = 0; i < ne; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        if (lo[(size_t)a] != lo[(size_t)b]) return lo[(size_t)a] < lo[(size_t)b];
        if (hi[(size_t)a] != hi[(size_t)b]) return hi[(size_t)a] < hi[(size_t)b];
        return fc[(size_t)a] < fc[(size_t)b];
    });
    v->edge_lo.resize((size_t)ne); v->edge_hi.resize((size_t)ne); v->edge_face.resize((size_t)ne);
    for (int64_t i = 0; i < ne; i++) {
        v->edge_lo[(size_t)i] = lo[(size_t)order[(size_t)i]];
        v->edge_hi[(size_t)i] = hi[(size_t)order[(size_t)i]];
        v->edge_face[(size_t)i] = fc[(size_t)order[(size_t)i]];
    }
    if (!v->add_exterior) {
        XR_REQUIRE(v->n_interior > 0, XR_ERR_INVALID, "voronoi: no node is shared by at least three faces, nothing to tessellate");
        DevBuf<int32_t> used((size_t)F), max_used(1);
        v->vertex_rank.alloc((size_t)F + 1);
        XR_LAUNCH("vor_used", k_vor_used, dim3(div_up(F, 256)), dim3(256), 0, mesh->faces_raw.get(), F, m, v->indptr.get(), used.get());
        exclusive_scan_i32(used.get(), v->vertex_rank.get(), F);
        DevBuf<double> packed((size_t)F * 2);
        fill_i32(max_used.get(), -1, 1);
        XR_LAUNCH("vor_compact", k_vor_compact, dim3(div_up(F, 256)), dim3(256), 0, v->centroids.get(), v->vertex_rank.get(), F,
                  packed.get(), max_used.get());
        v->n_used = read_scalar(v->vertex_rank.get() + F);
        v->max_used = read_scalar(max_used.get());
        v->centroids = std::move(packed); // (the first n_used entries: the vertices of the tessellation)
    }
    *out = v.release();
    XR_API_END
}

int xr_voronoi_vertex_info(const xr_voronoi *v, int64_t *n_generator_vertex, int64_t *max_used_face) {
    XR_API_BEGIN
    XR_REQUIRE(v && n_generator_vertex && max_used_face, XR_ERR_INVALID, "xr_voronoi_vertex_info: NULL argument");
    *n_generator_vertex = v->add_exterior ? v->n_face : v->n_used;
    *max_used_face = v->add_exterior ? v->n_face - 1 : v->max_used;
    XR_API_END
}

int xr_voronoi_info(const xr_voronoi *v, int64_t *n_node, int64_t *nnz, int64_t *n_exterior_edge, int64_t *n_interior_cell,
                    int64_t *max_interior_degree) {
    XR_API_BEGIN
    XR_REQUIRE(v, XR_ERR_INVALID, "xr_voronoi_info: NULL handle");
    if (n_node) *n_node = v->n_node;
    if (nnz) *nnz = v->nnz;
    if (n_exterior_edge) *n_exterior_edge = (int64_t)v->edge_lo.size();
    if (n_interior_cell) *n_interior_cell = v->n_interior;
    if (max_interior_degree) *max_interior_degree = v->max_degree;
    XR_API_END
}

int xr_voronoi_download(const xr_voronoi *v, int64_t *indptr, int64_t *indices, int64_t *edge_nodes, int64_t *edge_face,
                        double *centroids) {
    XR_API_BEGIN
    XR_REQUIRE(v && indptr && (v->nnz == 0 || indices), XR_ERR_INVALID, "xr_voronoi_download: NULL argument");
    XR_REQUIRE(v->add_exterior || !centroids, XR_ERR_INVALID,
               "xr_voronoi_download: a handle built without exterior keeps only the generator points its cells use");
    {
        DevBuf<int64_t> wide((size_t)std::max<int64_t>(v->n_node + 1, v->nnz));
        download_wide(v->indptr.get(), v->n_node + 1, indptr, wide);
        download_wide(v->faces_asc.get(), v->nnz, indices, wide);
    }
    const size_t ne = v->edge_lo.size();
    XR_REQUIRE(ne == 0 || (edge_nodes && edge_face), XR_ERR_INVALID, "xr_voronoi_download: NULL edge arrays");
    for (size_t i = 0; i < ne; i++) {
        edge_nodes[2 * i] = v->edge_lo[i];
        edge_nodes[2 * i + 1] = v->edge_hi[i];
        edge_face[i] = v->edge_face[i];
    }
    if (centroids && v->n_face > 0) d2h(centroids, v->centroids.get(), sizeof(double) * 2 * (size_t)v->n_face);
    XR_API_END
}

int xr_voronoi_boundary_info(xr_voronoi *v, int64_t *n_boundary_node, int64_t *n_boundary_entry) {
    XR_API_BEGIN
    XR_REQUIRE(v && n_boundary_node && n_boundary_entry, XR_ERR_INVALID, "xr_voronoi_boundary_info: NULL argument");
    voronoi_boundary(v);
    *n_boundary_node = (int64_t)v->b_nodes.size();
    *n_boundary_entry = (int64_t)v->b_faces.size();
    XR_API_END
}

int xr_voronoi_boundary(xr_voronoi *v, int64_t *nodes, int64_t *row_ptr, int64_t *faces, double *face_xy,
                        int64_t *edge_nodes, int64_t *edge_face, double *edge_face_xy) {
    XR_API_BEGIN
    XR_REQUIRE(v && row_ptr, XR_ERR_INVALID, "xr_voronoi_boundary: NULL argument");
    voronoi_boundary(v);
    const size_t nb = v->b_nodes.size(), nf = v->b_faces.size(), ne = v->edge_face.size();
    XR_REQUIRE((nb == 0 || nodes) && (nf == 0 || (faces && face_xy)) && (ne == 0 || (edge_nodes && edge_face && edge_face_xy)),
               XR_ERR_INVALID, "xr_voronoi_boundary: NULL output array");
    if (nb) memcpy(nodes, v->b_nodes.data(), sizeof(int64_t) * nb);
    memcpy(row_ptr, v->b_ptr.data(), sizeof(int64_t) * (nb + 1));
    if (nf) {
        memcpy(faces, v->b_faces.data(), sizeof(int64_t) * nf);
        memcpy(face_xy, v->b_face_xy.data(), sizeof(double) * 2 * nf);
    }
    for (size_t i = 0; i < ne; i++) {
        edge_nodes[2 * i] = v->edge_lo[i];
        edge_nodes[2 * i + 1] = v->edge_hi[i];
        edge_face[i] = v->edge_face[i];
    }
    if (ne) memcpy(edge_face_xy, v->b_edge_face_xy.data(), sizeof(double) * 2 * ne);
    XR_API_END
}

int xr_voronoi_mesh(const xr_voronoi *v, const double *extra_xy, int64_t n_extra_vertex, const int64_t *boundary_cells,
                    int64_t n_boundary_cell, int64_t n_max_boundary, xr_mesh **out) {
    XR_API_BEGIN
    XR_REQUIRE(v && out, XR_ERR_INVALID, "xr_voronoi_mesh: NULL argument");
    XR_REQUIRE(n_extra_vertex >= 0 && n_boundary_cell >= 0 && n_max_boundary >= 0, XR_ERR_INVALID,
               "xr_voronoi_mesh: negative sizes");
    XR_REQUIRE((n_extra_vertex == 0 || extra_xy) && (n_boundary_cell == 0 || boundary_cells), XR_ERR_INVALID,
               "xr_voronoi_mesh: NULL arrays");
    XR_REQUIRE(v->n_interior == 0 || v->min_degree >= 3, XR_ERR_INVALID,
               "xr_voronoi_mesh: an interior node is surrounded by only %d faces (non-manifold mesh)", v->min_degree);
    const int64_t n_generator = v->add_exterior ? v->n_face : v->n_used; // (without the exterior: the points some cell uses)
    XR_REQUIRE(v->add_exterior || (n_extra_vertex == 0 && n_boundary_cell == 0), XR_ERR_INVALID,
               "xr_voronoi_mesh: a tessellation without exterior has no boundary cells");
    const int64_t n_vertex = n_generator + n_extra_vertex;
    const int64_t n_cell = v->n_interior + n_boundary_cell;
    const int64_t m64 = std::max<int64_t>(std::max<int64_t>(v->max_degree, n_boundary_cell > 0 ? n_max_boundary : 0), 3);
    XR_REQUIRE(m64 <= XR_MAX_FACE_NODES, XR_ERR_LIMIT, "xr_voronoi_mesh: a Voronoi cell has %lld corners (limit %d)",
               (long long)m64, XR_MAX_FACE_NODES);
    XR_REQUIRE(n_vertex < ((int64_t)1 << 31) && n_cell * m64 < ((int64_t)1 << 31), XR_ERR_LIMIT,
               "xr_voronoi_mesh: mesh exceeds the int32 index range");
    const int m = (int)m64;
    const int mb = (int)n_max_boundary;
    XR_REQUIRE(n_boundary_cell == 0 || mb >= 3, XR_ERR_INVALID, "xr_voronoi_mesh: every boundary cell has fewer than 3 corners (n_max_boundary = %d)", mb);
    std::vector<int32_t> table((size_t)(n_boundary_cell * mb) + 1);
    for (int64_t r = 0; r < n_boundary_cell; r++) {
        for (int j = 0; j < mb; j++) {
            const int64_t c = boundary_cells[r * mb + j];
            XR_REQUIRE(c >= -1 && c < n_vertex, XR_ERR_INVALID, "xr_voronoi_mesh: boundary cell %lld references vertex %lld",
                       (long long)r, (long long)c);
            XR_REQUIRE(c >= 0 || j >= 3, XR_ERR_INVALID, "xr_voronoi_mesh: boundary cell %lld has fewer than 3 corners",
                       (long long)r);
            table[(size_t)(r * mb + j)] = (int32_t)c;
        }
    }
    Building<xr_mesh> mesh = new_raw_mesh(n_vertex, n_cell, m);
    if (n_generator > 0)
        XR_HIP(hipMemcpyAsync(mesh->node_xy.get(), v->centroids.get(), sizeof(double) * 2 * (size_t)n_generator,
                              hipMemcpyDeviceToDevice, launch_stream()));
    if (n_extra_vertex > 0)
        h2d(mesh->node_xy.get() + 2 * n_generator, extra_xy, sizeof(double) * 2 * (size_t)n_extra_vertex);
    if (v->n_node > 0 && v->n_interior > 0)
        XR_LAUNCH("vor_cells", k_vor_cells, dim3(div_up(v->n_node * m, 256)), dim3(256), 0, v->indptr.get(),
                  v->faces_ccw.get(), v->interior.get(), v->cell_rank.get(), v->n_node, m, mesh->faces_raw.get(),
                  v->add_exterior ? (const int32_t *)nullptr : v->vertex_rank.get());
    if (n_boundary_cell > 0) {
        DevBuf<int32_t> dtable((size_t)(n_boundary_cell * mb));
        h2d(dtable.get(), table.data(), sizeof(int32_t) * (size_t)(n_boundary_cell * mb));
        XR_LAUNCH("vor_boundary_cells", k_vor_boundary_cells, dim3(div_up(n_boundary_cell * m, 256)), dim3(256), 0,
                  dtable.get(), n_boundary_cell, mb, m, mesh->faces_raw.get() + v->n_interior * m);
        stream_sync();
    }
    stream_sync();
    *out = mesh.release();
    XR_API_END
}

/* The whole pre-step without a host language in between: the cells of the boundary nodes are computed by the library
 * (voronoi_boundary_cells) and the tessellation is assembled on the device.  n_tail = vertices added behind the face
 * centroids, n_map = rows of the interpolation map; fetch them with xr_voronoi_tail. */
int xr_voronoi_mesh_auto(xr_voronoi *v, xr_mesh **out, int64_t *n_tail, int64_t *n_map) {
    XR_API_BEGIN
    XR_REQUIRE(v && out && n_tail && n_map, XR_ERR_INVALID, "xr_voronoi_mesh_auto: NULL argument");
    const bool dbg = (option(OPT_DEBUG) & 4) != 0;
    const auto t0 = std::chrono::steady_clock::now();
    voronoi_boundary(v);
    const auto t1 = std::chrono::steady_clock::now();
    voronoi_boundary_cells(v);
    const auto t2 = std::chrono::steady_clock::now();
    if (dbg)
        fprintf(stderr, "[voronoi] gather %.3f ms, boundary cells %.3f ms\n",
                std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
    *n_tail = (int64_t)v->c_tail.size();
    *n_map = (int64_t)v->c_interp.size() / 2;
    const int rc = xr_voronoi_mesh(v, v->c_extra_xy.data(), (int64_t)v->c_extra_xy.size() / 2, v->c_cells.data(), v->c_n_cell,
                                   v->c_m, out);
    if (rc != XR_OK) return rc;
    XR_API_END
}

int xr_voronoi_tail(xr_voronoi *v, int64_t *tail_face_index, int64_t *interpolation_map) {
    XR_API_BEGIN
    XR_REQUIRE(v, XR_ERR_INVALID, "xr_voronoi_tail: NULL argument");
    voronoi_boundary_cells(v);
    XR_REQUIRE((v->c_tail.empty() || tail_face_index) && (v->c_interp.empty() || interpolation_map), XR_ERR_INVALID,
               "xr_voronoi_tail: NULL output array");
    if (!v->c_tail.empty()) memcpy(tail_face_index, v->c_tail.data(), sizeof(int64_t) * v->c_tail.size());
    if (!v->c_interp.empty()) memcpy(interpolation_map, v->c_interp.data(), sizeof(int64_t) * v->c_interp.size());
    XR_API_END
}

/* the boundary cells themselves (tests, hosts that assemble on their own): sizes, then the arrays */
int xr_voronoi_boundary_cells_info(xr_voronoi *v, int64_t *n_extra_vertex, int64_t *n_cell, int64_t *n_max) {
    XR_API_BEGIN
    XR_REQUIRE(v && n_extra_vertex && n_cell && n_max, XR_ERR_INVALID, "xr_voronoi_boundary_cells_info: NULL argument");
    voronoi_boundary_cells(v);
    *n_extra_vertex = (int64_t)v->c_extra_xy.size() / 2;
    *n_cell = v->c_n_cell;
    *n_max = v->c_m;
    XR_API_END
}

int xr_voronoi_boundary_cells(xr_voronoi *v, double *extra_xy, int64_t *cells) {
    XR_API_BEGIN
    XR_REQUIRE(v, XR_ERR_INVALID, "xr_voronoi_boundary_cells: NULL argument");
    voronoi_boundary_cells(v);
    XR_REQUIRE((v->c_extra_xy.empty() || extra_xy) && (v->c_cells.empty() || cells), XR_ERR_INVALID,
               "xr_voronoi_boundary_cells: NULL output array");
    if (!v->c_extra_xy.empty()) memcpy(extra_xy, v->c_extra_xy.data(), sizeof(double) * v->c_extra_xy.size());
    if (!v->c_cells.empty()) memcpy(cells, v->c_cells.data(), sizeof(int64_t) * v->c_cells.size());
    XR_API_END
}

int xr_voronoi_destroy(xr_voronoi *v) {
    XR_API_BEGIN
    if (v) {
        stream_sync();
        delete v;
    }
    XR_API_END
}

} // extern "C"
