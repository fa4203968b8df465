// xr_topology.hip -- the edge topology of a device mesh, built where the mesh is: what xugrid_amd/connectivity.py derives on
// the host (edge_connectivity: np.unique over every half-edge key + a stable argsort per row; invert_dense; coo -> csr for the
// two adjacencies) without a global sort and without an O(n) array crossing PCIe.
//
// Route:
//   1. node -> faces CSR by the counting sort of xr_node_faces.h (shared with xr_voronoi.hip), rows ascending.
//   2. per node the sorted list of its DISTINCT ring neighbours, gathered from the faces around it.  That list IS the node's row
//      of node_node_connectivity; its entries above the node are the edges the node owns (an undirected edge belongs to its lower
//      node).  One thread per node keeps the list in its LDS column; a node whose list outgrows the column (TOPO_CAP entries) is
//      handed to a wave-per-node kernel that rank-sorts in global scratch -- nothing is ever truncated.
//   3. exclusive scans of the two per-node counts give the row pointers of node_node and, directly, the lexicographic edge ids:
//      id(lo, hi) = edge_start[lo] + rank of hi among lo's higher neighbours.  A half-edge finds its id by a binary search in its
//      owner's stretch of edge_node.
//   4. edge -> faces: one thread per edge walks the (ascending) faces around its lower node, so the two faces come out ascending
//      and an edge with a third face is detected, with no atomic per slot (see the note on device-scope atomics in
//      xr_node_faces.h); the only atomics are one per overflowing node, one per wave for the exterior count and one per
//      non-manifold edge.
//   5. face -> face rows: count the distinct neighbours per face, scan, fill + insertion sort of the (<= m) entries.
#include <algorithm>
#include <vector>

#include "xr_node_faces.h"
#include "xr_prims.h"
#include "xr_topology.h"

namespace xr {

static constexpr int TB = 128;       // threads per block of the per-node kernel (one LDS column each)
static constexpr int TOPO_CAP = 16;  // distinct neighbours a thread's column holds (a Delaunay node has ~6)
static constexpr int TOPO_LONG_BLOCKS = 256; // waves that walk the list of overflowing nodes
enum TopoCounter : int { TC_LONG = 0, TC_NONMANIFOLD = 1, TC_EXTERIOR = 2, TC_COUNT = 4 };

// real nodes of a face: the fill (-1) trails
__device__ __forceinline__ int topo_face_len(const int32_t *__restrict__ face, int m) {
    int n = 0;
    while (n < m && face[n] >= 0) n++;
    return n;
}

// ring neighbours of the occ-th occurrence of node v in a face: predecessor p and successor q, -1 where that is v itself (a slot
// whose two nodes are equal is no edge) or where v does not occur that often
__device__ __forceinline__ void topo_ring_nbrs(const int32_t *__restrict__ face, int m, int v, int occ, int &p, int &q) {
    p = q = -1;
    const int L = topo_face_len(face, m);
    for (int k = 0; k < L; k++) {
        if (face[k] != v) continue;
        if (occ-- > 0) continue;
        const int a = face[k == 0 ? L - 1 : k - 1], b = face[k + 1 == L ? 0 : k + 1];
        p = a == v ? -1 : a;
        q = b == v ? -1 : b;
        return;
    }
}

// which occurrence of its face a row entry stands for (rows ascending: equal faces are adjacent)
__device__ __forceinline__ int topo_occurrence(const int32_t *__restrict__ rows, int s, int r) {
    int occ = 0;
    for (int j = r - 1; j >= s && rows[j] == rows[r]; j--) occ++;
    return occ;
}

// 2: one thread per node.  nbr[2 * nf_ptr[v] ..] receives the sorted distinct neighbours (a node of d face incidences has at
// most 2 d of them), n_all / n_high their number and how many lie above v.
__global__ void __launch_bounds__(TB)
k_topo_nbrs(const int32_t *__restrict__ faces, int m, const int32_t *__restrict__ nf_ptr, const int32_t *__restrict__ nf_rows,
            int64_t n_node, int32_t *__restrict__ nbr, int32_t *__restrict__ n_all, int32_t *__restrict__ n_high,
            int32_t *__restrict__ long_nodes, int32_t *__restrict__ counters) {
    __shared__ int32_t sh[TOPO_CAP][TB];
    const int t = threadIdx.x;
    const int64_t v = (int64_t)blockIdx.x * TB + t;
    if (v >= n_node) return;
    const int s = nf_ptr[v], e = nf_ptr[v + 1];
    int cnt = 0;
    bool over = false;
    for (int r = s; r < e && !over; r++) {
        int c[2];
        topo_ring_nbrs(faces + (int64_t)nf_rows[r] * m, m, (int)v, topo_occurrence(nf_rows, s, r), c[0], c[1]);
        for (int u = 0; u < 2; u++) {
            if (c[u] < 0) continue;
            int j = 0;
            while (j < cnt && sh[j][t] < c[u]) j++;
            if (j < cnt && sh[j][t] == c[u]) continue;
            if (cnt == TOPO_CAP) {
                over = true;
                break;
            }
            for (int i = cnt; i > j; i--) sh[i][t] = sh[i - 1][t];
            sh[j][t] = c[u];
            cnt++;
        }
    }
    if (over) { // (rare: one atomic per such node)
        long_nodes[atomicAdd(&counters[TC_LONG], 1)] = (int32_t)v;
        return;
    }
    int high = 0;
    for (int i = 0; i < cnt; i++) {
        const int x = sh[i][t];
        nbr[2 * (int64_t)s + i] = x;
        high += x > (int)v;
    }
    n_all[v] = cnt;
    n_high[v] = high;
}

// 2, nodes of high degree: one wave per node, any degree.  cand[4 * nf_ptr[v] ..]: the 2 d candidates, behind them the same with
// every repeat replaced by -1; the rank of a kept value among the kept values is its place in the sorted list.  O(d^2 / 64).
// (scratch pointers are not __restrict__: lanes read what other lanes of the wave wrote before the barrier)
__global__ void __launch_bounds__(64)
k_topo_nbrs_long(const int32_t *__restrict__ faces, int m, const int32_t *__restrict__ nf_ptr, const int32_t *__restrict__ nf_rows,
                 const int32_t *__restrict__ long_nodes, const int32_t *__restrict__ counters, int32_t *cand, int32_t *nbr,
                 int32_t *__restrict__ n_all, int32_t *__restrict__ n_high) {
    const int lane = threadIdx.x;
    const int n_long = counters[TC_LONG];
    for (int i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int v = long_nodes[i];
        const int s = nf_ptr[v], d = nf_ptr[v + 1] - s;
        int32_t *c0 = cand + 4 * (int64_t)s, *c1 = c0 + 2 * (int64_t)d, *out = nbr + 2 * (int64_t)s;
        for (int r = lane; r < d; r += 64) {
            int p, q;
            topo_ring_nbrs(faces + (int64_t)nf_rows[s + r] * m, m, v, topo_occurrence(nf_rows, s, s + r), p, q);
            c0[2 * r] = p;
            c0[2 * r + 1] = q;
        }
        __syncthreads();
        for (int a = lane; a < 2 * d; a += 64) {
            const int c = c0[a];
            bool first = c >= 0;
            for (int b = 0; b < a && first; b++) first = c0[b] != c;
            c1[a] = first ? c : -1;
        }
        __syncthreads();
        int cnt = 0, high = 0;
        for (int a = lane; a < 2 * d; a += 64) {
            const int c = c1[a];
            if (c < 0) continue;
            int rank = 0;
            for (int b = 0; b < 2 * d; b++) {
                const int x = c1[b];
                rank += x >= 0 && x < c;
            }
            out[rank] = c;
            cnt++;
            high += c > v;
        }
        cnt = wave_reduce<OpSum>(cnt), high = wave_reduce<OpSum>(high);
        if (lane == 0) {
            n_all[v] = cnt;
            n_high[v] = high;
        }
    }
}

// first index in [lo, hi) of the ascending `a` (stride `stride`, offset `off`) whose value is >= key
__device__ __forceinline__ int topo_lower_bound(const int32_t *__restrict__ a, int stride, int off, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[(int64_t)mid * stride + off] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 3: the node's row of node_node (columns = its neighbour list, data = the edge id) and the edges it owns
__global__ void __launch_bounds__(256)
k_topo_node_rows(const int32_t *__restrict__ nf_ptr, const int32_t *__restrict__ nbr, const int32_t *__restrict__ n_all,
                 const int32_t *__restrict__ n_high, const int32_t *__restrict__ nn_ptr, const int32_t *__restrict__ edge_start,
                 int64_t n_node, int32_t *__restrict__ nn_idx, int32_t *__restrict__ nn_dat, int32_t *__restrict__ edge_node) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_node) return;
    const int64_t s2 = 2 * (int64_t)nf_ptr[v];
    const int cnt = n_all[v], low = cnt - n_high[v], base = nn_ptr[v], es = edge_start[v];
    for (int i = 0; i < cnt; i++) {
        const int u = nbr[s2 + i];
        int id;
        if (i >= low) {
            id = es + (i - low);
            edge_node[2 * (int64_t)id] = (int32_t)v;
            edge_node[2 * (int64_t)id + 1] = u;
        } else { // the edge belongs to u: v's rank among u's higher neighbours
            const int64_t su = 2 * (int64_t)nf_ptr[u];
            const int cu = n_all[u], hu = n_high[u];
            const int pos = topo_lower_bound(nbr + su, 1, 0, cu - hu, cu, (int)v);
            id = pos < cu && nbr[su + pos] == (int)v ? edge_start[u] + (pos - (cu - hu)) : -1;
        }
        nn_idx[base + i] = u;
        nn_dat[base + i] = id;
    }
}

// id of the edge (lo, hi), lo < hi: hi's place in lo's stretch of edge_node
__device__ __forceinline__ int topo_edge_id(const int32_t *__restrict__ edge_node, const int32_t *__restrict__ edge_start, int lo, int hi) {
    const int e0 = edge_start[lo], e1 = edge_start[lo + 1];
    const int pos = topo_lower_bound(edge_node, 2, 1, e0, e1, hi);
    return pos < e1 && edge_node[2 * (int64_t)pos + 1] == hi ? pos : -1;
}

// 4: one thread per edge: every slot of the faces around the lower node that is this edge, faces ascending
__global__ void __launch_bounds__(256)
k_topo_edge_face(const int32_t *__restrict__ faces, int m, const int32_t *__restrict__ nf_ptr, const int32_t *__restrict__ nf_rows,
                 const int32_t *__restrict__ edge_node, int64_t n_edge, int32_t *__restrict__ edge_face,
                 uint8_t *__restrict__ exterior_edge, int32_t *__restrict__ counters) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool exterior = false;
    if (e < n_edge) {
        const int lo = edge_node[2 * e], hi = edge_node[2 * e + 1];
        const int s = nf_ptr[lo], end = nf_ptr[lo + 1];
        int cnt = 0;
        for (int r = s; r < end; r++) {
            const int f = nf_rows[r];
            int p, q;
            topo_ring_nbrs(faces + (int64_t)f * m, m, lo, topo_occurrence(nf_rows, s, r), p, q);
            for (int u = 0; u < 2; u++)
                if ((u ? q : p) == hi) {
                    if (cnt < 2) edge_face[2 * e + cnt] = f;
                    cnt++;
                }
        }
        if (cnt < 2) edge_face[2 * e + 1] = -1;
        if (cnt < 1) edge_face[2 * e] = -1; // (cannot happen: an edge comes from a slot)
        exterior = cnt == 1;
        exterior_edge[e] = exterior;
        if (cnt > 2) atomicAdd(&counters[TC_NONMANIFOLD], 1);
    }
    const unsigned long long ballot = __ballot(exterior);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&counters[TC_EXTERIOR], __popcll(ballot));
}

// one thread per slot (f, k): the edge of node k and its successor, written at the slot's rank among the face's valid slots
// (face_edge was filled with -1)
__global__ void __launch_bounds__(256)
k_topo_face_edge(const int32_t *__restrict__ faces, int64_t n_face, int m, const int32_t *__restrict__ edge_node,
                 const int32_t *__restrict__ edge_start, int32_t *__restrict__ face_edge) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_face * m) return;
    const int64_t f = i / m;
    const int k = (int)(i - f * m);
    const int32_t *face = faces + f * m;
    const int L = topo_face_len(face, m);
    if (k >= L) return;
    const int a = face[k], b = face[k + 1 == L ? 0 : k + 1];
    if (a == b) return;
    int rank = 0;
    for (int j = 0; j < k; j++) rank += face[j] != face[j + 1]; // (j + 1 <= k < L: never the closing slot)
    face_edge[f * m + rank] = topo_edge_id(edge_node, edge_start, min(a, b), max(a, b));
}

// the face across slot j of face f and the edge between them; -1: no such slot, or an exterior edge
__device__ __forceinline__ int topo_across(const int32_t *__restrict__ face_edge, const int32_t *__restrict__ edge_face, int64_t f,
                                           int m, int j, int &e) {
    e = face_edge[f * m + j];
    if (e < 0) return -1;
    const int a = edge_face[2 * (int64_t)e], b = edge_face[2 * (int64_t)e + 1];
    if (b < 0) return -1;
    return a == (int)f ? b : a;
}

// 5a: distinct neighbours per face; the face is exterior if one of its edges is
__global__ void __launch_bounds__(256)
k_topo_ff_count(const int32_t *__restrict__ face_edge, const int32_t *__restrict__ edge_face, int64_t n_face, int m,
                int32_t *__restrict__ count, uint8_t *__restrict__ exterior_face) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int cnt = 0;
    bool exterior = false;
    for (int j = 0; j < m; j++) {
        int e, e2;
        const int g = topo_across(face_edge, edge_face, f, m, j, e);
        if (e < 0) break; // (compacted to the left)
        if (g < 0) {
            exterior = true;
            continue;
        }
        bool first = true;
        for (int i = 0; i < j && first; i++) first = topo_across(face_edge, edge_face, f, m, i, e2) != g;
        cnt += first;
    }
    count[f] = cnt;
    exterior_face[f] = exterior;
}

// 5b: the row, columns ascending; faces that share several edges: one entry, the edge ids summed
__global__ void __launch_bounds__(256)
k_topo_ff_fill(const int32_t *__restrict__ face_edge, const int32_t *__restrict__ edge_face, int64_t n_face, int m,
               const int32_t *__restrict__ ff_ptr, int32_t *__restrict__ ff_idx, int32_t *__restrict__ ff_dat) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const int base = ff_ptr[f];
    int cnt = 0;
    for (int j = 0; j < m; j++) {
        int e, e2;
        const int g = topo_across(face_edge, edge_face, f, m, j, e);
        if (e < 0) break;
        if (g < 0) continue;
        bool first = true;
        for (int i = 0; i < j && first; i++) first = topo_across(face_edge, edge_face, f, m, i, e2) != g;
        if (!first) continue;
        int sum = e;
        for (int i = j + 1; i < m; i++)
            if (topo_across(face_edge, edge_face, f, m, i, e2) == g) sum += e2;
        int p = base + cnt;
        while (p > base && ff_idx[p - 1] > g) {
            ff_idx[p] = ff_idx[p - 1];
            ff_dat[p] = ff_dat[p - 1];
            p--;
        }
        ff_idx[p] = g;
        ff_dat[p] = sum;
        cnt++;
    }
}

__global__ void __launch_bounds__(256)
k_topo_edge_xy(const double *__restrict__ node_xy, const int32_t *__restrict__ edge_node, int64_t n_edge, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; // one thread per coordinate
    if (i >= 2 * n_edge) return;
    const int64_t e = i >> 1;
    const int c = (int)(i & 1);
    out[i] = 0.5 * (node_xy[2 * (int64_t)edge_node[2 * e] + c] + node_xy[2 * (int64_t)edge_node[2 * e + 1] + c]);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_topology_create(xr_mesh *mesh, xr_topology **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out, XR_ERR_INVALID, "xr_topology_create: NULL argument");
    const int64_t N = mesh->n_node, F = mesh->n_face;
    const int m = mesh->m;
    const int64_t total = F * m;
    // (scratch of 4 entries per slot is indexed with int32 row pointers times four in 64 bits; the sums of two edge ids and
    // every id stay below 2^31)
    XR_REQUIRE(total < ((int64_t)1 << 29) && N < INT32_MAX, XR_ERR_LIMIT, "xr_topology_create: more than 2^29 face slots");
    Building<xr_topology> t;
    t->mesh = mesh, t->n_node = N, t->n_face = F, t->m = m;
    const int32_t *faces = mesh->faces_raw.get();

    // 1: node -> faces
    // (kept in the handle: node -> face is a table of its own for the facet mapping, xr_facet.hip)
    DevBuf<int32_t> count_cursor(2 * ((size_t)N + 1));
    DevBuf<int32_t> &nf_ptr = t->nf_ptr, &nf_rows = t->nf_idx;
    nf_ptr.alloc((size_t)N + 1), nf_rows.alloc((size_t)std::max<int64_t>(total, 1));
    int32_t *const count = count_cursor.get(), *const cursor = count_cursor.get() + N + 1;
    fill_i32(count_cursor.get(), 0, 2 * (N + 1));
    if (total > 0) XR_LAUNCH("vor_count", k_vor_count, dim3(div_up(total, VOR_SLOTS)), dim3(256), 0, faces, total, count);
    exclusive_scan_i32(count, nf_ptr.get(), N);
    if (total > 0) {
        XR_LAUNCH("vor_scatter", k_vor_scatter, dim3(div_up(total, VOR_SLOTS)), dim3(256), 0, faces, total, m, nf_ptr.get(), cursor,
                  nf_rows.get());
        XR_LAUNCH("vor_sort_rows", k_vor_sort_rows, dim3(div_up(N, 256)), dim3(256), 0, nf_ptr.get(), N, nf_rows.get());
    }

    // 2: neighbour lists
    DevBuf<int32_t> nbr((size_t)std::max<int64_t>(2 * total, 1)), cand((size_t)std::max<int64_t>(4 * total, 1));
    DevBuf<int32_t> n_all((size_t)N + 1), n_high((size_t)N + 1), long_nodes((size_t)std::max<int64_t>(N, 1)), counters(TC_COUNT);
    fill_i32(counters.get(), 0, TC_COUNT);
    t->nn_ptr.alloc((size_t)N + 1);
    DevBuf<int32_t> edge_start((size_t)N + 1);
    if (N > 0) {
        XR_LAUNCH("topo_nbrs", k_topo_nbrs, dim3(div_up(N, TB)), dim3(TB), 0, faces, m, nf_ptr.get(), nf_rows.get(), N, nbr.get(),
                  n_all.get(), n_high.get(), long_nodes.get(), counters.get());
        XR_LAUNCH("topo_nbrs_long", k_topo_nbrs_long, dim3(TOPO_LONG_BLOCKS), dim3(64), 0, faces, m, nf_ptr.get(), nf_rows.get(),
                  long_nodes.get(), counters.get(), cand.get(), nbr.get(), n_all.get(), n_high.get());
    }
    // 3: row pointers and edge ids
    exclusive_scan_i32(n_all.get(), t->nn_ptr.get(), N);
    exclusive_scan_i32(n_high.get(), edge_start.get(), N);
    t->nn_nnz = read_scalar(t->nn_ptr.get() + N);
    const int64_t E = t->n_edge = read_scalar(edge_start.get() + N);
    t->edge_node.alloc((size_t)std::max<int64_t>(2 * E, 1));
    t->nn_idx.alloc((size_t)std::max<int64_t>(t->nn_nnz, 1));
    t->nn_dat.alloc((size_t)std::max<int64_t>(t->nn_nnz, 1));
    t->edge_face.alloc((size_t)std::max<int64_t>(2 * E, 1));
    t->exterior_edge.alloc((size_t)std::max<int64_t>(E, 1));
    if (N > 0)
        XR_LAUNCH("topo_node_rows", k_topo_node_rows, dim3(div_up(N, 256)), dim3(256), 0, nf_ptr.get(), nbr.get(), n_all.get(),
                  n_high.get(), t->nn_ptr.get(), edge_start.get(), N, t->nn_idx.get(), t->nn_dat.get(), t->edge_node.get());
    // 4: edge -> faces
    if (E > 0)
        XR_LAUNCH("topo_edge_face", k_topo_edge_face, dim3(div_up(E, 256)), dim3(256), 0, faces, m, nf_ptr.get(), nf_rows.get(),
                  t->edge_node.get(), E, t->edge_face.get(), t->exterior_edge.get(), counters.get());
    int32_t h[TC_COUNT];
    d2h(h, counters.get(), sizeof(h));
    t->n_long_nodes = h[TC_LONG], t->n_nonmanifold = h[TC_NONMANIFOLD], t->n_exterior = h[TC_EXTERIOR];
    if (t->n_nonmanifold > 0) { // two columns cannot hold such an edge: nothing is kept, the caller takes the host route
        t->edge_node.release(), t->edge_face.release(), t->exterior_edge.release();
        t->nn_ptr.release(), t->nn_idx.release(), t->nn_dat.release();
        t->nf_ptr.release(), t->nf_idx.release();
        t->nn_nnz = 0;
        stream_sync();
        *out = t.release();
        return XR_OK;
    }
    t->face_edge.alloc((size_t)std::max<int64_t>(total, 1));
    fill_i32(t->face_edge.get(), -1, total);
    if (total > 0)
        XR_LAUNCH("topo_face_edge", k_topo_face_edge, dim3(div_up(total, 256)), dim3(256), 0, faces, F, m, t->edge_node.get(),
                  edge_start.get(), t->face_edge.get());
    // 5: face -> face
    DevBuf<int32_t> ff_count((size_t)F + 1);
    t->ff_ptr.alloc((size_t)F + 1);
    t->exterior_face.alloc((size_t)std::max<int64_t>(F, 1));
    if (F > 0)
        XR_LAUNCH("topo_ff_count", k_topo_ff_count, dim3(div_up(F, 256)), dim3(256), 0, t->face_edge.get(), t->edge_face.get(), F, m,
                  ff_count.get(), t->exterior_face.get());
    exclusive_scan_i32(ff_count.get(), t->ff_ptr.get(), F);
    t->ff_nnz = read_scalar(t->ff_ptr.get() + F);
    t->ff_idx.alloc((size_t)std::max<int64_t>(t->ff_nnz, 1));
    t->ff_dat.alloc((size_t)std::max<int64_t>(t->ff_nnz, 1));
    if (F > 0)
        XR_LAUNCH("topo_ff_fill", k_topo_ff_fill, dim3(div_up(F, 256)), dim3(256), 0, t->face_edge.get(), t->edge_face.get(), F, m,
                  t->ff_ptr.get(), t->ff_idx.get(), t->ff_dat.get());
    stream_sync(); // (the scratch goes back to the pool behind its readers)
    *out = t.release();
    XR_API_END
}

int xr_topology_info(const xr_topology *t, int64_t *n_edge, int64_t *n_exterior_edge, int64_t *face_face_nnz,
                     int64_t *node_node_nnz, int64_t *n_nonmanifold) {
    XR_API_BEGIN
    XR_REQUIRE(t, XR_ERR_INVALID, "xr_topology_info: NULL handle");
    if (n_edge) *n_edge = t->n_edge;
    if (n_exterior_edge) *n_exterior_edge = t->n_exterior;
    if (face_face_nnz) *face_face_nnz = t->ff_nnz;
    if (node_node_nnz) *node_node_nnz = t->nn_nnz;
    if (n_nonmanifold) *n_nonmanifold = t->n_nonmanifold;
    XR_API_END
}

int xr_topology_long_nodes(const xr_topology *t, int64_t *n_long_nodes) {
    XR_API_BEGIN
    XR_REQUIRE(t && n_long_nodes, XR_ERR_INVALID, "xr_topology_long_nodes: NULL argument");
    *n_long_nodes = t->n_long_nodes;
    XR_API_END
}

int xr_topology_download(const xr_topology *t, int64_t *edge_node, int64_t *face_edge, int64_t *edge_face, int64_t *ff_indptr,
                         int64_t *ff_indices, int64_t *ff_data, int64_t *nn_indptr, int64_t *nn_indices, int64_t *nn_data,
                         int64_t *exterior_edge, int64_t *exterior_face) {
    XR_API_BEGIN
    XR_REQUIRE(t, XR_ERR_INVALID, "xr_topology_download: NULL handle");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_download: the mesh has %lld edges with more than two faces",
               (long long)t->n_nonmanifold);
    const int64_t E = t->n_edge, F = t->n_face, N = t->n_node;
    const int64_t longest = std::max({2 * E, F * t->m, F + 1, N + 1, t->ff_nnz, t->nn_nnz, (int64_t)1});
    DevBuf<int64_t> wide((size_t)longest);
    download_wide(t->edge_node.get(), 2 * E, edge_node, wide);
    download_wide(t->face_edge.get(), F * t->m, face_edge, wide);
    download_wide(t->edge_face.get(), 2 * E, edge_face, wide);
    download_wide(t->ff_ptr.get(), F + 1, ff_indptr, wide);
    download_wide(t->ff_idx.get(), t->ff_nnz, ff_indices, wide);
    download_wide(t->ff_dat.get(), t->ff_nnz, ff_data, wide);
    download_wide(t->nn_ptr.get(), N + 1, nn_indptr, wide);
    download_wide(t->nn_idx.get(), t->nn_nnz, nn_indices, wide);
    download_wide(t->nn_dat.get(), t->nn_nnz, nn_data, wide);
    download_wide(t->exterior_edge.get(), E, exterior_edge, wide);
    download_wide(t->exterior_face.get(), F, exterior_face, wide);
    XR_API_END
}

int xr_topology_download_node_tables(const xr_topology *t, int64_t *nf_indptr, int64_t *nf_indices, int64_t *ne_indptr,
                                     int64_t *ne_indices) {
    XR_API_BEGIN
    XR_REQUIRE(t, XR_ERR_INVALID, "xr_topology_download_node_tables: NULL handle");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID,
               "xr_topology_download_node_tables: the mesh has %lld edges with more than two faces", (long long)t->n_nonmanifold);
    const int64_t N = t->n_node;
    const int64_t nf_nnz = nf_indices ? read_scalar(t->nf_ptr.get() + N) : 0; // (nobody else needs it: not read back at build time)
    DevBuf<int64_t> wide((size_t)std::max({N + 1, nf_nnz, t->nn_nnz, (int64_t)1}));
    download_wide(t->nf_ptr.get(), N + 1, nf_indptr, wide);
    download_wide(t->nf_idx.get(), nf_nnz, nf_indices, wide);
    download_wide(t->nn_ptr.get(), N + 1, ne_indptr, wide);
    download_wide(t->nn_dat.get(), t->nn_nnz, ne_indices, wide);
    XR_API_END
}

int xr_topology_edge_xy_dev(const xr_topology *t, double *xy_dev) {
    XR_API_BEGIN
    XR_REQUIRE(t && (xy_dev || t->n_edge == 0), XR_ERR_INVALID, "xr_topology_edge_xy_dev: NULL argument");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_edge_xy_dev: the mesh has edges with more than two faces");
    if (t->n_edge > 0)
        XR_LAUNCH("topo_edge_xy", k_topo_edge_xy, dim3(div_up(2 * t->n_edge, 256)), dim3(256), 0, t->mesh->node_xy.get(),
                  t->edge_node.get(), t->n_edge, xy_dev);
    dev_call_done();
    XR_API_END
}

int xr_topology_exterior_face_dev(const xr_topology *t, uint8_t *flags_dev) {
    XR_API_BEGIN
    XR_REQUIRE(t && (flags_dev || t->n_face == 0), XR_ERR_INVALID, "xr_topology_exterior_face_dev: NULL argument");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_exterior_face_dev: the mesh has edges with more than two faces");
    if (t->n_face > 0)
        XR_HIP(hipMemcpyAsync(flags_dev, t->exterior_face.get(), (size_t)t->n_face, hipMemcpyDeviceToDevice, launch_stream()));
    dev_call_done();
    XR_API_END
}

int xr_topology_destroy(xr_topology *t) {
    XR_API_BEGIN
    if (t) {
        release_point();
        delete t;
    }
    XR_API_END
}

} // extern "C"
