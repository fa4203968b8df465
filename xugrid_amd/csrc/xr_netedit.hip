// xr_netedit.hip -- editing a network of line segments where it lies (Ugrid1d.topology_subset, ugrid1d.py:603-663; sel / clip_box,
// :574-601, :665-672; remove_self_loops, :714-738; merge_partitions, partitioning.py:81-116, :137-148; refine_by_vertices,
// ugrid1d.py:770-876).  DESIGN section 18.
//
// A network is two arrays of the CALLER in device memory: node_xy float64[n_node, 2] and edges int64[n_edge, 2].  Inside the
// kernels ids are int32; nothing is read through an id that has not been compared with its range, and an edge that names a node
// outside [0, n_node) is counted and never followed (the call then fails with XR_ERR_INVALID).
//
// Three patterns do the work, all shared with the mesh units:
//   - "distinct, ascending": a flag per old row (every writer stores the same 1), exclusive_scan_i32 (the dense rank), a
//     compaction (xr_index.h, as xr_subset.hip);
//   - "which rows are equal, and which came first": the key table of xr_key_table.h, as xr_merge.hip;
//   - "which vertices are near this segment": the cell grid of xr_nn.h over the VERTICES; every edge visits the cells its
//     tolerance-inflated segment passes, row of cells by row of cells.
// Atomics: one integer add per wave that saw a bad id; in the refinement an atomicMin per (vertex, edge within tolerance) --
// the LOWEST edge id wins, whatever the order of arrival, and the winner is read in the next launch --, an integer add per kept
// vertex (a count) and one whose RETURN VALUE is the vertex's slot in its edge's row.  The slots depend on arrival; the rows are
// ordered afterwards by (distance, position among the kept vertices), a total order, so nothing that leaves the unit does.
// No float atomics; no thread waits for another.
#include <algorithm>
#include <vector>

#include "xr_index.h"
#include "xr_nn.h"
#include "xr_objects.h"
#include "xr_prims.h"

#include "xr_key_table.h"

// the result of one edit: the new network and the indexes that came with it (include/xugrid_amd.h)
struct xr_netedit {
    bool has_network = false;
    int64_t n_node = 0, n_edge = 0;
    xr::DevBuf<double> node_xy;       // [n_node, 2]
    xr::DevBuf<int32_t> edges;        // [n_edge, 2]
    int64_t n_node_index = 0;
    xr::DevBuf<int32_t> node_index;   // subset: the old node of every new node; refine: the new ids of the inserted vertices, in order
    bool has_parent = false;
    xr::DevBuf<int32_t> parent_edge;  // refine: [n_edge] the old edge of every new edge
    int64_t n_node_all = 0;
    xr::DevBuf<int32_t> node_inverse; // merge: [n_node_all] the merged node of every concatenated node
    xr::DevBuf<int32_t> keep[2];      // merge: the kept nodes / edges as ids into the concatenation, ascending
    std::vector<int64_t> off[2], bound[2]; // merge: [n_part + 1] first row of partition p in the concatenation / in `keep`
    int64_t n_vertex = 0;
    xr::DevBuf<uint8_t> off_edge;     // refine that failed: [n_vertex] 1 for a vertex on no edge
};

namespace xr {

enum NetStatus : int { NS_RANGE = 0, NS_REPEAT = 1, NS_MOVED = 2, NS_BADNODE = 3, NS_COUNT = 4 };

static constexpr int NET_ROWS_LANE = 8;  // an edge whose cells span more rows than this is walked by its whole wave
static constexpr int NET_ROW_SMALL = 32; // vertices on one edge up to which a vertex finds its rank by counting; longer rows are sorted by a block

// the two nodes of edge e, both compared with [0, n_node) before anything is read through them
__device__ __forceinline__ bool net_edge(const int64_t *__restrict__ edges, int64_t e, int64_t n_node, int32_t &a, int32_t &b) {
    const int64_t u = edges[2 * e], v = edges[2 * e + 1];
    const bool ok = u >= 0 && u < n_node && v >= 0 && v < n_node;
    a = ok ? (int32_t)u : -1, b = ok ? (int32_t)v : -1;
    return ok;
}

// ---- subset
// one thread per i: pos[index[i]] = i + 1 (zero at the start; of a repeated id one writer wins, the others find out in the next
// launch); ids outside [0, n_edge) are counted, never used; status[NS_MOVED] = 1 when some index[i] != i
__global__ void __launch_bounds__(256)
k_net_mark(const int64_t *__restrict__ index, int64_t n, int64_t n_edge, int32_t *__restrict__ pos, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const int64_t e = index[i];
        bad = e < 0 || e >= n_edge;
        if (!bad) pos[e] = (int32_t)(i + 1);
        if (e != i) status[NS_MOVED] = 1;
    }
    wave_count(bad, status + NS_RANGE);
}

// one thread per i: a repeat is counted; both end nodes are flagged (all writers store 1)
__global__ void __launch_bounds__(256)
k_net_flag_nodes(const int64_t *__restrict__ index, int64_t n, int64_t n_edge, const int64_t *__restrict__ edges, int64_t n_node,
                 const int32_t *__restrict__ pos, int32_t *__restrict__ node_flag, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool repeat = false, bad_node = false;
    if (i < n) {
        const int64_t e = index[i];
        if (e >= 0 && e < n_edge) {
            repeat = pos[e] != (int32_t)(i + 1);
            int32_t a, b;
            bad_node = !net_edge(edges, e, n_node, a, b);
            if (!bad_node) node_flag[a] = 1, node_flag[b] = 1;
        }
    }
    wave_count(repeat, status + NS_REPEAT);
    wave_count(bad_node, status + NS_BADNODE);
}

// one thread per i: edge i of the new network through the dense ranks
__global__ void __launch_bounds__(256)
k_net_sub_edges(const int64_t *__restrict__ index, int64_t n, int64_t n_edge, const int64_t *__restrict__ edges, int64_t n_node,
                const int32_t *__restrict__ node_new, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t e = index[i];
    int32_t a, b;
    if (e < 0 || e >= n_edge || !net_edge(edges, e, n_node, a, b)) return; // (the call fails: the table is never handed out)
    out[2 * i] = node_new[a], out[2 * i + 1] = node_new[b];
}

// ---- flags of the selections
__global__ void __launch_bounds__(256)
k_net_edges_of_nodes(const int64_t *__restrict__ edges, int64_t n_edge, int64_t n_node, const int32_t *__restrict__ node_flag,
                     int32_t *__restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edge) return;
    int32_t a, b;
    flags[e] = net_edge(edges, e, n_node, a, b) && (node_flag[a] | node_flag[b]) != 0;
}

// the four comparisons of Ugrid1d.sel on the midpoint 0.5 * (a + b); a NaN midpoint fails them
__global__ void __launch_bounds__(256)
k_net_box_flags(const double2 *__restrict__ xy, int64_t n_node, const int64_t *__restrict__ edges, int64_t n_edge, double xmin, double ymin,
                double xmax, double ymax, int32_t *__restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edge) return;
    int32_t a, b;
    bool in = false;
    if (net_edge(edges, e, n_node, a, b)) {
        const double2 p = xy[a], q = xy[b];
        const double x = 0.5 * (p.x + q.x), y = 0.5 * (p.y + q.y);
        in = x >= xmin && x < xmax && y >= ymin && y < ymax;
    }
    flags[e] = in;
}

__global__ void __launch_bounds__(256) k_net_nonloop_flags(const int64_t *__restrict__ edges, int64_t n_edge, int32_t *__restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n_edge) flags[e] = edges[2 * e] != edges[2 * e + 1];
}

// ---- merge
// edges of one partition, one thread per edge: the merged node pair as given and as (lower, higher)
__global__ void __launch_bounds__(256)
k_net_merge_rows(const int64_t *__restrict__ edges, int64_t n_edge, int64_t n_node, int64_t node_off, const int32_t *__restrict__ inverse,
                 int32_t *__restrict__ given, int32_t *__restrict__ sorted, int32_t *__restrict__ bad_nodes) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (e < n_edge) {
        int32_t a, b;
        bad = !net_edge(edges, e, n_node, a, b);
        const int32_t u = bad ? -1 : inverse[node_off + a], v = bad ? -1 : inverse[node_off + b];
        given[2 * e] = u, given[2 * e + 1] = v;
        sorted[2 * e] = u < v ? u : v, sorted[2 * e + 1] = u < v ? v : u;
    }
    wave_count(bad, bad_nodes);
}

// a kept edge goes to its rank with its own orientation
__global__ void __launch_bounds__(256)
k_net_compact_edges(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n, const int32_t *__restrict__ given,
                    int32_t *__restrict__ keep, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int j = rank[i];
    keep[j] = (int32_t)i;
    out[2 * j] = given[2 * i], out[2 * j + 1] = given[2 * i + 1];
}

// ---- refine: locate
// Distance from p to the closed segment (a, b), the projection clamped to the segment WITHOUT a division: before a (dot <= 0,
// a zero-length edge included) the distance to a, behind b (dot >= |b - a|^2) the distance to b, between them |cross| / |b - a|.
// A point exactly on the carrier line of a segment with exactly representable differences has cross == 0: distance 0.0, found
// at tolerance 0.  NaN anywhere gives NaN: on no edge.
__device__ __forceinline__ double net_point_segment(double2 p, double2 a, double2 b) {
    const double ux = b.x - a.x, uy = b.y - a.y, vx = p.x - a.x, vy = p.y - a.y;
    const double len2 = ux * ux + uy * uy, dot = vx * ux + vy * uy;
    if (dot <= 0.0) return sqrt(vx * vx + vy * vy);
    if (dot >= len2) {
        const double wx = p.x - b.x, wy = p.y - b.y;
        return sqrt(wx * wx + wy * wy);
    }
    return fabs(ux * vy - uy * vx) / sqrt(len2);
}

// one row of cells for one edge: the stretch of the segment inside the row's band (half a cell and the tolerance wider on both
// sides, the outermost rows open-ended), its x range widened by the tolerance and a cell on both sides; the vertices of those
// cells lie next to each other in the index
__device__ __forceinline__ void net_visit_row(const SampleGrid &g, const int32_t *__restrict__ start, const double2 *__restrict__ pxy,
                                              const int32_t *__restrict__ pid, int cy, double2 a, double2 b, double tol, int32_t e,
                                              int32_t *__restrict__ win) {
    const double lo = cy == 0 ? -INFINITY : g.y0 + ((double)cy - 0.5) * g.h - tol;
    const double hi = cy == g.ny - 1 ? INFINITY : g.y0 + ((double)cy + 1.5) * g.h + tol;
    const double dy = b.y - a.y;
    double s0 = 0.0, s1 = 1.0;
    if (dy != 0.0) {
        const double t0 = (lo - a.y) / dy, t1 = (hi - a.y) / dy;
        s0 = fmax(fmin(t0, t1), 0.0), s1 = fmin(fmax(t0, t1), 1.0);
        if (s0 > s1) return;
    } else if (!(a.y >= lo && a.y <= hi)) {
        return;
    }
    const double xa = a.x + s0 * (b.x - a.x), xb = a.x + s1 * (b.x - a.x);
    const int cx0 = max(sp_cell_x(g, fmin(xa, xb) - tol) - 1, 0), cx1 = min(sp_cell_x(g, fmax(xa, xb) + tol) + 1, g.nx - 1);
    const int64_t base = (int64_t)cy * g.nx;
    for (int k = start[base + cx0]; k < start[base + cx1 + 1]; k++)
        if (net_point_segment(pxy[k], a, b) <= tol) atomicMin(win + pid[k], e);
}

// one thread per edge; win[v] (INT32_MAX at the start) ends as the lowest edge within `tol` of vertex v.  An edge of few rows
// of cells is walked by its lane; the others one after the other by the whole wave, a row per lane.
__global__ void __launch_bounds__(256)
k_net_locate(const double2 *__restrict__ xy, int64_t n_node, const int64_t *__restrict__ edges, int64_t n_edge, SampleGrid g,
             const int32_t *__restrict__ start, const double2 *__restrict__ pxy, const int32_t *__restrict__ pid, double tol,
             int32_t *__restrict__ win, int32_t *__restrict__ bad_nodes) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double2 a = make_double2(0.0, 0.0), b = a;
    int cy0 = 0, cy1 = -1;
    bool bad = false;
    if (e < n_edge) {
        int32_t u, v;
        bad = !net_edge(edges, e, n_node, u, v);
        if (!bad) {
            a = xy[u], b = xy[v];
            // (an edge whose box misses the grid by more than a cell and the tolerance has no vertex near it)
            const double x_lo = fmin(a.x, b.x) - tol, x_hi = fmax(a.x, b.x) + tol, y_lo = fmin(a.y, b.y) - tol, y_hi = fmax(a.y, b.y) + tol;
            const bool apart = x_hi < g.x0 - g.h || x_lo > g.x0 + ((double)g.nx + 1.0) * g.h || y_hi < g.y0 - g.h ||
                               y_lo > g.y0 + ((double)g.ny + 1.0) * g.h;
            if (!apart) cy0 = max(sp_cell_y(g, y_lo) - 1, 0), cy1 = min(sp_cell_y(g, y_hi) + 1, g.ny - 1);
        }
    }
    const bool wide = cy1 - cy0 + 1 > NET_ROWS_LANE;
    if (!wide)
        for (int cy = cy0; cy <= cy1; cy++) net_visit_row(g, start, pxy, pid, cy, a, b, tol, (int32_t)e, win);
    const int lane = threadIdx.x & 63;
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {
        const int src = __ffsll((long long)todo) - 1;
        const double2 sa = make_double2(__shfl(a.x, src), __shfl(a.y, src)), sb = make_double2(__shfl(b.x, src), __shfl(b.y, src));
        const int s_cy0 = __shfl(cy0, src), s_cy1 = __shfl(cy1, src);
        const int32_t s_e = (int32_t)(e - lane + src);
        for (int cy = s_cy0 + lane; cy <= s_cy1; cy += 64) net_visit_row(g, start, pxy, pid, cy, sa, sb, tol, s_e, win);
    }
    wave_count(bad, bad_nodes);
}

// mask[v] = vertex v is on no edge, counted
__global__ void __launch_bounds__(256)
k_net_off_edge(const int32_t *__restrict__ win, int64_t n_vertex, uint8_t *__restrict__ mask, int32_t *__restrict__ count) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool off = v < n_vertex && win[v] == INT32_MAX;
    if (v < n_vertex) mask[v] = off;
    wave_count(off, count);
}

// ---- refine: drop, count, order, emit
// a vertex is kept iff the first row of [nodes; vertices] with its coordinates is a vertex
__global__ void __launch_bounds__(256)
k_net_keep_flags(const int32_t *__restrict__ rep, int64_t n_node, int64_t n_vertex, int32_t *__restrict__ keep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vertex) keep[v] = rep[n_node + v] >= n_node;
}

__global__ void __launch_bounds__(256)
k_net_count(const int32_t *__restrict__ keep, const int32_t *__restrict__ win, int64_t n_vertex, int64_t n_edge, int32_t *__restrict__ count) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertex || !keep[v]) return;
    const int32_t e = win[v];
    if (e >= 0 && e < n_edge) atomicAdd(count + e, 1);
}

// repeats[e] = 1 + count[e]; an edge with a long row goes on the list of the block sort (its order there is of no consequence)
__global__ void __launch_bounds__(256)
k_net_repeats(const int32_t *__restrict__ count, int64_t n_edge, int32_t *__restrict__ repeats, int32_t *__restrict__ long_rows,
              int32_t *__restrict__ n_long) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edge) return;
    const int32_t c = count[e];
    repeats[e] = 1 + c;
    if (c > NET_ROW_SMALL) long_rows[atomicAdd(n_long, 1)] = (int32_t)e;
}

// one thread per kept vertex: its coordinates go behind the nodes, at its position among the kept; it takes the next slot of its
// edge's row (row e starts at first[e] - e: the exclusive scan of the counts) with its distance from the edge's FIRST node
__global__ void __launch_bounds__(256)
k_net_fill_rows(const int32_t *__restrict__ keep, const int32_t *__restrict__ krank, const int32_t *__restrict__ win, int64_t n_vertex,
                const double2 *__restrict__ vertices, const double2 *__restrict__ xy, int64_t n_node, const int64_t *__restrict__ edges,
                int64_t n_edge, const int32_t *__restrict__ first, int32_t *__restrict__ cursor, double2 *__restrict__ out_xy,
                double *__restrict__ row_d, int32_t *__restrict__ row_k, int32_t *__restrict__ row_e) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertex || !keep[v]) return;
    const double2 p = vertices[v];
    const int32_t k = krank[v], e = win[v];
    out_xy[n_node + k] = p; // (16 bytes copied: bit for bit, never projected onto the edge)
    int32_t a, b;
    if (e < 0 || e >= n_edge || !net_edge(edges, e, n_node, a, b)) return; // (cannot happen: only valid edges take part in the search)
    const double2 q = xy[a];
    const double dx = p.x - q.x, dy = p.y - q.y;
    const int64_t at = (int64_t)first[e] - e + atomicAdd(cursor + e, 1);
    row_d[at] = sqrt(dx * dx + dy * dy), row_k[at] = k, row_e[at] = e;
}

// the order inside a row: by distance, then by position among the kept vertices (np.lexsort is stable)
__device__ __forceinline__ bool net_before(double d, int32_t k, double d2, int32_t k2) { return d < d2 || (d == d2 && k < k2); }

// one block per long row: a bitonic network whose every compare-exchange is ascending (the first step of a merge pairs i with
// its mirror image), so the slots behind the row's end, which stand for +infinity, never move and are never touched
__global__ void __launch_bounds__(256)
k_net_sort_long(const int32_t *__restrict__ long_rows, const int32_t *__restrict__ first, double *__restrict__ row_d, int32_t *__restrict__ row_k) {
    const int32_t e = long_rows[blockIdx.x];
    const int64_t base = (int64_t)first[e] - e;
    const int64_t len = (int64_t)first[e + 1] - first[e] - 1;
    double *d = row_d + base;
    int32_t *k = row_k + base;
    int64_t padded = 2;
    while (padded < len) padded <<= 1;
    auto exchange = [&](int64_t i, int64_t j) {
        if (j >= len) return;
        const double di = d[i], dj = d[j];
        const int32_t ki = k[i], kj = k[j];
        if (net_before(dj, kj, di, ki)) d[i] = dj, d[j] = di, k[i] = kj, k[j] = ki;
    };
    for (int64_t width = 2; width <= padded; width <<= 1) {
        const int64_t half = width >> 1;
        for (int64_t t = threadIdx.x; t < padded / 2; t += 256) {
            const int64_t block = t / half, o = t - block * half;
            exchange(block * width + o, block * width + width - 1 - o);
        }
        __syncthreads();
        for (int64_t s = half >> 1; s > 0; s >>= 1) {
            for (int64_t t = threadIdx.x; t < padded / 2; t += 256) {
                const int64_t i = 2 * s * (t / s) + t % s;
                exchange(i, i + s);
            }
            __syncthreads();
        }
    }
}

// one thread per row slot: the rank r of its vertex in the row (counted in a short row; a long row is sorted already), then
// the vertex's id at node_index[row start + r] and in the two edges it joins: first[e] + r ends in it, first[e] + r + 1 starts there
__global__ void __launch_bounds__(256)
k_net_emit(int64_t n_kept, const double *__restrict__ row_d, const int32_t *__restrict__ row_k, const int32_t *__restrict__ row_e,
           const int32_t *__restrict__ first, int64_t n_node, int32_t *__restrict__ node_index, int32_t *__restrict__ out_edges,
           int32_t *__restrict__ parent) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_kept) return;
    const int32_t e = row_e[p];
    const int64_t s = first[e], base = s - e, c = (int64_t)first[e + 1] - s - 1;
    int64_t r = p - base;
    if (c <= NET_ROW_SMALL) {
        const double d = row_d[p];
        const int32_t k = row_k[p];
        r = 0;
        for (int64_t q = base; q < base + c; q++) r += net_before(row_d[q], row_k[q], d, k);
    }
    const int32_t id = (int32_t)(n_node + row_k[p]);
    node_index[base + r] = id;
    out_edges[2 * (s + r) + 1] = id;
    out_edges[2 * (s + r + 1)] = id;
    parent[s + r + 1] = e;
}

// one thread per old edge: its first piece starts at its first node, its last piece ends at its second; an edge naming a node out
// of range is counted (without vertices no search has looked at the edges before)
__global__ void __launch_bounds__(256)
k_net_emit_ends(const int64_t *__restrict__ edges, int64_t n_edge, int64_t n_node, const int32_t *__restrict__ first,
                int32_t *__restrict__ out_edges, int32_t *__restrict__ parent, int32_t *__restrict__ bad_nodes) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (e < n_edge) {
        int32_t a, b;
        bad = !net_edge(edges, e, n_node, a, b);
        const int64_t s = first[e], last = (int64_t)first[e + 1] - 1;
        out_edges[2 * s] = a;
        out_edges[2 * last + 1] = b;
        parent[s] = (int32_t)e;
    }
    wave_count(bad, bad_nodes);
}

static void copy_dev(void *dst, const void *src, size_t bytes) {
    if (bytes) XR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, launch_stream()));
}

static void set_offsets(xr_netedit *net, int facet, const int64_t *sizes, int P) {
    net->off[facet].assign((size_t)P + 1, 0);
    for (int p = 0; p < P; p++) net->off[facet][(size_t)p + 1] = net->off[facet][(size_t)p] + sizes[p];
    net->bound[facet].assign((size_t)P + 1, 0);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_network_subset_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, const int64_t *edge_index_dev,
                          int64_t n, xr_netedit **out, int *is_identity, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(out && problems && (node_xy_dev || n_node == 0) && (edges_dev || n_edge == 0) && (edge_index_dev || n == 0) &&
                   n_node >= 0 && n_edge >= 0,
               XR_ERR_INVALID, "xr_network_subset_dev: bad argument");
    const int64_t N = n_node, E = n_edge;
    XR_REQUIRE(n >= 0 && n <= E, XR_ERR_INVALID, "index size %lld is larger than dimension size: %lld", (long long)n, (long long)E);
    XR_REQUIRE(N < INT32_MAX && 2 * E < INT32_MAX, XR_ERR_LIMIT, "xr_network_subset_dev: %lld nodes / %lld edges exceed the int32 index range",
               (long long)N, (long long)E);
    *out = nullptr;
    int identity_unused = 0;
    if (!is_identity) is_identity = &identity_unused; // (the caller wants the identity selection cut like any other)
    const bool keep_identity = is_identity != &identity_unused;
    *is_identity = 0;
    problems[0] = problems[1] = 0;
    Building<xr_netedit> sub(OnFailure::WaitFirst);
    sub->has_network = true;
    if (n > 0) {
        // one block: [node_new: N + 1][status: NS_COUNT][.. to a multiple of 4 words][node_flag: N][pos: E]; everything behind
        // node_new starts as zero (one fill), node_new[N] and the status words come back in one copy
        const int64_t flag_at = (N + 1 + NS_COUNT + 3) / 4 * 4;
        DevBuf<int32_t> work((size_t)(flag_at + N + E));
        int32_t *node_new = work.get(), *status = work.get() + N + 1, *node_flag = work.get() + flag_at, *pos = node_flag + N;
        fill_i32(status, 0, flag_at - (N + 1) + N + E);
        XR_LAUNCH("netedit_mark", k_net_mark, dim3(div_up(n, 256)), dim3(256), 0, edge_index_dev, n, E, pos, status);
        XR_LAUNCH("netedit_flag_nodes", k_net_flag_nodes, dim3(div_up(n, 256)), dim3(256), 0, edge_index_dev, n, E, edges_dev, N, pos, node_flag,
                  status);
        rank_of_flags(node_flag, node_new, N);
        sub->edges.alloc((size_t)n * 2);
        int32_t h[1 + NS_COUNT] = {0, 0, 0, 0, 0}; // node total, then the status words
        // (the new table needs the ranks, not their number: it is written while the number travels)
        d2h(h, node_new + N, sizeof(h), [&] {
            XR_LAUNCH("netedit_sub_edges", k_net_sub_edges, dim3(div_up(n, 256)), dim3(256), 0, edge_index_dev, n, E, edges_dev, N, node_new,
                      sub->edges.get());
        });
        problems[0] = h[1 + NS_RANGE];
        problems[1] = h[1 + NS_REPEAT];
        XR_REQUIRE(h[1 + NS_BADNODE] == 0, XR_ERR_INVALID, "xr_network_subset_dev: %d selected edges refer to nodes that do not exist",
                   (int)h[1 + NS_BADNODE]);
        if (problems[0] || problems[1] || (keep_identity && n == E && !h[1 + NS_MOVED])) {
            *is_identity = !problems[0] && !problems[1];
            stream_sync();
            return XR_OK; // (`sub` is freed on the way out)
        }
        const int64_t Nn = h[0];
        XR_REQUIRE(Nn > 0 && Nn <= N, XR_ERR_HIP, "xr_network_subset_dev: kept node count out of range");
        sub->n_node = Nn, sub->n_edge = n, sub->n_node_index = Nn;
        sub->node_xy.alloc((size_t)Nn * 2);
        sub->node_index.alloc((size_t)Nn);
        XR_LAUNCH("netedit_sub_nodes", k_merge_compact_xy, dim3(div_up(N, 256)), dim3(256), 0, node_flag, node_new, N,
                  reinterpret_cast<const double2 *>(node_xy_dev), sub->node_index.get(), reinterpret_cast<double2 *>(sub->node_xy.get()));
        stream_sync(); // (`work` goes back to the pool behind its readers)
    } else {
        *is_identity = keep_identity && E == 0;
        if (*is_identity) return XR_OK;
        sub->node_xy.alloc(0), sub->edges.alloc(0), sub->node_index.alloc(0); // the empty network: nothing is launched
    }
    *out = sub.release();
    XR_API_END
}

int xr_network_edges_of_nodes_dev(const int64_t *edges_dev, int64_t n_edge, int64_t n_node, const int64_t *node_index_dev, int64_t n,
                                  xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (edges_dev || n_edge == 0) && (node_index_dev || n == 0) && n >= 0 && n_edge >= 0 && n_node >= 0, XR_ERR_INVALID,
               "xr_network_edges_of_nodes_dev: bad argument");
    XR_REQUIRE(n_node < INT32_MAX && n_edge < INT32_MAX, XR_ERR_LIMIT, "xr_network_edges_of_nodes_dev: sizes exceed the int32 index range");
    DevBuf<int32_t> flags((size_t)n_edge), node_flag((size_t)n_node);
    fill_i32(node_flag.get(), 0, n_node);
    if (n > 0 && n_node > 0)
        XR_LAUNCH("index_flag_ids", k_flag_ids, dim3(div_up(n, 256)), dim3(256), 0, node_index_dev, n, n_node, node_flag.get());
    if (n_edge > 0)
        XR_LAUNCH("netedit_edges_of_nodes", k_net_edges_of_nodes, dim3(div_up(n_edge, 256)), dim3(256), 0, edges_dev, n_edge, n_node,
                  node_flag.get(), flags.get());
    *out = index_from_flags(flags.get(), n_edge);
    XR_API_END
}

int xr_network_box_edges_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, double xmin, double ymin,
                             double xmax, double ymax, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (node_xy_dev || n_node == 0) && (edges_dev || n_edge == 0) && n_edge >= 0 && n_node >= 0, XR_ERR_INVALID,
               "xr_network_box_edges_dev: bad argument");
    XR_REQUIRE(n_node < INT32_MAX && n_edge < INT32_MAX, XR_ERR_LIMIT, "xr_network_box_edges_dev: sizes exceed the int32 index range");
    DevBuf<int32_t> flags((size_t)n_edge);
    if (n_edge > 0)
        XR_LAUNCH("netedit_box_flags", k_net_box_flags, dim3(div_up(n_edge, 256)), dim3(256), 0, reinterpret_cast<const double2 *>(node_xy_dev),
                  n_node, edges_dev, n_edge, xmin, ymin, xmax, ymax, flags.get());
    *out = index_from_flags(flags.get(), n_edge);
    XR_API_END
}

int xr_network_nonloop_edges_dev(const int64_t *edges_dev, int64_t n_edge, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (edges_dev || n_edge == 0) && n_edge >= 0, XR_ERR_INVALID, "xr_network_nonloop_edges_dev: bad argument");
    XR_REQUIRE(n_edge < INT32_MAX, XR_ERR_LIMIT, "xr_network_nonloop_edges_dev: the edges exceed the int32 index range");
    DevBuf<int32_t> flags((size_t)n_edge);
    if (n_edge > 0) XR_LAUNCH("netedit_nonloop_flags", k_net_nonloop_flags, dim3(div_up(n_edge, 256)), dim3(256), 0, edges_dev, n_edge, flags.get());
    *out = index_from_flags(flags.get(), n_edge);
    XR_API_END
}

int xr_network_merge_dev(const double *const *node_xy_dev, const int64_t *n_node, const int64_t *const *edges_dev, const int64_t *n_edge,
                         int64_t n_part, xr_netedit **out) {
    XR_API_BEGIN
    XR_REQUIRE(node_xy_dev && n_node && edges_dev && n_edge && out && n_part >= 1 && n_part < (1 << 20), XR_ERR_INVALID,
               "xr_network_merge_dev: bad argument");
    const int P = (int)n_part;
    for (int p = 0; p < P; p++)
        XR_REQUIRE(n_node[p] >= 0 && n_edge[p] >= 0 && (node_xy_dev[p] || n_node[p] == 0) && (edges_dev[p] || n_edge[p] == 0), XR_ERR_INVALID,
                   "xr_network_merge_dev: bad partition %d", p);
    *out = nullptr;
    Building<xr_netedit> merge(OnFailure::WaitFirst);
    merge->has_network = true;
    set_offsets(merge.get(), 0, n_node, P), set_offsets(merge.get(), 1, n_edge, P);
    const std::vector<int64_t> &node_off = merge->off[0], &edge_off = merge->off[1];
    const int64_t N = node_off[(size_t)P], E = edge_off[(size_t)P];
    XR_REQUIRE(N < INT32_MAX && 2 * E < INT32_MAX, XR_ERR_LIMIT, "xr_network_merge_dev: %lld nodes / %lld edges in all exceed the int32 index range",
               (long long)N, (long long)E);
    merge->n_node_all = N;

    // nodes: concatenate, first occurrences, rank, inverse
    DevBuf<double> all_xy((size_t)N * 2);
    for (int p = 0; p < P; p++) copy_dev(all_xy.get() + 2 * node_off[(size_t)p], node_xy_dev[p], (size_t)n_node[p] * 16);
    DevBuf<int32_t> node_rep((size_t)N), node_flag((size_t)N), node_rank((size_t)N + 1);
    merge->node_inverse.alloc((size_t)N);
    if (N > 0) table_first_occurrence(XYRows{reinterpret_cast<const double2 *>(all_xy.get())}, N, node_rep.get(), node_flag.get());
    rank_of_flags(node_flag.get(), node_rank.get(), N);
    if (N > 0)
        XR_LAUNCH("netedit_inverse", k_merge_inverse, dim3(div_up(N, 256)), dim3(256), 0, node_rep.get(), node_rank.get(), N,
                  merge->node_inverse.get());

    // edges: the merged pairs as given and sorted; the same table on the sorted pairs
    DevBuf<int32_t> given((size_t)E * 2), sorted((size_t)E * 2), edge_rep((size_t)E), edge_flag((size_t)E), edge_rank((size_t)E + 1);
    // words: [at: 2 (P + 1)][the scans there: 2 (P + 1)][edges with a node out of range: 1]
    const int W = 2 * (P + 1);
    DevBuf<int32_t> words((size_t)2 * W + 1);
    int32_t *bad_nodes = words.get() + 2 * W;
    fill_i32(bad_nodes, 0, 1);
    for (int p = 0; p < P; p++)
        if (n_edge[p] > 0)
            XR_LAUNCH("netedit_merge_rows", k_net_merge_rows, dim3(div_up(n_edge[p], 256)), dim3(256), 0, edges_dev[p], n_edge[p], n_node[p],
                      node_off[(size_t)p], merge->node_inverse.get(), given.get() + 2 * edge_off[(size_t)p], sorted.get() + 2 * edge_off[(size_t)p],
                      bad_nodes);
    if (E > 0) table_first_occurrence(IntRows{sorted.get(), 2}, E, edge_rep.get(), edge_flag.get());
    rank_of_flags(edge_flag.get(), edge_rank.get(), E);

    // the one read-back: both scans at the partitions' boundaries (the last of each is its total) and the bad edges
    std::vector<int32_t> at((size_t)W), h((size_t)W + 1);
    for (int p = 0; p <= P; p++) at[(size_t)p] = (int32_t)node_off[(size_t)p], at[(size_t)(P + 1 + p)] = (int32_t)edge_off[(size_t)p];
    h2d(words.get(), at.data(), at.size() * sizeof(int32_t));
    XR_LAUNCH("netedit_bounds", k_merge_bounds, dim3(div_up(W, 256)), dim3(256), 0, node_rank.get(), edge_rank.get(), words.get(), P + 1, P + 1,
              words.get() + W);
    d2h(h.data(), words.get() + W, h.size() * sizeof(int32_t));
    XR_REQUIRE(h[(size_t)W] == 0, XR_ERR_INVALID, "xr_network_merge_dev: %d edges refer to nodes that do not exist", (int)h[(size_t)W]);
    for (int p = 0; p <= P; p++) merge->bound[0][(size_t)p] = h[(size_t)p], merge->bound[1][(size_t)p] = h[(size_t)(P + 1 + p)];
    const int64_t Nn = merge->bound[0][(size_t)P], En = merge->bound[1][(size_t)P];
    XR_REQUIRE(Nn >= 0 && Nn <= N && En >= 0 && En <= E, XR_ERR_HIP, "xr_network_merge_dev: kept counts out of range");

    merge->n_node = Nn, merge->n_edge = En;
    merge->node_xy.alloc((size_t)Nn * 2), merge->edges.alloc((size_t)En * 2);
    merge->keep[0].alloc((size_t)Nn), merge->keep[1].alloc((size_t)En);
    if (Nn > 0)
        XR_LAUNCH("netedit_compact_xy", k_merge_compact_xy, dim3(div_up(N, 256)), dim3(256), 0, node_flag.get(), node_rank.get(), N,
                  reinterpret_cast<const double2 *>(all_xy.get()), merge->keep[0].get(), reinterpret_cast<double2 *>(merge->node_xy.get()));
    if (En > 0)
        XR_LAUNCH("netedit_compact_edges", k_net_compact_edges, dim3(div_up(E, 256)), dim3(256), 0, edge_flag.get(), edge_rank.get(), E, given.get(),
                  merge->keep[1].get(), merge->edges.get());
    stream_sync(); // (the work arrays go back to the pool behind their readers)
    *out = merge.release();
    XR_API_END
}

int xr_network_refine_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, const double *vertices_dev,
                          int64_t n_vertex, double tolerance, xr_netedit **out, int64_t *n_off_edge) {
    XR_API_BEGIN
    XR_REQUIRE(out && n_off_edge && (node_xy_dev || n_node == 0) && (edges_dev || n_edge == 0) && (vertices_dev || n_vertex == 0) && n_node >= 0 &&
                   n_edge >= 0 && n_vertex >= 0,
               XR_ERR_INVALID, "xr_network_refine_dev: bad argument");
    XR_REQUIRE(tolerance >= 0.0, XR_ERR_INVALID, "xr_network_refine_dev: tolerance must be non-negative");
    const int64_t N = n_node, E = n_edge, V = n_vertex;
    XR_REQUIRE(N + V < INT32_MAX && 2 * (E + V) < INT32_MAX, XR_ERR_LIMIT,
               "xr_network_refine_dev: %lld nodes, %lld edges and %lld vertices exceed the int32 index range", (long long)N, (long long)E, (long long)V);
    *out = nullptr;
    *n_off_edge = 0;
    const double2 *xy = reinterpret_cast<const double2 *>(node_xy_dev), *vertices = reinterpret_cast<const double2 *>(vertices_dev);
    Building<xr_netedit> net(OnFailure::WaitFirst);
    net->n_vertex = V;

    // (a) locate: win[v] = the lowest edge within the tolerance, read in the launch after the search
    DevBuf<int32_t> win((size_t)V), words(2); // words: vertices on no edge, edges with a node out of range
    DevBuf<int32_t> rep((size_t)(N + V)), unused_flag((size_t)(N + V));
    DevBuf<double> all_xy((size_t)(N + V) * 2);
    fill_i32(words.get(), 0, 2);
    if (V > 0) {
        fill_i32(win.get(), INT32_MAX, V);
        std::unique_ptr<xr_nn> cells(nn_build(vertices_dev, V));
        if (E > 0)
            XR_LAUNCH("netedit_locate", k_net_locate, dim3(div_up(E, 256)), dim3(256), 0, xy, N, edges_dev, E, cells->grid, cells->start.get(),
                      cells->xy.get(), cells->id.get(), tolerance, win.get(), words.get() + 1);
        net->off_edge.alloc((size_t)V);
        XR_LAUNCH("netedit_off_edge", k_net_off_edge, dim3(div_up(V, 256)), dim3(256), 0, win.get(), V, net->off_edge.get(), words.get());
        int32_t h[2];
        // (b) rides behind the read-back: the first occurrences of [nodes; vertices]
        d2h(h, words.get(), sizeof(h), [&] {
            copy_dev(all_xy.get(), node_xy_dev, (size_t)N * 16);
            copy_dev(all_xy.get() + 2 * N, vertices_dev, (size_t)V * 16);
            table_first_occurrence(XYRows{reinterpret_cast<const double2 *>(all_xy.get())}, N + V, rep.get(), unused_flag.get());
        });
        stream_sync(); // (the cell index goes back to the pool behind its readers)
        XR_REQUIRE(h[1] == 0, XR_ERR_INVALID, "xr_network_refine_dev: %d edges refer to nodes that do not exist", (int)h[1]);
        if (h[0] > 0) {
            *n_off_edge = h[0];
            *out = net.release(); // (only the mask: xr_netedit_copy_dev(.., XR_NET_OFF_EDGE, ..))
            return XR_OK;
        }
    }
    net->off_edge.release();
    net->n_vertex = 0;

    // (b), (c): the kept vertices, their number per edge, the first new edge of every old edge
    DevBuf<int32_t> keep((size_t)V), krank((size_t)V + 2), count((size_t)E), repeats((size_t)E), first((size_t)E + 1), long_rows((size_t)(V / (NET_ROW_SMALL + 1) + 1));
    int32_t *n_long = krank.get() + V + 1;
    fill_i32(count.get(), 0, E);
    fill_i32(n_long, 0, 1);
    if (V > 0) XR_LAUNCH("netedit_keep_flags", k_net_keep_flags, dim3(div_up(V, 256)), dim3(256), 0, rep.get(), N, V, keep.get());
    rank_of_flags(keep.get(), krank.get(), V);
    if (V > 0 && E > 0) XR_LAUNCH("netedit_count", k_net_count, dim3(div_up(V, 256)), dim3(256), 0, keep.get(), win.get(), V, E, count.get());
    if (E > 0)
        XR_LAUNCH("netedit_repeats", k_net_repeats, dim3(div_up(E, 256)), dim3(256), 0, count.get(), E, repeats.get(), long_rows.get(), n_long);
    rank_of_flags(repeats.get(), first.get(), E);
    int32_t h[2]; // kept vertices, long rows
    d2h(h, krank.get() + V, sizeof(h));
    const int64_t K = h[0], L = h[1];
    XR_REQUIRE(K >= 0 && K <= V && L >= 0 && L <= V / (NET_ROW_SMALL + 1) + 1 && (E > 0 || K == 0), XR_ERR_HIP,
               "xr_network_refine_dev: kept counts out of range");

    // (d) emit
    const int64_t Nn = N + K, En = E + K;
    net->has_network = net->has_parent = true;
    net->n_node = Nn, net->n_edge = En, net->n_node_index = K;
    net->node_xy.alloc((size_t)Nn * 2), net->edges.alloc((size_t)En * 2), net->node_index.alloc((size_t)K), net->parent_edge.alloc((size_t)En);
    copy_dev(net->node_xy.get(), node_xy_dev, (size_t)N * 16);
    if (K > 0) {
        DevBuf<double> row_d((size_t)K);
        DevBuf<int32_t> row_k((size_t)K), row_e((size_t)K);
        fill_i32(count.get(), 0, E); // (now the rows' cursors)
        XR_LAUNCH("netedit_fill_rows", k_net_fill_rows, dim3(div_up(V, 256)), dim3(256), 0, keep.get(), krank.get(), win.get(), V, vertices, xy, N,
                  edges_dev, E, first.get(), count.get(), reinterpret_cast<double2 *>(net->node_xy.get()), row_d.get(), row_k.get(), row_e.get());
        if (L > 0) XR_LAUNCH("netedit_sort_long", k_net_sort_long, dim3((unsigned)L), dim3(256), 0, long_rows.get(), first.get(), row_d.get(), row_k.get());
        XR_LAUNCH("netedit_emit", k_net_emit, dim3(div_up(K, 256)), dim3(256), 0, K, row_d.get(), row_k.get(), row_e.get(), first.get(), N,
                  net->node_index.get(), net->edges.get(), net->parent_edge.get());
        if (E > 0)
            XR_LAUNCH("netedit_emit_ends", k_net_emit_ends, dim3(div_up(E, 256)), dim3(256), 0, edges_dev, E, N, first.get(), net->edges.get(),
                      net->parent_edge.get(), words.get() + 1);
        stream_sync(); // (the rows go back to the pool behind their readers)
    } else if (E > 0) {
        XR_LAUNCH("netedit_emit_ends", k_net_emit_ends, dim3(div_up(E, 256)), dim3(256), 0, edges_dev, E, N, first.get(), net->edges.get(),
                  net->parent_edge.get(), words.get() + 1);
        // (no vertex was kept: with no vertices at all, this is the first look at the edges)
        if (V == 0) {
            const int32_t bad = read_scalar(words.get() + 1);
            XR_REQUIRE(bad == 0, XR_ERR_INVALID, "xr_network_refine_dev: %d edges refer to nodes that do not exist", (int)bad);
        }
    }
    stream_sync();
    *out = net.release();
    XR_API_END
}

int xr_netedit_info(const xr_netedit *net, int64_t *sizes) {
    XR_API_BEGIN
    XR_REQUIRE(net && sizes, XR_ERR_INVALID, "xr_netedit_info: NULL argument");
    sizes[0] = net->has_network ? net->n_node : -1, sizes[1] = net->has_network ? net->n_edge : -1;
    sizes[2] = net->n_node_index, sizes[3] = net->has_parent ? net->n_edge : 0, sizes[4] = net->n_node_all;
    sizes[5] = net->off[0].empty() ? 0 : (int64_t)net->off[0].size() - 1, sizes[6] = net->n_vertex;
    XR_API_END
}

int xr_netedit_copy_dev(const xr_netedit *net, int what, void *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(net && what >= XR_NET_NODE_XY && what <= XR_NET_OFF_EDGE, XR_ERR_INVALID, "xr_netedit_copy_dev: bad argument");
    XR_REQUIRE(net->has_network || what == XR_NET_OFF_EDGE, XR_ERR_INVALID, "xr_netedit_copy_dev: the handle holds no network");
    int64_t *wide = static_cast<int64_t *>(out_dev);
    int64_t n = 0;
    switch (what) {
    case XR_NET_NODE_XY: n = net->n_node * 2; break;
    case XR_NET_EDGES: n = net->n_edge * 2; break;
    case XR_NET_NODE_INDEX: n = net->n_node_index; break;
    case XR_NET_PARENT_EDGE: n = net->has_parent ? net->n_edge : 0; break;
    case XR_NET_NODE_INVERSE: n = net->n_node_all; break;
    default: n = net->n_vertex; break;
    }
    XR_REQUIRE(out_dev || n == 0, XR_ERR_INVALID, "xr_netedit_copy_dev: NULL argument");
    switch (what) {
    case XR_NET_NODE_XY: copy_dev(out_dev, net->node_xy.get(), (size_t)n * sizeof(double)); break;
    case XR_NET_EDGES: widen_dev(net->edges.get(), n, wide); break;
    case XR_NET_NODE_INDEX: widen_dev(net->node_index.get(), n, wide); break;
    case XR_NET_PARENT_EDGE: widen_dev(net->parent_edge.get(), n, wide); break;
    case XR_NET_NODE_INVERSE: widen_dev(net->node_inverse.get(), n, wide); break;
    default: copy_dev(out_dev, net->off_edge.get(), (size_t)n); break;
    }
    dev_call_done();
    XR_API_END
}

int xr_netedit_part_info(const xr_netedit *net, int facet, int64_t part, int64_t *n) {
    XR_API_BEGIN
    XR_REQUIRE(net && n && facet >= 0 && facet < 2 && part >= 0 && part + 1 < (int64_t)net->bound[facet].size(), XR_ERR_INVALID,
               "xr_netedit_part_info: bad argument");
    *n = net->bound[facet][(size_t)part + 1] - net->bound[facet][(size_t)part];
    XR_API_END
}

int xr_netedit_part_copy_dev(const xr_netedit *net, int facet, int64_t part, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(net && facet >= 0 && facet < 2 && part >= 0 && part + 1 < (int64_t)net->bound[facet].size(), XR_ERR_INVALID,
               "xr_netedit_part_copy_dev: bad argument");
    const int64_t at = net->bound[facet][(size_t)part], n = net->bound[facet][(size_t)part + 1] - at;
    XR_REQUIRE(out_dev || n == 0, XR_ERR_INVALID, "xr_netedit_part_copy_dev: NULL argument");
    widen_dev(net->keep[facet].get() + at, n, out_dev, net->off[facet][(size_t)part]);
    dev_call_done();
    XR_API_END
}

int xr_netedit_destroy(xr_netedit *net) {
    XR_API_BEGIN
    if (net) {
        release_point();
        delete net;
    }
    XR_API_END
}

} // extern "C"
