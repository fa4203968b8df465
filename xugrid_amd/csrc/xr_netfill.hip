// xr_netfill.hip -- filling the NaN entries of network data along the edges: the nearest fill of xugrid/ugrid/ugrid1d.py
// (Ugrid1d._nearest_interpolate), which measures "nearest" with a multi-source scipy.sparse.csgraph.dijkstra over the node
// graph (weights: the edge lengths) or the edge graph (weights: half of the two edge lengths).
//
// Graphs: xr_network_graph_dev builds either CSR in HBM from the edge table -- degree counts, the int32 scan, the rows filled
// in any order, every row sorted ascending (one thread per short row, one block per long one: a hub's row fits neither a
// wave nor a block).  Self-loops and repeated node pairs are counted, not built.
//
// Nearest: per slice and vertex a state (d, s) = (distance, source id).  A round is a pull: the owner of vertex v reads the
// states of v and of its neighbours as they were and takes the lexicographic minimum of its own state and of the candidates
// (fl(d_u + w), s_u) within the limit; the round's results go to a second buffer (no state is ever read while it is written,
// so no half-updated pair exists).  Within a round a block sweeps its own 256 vertices several times in LDS, so a value
// crosses a block per round where neighbouring ids are adjacent.  States only decrease, so the rounds end, at the same fixed
// point whatever the sweeps; the host reads one word per chunk of rounds, and a round behind one that changed nothing returns
// at once.
#include <algorithm>
#include <cmath>
#include <vector>

#include "xr_objects.h"
#include "xr_prims.h"

namespace xr {

static constexpr int NB = 256;            // threads per block
static constexpr int NET_SHORT_ROW = 32;  // rows up to this many entries are sorted by one thread
static constexpr int NET_SWEEPS = NB;     // sweeps of a block over its own vertices within one round, at most
static constexpr int64_t NET_CHUNK = 32;  // rounds between two reads of the "changed" words

// ---------------------------------------------------------------------------------------------
// graph construction
// ---------------------------------------------------------------------------------------------
// per edge: node ids in range (counters[0] counts the ones that are not), self-loop (counters[1]), its length, the degrees
__global__ void __launch_bounds__(NB)
k_net_degree(const int64_t *__restrict__ edges, int64_t n_edge, int64_t n_node, const double *__restrict__ xy, int32_t *deg,
             double *__restrict__ len, int32_t *counters) {
    const int64_t e = (int64_t)blockIdx.x * NB + threadIdx.x;
    bool bad = false, loop = false;
    if (e < n_edge) {
        const int64_t a = edges[2 * e], b = edges[2 * e + 1];
        bad = a < 0 || a >= n_node || b < 0 || b >= n_node;
        double v = 0.0;
        if (!bad) {
            loop = a == b;
            const double dx = xy[2 * b] - xy[2 * a], dy = xy[2 * b + 1] - xy[2 * a + 1];
            v = sqrt(dx * dx + dy * dy);
            if (!loop) {
                atomicAdd(&deg[a], 1);
                atomicAdd(&deg[b], 1);
            }
        }
        len[e] = v;
    }
    wave_count(bad, counters);
    wave_count(loop, counters + 1);
}

// node -> (neighbour, edge) in the order the edges arrive: key = neighbour << 32 | edge.  Self-loops take no slot.
__global__ void __launch_bounds__(NB)
k_net_node_fill(const int64_t *__restrict__ edges, int64_t n_edge, const int32_t *__restrict__ nptr, int32_t *cursor,
                uint64_t *__restrict__ key) {
    const int64_t e = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (e >= n_edge) return;
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    if (a == b) return;
    key[nptr[a] + atomicAdd(&cursor[a], 1)] = ((uint64_t)b << 32) | (uint64_t)e;
    key[nptr[b] + atomicAdd(&cursor[b], 1)] = ((uint64_t)a << 32) | (uint64_t)e;
}

// rows of at most NET_SHORT_ROW keys: insertion sort by the row's thread; longer rows are flagged for k_net_sort_long
template <typename T>
__global__ void __launch_bounds__(NB)
k_net_sort_short(const int32_t *__restrict__ ptr, int64_t n, T *key, int32_t *__restrict__ is_long) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    const int32_t b = ptr[i], L = ptr[i + 1] - b;
    is_long[i] = L > NET_SHORT_ROW;
    if (L > NET_SHORT_ROW) return;
    T *row = key + b;
    for (int p = 1; p < L; p++) {
        const T v = row[p];
        int q = p;
        for (; q > 0 && row[q - 1] > v; q--) row[q] = row[q - 1];
        row[q] = v;
    }
}

// one block per long row, any length (block_sort_ascending, xr_prims.h)
template <typename T>
__global__ void __launch_bounds__(NB)
k_net_sort_long(const int32_t *__restrict__ ptr, const int32_t *__restrict__ rows, T *key) {
    const int32_t r = rows[blockIdx.x];
    block_sort_ascending<NB>(key + ptr[r], (int64_t)ptr[r + 1] - ptr[r]);
}

// sorted node rows -> indices (the neighbour), data (the edge's length); counters[2] counts the repeated node pairs, each at the
// lower node of the pair: m edges over one pair are m equal neighbours in a row, m - 1 repeats
__global__ void __launch_bounds__(NB)
k_net_node_finish(const int32_t *__restrict__ nptr, int64_t n_node, const uint64_t *__restrict__ key,
                  const double *__restrict__ len, int32_t *__restrict__ indices, double *__restrict__ data, int32_t *counters) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    int32_t repeats = 0;
    if (i < n_node) {
        int64_t before = -1;
        for (int32_t p = nptr[i]; p < nptr[i + 1]; p++) {
            const int64_t j = (int64_t)(key[p] >> 32);
            if (indices) {
                indices[p] = (int32_t)j;
                data[p] = len[key[p] & 0xffffffffu];
            }
            repeats += j == before && i < j;
            before = j;
        }
    }
    if (repeats) atomicAdd(counters + 2, repeats);
}

// entries of the edge graph's row e: the other edges at its two nodes; their 64-bit sum
__global__ void __launch_bounds__(NB)
k_net_edge_count(const int64_t *__restrict__ edges, int64_t n_edge, const int32_t *__restrict__ nptr, int32_t *__restrict__ rowlen,
                 unsigned long long *total) {
    const int64_t e = (int64_t)blockIdx.x * NB + threadIdx.x;
    long long v = 0;
    if (e < n_edge) {
        const int64_t a = edges[2 * e], b = edges[2 * e + 1];
        v = (long long)(nptr[a + 1] - nptr[a]) + (nptr[b + 1] - nptr[b]) - 2;
        rowlen[e] = (int32_t)v;
    }
    v = wave_reduce<OpSum>(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, (unsigned long long)v);
}

// row e = the edges of node a's row but e, then those of node b's (sorted afterwards)
__global__ void __launch_bounds__(NB)
k_net_edge_fill(const int64_t *__restrict__ edges, int64_t n_edge, const int32_t *__restrict__ nptr,
                const uint64_t *__restrict__ key, const int32_t *__restrict__ eptr, int32_t *__restrict__ indices) {
    const int64_t e = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (e >= n_edge) return;
    int32_t at = eptr[e];
    const int32_t end = eptr[e + 1];
    for (int side = 0; side < 2; side++) {
        const int64_t v = edges[2 * e + side];
        for (int32_t p = nptr[v]; p < nptr[v + 1]; p++) {
            const int32_t j = (int32_t)(key[p] & 0xffffffffu);
            if (j != (int32_t)e && at < end) indices[at++] = j;
        }
    }
}

__global__ void __launch_bounds__(NB)
k_net_edge_weights(const int32_t *__restrict__ eptr, const int32_t *__restrict__ indices, int64_t n_edge,
                   const double *__restrict__ len, double *__restrict__ data) {
    const int64_t e = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (e >= n_edge) return;
    const double own = len[e];
    for (int32_t p = eptr[e]; p < eptr[e + 1]; p++) data[p] = 0.5 * (own + len[indices[p]]);
}

// every row of the CSR (ptr [n + 1], keys in place) ascending
template <typename T> static void sort_rows(const int32_t *ptr, int64_t n, T *key) {
    if (n <= 0) return;
    DevBuf<int32_t> is_long((size_t)n), pos((size_t)n + 1);
    XR_LAUNCH("net_sort_short", k_net_sort_short<T>, dim3(div_up(n, NB)), dim3(NB), 0, ptr, n, key, is_long.get());
    exclusive_scan_i32(is_long.get(), pos.get(), n);
    const int32_t n_long = read_scalar(pos.get() + n);
    if (n_long > 0) {
        DevBuf<int32_t> rows((size_t)n_long);
        XR_LAUNCH("net_long_rows", k_compact_ids<int32_t>, dim3(div_up(n, 256)), dim3(256), 0, is_long.get(), pos.get(), n, rows.get());
        XR_LAUNCH("net_sort_long", k_net_sort_long<T>, dim3((unsigned)n_long), dim3(NB), 0, ptr, rows.get(), key);
        stream_sync(); // (`rows` goes back to the pool behind its reader)
    }
}

// ---------------------------------------------------------------------------------------------
// multi-source nearest
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NB)
k_net_init_sources(const uint8_t *__restrict__ is_source, int64_t n, double *__restrict__ d, int32_t *__restrict__ s) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    const int64_t o = (int64_t)blockIdx.y * n + i;
    const bool src = is_source[o] != 0;
    d[o] = src ? 0.0 : INFINITY;
    s[o] = src ? (int32_t)i : -1;
}

// sources = the non-NaN entries; has_valid / has_null per slice
__global__ void __launch_bounds__(NB)
k_net_init_data(const double *__restrict__ in, int64_t n, double *__restrict__ d, int32_t *__restrict__ s,
                uint8_t *__restrict__ has_valid, uint8_t *__restrict__ has_null) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    const int64_t k = blockIdx.y, o = k * n + i;
    const double v = in[o];
    const bool src = v == v;
    d[o] = src ? 0.0 : INFINITY;
    s[o] = src ? (int32_t)i : -1;
    if (src) has_valid[k] = 1;
    else has_null[k] = 1;
}

// one round (see the head of the file): up to NET_SWEEPS sweeps of the block over its own NB vertices.  A sweep is a pull on a
// snapshot: a neighbour inside the block is read from the block's LDS copy as of the sweep before, any other from the previous
// round's buffer; the new states go to the other half of the LDS copy behind a barrier, so no pair is read while it is written.
// The block stops sweeping when a sweep lowered nothing.  *go == 0: the round before changed nothing, both buffers hold the
// result already.
__global__ void __launch_bounds__(NB)
k_net_round(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data, int64_t n,
            double limit, const double *__restrict__ d0, const int32_t *__restrict__ s0, double *__restrict__ d1,
            int32_t *__restrict__ s1, const int32_t *go, int32_t *changed) {
    if (!*go) return;
    __shared__ double dl[2][NB];
    __shared__ int32_t sl[2][NB];
    const int64_t first = (int64_t)blockIdx.x * NB, i = first + threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * n;
    const bool live = i < n;
    double d = live ? d0[base + i] : INFINITY;
    int32_t s = live ? s0[base + i] : -1;
    const int32_t e0 = live ? indptr[i] : 0, e1 = live ? indptr[i + 1] : 0;
    dl[0][threadIdx.x] = d;
    sl[0][threadIdx.x] = s;
    __syncthreads();
    bool lower = false;
    int cur = 0;
    for (int sweep = 0; sweep < NET_SWEEPS; sweep++) {
        bool now = false;
        for (int32_t e = e0; e < e1; e++) {
            const int64_t u = indices[e], local = u - first;
            const bool inside = local >= 0 && local < NB;
            const double du = inside ? dl[cur][local] : d0[base + u];
            if (!(du < INFINITY)) continue; // (an unreached neighbour offers nothing)
            const double c = du + data[e];
            if (!(c <= limit)) continue;
            const int32_t su = inside ? sl[cur][local] : s0[base + u];
            if (c < d || (c == d && su < s)) {
                d = c;
                s = su;
                now = true;
            }
        }
        dl[cur ^ 1][threadIdx.x] = d;
        sl[cur ^ 1][threadIdx.x] = s;
        lower |= now;
        cur ^= 1;
        if (!__syncthreads_or(now)) break; // (the same answer in every thread)
    }
    if (live) {
        d1[base + i] = d;
        s1[base + i] = s;
    }
    wave_flag(lower, changed);
}

__global__ void __launch_bounds__(NB)
k_net_report(const double *__restrict__ d, const int32_t *__restrict__ s, int64_t total, double *__restrict__ distance,
             int64_t *__restrict__ source) {
    const int64_t o = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (o >= total) return;
    if (distance) distance[o] = d[o];
    if (source) source[o] = s[o];
}

// a valid entry keeps its value; a null one takes the value at its source, NaN without one
__global__ void __launch_bounds__(NB)
k_net_gather(const double *__restrict__ in, const int32_t *__restrict__ s, int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    const int64_t base = (int64_t)blockIdx.y * n;
    double v = in[base + i];
    if (v != v) {
        const int32_t j = s[base + i];
        v = j >= 0 ? in[base + j] : NAN;
    }
    out[base + i] = v;
}

// the states of K slices: two buffers of (d, s); rounds to the fixed point from whatever `init` put into buffer 0
struct NetState {
    DevBuf<double> d;
    DevBuf<int32_t> s;
    int64_t total;
    int at = 0; // the buffer that holds the current states
    explicit NetState(int64_t total) : d((size_t)total * 2), s((size_t)total * 2), total(total) {}
    double *dist(int b) const { return d.get() + (int64_t)b * total; }
    int32_t *src(int b) const { return s.get() + (int64_t)b * total; }
};

static int64_t net_relax(const xr_graph *g, NetState &st, int64_t K, double limit, int64_t chunk) {
    const int64_t n = g->n;
    if (chunk <= 0) chunk = NET_CHUNK;
    chunk = std::min<int64_t>(chunk, 4096);
    DevBuf<int32_t> flags((size_t)chunk + 1);
    std::vector<int32_t> h((size_t)chunk + 1);
    const dim3 grid(div_up(n, NB), (unsigned)K);
    const int64_t cap = 2 * n + 4; // (every round but the last lowers a state: far fewer in any valid graph)
    int64_t rounds = 0;
    for (;;) {
        fill_i32(flags.get(), 0, chunk + 1);
        fill_i32(flags.get(), 1, 1);
        for (int64_t r = 0; r < chunk; r++) {
            XR_LAUNCH("net_round", k_net_round, grid, dim3(NB), 0, g->indptr.get(), g->indices.get(), g->data.get(), n, limit,
                      st.dist(st.at), st.src(st.at), st.dist(st.at ^ 1), st.src(st.at ^ 1), flags.get() + r, flags.get() + r + 1);
            st.at ^= 1;
        }
        d2h(h.data(), flags.get(), sizeof(int32_t) * (size_t)(chunk + 1));
        for (int64_t r = 0; r < chunk && h[(size_t)r]; r++) rounds++;
        if (!h[(size_t)chunk]) break;
        XR_REQUIRE(rounds <= cap, XR_ERR_INVALID, "xr_graph_nearest_dev: no fixed point after %lld rounds (negative weights?)",
                   (long long)rounds);
    }
    return rounds;
}

static void check_nearest_args(const char *who, const xr_graph *g, int64_t K, double limit) {
    XR_REQUIRE(g, XR_ERR_INVALID, "%s: NULL handle", who);
    XR_REQUIRE(K >= 0 && K < 65536, XR_ERR_INVALID, "%s: K must be in [0, 65536)", who);
    XR_REQUIRE(g->has_data, XR_ERR_INVALID, "%s: the graph has no weights", who);
    XR_REQUIRE(limit >= 0.0, XR_ERR_INVALID, "%s: limit must be non-negative", who);
    XR_REQUIRE(g->n * std::max<int64_t>(K, 1) < ((int64_t)1 << 40), XR_ERR_LIMIT, "%s: too many states", who);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_network_graph_dev(const double *node_xy_dev, int64_t n_node, const int64_t *edges_dev, int64_t n_edge, int facet,
                         xr_graph **out, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(out && problems, XR_ERR_INVALID, "xr_network_graph_dev: NULL argument");
    *out = nullptr;
    problems[0] = problems[1] = 0;
    XR_REQUIRE(facet == XR_FACET_NODE || facet == XR_FACET_EDGE, XR_ERR_INVALID,
               "xr_network_graph_dev: facet must be XR_FACET_NODE or XR_FACET_EDGE");
    XR_REQUIRE(n_node >= 0 && n_edge >= 0, XR_ERR_INVALID, "xr_network_graph_dev: negative size");
    XR_REQUIRE((node_xy_dev || n_node == 0) && (edges_dev || n_edge == 0), XR_ERR_INVALID, "xr_network_graph_dev: NULL argument");
    XR_REQUIRE(n_node < INT32_MAX && 2 * n_edge < INT32_MAX, XR_ERR_LIMIT, "xr_network_graph_dev: more than 2^31 rows or entries");
    const bool by_edge = facet == XR_FACET_EDGE;
    Building<xr_graph> g(OnFailure::WaitFirst);

    // the node table: degrees -> row starts -> (neighbour, edge) keys, every row ascending
    DevBuf<int32_t> deg((size_t)n_node + 1), nptr((size_t)n_node + 1), counters(3);
    DevBuf<double> len((size_t)std::max<int64_t>(n_edge, 1));
    fill_i32(deg.get(), 0, n_node + 1);
    fill_i32(counters.get(), 0, 3);
    if (n_edge > 0)
        XR_LAUNCH("net_degree", k_net_degree, dim3(div_up(n_edge, NB)), dim3(NB), 0, edges_dev, n_edge, n_node, node_xy_dev,
                  deg.get(), len.get(), counters.get());
    int32_t h_count[3];
    d2h(h_count, counters.get(), sizeof(h_count));
    XR_REQUIRE(h_count[0] == 0, XR_ERR_INVALID, "xr_network_graph_dev: %d edges name nodes that do not exist", (int)h_count[0]);
    if (n_node > 0) exclusive_scan_i32(deg.get(), nptr.get(), n_node);
    else fill_i32(nptr.get(), 0, 1);
    const int64_t nn_nnz = 2 * (n_edge - h_count[1]);
    DevBuf<uint64_t> key((size_t)std::max<int64_t>(nn_nnz, 1));
    if (n_edge > 0) {
        fill_i32(deg.get(), 0, n_node + 1); // (the degrees are in nptr now: the words serve as the rows' cursors)
        XR_LAUNCH("net_node_fill", k_net_node_fill, dim3(div_up(n_edge, NB)), dim3(NB), 0, edges_dev, n_edge, nptr.get(), deg.get(),
                  key.get());
        sort_rows(nptr.get(), n_node, key.get());
    }
    if (!by_edge) {
        g->n = n_node, g->nnz = nn_nnz;
        g->indptr.alloc((size_t)n_node + 1);
        g->indices.alloc((size_t)std::max<int64_t>(nn_nnz, 1));
        g->data.alloc((size_t)std::max<int64_t>(nn_nnz, 1));
        XR_HIP(hipMemcpyAsync(g->indptr.get(), nptr.get(), sizeof(int32_t) * (size_t)(n_node + 1), hipMemcpyDeviceToDevice,
                              launch_stream()));
    }
    if (n_node > 0)
        XR_LAUNCH("net_node_finish", k_net_node_finish, dim3(div_up(n_node, NB)), dim3(NB), 0, nptr.get(), n_node, key.get(), len.get(),
                  by_edge ? nullptr : g->indices.get(), by_edge ? nullptr : g->data.get(), counters.get());
    d2h(h_count, counters.get(), sizeof(h_count));
    problems[0] = h_count[1], problems[1] = h_count[2];
    if (problems[0] || problems[1]) return XR_OK; // (the Building frees what was made; *out stays NULL)

    if (by_edge) {
        DevBuf<int32_t> rowlen((size_t)std::max<int64_t>(n_edge, 1));
        DevBuf<unsigned long long> total(1);
        XR_HIP(hipMemsetAsync(total.get(), 0, sizeof(unsigned long long), launch_stream()));
        g->n = n_edge;
        g->indptr.alloc((size_t)n_edge + 1);
        if (n_edge > 0)
            XR_LAUNCH("net_edge_count", k_net_edge_count, dim3(div_up(n_edge, NB)), dim3(NB), 0, edges_dev, n_edge, nptr.get(),
                      rowlen.get(), total.get());
        const unsigned long long ee_nnz = read_scalar(total.get());
        XR_REQUIRE(ee_nnz < (unsigned long long)INT32_MAX, XR_ERR_LIMIT, "xr_network_graph_dev: the edge graph has %llu entries, more than 2^31",
                   ee_nnz);
        g->nnz = (int64_t)ee_nnz;
        g->indices.alloc((size_t)std::max<int64_t>(g->nnz, 1));
        g->data.alloc((size_t)std::max<int64_t>(g->nnz, 1));
        if (n_edge > 0) {
            exclusive_scan_i32(rowlen.get(), g->indptr.get(), n_edge);
            XR_LAUNCH("net_edge_fill", k_net_edge_fill, dim3(div_up(n_edge, NB)), dim3(NB), 0, edges_dev, n_edge, nptr.get(), key.get(),
                      g->indptr.get(), g->indices.get());
            sort_rows(g->indptr.get(), n_edge, g->indices.get());
            XR_LAUNCH("net_edge_weights", k_net_edge_weights, dim3(div_up(n_edge, NB)), dim3(NB), 0, g->indptr.get(), g->indices.get(),
                      n_edge, len.get(), g->data.get());
        } else {
            fill_i32(g->indptr.get(), 0, 1);
        }
    }
    g->has_data = true;
    g->labels.alloc((size_t)std::max<int64_t>(g->n, 1));
    label_components(g.get());
    stream_sync();
    *out = g.release();
    XR_API_END
}

int xr_graph_nearest_dev(const xr_graph *g, const uint8_t *is_source_dev, int64_t K, double limit, int64_t chunk,
                         double *distance_dev, int64_t *source_dev, int64_t *rounds_out) {
    XR_API_BEGIN
    check_nearest_args("xr_graph_nearest_dev", g, K, limit);
    if (rounds_out) *rounds_out = 0;
    const int64_t n = g->n, total = n * K;
    XR_REQUIRE(is_source_dev || total == 0, XR_ERR_INVALID, "xr_graph_nearest_dev: NULL sources");
    if (total > 0) {
        NetState st(total);
        XR_LAUNCH("net_init_sources", k_net_init_sources, dim3(div_up(n, NB), (unsigned)K), dim3(NB), 0, is_source_dev, n, st.dist(0),
                  st.src(0));
        const int64_t rounds = net_relax(g, st, K, limit, chunk);
        if (rounds_out) *rounds_out = rounds;
        XR_LAUNCH("net_report", k_net_report, dim3(div_up(total, NB)), dim3(NB), 0, st.dist(st.at), st.src(st.at), total, distance_dev,
                  source_dev);
        stream_sync(); // (the states go back to the pool behind their last reader)
    }
    dev_call_done();
    XR_API_END
}

int xr_graph_nearest_fill_dev(const xr_graph *g, const double *in_dev, double *out_dev, int64_t K, double limit, int64_t chunk,
                              int64_t *rounds_out) {
    XR_API_BEGIN
    check_nearest_args("xr_graph_nearest_fill_dev", g, K, limit);
    if (rounds_out) *rounds_out = 0;
    const int64_t n = g->n, total = n * K;
    XR_REQUIRE((in_dev && out_dev) || total == 0, XR_ERR_INVALID, "xr_graph_nearest_fill_dev: NULL data");
    if (total > 0) {
        NetState st(total);
        DevBuf<uint8_t> has((size_t)K * 2);
        std::vector<uint8_t> h_has((size_t)K * 2);
        const dim3 grid(div_up(n, NB), (unsigned)K);
        XR_HIP(hipMemsetAsync(has.get(), 0, has.bytes(), launch_stream()));
        XR_LAUNCH("net_init_data", k_net_init_data, grid, dim3(NB), 0, in_dev, n, st.dist(0), st.src(0), has.get(), has.get() + K);
        d2h(h_has.data(), has.get(), has.bytes());
        bool any_null = false;
        for (int64_t k = 0; k < K; k++) {
            XR_REQUIRE(h_has[(size_t)k], XR_ERR_INVALID, "All values are NA.");
            any_null |= h_has[(size_t)(K + k)] != 0;
        }
        if (any_null) { // (without a NaN anywhere every state is a source's already)
            const int64_t rounds = net_relax(g, st, K, limit, chunk);
            if (rounds_out) *rounds_out = rounds;
        }
        XR_LAUNCH("net_gather", k_net_gather, grid, dim3(NB), 0, in_dev, st.src(st.at), n, out_dev);
        stream_sync(); // (the states go back to the pool behind their last reader)
    }
    dev_call_done();
    XR_API_END
}

} // extern "C"
