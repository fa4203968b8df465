// xr_rcm.hip -- renumbering the rows of a symmetric adjacency where it is: scipy.sparse.csgraph.reverse_cuthill_mckee
// (Ugrid2d.reverse_cuthill_mckee, xugrid/ugrid/ugrid2d.py:1734-1756), and the face table gathered by the new order.  DESIGN
// section 20.
//
// The rule (restated in include/xugrid_amd.h).  degree = entries of the row, plus one where the row holds its diagonal.  scipy
// walks a sequential breadth-first search: the seed is the first unvisited vertex in the order of ascending degree, every
// visited row appends its unvisited neighbours in stored column order, the new entries of that one row are insertion-sorted by
// degree (stable), a new seed follows whenever a component is exhausted, and the order is reversed at the end.  Here the
// seeds are taken in (degree, id) order -- the stable sort; numpy's default argsort, which scipy uses, places equal degrees as
// its sort kernel happens to -- and the search runs level by level:
//   every unvisited neighbour j of level L takes as parent the smallest POSITION in the order among its neighbours in level L;
//   level L + 1 is the claimed vertices sorted by (parent position, degree[j], j).
// For rows with ascending columns that is the sequential search, element for element.  The claim is an integer minimum, so
// the result does not depend on the order in which threads arrive.
//
// One level is four launches on state that stays in HBM (order, pos, parent, degree, the vertex list in seed order with its
// cursor, the bounds of the level, the keys of the level being placed):
//   claim  atomicMin(parent[j], own position) for the unvisited neighbours j of every vertex of the level
//   count  the children each vertex won (parent[j] == its position)
//   next   one block: the exclusive scan of the counts gives every parent its slots behind the level; with no child at all
//          the component is exhausted and the cursor moves on to the next unvisited vertex of the seed list -- it never
//          moves back, so all seeds together cost one pass over the list, and a seed without unvisited neighbours (an
//          isolated face) is followed by the next one in the same launch
//   place  every parent writes its children's (degree, id) keys into its slots and sorts them: one thread per row of up to
//          RCM_SHORT_ROW entries, the whole block for a longer one (any length: the network of block_sort_ascending)
// The host enqueues RCM_CHUNK levels and reads one word; a launch behind the last level returns at once.  No kernel waits for
// another block: nothing here can hang.
#include <algorithm>

#include "xr_objects.h"
#include "xr_prims.h"

namespace xr {

static constexpr int RB = 256;              // threads per block of every kernel here
static constexpr int RCM_SHORT_ROW = 32;    // rows up to this many entries are walked by one thread, longer ones by their block
static constexpr int RCM_GRID = 1024;       // blocks of a level kernel at most (a wider level takes several turns)
static constexpr int64_t RCM_CHUNK = 64;    // levels between two reads of the "done" word
static constexpr int32_t RCM_NONE = INT32_MAX; // parent of a vertex nobody has claimed

// the control words: the bounds [begin, end) of the level of either parity, then
enum RcmWord : int { RW_CURSOR = 4, RW_LEVELS = 5, RW_CHILDREN = 6, RW_DONE = 7, RW_MAXDEG = 8, RW_COUNT = 9 };

// degree (row length + 1 with a diagonal entry: columns ascend, so a binary search finds it), pos = -1, parent = none, the
// identity as the first list of the radix passes, the largest degree
__global__ void __launch_bounds__(RB)
k_rcm_init(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n, int32_t *__restrict__ deg,
           int32_t *__restrict__ pos, int32_t *__restrict__ parent, int32_t *__restrict__ ids, int32_t *ctl) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    int32_t d = 0;
    if (i < n) {
        int32_t lo = indptr[i], hi = indptr[i + 1];
        d = hi - lo;
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (indices[mid] < (int32_t)i) lo = mid + 1;
            else hi = mid;
        }
        if (lo < indptr[i + 1] && indices[lo] == (int32_t)i) d++;
        deg[i] = d;
        pos[i] = -1;
        parent[i] = RCM_NONE;
        ids[i] = (int32_t)i;
    }
    d = wave_reduce<OpMax>(d);
    if ((threadIdx.x & 63) == 0 && d > 0) atomicMax(ctl + RW_MAXDEG, d);
}

// one stable pass of the sort of the seed list on bit `bit` of the degree: flag = the bit is clear
__global__ void __launch_bounds__(RB)
k_rcm_bit_flag(const int32_t *__restrict__ ids, const int32_t *__restrict__ deg, int64_t n, int bit, int32_t *__restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (k < n) flag[k] = !((deg[ids[k]] >> bit) & 1);
}
// ... the vertices with the bit clear first, either group in the order it had (rank = exclusive scan of flag, rank[n] = zeros)
__global__ void __launch_bounds__(RB)
k_rcm_bit_split(const int32_t *__restrict__ ids, const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n,
                int32_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (k >= n) return;
    const int32_t r = rank[k];
    out[flag[k] ? (int64_t)r : (int64_t)rank[n] + (k - r)] = ids[k];
}

// The vertices of the level [b, e) of `order`, one thread each, RB consecutive positions per block and turn: short(q, u) for a
// row of up to RCM_SHORT_ROW entries by its thread, wide(q, u) for a longer one by the whole block (every thread of the block
// calls it with the same arguments; it may use barriers).
template <typename SHORT, typename WIDE>
__device__ __forceinline__ void rcm_level_rows(const int32_t *__restrict__ indptr, const int32_t *order, int32_t b,
                                               int32_t e, SHORT &&do_short, WIDE &&do_wide) {
    __shared__ int32_t wide_q[RB];
    __shared__ int32_t n_wide;
    for (int64_t base = (int64_t)b + (int64_t)blockIdx.x * RB; base < e; base += (int64_t)gridDim.x * RB) { // (the same trips for the whole block)
        if (threadIdx.x == 0) n_wide = 0;
        __syncthreads();
        const int64_t q = base + threadIdx.x;
        if (q < e) {
            const int32_t u = order[q];
            if (indptr[u + 1] - indptr[u] <= RCM_SHORT_ROW) do_short((int32_t)q, u);
            else wide_q[atomicAdd(&n_wide, 1)] = (int32_t)q;
        }
        __syncthreads();
        const int32_t nw = n_wide;
        for (int32_t k = 0; k < nw; k++) do_wide(wide_q[k], order[wide_q[k]]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(RB)
k_rcm_claim(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ order,
            const int32_t *__restrict__ pos, int32_t *parent, const int32_t *__restrict__ ctl, int parity) {
    if (ctl[RW_DONE]) return;
    auto claim = [&](int32_t q, int32_t u, int first, int step) {
        for (int32_t p = indptr[u] + first; p < indptr[u + 1]; p += step) {
            const int32_t j = indices[p];
            if (pos[j] < 0) atomicMin(parent + j, q);
        }
    };
    rcm_level_rows(indptr, order, ctl[2 * parity], ctl[2 * parity + 1], [&](int32_t q, int32_t u) { claim(q, u, 0, 1); },
                   [&](int32_t q, int32_t u) { claim(q, u, (int)threadIdx.x, RB); });
}

// the column of entry p if it is a child of the vertex at position q, else -1.  An entry that repeats the one before it (rows
// ascend) is no second child: the counts, and with them the slots, stay within the n vertices whatever the caller stored.
__device__ __forceinline__ int32_t rcm_child(int32_t row_start, const int32_t *__restrict__ indices, const int32_t *__restrict__ parent,
                                             int32_t p, int32_t q) {
    const int32_t j = indices[p];
    return parent[j] == q && (p == row_start || indices[p - 1] != j) ? j : -1;
}

// count[q] = the children of the vertex at position q.  parent[j] == q holds for exactly the vertices this level's claim gave
// to q: positions are unique over the whole run, and a vertex is placed in the level in which it is claimed.
__global__ void __launch_bounds__(RB)
k_rcm_count(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ order,
            const int32_t *__restrict__ parent, int32_t *__restrict__ count, const int32_t *__restrict__ ctl, int parity) {
    if (ctl[RW_DONE]) return;
    __shared__ int lds[RB / 64];
    auto children = [&](int32_t q, int32_t u, int first, int step) {
        int32_t c = 0;
        for (int32_t p = indptr[u] + first; p < indptr[u + 1]; p += step) c += rcm_child(indptr[u], indices, parent, p, q) >= 0;
        return c;
    };
    rcm_level_rows(indptr, order, ctl[2 * parity], ctl[2 * parity + 1], [&](int32_t q, int32_t u) { count[q] = children(q, u, 0, 1); },
                   [&](int32_t q, int32_t u) {
                       int total;
                       (void)block_excl_scan<RB>(children(q, u, (int)threadIdx.x, RB), &total, lds);
                       if (threadIdx.x == 0) count[q] = total;
                   });
}

// One block.  slot[q] = first position of the children of the vertex at q: the level's end plus the exclusive scan of the
// counts; the next level is [end, end + children).  Without children the component is exhausted: seeds are placed from the
// list (sorted by (degree, id)) at the cursor until one has an unvisited neighbour or every vertex is placed; with nothing
// left to place, done.
__global__ void __launch_bounds__(RB)
k_rcm_next(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ seeds, int64_t n,
           const int32_t *__restrict__ count, int32_t *__restrict__ slot, int32_t *__restrict__ order, int32_t *pos, int32_t *ctl,
           int parity) {
    if (ctl[RW_DONE]) return;
    __shared__ int lds[RB / 64];
    __shared__ int32_t found;
    const int32_t b = ctl[2 * parity], e = ctl[2 * parity + 1];
    int32_t carry = 0;
    for (int64_t base = b; base < e; base += RB) {
        const int64_t q = base + threadIdx.x;
        int total;
        const int ex = block_excl_scan<RB>(q < e ? count[q] : 0, &total, lds);
        if (q < e) slot[q] = e + carry + ex;
        carry += total;
    }
    int32_t *next = ctl + 2 * (parity ^ 1);
    if (carry > 0) {
        if (threadIdx.x == 0) {
            next[0] = e, next[1] = e + carry;
            ctl[RW_CHILDREN] = carry;
            ctl[RW_LEVELS] += 1;
        }
        return;
    }
    int32_t placed = e, levels = 0; // (`order` is full up to the end of the newest level)
    int64_t cursor = ctl[RW_CURSOR];
    bool open = false;
    while (placed < n && !open) {
        int32_t first = RCM_NONE; // the first unvisited vertex of the list at or behind the cursor: there is one while placed < n
        while (cursor < n) {
            if (threadIdx.x == 0) found = RCM_NONE;
            __syncthreads();
            const int64_t k = cursor + threadIdx.x;
            if (k < n && pos[seeds[k]] < 0) atomicMin(&found, (int32_t)k);
            __syncthreads();
            first = found;
            __syncthreads();
            if (first != RCM_NONE) break;
            cursor += RB;
        }
        if (first == RCM_NONE) break; // (not reached while placed < n; keeps the loop finite whatever the state)
        cursor = first;
        const int32_t v = seeds[cursor++];
        if (threadIdx.x == 0) {
            order[placed] = v;
            pos[v] = placed;
        }
        __syncthreads(); // (the neighbour test below reads pos[v] for a diagonal entry)
        bool any = false;
        for (int32_t p = indptr[v] + (int32_t)threadIdx.x; p < indptr[v + 1] && !any; p += RB) any = pos[indices[p]] < 0;
        open = __syncthreads_or(any);
        placed++, levels++;
    }
    if (threadIdx.x == 0) {
        next[0] = placed - (open ? 1 : 0), next[1] = placed;
        ctl[RW_CURSOR] = (int32_t)(cursor < n ? cursor : n);
        ctl[RW_CHILDREN] = 0;
        ctl[RW_LEVELS] += levels;
        if (!open) ctl[RW_DONE] = 1; // every vertex is placed (or, in a broken state, none can be found)
    }
}

// the children of every vertex of the level into its slots, ascending by (degree, id); keys [n] holds them meanwhile
__global__ void __launch_bounds__(RB)
k_rcm_place(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ deg,
            const int32_t *__restrict__ parent, const int32_t *__restrict__ slot, uint64_t *keys, int32_t *order, int32_t *pos,
            const int32_t *__restrict__ ctl, int parity) {
    if (ctl[RW_DONE] || ctl[RW_CHILDREN] == 0) return;
    __shared__ int32_t n_child;
    auto key_of = [&](int32_t j) { return ((uint64_t)(uint32_t)deg[j] << 32) | (uint32_t)j; };
    auto put = [&](int64_t at, uint64_t key) {
        const int32_t j = (int32_t)(key & 0xffffffffu);
        order[at] = j;
        pos[j] = (int32_t)at;
    };
    rcm_level_rows(
        indptr, order, ctl[2 * parity], ctl[2 * parity + 1],
        [&](int32_t q, int32_t u) { // the children arrive by ascending id: the insertion sort on the whole key is scipy's stable one on the degree
            uint64_t *row = keys + slot[q];
            int c = 0;
            for (int32_t p = indptr[u]; p < indptr[u + 1]; p++) {
                const int32_t j = rcm_child(indptr[u], indices, parent, p, q);
                if (j < 0) continue;
                const uint64_t v = key_of(j);
                int k = c++;
                for (; k > 0 && row[k - 1] > v; k--) row[k] = row[k - 1];
                row[k] = v;
            }
            for (int k = 0; k < c; k++) put((int64_t)slot[q] + k, row[k]);
        },
        [&](int32_t q, int32_t u) {
            uint64_t *row = keys + slot[q];
            if (threadIdx.x == 0) n_child = 0;
            __syncthreads();
            for (int32_t p = indptr[u] + (int32_t)threadIdx.x; p < indptr[u + 1]; p += RB) {
                const int32_t j = rcm_child(indptr[u], indices, parent, p, q);
                if (j >= 0) row[atomicAdd(&n_child, 1)] = key_of(j); // (in any order: the keys are distinct and sorted next)
            }
            __syncthreads();
            const int32_t c = n_child;
            block_sort_ascending<RB>(row, (int64_t)c);
            __syncthreads();
            for (int32_t k = (int32_t)threadIdx.x; k < c; k += RB) put((int64_t)slot[q] + k, row[k]);
        });
}

__global__ void __launch_bounds__(RB) k_rcm_reverse(const int32_t *__restrict__ order, int64_t n, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (i < n) out[i] = order[n - 1 - i];
}

// out[i, :] = faces[order[i], :]; ids outside [0, n_face) are counted and read nothing
__global__ void __launch_bounds__(RB)
k_rcm_gather_faces(const int32_t *__restrict__ faces, int64_t n_face, int m, const int64_t *__restrict__ order, int32_t *__restrict__ out,
                   int32_t *bad) {
    const int64_t t = (int64_t)blockIdx.x * RB + threadIdx.x;
    bool wrong = false;
    if (t < n_face * m) {
        const int64_t i = t / m, f = order[i];
        wrong = f < 0 || f >= n_face;
        out[t] = wrong ? -1 : faces[f * m + (t - i * m)];
    }
    wave_count(wrong, bad);
}

static int64_t rcm_order(const xr_graph *g, int64_t *order_dev) {
    const int64_t n = g->n;
    const int32_t *indptr = g->indptr.get(), *indices = g->indices.get();
    const unsigned nb = div_up(n, RB);
    // one block of words: [deg][pos][parent][order][count][slot][list a][list b][flag][rank: n + 1][ctl]
    DevBuf<int32_t> work((size_t)(10 * n + 1 + RW_COUNT));
    DevBuf<uint64_t> keys((size_t)n);
    int32_t *deg = work.get(), *pos = deg + n, *parent = pos + n, *order = parent + n, *count = order + n, *slot = count + n;
    int32_t *list[2] = {slot + n, slot + 2 * n}, *flag = slot + 3 * n, *rank = flag + n, *ctl = rank + n + 1;
    fill_i32(ctl, 0, RW_COUNT);
    XR_LAUNCH("rcm_init", k_rcm_init, dim3(nb), dim3(RB), 0, indptr, indices, n, deg, pos, parent, list[0], ctl);
    // the seed list: a stable counting sort on every bit of the degree, the lowest first, leaves (degree, id) order
    const int32_t max_degree = read_scalar(ctl + RW_MAXDEG);
    int at = 0;
    for (int bit = 0; bit < 31 && (max_degree >> bit); bit++) {
        XR_LAUNCH("rcm_bit_flag", k_rcm_bit_flag, dim3(nb), dim3(RB), 0, list[at], deg, n, bit, flag);
        exclusive_scan_i32(flag, rank, n);
        XR_LAUNCH("rcm_bit_split", k_rcm_bit_split, dim3(nb), dim3(RB), 0, list[at], flag, rank, n, list[at ^ 1]);
        at ^= 1;
    }
    const dim3 grid(std::min<unsigned>(nb, RCM_GRID));
    int32_t h[RW_COUNT];
    int64_t rounds = 0;
    for (;;) { // (the first level is empty: its `next` places the first seed)
        for (int64_t r = 0; r < RCM_CHUNK; r++, rounds++) {
            const int parity = (int)(rounds & 1);
            XR_LAUNCH("rcm_claim", k_rcm_claim, grid, dim3(RB), 0, indptr, indices, order, pos, parent, ctl, parity);
            XR_LAUNCH("rcm_count", k_rcm_count, grid, dim3(RB), 0, indptr, indices, order, parent, count, ctl, parity);
            XR_LAUNCH("rcm_next", k_rcm_next, dim3(1), dim3(RB), 0, indptr, indices, list[at], n, count, slot, order, pos, ctl, parity);
            XR_LAUNCH("rcm_place", k_rcm_place, grid, dim3(RB), 0, indptr, indices, deg, parent, slot, keys.get(), order, pos, ctl,
                      parity);
        }
        d2h(h, ctl, sizeof(h));
        if (h[RW_DONE]) break;
        XR_REQUIRE(rounds <= n + 1 + RCM_CHUNK, XR_ERR_INVALID, "xr_graph_rcm_dev: %lld levels for %lld rows (is the adjacency symmetric?)",
                   (long long)rounds, (long long)n); // (every level but the first places a vertex)
    }
    const int32_t placed = std::max(h[1], h[3]); // the end of the newest level
    XR_REQUIRE(placed == n, XR_ERR_INVALID, "xr_graph_rcm_dev: %d of %lld rows placed", (int)placed, (long long)n);
    XR_LAUNCH("rcm_reverse", k_rcm_reverse, dim3(nb), dim3(RB), 0, order, n, order_dev);
    stream_sync(); // (the state goes back to the pool behind its last reader)
    return h[RW_LEVELS];
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_graph_rcm_dev(const xr_graph *g, int64_t *order_dev, int64_t *levels_out) {
    XR_API_BEGIN
    XR_REQUIRE(g && (order_dev || g->n == 0), XR_ERR_INVALID, "xr_graph_rcm_dev: NULL argument");
    const int64_t levels = g->n > 0 ? rcm_order(g, order_dev) : 0;
    if (levels_out) *levels_out = levels;
    dev_call_done();
    XR_API_END
}

int xr_mesh_reorder_faces_dev(const xr_mesh *mesh, const int64_t *order_dev, xr_mesh **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out && (order_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_mesh_reorder_faces_dev: NULL argument");
    *out = nullptr;
    const int64_t F = mesh->n_face, N = mesh->n_node;
    const int m = mesh->m;
    Building<xr_mesh> made = new_raw_mesh(N, F, m, OnFailure::WaitFirst);
    if (N > 0)
        XR_HIP(hipMemcpyAsync(made->node_xy.get(), mesh->node_xy.get(), sizeof(double) * (size_t)N * 2, hipMemcpyDeviceToDevice,
                              launch_stream()));
    if (F * m > 0) {
        DevBuf<int32_t> bad(1);
        fill_i32(bad.get(), 0, 1);
        XR_LAUNCH("rcm_gather_faces", k_rcm_gather_faces, dim3(div_up(F * m, RB)), dim3(RB), 0, mesh->faces_raw.get(), F, m, order_dev,
                  made->faces_raw.get(), bad.get());
        const int32_t n_bad = read_scalar(bad.get());
        XR_REQUIRE(n_bad == 0, XR_ERR_INVALID, "xr_mesh_reorder_faces_dev: the order names faces that do not exist");
    }
    stream_sync();
    *out = made.release();
    XR_API_END
}

} // extern "C"
