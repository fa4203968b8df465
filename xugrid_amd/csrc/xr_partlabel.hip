// xr_partlabel.hip -- balanced part labels for the vertices of a symmetric adjacency where it is (Ugrid2d.label_partitions /
// partition, xugrid/ugrid/ugridbase.py:1508-1596; the reference hands the graph to METIS, whose output is not a function one
// can specify).  DESIGN section 22.
//
// The rule (restated in include/xugrid_amd.h: xr_graph_partition_dev; numpy: tests/partlabel_cases.py).
//   key     the 32-bit Hilbert index of the vertex' cell in a 65536 x 65536 raster over the bounds of all coordinates
//   seed    the vertices in (key, id) order, cut where the weight in front of a vertex reaches the next multiple of T / P
//   rounds  at most PL_MAX_ROUNDS synchronous rounds on a snapshot of the labels: every vertex names the other label most of
//           its neighbours carry; it moves when that lowers the cut, when no neighbour wants to move with a higher priority
//           (gain descending, id ascending: movers are an independent set) and when the weight the round's movers bring to the
//           destination and take from the source, summed in priority order, stays within the bounds L and Lmin
// Everything that decides a label is integer arithmetic, an integer sum or an order-independent minimum / maximum: the labels
// do not depend on the order in which threads arrive.
//
// How the orders are obtained: stable bit-split passes (flag, exclusive scan, split), the lowest bit first, over a list of
// vertex ids -- 32 passes on the key for the seed; per round the movers are compacted in id order, split on the bits of the
// gain, and that list is split once on the bits of the destination and once on those of the source label.  The weights along
// a sorted list go through an int64 exclusive scan, and a vertex finds the start of its label's run by bisection.
// A round is a fixed chain of launches on state that stays in HBM; its kernels return at once behind the last round, the host
// enqueues PL_CHUNK rounds and reads the control words once per chunk.  No kernel waits for another block.
#include <algorithm>

#include "xr_objects.h"
#include "xr_prims.h"

namespace xr {

static constexpr int PB = 256;            // threads per block of every kernel here
static constexpr int PL_SHORT_ROW = 32;   // rows up to this many entries are walked by one thread, longer ones by their block
static constexpr int PL_MAX_ROUNDS = 16;  // refinement rounds at most
static constexpr int64_t PL_EPS_NUM = 3, PL_EPS_DEN = 100; // EPS = 3 / 100: a part may weigh 1.03 T / P (the k-way default of METIS)
static constexpr int PL_CHUNK = 4;        // rounds between two reads of the control words
static constexpr uint32_t PL_CELLS = 65536; // cells per axis of the curve's raster

enum PlWord : int { PW_DONE, PW_ROUNDS, PW_MOVES, PW_ROUND_MOVES, PW_MOVERS, PW_N, PW_COUNT };
enum PlWide : int { PA_TOTAL, PA_MAXDEG, PA_CUT_SEED, PA_CUT_RESULT, PA_COUNT };

__device__ __forceinline__ int64_t pl_weight(const int64_t *__restrict__ w, int32_t v) { return w ? w[v] : 1; }

// ---- int64 exclusive scan over a device array: tiles of PB, the tiles' totals by one block, the totals added back ----------------
__global__ void __launch_bounds__(PB)
k_pl_scan_tiles(const int64_t *__restrict__ in, int64_t n, int64_t *__restrict__ out, int64_t *__restrict__ tile_total) {
    __shared__ long long lds[PB / 64];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    long long total;
    const long long ex = block_excl_scan<PB, long long>(i < n ? in[i] : 0, &total, lds);
    if (i < n) out[i] = ex;
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}
__global__ void __launch_bounds__(PB) k_pl_scan_totals(int64_t *tile_total, int64_t n_tile) {
    __shared__ long long lds[PB / 64];
    long long carry = 0;
    for (int64_t base = 0; base < n_tile; base += PB) {
        const int64_t t = base + threadIdx.x;
        long long total;
        const long long ex = block_excl_scan<PB, long long>(t < n_tile ? tile_total[t] : 0, &total, lds);
        if (t < n_tile) tile_total[t] = carry + ex;
        carry += total;
    }
}
__global__ void __launch_bounds__(PB) k_pl_scan_add(int64_t *__restrict__ out, int64_t n, const int64_t *__restrict__ tile_total) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i < n) out[i] += tile_total[blockIdx.x];
}

static void exclusive_scan_i64(const int64_t *in, int64_t *out, int64_t n, int64_t *tile_total) {
    const unsigned nb = div_up(n, PB);
    XR_LAUNCH("pl_scan_tiles", k_pl_scan_tiles, dim3(nb), dim3(PB), 0, in, n, out, tile_total);
    XR_LAUNCH("pl_scan_totals", k_pl_scan_totals, dim3(1), dim3(PB), 0, tile_total, (int64_t)nb);
    XR_LAUNCH("pl_scan_add", k_pl_scan_add, dim3(nb), dim3(PB), 0, out, n, tile_total);
}

// ---- the stable bit-split pass over the first *limit entries of a list of vertex ids --------------------------------------------
// flag = bit `bit` of (key[id] ^ flip) is clear; zero behind the limit
__global__ void __launch_bounds__(PB)
k_pl_bit_flag(const int32_t *__restrict__ list, const int32_t *__restrict__ key, const int32_t *__restrict__ limit, int64_t n,
              uint32_t flip, int bit, int32_t *__restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (k < n) flag[k] = k < *limit ? !((((uint32_t)key[list[k]] ^ flip) >> bit) & 1u) : 0;
}
// ... the ids with the bit clear first, either group in the order it had (rank = exclusive scan of flag, rank[n] = the clear ones)
__global__ void __launch_bounds__(PB)
k_pl_bit_split(const int32_t *__restrict__ list, const int32_t *__restrict__ flag, const int32_t *__restrict__ rank,
               const int32_t *__restrict__ limit, int64_t n, int32_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (k >= n || k >= *limit) return;
    const int32_t r = rank[k];
    out[flag[k] ? (int64_t)r : (int64_t)rank[n] + (k - r)] = list[k]; // (a position in front of the limit: the two groups fill [0, limit))
}

struct PlSort {
    int64_t n;
    int32_t *flag, *rank, *spare[2]; // flag [n], rank [n + 1], two lists [n] that passes may write
    // `list` ordered by the lowest `bits` bits of key ^ flip, stable -> the list that holds the result (`list` itself is only read)
    int32_t *run(int32_t *list, const int32_t *key, uint32_t flip, int bits, const int32_t *limit) const {
        const unsigned nb = div_up(n, PB);
        for (int bit = 0; bit < bits; bit++) {
            int32_t *out = list == spare[0] ? spare[1] : spare[0];
            XR_LAUNCH("pl_bit_flag", k_pl_bit_flag, dim3(nb), dim3(PB), 0, list, key, limit, n, flip, bit, flag);
            exclusive_scan_i32(flag, rank, n);
            XR_LAUNCH("pl_bit_split", k_pl_bit_split, dim3(nb), dim3(PB), 0, list, flag, rank, limit, n, out);
            list = out;
        }
        return list;
    }
};

static int bits_of(int64_t v) {
    int b = 0;
    while (b < 31 && (v >> b)) b++;
    return b;
}

// ---- every vertex, one thread each: short(v) for a row of up to PL_SHORT_ROW entries by its thread, wide(v) for a longer one by
// the whole block (every thread of the block calls it with the same v; it may use barriers)
template <typename SHORT, typename WIDE>
__device__ __forceinline__ void pl_rows(const int32_t *__restrict__ indptr, int64_t n, SHORT &&do_short, WIDE &&do_wide) {
    __shared__ int32_t wide_v[PB];
    __shared__ int32_t n_wide;
    if (threadIdx.x == 0) n_wide = 0;
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (v < n) {
        if (indptr[v + 1] - indptr[v] <= PL_SHORT_ROW) do_short((int32_t)v);
        else wide_v[atomicAdd(&n_wide, 1)] = (int32_t)v; // (in any order: a row's result does not depend on the others')
    }
    __syncthreads();
    const int32_t nw = n_wide;
    for (int32_t k = 0; k < nw; k++) do_wide(wide_v[k]);
}

// ---- the seed -------------------------------------------------------------------------------------------------------------------
// the identity list, the largest row, the total weight; per block the bounds of its coordinates
__global__ void __launch_bounds__(PB)
k_pl_init(const int32_t *__restrict__ indptr, const double *__restrict__ xy, const int64_t *__restrict__ w, int64_t n,
          int32_t *__restrict__ ids, double *__restrict__ tile_bounds, unsigned long long *wide) {
    __shared__ double red[4 * (PB / 64)];
    __shared__ int32_t red_deg[PB / 64];
    __shared__ long long red_weight[PB / 64];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    int32_t deg = 0;
    long long weight = 0;
    double lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    if (i < n) {
        deg = indptr[i + 1] - indptr[i];
        weight = pl_weight(w, (int32_t)i);
        ids[i] = (int32_t)i;
        lo_x = hi_x = xy[2 * i];
        lo_y = hi_y = xy[2 * i + 1];
    }
    block_reduce<PB, OpMin, OpMin, OpMax, OpMax>(red, lo_x, lo_y, hi_x, hi_y);
    block_reduce<PB, OpMax>(red_deg, deg);
    block_reduce<PB, OpSum>(red_weight, weight);
    if (threadIdx.x == 0) { // (one add per block: thousands of waves on one word wait in line)
        if (deg > 0) atomicMax(wide + PA_MAXDEG, (unsigned long long)deg);
        if (weight != 0) atomicAdd(wide + PA_TOTAL, (unsigned long long)weight);
        double *out = tile_bounds + 4 * (int64_t)blockIdx.x;
        out[0] = lo_x, out[1] = lo_y, out[2] = hi_x, out[3] = hi_y;
    }
}

// one block: frame = lo_x, lo_y, 65536 / max(side, 1e-300)
__global__ void __launch_bounds__(PB) k_pl_frame(const double *__restrict__ tile_bounds, int n_tile, double *__restrict__ frame) {
    __shared__ double red[4 * (PB / 64)];
    double b[4]; // lo_x, lo_y, hi_x, hi_y
    block_fold_partials<false, PB, OpMin, OpMin, OpMax, OpMax>(red, tile_bounds, n_tile, b);
    if (threadIdx.x == 0) {
        const double side = fmax(b[2] - b[0], b[3] - b[1]);
        frame[0] = b[0], frame[1] = b[1], frame[2] = (double)PL_CELLS / fmax(side, 1e-300);
    }
}

// the cell of a coordinate: a subtraction, a multiplication (the unit is compiled without contraction), floor, clamp
__device__ __forceinline__ uint32_t pl_cell(double v, double lo, double scale) {
    const double c = floor((v - lo) * scale);
    return (uint32_t)fmin(fmax(c, 0.0), (double)(PL_CELLS - 1));
}

__global__ void __launch_bounds__(PB)
k_pl_key(const double *__restrict__ xy, int64_t n, const double *__restrict__ frame, int32_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    uint32_t x = pl_cell(xy[2 * i], frame[0], frame[2]), y = pl_cell(xy[2 * i + 1], frame[1], frame[2]), d = 0;
    for (uint32_t s = PL_CELLS / 2; s > 0; s >>= 1) {
        const uint32_t rx = (x & s) > 0, ry = (y & s) > 0;
        d += s * s * ((3 * rx) ^ ry);
        if (ry == 0) {
            if (rx == 1) x = PL_CELLS - 1 - x, y = PL_CELLS - 1 - y;
            const uint32_t t = x;
            x = y, y = t;
        }
    }
    key[i] = (int32_t)d;
}

// value[k] = the weight of the k-th vertex of the list, zero behind the limit
__global__ void __launch_bounds__(PB)
k_pl_list_weights(const int32_t *__restrict__ list, const int32_t *__restrict__ limit, int64_t n, const int64_t *__restrict__ w,
                  int64_t *__restrict__ value) {
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (k < n) value[k] = k < *limit ? pl_weight(w, list[k]) : 0;
}

// label = min(P - 1, before * P / T) along the order; the parts' weights (a wave whose lanes agree adds once)
__global__ void __launch_bounds__(PB)
k_pl_seed(const int32_t *__restrict__ order, const int64_t *__restrict__ before, int64_t n, const int64_t *__restrict__ w, int64_t P,
          int64_t T, int32_t *__restrict__ lab, unsigned long long *part_weight) {
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    int32_t l = -1;
    long long weight = 0;
    if (k < n) {
        const int32_t v = order[k];
        const int64_t cut = before[k] * P / T;
        l = (int32_t)(cut < P - 1 ? cut : P - 1);
        lab[v] = l;
        weight = pl_weight(w, v);
    }
    const int32_t lead = __shfl(l, 0, 64); // (lane 0 holds the wave's first position: valid whenever any lane is)
    if (__all(l == lead || l < 0)) {
        weight = wave_reduce<OpSum>(weight);
        if ((threadIdx.x & 63) == 0 && lead >= 0 && weight != 0) atomicAdd(part_weight + lead, (unsigned long long)weight);
    } else if (l >= 0 && weight != 0) {
        atomicAdd(part_weight + l, (unsigned long long)weight);
    }
}

// twice the edge cut: entries whose two ends carry different labels (the diagonal never does)
__global__ void __launch_bounds__(PB)
k_pl_cut(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n, const int32_t *__restrict__ lab,
         unsigned long long *twice_cut) {
    __shared__ int lds[PB / 64];
    long long mine = 0;
    auto differing = [&](int32_t v, int first, int step) {
        int c = 0;
        const int32_t a = lab[v];
        for (int32_t p = indptr[v] + first; p < indptr[v + 1]; p += step) c += lab[indices[p]] != a;
        return c;
    };
    pl_rows(indptr, n, [&](int32_t v) { mine += differing(v, 0, 1); },
            [&](int32_t v) {
                int total;
                (void)block_excl_scan<PB>(differing(v, (int)threadIdx.x, PB), &total, lds);
                if (threadIdx.x == 0) mine += total;
            });
    mine = wave_reduce<OpSum>(mine);
    if ((threadIdx.x & 63) == 0 && mine != 0) atomicAdd(twice_cut, (unsigned long long)mine);
}

// ---- a round --------------------------------------------------------------------------------------------------------------------
// gain[v], dest[v]: the label other than v's own that most neighbours carry (the smallest on a tie) and what moving there takes
// off the cut; gain 0 (dest = the own label) where that is nothing.  The entry of v itself is no neighbour.
__global__ void __launch_bounds__(PB)
k_pl_candidate(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n, const int32_t *__restrict__ lab,
               int32_t *__restrict__ gain, int32_t *__restrict__ dest, const int32_t *__restrict__ ctl) {
    if (ctl[PW_DONE]) return;
    __shared__ int lds[PB / 64];
    __shared__ unsigned long long best_lds[PB / 64];
    auto store = [&](int32_t v, int32_t a, int32_t own, int32_t other, int32_t label) {
        const bool moves = label >= 0 && other > own;
        gain[v] = moves ? other - own : 0;
        dest[v] = moves ? label : a;
    };
    pl_rows(
        indptr, n,
        [&](int32_t v) { // a label is counted where the row names it first: rows are short, the labels come from cache
            const int32_t lo = indptr[v], hi = indptr[v + 1], a = lab[v];
            int32_t own = 0, best = 0, best_label = -1;
            for (int32_t p = lo; p < hi; p++) {
                const int32_t j = indices[p];
                if (j == v) continue;
                const int32_t l = lab[j];
                if (l == a) {
                    own++;
                    continue;
                }
                int32_t c = 0;
                bool first = true;
                for (int32_t q = lo; q < hi; q++) {
                    const int32_t jq = indices[q];
                    if (jq == v || lab[jq] != l) continue;
                    if (q < p) {
                        first = false;
                        break;
                    }
                    c++;
                }
                if (first && (c > best || (c == best && l < best_label))) best = c, best_label = l;
            }
            store(v, a, own, best, best_label);
        },
        [&](int32_t v) { // every thread counts the labels of its entries over the whole row: (count, smallest label) by a maximum
            const int32_t lo = indptr[v], hi = indptr[v + 1], a = lab[v];
            int own = 0;
            unsigned long long best = 0;
            for (int32_t p = lo + (int32_t)threadIdx.x; p < hi; p += PB) {
                const int32_t j = indices[p];
                if (j == v) continue;
                const int32_t l = lab[j];
                if (l == a) {
                    own++;
                    continue;
                }
                uint32_t c = 0;
                for (int32_t q = lo; q < hi; q++) c += indices[q] != v && lab[indices[q]] == l;
                const unsigned long long key = ((unsigned long long)c << 32) | (uint32_t)(INT32_MAX - l);
                best = key > best ? key : best;
            }
            int own_total;
            (void)block_excl_scan<PB>(own, &own_total, lds);
            block_reduce_all<PB, OpMax>(best_lds, best);
            if (threadIdx.x == 0)
                store(v, a, own_total, (int32_t)(best >> 32), best ? INT32_MAX - (int32_t)(best & 0xffffffffu) : -1);
        });
}

// flag[v] = v is a mover: a candidate none of whose neighbours is a candidate of higher priority (gain descending, id ascending)
__global__ void __launch_bounds__(PB)
k_pl_mover(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n, const int32_t *__restrict__ gain,
           int32_t *__restrict__ flag, const int32_t *__restrict__ ctl) {
    if (ctl[PW_DONE]) return;
    auto outranked = [&](int32_t v, int32_t g, int first, int step) {
        for (int32_t p = indptr[v] + first; p < indptr[v + 1]; p += step) {
            const int32_t j = indices[p], gj = gain[j];
            if (j != v && (gj > g || (gj == g && j < v))) return true;
        }
        return false;
    };
    pl_rows(indptr, n,
            [&](int32_t v) {
                const int32_t g = gain[v];
                flag[v] = g > 0 && !outranked(v, g, 0, 1);
            },
            [&](int32_t v) {
                const int32_t g = gain[v];
                const int any = __syncthreads_or(g > 0 && outranked(v, g, (int)threadIdx.x, PB));
                if (threadIdx.x == 0) flag[v] = g > 0 && !any;
            });
}

// the movers in id order (rank = exclusive scan of flag), their number
__global__ void __launch_bounds__(PB)
k_pl_compact(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n, int32_t *__restrict__ list, int32_t *ctl) {
    if (ctl[PW_DONE]) return;
    const int64_t v = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (v < n && flag[v]) list[rank[v]] = (int32_t)v;
    if (v == 0) ctl[PW_MOVERS] = rank[n];
}

// The list holds the movers by (part, gain descending, id); before = the exclusive scan of their weights along it.  A mover
// passes when the weight of its part's movers up to and including it fits the part's budget: L - W[part] where the part is
// the destination (source == 0), W[part] - Lmin where it is the source.  ok[v]: the first call stores, the second one ands.
__global__ void __launch_bounds__(PB)
k_pl_budget(const int32_t *__restrict__ list, const int32_t *__restrict__ part, const int64_t *__restrict__ before,
            const int64_t *__restrict__ w, const unsigned long long *__restrict__ part_weight, int64_t bound, int source,
            int32_t *__restrict__ ok, const int32_t *__restrict__ ctl) {
    if (ctl[PW_DONE]) return;
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (k >= ctl[PW_MOVERS]) return;
    const int32_t v = list[k], b = part[v];
    int64_t lo = 0, hi = k; // the first position of the run of b: the parts ascend along the list
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (part[list[mid]] < b) lo = mid + 1;
        else hi = mid;
    }
    const int64_t sum = before[k] + pl_weight(w, v) - before[lo], W = (int64_t)part_weight[b];
    const bool pass = sum <= (source ? W - bound : bound - W);
    ok[v] = source ? (ok[v] && pass) : pass;
}

// movers that passed both budgets take their destination; the parts' weights follow
__global__ void __launch_bounds__(PB)
k_pl_accept(const int32_t *__restrict__ list, const int32_t *__restrict__ dest, const int32_t *__restrict__ ok,
            const int64_t *__restrict__ w, int32_t *__restrict__ lab, unsigned long long *part_weight, int32_t *ctl) {
    if (ctl[PW_DONE]) return;
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    bool moved = false;
    if (k < ctl[PW_MOVERS]) {
        const int32_t v = list[k];
        if (ok[v]) {
            const int64_t weight = pl_weight(w, v);
            atomicAdd(part_weight + dest[v], (unsigned long long)weight);
            atomicAdd(part_weight + lab[v], (unsigned long long)(-weight));
            lab[v] = dest[v];
            moved = true;
        }
    }
    wave_count(moved, ctl + PW_ROUND_MOVES);
}

__global__ void k_pl_round_end(int32_t *ctl) {
    if (ctl[PW_DONE]) return;
    const int32_t moves = ctl[PW_ROUND_MOVES];
    ctl[PW_ROUNDS] += 1;
    ctl[PW_MOVES] += moves;
    ctl[PW_ROUND_MOVES] = 0;
    if (moves == 0 || ctl[PW_ROUNDS] >= PL_MAX_ROUNDS) ctl[PW_DONE] = 1;
}

static void fill_zero_bytes(void *p, size_t bytes) { XR_HIP(hipMemsetAsync(p, 0, bytes, launch_stream())); }

static void partition_labels(const xr_graph *g, const double *xy, const int64_t *w, int64_t P, int64_t *labels_dev, int64_t *info) {
    const int64_t n = g->n;
    const int32_t *indptr = g->indptr.get(), *indices = g->indices.get();
    const unsigned nb = div_up(n, PB);
    // int32 words: [key][lab][gain][dest][ok][flag][rank: n + 1][list: 3 n][ctl]
    DevBuf<int32_t> work((size_t)(10 * n + 1 + PW_COUNT));
    int32_t *key = work.get(), *lab = key + n, *gain = lab + n, *dest = gain + n, *ok = dest + n, *flag = ok + n, *rank = flag + n;
    int32_t *list[3] = {rank + n + 1, rank + 2 * n + 1, rank + 3 * n + 1}, *ctl = rank + 4 * n + 1;
    // 64-bit words: [value: n][before: n][tile totals: nb][part weights: P][wide counters]
    DevBuf<int64_t> wide_work((size_t)(2 * n + nb + P + PA_COUNT));
    int64_t *value = wide_work.get(), *before = value + n, *tile_total = before + n;
    unsigned long long *part_weight = reinterpret_cast<unsigned long long *>(tile_total + nb), *wide = part_weight + P;
    DevBuf<double> bounds((size_t)(4 * nb + 3));
    double *frame = bounds.get() + 4 * (size_t)nb;
    const PlSort sort{n, flag, rank, {list[1], list[2]}};

    fill_i32(ctl, 0, PW_COUNT);
    fill_i32(ctl + PW_N, (int32_t)n, 1);
    fill_zero_bytes(part_weight, sizeof(int64_t) * (size_t)(P + PA_COUNT));
    XR_LAUNCH("pl_init", k_pl_init, dim3(nb), dim3(PB), 0, indptr, xy, w, n, list[0], bounds.get(), wide);
    unsigned long long h[PA_COUNT];
    d2h(h, wide, sizeof(h), [&] { // (the key needs nothing the host is waiting for)
        XR_LAUNCH("pl_frame", k_pl_frame, dim3(1), dim3(PB), 0, bounds.get(), (int)nb, frame);
        XR_LAUNCH("pl_key", k_pl_key, dim3(nb), dim3(PB), 0, xy, n, frame, key);
    });
    int64_t T = (int64_t)h[PA_TOTAL];
    if (w && T == 0) { // weights that are all zero count as all ones
        w = nullptr;
        T = n;
    }
    if (!(T > 0 && T <= INT64_MAX / 100 / P)) stream_sync(); // (nothing in flight reads the caller's arrays when the call fails)
    XR_REQUIRE(T > 0 && T <= INT64_MAX / 100 / P, XR_ERR_INVALID,
               "xr_graph_partition_dev: 100 * n_part * sum(weights) does not fit in int64 (n_part %lld, sum %lld)", (long long)P, (long long)T);
    const int64_t L = std::max((T + P - 1) / P, T * (PL_EPS_DEN + PL_EPS_NUM) / (PL_EPS_DEN * P));
    const int64_t Lmin = std::min(T / P, (T * (PL_EPS_DEN - PL_EPS_NUM) + PL_EPS_DEN * P - 1) / (PL_EPS_DEN * P));

    const int32_t *order = sort.run(list[0], key, 0, 32, ctl + PW_N);
    XR_LAUNCH("pl_list_weights", k_pl_list_weights, dim3(nb), dim3(PB), 0, order, ctl + PW_N, n, w, value);
    exclusive_scan_i64(value, before, n, tile_total);
    XR_LAUNCH("pl_seed", k_pl_seed, dim3(nb), dim3(PB), 0, order, before, n, w, P, T, lab, part_weight);
    XR_LAUNCH("pl_cut", k_pl_cut, dim3(nb), dim3(PB), 0, indptr, indices, n, lab, wide + PA_CUT_SEED);

    int32_t c[PW_COUNT] = {0};
    if (P > 1 && T / P > 0) {
        const int gain_bits = bits_of((int64_t)h[PA_MAXDEG]), part_bits = bits_of(P - 1);
        const uint32_t descending = (uint32_t)((1ll << gain_bits) - 1); // gain ^ this descends where gain ascends
        for (int enqueued = 0; enqueued < PL_MAX_ROUNDS && !c[PW_DONE];) {
            for (int r = 0; r < PL_CHUNK && enqueued < PL_MAX_ROUNDS; r++, enqueued++) {
                XR_LAUNCH("pl_candidate", k_pl_candidate, dim3(nb), dim3(PB), 0, indptr, indices, n, lab, gain, dest, ctl);
                XR_LAUNCH("pl_mover", k_pl_mover, dim3(nb), dim3(PB), 0, indptr, indices, n, gain, flag, ctl);
                exclusive_scan_i32(flag, rank, n);
                XR_LAUNCH("pl_compact", k_pl_compact, dim3(nb), dim3(PB), 0, flag, rank, n, list[0], ctl);
                int32_t *by_gain = sort.run(list[0], gain, descending, gain_bits, ctl + PW_MOVERS);
                if (by_gain != list[0]) { // (the two sorts below write the spare lists: the common start moves out of their way)
                    XR_HIP(hipMemcpyAsync(list[0], by_gain, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, launch_stream()));
                    by_gain = list[0];
                }
                for (int source = 0; source < 2; source++) {
                    const int32_t *part = source ? lab : dest;
                    const int32_t *by_part = sort.run(by_gain, part, 0, part_bits, ctl + PW_MOVERS);
                    XR_LAUNCH("pl_list_weights", k_pl_list_weights, dim3(nb), dim3(PB), 0, by_part, ctl + PW_MOVERS, n, w, value);
                    exclusive_scan_i64(value, before, n, tile_total);
                    XR_LAUNCH("pl_budget", k_pl_budget, dim3(nb), dim3(PB), 0, by_part, part, before, w, part_weight, source ? Lmin : L,
                              source, ok, ctl);
                    if (source)
                        XR_LAUNCH("pl_accept", k_pl_accept, dim3(nb), dim3(PB), 0, by_part, dest, ok, w, lab, part_weight, ctl);
                }
                XR_LAUNCH("pl_round_end", k_pl_round_end, dim3(1), dim3(1), 0, ctl);
            }
            d2h(c, ctl, sizeof(c));
        }
    }
    XR_LAUNCH("pl_cut", k_pl_cut, dim3(nb), dim3(PB), 0, indptr, indices, n, lab, wide + PA_CUT_RESULT);
    widen_dev(lab, n, labels_dev);
    d2h(h, wide, sizeof(h)); // (waits: the state goes back to the pool behind its last reader)
    if (info) info[0] = c[PW_ROUNDS], info[1] = c[PW_MOVES], info[2] = (int64_t)h[PA_CUT_SEED] / 2, info[3] = (int64_t)h[PA_CUT_RESULT] / 2;
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_graph_partition_dev(const xr_graph *g, const double *xy_dev, const int64_t *weights_dev, int64_t n_part, int64_t *labels_dev,
                           int64_t *info) {
    XR_API_BEGIN
    XR_REQUIRE(g && ((xy_dev && labels_dev) || g->n == 0), XR_ERR_INVALID, "xr_graph_partition_dev: NULL argument");
    XR_REQUIRE(n_part >= 1 && (n_part <= g->n || g->n == 0), XR_ERR_INVALID,
               "xr_graph_partition_dev: n_part must be in [1, %lld], received: %lld", (long long)g->n, (long long)n_part);
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (g->n > 0) partition_labels(g, xy_dev, weights_dev, n_part, labels_dev, info);
    dev_call_done();
    XR_API_END
}

} // extern "C"
