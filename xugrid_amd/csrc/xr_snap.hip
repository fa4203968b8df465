// xr_snap.hip -- snapping points on the device: snap_nodes (xugrid/ugrid/snapping.py:46-143: a KD-tree distance matrix and a
// sequential greedy loop) and snap_to_nodes (:146-219: a second distance matrix, row counts and a groupby).  DESIGN section 19.
//
// Both rest on the uniform grid of xr_nn.h and on one RADIUS WALK: for a point p and a distance d, every indexed point s with
// dx * dx + dy * dy <= d * d (float64, uncontracted, inclusive: the KD-tree's own test) is visited by walking the block of
// cells that covers the disc.  The block is taken a hair wider than d (snap_reach) so that no rounding of the squares can let a
// point pass the test from outside it.
//
// snap_nodes: the greedy loop makes candidate i a target exactly when no lower-numbered target lies within d -- the
// lexicographically first maximal independent set of the proximity graph -- and then sends every other point to its nearest
// target (the stored square roots compared, strictly: the lowest id among equal ones).  Here: count, scan, fill the adjacency
// as CSR once; decide in level-synchronous rounds on a state byte per point; assign; rank the targets.
#include <cmath>

#include "xr_nn.h"
#include "xr_prims.h"
#include "xr_snap_rounds.h"

namespace xr {

static constexpr int NB = 256; // threads per block

enum : uint8_t { SNAP_UNDECIDED = 0, SNAP_TARGET = 1, SNAP_SNAPPED = 2 };
// status words of one merge: [0] points decided so far, [1] the last round in which a point was decided
enum { SNAP_DECIDED = 0, SNAP_LAST_ROUND = 1, SNAP_WORDS = 2 };

// Half the side of the block of cells that must be walked for distance d.  A point passes the test only if fl(dx * dx) <=
// fl(d * d); for |dx| >= d (1 + 2^-50) the two squares are at least four ulp apart, so such a point never passes.  Below
// 1e-150 the squares leave the normal range (they underflow to zero and pass even d = 0), hence the floor.
__device__ __forceinline__ double snap_reach(double d) { return fmax(d * (1.0 + 0x1p-50), 1e-150); }

struct SnapBlock {
    int x0, x1, y0, y1;
};
__device__ __forceinline__ SnapBlock snap_block(const SampleGrid &g, double2 p, double reach) {
    return {sp_cell_x(g, p.x - reach), sp_cell_x(g, p.x + reach), sp_cell_y(g, p.y - reach), sp_cell_y(g, p.y + reach)};
}

// f(position in the index, squared distance) for every indexed point within the distance of p, a row of cells at a time (the
// cells of one row are one run of storage)
template <typename F>
__device__ __forceinline__ void snap_walk(const double2 *__restrict__ pxy, const int32_t *__restrict__ start, const SampleGrid &g,
                                          double2 p, double d2max, double reach, F &&f) {
    const SnapBlock b = snap_block(g, p, reach);
    for (int yy = b.y0; yy <= b.y1; yy++) {
        const int64_t row = (int64_t)yy * g.nx;
        for (int e = start[row + b.x0]; e < start[row + b.x1 + 1]; e++) {
            const double2 s = pxy[e];
            const double dx = s.x - p.x, dy = s.y - p.y;
            const double d2 = dx * dx + dy * dy;
            if (d2 <= d2max) f(e, d2);
        }
    }
}

// xy[i] = (x[i * stride], y[i * stride]); *bad = 1 if a coordinate is NaN or infinite
__global__ void __launch_bounds__(NB)
k_snap_pack(const double *__restrict__ x, const double *__restrict__ y, int64_t stride, int64_t n, double2 *__restrict__ xy,
            int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    bool mine_bad = false;
    if (i < n) {
        const double2 p = make_double2(x[i * stride], y[i * stride]);
        mine_bad = !isfinite(p.x) || !isfinite(p.y);
        xy[i] = p;
    }
    wave_flag(mine_bad, bad);
}

// count[i] = points within the distance of point i, itself excluded (it always passes: 0 <= d * d); *total: their sum
__global__ void __launch_bounds__(NB)
k_snap_count(const double2 *__restrict__ xy, int64_t n, const double2 *__restrict__ pxy, const int32_t *__restrict__ start,
             SampleGrid g, double d2max, double d, int32_t *__restrict__ count, unsigned long long *__restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    int32_t c = 0;
    if (i < n) {
        snap_walk(pxy, start, g, xy[i], d2max, snap_reach(d), [&](int, double) { c++; });
        c -= 1;
        count[i] = c;
    }
    const unsigned long long sum = wave_reduce<OpSum>((unsigned long long)c);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
}

// row i of the adjacency: the ids of those points and the ROUNDED SQUARE ROOT of each squared distance, which is what the
// reference stores and compares
__global__ void __launch_bounds__(NB)
k_snap_fill(const double2 *__restrict__ xy, int64_t n, const double2 *__restrict__ pxy, const int32_t *__restrict__ pid,
            const int32_t *__restrict__ start, SampleGrid g, double d2max, double d, const int32_t *__restrict__ indptr,
            int32_t *__restrict__ nbr, double *__restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    int32_t at = indptr[i];
    const int32_t end = indptr[i + 1];
    snap_walk(pxy, start, g, xy[i], d2max, snap_reach(d), [&](int e, double d2) {
        const int32_t j = pid[e];
        if (j != (int32_t)i && at < end) {
            nbr[at] = j;
            dist[at] = sqrt(d2);
            at++;
        }
    });
}

// One round of decisions.  An undecided point becomes SNAPPED if a lower-numbered neighbour is a target and a TARGET if every
// lower-numbered neighbour is snapped; both are final, and both read only final states of lower ids -- so a state stored
// earlier in this very launch may be used, and a state not yet seen only delays a decision.  SWEEPS bounded passes per launch;
// no lane waits for another.  Decided points leave at their first read.
__global__ void __launch_bounds__(NB)
k_snap_round(const int32_t *__restrict__ indptr, const int32_t *__restrict__ nbr, int64_t n, int32_t round, uint8_t *state,
             int32_t *__restrict__ words) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    bool decided = false;
    if (i < n && state[i] == SNAP_UNDECIDED) {
        const int32_t a = indptr[i], b = indptr[i + 1];
        for (int sweep = 0; sweep < XR_SNAP_SWEEPS && !decided; sweep++) {
            bool target_below = false, open_below = false;
            for (int32_t e = a; e < b; e++) {
                const int32_t j = nbr[e];
                if (j >= (int32_t)i) continue;
                const uint8_t s = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                target_below |= s == SNAP_TARGET;
                open_below |= s == SNAP_UNDECIDED;
            }
            if (target_below || !open_below) {
                __hip_atomic_store(&state[i], target_below ? SNAP_SNAPPED : SNAP_TARGET, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                decided = true;
            }
        }
    }
    const unsigned long long ballot = __ballot(decided);
    if ((threadIdx.x & 63) == 0 && ballot) {
        atomicAdd(&words[SNAP_DECIDED], __popcll(ballot));
        atomicMax(&words[SNAP_LAST_ROUND], round);
    }
}

// visited[i]: a target keeps itself; a snapped point takes, among its neighbours that are targets, the one with the smallest
// stored distance, the lowest id on equal distances.  is_target[i] = 1 for the targets.
__global__ void __launch_bounds__(NB)
k_snap_assign(const int32_t *__restrict__ indptr, const int32_t *__restrict__ nbr, const double *__restrict__ dist,
              const uint8_t *__restrict__ state, int64_t n, int32_t *__restrict__ visited, int32_t *__restrict__ is_target) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    int32_t to = (int32_t)i;
    if (state[i] != SNAP_TARGET) {
        double best = INFINITY;
        to = -1;
        for (int32_t e = indptr[i]; e < indptr[i + 1]; e++) {
            const int32_t j = nbr[e];
            if (state[j] != SNAP_TARGET) continue;
            const double d = dist[e];
            if (to < 0 || d < best || (d == best && j < to)) best = d, to = j;
        }
        if (to < 0) to = (int32_t)i; // (never: a snapped point has a target below it)
    }
    visited[i] = to;
    is_target[i] = to == (int32_t)i;
}

// inverse[i] = rank of the target point i went to; the kept coordinates, gathered
__global__ void __launch_bounds__(NB)
k_snap_emit(const int32_t *__restrict__ visited, const int32_t *__restrict__ rank, const double2 *__restrict__ xy, int64_t n,
            int32_t *__restrict__ inverse, int32_t *__restrict__ index, double2 *__restrict__ kept_xy) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    const int32_t to = visited[i];
    inverse[i] = rank[to];
    if (to == (int32_t)i) {
        index[rank[i]] = (int32_t)i;
        kept_xy[rank[i]] = xy[i];
    }
}

// out[k] = in[2 k + column]
__global__ void __launch_bounds__(NB) k_snap_column(const double *__restrict__ in, int column, int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i < n) out[i] = in[2 * i + column];
}

// *bad = 1 if an id lies outside [0, n)
__global__ void __launch_bounds__(NB) k_snap_id_check(const int64_t *__restrict__ ids, int64_t count, int64_t n, int32_t *__restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * NB + threadIdx.x;
    wave_flag(k < count && (ids[k] < 0 || ids[k] >= n), bad);
}

__global__ void __launch_bounds__(NB)
k_snap_relabel(const int32_t *__restrict__ inverse, const int64_t *__restrict__ ids, int64_t count, int64_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (k < count) out[k] = inverse[ids[k]];
}

// *bad = 1 if an indexed point has a NaN or infinite coordinate
__global__ void __launch_bounds__(NB) k_snap_finite(const double2 *__restrict__ pxy, int64_t n, int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    wave_flag(i < n && (!isfinite(pxy[i].x) || !isfinite(pxy[i].y)), bad);
}

// One lane per point: the to-points within the distance are counted, the nearest is kept (smallest squared distance, lowest id
// on equal squares).  With at least one the point moves onto it, else it is copied.  words[0]: a non-finite point was met,
// words[1]: points with more than one to-point within the distance.  Without an index (pxy NULL) every point is copied.
__global__ void __launch_bounds__(NB)
k_snap_to(const double *__restrict__ x, const double *__restrict__ y, int64_t stride, int64_t n, const double2 *__restrict__ pxy,
          const int32_t *__restrict__ pid, const int32_t *__restrict__ start, SampleGrid g, double d2max, double d,
          double *__restrict__ x_out, double *__restrict__ y_out, int64_t out_stride, int64_t *__restrict__ index_out,
          int32_t *__restrict__ words) {
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    bool bad = false, tied = false;
    if (i < n) {
        double2 p = make_double2(x[i * stride], y[i * stride]);
        bad = !isfinite(p.x) || !isfinite(p.y);
        int32_t within = 0, to = -1, at = -1;
        if (!bad && pxy) {
            double best = INFINITY;
            snap_walk(pxy, start, g, p, d2max, snap_reach(d), [&](int e, double d2) {
                within++;
                if (d2 <= best) {
                    const int32_t j = pid[e];
                    if (d2 < best || j < to) best = d2, to = j, at = e;
                }
            });
        }
        if (at >= 0) p = pxy[at];
        tied = within > 1;
        x_out[i * out_stride] = p.x;
        y_out[i * out_stride] = p.y;
        if (index_out) index_out[i] = to;
    }
    wave_flag(bad, &words[0]);
    wave_count(tied, &words[1]);
}

} // namespace xr

// The result of one snap_nodes (include/xugrid_amd.h)
struct xr_snap {
    int64_t n = 0, n_kept = 0, n_pair = 0, rounds = 0;
    xr::DevBuf<int32_t> inverse; // [n] the kept node every node went to
    xr::DevBuf<int32_t> index;   // [n_kept] the kept nodes, ascending
    xr::DevBuf<double2> xy;      // [n_kept] their coordinates
};

using namespace xr;

extern "C" {

int xr_snap_nodes_dev(const double *x_dev, const double *y_dev, int64_t stride, int64_t n, double max_distance, xr_snap **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && n >= 0 && ((x_dev && y_dev) || n == 0), XR_ERR_INVALID, "xr_snap_nodes_dev: NULL argument or negative size");
    XR_REQUIRE(stride >= 1, XR_ERR_INVALID, "xr_snap_nodes_dev: stride must be at least 1");
    XR_REQUIRE(max_distance >= 0.0, XR_ERR_INVALID, "xr_snap_nodes_dev: max_distance must be non-negative");
    XR_REQUIRE(n < INT32_MAX, XR_ERR_LIMIT, "xr_snap_nodes_dev: more than 2^31 points");
    Building<xr_snap> snap(OnFailure::WaitFirst);
    snap->n = snap->n_kept = n;
    if (n == 0) {
        *out = snap.release();
        return XR_OK;
    }
    const unsigned nb = div_up(n, NB);
    DevBuf<double2> xy((size_t)n);
    DevBuf<int32_t> words(SNAP_WORDS);
    fill_i32(words.get(), 0, SNAP_WORDS);
    XR_LAUNCH("snap_pack", k_snap_pack, dim3(nb), dim3(NB), 0, x_dev, y_dev, stride, n, xy.get(), words.get());
    // (the box of the index is read back next: the flag travels with the same wait)
    const NnExtent extent = nn_extent(reinterpret_cast<const double *>(xy.get()), n);
    XR_REQUIRE(read_scalar(words.get()) == 0, XR_ERR_INVALID, "data must be finite");
    std::unique_ptr<xr_nn> nn(nn_build(reinterpret_cast<const double *>(xy.get()), n, nullptr, extent));

    // 1. count
    const double d2max = max_distance * max_distance;
    DevBuf<int32_t> count((size_t)n), indptr((size_t)n + 1);
    DevBuf<unsigned long long> total(1);
    fill_i32(reinterpret_cast<int32_t *>(total.get()), 0, 2);
    XR_LAUNCH("snap_count", k_snap_count, dim3(nb), dim3(NB), 0, xy.get(), n, nn->xy.get(), nn->start.get(), nn->grid, d2max,
              max_distance, count.get(), total.get());
    const unsigned long long n_pair = read_scalar(total.get());
    XR_REQUIRE(snap_pairs_fit(n_pair), XR_ERR_INVALID,
               "xr_snap_nodes_dev: %llu pairs of points lie within max_distance = %g of each other, more than 2^31 - 1: the "
               "distance is too large for these points",
               n_pair, max_distance);
    snap->n_pair = (int64_t)n_pair;
    if (n_pair == 0) { // nothing to snap
        *out = snap.release();
        return XR_OK;
    }

    // 2. the adjacency, once
    DevBuf<int32_t> nbr((size_t)n_pair);
    DevBuf<double> dist((size_t)n_pair);
    exclusive_scan_i32(count.get(), indptr.get(), n);
    XR_LAUNCH("snap_fill", k_snap_fill, dim3(nb), dim3(NB), 0, xy.get(), n, nn->xy.get(), nn->id.get(), nn->start.get(), nn->grid,
              d2max, max_distance, indptr.get(), nbr.get(), dist.get());

    // 3. rounds: every launch decides at least the lowest undecided point, so n launches always suffice
    DevBuf<uint8_t> state((size_t)n);
    XR_HIP(hipMemsetAsync(state.get(), SNAP_UNDECIDED, (size_t)n, launch_stream()));
    int32_t h[SNAP_WORDS] = {0, 0};
    const int64_t launches = snap_run_rounds(
        n,
        [&](int64_t round) {
            XR_LAUNCH("snap_round", k_snap_round, dim3(nb), dim3(NB), 0, indptr.get(), nbr.get(), n, (int32_t)round, state.get(), words.get());
        },
        [&]() {
            d2h(h, words.get(), sizeof(h));
            return (int64_t)h[SNAP_DECIDED];
        });
    XR_REQUIRE(launches > 0, XR_ERR_HIP, "xr_snap_nodes_dev: the decision rounds did not end");
    snap->rounds = h[SNAP_LAST_ROUND];

    // 4. assign, 5. rank the targets and emit
    DevBuf<int32_t> visited((size_t)n), is_target((size_t)n), rank((size_t)n + 1);
    XR_LAUNCH("snap_assign", k_snap_assign, dim3(nb), dim3(NB), 0, indptr.get(), nbr.get(), dist.get(), state.get(), n, visited.get(),
              is_target.get());
    exclusive_scan_i32(is_target.get(), rank.get(), n);
    const int64_t n_kept = read_scalar(rank.get() + n);
    XR_REQUIRE(n_kept >= 1 && n_kept <= n, XR_ERR_HIP, "xr_snap_nodes_dev: kept count out of range");
    snap->n_kept = n_kept;
    snap->inverse.alloc((size_t)n), snap->index.alloc((size_t)n_kept), snap->xy.alloc((size_t)n_kept);
    XR_LAUNCH("snap_emit", k_snap_emit, dim3(nb), dim3(NB), 0, visited.get(), rank.get(), xy.get(), n, snap->inverse.get(),
              snap->index.get(), snap->xy.get());
    dev_call_done();
    *out = snap.release();
    XR_API_END
}

int xr_snap_info(const xr_snap *snap, int64_t *n_kept, int64_t *n_pair, int64_t *rounds) {
    XR_API_BEGIN
    XR_REQUIRE(snap, XR_ERR_INVALID, "xr_snap_info: NULL handle");
    if (n_kept) *n_kept = snap->n_kept;
    if (n_pair) *n_pair = snap->n_pair;
    if (rounds) *rounds = snap->rounds;
    XR_API_END
}

int xr_snap_copy_dev(const xr_snap *snap, int what, void *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(snap && what >= XR_SNAP_INVERSE && what <= XR_SNAP_Y, XR_ERR_INVALID, "xr_snap_copy_dev: bad argument");
    XR_REQUIRE(snap->n_pair > 0, XR_ERR_INVALID, "xr_snap_copy_dev: nothing was snapped, the handle holds no arrays");
    XR_REQUIRE(out_dev, XR_ERR_INVALID, "xr_snap_copy_dev: NULL argument");
    const int64_t K = snap->n_kept;
    const double *kept = reinterpret_cast<const double *>(snap->xy.get());
    switch (what) {
    case XR_SNAP_INVERSE: widen_dev(snap->inverse.get(), snap->n, static_cast<int64_t *>(out_dev)); break;
    case XR_SNAP_INDEX: widen_dev(snap->index.get(), K, static_cast<int64_t *>(out_dev)); break;
    case XR_SNAP_XY: XR_HIP(hipMemcpyAsync(out_dev, kept, (size_t)K * 16, hipMemcpyDeviceToDevice, launch_stream())); break;
    default:
        XR_LAUNCH("snap_column", k_snap_column, dim3(div_up(K, NB)), dim3(NB), 0, kept, what == XR_SNAP_Y ? 1 : 0, K,
                  static_cast<double *>(out_dev));
        break;
    }
    dev_call_done();
    XR_API_END
}

int xr_snap_relabel_dev(const xr_snap *snap, const int64_t *ids_dev, int64_t count, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(snap && count >= 0 && ((ids_dev && out_dev) || count == 0), XR_ERR_INVALID, "xr_snap_relabel_dev: bad argument");
    XR_REQUIRE(snap->n_pair > 0, XR_ERR_INVALID, "xr_snap_relabel_dev: nothing was snapped, the handle holds no arrays");
    if (count > 0) {
        DevBuf<int32_t> bad(1);
        fill_i32(bad.get(), 0, 1);
        XR_LAUNCH("snap_id_check", k_snap_id_check, dim3(div_up(count, NB)), dim3(NB), 0, ids_dev, count, snap->n, bad.get());
        XR_REQUIRE(read_scalar(bad.get()) == 0, XR_ERR_INVALID, "xr_snap_relabel_dev: an id lies outside [0, %lld)", (long long)snap->n);
        XR_LAUNCH("snap_relabel", k_snap_relabel, dim3(div_up(count, NB)), dim3(NB), 0, snap->inverse.get(), ids_dev, count, out_dev);
    }
    dev_call_done();
    XR_API_END
}

int xr_snap_destroy(xr_snap *snap) {
    XR_API_BEGIN
    if (snap) {
        release_point();
        delete snap;
    }
    XR_API_END
}

int xr_nn_snap_dev(const xr_nn *to_index, const double *x_dev, const double *y_dev, int64_t stride, int64_t n, double max_distance,
                   double *x_out_dev, double *y_out_dev, int64_t out_stride, int64_t *index_out_dev, int64_t *n_tied) {
    XR_API_BEGIN
    XR_REQUIRE(n >= 0 && n < INT32_MAX, XR_ERR_LIMIT, "xr_nn_snap_dev: n must be in [0, 2^31)");
    XR_REQUIRE((x_dev && y_dev && x_out_dev && y_out_dev) || n == 0, XR_ERR_INVALID, "xr_nn_snap_dev: NULL argument");
    XR_REQUIRE(stride >= 1 && out_stride >= 1, XR_ERR_INVALID, "xr_nn_snap_dev: strides must be at least 1");
    XR_REQUIRE(max_distance >= 0.0, XR_ERR_INVALID, "xr_nn_snap_dev: max_distance must be non-negative");
    if (n_tied) *n_tied = 0;
    DevBuf<int32_t> words(2);
    fill_i32(words.get(), 0, 2);
    if (to_index)
        XR_LAUNCH("snap_finite", k_snap_finite, dim3(div_up(to_index->n, NB)), dim3(NB), 0, to_index->xy.get(), to_index->n, words.get());
    if (n > 0)
        XR_LAUNCH("snap_to", k_snap_to, dim3(div_up(n, NB)), dim3(NB), 0, x_dev, y_dev, stride, n,
                  to_index ? to_index->xy.get() : (const double2 *)nullptr, to_index ? to_index->id.get() : (const int32_t *)nullptr,
                  to_index ? to_index->start.get() : (const int32_t *)nullptr, to_index ? to_index->grid : SampleGrid{},
                  max_distance * max_distance, max_distance, x_out_dev, y_out_dev, out_stride, index_out_dev, words.get());
    int32_t h[2];
    d2h(h, words.get(), sizeof(h));
    XR_REQUIRE(h[0] == 0, XR_ERR_INVALID, "data must be finite");
    if (n_tied) *n_tied = h[1];
    XR_API_END
}

} // extern "C"
