// xr_geometry.hip -- meshes from cell geometry, where the geometry is: the sorted unique rows of a coordinate array
// (np.unique(axis=0)), CF cell bounds (N, M, 4) -> faces (conversion.bounds2d_to_topology2d, conversion.py:297-354), interval
// breaks and curvilinear lattices (conversion.py:171-199, ugrid2d.py:1894-1971), rings -> faces (conversion.polygons_to_faces,
// conversion.py:82-117) and faces -> rings (faces_to_polygons).  DESIGN section 24.
//
// SORTED UNIQUE ROWS.  The key table (xr_key_table.h) says which rows are equal and which came first; the representatives are
// compacted with the scan and sorted by (x, y) with a stable least-significant-digit radix sort over the order-preserving
// images of the two doubles (xr_sort_keys.h): one byte per pass, 16 passes for the 128-bit key, of which those whose byte is
// the same in every key are skipped (one OR and one AND reduction up front).  A pass is three launches:
//     k_sort_count    per block, the number of keys of every digit               -> hist[digit][block]
//     exclusive_scan_i32 over hist: digits ascending, blocks ascending inside a digit (the stable order)
//     k_sort_scatter  key to scan[digit][block] + its rank among the block's keys of that digit
// The rank inside a block needs no atomics: the lanes of a wave with one digit find each other with eight ballots (one per
// bit), the waves' counts are added up in wave order.  Keys are distinct after the table, so the result does not depend on
// anything but the keys.  Integer atomics only count (wave_count); no floating-point atomics anywhere.
//
// Ids are int32 in HBM; whatever is read through an id read from memory is compared with its range first.
#include <algorithm>
#include <vector>

#include "xr_objects.h"
#include "xr_prims.h"

#include "xr_key_table.h"
#include "xr_sort_keys.h"

namespace xr {

// the sorted unique rows of n coordinate rows
struct UniqueRows {
    int64_t n = 0, n_unique = 0, n_nonfinite = 0;
    int passes_run = 0, passes_skipped = 0;
    DevBuf<double> xy;        // [n_unique * 2] ascending by x, then y; the bits of each key's first row
    DevBuf<int32_t> index;    // [n_unique] that row's position in the input
    DevBuf<int32_t> inverse;  // [n] the rank of every row's key
};

} // namespace xr

struct xr_unique_xy {
    xr::UniqueRows rows;
};

namespace xr {

struct OpOr {
    template <typename T> static constexpr T identity() { return T(0); }
    template <typename T> __device__ __forceinline__ static T apply(T a, T b) { return a | b; }
};
struct OpAnd {
    template <typename T> static constexpr T identity() { return ~T(0); }
    template <typename T> __device__ __forceinline__ static T apply(T a, T b) { return a & b; }
};

enum KeyStat : int { KS_ANY_X = 0, KS_ALL_X, KS_ANY_Y, KS_ALL_Y, KS_NONFINITE, KS_COUNT };

// first stage of the reduction over all rows: OR and AND of the key images, and the rows with a non-finite coordinate
__global__ void __launch_bounds__(256) k_unique_key_stats(const double2 *__restrict__ xy, int64_t n, uint64_t *__restrict__ partial) {
    __shared__ uint64_t lds[KS_COUNT * 4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t any_x = 0, all_x = ~0ull, any_y = 0, all_y = ~0ull, bad = 0;
    if (i < n) {
        const double2 p = xy[i];
        any_x = all_x = sort_key_image(p.x);
        any_y = all_y = sort_key_image(p.y);
        bad = !(isfinite(p.x) && isfinite(p.y));
    }
    block_reduce<256, OpOr, OpAnd, OpOr, OpAnd, OpSum>(lds, any_x, all_x, any_y, all_y, bad);
    if (threadIdx.x == 0) {
        uint64_t *out = partial + (int64_t)blockIdx.x * KS_COUNT;
        out[KS_ANY_X] = any_x, out[KS_ALL_X] = all_x, out[KS_ANY_Y] = any_y, out[KS_ALL_Y] = all_y, out[KS_NONFINITE] = bad;
    }
}

// the representatives to their dense rank: key images and row id
__global__ void __launch_bounds__(256)
k_unique_compact(const double2 *__restrict__ xy, const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n, int64_t n_unique,
                 uint64_t *__restrict__ key_x, uint64_t *__restrict__ key_y, int32_t *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t j = rank[i];
    if (j < 0 || j >= n_unique) return;
    const double2 p = xy[i];
    key_x[j] = sort_key_image(p.x);
    key_y[j] = sort_key_image(p.y);
    ids[j] = (int32_t)i;
}

// The block's keys by digit (every thread of the block must get here): -> this thread's rank among the keys of its digit in
// its WAVE; counts[w * SORT_BUCKETS + d] = the keys of digit d in wave w.  Ends behind a barrier.
__device__ __forceinline__ int block_digit_ranks(unsigned digit, bool live, int32_t *counts /* [4 * SORT_BUCKETS] LDS */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < 4 * SORT_BUCKETS; t += 256) counts[t] = 0;
    __syncthreads();
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < SORT_DIGIT_BITS; b++) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long with = __ballot(live && bit);
        peers &= bit ? with : ~with;
    }
    int rank = 0;
    if (live) {
        rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (rank == 0) counts[wave * SORT_BUCKETS + (int)digit] = __popcll(peers);
    }
    __syncthreads();
    return rank;
}

__global__ void __launch_bounds__(256)
k_sort_count(const uint64_t *__restrict__ key_x, const uint64_t *__restrict__ key_y, int64_t n, int pass, int64_t n_block,
             int32_t *__restrict__ hist) {
    __shared__ int32_t counts[4 * SORT_BUCKETS];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const unsigned digit = live ? sort_digit(key_x[i], key_y[i], pass) : 0u;
    block_digit_ranks(digit, live, counts);
    const int d = threadIdx.x; // (256 threads, 256 digits)
    hist[(int64_t)d * n_block + blockIdx.x] = counts[d] + counts[SORT_BUCKETS + d] + counts[2 * SORT_BUCKETS + d] + counts[3 * SORT_BUCKETS + d];
}

__global__ void __launch_bounds__(256)
k_sort_scatter(const uint64_t *__restrict__ key_x, const uint64_t *__restrict__ key_y, const int32_t *__restrict__ ids, int64_t n, int pass,
               int64_t n_block, const int32_t *__restrict__ start, uint64_t *__restrict__ out_x, uint64_t *__restrict__ out_y,
               int32_t *__restrict__ out_ids) {
    __shared__ int32_t counts[4 * SORT_BUCKETS];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    uint64_t kx = 0, ky = 0;
    if (live) kx = key_x[i], ky = key_y[i];
    const unsigned digit = live ? sort_digit(kx, ky, pass) : 0u;
    const int rank = block_digit_ranks(digit, live, counts);
    {   // column d of `counts` becomes where each wave's keys of digit d start (thread d owns the column)
        const int d = threadIdx.x;
        int32_t at = start[(int64_t)d * n_block + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int32_t c = counts[w * SORT_BUCKETS + d];
            counts[w * SORT_BUCKETS + d] = at;
            at += c;
        }
    }
    __syncthreads();
    if (!live) return;
    const int64_t to = (int64_t)counts[(threadIdx.x >> 6) * SORT_BUCKETS + (int)digit] + rank;
    if (to < 0 || to >= n) return; // (cannot happen: the scan of the counts places every key once)
    out_x[to] = kx, out_y[to] = ky, out_ids[to] = ids[i];
}

// sorted position k holds row ids[k]: its coordinates (16 bytes, bit for bit), its position, and the way back
__global__ void __launch_bounds__(256)
k_unique_emit(const double2 *__restrict__ xy, const int32_t *__restrict__ ids, int64_t n_unique, int64_t n, double2 *__restrict__ out_xy,
              int32_t *__restrict__ index, int32_t *__restrict__ rank_of_row) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_unique) return;
    const int32_t i = ids[k];
    if (i < 0 || (int64_t)i >= n) return;
    out_xy[k] = xy[i];
    index[k] = i;
    rank_of_row[i] = (int32_t)k;
}

// stable LSD radix sort of n distinct keys with their ids; -> true when the result is in the second set of buffers
static bool radix_sort_keys(uint64_t *key_x[2], uint64_t *key_y[2], int32_t *ids[2], int64_t n, uint32_t pass_mask) {
    const int64_t n_block = div_up(n, 256);
    DevBuf<int32_t> hist((size_t)(SORT_BUCKETS * n_block)), start((size_t)(SORT_BUCKETS * n_block) + 1);
    int cur = 0;
    for (int pass = 0; pass < SORT_PASSES; pass++) {
        if (!((pass_mask >> pass) & 1u)) continue;
        XR_LAUNCH("sort_count", k_sort_count, dim3((unsigned)n_block), dim3(256), 0, key_x[cur], key_y[cur], n, pass, n_block, hist.get());
        exclusive_scan_i32(hist.get(), start.get(), SORT_BUCKETS * n_block);
        XR_LAUNCH("sort_scatter", k_sort_scatter, dim3((unsigned)n_block), dim3(256), 0, key_x[cur], key_y[cur], ids[cur], n, pass, n_block,
                  start.get(), key_x[1 - cur], key_y[1 - cur], ids[1 - cur]);
        cur = 1 - cur;
    }
    return cur == 1;
}

// the contract of xr_unique_xy_dev on rows that are on the device.  With non-finite rows only their count is set.
static void unique_rows(const double2 *xy, int64_t n, UniqueRows &out) {
    XR_REQUIRE(n < ((int64_t)1 << 30), XR_ERR_LIMIT, "unique rows: %lld rows exceed the int32 index range", (long long)n);
    out.n = n;
    out.n_unique = out.n_nonfinite = 0;
    out.passes_run = out.passes_skipped = 0;
    if (n == 0) {
        out.xy.alloc(0), out.index.alloc(0), out.inverse.alloc(0);
        return;
    }
    uint64_t stats[KS_COUNT];
    {
        const unsigned nb = div_up(n, 256);
        TwoStageReduce<256, uint64_t, OpOr, OpAnd, OpOr, OpAnd, OpSum> reduce("unique_key_fold", nb, [&](uint64_t *partial) {
            XR_LAUNCH("unique_key_stats", k_unique_key_stats, dim3(nb), dim3(256), 0, xy, n, partial);
        });
        reduce.read(stats);
    }
    out.n_nonfinite = (int64_t)stats[KS_NONFINITE];
    if (out.n_nonfinite > 0) return;
    const uint32_t pass_mask = sort_pass_mask(stats[KS_ANY_X], stats[KS_ALL_X], stats[KS_ANY_Y], stats[KS_ALL_Y]);
    for (int pass = 0; pass < SORT_PASSES; pass++) ((pass_mask >> pass) & 1u ? out.passes_run : out.passes_skipped)++;

    DevBuf<int32_t> rep((size_t)n), flag((size_t)n), rank((size_t)n + 1);
    table_first_occurrence(XYRows{xy}, n, rep.get(), flag.get());
    rank_of_flags(flag.get(), rank.get(), n);
    const int64_t U = read_scalar(rank.get() + n);
    XR_REQUIRE(U >= 1 && U <= n, XR_ERR_INVALID, "unique rows: %lld representatives of %lld rows", (long long)U, (long long)n);
    out.n_unique = U;

    DevBuf<uint64_t> keys((size_t)U * 4);
    DevBuf<int32_t> id_buf((size_t)U * 2);
    uint64_t *key_x[2] = {keys.get(), keys.get() + U}, *key_y[2] = {keys.get() + 2 * U, keys.get() + 3 * U};
    int32_t *ids[2] = {id_buf.get(), id_buf.get() + U};
    XR_LAUNCH("unique_compact", k_unique_compact, dim3(div_up(n, 256)), dim3(256), 0, xy, flag.get(), rank.get(), n, U, key_x[0], key_y[0], ids[0]);
    const int at = radix_sort_keys(key_x, key_y, ids, U, pass_mask) ? 1 : 0;

    out.xy.alloc((size_t)U * 2), out.index.alloc((size_t)U), out.inverse.alloc((size_t)n);
    // (`flag` has been read for the last time: it holds the sorted rank of every representative from here on)
    XR_LAUNCH("unique_emit", k_unique_emit, dim3(div_up(U, 256)), dim3(256), 0, xy, ids[at], U, n, reinterpret_cast<double2 *>(out.xy.get()),
              out.index.get(), flag.get());
    XR_LAUNCH("merge_inverse", k_merge_inverse, dim3(div_up(n, 256)), dim3(256), 0, rep.get(), flag.get(), n, out.inverse.get());
}

// ---- (N, M, 4) bounds -----------------------------------------------------------------------------------------------------------
struct Quad {
    double2 a, b, c, d;
};

__device__ __forceinline__ bool xy_less(const double2 &p, const double2 &q) { return p.x < q.x || (p.x == q.x && p.y < q.y); }

// ascending by (x, y): the odd-even transposition network on four registers, neighbours only and `<` only, so equal corners
// keep their order (np.lexsort is stable)
__device__ __forceinline__ void order_corners(double2 &p, double2 &q) {
    if (xy_less(q, p)) {
        const double2 t = p;
        p = q;
        q = t;
    }
}
__device__ __forceinline__ void sort_corners(Quad &v) {
    order_corners(v.a, v.b), order_corners(v.c, v.d);
    order_corners(v.b, v.c);
    order_corners(v.a, v.b), order_corners(v.c, v.d);
    order_corners(v.b, v.c);
}

__device__ __forceinline__ Quad load_corners(const double *__restrict__ x, const double *__restrict__ y, int64_t cell) {
    const double *xs = x + 4 * cell, *ys = y + 4 * cell;
    Quad v{make_double2(xs[0], ys[0]), make_double2(xs[1], ys[1]), make_double2(xs[2], ys[2]), make_double2(xs[3], ys[3])};
    sort_corners(v);
    return v;
}

__device__ __forceinline__ bool differs(const double2 &p, const double2 &q) { return p.x != q.x || p.y != q.y; }

// corners that differ from their cyclic predecessor (a NaN differs from everything)
__device__ __forceinline__ int count_unique(const Quad &v) { return differs(v.a, v.d) + differs(v.b, v.a) + differs(v.c, v.b) + differs(v.d, v.c); }

__device__ __forceinline__ double cross_from(const double2 &o, const double2 &p, const double2 &q) {
    const double ax = p.x - o.x, ay = p.y - o.y, bx = q.x - o.x, by = q.y - o.y;
    return ax * by - ay * bx;
}

// conversion.quad_area on the sorted corners: the fan from the first corner, |.| per triangle, summed left to right
__device__ __forceinline__ double fan_area(const Quad &v) {
    return 0.5 * ((fabs(cross_from(v.a, v.a, v.b)) + fabs(cross_from(v.a, v.b, v.c))) + fabs(cross_from(v.a, v.c, v.d)));
}

enum BoundsStatus : int { BS_INVALID = 0, BS_COUNT = 2 };

// one thread per cell: keep[c] = valid and finite (also as a byte for the caller), the count of cells that are not valid
__global__ void __launch_bounds__(256)
k_bounds_test(const double *__restrict__ x, const double *__restrict__ y, int64_t n_cell, int32_t *__restrict__ keep, uint8_t *__restrict__ index,
              int32_t *__restrict__ status) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool invalid = false;
    if (c < n_cell) {
        const Quad v = load_corners(x, y, c);
        const bool valid = count_unique(v) >= 3 && fan_area(v) > 0.0;
        const bool finite = isfinite(v.a.x) && isfinite(v.a.y) && isfinite(v.b.x) && isfinite(v.b.y) && isfinite(v.c.x) && isfinite(v.c.y) &&
                            isfinite(v.d.x) && isfinite(v.d.y);
        invalid = !valid;
        keep[c] = valid && finite;
        index[c] = valid && finite;
    }
    wave_count(invalid, status + BS_INVALID);
}

__device__ __forceinline__ void order_angles(double &s, double2 &p, double &t, double2 &q) {
    if (t < s) {
        const double u = s;
        s = t;
        t = u;
        const double2 r = p;
        p = q;
        q = r;
    }
}

// one thread per cell, kept cells only: the sorted corners by their angle about the mean corner, into row rank[c]
__global__ void __launch_bounds__(256)
k_bounds_orient(const double *__restrict__ x, const double *__restrict__ y, int64_t n_cell, const int32_t *__restrict__ keep,
                const int32_t *__restrict__ rank, int64_t n_kept, double2 *__restrict__ rows, uint8_t *__restrict__ triangle) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cell || !keep[c]) return;
    const int64_t j = rank[c];
    if (j < 0 || j >= n_kept) return;
    Quad v = load_corners(x, y, c);
    const int n_unique = count_unique(v);
    const double mx = (((v.a.x + v.b.x) + v.c.x) + v.d.x) / 4.0, my = (((v.a.y + v.b.y) + v.c.y) + v.d.y) / 4.0;
    const double ta = atan2(v.a.y - my, v.a.x - mx), tb = atan2(v.b.y - my, v.b.x - mx), tc = atan2(v.c.y - my, v.c.x - mx),
                 td = atan2(v.d.y - my, v.d.x - mx);
    // a corner at its predecessor's angle goes last (the angles compared are the computed ones, as in the reference's mask)
    double sa = ta, sb = tb == ta ? INFINITY : tb, sc = tc == tb ? INFINITY : tc, sd = td == tc ? INFINITY : td;
    order_angles(sa, v.a, sb, v.b), order_angles(sc, v.c, sd, v.d);
    order_angles(sb, v.b, sc, v.c);
    order_angles(sa, v.a, sb, v.b), order_angles(sc, v.c, sd, v.d);
    order_angles(sb, v.b, sc, v.c);
    rows[4 * j] = v.a, rows[4 * j + 1] = v.b, rows[4 * j + 2] = v.c, rows[4 * j + 3] = v.d;
    triangle[j] = n_unique == 3;
}

// one thread per slot of the kept faces: the node of the corner, -1 in the last slot of a triangle
__global__ void __launch_bounds__(256)
k_bounds_faces(const int32_t *__restrict__ inverse, const uint8_t *__restrict__ triangle, int64_t n_slot, int32_t *__restrict__ faces) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_slot) return;
    faces[t] = (t & 3) == 3 && triangle[t >> 2] ? -1 : inverse[t];
}

// ---- interval breaks and lattices ---------------------------------------------------------------------------------------------------
enum BreakStatus : int { BK_NOT_ASCENDING = 0, BK_NOT_DESCENDING = 1, BK_COUNT = 2 };

// conversion.infer_interval_breaks along `axis` of a (rows, cols) array, one thread per output element; a thread of an inner
// break also tests the pair of inputs around it for the monotonic check (status: some pair does not ascend / does not descend)
__global__ void __launch_bounds__(256)
k_interval_breaks(const double *__restrict__ coord, int64_t rows, int64_t cols, int axis, double *__restrict__ out, int32_t *__restrict__ status) {
    const int64_t out_cols = cols + (axis == 1), n_out = (rows + (axis == 0)) * out_cols;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool not_ascending = false, not_descending = false;
    if (t < n_out) {
        const int64_t r = t / out_cols, c = t - r * out_cols;
        const int64_t n = axis == 0 ? rows : cols, j = axis == 0 ? r : c, stride = axis == 0 ? cols : 1;
        const double *line = coord + (axis == 0 ? c : r * cols); // element k of the line: line[k * stride]
        double value;
        if (n == 1) value = j == 0 ? line[0] - 0.0 : line[0] + 0.0;
        else if (j == 0) value = line[0] - 0.5 * (line[stride] - line[0]);
        else if (j == n) value = line[(n - 1) * stride] + 0.5 * (line[(n - 1) * stride] - line[(n - 2) * stride]);
        else {
            const double lo = line[(j - 1) * stride], hi = line[j * stride];
            value = lo + 0.5 * (hi - lo);
            not_ascending = !(hi >= lo), not_descending = !(hi <= lo);
        }
        out[t] = value;
    }
    wave_flag(not_ascending, status + BK_NOT_ASCENDING); // (flags, not counts: of an ascending coordinate EVERY pair does not descend,
    wave_flag(not_descending, status + BK_NOT_DESCENDING); //  and an atomic per wave on one word would cost more than the breaks)
}

// the lattice of (ny + 1, nx + 1) nodes: node rows (x, y) and the quads of Ugrid2d._from_intervals_helper
__global__ void __launch_bounds__(256)
k_lattice(const double *__restrict__ x, const double *__restrict__ y, int64_t ny, int64_t nx, double2 *__restrict__ node_xy,
          int32_t *__restrict__ faces) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t w = nx + 1, n_node = (ny + 1) * w;
    if (t >= n_node) return;
    node_xy[t] = make_double2(x[t], y[t]);
    if (t >= ny * nx) return;
    const bool x_decreasing = x[1] < x[0], y_decreasing = y[w] < y[0]; // (first element of the second row: DESIGN section 7)
    const int64_t j = t / nx, i = t - j * nx;
    const int64_t left = i + x_decreasing, right = i + !x_decreasing, lower = j + y_decreasing, upper = j + !y_decreasing;
    faces[4 * t] = (int32_t)(lower * w + left), faces[4 * t + 1] = (int32_t)(lower * w + right);
    faces[4 * t + 2] = (int32_t)(upper * w + right), faces[4 * t + 3] = (int32_t)(upper * w + left);
}

// ---- rings and lines ------------------------------------------------------------------------------------------------------------------
// segment r of n_seg must be [off[r], off[r + 1]) inside [0, total), ascending, the first from 0 and the last to `total`
__device__ __forceinline__ bool bad_segment(const int64_t *__restrict__ off, int64_t r, int64_t n_seg, int64_t total) {
    const int64_t a = off[r], b = off[r + 1];
    return a < 0 || b < a || b > total || (r == 0 && a != 0) || (r == n_seg - 1 && b != total);
}

enum RingStatus : int { RS_SHORT = 0, RS_OPEN = 1, RS_OFFSETS = 2, RS_HOLES = 3, RS_LONGEST = 4, RS_COUNT = 5 };

// one thread per offset pair: rings [off[r], off[r + 1]) must lie in [0, n_vertex), ascending, from 0 to n_vertex; a ring needs
// four vertices and first == last; the longest ring.  Polygons (n_poly > 0 pairs of poly_off) likewise cover the rings from 0 to
// n_ring; one with more than one ring has a hole.
__global__ void __launch_bounds__(256)
k_ring_check(const double2 *__restrict__ xy, int64_t n_vertex, const int64_t *__restrict__ off, int64_t n_ring, const int64_t *__restrict__ poly_off,
             int64_t n_poly, int32_t *__restrict__ status) {
    __shared__ int32_t lds[4];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad_off = false, is_short = false, is_open = false, hole = false;
    int32_t len = 0;
    if (r < n_ring) {
        const int64_t a = off[r], b = off[r + 1];
        bad_off = bad_segment(off, r, n_ring, n_vertex);
        if (!bad_off) {
            is_short = b - a < 4;
            if (!is_short) {
                const double2 p = xy[a], q = xy[b - 1];
                is_open = !(p.x == q.x && p.y == q.y);
                len = (int32_t)std::min<int64_t>(b - a - 1, INT32_MAX);
            }
        }
    }
    if (r < n_poly) { // (all polygons of one ring, from 0 to n_ring: poly_off counts up by one)
        const int64_t a = poly_off[r], b = poly_off[r + 1];
        hole = b - a > 1;
        bad_off |= b - a < 1 || bad_segment(poly_off, r, n_poly, n_ring);
    }
    wave_count(bad_off, status + RS_OFFSETS);
    wave_count(is_short, status + RS_SHORT);
    wave_count(is_open, status + RS_OPEN);
    wave_count(hole, status + RS_HOLES);
    block_reduce<256, OpMax>(lds, len);
    if (threadIdx.x == 0 && len > 0) atomicMax(status + RS_LONGEST, len);
}

// the segment [off[s], off[s + 1]) that holds v, for checked offsets (ascending, off[0] = 0 <= v < off[n_seg])
__device__ __forceinline__ int64_t segment_of(const int64_t *__restrict__ off, int64_t n_seg, int64_t v) {
    int64_t lo = 0, hi = n_seg; // off[lo] <= v < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one thread per vertex: every vertex but its ring's last goes to row v - ring (every ring before it gave up one)
__global__ void __launch_bounds__(256)
k_ring_rows(const double2 *__restrict__ xy, int64_t n_vertex, const int64_t *__restrict__ off, int64_t n_ring, double2 *__restrict__ rows) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertex) return;
    const int64_t r = segment_of(off, n_ring, v);
    if (v != off[r + 1] - 1) rows[v - r] = xy[v];
}

// one thread per slot of the (n_ring, m) faces
__global__ void __launch_bounds__(256)
k_ring_faces(const int32_t *__restrict__ inverse, const int64_t *__restrict__ off, int64_t n_ring, int m, int32_t *__restrict__ faces) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_ring * m) return;
    const int64_t r = t / m, k = t - r * m;
    const int64_t a = off[r], len = off[r + 1] - a - 1;
    faces[t] = k < len ? inverse[a - r + k] : -1;
}

// faces -> closed rings: len[f] = the face's nodes + 1, 0 for a face without nodes
__global__ void __launch_bounds__(256) k_face_ring_len(const int32_t *__restrict__ faces, int64_t n_face, int m, int64_t n_node, int32_t *__restrict__ len) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int n = 0;
    for (int k = 0; k < m; k++) {
        const int32_t node = faces[f * m + k];
        n += node >= 0 && node < n_node;
    }
    len[f] = n > 0 ? n + 1 : 0; // (a face without a node gives an empty ring)
}

// out[i] = i: the polygon offsets of one ring per polygon
__global__ void __launch_bounds__(256) k_count_up(int64_t n, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = i;
}

__global__ void __launch_bounds__(256)
k_face_ring_coords(const int32_t *__restrict__ faces, int64_t n_face, int m, const double2 *__restrict__ node_xy, int64_t n_node,
                   const int64_t *__restrict__ off, int64_t n_vertex, double2 *__restrict__ coords) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int64_t at = off[f];
    const int64_t end = off[f + 1];
    if (at < 0 || end > n_vertex) return;
    int32_t first = -1;
    for (int k = 0; k < m; k++) {
        const int32_t node = faces[f * m + k];
        if (node < 0 || node >= n_node) continue;
        if (first < 0) first = node;
        if (at < end) coords[at++] = node_xy[node];
    }
    if (first >= 0 && at < end) coords[at] = node_xy[first];
}

// one thread per vertex: flag[v] = v and v + 1 are consecutive vertices of one line
__global__ void __launch_bounds__(256)
k_line_flags(int64_t n_vertex, const int64_t *__restrict__ off, int64_t n_line, int32_t *__restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertex) return;
    flag[v] = v + 1 < n_vertex && v + 1 < off[segment_of(off, n_line, v) + 1];
}

__global__ void __launch_bounds__(256)
k_line_edges(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n_vertex, int64_t n_edge, const int32_t *__restrict__ inverse,
             int64_t *__restrict__ edges) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertex || !flag[v]) return;
    const int64_t e = rank[v];
    if (e < 0 || e >= n_edge) return;
    edges[2 * e] = inverse[v], edges[2 * e + 1] = inverse[v + 1];
}

// offsets of line segments without rings: ascending from 0 to n_vertex
__global__ void __launch_bounds__(256) k_offsets_check(const int64_t *__restrict__ off, int64_t n_seg, int64_t n_vertex, int32_t *__restrict__ status) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    wave_count(r < n_seg && bad_segment(off, r, n_seg, n_vertex), status);
}

// a mesh from the unique rows (its nodes) -- `fill_faces(faces_raw)` launches what writes the connectivity
template <typename FILL> static xr_mesh *mesh_of_unique(UniqueRows &nodes, int64_t n_face, int m, FILL &&fill_faces) {
    Building<xr_mesh> mesh = new_raw_mesh(nodes.n_unique, n_face, m, OnFailure::WaitFirst);
    if (nodes.n_unique > 0)
        XR_HIP(hipMemcpyAsync(mesh->node_xy.get(), nodes.xy.get(), (size_t)nodes.n_unique * 16, hipMemcpyDeviceToDevice, launch_stream()));
    if (n_face > 0) fill_faces(mesh->faces_raw.get());
    stream_sync(); // (the work arrays go back to the pool behind their readers)
    return mesh.release();
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_unique_xy_dev(const double *xy_dev, int64_t n, xr_unique_xy **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (xy_dev || n == 0) && n >= 0, XR_ERR_INVALID, "xr_unique_xy_dev: bad argument");
    Building<xr_unique_xy> unique(OnFailure::WaitFirst);
    unique_rows(reinterpret_cast<const double2 *>(xy_dev), n, unique->rows);
    stream_sync();
    *out = unique.release();
    XR_API_END
}

int xr_unique_xy_info(const xr_unique_xy *unique, int64_t *sizes) {
    XR_API_BEGIN
    XR_REQUIRE(unique && sizes, XR_ERR_INVALID, "xr_unique_xy_info: NULL argument");
    const UniqueRows &rows = unique->rows;
    sizes[0] = rows.n, sizes[1] = rows.n_unique, sizes[2] = rows.n_nonfinite, sizes[3] = rows.passes_run, sizes[4] = rows.passes_skipped;
    XR_API_END
}

int xr_unique_xy_copy_dev(const xr_unique_xy *unique, int what, void *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(unique && what >= 0 && what <= 2 && unique->rows.n_nonfinite == 0, XR_ERR_INVALID, "xr_unique_xy_copy_dev: bad argument");
    const UniqueRows &rows = unique->rows;
    const int64_t count = what == 2 ? rows.n : rows.n_unique;
    XR_REQUIRE(out_dev || count == 0, XR_ERR_INVALID, "xr_unique_xy_copy_dev: NULL argument");
    if (what == 0) {
        if (count > 0) XR_HIP(hipMemcpyAsync(out_dev, rows.xy.get(), (size_t)count * 16, hipMemcpyDeviceToDevice, launch_stream()));
    } else {
        widen_dev(what == 1 ? rows.index.get() : rows.inverse.get(), count, static_cast<int64_t *>(out_dev));
    }
    dev_call_done();
    XR_API_END
}

int xr_unique_xy_destroy(xr_unique_xy *unique) {
    XR_API_BEGIN
    if (unique) {
        release_point();
        delete unique;
    }
    XR_API_END
}

int xr_mesh_from_bounds_dev(const double *x_dev, const double *y_dev, int64_t n_cell, xr_mesh **out, uint8_t *index_out_dev, int64_t *counts) {
    XR_API_BEGIN
    XR_REQUIRE(out && counts && n_cell >= 0 && ((x_dev && y_dev && index_out_dev) || n_cell == 0), XR_ERR_INVALID,
               "xr_mesh_from_bounds_dev: bad argument");
    XR_REQUIRE(n_cell < ((int64_t)1 << 28), XR_ERR_LIMIT, "xr_mesh_from_bounds_dev: %lld cells exceed the int32 index range", (long long)n_cell);
    for (int k = 0; k < 4; k++) counts[k] = 0;
    int64_t n_kept = 0;
    UniqueRows nodes;
    DevBuf<uint8_t> triangle;
    if (n_cell > 0) {
        DevBuf<int32_t> keep((size_t)n_cell), rank((size_t)n_cell + 1), status(BS_COUNT);
        fill_i32(status.get(), 0, BS_COUNT);
        XR_LAUNCH("bounds_test", k_bounds_test, dim3(div_up(n_cell, 256)), dim3(256), 0, x_dev, y_dev, n_cell, keep.get(), index_out_dev, status.get());
        exclusive_scan_i32(keep.get(), rank.get(), n_cell);
        n_kept = read_scalar(rank.get() + n_cell);
        counts[1] = read_scalar(status.get() + BS_INVALID);
        XR_REQUIRE(n_kept >= 0 && n_kept <= n_cell, XR_ERR_INVALID, "xr_mesh_from_bounds_dev: %lld cells kept of %lld", (long long)n_kept, (long long)n_cell);
        DevBuf<double> rows((size_t)n_kept * 8);
        triangle.alloc((size_t)n_kept);
        if (n_kept > 0)
            XR_LAUNCH("bounds_orient", k_bounds_orient, dim3(div_up(n_cell, 256)), dim3(256), 0, x_dev, y_dev, n_cell, keep.get(), rank.get(), n_kept,
                      reinterpret_cast<double2 *>(rows.get()), triangle.get());
        unique_rows(reinterpret_cast<const double2 *>(rows.get()), 4 * n_kept, nodes);
        XR_REQUIRE(nodes.n_nonfinite == 0, XR_ERR_INVALID, "xr_mesh_from_bounds_dev: non-finite corner among the kept cells");
        stream_sync(); // (`rows` goes back to the pool here)
    } else {
        unique_rows(nullptr, 0, nodes);
    }
    counts[0] = n_kept, counts[2] = nodes.passes_run, counts[3] = nodes.passes_skipped;
    *out = mesh_of_unique(nodes, n_kept, 4, [&](int32_t *faces) {
        XR_LAUNCH("bounds_faces", k_bounds_faces, dim3(div_up(4 * n_kept, 256)), dim3(256), 0, nodes.inverse.get(), triangle.get(), 4 * n_kept, faces);
    });
    XR_API_END
}

int xr_interval_breaks_dev(const double *coord_dev, int64_t rows, int64_t cols, int axis, double *out_dev, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(coord_dev && out_dev && problems && rows >= 1 && cols >= 1 && (axis == 0 || axis == 1), XR_ERR_INVALID,
               "xr_interval_breaks_dev: bad argument");
    const int64_t n_out = (rows + (axis == 0)) * (cols + (axis == 1));
    XR_REQUIRE(n_out < INT32_MAX, XR_ERR_LIMIT, "xr_interval_breaks_dev: %lld breaks exceed the int32 index range", (long long)n_out);
    DevBuf<int32_t> status(BK_COUNT);
    fill_i32(status.get(), 0, BK_COUNT);
    XR_LAUNCH("interval_breaks", k_interval_breaks, dim3(div_up(n_out, 256)), dim3(256), 0, coord_dev, rows, cols, axis, out_dev, status.get());
    int32_t h[BK_COUNT];
    d2h(h, status.get(), sizeof(h));
    problems[0] = h[BK_NOT_ASCENDING], problems[1] = h[BK_NOT_DESCENDING];
    XR_API_END
}

int xr_mesh_from_intervals_dev(const double *x_dev, const double *y_dev, int64_t ny, int64_t nx, xr_mesh **out) {
    XR_API_BEGIN
    XR_REQUIRE(x_dev && y_dev && out && ny >= 1 && nx >= 1, XR_ERR_INVALID, "xr_mesh_from_intervals_dev: bad argument");
    const int64_t n_node = (ny + 1) * (nx + 1);
    XR_REQUIRE(n_node < INT32_MAX / 4, XR_ERR_LIMIT, "xr_mesh_from_intervals_dev: %lld nodes exceed the int32 index range", (long long)n_node);
    Building<xr_mesh> mesh = new_raw_mesh(n_node, ny * nx, 4, OnFailure::WaitFirst);
    XR_LAUNCH("lattice", k_lattice, dim3(div_up(n_node, 256)), dim3(256), 0, x_dev, y_dev, ny, nx, reinterpret_cast<double2 *>(mesh->node_xy.get()),
              mesh->faces_raw.get());
    stream_sync();
    *out = mesh.release();
    XR_API_END
}

int xr_mesh_from_rings_dev(const double *coords_dev, int64_t n_vertex, const int64_t *ring_off_dev, int64_t n_ring, const int64_t *poly_off_dev,
                           int64_t n_poly, xr_mesh **out, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(out && problems && n_vertex >= 0 && n_ring >= 0 && n_poly >= 0 && (coords_dev || n_vertex == 0) && ring_off_dev &&
                   (poly_off_dev || n_poly == 0),
               XR_ERR_INVALID, "xr_mesh_from_rings_dev: bad argument");
    XR_REQUIRE(n_vertex < ((int64_t)1 << 30), XR_ERR_LIMIT, "xr_mesh_from_rings_dev: %lld vertices exceed the int32 index range", (long long)n_vertex);
    *out = nullptr;
    for (int k = 0; k < 5; k++) problems[k] = 0;
    if (n_ring == 0 && n_vertex > 0) problems[RS_OFFSETS] = 1;
    int m = 3;
    const int64_t n_check = std::max(n_ring, n_poly);
    if (n_check > 0) {
        DevBuf<int32_t> status(RS_COUNT);
        fill_i32(status.get(), 0, RS_COUNT);
        XR_LAUNCH("ring_check", k_ring_check, dim3(div_up(n_check, 256)), dim3(256), 0, reinterpret_cast<const double2 *>(coords_dev), n_vertex,
                  ring_off_dev, n_ring, poly_off_dev, n_poly, status.get());
        int32_t h[RS_COUNT];
        d2h(h, status.get(), sizeof(h));
        for (int k = 0; k < 4; k++) problems[k] += h[k];
        m = std::max(3, (int)h[RS_LONGEST]);
    }
    if (problems[0] || problems[1] || problems[2] || problems[3]) return XR_OK; // (the caller words the error; no mesh)
    XR_REQUIRE((int64_t)m * n_ring < INT32_MAX, XR_ERR_LIMIT, "xr_mesh_from_rings_dev: %lld face slots exceed the int32 index range",
               (long long)m * (long long)n_ring);
    const int64_t n_row = n_vertex - n_ring;
    UniqueRows nodes;
    DevBuf<double> rows((size_t)n_row * 2);
    if (n_row > 0)
        XR_LAUNCH("ring_rows", k_ring_rows, dim3(div_up(n_vertex, 256)), dim3(256), 0, reinterpret_cast<const double2 *>(coords_dev), n_vertex,
                  ring_off_dev, n_ring, reinterpret_cast<double2 *>(rows.get()));
    unique_rows(reinterpret_cast<const double2 *>(rows.get()), n_row, nodes);
    if (nodes.n_nonfinite > 0) {
        stream_sync();
        problems[4] = nodes.n_nonfinite;
        return XR_OK;
    }
    *out = mesh_of_unique(nodes, n_ring, m, [&](int32_t *faces) {
        XR_LAUNCH("ring_faces", k_ring_faces, dim3(div_up(n_ring * m, 256)), dim3(256), 0, nodes.inverse.get(), ring_off_dev, n_ring, m, faces);
    });
    XR_API_END
}

int xr_mesh_ring_offsets_dev(const xr_mesh *mesh, int64_t *ring_off_out_dev, int64_t *poly_off_out_dev, int64_t *n_vertex) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && ring_off_out_dev && n_vertex, XR_ERR_INVALID, "xr_mesh_ring_offsets_dev: NULL argument");
    const int64_t F = mesh->n_face;
    XR_REQUIRE(F * (mesh->m + 1) < INT32_MAX, XR_ERR_LIMIT, "xr_mesh_ring_offsets_dev: the ring vertices exceed the int32 index range");
    DevBuf<int32_t> len((size_t)F), off((size_t)F + 1);
    if (F > 0)
        XR_LAUNCH("face_ring_len", k_face_ring_len, dim3(div_up(F, 256)), dim3(256), 0, mesh->faces_raw.get(), F, mesh->m, mesh->n_node, len.get());
    rank_of_flags(len.get(), off.get(), F);
    widen_dev(off.get(), F + 1, ring_off_out_dev);
    if (poly_off_out_dev) XR_LAUNCH("count_up", k_count_up, dim3(div_up(F + 1, 256)), dim3(256), 0, F + 1, poly_off_out_dev);
    *n_vertex = read_scalar(off.get() + F);
    stream_sync();
    XR_API_END
}

int xr_mesh_ring_coords_dev(const xr_mesh *mesh, const int64_t *ring_off_dev, int64_t n_vertex, double *coords_out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && ring_off_dev && n_vertex >= 0 && (coords_out_dev || n_vertex == 0), XR_ERR_INVALID, "xr_mesh_ring_coords_dev: bad argument");
    const int64_t F = mesh->n_face;
    if (F > 0)
        XR_LAUNCH("face_ring_coords", k_face_ring_coords, dim3(div_up(F, 256)), dim3(256), 0, mesh->faces_raw.get(), F, mesh->m,
                  reinterpret_cast<const double2 *>(mesh->node_xy.get()), mesh->n_node, ring_off_dev, n_vertex,
                  reinterpret_cast<double2 *>(coords_out_dev));
    dev_call_done();
    XR_API_END
}

int xr_lines_to_network_dev(const double *coords_dev, int64_t n_vertex, const int64_t *line_off_dev, int64_t n_line, xr_unique_xy **nodes_out,
                            int64_t *edges_out_dev, int64_t *counts) {
    XR_API_BEGIN
    XR_REQUIRE(nodes_out && counts && n_vertex >= 0 && n_line >= 0 && (coords_dev || n_vertex == 0) && line_off_dev && (edges_out_dev || n_vertex < 2),
               XR_ERR_INVALID, "xr_lines_to_network_dev: bad argument");
    *nodes_out = nullptr;
    counts[0] = counts[1] = counts[2] = 0;
    if (n_line == 0 && n_vertex > 0) counts[1] = 1;
    if (n_line > 0) {
        DevBuf<int32_t> status(1);
        fill_i32(status.get(), 0, 1);
        XR_LAUNCH("offsets_check", k_offsets_check, dim3(div_up(n_line, 256)), dim3(256), 0, line_off_dev, n_line, n_vertex, status.get());
        counts[1] = read_scalar(status.get());
    }
    if (counts[1]) return XR_OK;
    Building<xr_unique_xy> unique(OnFailure::WaitFirst);
    unique_rows(reinterpret_cast<const double2 *>(coords_dev), n_vertex, unique->rows);
    counts[2] = unique->rows.n_nonfinite;
    if (n_vertex > 0 && counts[2] == 0) {
        DevBuf<int32_t> flag((size_t)n_vertex), rank((size_t)n_vertex + 1);
        XR_LAUNCH("line_flags", k_line_flags, dim3(div_up(n_vertex, 256)), dim3(256), 0, n_vertex, line_off_dev, n_line, flag.get());
        exclusive_scan_i32(flag.get(), rank.get(), n_vertex);
        const int64_t n_edge = read_scalar(rank.get() + n_vertex);
        XR_REQUIRE(n_edge >= 0 && n_edge < n_vertex, XR_ERR_INVALID, "xr_lines_to_network_dev: %lld edges of %lld vertices", (long long)n_edge,
                   (long long)n_vertex);
        counts[0] = n_edge;
        if (n_edge > 0)
            XR_LAUNCH("line_edges", k_line_edges, dim3(div_up(n_vertex, 256)), dim3(256), 0, flag.get(), rank.get(), n_vertex, n_edge,
                      unique->rows.inverse.get(), edges_out_dev);
    }
    stream_sync();
    *nodes_out = unique.release();
    XR_API_END
}

} // extern "C"
