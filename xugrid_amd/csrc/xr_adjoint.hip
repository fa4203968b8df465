// xr_adjoint.hip -- the adjoint of the sparse apply for the reducers that are linear in the source values for a fixed NaN
// pattern (mean, sum, first_order_conservative / conductance, select): target-side quantities (K, T) back onto the source
// (K, S).  The contract is in include/xugrid_amd.h; DESIGN section 23 has the kernels and the measurements.
//
// Three parts:
//   1. the transposed weights, built once per matrix on the device and kept on the xr_csr next to the apply plan: histogram of
//      the columns -> scan -> fill through per-column cursors (integer atomics decide a slot, never a value) -> every column
//      segment sorted by the 64-bit key (row << 32 | storage position), which makes the structure independent of the order
//      the atomics arrived in;
//   2. the row pass: Wsum[k, i] by the forward reducers' own walks (Red<METHOD>::add, sequential up to APPLY_LONG entries,
//      the lane-group / wave / block order beyond), r[k, i] = g[k, i] (/ Wsum) into a (K, T) scratch, 0 where the row is not live;
//   3. the column pass: a[k, j] = sum over the column's entries of r[k, i] * coefficient, GATHERED per destination in a fixed
//      order.  No floating-point atomics anywhere: two calls give the same bits.
// A row that is not live has r = +0.0, and its terms are added like any other: x + (+-0.0) = x for every x the sum can hold
// (it starts at +0.0 and can therefore never be -0.0), so "contributes nothing" costs no branch.
#include <algorithm>

#include "xr_apply.h"
#include "xr_prims.h"
#include "xr_reduce.h"

namespace xr {

static constexpr int ADJ_KT = 8;                    // variables per pass over a row or column (registers)
static constexpr uint32_t TR_LAST = 0x80000000u;    // tr_row: the entry is the last of its row
static constexpr uint32_t TR_ROW_MASK = 0x7fffffffu;

template <typename F> static void with_adjoint_reducer(int method, F &&f) {
    const bool known = with_id<XR_MEAN, XR_SUM, XR_FIRST_ORDER_CONSERVATIVE, XR_SELECT>(method, f);
    XR_REQUIRE(known, XR_ERR_INVALID,
               "the adjoint apply serves mean (0), sum (3), first_order_conservative (8) and select (10): reducer id %d is not "
               "linear in the source values",
               method);
}

// ---------------------------------------------------------------------------------------------
// 1. transposed weights
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int caller_col(const int32_t *__restrict__ col_of, int c) { return col_of ? col_of[c] : c; }

__global__ void __launch_bounds__(256)
k_tr_count(const int32_t *__restrict__ indices, const int32_t *__restrict__ col_of, int64_t nnz, int32_t *__restrict__ count) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < nnz) atomicAdd(&count[caller_col(col_of, indices[p])], 1);
}

// one wave per stored row: key = (output row << 32) | last-of-row flag | storage position.  The flag sits above the position,
// and the last entry of a row has the row's largest position anyway: the order by key is the order by (row, position).
__global__ void __launch_bounds__(256)
k_tr_fill(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ row_order,
          const int32_t *__restrict__ col_of, int64_t n, const int32_t *__restrict__ start, int32_t *__restrict__ cursor,
          uint64_t *__restrict__ keys) {
    const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (t >= n) return;
    const int s = indptr[t], e = indptr[t + 1];
    const uint64_t row = (uint64_t)(uint32_t)(row_order ? row_order[t] : (int32_t)t) << 32;
    for (int p = s + lane; p < e; p += 64) {
        const int c = caller_col(col_of, indices[p]);
        const int slot = start[c] + atomicAdd(&cursor[c], 1);
        keys[slot] = row | (p == e - 1 ? TR_LAST : 0u) | (uint32_t)p;
    }
}

// columns of at most APPLY_LONG entries: one thread sorts its segment (insertion: the cursors hand the slots out in nearly
// ascending order).  Longer ones are flagged for the block sort; stats[0] = the longest column.
__global__ void __launch_bounds__(256)
k_tr_sort_short(const int32_t *__restrict__ start, int64_t m, uint64_t *__restrict__ keys, int32_t *__restrict__ is_long,
                int32_t *__restrict__ stats) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int len = 0;
    if (j < m) {
        const int s = start[j];
        len = start[j + 1] - s;
        is_long[j] = len > APPLY_LONG;
        if (len <= APPLY_LONG) {
            uint64_t *seg = keys + s;
            for (int a = 1; a < len; a++) {
                const uint64_t key = seg[a];
                int b = a - 1;
                while (b >= 0 && seg[b] > key) {
                    seg[b + 1] = seg[b];
                    b--;
                }
                seg[b + 1] = key;
            }
        }
    }
    const int longest = wave_reduce<OpMax>(len);
    if ((threadIdx.x & 63) == 0 && longest > 0) atomicMax(&stats[0], longest);
}

// one block per listed column
__global__ void __launch_bounds__(256)
k_tr_sort_long(const int32_t *__restrict__ start, const int32_t *__restrict__ long_cols, int n_long, uint64_t *__restrict__ keys) {
    for (int li = blockIdx.x; li < n_long; li += gridDim.x) {
        const int j = long_cols[li];
        const int s = start[j];
        block_sort_ascending<256>(keys + s, (int64_t)(start[j + 1] - s));
    }
}

__global__ void __launch_bounds__(256)
k_tr_finish(const uint64_t *__restrict__ keys, const double *__restrict__ data, int64_t nnz, uint32_t *__restrict__ tr_row,
            double *__restrict__ tr_w) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nnz) return;
    const uint64_t key = keys[q];
    const uint32_t low = (uint32_t)key;
    tr_row[q] = (uint32_t)(key >> 32) | (low & TR_LAST);
    tr_w[q] = data[low & TR_ROW_MASK];
}

__global__ void __launch_bounds__(256) k_tr_row_ids(const uint32_t *__restrict__ tr_row, int64_t nnz, int32_t *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < nnz) out[q] = (int32_t)(tr_row[q] & TR_ROW_MASK);
}

void ensure_transposed(const xr_csr *ccsr) {
    xr_csr *csr = const_cast<xr_csr *>(ccsr); // like the plan: a cache attached to the weights
    if (csr->tr.ready && csr->tr.output_stored == csr->stored.output_stored) return;
    XR_REQUIRE(exclusive_held(), XR_ERR_INVALID, "internal: transposed weights requested outside the exclusive scope");
    csr->tr.release();
    const int64_t n = csr->n, m = csr->m, nnz = csr->nnz;
    const int32_t *col_of = csr->cols.permuted ? csr->cols.col_of.get() : nullptr;
    DevBuf<int32_t> count((size_t)m + 1), cursor((size_t)m + 1), is_long((size_t)m + 1), pos((size_t)m + 1), stats(1);
    DevBuf<uint64_t> keys((size_t)nnz);
    csr->tr.indptr.alloc((size_t)m + 1);
    fill_i32(count.get(), 0, m + 1);
    fill_i32(cursor.get(), 0, m + 1);
    fill_i32(stats.get(), 0, 1);
    if (nnz > 0) XR_LAUNCH("tr_count", k_tr_count, dim3(div_up(nnz, 256)), dim3(256), 0, csr->indices.get(), col_of, nnz, count.get());
    if (m > 0) exclusive_scan_i32(count.get(), csr->tr.indptr.get(), m);
    else fill_i32(csr->tr.indptr.get(), 0, 1);
    if (nnz > 0)
        XR_LAUNCH("tr_fill", k_tr_fill, dim3(div_up(n * 64, 256)), dim3(256), 0, csr->indptr.get(), csr->indices.get(),
                  row_order_of(csr), col_of, n, csr->tr.indptr.get(), cursor.get(), keys.get());
    int32_t n_long = 0;
    if (m > 0) {
        XR_LAUNCH("tr_sort_short", k_tr_sort_short, dim3(div_up(m, 256)), dim3(256), 0, csr->tr.indptr.get(), m, keys.get(),
                  is_long.get(), stats.get());
        exclusive_scan_i32(is_long.get(), pos.get(), m);
        n_long = read_scalar(pos.get() + m);
        csr->tr.max_len = read_scalar(stats.get());
    }
    if (n_long > 0) {
        csr->tr.long_cols.alloc((size_t)n_long);
        XR_LAUNCH("tr_long_ids", k_compact_ids<int32_t>, dim3(div_up(m, 256)), dim3(256), 0, is_long.get(), pos.get(), m,
                  csr->tr.long_cols.get());
        XR_LAUNCH("tr_sort_long", k_tr_sort_long, dim3((unsigned)std::min<int64_t>(n_long, (int64_t)engine().num_cu * 32)),
                  dim3(256), 0, csr->tr.indptr.get(), csr->tr.long_cols.get(), n_long, keys.get());
    }
    csr->tr.row.alloc((size_t)nnz);
    csr->tr.w.alloc((size_t)nnz);
    if (nnz > 0)
        XR_LAUNCH("tr_finish", k_tr_finish, dim3(div_up(nnz, 256)), dim3(256), 0, keys.get(), csr->data.get(), nnz,
                  csr->tr.row.get(), csr->tr.w.get());
    csr->tr.n_long = n_long;
    csr->tr.output_stored = csr->stored.output_stored;
    csr->tr.ready = true;
}

int prepare_for_adjoint(const xr_csr *csr, int method) {
    XR_API_BEGIN
    with_adjoint_reducer(method, [](auto) {}); // (a reducer without an adjoint builds nothing)
    if (csr && !(csr->tr.ready && csr->tr.output_stored == csr->stored.output_stored)) {
        ensure_transposed(csr);
        stream_sync();
    }
    XR_API_END
}

// ---------------------------------------------------------------------------------------------
// 2. row pass
// ---------------------------------------------------------------------------------------------
// (src == nullptr: no NaN in the source -- every entry is valid)
template <typename SRC> __device__ __forceinline__ double adj_value(const SRC *__restrict__ src, int64_t i) {
    return src ? ld_src(src, i) : 0.0;
}

template <int METHOD> __device__ __forceinline__ double adj_row_factor(double g, double wsum) {
    if (wsum == 0) return 0.0; // not live: the forward returned NaN here
    return METHOD == XR_MEAN ? g / wsum : g;
}

// rows of at most APPLY_LONG entries (every row when the matrix lists no long ones): one thread per stored row, the
// forward's sequential walk, ADJ_KT variables per pass
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_adj_rows(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
           const int32_t *__restrict__ row_order, bool skip_long, int64_t T, int64_t S, const SRC *__restrict__ source,
           const double *__restrict__ grad, int64_t K, double *__restrict__ r) {
    const int64_t t = (int64_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int s = indptr[t], e = indptr[t + 1];
    if (skip_long && e - s > APPLY_LONG) return;
    const int64_t t_out = row_order ? (int64_t)row_order[t] : t;
    for (int64_t k0 = (int64_t)blockIdx.y * ADJ_KT; k0 < K; k0 += (int64_t)gridDim.y * ADJ_KT) {
        const int kn = (int)((K - k0) < ADJ_KT ? (K - k0) : ADJ_KT);
        const SRC *src = source ? source + k0 * S : nullptr;
        Red<METHOD> red[ADJ_KT];
        for (int j = s; j < e; j++) {
            const int64_t col = indices[j];
            const double w = data[j];
            double v[ADJ_KT];
#pragma unroll
            for (int kk = 0; kk < ADJ_KT; kk++) v[kk] = kk < kn ? adj_value(src, (int64_t)kk * S + col) : 0.0;
#pragma unroll
            for (int kk = 0; kk < ADJ_KT; kk++)
                if (kk < kn) red[kk].add(v[kk], w, 0.0);
        }
#pragma unroll
        for (int kk = 0; kk < ADJ_KT; kk++)
            if (kk < kn) r[(k0 + kk) * T + t_out] = adj_row_factor<METHOD>(grad[(k0 + kk) * T + t_out], red[kk].b);
    }
}

// a listed row by a group of G lanes, as apply_row_group walks it: entry j goes to lane j % G, butterfly merge
template <int METHOD, typename SRC, int G>
__device__ __forceinline__ void adj_row_group(const int32_t *__restrict__ indices, const double *__restrict__ data, int s, int e,
                                              int64_t t_out, int64_t T, int64_t S, const SRC *__restrict__ source,
                                              const double *__restrict__ grad, int64_t K, double *__restrict__ r) {
    const int gl = threadIdx.x & (G - 1);
    for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
        const SRC *src = source ? source + k * S : nullptr;
        Red<METHOD> red;
        for (int j = s + gl; j < e; j += G) red.add(adj_value(src, (int64_t)indices[j]), data[j], 0.0);
        group_merge<METHOD, G>(red);
        if (gl == 0) r[k * T + t_out] = adj_row_factor<METHOD>(grad[k * T + t_out], red.b);
    }
}

// the listed rows of APPLY_LONG + 1 ... APPLY_WAVE entries (apply_wave_rows: four rows per wave up to APPLY_GROUP16 entries,
// one row per wave beyond)
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_adj_rows_wave(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
                const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows, const int32_t *__restrict__ n_long,
                int64_t T, int64_t S, const SRC *__restrict__ source, const double *__restrict__ grad, int64_t K,
                double *__restrict__ r) {
    const int wave = (blockIdx.x * AP_BLOCK + threadIdx.x) >> 6, n_waves = gridDim.x * (AP_BLOCK / 64);
    const int lane = threadIdx.x & 63;
    const int nl = *n_long;
    for (int li0 = wave * 4; li0 < nl; li0 += n_waves * 4) {
        const int li = li0 + (lane >> 4);
        int s = 0, e = 0;
        int64_t t_out = 0;
        if (li < nl) {
            const int t = long_rows[li];
            s = indptr[t];
            e = indptr[t + 1];
            t_out = row_order ? (int64_t)row_order[t] : t;
            if (e - s > APPLY_GROUP16) e = s; // second pass
        }
        // (the shuffles inside are wave-wide: every lane takes part, idle groups carry empty rows and store nothing)
        if (__any(e > s)) {
            if (e > s) adj_row_group<METHOD, SRC, 16>(indices, data, s, e, t_out, T, S, source, grad, K, r);
        }
    }
    for (int li = wave; li < nl; li += n_waves) {
        const int t = long_rows[li];
        const int s = indptr[t], e = indptr[t + 1];
        if (e - s <= APPLY_GROUP16 || e - s > APPLY_WAVE) continue;
        adj_row_group<METHOD, SRC, 64>(indices, data, s, e, row_order ? (int64_t)row_order[t] : t, T, S, source, grad, K, r);
    }
}

// the listed rows beyond APPLY_WAVE entries: one block each (apply_row_block's strided walk and block_merge)
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_adj_rows_block(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
                 const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows, const int32_t *__restrict__ n_long,
                 int64_t T, int64_t S, const SRC *__restrict__ source, const double *__restrict__ grad, int64_t K,
                 double *__restrict__ r) {
    __shared__ double lds[AP_BLOCK / 64][3];
    const int nl = *n_long;
    for (int li = blockIdx.x; li < nl; li += gridDim.x) {
        const int t = long_rows[li];
        const int s = indptr[t], e = indptr[t + 1];
        if (e - s <= APPLY_WAVE) continue; // (block-uniform)
        const int64_t t_out = row_order ? (int64_t)row_order[t] : t;
        for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
            const SRC *src = source ? source + k * S : nullptr;
            Red<METHOD> red;
            for (int j = s + threadIdx.x; j < e; j += AP_BLOCK) red.add(adj_value(src, (int64_t)indices[j]), data[j], 0.0);
            block_merge<METHOD>(red, lds);
            if (threadIdx.x == 0) r[k * T + t_out] = adj_row_factor<METHOD>(grad[k * T + t_out], red.b);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 3. column pass
// ---------------------------------------------------------------------------------------------
template <int METHOD> __device__ __forceinline__ double adj_coefficient(double w, uint32_t row_word) {
    if (METHOD == XR_SUM) return 1.0; // (zero-weight entries included: the forward adds v, not w v)
    if (METHOD == XR_SELECT) return (row_word & TR_LAST) ? 1.0 : 0.0;
    return w;
}

// a NaN in the forward input took no part in any row: nothing flows back to it (select copies NaN like any value)
template <int METHOD, typename SRC>
__device__ __forceinline__ double adj_result(const SRC *__restrict__ source, int64_t at, double sum) {
    if (METHOD != XR_SELECT && source) {
        const double v = ld_src(source, at);
        if (v != v) return 0.0;
    }
    return sum;
}

// columns of at most APPLY_LONG entries: lanes along the columns, ADJ_KT variables per pass, ascending (row, position)
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_adj_cols(const int32_t *__restrict__ tr_indptr, const uint32_t *__restrict__ tr_row, const double *__restrict__ tr_w,
           bool skip_long, int64_t T, int64_t S, const SRC *__restrict__ source, const double *__restrict__ r, int64_t K,
           double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (j >= S) return;
    const int s = tr_indptr[j], e = tr_indptr[j + 1];
    if (skip_long && e - s > APPLY_LONG) return;
    for (int64_t k0 = (int64_t)blockIdx.y * ADJ_KT; k0 < K; k0 += (int64_t)gridDim.y * ADJ_KT) {
        const int kn = (int)((K - k0) < ADJ_KT ? (K - k0) : ADJ_KT);
        double acc[ADJ_KT];
#pragma unroll
        for (int kk = 0; kk < ADJ_KT; kk++) acc[kk] = 0.0;
        for (int q = s; q < e; q++) {
            const uint32_t word = tr_row[q];
            const int64_t i = word & TR_ROW_MASK;
            const double c = adj_coefficient<METHOD>(tr_w[q], word);
            double rv[ADJ_KT];
#pragma unroll
            for (int kk = 0; kk < ADJ_KT; kk++) rv[kk] = kk < kn ? r[(k0 + kk) * T + i] : 0.0;
#pragma unroll
            for (int kk = 0; kk < ADJ_KT; kk++) acc[kk] += rv[kk] * c;
        }
#pragma unroll
        for (int kk = 0; kk < ADJ_KT; kk++)
            if (kk < kn) out[(k0 + kk) * S + j] = adj_result<METHOD>(source, (k0 + kk) * S + j, acc[kk]);
    }
}

// listed columns of APPLY_LONG + 1 ... APPLY_WAVE entries (all listed ones when `upto_wave` is false): one wave each, lane l
// takes the entries l, l + 64, ... in that order, then the xor butterfly of xr_prims.h
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_adj_cols_wave(const int32_t *__restrict__ tr_indptr, const uint32_t *__restrict__ tr_row, const double *__restrict__ tr_w,
                const int32_t *__restrict__ long_cols, int n_long, bool upto_wave, int64_t T, int64_t S,
                const SRC *__restrict__ source, const double *__restrict__ r, int64_t K, double *__restrict__ out) {
    const int wave = (blockIdx.x * AP_BLOCK + threadIdx.x) >> 6, n_waves = gridDim.x * (AP_BLOCK / 64);
    const int lane = threadIdx.x & 63;
    for (int li = wave; li < n_long; li += n_waves) {
        const int64_t j = long_cols[li];
        const int s = tr_indptr[j], e = tr_indptr[j + 1];
        if (upto_wave && e - s > APPLY_WAVE) continue; // (wave-uniform)
        for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
            double acc = 0.0;
            for (int q = s + lane; q < e; q += 64) {
                const uint32_t word = tr_row[q];
                acc += r[k * T + (int64_t)(word & TR_ROW_MASK)] * adj_coefficient<METHOD>(tr_w[q], word);
            }
            acc = wave_reduce<OpSum>(acc);
            if (lane == 0) out[k * S + j] = adj_result<METHOD>(source, k * S + j, acc);
        }
    }
}

// listed columns beyond APPLY_WAVE entries: one block each, thread t takes the entries t, t + 256, ..., then the block
// reduction of xr_prims.h
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_adj_cols_block(const int32_t *__restrict__ tr_indptr, const uint32_t *__restrict__ tr_row, const double *__restrict__ tr_w,
                 const int32_t *__restrict__ long_cols, int n_long, int64_t T, int64_t S, const SRC *__restrict__ source,
                 const double *__restrict__ r, int64_t K, double *__restrict__ out) {
    __shared__ double lds[AP_BLOCK / 64];
    for (int li = blockIdx.x; li < n_long; li += gridDim.x) {
        const int64_t j = long_cols[li];
        const int s = tr_indptr[j], e = tr_indptr[j + 1];
        if (e - s <= APPLY_WAVE) continue; // (block-uniform)
        for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
            double acc = 0.0;
            for (int q = s + threadIdx.x; q < e; q += AP_BLOCK) {
                const uint32_t word = tr_row[q];
                acc += r[k * T + (int64_t)(word & TR_ROW_MASK)] * adj_coefficient<METHOD>(tr_w[q], word);
            }
            block_reduce<AP_BLOCK, OpSum>(lds, acc);
            if (threadIdx.x == 0) out[k * S + j] = adj_result<METHOD>(source, k * S + j, acc);
            __syncthreads(); // (the next reduction reuses lds)
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
template <int METHOD, typename SRC>
static void launch_adjoint(const xr_csr *csr, const SRC *src, const SRC *src_stored, const double *grad, int64_t K, double *out) {
    const int64_t T = csr->n, S = csr->m;
    const unsigned ytiles = (unsigned)std::min<int64_t>(div_up(K, ADJ_KT), 65535);
    const unsigned ylong = (unsigned)std::min<int64_t>(K, 8);
    const unsigned cu = (unsigned)engine().num_cu;
    const double *r = grad; // select: every non-empty row is live with r = g, and empty rows are in no column
    DevBuf<double> scratch;
    if (METHOD != XR_SELECT && T > 0) {
        scratch.alloc((size_t)K * (size_t)T);
        r = scratch.get();
        const int32_t *row_order = row_order_of(csr);
        XR_LAUNCH("adjoint_rows", (k_adj_rows<METHOD, SRC>), dim3(div_up(T, AP_BLOCK), ytiles), dim3(AP_BLOCK), 0,
                  csr->indptr.get(), csr->indices.get(), csr->data.get(), row_order, csr->longs.any, T, S, src_stored, grad, K,
                  scratch.get());
        if (csr->longs.any) {
            XR_LAUNCH("adjoint_rows_wave", (k_adj_rows_wave<METHOD, SRC>), dim3(cu * 16 / ylong, ylong), dim3(AP_BLOCK), 0,
                      csr->indptr.get(), csr->indices.get(), csr->data.get(), row_order, csr->longs.rows.get(),
                      csr->longs.n_dev.get(), T, S, src_stored, grad, K, scratch.get());
            if (!(csr->longs.max_row_len >= 0 && csr->longs.max_row_len <= APPLY_WAVE))
                XR_LAUNCH("adjoint_rows_block", (k_adj_rows_block<METHOD, SRC>), dim3(cu * 8 / ylong, ylong), dim3(AP_BLOCK), 0,
                          csr->indptr.get(), csr->indices.get(), csr->data.get(), row_order, csr->longs.rows.get(),
                          csr->longs.n_dev.get(), T, S, src_stored, grad, K, scratch.get());
        }
    }
    const bool has_long = csr->tr.n_long > 0;
    XR_LAUNCH("adjoint_cols", (k_adj_cols<METHOD, SRC>), dim3(div_up(S, AP_BLOCK), ytiles), dim3(AP_BLOCK), 0,
              csr->tr.indptr.get(), csr->tr.row.get(), csr->tr.w.get(), has_long, T, S, src, r, K, out);
    if (has_long) {
        const int n_long = (int)csr->tr.n_long;
        const bool any_huge = csr->tr.max_len > APPLY_WAVE;
        const unsigned gx = (unsigned)std::min<int64_t>(div_up(n_long, AP_BLOCK / 64), cu * 16 / ylong);
        XR_LAUNCH("adjoint_cols_wave", (k_adj_cols_wave<METHOD, SRC>), dim3(gx, ylong), dim3(AP_BLOCK), 0, csr->tr.indptr.get(),
                  csr->tr.row.get(), csr->tr.w.get(), csr->tr.long_cols.get(), n_long, any_huge, T, S, src, r, K, out);
        if (any_huge)
            XR_LAUNCH("adjoint_cols_block", (k_adj_cols_block<METHOD, SRC>),
                      dim3((unsigned)std::min<int64_t>(n_long, cu * 8 / ylong), ylong), dim3(AP_BLOCK), 0, csr->tr.indptr.get(),
                      csr->tr.row.get(), csr->tr.w.get(), csr->tr.long_cols.get(), n_long, T, S, src, r, K, out);
    }
}

void csr_adjoint_dev(const xr_csr *csr, int method, const void *src_dev, int dtype, const double *grad_dev, int64_t K,
                     double *out_dev) {
    with_adjoint_reducer(method, [](auto) {}); // (the reducer is checked whatever the sizes are)
    XR_REQUIRE(!(csr->cols.permuted && csr->cols.source_permuted), XR_ERR_INVALID,
               "the adjoint apply takes and returns source blocks in the caller's column order: call "
               "xr_csr_expect_permuted(csr, 0) first");
    XR_REQUIRE(csr->tr.ready && csr->tr.output_stored == csr->stored.output_stored, XR_ERR_INVALID,
               "internal: adjoint apply without transposed weights");
    if (K == 0 || csr->m == 0) return;
    with_source_type(src_dev ? dtype : XR_F64, [&](auto tag) {
        using SRC = decltype(tag);
        const SRC *src = static_cast<const SRC *>(src_dev);
        DevBuf<char> permuted; // (the row pass walks the stored matrix: stored column ids)
        const SRC *src_stored = src ? stored_source(csr, src, K, permuted) : nullptr;
        with_adjoint_reducer(method, [&](auto m) {
            constexpr int METHOD = decltype(m)::value;
            launch_adjoint<METHOD, SRC>(csr, src, src_stored, grad_dev, K, out_dev);
        });
    });
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_csr_transpose(const xr_csr *csr, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(csr && out, XR_ERR_INVALID, "xr_csr_transpose: NULL argument");
    ensure_transposed(csr);
    Building<xr_csr> t;
    t->n = csr->m; t->m = csr->n; t->nnz = csr->nnz;
    t->indptr.alloc((size_t)t->n + 1);
    t->indices.alloc((size_t)t->nnz);
    t->data.alloc((size_t)t->nnz);
    hipStream_t st = launch_stream();
    XR_HIP(hipMemcpyAsync(t->indptr.get(), csr->tr.indptr.get(), sizeof(int32_t) * ((size_t)t->n + 1), hipMemcpyDeviceToDevice, st));
    if (t->nnz > 0) {
        XR_HIP(hipMemcpyAsync(t->data.get(), csr->tr.w.get(), sizeof(double) * (size_t)t->nnz, hipMemcpyDeviceToDevice, st));
        XR_LAUNCH("tr_row_ids", k_tr_row_ids, dim3(div_up(t->nnz, 256)), dim3(256), 0, csr->tr.row.get(), t->nnz, t->indices.get());
    }
    t->longs.any = csr->tr.n_long > 0;
    if (t->longs.any) {
        const int32_t count = (int32_t)csr->tr.n_long;
        t->longs.rows.alloc((size_t)count);
        t->longs.n_dev.alloc(1);
        XR_HIP(hipMemcpyAsync(t->longs.rows.get(), csr->tr.long_cols.get(), sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToDevice, st));
        h2d(t->longs.n_dev.get(), &count, sizeof(int32_t));
    }
    t->longs.max_row_len = csr->tr.max_len;
    stream_sync();
    *out = t.release();
    XR_API_END
}

int xr_csr_drop_transpose(xr_csr *csr) {
    XR_API_BEGIN
    XR_REQUIRE(csr, XR_ERR_INVALID, "xr_csr_drop_transpose: NULL argument");
    if (csr->tr.indptr.get()) { // (also a structure the row tiling has invalidated)
        release_point();
        csr->tr.release();
    }
    XR_API_END
}

int xr_apply_csr_adjoint_dev(const xr_csr *csr, int method, const void *source_dev, int source_dtype, const double *grad_dev,
                             int64_t K, double *out_dev) {
    {
        const int rc = prepare_for_adjoint(csr, method);
        if (rc != XR_OK) return rc;
    }
    XR_API_BEGIN_SHARED
    XR_REQUIRE(csr && K >= 0 && (grad_dev || csr->n == 0 || K == 0) && (out_dev || csr->m == 0 || K == 0), XR_ERR_INVALID,
               "xr_apply_csr_adjoint_dev: invalid argument");
    csr_adjoint_dev(csr, method, source_dev, source_dtype, grad_dev, K, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_apply_csr_adjoint(const xr_csr *csr, int method, const void *source, int source_dtype, const double *grad, int64_t K,
                         double *out) {
    {
        const int rc = prepare_for_adjoint(csr, method);
        if (rc != XR_OK) return rc;
    }
    XR_API_BEGIN_SHARED
    XR_REQUIRE(csr && K >= 0 && (grad || csr->n == 0 || K == 0) && (out || csr->m == 0 || K == 0), XR_ERR_INVALID,
               "xr_apply_csr_adjoint: invalid argument");
    with_adjoint_reducer(method, [](auto) {});
    const size_t esz = source ? source_size(source_dtype) : 0;
    const int64_t T = csr->n, S = csr->m;
    // per variable: the source block in, the gradient in (staged behind the result block), the result out
    staged_chunks(K, source ? S : 0, esz, S + T, [&](int64_t k0, int64_t kc, char *src, double *dst) {
        double *g = dst + (size_t)kc * (size_t)S;
        if (source && S > 0) h2d_big(src, static_cast<const char *>(source) + (size_t)k0 * (size_t)S * esz, (size_t)kc * (size_t)S * esz);
        if (T > 0) h2d_big(g, grad + (size_t)k0 * (size_t)T, (size_t)kc * (size_t)T * sizeof(double));
        csr_adjoint_dev(csr, method, source ? src : nullptr, source_dtype, g, kc, dst);
        if (S > 0) d2h_big(out + (size_t)k0 * (size_t)S, dst, (size_t)kc * (size_t)S * sizeof(double));
    });
    XR_API_END
}

} // extern "C"
