// xr_apply_workspace.hip -- the workspace reducers of the sparse apply: mode and percentile (reduce.py:126-203), which need a
// row's values side by side.  One thread per (row, k); per-row scratch lives in a global workspace laid out like the CSR
// data (ws[k_local][nnz]).  Rows of APPLY_LONG + 1 ... APPLY_WAVE entries are sorted in LDS by one wave each instead.
#include "xr_apply.h"
#include "xr_reduce.h"
#include "xr_prims.h"

namespace xr {

__device__ __forceinline__ bool nan_le(double a, double b) { // nanpercentile.py:19-27
    if (a != a) return false;
    if (b != b) return true;
    return a < b;
}
__device__ __forceinline__ void dswap(double *A, int i, int j) {
    const double t = A[i];
    A[i] = A[j];
    A[j] = t;
}
__device__ int q_partition(double *A, int low, int high) { // nanpercentile.py:30-63
    const int mid = (low + high) >> 1;
    if (nan_le(A[mid], A[low])) dswap(A, low, mid);
    if (nan_le(A[high], A[mid])) dswap(A, high, mid);
    if (nan_le(A[mid], A[low])) dswap(A, low, mid);
    const double pivot = A[mid];
    dswap(A, high, mid);
    int i = low, j = high - 1;
    for (;;) {
        while (i < high && nan_le(A[i], pivot)) i++;
        while (j >= low && nan_le(pivot, A[j])) j--;
        if (i >= j) break;
        dswap(A, i, j);
        i++;
        j--;
    }
    dswap(A, i, high);
    return i;
}
__device__ double q_select(double *A, int k, int low, int high) { // nanpercentile.py:66-77
    int i = q_partition(A, low, high);
    while (i != k) {
        if (i < k) {
            low = i + 1;
            i = q_partition(A, low, high);
        } else {
            high = i - 1;
            i = q_partition(A, low, high);
        }
    }
    return A[k];
}
__device__ void q_select_two(double *A, int k, int low, int high, double &lo, double &hi) { // :80-102
    for (;;) {
        const int i = q_partition(A, low, high);
        if (i < k) {
            low = i + 1;
        } else if (i > k + 1) {
            high = i - 1;
        } else if (i == k) {
            q_select(A, k + 1, i + 1, high);
            break;
        } else {
            q_select(A, k, low, i - 1);
            break;
        }
    }
    lo = A[k];
    hi = A[k + 1];
}

template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_workspace(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                  const double *__restrict__ data, const int32_t *__restrict__ row_order, int64_t T, int64_t S,
                  int64_t nnz,
                  const SRC *__restrict__ source, int64_t k_base, double p, double *__restrict__ ws,
                  double *__restrict__ out, bool skip_sorted) {
    const int64_t t = (int64_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int64_t k = k_base + blockIdx.y;
    const int s = indptr[t], e = indptr[t + 1], n = e - s;
    if (skip_sorted && n > APPLY_LONG && n <= APPLY_WAVE) return; // k_apply_sorted
    double res = NAN;
    if (n > 0) {
        const SRC *src = source + k * S;
        double *w_row = ws + (int64_t)blockIdx.y * nnz + s;
        if (METHOD == XR_MODE) { // reduce.py:126-158
            for (int i = 0; i < n; i++) w_row[i] = data[s + i];
            int w_sum = 0;
            double w_max = 0.0;
            for (int i = 0; i < n; i++) {
                const double v = ld_src(src, indices[s + i]);
                if (v != v) continue;
                const double w = data[s + i];
                if (w > w_max) w_max = w;
                w_sum += 1;
                for (int j = 0; j < i; j++) {
                    if (ld_src(src, indices[s + j]) == v) {
                        w_row[j] += w;
                        break;
                    }
                }
            }
            if (!(w_sum == 0 || w_max == 0.0)) {
                w_max = 0;
                double mode_value = ld_src(src, indices[s]);
                for (int i = 0; i < n; i++) {
                    const double v = ld_src(src, indices[s + i]);
                    if (v == v) {
                        const double wa = w_row[i];
                        if ((wa > w_max) || (wa == w_max && v > mode_value)) {
                            w_max = wa;
                            mode_value = v;
                        }
                    }
                }
                res = mode_value;
            }
        } else { // percentile, reduce.py:161-203
            double w_max = 0.0;
            for (int i = 0; i < n; i++) {
                const double w = data[s + i];
                if (w > w_max) w_max = w;
            }
            if (w_max != 0.0) {
                if (p == 0 || p == 100) {
                    double v_ext = p == 0 ? INFINITY : -INFINITY, wm = 0.0;
                    for (int i = 0; i < n; i++) {
                        const double v = ld_src(src, indices[s + i]);
                        if (v != v) continue;
                        if (p == 0 ? (v < v_ext) : (v > v_ext)) v_ext = v;
                        const double w = data[s + i];
                        if (w > wm) wm = w;
                    }
                    res = wm == 0.0 ? NAN : v_ext;
                } else {
                    int m = 0;
                    for (int i = 0; i < n; i++) {
                        const double v = ld_src(src, indices[s + i]);
                        if (v == v) w_row[m++] = v;
                    }
                    if (m == 1) {
                        res = w_row[0];
                    } else if (m > 1) {
                        const double rank = 1 + (double)(m - 1) * p / 100.0;
                        const double f = floor(rank);
                        const double frac = rank - f;
                        double lower, upper;
                        q_select_two(w_row, (int)(f - 1), 0, m - 1, lower, upper);
                        res = lower * (1 - frac) + upper * frac;
                    }
                }
            }
        }
    }
    out[k * T + (row_order ? (int64_t)row_order[t] : t)] = res;
}

// mode / percentile of rows with APPLY_LONG < entries <= APPLY_WAVE: one WAVE per (row, variable).  The row's
// values are sorted in LDS (bitonic network on (value, entry index) pairs -- a total order, i.e. a stable sort)
// instead of the reference's per-row O(n^2) linear search (mode) / serial quickselect (percentile):
//   percentile  order statistics do not depend on how they are found: sorted[k], sorted[k + 1], same
//               interpolation as reduce.py:196-203 -> identical values
//   mode        equal values become contiguous in entry order, so the weight of a distinct value is summed
//               left to right exactly as the reference accumulates it onto the first occurrence
//               (reduce.py:134-142); the winner is the largest (total weight, value) pair (:150-157)
static constexpr int SORT_MAX = XR_APPLY_WAVE_ROW; // 2048

template <int METHOD, typename SRC>
__global__ void __launch_bounds__(64)
k_apply_sorted(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
               const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
               const int32_t *__restrict__ n_long, int64_t T, int64_t S, const SRC *__restrict__ source, int64_t K,
               double p, double *__restrict__ out) {
    __shared__ double sv[SORT_MAX];   // value (NaN and padding as +inf: sorted to the end)
    __shared__ uint16_t si[SORT_MAX]; // entry index within the row; bit 15 = not a valid value (NaN / padding), so that
                                      // among equal sort keys (+inf) the valid entries come first
    __shared__ double sw[METHOD == XR_MODE ? SORT_MAX : 1]; // weights in entry order (mode)
    const int lane = threadIdx.x;
    const int nl = *n_long;
    for (int li = blockIdx.x; li < nl; li += gridDim.x) {
        const int t = long_rows[li];
        const int s = indptr[t], n = indptr[t + 1] - s;
        if (n > SORT_MAX) continue; // thread-per-row kernel
        const int64_t t_out = row_order ? (int64_t)row_order[t] : t;
        int np2 = 64;
        while (np2 < n) np2 <<= 1;
        for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
            const SRC *src = source + k * S;
            __syncthreads();
            // load: values, validity count, largest weight of a valid (mode) / any (percentile) entry
            int n_valid = 0;
            double w_max = 0.0, v_min = INFINITY, v_max = -INFINITY;
            for (int i = lane; i < np2; i += 64) {
                double v = INFINITY;
                if (i < n) {
                    const double x = ld_src(src, indices[s + i]);
                    const double w = data[s + i];
                    if (METHOD == XR_MODE) sw[i] = w;
                    const bool ok = x == x;
                    if (ok) {
                        v = x;
                        n_valid++;
                        v_min = fmin(v_min, x);
                        v_max = fmax(v_max, x);
                    }
                    if (METHOD != XR_MODE || ok) w_max = fmax(w_max, w);
                }
                sv[i] = v;
                si[i] = (uint16_t)(v == INFINITY && !(i < n && ld_src(src, indices[s + i]) == INFINITY) ? (i | 0x8000) : i);
            }
            n_valid = wave_reduce<OpSum>(n_valid), w_max = wave_reduce<OpMax>(w_max);
            v_min = wave_reduce<OpMin>(v_min), v_max = wave_reduce<OpMax>(v_max);
            double res = NAN;
            if (METHOD == XR_PERCENTILE && (p == 0 || p == 100)) {
                // reduce.py:172-176: _minimum / _maximum (NaN skipped; NaN if every weight of a valid entry is 0)
                double wm = 0.0;
                for (int i = lane; i < n; i += 64)
                    if (!(si[i] & 0x8000)) wm = fmax(wm, data[s + i]);
                wm = wave_reduce<OpMax>(wm);
                if (w_max != 0.0 && n_valid > 0 && wm != 0.0) res = p == 0 ? v_min : v_max;
                if (lane == 0) out[k * T + t_out] = res;
                continue;
            }
            const bool trivial = w_max == 0.0 || n_valid == 0;
            if (!trivial && !(METHOD == XR_PERCENTILE && n_valid == 1)) {
                // bitonic sort of (value, index) ascending
                for (int size = 2; size <= np2; size <<= 1) {
                    for (int stride = size >> 1; stride > 0; stride >>= 1) {
                        __syncthreads();
                        for (int q = lane; q < np2 / 2; q += 64) {
                            const int lo = 2 * q - (q & (stride - 1));
                            const int hi = lo + stride;
                            const bool up = (lo & size) == 0;
                            const double a = sv[lo], b = sv[hi];
                            const uint16_t ia = si[lo], ib = si[hi];
                            const bool a_gt_b = (a > b) || (a == b && ia > ib);
                            if (a_gt_b == up) {
                                sv[lo] = b; sv[hi] = a;
                                si[lo] = ib; si[hi] = ia;
                            }
                        }
                    }
                }
                __syncthreads();
            }
            if (METHOD == XR_PERCENTILE) {
                if (!trivial) {
                    if (n_valid == 1) {
                        res = v_min;
                    } else {
                        // +inf VALUES sort among the padding; their count does not matter: ranks only reach n_valid - 1
                        const double rank = 1 + (double)(n_valid - 1) * p / 100.0;
                        const double f = floor(rank);
                        const double frac = rank - f;
                        const int kk = (int)(f - 1);
                        const double lower = sv[kk], upper = sv[kk + 1];
                        res = lower * (1 - frac) + upper * frac;
                    }
                }
            } else if (!trivial) {
                // group starts sum their group left to right; then the largest (total, value) pair wins
                double best_w = -1.0, best_v = -INFINITY;
                for (int i = lane; i < n_valid; i += 64) {
                    const double v = sv[i];
                    if (i == 0 || sv[i - 1] != v) {
                        double tot = sw[si[i]];
                        for (int j = i + 1; j < n_valid && sv[j] == v; j++) tot += sw[si[j]];
                        if (tot > best_w || (tot == best_w && v > best_v)) {
                            best_w = tot;
                            best_v = v;
                        }
                    }
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const double ow = __shfl_xor(best_w, d, 64), ov = __shfl_xor(best_v, d, 64);
                    if (ow > best_w || (ow == best_w && ov > best_v)) {
                        best_w = ow;
                        best_v = ov;
                    }
                }
                res = best_v;
            }
            if (lane == 0) out[k * T + t_out] = res;
        }
    }
}

template <int METHOD, typename SRC>
static void launch_workspace(const xr_csr *csr, const SRC *src, int64_t K, double p, double *out) {
    // scratch budget: at most ~512 MB of per-(k,row) workspace at a time
    int64_t kchunk = csr->nnz > 0 ? ((int64_t)64 << 20) / csr->nnz : K;
    if (kchunk < 1) kchunk = 1;
    if (kchunk > K) kchunk = K;
    if (kchunk > 65535) kchunk = 65535;
    DevBuf<double> ws((size_t)kchunk * (size_t)(csr->nnz > 0 ? csr->nnz : 1));
    for (int64_t k0 = 0; k0 < K; k0 += kchunk) {
        const int64_t kc = (K - k0) < kchunk ? (K - k0) : kchunk;
        dim3 grid(div_up(csr->n, AP_BLOCK), (unsigned)kc);
        XR_LAUNCH("apply_workspace", (k_apply_workspace<METHOD, SRC>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                  csr->indices.get(), csr->data.get(), row_order_of(csr), csr->n, csr->m, csr->nnz, src, k0, p,
                  ws.get(), out, csr->longs.any);
    }
    if (csr->longs.any) {
        // rows of APPLY_LONG + 1 ... APPLY_WAVE entries: sorted in LDS by one wave per (row, variable)
        const unsigned gy = (unsigned)std::min<int64_t>(K, 16);
        dim3 grid((unsigned)engine().num_cu * 32 / gy, gy);
        XR_LAUNCH("apply_sorted", (k_apply_sorted<METHOD, SRC>), grid, dim3(64), 0, csr->indptr.get(), csr->indices.get(),
                  csr->data.get(), row_order_of(csr), csr->longs.rows.get(), csr->longs.n_dev.get(), csr->n, csr->m, src, K, p,
                  out);
    }
}

void apply_workspace(const xr_csr *csr, int method, double p, const void *src, int dtype, int64_t K, double *out) {
    with_reducer(method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        XR_REQUIRE(!streamed_reducer<METHOD>, XR_ERR_INVALID, "internal: reducer %d needs no workspace", METHOD);
        if constexpr (!streamed_reducer<METHOD>)
            with_source_type(dtype, [&](auto tag) {
                using SRC = decltype(tag);
                launch_workspace<METHOD, SRC>(csr, static_cast<const SRC *>(src), K, p, out);
            });
    });
}

} // namespace xr
