// xr_partial.hip -- the partial states of the source-sharded apply (multi-GPU split over the source faces): every shard
// reduces its columns of a row to the state of a shard-decomposable reducer (PartialState, xr_reduce.h; component table in
// include/xugrid_amd.h), the states of a row are combined across the shards and finalised.
#include "xr_apply.h"
#include "xr_reduce.h"
#include "xr_prims.h"

namespace xr {

// ---- the pieces the kernels below share ----------------------------------------------------------------------------

// component c of the state of (row t_out, variable k) into a state table of either layout: rows (T, C * K) or planes (C, K, T)
__device__ __forceinline__ void partial_store(double *__restrict__ out, bool rows_layout, int64_t T, int C, int64_t K,
                                              int64_t t_out, int64_t k, int c, double v) {
    out[rows_layout ? t_out * (C * K) + c * K + k : ((int64_t)c * K + k) * T + t_out] = v;
}
// ... the whole state.  (The loop unrolls to static indices where C is a compile-time constant.  In the kernels with a run-time
// reducer it indexes the state at run time, for which the compiler keeps the state in LDS -- 8 KB per block of 256; guarding four
// static indices instead frees the LDS for five more scalar registers in k_apply_partial_long.)
__device__ __forceinline__ void partial_store(double *__restrict__ out, bool rows_layout, int64_t T, int C, int64_t K,
                                              int64_t t_out, int64_t k, const PartialState &st) {
    for (int c = 0; c < C; c++) partial_store(out, rows_layout, T, C, K, t_out, k, c, st.c[c]);
}

// the partial state of stored row t by one WAVE (a listed long row: hull slivers of thousands of entries): the lanes stride the
// row in CSR order, then a butterfly combines their states component by component in a fixed order; every lane returns the
// row's state.  (`method` a compile-time constant: the switches fold to the reducer's own lines.)
template <typename SRC>
__device__ __forceinline__ PartialState partial_row_by_wave(int method, const int32_t *__restrict__ indptr,
                                                            const int32_t *__restrict__ indices, const double *__restrict__ data,
                                                            const SRC *__restrict__ src, int t) {
    const int lane = threadIdx.x & 63;
    PartialState st = partial_identity(method);
    for (int j = indptr[t] + lane; j < indptr[t + 1]; j += 64) partial_add(method, st, ld_src(src, indices[j]), data[j]);
    const int C = partial_components(method);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c < C) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double o = __shfl_xor(st.c[c], d, 64);
                st.c[c] = partial_is_max(method) ? fmax(st.c[c], o) : st.c[c] + o;
            }
        }
    }
    return st;
}

// one thread per (stored row, variable)
template <typename SRC>
__global__ void __launch_bounds__(256)
k_apply_partial(int method, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                const double *__restrict__ data, const int32_t *__restrict__ row_order, int64_t T, int64_t S,
                const SRC *__restrict__ source, int64_t K, double *__restrict__ out, bool rows_layout, bool skip_long) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = blockIdx.y;
    if (t >= T) return;
    if (skip_long && indptr[t + 1] - indptr[t] > APPLY_LONG) return; // reduced by one wave each (k_apply_partial_long)
    PartialState st = partial_identity(method);
    const SRC *src = source + k * S;
    for (int j = indptr[t]; j < indptr[t + 1]; j++) partial_add(method, st, ld_src(src, indices[j]), data[j]);
    partial_store(out, rows_layout, T, partial_components(method), K, row_order ? (int64_t)row_order[t] : t, k, st);
}

// K = 1, one specialisation per decomposable reducer (round 5): the partial state of 64 stored rows per WAVE through the wave's
// private LDS window, exactly as k_apply_rows1 reduces them -- the CSR segment of the 64 rows is contiguous: column and weight
// loaded coalesced, the source value gathered by the same lane and parked next to the weight, then every lane walks ITS row in
// CSR order (the same additions in the same order as k_apply_partial's thread-per-row loop, so the states are bit-identical).
// With the reducer a run-time switch this form was slower than the plain kernel (73 against 61 us, round 4: four state
// components and a switch per entry in the walk); as a template the walk of `mean` is two selects per entry.
// Rows beyond APPLY_LONG entries are left to k_apply_partial_long.
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_partial_w1(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
                   const int32_t *__restrict__ row_order, int64_t T, int64_t S, const SRC *__restrict__ source,
                   double *__restrict__ out, bool rows_layout, bool skip_long, const int32_t *__restrict__ gate,
                   const int32_t *__restrict__ long_rows, const int32_t *__restrict__ n_long, int n_long_blocks) {
    __shared__ double2 sh_win[AP_BLOCK / 64][W1_CAP]; // (.x = weight, .y = source value)
    if (gate && *gate == 0) return; // (enqueued behind a weight build whose attempt failed: the host redoes both)
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    constexpr int C = partial_components(METHOD);
    if ((int)blockIdx.x < n_long_blocks) {
        // the listed long rows (hull slivers), one WAVE each, in the blocks dispatched first: beside the short rows instead of
        // in a launch of their own behind them (as k_apply_rows1; the same walk as k_apply_partial_long: partial_row_by_wave)
        const int nl = *n_long;
        for (int64_t li = (int64_t)blockIdx.x * (AP_BLOCK / 64) + wib; li < nl; li += (int64_t)n_long_blocks * (AP_BLOCK / 64)) {
            const int t = long_rows[li];
            const PartialState st = partial_row_by_wave(METHOD, indptr, indices, data, source, t);
            if (lane == 0) partial_store(out, rows_layout, T, C, 1, row_order ? (int64_t)row_order[t] : t, 0, st);
        }
        return;
    }
    const int64_t row0 = ((int64_t)(gridDim.x - 1 - blockIdx.x) * (AP_BLOCK / 64) + wib) * 64;
    if (row0 >= T) return;
    const int64_t t = row0 + lane;
    int s = 0, e = 0;
    if (t < T) {
        s = indptr[t];
        e = indptr[t + 1];
    }
    const bool skip = skip_long && (e - s > APPLY_LONG);
    const int seg0 = __shfl(s, 0, 64);
    const int seg1 = wave_reduce<OpMax>(e);
    if (skip) e = s;
    const bool jumpy = __any(skip);
    double2 *win = sh_win[wib];
    auto next_chunk = [&](int c0) -> int { // first entry any lane still needs at or behind c0 (skipped long rows are not streamed)
        if (!jumpy) return c0;
        int mine = (e > s && e > c0) ? (s > c0 ? s : c0) : INT_MAX;
        return wave_reduce<OpMin>(mine);
    };
    PartialState st = partial_identity(METHOD);
    for (int c0 = seg0; c0 < seg1; c0 += W1_CAP) {
        c0 = next_chunk(c0);
        if (c0 >= seg1) break;
        {
            constexpr int PER = W1_CAP / 64;
            int col[PER];
            double w[PER];
#pragma unroll
            for (int u = 0; u < PER; u++) {
                const int j = c0 + u * 64 + lane;
                col[u] = j < seg1 ? indices[j] : -1;
                w[u] = j < seg1 ? data[j] : 0.0;
            }
            double v[PER];
#pragma unroll
            for (int u = 0; u < PER; u++) v[u] = col[u] >= 0 ? ld_src(source, (int64_t)col[u]) : 0.0;
#pragma unroll
            for (int u = 0; u < PER; u++)
                if (col[u] >= 0) win[u * 64 + lane] = make_double2(w[u], v[u]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int a = s > c0 ? s : c0, b = e < c0 + W1_CAP ? e : c0 + W1_CAP;
        for (int j = a; j < b; j++) {
            const double2 wv = win[j - c0];
            partial_add(METHOD, st, wv.y, wv.x); // (METHOD is a constant: the switch folds to the reducer's own lines)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (the window is overwritten by the next chunk)
        __builtin_amdgcn_wave_barrier();
    }
    if (t < T && !skip) partial_store(out, rows_layout, T, C, 1, row_order ? (int64_t)row_order[t] : t, 0, st);
}

// KT variables per thread (K >= KT): the row's entries are read once per tile instead of once per variable, the KT
// gathers of an entry are independent loads in flight, and in the rows layout a thread writes KT consecutive doubles per
// component (whole 64-byte lines) where the one-variable kernel scatters single doubles C * K apart.  Same additions in
// the same order per variable.  (One rank, 1M x 1M matrix, 32 variables per call: see DESIGN section 6.)
// (The walk over the row is written out here and in k_apply_partial_rows: as one inline function taking the KT states by
// reference -- per row or per entry -- both kernels compile to 184 instead of 119 vector registers, two waves per SIMD
// instead of four.)
template <typename SRC, int KT>
__global__ void __launch_bounds__(256)
k_apply_partial_kt(int method, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                   const double *__restrict__ data, const int32_t *__restrict__ row_order, int64_t T, int64_t S,
                   const SRC *__restrict__ source, int64_t K, double *__restrict__ out, bool rows_layout, bool skip_long) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.y * KT;
    if (t >= T) return;
    const int s = indptr[t], e = indptr[t + 1];
    if (skip_long && e - s > APPLY_LONG) return; // reduced by one wave each (k_apply_partial_long)
    const int kn = (int)((K - k0) < KT ? (K - k0) : KT);
    PartialState st[KT];
#pragma unroll
    for (int kk = 0; kk < KT; kk++) st[kk] = partial_identity(method);
    const SRC *src = source + k0 * S;
    for (int j = s; j < e; j++) {
        const int64_t col = indices[j];
        const double w = data[j];
        double v[KT];
#pragma unroll
        for (int kk = 0; kk < KT; kk++) v[kk] = kk < kn ? ld_src(src, (int64_t)kk * S + col) : 0.0;
#pragma unroll
        for (int kk = 0; kk < KT; kk++)
            if (kk < kn) partial_add(method, st[kk], v[kk], w);
    }
    const int C = partial_components(method);
    const int64_t t_out = row_order ? (int64_t)row_order[t] : t;
#pragma unroll
    for (int c = 0; c < 4; c++) { // (static indices into the states: see partial_combine)
        if (c >= C) break;
#pragma unroll
        for (int kk = 0; kk < KT; kk++) {
            if (kk < kn) partial_store(out, rows_layout, T, C, K, t_out, k0 + kk, c, st[kk].c[c]);
        }
    }
}
// The same for the ROWS layout (T, C * K) of the sparse exchange.  There a row's states lie C * K doubles apart from the
// next row's: a thread that stores its own doubles makes every store instruction of the wave touch 64 different lines, 8
// bytes each (measured: 2.2 ms for 32 variables x 1M rows, one rank -- 7 x what the bytes cost).  The block therefore
// parks its 128 rows x C x KT states in LDS and writes them out with 8 lanes per (row, component): whole 64-byte lines.
template <typename SRC, int KT>
__global__ void __launch_bounds__(128)
k_apply_partial_rows(int method, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                     const double *__restrict__ data, const int32_t *__restrict__ row_order, int64_t T, int64_t S,
                     const SRC *__restrict__ source, int64_t K, double *__restrict__ out, bool skip_long) {
    static_assert(KT == 8, "one 64-byte line per (row, component)");
    extern __shared__ double sh_dyn[]; // [128][C * KT + 1] states (sized for the reducer's C: 17 KB for two components)
    __shared__ int32_t sh_tout[128];
    const int64_t t = (int64_t)blockIdx.x * 128 + threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.y * KT;
    const int kn = (int)((K - k0) < KT ? (K - k0) : KT);
    const int C = partial_components(method);
    const int ld = C * KT + 1;
    int s = 0, e = 0;
    bool mine = false;
    if (t < T) {
        s = indptr[t];
        e = indptr[t + 1];
        mine = !(skip_long && e - s > APPLY_LONG); // (long rows: one wave each, k_apply_partial_long)
    }
    PartialState st[KT];
#pragma unroll
    for (int kk = 0; kk < KT; kk++) st[kk] = partial_identity(method);
    const SRC *src = source + k0 * S;
    if (mine) {
        for (int j = s; j < e; j++) {
            const int64_t col = indices[j];
            const double w = data[j];
            double v[KT];
#pragma unroll
            for (int kk = 0; kk < KT; kk++) v[kk] = kk < kn ? ld_src(src, (int64_t)kk * S + col) : 0.0;
#pragma unroll
            for (int kk = 0; kk < KT; kk++)
                if (kk < kn) partial_add(method, st[kk], v[kk], w);
        }
    }
    sh_tout[threadIdx.x] = mine ? (int32_t)(row_order ? row_order[t] : t) : -1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= C) break;
#pragma unroll
        for (int kk = 0; kk < KT; kk++) sh_dyn[threadIdx.x * ld + c * KT + kk] = st[kk].c[c];
    }
    __syncthreads();
    // 8 lanes per (row, component) line
    const int n_lines = 128 * C;
    for (int line = threadIdx.x >> 3; line < n_lines; line += 16) {
        const int r = line / C, c = line - r * C, kk = threadIdx.x & 7;
        const int t_out = sh_tout[r];
        if (t_out >= 0 && kk < kn) out[(int64_t)t_out * (C * K) + (int64_t)c * K + k0 + kk] = sh_dyn[r * ld + c * KT + kk];
    }
}

// Combination + finalisation of the received rows (sparse exchange), coalesced both ways: a block takes 64 owned targets
// x a chunk of 32 variables; a thread reads the states of ITS (target, variable) with the variable running fastest across
// the lanes -- 256-byte runs of the (R, C * K) rows -- and the finalised values cross LDS so that the (K, n_targets)
// output is written with the target running fastest.  (One thread per output element read one double per 64-byte line
// and line 8 times over: 1.4 ms for 32 variables x 1M targets.)
__global__ void __launch_bounds__(256)
k_reduce_partial_rows_t(int method, const double *__restrict__ rows, const int64_t *__restrict__ indptr,
                        const int64_t *__restrict__ order, int64_t n_targets, int64_t K, double *__restrict__ out) {
    constexpr int TT = 64, KC = 32;
    __shared__ double sh_val[KC][TT + 1];
    const int C = partial_components(method);
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    for (int64_t kc0 = (int64_t)blockIdx.y * KC; kc0 < K; kc0 += (int64_t)gridDim.y * KC) {
        const int kk = threadIdx.x & (KC - 1);
        const int64_t k = kc0 + kk;
        for (int tl = threadIdx.x / KC; tl < TT; tl += 256 / KC) {
            const int64_t t = t0 + tl;
            double v = NAN;
            if (t < n_targets && k < K) {
                PartialState st = partial_identity(method);
                for (int64_t j = indptr[t]; j < indptr[t + 1]; j++) partial_combine(method, st, rows + order[j] * (C * K) + k, K, C);
                v = partial_finalize(method, st);
            }
            sh_val[kk][tl] = v;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < KC * TT; q += 256) {
            const int kq = q / TT, tl = q - kq * TT;
            if (t0 + tl < n_targets && kc0 + kq < K) out[(kc0 + kq) * n_targets + t0 + tl] = sh_val[kq][tl];
        }
        __syncthreads();
    }
}

// the listed long rows (hull slivers: thousands of entries): one wave per (row, variable), partial_row_by_wave
template <typename SRC>
__global__ void __launch_bounds__(256)
k_apply_partial_long(int method, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                     const double *__restrict__ data, const int32_t *__restrict__ row_order,
                     const int32_t *__restrict__ long_rows, const int32_t *__restrict__ n_long, int64_t T, int64_t S,
                     const SRC *__restrict__ source, int64_t K, double *__restrict__ out, bool rows_layout,
                     const int32_t *__restrict__ gate = nullptr) {
    if (gate && *gate == 0) return; // (see k_apply_partial_w1)
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
    const int64_t k = blockIdx.y;
    const int nl = *n_long;
    for (int64_t li = wave; li < nl; li += n_waves) {
        const int t = long_rows[li];
        const PartialState st = partial_row_by_wave(method, indptr, indices, data, source + k * S, t);
        if (lane == 0) partial_store(out, rows_layout, T, partial_components(method), K, row_order ? (int64_t)row_order[t] : t, k, st);
    }
}

__global__ void k_partial_identity(int method, double *__restrict__ planes, int64_t per_component) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C = partial_components(method);
    if (i >= per_component * C) return;
    const PartialState st = partial_identity(method);
    planes[i] = st.c[i / per_component];
}

__global__ void k_finalize_partial(int method, const double *__restrict__ planes, int64_t n /* K * T */,
                                   double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    PartialState st;
    const int C = partial_components(method);
    for (int c = 0; c < C; c++) st.c[c] = planes[(int64_t)c * n + i];
    out[i] = partial_finalize(method, st);
}

__global__ void k_reduce_partial_rows(int method, const double *__restrict__ rows, const int64_t *__restrict__ indptr,
                                      const int64_t *__restrict__ order, int64_t n_targets, int64_t K,
                                      double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_targets * K) return;
    const int64_t k = i / n_targets, t = i - k * n_targets;
    const int C = partial_components(method);
    PartialState st = partial_identity(method);
    for (int64_t j = indptr[t]; j < indptr[t + 1]; j++) partial_combine(method, st, rows + order[j] * (C * K) + k, K, C);
    out[i] = partial_finalize(method, st);
}

// One variable: a thread per owned target, one specialisation per reducer (the components are compile-time registers, a row of
// the (R, C) state table is one or two 16-byte loads) -- the run-time form above indexes the state by a loop over C and took
// 40 us for 1M targets of one row each, 2.5 x what its 40 MB need.
template <int METHOD>
__global__ void __launch_bounds__(256)
k_reduce_partial_rows_k1(const double *__restrict__ rows, const int64_t *__restrict__ indptr, const int64_t *__restrict__ order,
                         int64_t n_targets, double *__restrict__ out) {
    constexpr int C = partial_components(METHOD);
    constexpr bool IS_MAX = partial_is_max(METHOD);
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_targets) return;
    const int64_t j0 = indptr[t], j1 = indptr[t + 1];
    PartialState st = partial_identity(METHOD);
    for (int64_t j = j0; j < j1; j++) {
        const double2 *row = reinterpret_cast<const double2 *>(rows + order[j] * C);
        const double2 a = row[0];
        if (IS_MAX) {
            st.c[0] = fmax(st.c[0], a.x);
            st.c[1] = fmax(st.c[1], a.y);
        } else {
            st.c[0] += a.x;
            st.c[1] += a.y;
        }
        if (C == 4) {
            const double2 b = row[1];
            st.c[2] += b.x;
            st.c[3] += b.y;
        }
    }
    out[t] = partial_finalize(METHOD, st);
}

} // namespace xr

using namespace xr;

// the partial state of every stored row (xr_apply_partial_dev; also enqueued right behind a weight build by
// xr_overlap_partial_dev, then gated like the early apply: ctx)
void xr::csr_partial_dev(const xr_csr *csr, int method, const void *source_dev, int source_dtype, int64_t K, double *out_dev,
                         int rows_layout, const ApplyContext *ctx) {
    const bool has_long = ctx ? ctx->has_long : csr->longs.any;
    XR_REQUIRE(partial_components(method) > 0, XR_ERR_INVALID, "reducer %d does not decompose over source shards", method);
    with_source_type(source_dtype, [&](auto tag) {
        using SRC = decltype(tag);
        XR_REQUIRE(K >= 0 && K < 65536, XR_ERR_LIMIT, "xr_apply_partial_dev: K out of range (tile the variables)");
        const int32_t *gate = ctx ? ctx->gate : (const int32_t *)nullptr;
        XR_REQUIRE(!gate || K == 1, XR_ERR_INVALID, "internal: a gated partial apply is one variable");
        if (csr->n == 0 || K == 0) return;
        XR_REQUIRE(source_dev || csr->m == 0, XR_ERR_INVALID, "xr_apply_partial_dev: NULL source");
        DevBuf<char> permuted;
        const SRC *src = stored_source(csr, static_cast<const SRC *>(source_dev), K, permuted);
        constexpr int PKT = 8;
        bool long_done = false; // (the long rows went with the short ones)
        if (K >= PKT && rows_layout != 0) {
            dim3 grid(div_up(csr->n, 128), (unsigned)div_up(K, PKT));
            const size_t rows_shmem = sizeof(double) * 128 * (size_t)(partial_components(method) * PKT + 1);
            XR_LAUNCH("apply_partial", (k_apply_partial_rows<SRC, PKT>), grid, dim3(128), rows_shmem, method, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->n, csr->m, src, K, out_dev, has_long);
        } else if (K >= PKT) {
            dim3 grid(div_up(csr->n, 256), (unsigned)div_up(K, PKT));
            XR_LAUNCH("apply_partial", (k_apply_partial_kt<SRC, PKT>), grid, dim3(256), 0, method, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->n, csr->m, src, K, out_dev,
                      rows_layout != 0, has_long);
        } else if (K == 1) {
            // one variable: the wave-window kernel, one specialisation per reducer; the long rows in its first blocks
            const int n_long_blocks = has_long ? engine().num_cu / 2 : 0;
            dim3 grid((unsigned)(div_up(csr->n, AP_BLOCK) + n_long_blocks));
            long_done = true;
            with_decomposable(method, [&](auto m) {
                XR_LAUNCH("apply_partial", (k_apply_partial_w1<decltype(m)::value, SRC>), grid, dim3(AP_BLOCK), 0,
                          csr->indptr.get(), csr->indices.get(), csr->data.get(), row_order_of(csr), csr->n, csr->m, src,
                          out_dev, rows_layout != 0, has_long, gate, csr->longs.rows.get(), csr->longs.n_dev.get(),
                          n_long_blocks);
            });
        } else { // K = 2 ... 7: one thread per (stored row, variable)
            dim3 grid(div_up(csr->n, 256), (unsigned)K);
            XR_LAUNCH("apply_partial", k_apply_partial<SRC>, grid, dim3(256), 0, method, csr->indptr.get(), csr->indices.get(),
                      csr->data.get(), row_order_of(csr), csr->n, csr->m, src, K, out_dev, rows_layout != 0, has_long);
        }
        if (has_long && !long_done) {
            dim3 lgrid(64, (unsigned)K);
            XR_LAUNCH("apply_partial_long", k_apply_partial_long<SRC>, lgrid, dim3(256), 0, method, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->longs.rows.get(), csr->longs.n_dev.get(),
                      csr->n, csr->m, src, K, out_dev, rows_layout != 0, gate);
        }
    });
}

extern "C" {

int xr_partial_components(int method) { return partial_components(method); }
int xr_partial_combine_is_max(int method) { return partial_is_max(method) ? 1 : 0; }

int xr_apply_partial_dev(const xr_csr *csr, int method, const void *source_dev, int source_dtype, int64_t K,
                         double *out_dev, int rows_layout) {
    XR_API_BEGIN
    XR_REQUIRE(csr && out_dev, XR_ERR_INVALID, "xr_apply_partial_dev: NULL argument");
    csr_partial_dev(csr, method, source_dev, source_dtype, K, out_dev, rows_layout);
    dev_call_done();
    XR_API_END
}

int xr_partial_fill_identity_dev(int method, double *planes_dev, int64_t K, int64_t T) {
    XR_API_BEGIN
    XR_REQUIRE(partial_components(method) > 0, XR_ERR_INVALID, "reducer %d does not decompose over source shards", method);
    XR_REQUIRE(K >= 0 && T >= 0, XR_ERR_INVALID, "xr_partial_fill_identity_dev: negative size");
    if (K * T > 0) {
        XR_REQUIRE(planes_dev, XR_ERR_INVALID, "xr_partial_fill_identity_dev: NULL argument");
        XR_LAUNCH("partial_identity", k_partial_identity, dim3(div_up(K * T * partial_components(method), 256)), dim3(256), 0,
                  method, planes_dev, K * T);
    }
    dev_call_done();
    XR_API_END
}

int xr_finalize_partial_dev(int method, const double *planes_dev, int64_t K, int64_t T, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(partial_components(method) > 0, XR_ERR_INVALID, "reducer %d does not decompose over source shards", method);
    XR_REQUIRE(K >= 0 && T >= 0, XR_ERR_INVALID, "xr_finalize_partial_dev: negative size");
    if (K * T > 0) {
        XR_REQUIRE(planes_dev && out_dev, XR_ERR_INVALID, "xr_finalize_partial_dev: NULL argument");
        XR_LAUNCH("finalize_partial", k_finalize_partial, dim3(div_up(K * T, 256)), dim3(256), 0, method, planes_dev, K * T,
                  out_dev);
    }
    dev_call_done();
    XR_API_END
}

int xr_reduce_partial_rows_dev(int method, const double *rows_dev, const int64_t *indptr_dev, const int64_t *order_dev,
                               int64_t n_targets, int64_t K, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(partial_components(method) > 0, XR_ERR_INVALID, "reducer %d does not decompose over source shards", method);
    XR_REQUIRE(n_targets >= 0 && K >= 0, XR_ERR_INVALID, "xr_reduce_partial_rows_dev: negative size");
    if (n_targets * K > 0) {
        XR_REQUIRE(indptr_dev && out_dev, XR_ERR_INVALID, "xr_reduce_partial_rows_dev: NULL argument");
        if (K == 1 && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0) {
            with_decomposable(method, [&](auto m) {
                XR_LAUNCH("reduce_partial_rows_k1", k_reduce_partial_rows_k1<decltype(m)::value>, dim3(div_up(n_targets, 256)),
                          dim3(256), 0, rows_dev, indptr_dev, order_dev, n_targets, out_dev);
            });
        } else if (K >= 8)
            XR_LAUNCH("reduce_partial_rows_t", k_reduce_partial_rows_t, dim3(div_up(n_targets, 64), (unsigned)std::min<int64_t>(div_up(K, 32), 64)),
                      dim3(256), 0, method, rows_dev, indptr_dev, order_dev, n_targets, K, out_dev);
        else
            XR_LAUNCH("reduce_partial_rows", k_reduce_partial_rows, dim3(div_up(n_targets * K, 256)), dim3(256), 0, method,
                      rows_dev, indptr_dev, order_dev, n_targets, K, out_dev);
    }
    dev_call_done();
    XR_API_END
}

} // extern "C"
