// xr_apply.hip -- the sparse weight x data apply.
//
// Replaces make_regrid(func)._regrid (xugrid/regrid/regridder.py:41-67) with one kernel
// specialisation per reducer of xugrid/regrid/reduce.py, and CentroidLocatorRegridder._regrid
// (regridder.py:400-409).  The reducers themselves are in xr_reduce.h; the MatrixCSR handle with its row
// tiling is in xr_csr.hip, the partial states of the source-sharded apply in xr_partial.hip, the separable
// weights in xr_outer.hip; what these units share is in xr_apply.h.
//
// Reducer semantics are those of reduce.py line by line; entries of a
// row are consumed in CSR order by one thread per (row, k-tile), so that results are
// bit-identical to the reference loop on the same CSR (except exp/log in geometric_mean).
//
// HBM layout: source (K, S) row-major, out (K, T) row-major (regridder.py:163, :44);
// CSR = indptr i32[T+1], indices i32[nnz], data f64[nnz].
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xr_apply.h"
#include "xr_reduce.h"
#include "xr_prims.h"

namespace xr {

static constexpr int KT = 16; // source variables reduced per pass over the CSR (K >= 2)

// Where the cooperative reducers find a listed row: its segment, the arrays the segment indexes, its output position.
// CsrRows: stored row t of one CSR.
struct CsrRows {
    const int32_t *__restrict__ indptr, *__restrict__ indices;
    const double *__restrict__ data;
    const int32_t *__restrict__ row_order;
    __device__ __forceinline__ void segment(int t, int &s, int &e) const {
        s = indptr[t];
        e = indptr[t + 1];
    }
    __device__ __forceinline__ const int32_t *columns(int) const { return indices; }
    __device__ __forceinline__ const double *weights(int) const { return data; }
    __device__ __forceinline__ int64_t out_row(int t) const { return row_order ? (int64_t)row_order[t] : t; }
};
// TailRows: the matrix of a fused weight build whose big faces' rows have not been copied behind the regular ones yet
// (k_apply_tail1).  Stored rows [t_big, T) are rows 0 ... of the big faces' own CSR, row k the row of face slot_face[k] in
// the query order.
struct TailRows {
    CsrRows reg;
    int t_big;
    const int32_t *__restrict__ big_indptr, *__restrict__ big_indices;
    const double *__restrict__ big_data;
    const int32_t *__restrict__ slot_face, *__restrict__ q_perm;
    __device__ __forceinline__ void segment(int t, int &s, int &e) const {
        const int32_t *ip = t >= t_big ? big_indptr + (t - t_big) : reg.indptr + t;
        s = ip[0];
        e = ip[1];
    }
    __device__ __forceinline__ const int32_t *columns(int t) const { return t >= t_big ? big_indices : reg.indices; }
    __device__ __forceinline__ const double *weights(int t) const { return t >= t_big ? big_data : reg.data; }
    __device__ __forceinline__ int64_t big_out_row(int k) const {
        const int f = slot_face[k];
        return q_perm ? (int64_t)q_perm[f] : f;
    }
    __device__ __forceinline__ int64_t out_row(int t) const { return t >= t_big ? big_out_row(t - t_big) : reg.out_row(t); }
};

// one listed row reduced by the whole block (all threads call; rows beyond APPLY_WAVE entries)
template <int METHOD, typename SRC, typename ROWS>
__device__ __forceinline__ void apply_row_block(const ROWS &rows, int t, int64_t T, int64_t S, const SRC *__restrict__ source,
                                                int64_t K, double *__restrict__ out, double (*lds)[3]) {
    int s, e;
    rows.segment(t, s, e);
    const int32_t *__restrict__ indices = rows.columns(t);
    const double *__restrict__ data = rows.weights(t);
    const int64_t t_out = rows.out_row(t);
    double normsum = 0.0;
    if (METHOD == XR_GEOMETRIC_MEAN) {
        Red<XR_SUM> ws; // b accumulates the weights
        for (int j = s + threadIdx.x; j < e; j += AP_BLOCK) ws.b += data[j];
        block_merge<XR_SUM>(ws, lds);
        normsum = ws.b;
    }
    for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
        const SRC *src = source + k * S;
        Red<METHOD> r;
        int j = s + threadIdx.x;
        // four entries in flight per thread; the additions keep their sequential order
        for (; j + 3 * AP_BLOCK < e; j += 4 * AP_BLOCK) {
            const int c0 = indices[j], c1 = indices[j + AP_BLOCK], c2 = indices[j + 2 * AP_BLOCK],
                      c3 = indices[j + 3 * AP_BLOCK];
            const double w0 = data[j], w1 = data[j + AP_BLOCK], w2 = data[j + 2 * AP_BLOCK],
                         w3 = data[j + 3 * AP_BLOCK];
            const double v0 = ld_src(src, c0), v1 = ld_src(src, c1), v2 = ld_src(src, c2), v3 = ld_src(src, c3);
            r.add(v0, w0, normsum);
            r.add(v1, w1, normsum);
            r.add(v2, w2, normsum);
            r.add(v3, w3, normsum);
        }
        for (; j < e; j += AP_BLOCK) r.add(ld_src(src, indices[j]), data[j], normsum);
        block_merge<METHOD>(r, lds);
        if (threadIdx.x == 0) {
            double v = r.fin();
            if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) v = NAN;
            out[k * T + t_out] = v;
        }
    }
}

template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_long(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
             const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
             const int32_t *__restrict__ n_long, int64_t T, int64_t S, const SRC *__restrict__ source, int64_t K,
             double *__restrict__ out) {
    __shared__ double lds[AP_BLOCK / 64][3];
    const int nl = *n_long;
    for (int li = blockIdx.x; li < nl; li += gridDim.x)
        apply_row_block<METHOD, SRC>(CsrRows{indptr, indices, data, row_order}, long_rows[li], T, S, source, K, out, lds);
}

// Listed rows with APPLY_LONG < entries <= APPLY_WAVE, KTILE source variables per pass, reduced by a GROUP of
// G lanes each: G = 16 (four rows per wave) up to APPLY_GROUP16 entries, G = 64 (one row per wave) beyond.
// The lanes of a group stride the row (entry j goes to lane j % G), so the CSR entries are read coalesced and
// -- rows are sorted by column -- neighbouring lanes gather neighbouring source values; the group's partial
// states are merged by a butterfly of log2(G) shuffles.  A lane's first four entries stay in registers across
// the variable tiles.  (APPLY_GROUP16: xr_apply.h)

template <int METHOD, typename SRC, int KTILE, int G>
__device__ __forceinline__ void apply_row_group(const int32_t *__restrict__ indices, const double *__restrict__ data,
                                                int s, int e, int64_t t_out, int64_t T, int64_t S,
                                                const SRC *__restrict__ source, int64_t K, double *__restrict__ out) {
    const int gl = threadIdx.x & (G - 1); // lane within the group
    int col4[4];
    double w4[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int j = s + gl + G * u;
        col4[u] = j < e ? indices[j] : -1;
        w4[u] = j < e ? data[j] : 0.0;
    }
    double normsum = 0.0;
    if (METHOD == XR_GEOMETRIC_MEAN) {
        Red<XR_SUM> ws; // b accumulates the weights
        for (int j = s + gl; j < e; j += G) ws.b += data[j];
        group_merge<XR_SUM, G>(ws);
        normsum = ws.b;
    }
    for (int64_t k0 = (int64_t)blockIdx.y * KTILE; k0 < K; k0 += (int64_t)gridDim.y * KTILE) {
        const int kn = (int)((K - k0) < KTILE ? (K - k0) : KTILE);
        const SRC *src = source + k0 * S;
        Red<METHOD> r[KTILE];
        double v[4][KTILE];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++)
                v[u][kk] = (col4[u] >= 0 && kk < kn) ? ld_src(src, (int64_t)kk * S + col4[u]) : 0.0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (col4[u] >= 0) {
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++)
                    if (kk < kn) r[kk].add(v[u][kk], w4[u], normsum);
            }
        }
        for (int j = s + gl + 4 * G; j < e; j += G) {
            const int64_t col = indices[j];
            const double w = data[j];
            double vv[KTILE];
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++) vv[kk] = kk < kn ? ld_src(src, (int64_t)kk * S + col) : 0.0;
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++)
                if (kk < kn) r[kk].add(vv[kk], w, normsum);
        }
#pragma unroll
        for (int kk = 0; kk < KTILE; kk++) group_merge<METHOD, G>(r[kk]);
        if (gl == 0) {
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++) {
                if (kk < kn) {
                    double res = r[kk].fin();
                    if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) res = NAN;
                    out[(k0 + kk) * T + t_out] = res;
                }
            }
        }
    }
}

// the listed rows of APPLY_LONG + 1 ... APPLY_WAVE entries, dealt to `n_waves` waves (this one is `wave`); rows beyond
// APPLY_WAVE entries are queued in huge_rows ([0] = count) when given, else left to the caller
template <int METHOD, typename SRC, int KTILE, typename ROWS>
__device__ __forceinline__ void apply_wave_rows(const ROWS &rows, const int32_t *__restrict__ long_rows, int nl, int wave,
                                                int n_waves, int64_t T, int64_t S, const SRC *__restrict__ source, int64_t K,
                                                double *__restrict__ out, int32_t *__restrict__ huge_rows) {
    const int lane = threadIdx.x & 63;
    // pass 1: four listed rows per wave, 16 lanes each
    for (int li0 = wave * 4; li0 < nl; li0 += n_waves * 4) {
        const int li = li0 + (lane >> 4);
        int t = 0, s = 0, e = 0;
        int64_t t_out = 0;
        if (li < nl) {
            t = long_rows[li];
            rows.segment(t, s, e);
            t_out = rows.out_row(t);
            if (e - s > APPLY_GROUP16) e = s; // other passes
        }
        // (the shuffles inside are wave-wide: every lane takes part, idle groups carry empty rows)
        if (__any(e > s)) {
            if (e > s)
                apply_row_group<METHOD, SRC, KTILE, 16>(rows.columns(t), rows.weights(t), s, e, t_out, T, S, source, K, out);
        }
    }
    // pass 2: one listed row per wave; rows beyond APPLY_WAVE entries are queued for the block kernel
    for (int li = wave; li < nl; li += n_waves) {
        const int t = long_rows[li];
        int s, e;
        rows.segment(t, s, e);
        if (e - s <= APPLY_GROUP16) continue;
        if (e - s > APPLY_WAVE) { // [0] = count
            if (huge_rows && lane == 0 && blockIdx.y == 0) huge_rows[1 + atomicAdd(huge_rows, 1)] = t;
            continue;
        }
        apply_row_group<METHOD, SRC, KTILE, 64>(rows.columns(t), rows.weights(t), s, e, rows.out_row(t), T, S, source, K, out);
    }
}

template <int METHOD, typename SRC, int KTILE>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_wave(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
             const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
             const int32_t *__restrict__ n_long, int64_t T, int64_t S, const SRC *__restrict__ source, int64_t K,
             double *__restrict__ out, int32_t *__restrict__ huge_rows) {
    const int wave = (blockIdx.x * AP_BLOCK + threadIdx.x) >> 6, n_waves = gridDim.x * (AP_BLOCK / 64);
    apply_wave_rows<METHOD, SRC, KTILE>(CsrRows{indptr, indices, data, row_order}, long_rows, *n_long, wave, n_waves, T, S,
                                        source, K, out, huge_rows);
}

// K = 1, every row in ONE launch.  Blocks [0, n_long_blocks) take the listed long rows (lane groups / waves, then the rows
// beyond APPLY_WAVE entries block by block) -- they are dispatched first and run beside the short rows, no second and third
// launch behind the kernel, no fork / join.  The other blocks take AP_BLOCK stored rows each, every WAVE on its own: a wave
// stages the CSR segment of its 64 consecutive rows -- contiguous -- in a private LDS window in chunks of W1_CAP entries
// (column and weight loaded coalesced, the source value gathered by the same lane and parked next to the weight), then every
// lane reduces ITS row from the window, sequentially in CSR order (bit-identical to the reference loop,
// regridder.py:52-62).  No block barrier anywhere and 6 KB of LDS per wave: 24 waves per CU keep three dependent
// round trips (row pointers -> entries -> source values) in flight, where the block-wide version of rounds 1-2 (32 KB
// and four barriers per block) held 20 (MI355X, 1M x 1M benchmark: 42.6 -> see DESIGN section 5).
// The long-row role of the K = 1 kernels: block `block` of `n_blocks` leading blocks takes its share of the listed rows (lane
// groups / waves, then the rows beyond APPLY_WAVE entries block by block).  sh_win: the block's window memory (these
// blocks stage nothing in it).
template <int METHOD, typename SRC, typename ROWS>
__device__ __forceinline__ void rows1_long_role(const ROWS &rows, const int32_t *__restrict__ long_rows, int nl, int block,
                                                int n_blocks, bool any_huge, int64_t T, int64_t S,
                                                const SRC *__restrict__ source, double *__restrict__ out, double2 *sh_win) {
    double(*sh_merge)[3] = reinterpret_cast<double(*)[3]>(sh_win);
    const int wib = threadIdx.x >> 6;
    apply_wave_rows<METHOD, SRC, 1>(rows, long_rows, nl, block * (AP_BLOCK / 64) + wib, n_blocks * (AP_BLOCK / 64), T, S, source, 1,
                                    out, nullptr);
    if (any_huge) {
        // rows beyond the wave kernel's reach, a block each.  The block's share of the list is looked at by all its
        // threads AT ONCE (entry li = block + n_blocks * thread: two dependent loads per thread, in flight
        // together) and the few hits are parked in LDS -- walking the share entry by entry was a chain of ~9 x 2
        // dependent round trips that made these blocks the last to finish (the kernel's 28 us on the benchmark).
        int *sh_list = reinterpret_cast<int *>(sh_win + W1_CAP), *sh_cnt = reinterpret_cast<int *>(sh_win + 2 * W1_CAP);
        for (int base = 0; base < nl; base += n_blocks * AP_BLOCK) {
            if (threadIdx.x == 0) *sh_cnt = 0;
            __syncthreads();
            const int li = base + block + n_blocks * (int)threadIdx.x;
            if (li < nl) {
                const int t = long_rows[li];
                int s, e;
                rows.segment(t, s, e);
                if (e - s > APPLY_WAVE) sh_list[atomicAdd(sh_cnt, 1)] = t; // (at most one per thread)
            }
            __syncthreads();
            const int n_hit = *sh_cnt;
            for (int i = 0; i < n_hit; i++) // (uniform: every thread of the block works on the row)
                apply_row_block<METHOD, SRC>(rows, sh_list[i], T, S, source, 1, out, sh_merge);
            __syncthreads();
        }
    }
}

// The regular role: block `block` of `n_blocks` takes AP_BLOCK of the stored rows [0, T), every wave on its own window.
// skip_long: rows beyond APPLY_LONG entries are left to the long-row role.
template <int METHOD, typename SRC>
__device__ __forceinline__ void rows1_regular_role(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                   const double *__restrict__ data, const int32_t *__restrict__ row_order,
                                                   int block, int n_blocks, bool skip_long, int64_t T,
                                                   const SRC *__restrict__ source, double *__restrict__ out, double2 *sh_win) {
    // (last row blocks first: weights built by xr_overlap keep the rows of the big target faces at the end)
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int64_t row0 = ((int64_t)(n_blocks - 1 - block) * (AP_BLOCK / 64) + wib) * 64;
    if (row0 >= T) return;
    const int64_t t = row0 + lane;
    int s = 0, e = 0;
    if (t < T) {
        s = indptr[t];
        e = indptr[t + 1];
    }
    const bool skip = skip_long && (e - s > APPLY_LONG); // reduced by the long-row blocks
    const int seg0 = __shfl(s, 0, 64);
    const int seg1 = wave_reduce<OpMax>(e); // (lanes beyond T hold 0: the maximum is the end of the last valid row)
    if (skip) e = s;
    const bool jumpy = __any(skip);
    double2 *win = sh_win + (size_t)wib * W1_CAP;
    // first entry any lane still needs at or behind c0 (a window must not stream the entries of skipped long rows)
    auto next_chunk = [&](int c0) -> int {
        if (!jumpy) return c0;
        int mine = (e > s && e > c0) ? (s > c0 ? s : c0) : INT_MAX;
        return wave_reduce<OpMin>(mine);
    };
    double normsum = 0.0;
    if (METHOD == XR_GEOMETRIC_MEAN) {
        for (int c0 = seg0; c0 < seg1; c0 += W1_CAP) {
            c0 = next_chunk(c0);
            if (c0 >= seg1) break;
            for (int j = c0 + lane; j < c0 + W1_CAP && j < seg1; j += 64) win[j - c0].x = data[j];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int a = s > c0 ? s : c0, b = e < c0 + W1_CAP ? e : c0 + W1_CAP;
            for (int j = a; j < b; j++) normsum += win[j - c0].x;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    Red<METHOD> red;
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
            red.add(wv.y, wv.x, normsum);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (the window is overwritten by the next chunk)
        __builtin_amdgcn_wave_barrier();
    }
    if (t < T && !skip) {
        const int64_t t_out = row_order ? (int64_t)row_order[t] : t;
        double r = NAN; // regridder.py:44,62: rows without entries stay NaN
        if (e > s) {
            r = red.fin();
            if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) r = NAN;
        }
        out[t_out] = r;
    }
}

template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_rows1(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
              const int32_t *__restrict__ row_order, const int32_t *__restrict__ long_rows,
              const int32_t *__restrict__ n_long, int n_long_blocks, bool any_huge, int64_t T, int64_t S,
              const SRC *__restrict__ source, double *__restrict__ out, const int32_t *__restrict__ gate) {
    __shared__ double2 sh_win[AP_BLOCK / 64][W1_CAP]; // (.x = weight, .y = source value); 24 KB: 6 blocks per CU
    if (gate && *gate == 0) return; // (enqueued behind a weight build whose attempt failed: the host redoes both)
    if ((int)blockIdx.x < n_long_blocks)
        return rows1_long_role<METHOD, SRC>(CsrRows{indptr, indices, data, row_order}, long_rows, *n_long, (int)blockIdx.x,
                                            n_long_blocks, any_huge, T, S, source, out, &sh_win[0][0]);
    rows1_regular_role<METHOD, SRC>(indptr, indices, data, row_order, (int)blockIdx.x - n_long_blocks,
                                    (int)gridDim.x - n_long_blocks, n_long_blocks > 0, T, source, out, &sh_win[0][0]);
}

// k_apply_rows1 enqueued behind a fused weight build (overlap_tri) whose big faces' rows have NOT been copied behind the regular
// ones: the launch makes that copy itself and needs it for nothing.  Three block-uniform roles:
//   blocks [0, TAIL_PLACE_BLOCKS)     place_big_copy, the body of k_place_big (the matrix is complete behind the launch), then
//                                     the big rows of at most APPLY_LONG entries, which are on no list: one lane each,
//                                     sequentially in CSR order like a window lane -- eight entries' loads in flight
//   the n_long_blocks behind them     the listed long rows; a listed row >= T - n_big is read from the big faces' own CSR
//                                     (TailRows)
//   the others                        the wave windows over the stored rows [0, T - n_big): indptr[T - n_big] is the assembly's
// No block waits for, or reads, what another block of the launch writes; every row is summed in the order k_apply_rows1 sums it.
// The launch runs behind k_publish_all, on the words it left in the matrix (TailWord): the gate, n_big, the regular rows'
// entries, the number of listed rows.
template <int METHOD, typename SRC>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_tail1(ApplyTail tail, const int32_t *__restrict__ long_rows, int n_long_blocks, int64_t T, int64_t S,
              const SRC *__restrict__ source, double *__restrict__ out) {
    __shared__ double2 sh_win[AP_BLOCK / 64][W1_CAP]; // 24 KB: 6 blocks per CU, as k_apply_rows1
    const PlaceBig &p = tail.place;
    if (tail.words[TAIL_GATE] == 0) return; // (a failed attempt: the host redoes build and apply; nothing is touched)
    const int n_big = tail.words[TAIL_N_BIG];
    const int t_big = (int)(T - n_big);
    const int b = (int)blockIdx.x;
    const TailRows rows{CsrRows{p.indptr, p.indices, p.data, p.row_order}, t_big, p.big_indptr, p.big_indices, p.big_data,
                        p.slot_face, p.q_perm};
    if (b < TAIL_PLACE_BLOCKS) {
        if (n_big == 0) return;
        // (the gate has made k_place_big's checks; the control block is at rest and not touched)
        place_big_copy<true>(p, n_big, tail.words[TAIL_P_REGULAR], p.big_indptr[n_big], b, TAIL_PLACE_BLOCKS);
        for (int k = b * AP_BLOCK + (int)threadIdx.x; k < n_big; k += TAIL_PLACE_BLOCKS * AP_BLOCK) {
            const int s = p.big_indptr[k], e = p.big_indptr[k + 1];
            if (e - s > APPLY_LONG) continue; // listed
            double normsum = 0.0;
            if (METHOD == XR_GEOMETRIC_MEAN) {
                for (int j0 = s; j0 < e; j0 += 8) {
                    double w[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) w[u] = j0 + u < e ? p.big_data[j0 + u] : 0.0;
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (j0 + u < e) normsum += w[u];
                }
            }
            Red<METHOD> red;
            for (int j0 = s; j0 < e; j0 += 8) {
                int col[8];
                double w[8], v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    col[u] = j0 + u < e ? p.big_indices[j0 + u] : -1;
                    w[u] = j0 + u < e ? p.big_data[j0 + u] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = col[u] >= 0 ? ld_src(source, (int64_t)col[u]) : 0.0;
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (col[u] >= 0) red.add(v[u], w[u], normsum);
            }
            double r = NAN; // rows without entries stay NaN
            if (e > s) {
                r = red.fin();
                if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) r = NAN;
            }
            out[rows.big_out_row(k)] = r;
        }
        return;
    }
    if (b < TAIL_PLACE_BLOCKS + n_long_blocks)
        return rows1_long_role<METHOD, SRC>(rows, long_rows, tail.words[TAIL_N_LONG], b - TAIL_PLACE_BLOCKS, n_long_blocks, true, T,
                                            S, source, out, &sh_win[0][0]);
    const int n_lead = TAIL_PLACE_BLOCKS + n_long_blocks;
    rows1_regular_role<METHOD, SRC>(p.indptr, p.indices, p.data, p.row_order, b - n_lead, (int)gridDim.x - n_lead, true, t_big,
                                    source, out, &sh_win[0][0]);
}

// Many source variables (K >= 2): one thread per row keeps KTILE reducer states in registers and
// walks its row once per k-tile; no LDS, so occupancy is limited by registers only and every
// thread has KTILE independent gathers in flight per entry.  Rows are visited in stored (spatial)
// order, so the gathers of neighbouring threads hit the same cache lines.
template <int METHOD, typename SRC, int KTILE>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_direct(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
               const double *__restrict__ data, const int32_t *__restrict__ row_order, bool skip_long, int64_t T,
               int64_t S, const SRC *__restrict__ source, int64_t K, double *__restrict__ out,
               const int32_t *__restrict__ block_list) {
    // block_list != nullptr: only these 256-row blocks (the ones the apply plan could not take)
    const int64_t t = (int64_t)(block_list ? block_list[blockIdx.x] : blockIdx.x) * AP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int64_t k0 = (int64_t)blockIdx.y * KTILE;
    const int kn = (int)((K - k0) < KTILE ? (K - k0) : KTILE);
    const int s = indptr[t], e = indptr[t + 1];
    if (skip_long && e - s > APPLY_LONG) return; // reduced by k_apply_long
    const int64_t t_out = row_order ? (int64_t)row_order[t] : t;
    const SRC *src = source + k0 * S;
    double normsum = 0.0;
    if (METHOD == XR_GEOMETRIC_MEAN)
        for (int j = s; j < e; j++) normsum += data[j];
    Red<METHOD> red[KTILE];
    int j = s;
    if (KTILE <= 4) {
        // four entries' gathers in flight before their (sequential, CSR-order) additions: a thread that walks a
        // long row alone is otherwise one HBM latency per entry
        for (; j + 3 < e; j += 4) {
            int64_t col[4];
            double w[4], v[4][KTILE];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                col[u] = indices[j + u];
                w[u] = data[j + u];
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++) v[u][kk] = kk < kn ? ld_src(src, (int64_t)kk * S + col[u]) : 0.0;
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++)
                    if (kk < kn) red[kk].add(v[u][kk], w[u], normsum);
        }
    }
    for (; j < e; j++) {
        const int64_t col = indices[j];
        const double w = data[j];
        double v[KTILE];
#pragma unroll
        for (int kk = 0; kk < KTILE; kk++) v[kk] = kk < kn ? ld_src(src, (int64_t)kk * S + col) : 0.0;
#pragma unroll
        for (int kk = 0; kk < KTILE; kk++)
            if (kk < kn) red[kk].add(v[kk], w, normsum);
    }
#pragma unroll
    for (int kk = 0; kk < KTILE; kk++) {
        if (kk < kn) {
            double r = NAN;
            if (e > s) {
                r = red[kk].fin();
                if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) r = NAN;
            }
            out[(k0 + kk) * T + t_out] = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// apply plan: blocked CSR with per-block distinct-column lists.
// A block of 256 spatially adjacent rows references ~5x fewer DISTINCT source faces than it has
// entries.  With many source variables the gathers dominate, so each distinct source value is
// loaded ONCE per (block, variable) -- lanes run over the ascending column list, neighbours share
// cache lines -- into LDS, and the rows are reduced from LDS through 16-bit local indices.
// ---------------------------------------------------------------------------------------------
static constexpr int PLAN_LMAX = 4096; // entries of a block the builder can sort in LDS
static constexpr int PLAN_UMAX = 512;  // distinct columns per block kept in the plan

__global__ void __launch_bounds__(AP_BLOCK)
k_plan_build(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t T,
             int32_t *__restrict__ ucol, int32_t *__restrict__ nuniq, uint16_t *__restrict__ loc,
             int32_t *__restrict__ max_entries, int32_t *__restrict__ unplanned, int32_t *__restrict__ n_unplanned,
             int entry_cap) {
    __shared__ int32_t keys[PLAN_LMAX];
    __shared__ int32_t uniq[PLAN_UMAX];
    __shared__ int32_t sh_wave[4];
    __shared__ int32_t sh_lines;
    const int64_t row0 = (int64_t)blockIdx.x * AP_BLOCK;
    const int64_t row_end = row0 + AP_BLOCK < T ? row0 + AP_BLOCK : T;
    const int seg0 = indptr[row0], seg1 = indptr[row_end];
    const int n = seg1 - seg0;
    if (n > entry_cap) {
        if (threadIdx.x == 0) {
            nuniq[blockIdx.x] = -1;
            unplanned[atomicAdd(n_unplanned, 1)] = (int32_t)blockIdx.x;
        }
        return;
    }
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += AP_BLOCK) keys[i] = i < n ? indices[seg0 + i] : 0x7fffffff;
    __syncthreads();
    // bitonic sort, ascending
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += AP_BLOCK) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // unique: each thread owns a contiguous slice of the sorted keys
    const int per = (n + AP_BLOCK - 1) / AP_BLOCK;
    const int a0 = threadIdx.x * per, a1 = a0 + per < n ? a0 + per : n;
    int cnt = 0;
    for (int i = a0; i < a1; i++) cnt += (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(cnt);
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) woff += sh_wave[w];
        total += sh_wave[w];
    }
    if (total > PLAN_UMAX) {
        if (threadIdx.x == 0) {
            nuniq[blockIdx.x] = -1;
            unplanned[atomicAdd(n_unplanned, 1)] = (int32_t)blockIdx.x;
        }
        return;
    }
    int pos = woff + incl - cnt;
    for (int i = a0; i < a1; i++) {
        if (i == 0 || keys[i] != keys[i - 1]) uniq[pos++] = keys[i];
    }
    __syncthreads();
    for (int u = threadIdx.x; u < total; u += AP_BLOCK) ucol[(int64_t)blockIdx.x * PLAN_UMAX + u] = uniq[u];
    // how well the block uses the source lines it touches (16 values of 8 bytes per 128-byte line): the sums over all blocks
    // decide whether a merged plan pays (ensure_plan)
    if (threadIdx.x == 0) sh_lines = 0;
    __syncthreads();
    {
        int mine = 0;
        for (int u = threadIdx.x; u < total; u += AP_BLOCK) mine += (u == 0 || (uniq[u] >> 4) != (uniq[u - 1] >> 4)) ? 1 : 0;
        if (mine) atomicAdd(&sh_lines, mine);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(max_entries + 2, total);
        atomicAdd(max_entries + 3, sh_lines);
    }
    if (threadIdx.x == 0) atomicMax(max_entries, n); // the apply kernel sizes its LDS stage for the largest planned block
    if (threadIdx.x == 0) nuniq[blockIdx.x] = total;
    // local index of every entry: binary search in the distinct list
    for (int i = threadIdx.x; i < n; i += AP_BLOCK) {
        const int c = indices[seg0 + i];
        int lo = 0, hi = total - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (uniq[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        loc[seg0 + i] = (uint16_t)lo;
    }
}

// MERGED plan (round 5): ONE distinct-column list per GROUP of PLAN_GROUP neighbouring row blocks.  On a qhull-numbered mesh a
// block of 256 rows uses ~4 of the 16 values of every source line it touches, a group of 512 rows 4.5, of 1024 rows 5 (66 / 52
// lines per 256 rows instead of 85: profiles/r05_experiments/analysis_column_locality.*): the group's workgroup gathers every
// line once for all its row blocks.  (Blocks in lockstep with a list EACH -- XR_PLAN_SUBS -- do not get there: the lines in
// flight, 4 x 85 x 8 variables x 128 bytes, are ten times the L1, the siblings' requests miss again.)  Groups of two and of four
// measured the same on the benchmark matrix (K = 256: 1.64 -> 1.53 / 1.56 ms: what the larger group saves in line fills its
// 16-wave barriers cost); two blocks need 58 KB of LDS (two workgroups per CU) and cost a lattice-numbered matrix 2 %, four 7 %.
static constexpr int PLAN_GROUP = 2;
static constexpr int PLAN_GUMAX = 1024; // distinct columns per group kept in the plan
__global__ void __launch_bounds__(AP_BLOCK * PLAN_GROUP)
k_plan_build_group(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t T,
                   int32_t *__restrict__ ucol, int32_t *__restrict__ nuniq, uint16_t *__restrict__ loc,
                   int32_t *__restrict__ max_entries, int32_t *__restrict__ unplanned, int32_t *__restrict__ n_unplanned,
                   int entry_cap) {
    constexpr int NT = AP_BLOCK * PLAN_GROUP, KMAX = PLAN_LMAX * 2; // (8192 keys: the group's blocks of up to 2048 entries each)
    __shared__ int32_t keys[KMAX];
    __shared__ int32_t uniq[PLAN_GUMAX];
    __shared__ int32_t sh_wave[NT / 64];
    __shared__ int32_t sh_bad;
    const int64_t n_blocks = (T + AP_BLOCK - 1) / AP_BLOCK;
    const int64_t b0 = (int64_t)blockIdx.x * PLAN_GROUP;
    const int64_t row0 = b0 * AP_BLOCK;
    const int64_t row_end = row0 + NT < T ? row0 + NT : T;
    const int seg0 = indptr[row0], seg1 = indptr[row_end];
    const int n = seg1 - seg0;
    if (threadIdx.x == 0) sh_bad = 0;
    __syncthreads();
    // every block of the group has to fit the apply's per-block stage
    if (threadIdx.x < PLAN_GROUP) {
        const int64_t r0 = row0 + (int64_t)threadIdx.x * AP_BLOCK;
        if (r0 < T) {
            const int64_t r1 = r0 + AP_BLOCK < T ? r0 + AP_BLOCK : T;
            const int nb_e = indptr[r1] - indptr[r0];
            if (nb_e > entry_cap) sh_bad = 1;
        }
    }
    __syncthreads();
    auto give_up = [&]() {
        if (threadIdx.x == 0) {
            nuniq[blockIdx.x] = -1;
            for (int g = 0; g < PLAN_GROUP; g++)
                if (b0 + g < n_blocks) unplanned[atomicAdd(n_unplanned, 1)] = (int32_t)(b0 + g);
        }
    };
    if (sh_bad || n > KMAX) {
        give_up();
        return;
    }
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += NT) keys[i] = i < n ? indices[seg0 + i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1) { // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    const int per = (n + NT - 1) / NT;
    const int a0 = threadIdx.x * per < n ? threadIdx.x * per : n, a1 = a0 + per < n ? a0 + per : n;
    int cnt = 0;
    for (int i = a0; i < a1; i++) cnt += (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(cnt);
    __syncthreads();
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < NT / 64; w++) {
        if (w < wave) woff += sh_wave[w];
        total += sh_wave[w];
    }
    if (total > PLAN_GUMAX) {
        give_up();
        return;
    }
    int pos = woff + incl - cnt;
    for (int i = a0; i < a1; i++)
        if (i == 0 || keys[i] != keys[i - 1]) uniq[pos++] = keys[i];
    __syncthreads();
    for (int u = threadIdx.x; u < total; u += NT) ucol[(int64_t)blockIdx.x * PLAN_GUMAX + u] = uniq[u];
    if (threadIdx.x < PLAN_GROUP) { // the apply kernel sizes its per-block stage for the largest planned block
        const int64_t r0 = row0 + (int64_t)threadIdx.x * AP_BLOCK;
        if (r0 < T) {
            const int64_t r1 = r0 + AP_BLOCK < T ? r0 + AP_BLOCK : T;
            atomicMax(max_entries, indptr[r1] - indptr[r0]);
        }
    }
    if (threadIdx.x == 0) nuniq[blockIdx.x] = total;
    for (int i = threadIdx.x; i < n; i += NT) { // local index of every entry: binary search in the group's list
        const int c = indices[seg0 + i];
        int lo = 0, hi = total - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (uniq[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        loc[seg0 + i] = (uint16_t)lo;
    }
}

// One block = 256 stored rows, ALL variables: the block's CSR entries (weight + 16-bit local column)
// are staged in LDS once, then the block walks the variables in tiles of KTILE.  Software pipeline
// (global -> registers -> LDS): the distinct source values of tile i+1 are requested into registers
// before tile i is reduced, and written to LDS after it -- HBM latency overlaps the reduction, so one
// resident block per CU is enough to keep its share of the memory system busy.
// SUBS > 1 (round 5): one workgroup = SUBS neighbouring row blocks (SUBS x 256 threads, every sub-block with its own plan and its
// own LDS region) that walk the variable tiles in LOCKSTEP -- the group's barriers are the workgroup's.  On a mesh whose
// numbering is coherent but not compact (qhull) a row block uses ~4 of the 16 source values of a 128-byte line and its
// neighbours use the rest: as separate workgroups they drift apart and every one of them fetches the line on its own -- the L1
// of a CU holds 256 lines, the L2 of an XCD four microseconds of traffic --, in lockstep on ONE CU the requests for a line meet
// in that CU's L1.
// FAST (round 6; opt-in for `mean` / `first_order_conservative`: option "apply_contract"): on NaN-free tiles the
// products are CONTRACTED into the running sums (one fused multiply-add per entry and variable instead of a multiplication and
// an addition) and the mean is the sum times ONE reciprocal of the row's weight sum (computed once per row, outside the loop
// over the variable tiles) instead of an IEEE division per variable -- the reduction was the kernel's floor (0.71-0.81 ms of
// vector work per K = 256 apply against 0.52 ms of memory time).  The results then differ from the reference's sequential
// loop (regridder.py:41-67) by the roundings of at most n products (n = entries of the row, 4 on average) and one
// multiplication: <= (n + 2) ulp of sum |w v| / sum w -- measured at full size 8e-16 of the field's range, but 1e-9 RELATIVE where a
// mean of mixed-sign data cancels to ~1e-7 of that range.  What it buys (profiles/r06_apply_fast_ab.txt): K = 256 on the
// lattice-numbered pair 1.01 -> 0.92 ms (50 -> 56 % of HBM), on the qhull-numbered benchmark matrix 1.57 -> 1.53 ms (that one is
// bound by its line fills, not by the reduction).  The default stays the reference's operation order, bit for bit.
// The staged tile of distinct source values in LDS is VARIABLE-minor (round 6): the KTILE values of a column in KTILE / 2 consecutive
// 16-byte slots, read with ds_read_b128 (which reaches its rate from one wave per SIMD; ds_read_b64 needs ~4 and the kernel has 3) --
// the slot of a pair XOR-swizzled with the column so that, for a fixed pair, the columns spread over all 16 slot positions of a
// 256-byte LDS row.  Until round 5 it was variable-MAJOR (vals[kk][u]: a ds_read_b64 at a random column per variable).  Same values,
// same arithmetic; measured with gathers and stores off (option plan_dbg = 3, the reduction's floor): merged plan 0.785 -> 0.685 ms,
// per-block plan 0.588 -> 0.502 ms per K = 256 apply; whole kernel - 1.5 ... 2 % (profiles/r06_experiments/apply_lds_layout_ab.txt).
template <int KTILE> __device__ __forceinline__ int plan_slot(int u, int k2) {
    static_assert(KTILE == 8 || KTILE == 4, "tiles of 4 or 8 variables");
    return KTILE == 8 ? u * 4 + (k2 ^ ((u >> 2) & 3)) : u * 2 + (k2 ^ ((u >> 3) & 1));
}
template <int METHOD, typename SRC, int KTILE, int SUBS, bool MERGE = false, bool FAST = false>
__global__ void __launch_bounds__(AP_BLOCK * SUBS)
k_apply_plan(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
             const int32_t *__restrict__ ucol, const int32_t *__restrict__ nuniq, const uint16_t *__restrict__ loc,
             const int32_t *__restrict__ row_order, bool skip_long, int64_t T, int64_t S,
             const SRC *__restrict__ source, int64_t K, double *__restrict__ out, int lmax, int super_blocks, int item_tiles, int dbg) {
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const int sub = SUBS > 1 ? (int)threadIdx.x / AP_BLOCK : 0, tid = SUBS > 1 ? (int)threadIdx.x % AP_BLOCK : (int)threadIdx.x;
    // MERGE: ONE value table for the workgroup (the group's distinct columns), the entries of every row block behind it
    static_assert(!MERGE || SUBS == PLAN_GROUP, "a merged plan is built for groups of PLAN_GROUP row blocks");
    constexpr int UMAX = MERGE ? PLAN_GUMAX : PLAN_UMAX;                  // columns of the value table
    constexpr int GATHERERS = MERGE ? AP_BLOCK * SUBS : AP_BLOCK;         // threads that share a list
    const size_t stage_bytes = ((sizeof(double) * (size_t)lmax + sizeof(uint16_t) * (size_t)lmax) + 15) / 16 * 16;
    char *smem = MERGE ? smem_all
                       : smem_all + (size_t)sub * (((sizeof(double) * (KTILE * PLAN_UMAX + lmax) + sizeof(uint16_t) * lmax) + 15) / 16 * 16);
    double *vals = reinterpret_cast<double *>(smem);                      // [UMAX][KTILE / 2] 16-byte slots, swizzled (plan_slot)
    double *sh_w = MERGE ? reinterpret_cast<double *>(smem_all + sizeof(double) * KTILE * UMAX + (size_t)sub * stage_bytes)
                         : vals + KTILE * PLAN_UMAX;                      // [lmax] = entries of the largest planned block
    uint16_t *sh_loc = reinterpret_cast<uint16_t *>(sh_w + lmax);         // [lmax]
    constexpr int UPT = UMAX / GATHERERS;                                 // distinct columns per thread
    const int gtid = MERGE ? (int)threadIdx.x : tid;                      // index among the threads that share the list
    // XCD-aware block order: hardware block b runs on XCD b % 8; give every XCD a CONTIGUOUS range of
    // row blocks (= one spatial region), so that lines shared by neighbouring blocks stay in one L2
    const int64_t n_blocks = (T + AP_BLOCK - 1) / AP_BLOCK;           // row blocks
    const int64_t n_groups = (n_blocks + SUBS - 1) / SUBS;            // workgroups' worth of them
    const int64_t per_xcd = (n_groups + 7) / 8;
    int64_t lg = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    int64_t k_begin = 0, k_end = K;
    if (super_blocks > 0) {
        // L2-blocked order (round 5).  A block of 256 rows uses ~4 of the 16 source values of every 128-byte line it touches
        // (a qhull-numbered mesh: spatial neighbours are not id neighbours); the rest of the line belongs to NEIGHBOURING row
        // blocks, and a block that walks all K variables on its own drifts away from them -- the line comes from HBM once per
        // block (PMC, K = 128: 24 M fabric reads against 7 M for a lattice-numbered pair).  Here a work item is one row block x
        // `item_tiles` variable tiles, and an XCD's items are ordered (super tile of `super_blocks` neighbouring row blocks) ->
        // (variable item) -> (row block): the blocks resident on an XCD at any time share one super tile and one variable
        // item, whose source lines (~1.4 MB for 64 blocks x 8 variables) stay in that XCD's 4 MB L2.
        const int64_t n_items = (K + (int64_t)KTILE * item_tiles - 1) / ((int64_t)KTILE * item_tiles);
        const int64_t i = blockIdx.x >> 3;
        const int64_t per_super = (int64_t)super_blocks * n_items;
        const int64_t sup = i / per_super, rem = i - sup * per_super;
        const int64_t item = rem / super_blocks, b = rem - item * super_blocks;
        const int64_t local = sup * super_blocks + b;
        if (local >= per_xcd) return;
        lg = (int64_t)(blockIdx.x & 7) * per_xcd + local;
        k_begin = item * KTILE * item_tiles;
        k_end = k_begin + (int64_t)KTILE * item_tiles < K ? k_begin + (int64_t)KTILE * item_tiles : K;
    }
    if (lg >= n_groups) return; // (uniform over the workgroup)
    const int64_t lb = lg * SUBS + sub;
    // (a sub-block without work -- past the last row block, or unplanned: too many entries / distinct columns, k_apply_direct takes
    // those over its block list -- stays for the workgroup's barriers; SUBS == 1: it leaves)
    const int64_t row0 = (lb < n_blocks ? lb : 0) * AP_BLOCK;
    const int nu = MERGE ? nuniq[lg] : (lb < n_blocks ? nuniq[lb] : -1);
    if ((SUBS == 1 || MERGE) && nu < 0) return; // (uniform over the workgroup)
    const bool active = nu >= 0 && lb < n_blocks;
    const int64_t t = active ? row0 + tid : T;
    const int64_t row_end = row0 + AP_BLOCK < T ? row0 + AP_BLOCK : T;
    int s = 0, e = 0;
    if (t < T) {
        s = indptr[t];
        e = indptr[t + 1];
    }
    const bool is_long = skip_long && (e - s > APPLY_LONG); // reduced by k_apply_long
    const int64_t t_out = (t < T && row_order) ? (int64_t)row_order[t] : t;
    // stage the block's entries once
    const int seg0 = indptr[row0], seg1 = active ? indptr[row_end] : seg0;
    for (int j = seg0 + tid; j < seg1; j += AP_BLOCK) {
        sh_w[j - seg0] = data[j];
        sh_loc[j - seg0] = loc[j];
    }
    // this thread's distinct columns
    int64_t mycol[UPT];
#pragma unroll
    for (int q = 0; q < UPT; q++) {
        const int u = q * GATHERERS + gtid;
        mycol[q] = (u < nu && !(dbg & 1)) ? (int64_t)ucol[(MERGE ? lg : lb) * UMAX + u] : -1; // (dbg: measurement switches, XR_PLAN_DBG)
    }
    __syncthreads();
    double normsum = 0.0;
    if (METHOD == XR_GEOMETRIC_MEAN && !is_long)
        for (int j = s; j < e; j++) normsum += sh_w[j - seg0];
    double wsum_row = 0.0; // sum of the row's weights in entry order (= Red::b when no value is NaN)
    if (!is_long)
        for (int j = s; j < e; j++) wsum_row += sh_w[j - seg0];
    const double inv_wsum = FAST ? 1.0 / wsum_row : 0.0; // (FAST: one division per row for all K variables)
    // prologue: request tile 0
    double stage[UPT][KTILE];
    {
        const int kn = (int)(k_end - k_begin < KTILE ? k_end - k_begin : KTILE);
        const SRC *src0 = source + k_begin * S;
#pragma unroll
        for (int q = 0; q < UPT; q++)
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++)
                stage[q][kk] = (mycol[q] >= 0 && kk < kn) ? ld_src(src0, (int64_t)kk * S + mycol[q]) : 0.0;
    }
    for (int64_t k0 = k_begin; k0 < k_end; k0 += KTILE) {
        const int kn = (int)((k_end - k0) < KTILE ? (k_end - k0) : KTILE);
        __syncthreads(); // everybody finished reading the previous tile
        int my_nan = 0;
#pragma unroll
        for (int q = 0; q < UPT; q++) {
            const int u = q * GATHERERS + gtid;
            if (u < nu) {
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++) my_nan |= (stage[q][kk] != stage[q][kk]) ? 1 : 0;
#pragma unroll
                for (int k2 = 0; k2 < KTILE / 2; k2++)
                    reinterpret_cast<double2 *>(vals)[plan_slot<KTILE>(u, k2)] = make_double2(stage[q][2 * k2], stage[q][2 * k2 + 1]);
            }
        }
        // block-uniform: does this tile hold any NaN?  (NaN-free tiles take the short path below)
        const bool tile_has_nan = __syncthreads_or(my_nan) != 0;
        // request the next tile while this one is reduced
        const int64_t k1 = k0 + KTILE;
        if (k1 < k_end) {
            const int kn1 = (int)((k_end - k1) < KTILE ? (k_end - k1) : KTILE);
            const SRC *src1 = source + k1 * S;
#pragma unroll
            for (int q = 0; q < UPT; q++)
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++)
                    stage[q][kk] = (mycol[q] >= 0 && kk < kn1) ? ld_src(src1, (int64_t)kk * S + mycol[q]) : 0.0;
        }
        constexpr bool LINEAR = METHOD == XR_MEAN || METHOD == XR_SUM || METHOD == XR_FIRST_ORDER_CONSERVATIVE;
        if (LINEAR && !tile_has_nan) {
            // no NaN anywhere in the tile: the weight sum of a row is the same for every variable
            // (computed once, wsum_row) and the value sums need no per-entry test.  Same additions
            // in the same order as the general path -> bit-identical results.
            if (t < T && !is_long) {
                double acc[KTILE];
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++) acc[kk] = 0.0;
                for (int j = s - seg0; j < e - seg0; j++) {
                    const int l = sh_loc[j];
                    const double w = sh_w[j];
                    double v[KTILE];
#pragma unroll
                    for (int k2 = 0; k2 < KTILE / 2; k2++) {
                        const double2 t2 = reinterpret_cast<const double2 *>(vals)[plan_slot<KTILE>(l, k2)];
                        v[2 * k2] = t2.x;
                        v[2 * k2 + 1] = t2.y;
                    }
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++) {
                        if (METHOD == XR_SUM) acc[kk] += v[kk];
                        else if (FAST) acc[kk] = fma(w, v[kk], acc[kk]);
                        else if (METHOD == XR_MEAN) acc[kk] += w * v[kk];
                        else acc[kk] += v[kk] * w;
                    }
                }
                if (FAST && METHOD == XR_MEAN) {
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++) acc[kk] *= inv_wsum;
                }
                const bool defined = e > s && wsum_row != 0;
                double *o = out + k0 * T + t_out;
                if (dbg & 2) { // (measurement: no stores -- the compiler must not know)
                    if (acc[0] != 12345.678) continue;
                }
                if (kn == KTILE && !(dbg & 4)) {
                    // whole tile: no per-variable branch around the stores.  Non-temporal: the result is written once and not
                    // read here -- it should not push the source lines that neighbouring row blocks still need out of the L2
                    // (1M x 1M, K = 256: 1.52 -> 1.44 ms qhull-numbered, 1.04 -> 0.99 ms lattice-numbered; XR_PLAN_DBG=4: plain stores)
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++)
                        __builtin_nontemporal_store(defined ? (METHOD == XR_MEAN && !FAST ? acc[kk] / wsum_row : acc[kk]) : NAN, &o[kk * T]);
                } else if (kn == KTILE) {
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++) o[kk * T] = defined ? (METHOD == XR_MEAN && !FAST ? acc[kk] / wsum_row : acc[kk]) : NAN;
                } else {
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++)
                        if (kk < kn) o[kk * T] = defined ? (METHOD == XR_MEAN && !FAST ? acc[kk] / wsum_row : acc[kk]) : NAN;
                }
            }
        } else if (t < T && !is_long) {
            Red<METHOD> red[KTILE];
            for (int j = s - seg0; j < e - seg0; j++) {
                const int l = sh_loc[j];
                const double w = sh_w[j];
                double v[KTILE];
#pragma unroll
                for (int k2 = 0; k2 < KTILE / 2; k2++) {
                    const double2 t2 = reinterpret_cast<const double2 *>(vals)[plan_slot<KTILE>(l, k2)];
                    v[2 * k2] = t2.x;
                    v[2 * k2 + 1] = t2.y;
                }
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++)
                    if (kk < kn) red[kk].add(v[kk], w, normsum);
            }
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++) {
                if (kk < kn) {
                    double r = NAN;
                    if (e > s) {
                        r = red[kk].fin();
                        if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) r = NAN;
                    }
                    out[(k0 + kk) * T + t_out] = r;
                }
            }
        }
    }
}

// option "plan_merge": 1 / 0 force a merged / per-block plan; -1 (default): merged when the blocks use less than PLAN_MERGE_UTIL of the 16
// values of the source lines they touch (measured by the per-block builder: ~4 on a qhull-numbered mesh, ~12 on a
// lattice-numbered one -- there the lockstep of a group costs 2 % and saves nothing)
static constexpr double PLAN_MERGE_UTIL = 6.0;
static int plan_merge_mode() { // (read when a matrix' plan is built, once per matrix: a test can switch between matrices)
    const int64_t e = option(OPT_PLAN_MERGE);
    return e < 0 ? -1 : (e == 1 ? 1 : 0);
}

void ensure_plan(const xr_csr *ccsr) {
    xr_csr *csr = const_cast<xr_csr *>(ccsr); // the plan is a cache attached to the weights
    if (csr->plan_ready) return;
    XR_REQUIRE(exclusive_held(), XR_ERR_INVALID, "internal: apply plan requested outside the exclusive scope");
    const int64_t nb = (csr->n + AP_BLOCK - 1) / AP_BLOCK;
    bool merged = plan_merge_mode() == 1;
    int64_t n_lists = nb;
    csr->plan_loc.alloc((size_t)csr->nnz);
    csr->plan_lmax = 256;
    csr->plan_n_unplanned = 0;
    // The apply sizes its LDS stage for the LARGEST planned block, and that decides how many blocks a CU holds: one block
    // of 4096 entries among thousands of 1000 (a Delaunay hull) costs every block a third of the occupancy (K = 256 on
    // the benchmark matrix: 1.76 -> 1.2 ms).  Blocks beyond 2048 entries (twice the typical triangle-mesh block) go to
    // the direct kernel instead.
    constexpr int plan_cap = 2048;
    if (nb > 0) {
        DevBuf<int32_t> max_entries(4); // [0] largest planned block, [1] number of unplanned blocks, [2] distinct columns, [3] distinct lines (sums over the planned blocks)
        csr->plan_unplanned.alloc((size_t)nb);
        auto build = [&](bool group) {
            n_lists = group ? (nb + PLAN_GROUP - 1) / PLAN_GROUP : nb;
            csr->plan_ucol.alloc((size_t)n_lists * (group ? PLAN_GUMAX : PLAN_UMAX));
            csr->plan_nuniq.alloc((size_t)n_lists);
            fill_i32(max_entries.get(), 0, 4);
            if (group)
                XR_LAUNCH("plan_build", k_plan_build_group, dim3((unsigned)n_lists), dim3(AP_BLOCK * PLAN_GROUP), 0, csr->indptr.get(),
                          csr->indices.get(), csr->n, csr->plan_ucol.get(), csr->plan_nuniq.get(), csr->plan_loc.get(),
                          max_entries.get(), csr->plan_unplanned.get(), max_entries.get() + 1, plan_cap);
            else
                XR_LAUNCH("plan_build", k_plan_build, dim3((unsigned)nb), dim3(AP_BLOCK), 0, csr->indptr.get(),
                          csr->indices.get(), csr->n, csr->plan_ucol.get(), csr->plan_nuniq.get(), csr->plan_loc.get(),
                          max_entries.get(), csr->plan_unplanned.get(), max_entries.get() + 1, plan_cap);
        };
        build(merged);
        int32_t h[4];
        d2h(h, max_entries.get(), sizeof(h));
        if (!merged && plan_merge_mode() < 0 && h[3] > 0 && nb >= 4 * PLAN_GROUP && (double)h[2] / (double)h[3] < PLAN_MERGE_UTIL) {
            // (poor use of the source lines: the group plan gathers a line once for the group's row blocks)
            merged = true;
            build(true);
            d2h(h, max_entries.get(), sizeof(h));
        }
        const int m = h[0];
        csr->plan_n_unplanned = h[1];
        csr->plan_lmax = std::min(PLAN_LMAX, std::max(256, (m + 255) / 256 * 256));
        if (option(OPT_DEBUG) & 2) {
            std::vector<int32_t> nu((size_t)n_lists);
            d2h(nu.data(), csr->plan_nuniq.get(), sizeof(int32_t) * (size_t)n_lists);
            double sum = 0; int cnt = 0, mx = 0;
            for (auto v : nu) if (v >= 0) { sum += v; cnt++; mx = std::max(mx, (int)v); }
            fprintf(stderr, "[plan] %s blocks %lld planned %d unplanned %d lmax %d avg distinct columns %.1f max %d nnz/block %.1f\n", merged ? "merged (a list per group of row blocks)" : "per block", (long long)nb, cnt,
                    csr->plan_n_unplanned, csr->plan_lmax, cnt ? sum / cnt : 0.0, mx, (double)csr->nnz / nb);
        }
    }
    csr->plan_merged = merged;
    csr->plan_ready = true;
}

// ---------------------------------------------------------------------------------------------
// workspace reducers: mode and percentile.  One thread per (row, k); per-row scratch lives in a
// global workspace laid out like the CSR data (ws[k_local][nnz]).
// ---------------------------------------------------------------------------------------------
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

template <typename SRC>
__global__ void k_apply_coo(const int32_t *__restrict__ row, const int32_t *__restrict__ col, int64_t nnz, int64_t T,
                            int64_t S, const SRC *__restrict__ source, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int64_t k = blockIdx.y;
    out[k * T + row[i]] = ld_src(source + k * S, col[i]);
}

// k_apply_plan over the matrix's plan: KT variables per tile, SUBS row blocks per workgroup (MERGED: one value table for
// the workgroup's SUBS = PLAN_GROUP row blocks).  LDS is sized for the largest planned block, so typical matrices run
// three blocks per CU instead of two.
// (tuning hooks: row blocks per workgroup, variables per tile, the L2-blocked order of k_apply_plan: super tiles of
// `super_blocks` workgroups x items of `item_tiles` variable tiles)
template <int METHOD, typename SRC, int KT, int SUBS, bool MERGED, bool FAST>
static void launch_plan(const xr_csr *csr, const SRC *src, int64_t K, double *out) {
    // default: items of 64 variables, super tile = the XCD's whole range of row blocks -- every XCD sweeps its row blocks
    // once per 64 variables (the source planes in flight: 0.5 GB instead of all K of them; what the host-side split
    // into groups of 128 variables did until round 4, without its extra launches, forks and joins)
    const int plan_dbg = (int)option(OPT_PLAN_DBG); // measurement: 1 no gathers, 2 no stores, 4 plain instead of non-temporal stores
    // LDS per row block: a tile of distinct source values + the block's entries (weight + 16-bit local column), sized for
    // the largest planned block of the matrix.  4 row blocks per workgroup: tiles of 4 variables (4 x 34 KB)
    const int lmax = csr->plan_lmax;
    const size_t sub_bytes = ((sizeof(double) * ((size_t)KT * PLAN_UMAX + lmax) + sizeof(uint16_t) * lmax) + 15) / 16 * 16;
    const size_t stage_bytes = ((sizeof(double) * (size_t)lmax + sizeof(uint16_t) * (size_t)lmax) + 15) / 16 * 16;
    const size_t shmem = MERGED ? sizeof(double) * (size_t)KT * PLAN_GUMAX + stage_bytes * PLAN_GROUP : sub_bytes * SUBS;
    XR_REQUIRE(shmem <= (size_t)160 * 1024, XR_ERR_LIMIT, "internal: apply plan needs %zu bytes of LDS", shmem);
    // (dynamic LDS beyond 64 KB has to be allowed per kernel; applies run concurrently under the shared scope, so the
    // high-water mark of this instantiation sits behind a mutex)
    {
        static std::mutex attr_mutex;
        static size_t granted = 0;
        std::lock_guard<std::mutex> lock(attr_mutex);
        if (shmem > granted) {
            XR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_apply_plan<METHOD, SRC, KT, SUBS, MERGED, FAST>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
            granted = shmem;
        }
    }
    const int64_t n_groups = div_up(div_up(csr->n, AP_BLOCK), SUBS);
    const int item_tiles = 64 / KT;
    const int super_blocks = K > (int64_t)KT * item_tiles ? (int)std::min<int64_t>((n_groups + 7) / 8, 1 << 30) : 0;
    int64_t plan_grid = (n_groups + 7) / 8 * 8;
    if (super_blocks > 0) {
        const int64_t per_xcd = (n_groups + 7) / 8;
        const int64_t n_items = div_up(K, (int64_t)KT * item_tiles);
        plan_grid = 8 * div_up(per_xcd, super_blocks) * super_blocks * n_items;
    }
    XR_LAUNCH("apply_plan", (k_apply_plan<METHOD, SRC, KT, SUBS, MERGED, FAST>), dim3((unsigned)plan_grid), dim3(AP_BLOCK * SUBS),
              shmem, csr->indptr.get(), csr->indices.get(), csr->data.get(), csr->plan_ucol.get(), csr->plan_nuniq.get(),
              csr->plan_loc.get(), row_order_of(csr), csr->has_long, csr->n, csr->m, src, K, out, csr->plan_lmax, super_blocks,
              item_tiles, plan_dbg);
}

template <int METHOD, typename SRC>
static void launch_stream(const xr_csr *csr, const SRC *src, int64_t K, double *out, const ApplyContext *ctx) {
    // (enqueued behind a weight build whose sizes the host has not read yet: the context's flags, not the matrix')
    const bool has_long = ctx ? ctx->has_long : csr->has_long;
    const int64_t max_row_len = ctx ? ctx->max_row_len : csr->max_row_len;
    // The long rows (hull slivers: a few hundred latency-bound rows).  With many variables they run on the side stream BESIDE
    // the short ones -- disjoint output rows (0.25 ms of the 1.9 ms at K = 256).  For one variable the fork / join events
    // cost more than the 30 us they could hide (0.069 -> 0.075 ms): there they follow apply_stream in line, which also
    // zeroes their queue counter (no memset launch), and the block-per-row kernel is skipped when the builder reported
    // that no row exceeds the wave kernel's reach.
    DevBuf<int32_t> huge;
    if (has_long) huge.alloc((size_t)(csr->nnz / APPLY_WAVE + 2));
    auto launch_long_rows = [&](bool zeroed) {
        if (!zeroed) XR_HIP(hipMemsetAsync(huge.get(), 0, sizeof(int32_t), launch_stream()));
        if (K == 1) {
            // rows of APPLY_LONG + 1 ... APPLY_WAVE entries: lane groups / waves; a single variable
            dim3 wgrid((unsigned)engine().num_cu * 16, 1);
            XR_LAUNCH("apply_wave", (k_apply_wave<METHOD, SRC, 1>), wgrid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->long_rows.get(), csr->n_long.get(),
                      csr->n, csr->m, src, K, out, huge.get());
        } else {
            // ... 8 variables per pass
            constexpr int WT = 8;
            const unsigned wy = (unsigned)std::min<int64_t>(div_up(K, WT), 8);
            dim3 wgrid((unsigned)engine().num_cu * 16 / wy, wy);
            XR_LAUNCH("apply_wave", (k_apply_wave<METHOD, SRC, WT>), wgrid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->long_rows.get(), csr->n_long.get(),
                      csr->n, csr->m, src, K, out, huge.get());
        }
        if (max_row_len >= 0 && max_row_len <= APPLY_WAVE) return; // no row for the block kernel
        // rows beyond APPLY_WAVE entries, as queued by the wave kernel: one block each
        const unsigned gy = (unsigned)(K < 8 ? K : 8);
        dim3 grid((unsigned)engine().num_cu * (8 / gy), gy); // 8 blocks per CU; blocks past the count exit at once
        XR_LAUNCH("apply_long", (k_apply_long<METHOD, SRC>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                  csr->indices.get(), csr->data.get(), row_order_of(csr), huge.get() + 1, huge.get(),
                  csr->n, csr->m, src, K, out);
    };
    const bool long_on_side = has_long && K >= PLAN_KT;
    const bool use_plan = K > 1 && K >= PLAN_KT && option(OPT_APPLY_PLAN) != 0; // (measurement / test switch)
    if (use_plan) { // (built once per matrix, on the main stream, in front of the fork)
        ensure_tiled(csr);
        ensure_plan(csr);
    }
    // the few blocks the plan could not take (hull slivers: too many entries or distinct columns): direct gathers, parallel
    // over the variable tiles as well so that no thread walks a long row K / 8 times (tiles of 4 variables: these blocks hold
    // rows of up to 256 entries that one thread walks alone).  Beside the planned blocks when the side stream is in use
    // anyway (disjoint output rows; in line they were 0.07 ms behind the 1.5 ms of a K = 256 apply).
    auto launch_unplanned = [&]() {
        if (csr->plan_n_unplanned <= 0) return;
        dim3 grid((unsigned)csr->plan_n_unplanned, div_up(K, 4));
        XR_LAUNCH("apply_direct", (k_apply_direct<METHOD, SRC, 4>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                  csr->indices.get(), csr->data.get(), row_order_of(csr), has_long, csr->n, csr->m, src, K, out,
                  csr->plan_unplanned.get());
    };
    // with a plan the side work is launched BEHIND the plan kernel but depends only on what precedes it (side_mark): the host
    // reaches the long kernel's launch first, the three short side launches follow while it runs
    const bool side_late = long_on_side && use_plan && side_mark();
    if (long_on_side && !side_late) {
        SideScope side;
        launch_long_rows(false);
        if (use_plan) launch_unplanned();
    }
    if (K == 1) {
        // one launch: long-row blocks in front, then one wave per 64 stored rows
        const int n_long_blocks = has_long ? engine().num_cu / 2 : 0;
        const bool any_huge = has_long && !(max_row_len >= 0 && max_row_len <= APPLY_WAVE);
        dim3 grid((unsigned)(div_up(csr->n, AP_BLOCK) + n_long_blocks), 1);
        if (ctx && ctx->tail) {
            // enqueued by the fused weight build in front of its place_big: this launch places the big rows itself
            XR_REQUIRE(ctx->gate && n_long_blocks > 0 && row_order_of(csr) == csr->row_order.get() && !csr->has_col_perm,
                       XR_ERR_INVALID, "xr_apply: the tail of a weight build needs its fresh matrix");
            grid.x += TAIL_PLACE_BLOCKS;
            XR_LAUNCH("apply_rows1", (k_apply_tail1<METHOD, SRC>), grid, dim3(AP_BLOCK), 0, *ctx->tail, csr->long_rows.get(),
                      n_long_blocks, csr->n, csr->m, src, out);
        } else {
            XR_LAUNCH("apply_rows1", (k_apply_rows1<METHOD, SRC>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(), csr->indices.get(),
                      csr->data.get(), row_order_of(csr), csr->long_rows.get(), csr->n_long.get(), n_long_blocks, any_huge,
                      csr->n, csr->m, src, out, ctx ? ctx->gate : (const int32_t *)nullptr);
        }
    } else {
        if (use_plan) {
            // many variables: rows regrouped into 2-D tiles, then a blocked CSR with per-block distinct-column
            // lists (both built once per matrix, above)
            // contracted products + one reciprocal per row (k_apply_plan, FAST): opt-in
            constexpr bool FAST_OK = METHOD == XR_MEAN || METHOD == XR_FIRST_ORDER_CONSERVATIVE;
            const bool fast = FAST_OK && option(OPT_APPLY_CONTRACT) != 0;
            if (csr->plan_merged && fast) launch_plan<METHOD, SRC, 4, PLAN_GROUP, true, FAST_OK>(csr, src, K, out);
            else if (csr->plan_merged) launch_plan<METHOD, SRC, 4, PLAN_GROUP, true, false>(csr, src, K, out);
            else if (fast) launch_plan<METHOD, SRC, PLAN_KT, 1, false, FAST_OK>(csr, src, K, out);
            else launch_plan<METHOD, SRC, PLAN_KT, 1, false, false>(csr, src, K, out);
            if (side_late) {
                SideScope side(true);
                launch_long_rows(false);
                launch_unplanned();
            } else if (!long_on_side) {
                launch_unplanned();
            }
        } else {
            // a few variables: register-resident k-tiles, direct gathers, no LDS
            dim3 grid(div_up(csr->n, AP_BLOCK), div_up(K, KT));
            XR_LAUNCH("apply_direct", (k_apply_direct<METHOD, SRC, KT>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), has_long, csr->n, csr->m, src, K,
                      out, (const int32_t *)nullptr);
        }
    }
    if (has_long && K > 1 && !long_on_side) launch_long_rows(false); // (a few variables: in line, behind the short rows)
    if (long_on_side) side_join();
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
                  ws.get(), out, csr->has_long);
    }
    if (csr->has_long) {
        // rows of APPLY_LONG + 1 ... APPLY_WAVE entries: sorted in LDS by one wave per (row, variable)
        const unsigned gy = (unsigned)std::min<int64_t>(K, 16);
        dim3 grid((unsigned)engine().num_cu * 32 / gy, gy);
        XR_LAUNCH("apply_sorted", (k_apply_sorted<METHOD, SRC>), grid, dim3(64), 0, csr->indptr.get(), csr->indices.get(),
                  csr->data.get(), row_order_of(csr), csr->long_rows.get(), csr->n_long.get(), csr->n, csr->m, src, K, p,
                  out);
    }
}

template <typename SRC>
static void apply_dispatch(const xr_csr *csr, int method, double p, const SRC *src, int64_t K, double *out, const ApplyContext *ctx) {
    if (csr->n == 0 || K == 0) return;
    // (Until round 4 many variables were walked in host-side groups of 128; since round 5 the many-variable kernel orders its
    // own work by groups of 64 variables -- k_apply_plan, L2-blocked order.)
    with_reducer(method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        if constexpr (streamed_reducer<METHOD>) {
            launch_stream<METHOD, SRC>(csr, src, K, out, ctx);
        } else {
            XR_REQUIRE(!ctx, XR_ERR_INVALID, "internal: a gated apply is a streaming reducer");
            if (METHOD == XR_PERCENTILE)
                XR_REQUIRE(p >= 0.0 && p <= 100.0, XR_ERR_INVALID,
                           "percentile must be in the range [0, 100], received: %g", p);
            launch_workspace<METHOD, SRC>(csr, src, K, p, out);
        }
    });
}

static void apply_dev(const xr_csr *csr, int method, double p, const void *src, int dtype, int64_t K, double *out,
                      const ApplyContext *ctx = nullptr) {
    with_source_type(dtype, [&](auto tag) {
        using SRC = decltype(tag);
        DevBuf<char> permuted; // (goes back to the pool at return; the pool hands blocks out in stream order)
        apply_dispatch<SRC>(csr, method, p, stored_source(csr, static_cast<const SRC *>(src), K, permuted), K, out, ctx);
    });
}

void csr_apply_dev(const xr_csr *csr, int method, double percentile, const void *src_dev, int dtype, int64_t K, double *out_dev,
                   const ApplyContext *ctx) {
    apply_dev(csr, method, percentile, src_dev, dtype, K, out_dev, ctx);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_apply_csr_dev(const xr_csr *csr, int method, double percentile, const void *source_dev, int source_dtype,
                     int64_t K, double *out_dev) {
    {
        const int rc = prepare_for_apply(csr, K);
        if (rc != XR_OK) return rc;
    }
    XR_API_BEGIN_SHARED
    XR_REQUIRE(csr && (source_dev || csr->m == 0 || K == 0) && (out_dev || csr->n == 0 || K == 0), XR_ERR_INVALID,
               "xr_apply_csr_dev: NULL argument");
    XR_REQUIRE(K >= 0, XR_ERR_INVALID, "xr_apply_csr_dev: negative K");
    apply_dev(csr, method, percentile, source_dev, source_dtype, K, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_apply_csr(const xr_csr *csr, int method, double percentile, const void *source, int source_dtype, int64_t K,
                 double *out) {
    {
        const int rc = prepare_for_apply(csr, K);
        if (rc != XR_OK) return rc;
    }
    XR_API_BEGIN_SHARED
    XR_REQUIRE(csr && (source || csr->m == 0 || K == 0) && (out || csr->n == 0 || K == 0), XR_ERR_INVALID,
               "xr_apply_csr: NULL argument");
    XR_REQUIRE(K >= 0, XR_ERR_INVALID, "xr_apply_csr: negative K");
    const size_t esz = source_size(source_dtype);
    staged_chunks(K, csr->m, esz, csr->n, [&](int64_t k0, int64_t kc, char *src, double *dst) {
        const size_t n_src = (size_t)kc * (size_t)csr->m, n_out = (size_t)kc * (size_t)csr->n;
        h2d_big(src, static_cast<const char *>(source) + (size_t)k0 * (size_t)csr->m * esz, n_src * esz);
        apply_dev(csr, method, percentile, src, source_dtype, kc, dst);
        if (n_out > 0) d2h_big(out + (size_t)k0 * (size_t)csr->n, dst, n_out * sizeof(double));
    });
    XR_API_END
}

int xr_apply_coo(const int64_t *row, const int64_t *col, int64_t nnz, int64_t T, const void *source, int source_dtype,
                 int64_t K, int64_t S, double *out) {
    XR_API_BEGIN
    XR_REQUIRE(nnz >= 0 && T >= 0 && K >= 0 && S >= 0, XR_ERR_INVALID, "xr_apply_coo: negative sizes");
    const size_t esz = source_size(source_dtype);
    XR_REQUIRE(T < ((int64_t)1 << 31) && S < ((int64_t)1 << 31) && K < 65536, XR_ERR_LIMIT, "xr_apply_coo: too large");
    for (int64_t i = 0; i < nnz; i++)
        XR_REQUIRE(row[i] >= 0 && row[i] < T && col[i] >= 0 && col[i] < S, XR_ERR_INVALID,
                   "xr_apply_coo: entry %lld out of range", (long long)i);
    const size_t n_src = (size_t)K * (size_t)S, n_out = (size_t)K * (size_t)T;
    DevBuf<char> src(n_src * esz);
    DevBuf<double> dst(n_out);
    DevBuf<int32_t> r32((size_t)nnz), c32((size_t)nnz);
    h2d(src.get(), source, n_src * esz);
    upload_narrow(row, nnz, r32.get());
    upload_narrow(col, nnz, c32.get());
    fill_f64(dst.get(), NAN, (int64_t)n_out);
    if (nnz > 0 && K > 0) {
        dim3 grid(div_up(nnz, 256), (unsigned)K);
        with_source_type(source_dtype, [&](auto tag) {
            using SRC = decltype(tag);
            XR_LAUNCH("apply_coo", k_apply_coo<SRC>, grid, dim3(256), 0, r32.get(), c32.get(), nnz, T, S,
                      reinterpret_cast<const SRC *>(src.get()), dst.get());
        });
    }
    if (n_out > 0) {
        XR_HIP(hipMemcpyAsync(out, dst.get(), n_out * sizeof(double), hipMemcpyDeviceToHost, launch_stream()));
    }
    stream_sync();
    XR_API_END
}

} // extern "C"
