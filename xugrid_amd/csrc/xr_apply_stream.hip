// xr_apply_stream.hip -- the streamed reducers of the sparse apply (every reducer but mode and percentiles): the wave windows
// of K = 1 with the fused weight build's tail, the register tiles of a few variables, the cooperative kernels of the long
// rows, and the launch sequence that places them around the many-variable plan (xr_apply_plan.hip).
//
// Entries of a row are consumed in CSR order by one thread per (row, k-tile), so that results are bit-identical to the
// reference loop on the same CSR (regridder.py:41-67; except exp/log in geometric_mean); the cooperative long-row kernels
// merge strided partial states in a fixed butterfly order (xr_apply.h).
#include "xr_apply.h"
#include "xr_reduce.h"
#include "xr_prims.h"

namespace xr {

static constexpr int DIRECT_KT = 16; // source variables per pass of the direct kernel (k_apply_direct without a plan: 2 <= K < PLAN_KT)

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

template <int METHOD, typename SRC>
static void launch_stream(const xr_csr *csr, const SRC *src, int64_t K, double *out, const ApplyContext *ctx) {
    // (enqueued behind a weight build whose sizes the host has not read yet: the context's flags, not the matrix')
    const bool has_long = ctx ? ctx->has_long : csr->longs.any;
    const int64_t max_row_len = ctx ? ctx->max_row_len : csr->longs.max_row_len;
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
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->longs.rows.get(), csr->longs.n_dev.get(),
                      csr->n, csr->m, src, K, out, huge.get());
        } else {
            // ... 8 variables per pass
            constexpr int WT = 8;
            const unsigned wy = (unsigned)std::min<int64_t>(div_up(K, WT), 8);
            dim3 wgrid((unsigned)engine().num_cu * 16 / wy, wy);
            XR_LAUNCH("apply_wave", (k_apply_wave<METHOD, SRC, WT>), wgrid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), csr->longs.rows.get(), csr->longs.n_dev.get(),
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
        if (csr->plan.n_unplanned <= 0) return;
        dim3 grid((unsigned)csr->plan.n_unplanned, div_up(K, 4));
        XR_LAUNCH("apply_direct", (k_apply_direct<METHOD, SRC, 4>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                  csr->indices.get(), csr->data.get(), row_order_of(csr), has_long, csr->n, csr->m, src, K, out,
                  csr->plan.unplanned.get());
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
            XR_REQUIRE(ctx->gate && n_long_blocks > 0 && row_order_of(csr) == csr->stored.row_order.get() && !csr->cols.permuted,
                       XR_ERR_INVALID, "xr_apply: the tail of a weight build needs its fresh matrix");
            grid.x += TAIL_PLACE_BLOCKS;
            XR_LAUNCH("apply_rows1", (k_apply_tail1<METHOD, SRC>), grid, dim3(AP_BLOCK), 0, *ctx->tail, csr->longs.rows.get(),
                      n_long_blocks, csr->n, csr->m, src, out);
        } else {
            XR_LAUNCH("apply_rows1", (k_apply_rows1<METHOD, SRC>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(), csr->indices.get(),
                      csr->data.get(), row_order_of(csr), csr->longs.rows.get(), csr->longs.n_dev.get(), n_long_blocks, any_huge,
                      csr->n, csr->m, src, out, ctx ? ctx->gate : (const int32_t *)nullptr);
        }
    } else {
        if (use_plan) {
            // many variables: rows regrouped into 2-D tiles, then a blocked CSR with per-block distinct-column
            // lists (both built once per matrix, above)
            apply_planned(csr, METHOD, src, source_dtype<SRC>, K, out);
            if (side_late) {
                SideScope side(true);
                launch_long_rows(false);
                launch_unplanned();
            } else if (!long_on_side) {
                launch_unplanned();
            }
        } else {
            // a few variables: register-resident k-tiles, direct gathers, no LDS
            dim3 grid(div_up(csr->n, AP_BLOCK), div_up(K, DIRECT_KT));
            XR_LAUNCH("apply_direct", (k_apply_direct<METHOD, SRC, DIRECT_KT>), grid, dim3(AP_BLOCK), 0, csr->indptr.get(),
                      csr->indices.get(), csr->data.get(), row_order_of(csr), has_long, csr->n, csr->m, src, K,
                      out, (const int32_t *)nullptr);
        }
    }
    if (has_long && K > 1 && !long_on_side) launch_long_rows(false); // (a few variables: in line, behind the short rows)
    if (long_on_side) side_join();
}

void apply_stream(const xr_csr *csr, int method, const void *src, int dtype, int64_t K, double *out, const ApplyContext *ctx) {
    with_reducer(method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        XR_REQUIRE(streamed_reducer<METHOD>, XR_ERR_INVALID, "internal: reducer %d does not stream over a row", METHOD);
        if constexpr (streamed_reducer<METHOD>)
            with_source_type(dtype, [&](auto tag) {
                using SRC = decltype(tag);
                launch_stream<METHOD, SRC>(csr, static_cast<const SRC *>(src), K, out, ctx);
            });
    });
}

} // namespace xr
