// xr_prims.h -- the library's small device idioms, one copy each: a per-wave counter and flag, the per-run counter of a wave,
// the wave / block reduction and the two-launch reduction of an array, the wave / block scan and the block sort of a row, the
// int32 -> int64 widening on the way out of the library, and the compaction behind "flags -> exclusive scan -> ascending ids".
// The regrid units (search, clip, assembly, mesh statistics, apply, locate) use them as the mesh-operation units do.  Kernels
// are `static`: every translation unit that includes this header gets its own copy (as in xr_node_faces.h).
#pragma once
#include <limits>
#include <type_traits>

#include "xr_internal.h"

namespace xr {

// one integer add per wave in which `pred` holds for some lane (every lane of the wave must get here)
__device__ __forceinline__ void wave_count(bool pred, int32_t *counter) {
    const unsigned long long ballot = __ballot(pred);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(counter, __popcll(ballot));
}

// *flag = 1 if `bad` holds for some lane of the wave: one plain store per such wave (every lane of the wave must get here)
__device__ __forceinline__ void wave_flag(bool bad, int32_t *flag) {
    if (__ballot(bad) && (threadIdx.x & 63) == 0) *flag = 1;
}

// counts[key] += the lanes with `pred` among each maximal run of adjacent lanes with equal `key`: one atomic by the run's first
// lane, none for a run without such a lane; lanes with key < 0 take no part (every lane of the wave must get here).  Sorted
// keys -- the pairs of one target face are contiguous in a pair queue -- make that a few atomics per wave.
__device__ __forceinline__ void wave_run_add(int key, bool pred, int32_t *counts) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long surv = __ballot(pred);
    if (head && key >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
        const int next = above ? lane + 1 + (__ffsll((long long)above) - 1) : 64;
        unsigned long long run = next == 64 ? ~0ull : ((1ull << next) - 1);
        run &= ~((1ull << lane) - 1);
        const int n = __popcll(surv & run);
        if (n > 0) atomicAdd(&counts[key], n);
    }
}

// ---- reductions -----------------------------------------------------------------------------------------------------------------
// THE ORDER IS A CONTRACT: results are compared bit for bit, and several callers sum doubles (the dot products of the Laplace
// fill's CG and its mean edge length, the |dy| total that sizes the burn strips, the ring areas of polygonize).
//   1. the 64 lane values of a wave are combined by the xor butterfly over the offsets 32, 16, 8, 4, 2, 1, each step
//      v = op(v, the partner's v);
//   2. the wave results are folded in ascending wave number, starting from wave 0's value: ((w0 op w1) op w2) op w3;
//   3. the second stage of a two-launch reduction: thread t starts from the operator's identity and takes the partials
//      t, t + BLOCK, t + 2 BLOCK, ... in that order; then 1 and 2.
// Changing any of the three changes stored results without failing a test that compares within a tolerance.
//
// An operator: identity<T>() and apply(a, b).  Floating-point minimum and maximum are fmin / fmax (a NaN is passed over; only
// an all-NaN input gives NaN), integer ones are comparisons.  The identity of a floating-point sum is +0.0, so a fold of
// partials never hands on a -0.0.
struct OpMin {
    template <typename T> static constexpr T identity() {
        return std::numeric_limits<T>::has_infinity ? std::numeric_limits<T>::infinity() : std::numeric_limits<T>::max();
    }
    template <typename T> __device__ __forceinline__ static T apply(T a, T b) {
        if constexpr (std::is_floating_point_v<T>) return fmin(a, b);
        else return b < a ? b : a;
    }
};
struct OpMax {
    template <typename T> static constexpr T identity() {
        return std::numeric_limits<T>::has_infinity ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::lowest();
    }
    template <typename T> __device__ __forceinline__ static T apply(T a, T b) {
        if constexpr (std::is_floating_point_v<T>) return fmax(a, b);
        else return b > a ? b : a;
    }
};
struct OpSum {
    template <typename T> static constexpr T identity() { return T(0); }
    template <typename T> __device__ __forceinline__ static T apply(T a, T b) { return a + b; }
};

// step 1 of the order: the value of the whole wave, in every lane (every lane of the wave must get here)
template <typename OP, typename T> __device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = OP::apply(v, __shfl_xor(v, o, 64));
    return v;
}

// step 2: v[u] holds the value of the caller's wave under OPS[u] -> the block's.  ALL = false: in thread 0 only, and no barrier
// behind the read of `lds` (a second call on the same `lds` needs one in front); ALL = true: in every thread, behind a barrier.
// lds: sizeof...(OPS) * BLOCK / 64 values.  Every thread of the block must get here.
template <bool ALL, int BLOCK, typename... OPS, typename T>
__device__ __forceinline__ void block_fold_waves(T *lds, T (&v)[sizeof...(OPS)]) {
    constexpr int W = BLOCK / 64;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int u = 0; u < (int)sizeof...(OPS); u++) lds[u * W + wave] = v[u];
    }
    __syncthreads();
    if (ALL || threadIdx.x == 0) {
        int u = 0;
        auto fold = [&](auto op) {
            T r = lds[u * W];
#pragma unroll
            for (int w = 1; w < W; w++) r = decltype(op)::apply(r, lds[u * W + w]);
            v[u++] = r;
        };
        (fold(OPS()), ...);
    }
    if (ALL) __syncthreads();
}

// steps 1 and 2: one value per thread and operator -> the block's (where, and `lds`: see block_fold_waves)
template <bool ALL, int BLOCK, typename... OPS, typename T>
__device__ __forceinline__ void block_reduce_array(T *lds, T (&v)[sizeof...(OPS)]) {
    int u = 0;
    ((v[u] = wave_reduce<OPS>(v[u]), u++), ...);
    block_fold_waves<ALL, BLOCK, OPS...>(lds, v);
}

// ... of separate variables: block_reduce<256, OpMin, OpMax>(lds, lo, hi).  The results are in thread 0 ...
template <int BLOCK, typename... OPS, typename T, typename... TS> __device__ __forceinline__ void block_reduce(T *lds, TS &...v) {
    static_assert(sizeof...(OPS) == sizeof...(TS) && (std::is_same_v<T, TS> && ...), "one operator per value, one value type");
    T a[] = {v...};
    block_reduce_array<false, BLOCK, OPS...>(lds, a);
    int u = 0;
    ((v = a[u++]), ...);
}
// ... or in every thread
template <int BLOCK, typename... OPS, typename T, typename... TS> __device__ __forceinline__ void block_reduce_all(T *lds, TS &...v) {
    static_assert(sizeof...(OPS) == sizeof...(TS) && (std::is_same_v<T, TS> && ...), "one operator per value, one value type");
    T a[] = {v...};
    block_reduce_array<true, BLOCK, OPS...>(lds, a);
    int u = 0;
    ((v = a[u++]), ...);
}

// step 3 and the block reduction behind it, by one block: record b of `partial` holds one value per operator
template <bool ALL, int BLOCK, typename... OPS, typename T>
__device__ __forceinline__ void block_fold_partials(T *lds, const T *__restrict__ partial, int n_partial, T (&v)[sizeof...(OPS)]) {
    constexpr int N = (int)sizeof...(OPS);
    int u = 0;
    ((v[u++] = OPS::template identity<T>()), ...);
    for (int b = threadIdx.x; b < n_partial; b += BLOCK) {
        const T *p = partial + (int64_t)b * N;
        u = 0;
        ((v[u] = OPS::apply(v[u], p[u]), u++), ...);
    }
    block_reduce_array<ALL, BLOCK, OPS...>(lds, v);
}

// the second launch of a two-launch reduction: one block, out[u] = OPS[u] over value u of the n_partial records
template <int BLOCK, typename T, typename... OPS>
static __global__ void __launch_bounds__(BLOCK) k_fold_partials(const T *__restrict__ partial, int n_partial, T *__restrict__ out) {
    constexpr int N = (int)sizeof...(OPS);
    __shared__ T lds[N * (BLOCK / 64)];
    T v[N];
    block_fold_partials<false, BLOCK, OPS...>(lds, partial, n_partial, v);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int u = 0; u < N; u++) out[u] = v[u];
    }
}

// A two-launch reduction: first_stage(partial) launches the unit's own kernel, whose block b writes record b of n_block
// records; the fold (timed as `fold_name`) leaves the sizeof...(OPS) results behind the records, where result() points.
// read() brings them to the host: one read-back.
template <int BLOCK, typename T, typename... OPS> struct TwoStageReduce {
    static constexpr int N = (int)sizeof...(OPS);
    DevBuf<T> buf;
    unsigned n_block;
    template <typename FIRST>
    TwoStageReduce(const char *fold_name, unsigned n_block, FIRST &&first_stage) : buf((size_t)(n_block + 1) * N), n_block(n_block) {
        first_stage(buf.get());
        XR_LAUNCH(fold_name, (k_fold_partials<BLOCK, T, OPS...>), dim3(1), dim3(BLOCK), 0, buf.get(), (int)n_block, result());
    }
    T *result() { return buf.get() + (size_t)n_block * N; }
    void read(T (&host)[N]) { d2h(host, result(), sizeof(host)); }
};

// ---- scans ----------------------------------------------------------------------------------------------------------------------
// inclusive scan of one value per lane of the wave
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        T t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// block-wide exclusive scan of one value per thread; returns exclusive prefix, total via *total (every thread must get here;
// ends behind a barrier)
template <int BLOCK = 256, typename T = int> __device__ __forceinline__ T block_excl_scan(T v, T *total, T *lds /* >= BLOCK / 64 values */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = wave_incl_scan(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    T woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
        T s = lds[w];
        if (w < wave) woff += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return woff + incl - v;
}

template <typename T> __device__ __forceinline__ void order_pair(T *row, int64_t l, int64_t p) {
    const T a = row[l], b = row[p];
    if (a > b) {
        row[l] = b;
        row[p] = a;
    }
}

// row[0 .. L) ascending, in place in global memory, by the BLOCK threads of one block (every thread must get here; ends behind a
// barrier): a bitonic network in which every comparison puts the smaller key first (the first step of a merge pairs l with its
// mirror image in the run, the others pair l with l + j).  The row is thought padded with +inf to a power of two; a pair whose
// upper element is padding changes nothing and is skipped, so padding never moves.
template <int BLOCK, typename T> __device__ __forceinline__ void block_sort_ascending(T *row, int64_t L) {
    int64_t P = 1;
    while (P < L) P <<= 1;
    for (int64_t k = 2; k <= P; k <<= 1) {
        const int64_t half = k >> 1;
        for (int64_t t = threadIdx.x; t < (P >> 1); t += BLOCK) {
            const int64_t base = (t / half) * k, off = t & (half - 1);
            const int64_t l = base + off, p = base + k - 1 - off;
            if (p < L) order_pair(row, l, p);
        }
        __syncthreads();
        for (int64_t j = half >> 1; j > 0; j >>= 1) {
            for (int64_t t = threadIdx.x; t < (P >> 1); t += BLOCK) {
                const int64_t l = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = l + j;
                if (p < L) order_pair(row, l, p);
            }
            __syncthreads();
        }
    }
}

// out[i] = in[i] - subtract: indices are int32 (flags uint8) in HBM, int64 in the C ABI
template <typename T>
static __global__ void __launch_bounds__(256) k_widen(const T *__restrict__ in, int64_t n, int64_t subtract, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i] - subtract;
}

template <typename T> static void widen_dev(const T *in, int64_t n, int64_t *out_dev, int64_t subtract = 0) {
    if (n > 0) XR_LAUNCH("widen_i32", k_widen<T>, dim3(div_up(n, 256)), dim3(256), 0, in, n, subtract, out_dev);
}

// ... to host memory through `scratch` (at least n words; d2h waits, so one buffer serves a run of downloads)
template <typename T> static void download_wide(const T *dev, int64_t n, int64_t *host, DevBuf<int64_t> &scratch) {
    if (!host || n <= 0) return;
    widen_dev(dev, n, scratch.get());
    d2h(host, scratch.get(), sizeof(int64_t) * (size_t)n);
}

// ids[pos[i]] = i for the flagged i: with pos the exclusive scan of flag, the ascending ids of the ones
template <typename OUT>
static __global__ void __launch_bounds__(256)
k_compact_ids(const int32_t *__restrict__ flag, const int32_t *__restrict__ pos, int64_t n, OUT *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) ids[pos[i]] = (OUT)i;
}

} // namespace xr
