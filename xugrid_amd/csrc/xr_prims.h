// xr_prims.h -- the small device idioms the mesh-operation units share: a per-wave counter and flag, the wave / block scan and the block sort of a row, the int32 -> int64
// widening on the way out of the library, and the compaction behind "flags -> exclusive scan -> ascending ids".  Kernels are
// `static`: every translation unit that includes this header gets its own copy (as in xr_node_faces.h).
#pragma once
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

// inclusive scan of one value per lane of the wave
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// block-wide exclusive scan of one value per thread; returns exclusive prefix, total via *total
template <int BLOCK = 256> __device__ __forceinline__ int block_excl_scan(int v, int *total, int *lds /* >= BLOCK / 64 ints */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = wave_incl_scan(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
        int s = lds[w];
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
