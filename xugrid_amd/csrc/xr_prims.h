// xr_prims.h -- the small device idioms the mesh-operation units share: a per-wave counter and flag, the int32 -> int64
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
