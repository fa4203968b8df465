// xr_merge_keys.h -- the arithmetic of the key table of xr_merge.hip that needs no device: the hash of a coordinate pair and
// of a row of ints, the table's capacity, the sort of a short row.  Compiles for the host too (tests/native/merge_keys_main.cpp
// runs it under the sanitizers).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XR_KEYS_FN __host__ __device__ __forceinline__
#else
#define XR_KEYS_FN inline
#endif

namespace xr {

// a 64-bit finaliser (splitmix64): every input bit reaches every output bit
XR_KEYS_FN uint64_t key_mix(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

XR_KEYS_FN uint64_t key_bits(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    return b;
}

// -0.0 == 0.0, so both must land in one chain: v + 0.0 is +0.0 for either zero and v for everything else
XR_KEYS_FN uint32_t key_hash_xy(double x, double y) {
    return (uint32_t)key_mix(key_mix(key_bits(x + 0.0)) ^ key_bits(y + 0.0));
}

XR_KEYS_FN uint32_t key_hash_row(const int32_t *row, int m) {
    uint64_t h = 0;
    for (int k = 0; k < m; k++) h = key_mix(h ^ (uint32_t)row[k]);
    return (uint32_t)h;
}

// Slots of the table for n rows: a power of two STRICTLY greater than n (an empty slot always exists, so every probe sequence
// ends), and at least 2 n unless `smallest` (the test switch merge_table_slack) or unless that would pass 2^31 slots (the
// probe counter and the slot mask are 32-bit: n < 2^31 - 1 -> capacity <= 2^31).
XR_KEYS_FN int64_t key_table_capacity(int64_t n, bool smallest) {
    int64_t cap = 1;
    while (cap <= n) cap <<= 1;
    if (!smallest && cap < 2 * n && cap < ((int64_t)1 << 31)) cap <<= 1;
    return cap;
}

// ascending sort of v[0..M) by an odd-even transposition network: M rounds of fixed compare-exchanges, every index a
// compile-time constant once unrolled (the row stays in registers)
template <int M> XR_KEYS_FN void key_sort_row(int32_t (&v)[M]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < M; round++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = round & 1; k + 1 < M; k += 2) {
            const int32_t a = v[k], b = v[k + 1];
            v[k] = a < b ? a : b;
            v[k + 1] = a < b ? b : a;
        }
    }
}

// the same order for a row of any length where it lies (rows wider than the register variants): insertion sort
XR_KEYS_FN void key_sort_row_inplace(int32_t *row, int m) {
    for (int k = 1; k < m; k++) {
        const int32_t x = row[k];
        int j = k - 1;
        for (; j >= 0 && row[j] > x; j--) row[j + 1] = row[j];
        row[j + 1] = x;
    }
}

} // namespace xr
