// xr_sort_keys.h -- the arithmetic of the radix sort of xr_geometry.hip that needs no device: the order-preserving 64-bit image
// of a double, the digit of a pass and which passes may be skipped.  Compiles for the host too (tests/native/sort_keys_main.cpp
// runs it under the sanitizers).  DESIGN section 24.
#pragma once
#include "xr_merge_keys.h"

namespace xr {

static constexpr int SORT_DIGIT_BITS = 8;                            // one pass sorts by one byte of the key
static constexpr int SORT_BUCKETS = 1 << SORT_DIGIT_BITS;            // 256: one bucket per thread of a block
static constexpr int SORT_PASSES = 2 * 64 / SORT_DIGIT_BITS;         // the key is (image of x, image of y): 128 bits

// a < b as doubles  <=>  image(a) < image(b) as unsigned integers, for everything but NaN; both zeros share the image of +0.0
// (v + 0.0, as in key_hash_xy).  Non-negatives get their sign bit set, negatives all bits flipped.
XR_KEYS_FN uint64_t sort_key_image(double v) {
    const uint64_t b = key_bits(v + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the digit of pass 0 .. SORT_PASSES - 1, least significant first: the bytes of y's image, then those of x's (x decides first)
XR_KEYS_FN unsigned sort_digit(uint64_t key_x, uint64_t key_y, int pass) {
    const int half = SORT_PASSES / 2;
    const uint64_t word = pass < half ? key_y : key_x;
    return (unsigned)((word >> (SORT_DIGIT_BITS * (pass % half))) & (uint64_t)(SORT_BUCKETS - 1));
}

// With `any` the OR and `all` the AND of every key's image, a bit is the same in all keys where the two agree.  Bit p of the
// result: pass p has a digit that differs between some keys and must run; the other passes would move nothing.
XR_KEYS_FN uint32_t sort_pass_mask(uint64_t any_x, uint64_t all_x, uint64_t any_y, uint64_t all_y) {
    const uint64_t vary_x = any_x ^ all_x, vary_y = any_y ^ all_y;
    uint32_t mask = 0;
    for (int pass = 0; pass < SORT_PASSES; pass++)
        if (sort_digit(vary_x, vary_y, pass) != 0) mask |= (uint32_t)1 << pass;
    return mask;
}

} // namespace xr
