// Stand-alone driver of xugrid_amd/csrc/xr_sort_keys.h for the host sanitizers (tests/test_geometry_cpu.py compiles it with
// -fsanitize=address,undefined): the key image, the digit of a pass and the pass mask, and the stable LSD radix sort of
// xr_geometry.hip run sequentially on the host.
// stdin:  k, then k rows "x y" (finite; -0.0 and subnormals allowed).
// stdout: the rows' ids in sorted order (ties in input order); the pass mask in hex; "images ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xugrid_amd/csrc/xr_sort_keys.h"

int main() {
    long long k = 0;
    if (std::scanf("%lld", &k) != 1 || k < 0) return 2;
    std::vector<double> xy((size_t)(2 * k));
    for (auto &v : xy) {
        char word[64];
        if (std::scanf("%63s", word) != 1) return 2;
        v = std::strtod(word, nullptr);
    }
    std::vector<uint64_t> kx((size_t)k), ky((size_t)k);
    uint64_t any_x = 0, all_x = ~0ull, any_y = 0, all_y = ~0ull;
    for (long long i = 0; i < k; i++) {
        kx[(size_t)i] = xr::sort_key_image(xy[(size_t)(2 * i)]), ky[(size_t)i] = xr::sort_key_image(xy[(size_t)(2 * i + 1)]);
        any_x |= kx[(size_t)i], all_x &= kx[(size_t)i], any_y |= ky[(size_t)i], all_y &= ky[(size_t)i];
    }
    // the image keeps the order of the doubles, and both zeros are one key
    for (long long a = 0; a < 2 * k; a++)
        for (long long b = 0; b < 2 * k; b++) {
            const uint64_t ia = xr::sort_key_image(xy[(size_t)a]), ib = xr::sort_key_image(xy[(size_t)b]);
            if ((xy[(size_t)a] < xy[(size_t)b]) != (ia < ib) || (xy[(size_t)a] == xy[(size_t)b]) != (ia == ib)) return 3;
        }
    if (xr::sort_key_image(-0.0) != xr::sort_key_image(0.0)) return 3;

    const uint32_t mask = k > 0 ? xr::sort_pass_mask(any_x, all_x, any_y, all_y) : 0;
    std::vector<int32_t> ids((size_t)k), next((size_t)k);
    for (long long i = 0; i < k; i++) ids[(size_t)i] = (int32_t)i;
    for (int pass = 0; pass < xr::SORT_PASSES; pass++) {
        auto digit = [&](int32_t id) { return xr::sort_digit(kx[(size_t)id], ky[(size_t)id], pass); };
        if (!((mask >> pass) & 1)) { // a skipped pass would have moved nothing: every key has the same digit
            for (int32_t id : ids)
                if (digit(id) != digit(ids[0])) return 4;
            continue;
        }
        std::vector<size_t> start((size_t)xr::SORT_BUCKETS + 1, 0);
        for (int32_t id : ids) start[digit(id) + 1]++;
        for (int d = 0; d < xr::SORT_BUCKETS; d++) start[(size_t)d + 1] += start[(size_t)d];
        for (int32_t id : ids) next[start[digit(id)]++] = id;
        ids.swap(next);
    }
    for (int32_t id : ids) std::printf("%d ", id);
    std::printf("\n%x\nimages ok\n", (unsigned)mask);
    return 0;
}
