// Stand-alone driver of xugrid_amd/csrc/xr_merge_keys.h for the host sanitizers (tests/test_partition_cpu.py compiles it with
// -fsanitize=address,undefined): the row sorts, the two hashes, the table's capacity, and the insert / look-up rule of
// xr_merge.hip run sequentially on the host.
// stdin:  n m, then n rows of m ints; then k, then k rows "x y" (nan and -0.0 allowed).
// stdout: rep[] of the int rows with the smallest and with the default capacity; the same two lines for the coordinate rows;
//         "capacity ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xugrid_amd/csrc/xr_merge_keys.h"

// the device's rule, one row after the other: the slot of a key ends up holding its smallest id
template <typename HASH, typename EQUAL>
static std::vector<int32_t> first_occurrence(int64_t n, bool smallest, HASH hash, EQUAL equal) {
    const int64_t cap = xr::key_table_capacity(n, smallest);
    std::vector<int32_t> table((size_t)cap, -1), rep((size_t)n);
    const uint32_t mask = (uint32_t)(cap - 1);
    for (int64_t i = n - 1; i >= 0; i--) { // (descending: every equal row arrives before the one that must win)
        uint32_t h = hash(i) & mask;
        for (int64_t probe = 0; probe < cap; probe++, h = (h + 1) & mask) {
            int32_t &slot = table[h];
            if (slot < 0) {
                slot = (int32_t)i;
                break;
            }
            if (equal(slot, i)) {
                if ((int32_t)i < slot) slot = (int32_t)i;
                break;
            }
        }
    }
    for (int64_t i = 0; i < n; i++) {
        uint32_t h = hash(i) & mask;
        rep[(size_t)i] = (int32_t)i;
        for (int64_t probe = 0; probe < cap; probe++, h = (h + 1) & mask) {
            const int32_t occ = table[h];
            if (occ < 0) break;
            if (occ == (int32_t)i || equal(occ, i)) {
                rep[(size_t)i] = occ;
                break;
            }
        }
    }
    return rep;
}

static void print(const std::vector<int32_t> &v) {
    for (int32_t x : v) std::printf("%d ", x);
    std::printf("\n");
}

template <int M> static bool network_agrees(const int32_t *row, const int32_t *sorted) {
    int32_t v[M];
    for (int k = 0; k < M; k++) v[k] = row[k];
    xr::key_sort_row(v);
    for (int k = 0; k < M; k++)
        if (v[k] != sorted[k]) return false;
    return true;
}

int main() {
    long long n = 0, m = 0;
    if (std::scanf("%lld %lld", &n, &m) != 2 || n < 0 || m < 1 || m > 8) return 2;
    std::vector<int32_t> rows((size_t)(n * m)), sorted;
    for (auto &v : rows)
        if (std::scanf("%d", &v) != 1) return 2;
    sorted = rows;
    for (long long i = 0; i < n; i++) {
        xr::key_sort_row_inplace(sorted.data() + i * m, (int)m);
        const int32_t *row = rows.data() + i * m, *s = sorted.data() + i * m;
        const bool ok = m == 1 ? network_agrees<1>(row, s) : m == 2 ? network_agrees<2>(row, s) : m == 3 ? network_agrees<3>(row, s)
                      : m == 4 ? network_agrees<4>(row, s) : m == 5 ? network_agrees<5>(row, s) : m == 6 ? network_agrees<6>(row, s)
                      : m == 7 ? network_agrees<7>(row, s) : network_agrees<8>(row, s);
        if (!ok) return 3;
    }
    auto row_hash = [&](int64_t i) { return xr::key_hash_row(sorted.data() + i * m, (int)m); };
    auto row_equal = [&](int64_t a, int64_t b) {
        for (int k = 0; k < m; k++)
            if (sorted[(size_t)(a * m + k)] != sorted[(size_t)(b * m + k)]) return false;
        return true;
    };
    print(first_occurrence(n, true, row_hash, row_equal));
    print(first_occurrence(n, false, row_hash, row_equal));

    long long k = 0;
    if (std::scanf("%lld", &k) != 1 || k < 0) return 2;
    std::vector<double> xy((size_t)(2 * k));
    for (auto &v : xy) {
        char word[64];
        if (std::scanf("%63s", word) != 1) return 2;
        v = std::strtod(word, nullptr);
    }
    auto xy_hash = [&](int64_t i) { return xr::key_hash_xy(xy[(size_t)(2 * i)], xy[(size_t)(2 * i + 1)]); };
    auto xy_equal = [&](int64_t a, int64_t b) {
        return xy[(size_t)(2 * a)] == xy[(size_t)(2 * b)] && xy[(size_t)(2 * a + 1)] == xy[(size_t)(2 * b + 1)];
    };
    print(first_occurrence(k, true, xy_hash, xy_equal));
    print(first_occurrence(k, false, xy_hash, xy_equal));
    if (xr::key_hash_xy(-0.0, 1.0) != xr::key_hash_xy(0.0, 1.0)) return 4; // both zeros in one chain

    for (long long c = 0; c < 70000; c = c < 70 ? c + 1 : c * 3) {
        const int64_t small = xr::key_table_capacity(c, true), usual = xr::key_table_capacity(c, false);
        if (small <= c || (small & (small - 1)) || (c > 0 && small > 2 * c)) return 5;
        if (usual < 2 * c || usual <= c || (usual & (usual - 1))) return 5;
    }
    if (xr::key_table_capacity(2147483646, false) != ((int64_t)1 << 31)) return 5; // (the 32-bit probe counter's limit)
    std::printf("capacity ok\n");
    return 0;
}
