// Stand-alone driver of xugrid_amd/csrc/xr_polygonize_order.h for the host sanitizers (tests/test_polygonize_cpu.py compiles it
// with -fsanitize=address,undefined and runs it on ring tables of the yardstick).
// stdin:  n_ring n_polygon, then n_ring lines "polygon sign segments".
// stdout: the status, then new_pos, ring_offsets and polygon_offsets, one array per line.
#include <cstdio>
#include <vector>

#include "../../xugrid_amd/csrc/xr_polygonize_order.h"

int main() {
    long long n_ring = 0, n_polygon = 0;
    if (std::scanf("%lld %lld", &n_ring, &n_polygon) != 2 || n_ring < 0 || n_polygon < 0) return 2;
    std::vector<int32_t> poly((size_t)n_ring), sign((size_t)n_ring), len((size_t)n_ring), new_pos((size_t)n_ring);
    for (long long r = 0; r < n_ring; r++) {
        int a, b, c;
        if (std::scanf("%d %d %d", &a, &b, &c) != 3) return 2;
        poly[(size_t)r] = a, sign[(size_t)r] = b, len[(size_t)r] = c;
    }
    std::vector<int64_t> ring_offsets((size_t)n_ring + 1), polygon_offsets((size_t)n_polygon + 1);
    const int64_t status = xr::polygonize_order_rings(n_ring, n_polygon, poly.data(), sign.data(), len.data(), new_pos.data(),
                                                      ring_offsets.data(), polygon_offsets.data());
    std::printf("%lld\n", (long long)status);
    if (status != 0) return 0;
    for (int32_t v : new_pos) std::printf("%d ", v);
    std::printf("\n");
    for (int64_t v : ring_offsets) std::printf("%lld ", (long long)v);
    std::printf("\n");
    for (int64_t v : polygon_offsets) std::printf("%lld ", (long long)v);
    std::printf("\n");
    return 0;
}
