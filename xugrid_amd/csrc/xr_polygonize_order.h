// xr_polygonize_order.h -- the one host step of xr_polygonize.hip: putting the rings of every polygon in canonical order.
// Plain C++ over the ring table alone (one record per RING: polygon, sign of the shoelace sum, segments), no HIP: the same
// function is compiled into a stand-alone program for the host sanitizers (tests/native/polygonize_order_main.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace xr {

// Rings come in ascending order of their leader (the half-edge of smallest (face, slot)), ring r with poly[r] in [0, n_polygon),
// sign[r] the sign of its shoelace sum and len[r] >= 1 segments.  Canonical order: by polygon; within a polygon the ring of
// positive sign first, then the others ascending by leader -- a stable counting sort, O(n_ring + n_polygon).
//   new_pos[r]                   place of ring r in that order
//   ring_offsets[n_ring + 1]     vertex offsets of the ordered rings, closed: a ring of k segments takes k + 1 vertices
//   polygon_offsets[n_polygon+1] ring offsets of the polygons
// -> 0, or 1 + the first polygon that has other than exactly one ring of positive sign, or -1 - r for a ring r whose polygon
// or length is out of range; the outputs are unspecified then.
inline int64_t polygonize_order_rings(int64_t n_ring, int64_t n_polygon, const int32_t *poly, const int32_t *sign,
                                      const int32_t *len, int32_t *new_pos, int64_t *ring_offsets, int64_t *polygon_offsets) {
    std::vector<int64_t> count((size_t)n_polygon + 1, 0), positive((size_t)n_polygon + 1, 0);
    for (int64_t r = 0; r < n_ring; r++) {
        if (poly[r] < 0 || poly[r] >= n_polygon || len[r] < 1) return -1 - r;
        count[(size_t)poly[r]]++;
        positive[(size_t)poly[r]] += sign[r] > 0;
    }
    polygon_offsets[0] = 0;
    for (int64_t p = 0; p < n_polygon; p++) {
        if (positive[(size_t)p] != 1) return 1 + p;
        polygon_offsets[p + 1] = polygon_offsets[p] + count[(size_t)p];
    }
    // (exactly one positive ring per polygon: its count - 1 others fill the places behind the first)
    std::vector<int64_t> &cursor = count;
    for (int64_t p = 0; p < n_polygon; p++) cursor[(size_t)p] = polygon_offsets[p] + 1;
    for (int64_t r = 0; r < n_ring; r++) {
        const size_t p = (size_t)poly[r];
        new_pos[r] = (int32_t)(sign[r] > 0 ? polygon_offsets[p] : cursor[p]++);
    }
    for (int64_t r = 0; r < n_ring; r++) ring_offsets[new_pos[r] + 1] = (int64_t)len[r] + 1;
    ring_offsets[0] = 0;
    for (int64_t r = 0; r < n_ring; r++) ring_offsets[r + 1] += ring_offsets[r];
    return 0;
}

} // namespace xr
