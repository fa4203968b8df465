// xr_mesh_plan.h -- what the host decides from a mesh's eight statistics (stat::Slot, xr_geom.h) before it allocates or launches
// anything: the levels of the tree index, the coarse Morton grid of an ordering, whether the caller's numbering is kept.  Pure
// functions of their arguments, no HIP calls: tests/test_mesh_plan_host.py compiles this header with g++ and table-tests it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "xr_geom.h"

namespace xr {

// The hierarchical grid of the tree index (layout: xr_geom.h) for a mesh of n_face faces.  sampled: the extents come from a
// sample of stats[FACES_SAMPLED] faces; the largest extent is then only bounded by the domain.
// false: the levels together have 2^31 cells or more (g is not to be used).
inline bool index_grid(const double *stats, int64_t n_face, bool sampled, GridParams &g) {
    const int64_t F = n_face;
    const double xmin = stats[stat::XMIN], xmax = stats[stat::XMAX], ymin = stats[stat::YMIN], ymax = stats[stat::YMAX];
    const double n_ext = sampled ? std::max(stats[stat::FACES_SAMPLED], 1.0) : (double)F;
    const double sum_ext = stats[stat::SUM_EXTENT] * ((double)F / n_ext);
    const double max_ext = sampled ? std::max(xmax - xmin, ymax - ymin) : stats[stat::MAX_EXTENT];
    double W = F > 0 ? xmax - xmin : 1.0, H = F > 0 ? ymax - ymin : 1.0;
    if (!(W > 0)) W = 1.0;
    if (!(H > 0)) H = 1.0;
    // level-0 cell size = 1.4 mean bbox extents (measured on the 1M benchmark.  Round 1's search kernel: 0.75 -> 0.168 ms,
    // 1.0 -> 0.155, 1.25 -> 0.137, 1.5 -> 0.134, 2.0 -> 0.144; round 5's, interleaved on one box: 1.25 -> 0.0924,
    // 1.4 -> 0.0898, 1.5 -> 0.0976, 1.6 -> 0.111 -- at 1.5 the second level still holds more than 1/64 of the records, so every
    // face walks it, yet it is too empty to pay for its cell bounds)
    constexpr double h0_factor = 1.4;
    double h0 = F > 0 ? h0_factor * sum_ext / (double)F : 1.0;
    if (!(h0 > 0)) h0 = std::max(W, H);
    // bound the level-0 cell count by ~4 cells per face
    const double max_cells0 = std::max(4.0 * (double)F, 1024.0);
    while ((floor(W / h0) + 1.0) * (floor(H / h0) + 1.0) > max_cells0) h0 *= 2.0;
    g.x0 = F > 0 ? xmin : 0.0;
    g.y0 = F > 0 ? ymin : 0.0;
    g.h0 = h0;
    g.inv_h0 = 1.0 / h0;
    int L = 1;
    while (L < MAX_LEVELS && !(max_ext <= 0.999 * ldexp(h0, (L - 1) * LEVEL_SHIFT))) L++;
    g.n_levels = L;
    int64_t total = 0;
    for (int l = 0; l < L; l++) {
        const double inv_h = ldexp(g.inv_h0, -l * LEVEL_SHIFT);
        const int64_t nx = (int64_t)floor(W * inv_h) + 1, ny = (int64_t)floor(H * inv_h) + 1;
        if (!(total + nx * ny < ((int64_t)1 << 31))) return false;
        g.base[l] = (int)total;
        g.nx[l] = (int)nx;
        g.ny[l] = (int)ny;
        total += nx * ny;
    }
    g.n_cells = (int)total;
    return true;
}

// The coarse Morton grid over a mesh's domain: 2^bits cells a side, the fewest bits in [first_bits, max_bits] with which a cell
// is at most extents_per_cell mean face extents wide (max_bits if none is).  n_side = 2^bits; keys are in [0, n_side^2).
inline MortonParams morton_cover(const double *stats, int64_t n_face, double extents_per_cell, int first_bits, int max_bits) {
    const double xmin = stats[stat::XMIN], xmax = stats[stat::XMAX], ymin = stats[stat::YMIN], ymax = stats[stat::YMAX];
    double span = std::max(xmax - xmin, ymax - ymin);
    if (!(span > 0)) span = 1.0;
    double h = extents_per_cell * stats[stat::SUM_EXTENT] / (double)n_face;
    if (!(h > 0)) h = span;
    int bits = first_bits;
    while (bits < max_bits && ldexp(h, bits) < span) bits++;
    return MortonParams{xmin, ymin, (double)(1 << bits) / (span * (1.0 + 1e-9)), 1 << bits};
}

// Coherent numbering (consecutive faces are, on average, within a few face extents of each other -- typical for mesh
// generators, not for qhull output): the caller's order is kept as the query order.  Needs statistics over ALL faces.
// (a jump is measured between the lanes of a wave: 63 per 64 faces)
inline bool numbering_coherent(const double *stats, int64_t n_face) {
    const int64_t F = n_face;
    const double mean_ext = F > 0 ? stats[stat::SUM_EXTENT] / (double)F : 0.0;
    const double mean_jump = F > 0 ? stats[stat::SUM_JUMP] / ((double)F * 63.0 / 64.0) : 0.0;
    return F == 0 || mean_jump <= 4.0 * mean_ext;
}

} // namespace xr
