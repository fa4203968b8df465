// xr_mesh.h -- what the units of the mesh handle share: xr_mesh.hip (handle, ingest, downloads), xr_mesh_front.hip (statistics,
// preparation), xr_mesh_order.hip (query order, tree index), xr_mesh_derived.hip (centroids, derived quantities and meshes).
#pragma once
#include "xr_objects.h"

namespace xr {

// What a statistics kernel is handed for one launch (MeshStatsBox::begin).  done == nullptr: the kernel stores its blocks'
// partials and k_reduce_stats follows; else its last block reduces them and publishes (stats_tail, xr_mesh_front.hip).
static constexpr int STATS_SHARDS = 64;
struct StatsTail {
    double *partials;     // [nb][8]
    unsigned *done;       // [16 * (1 + STATS_SHARDS)] arrival counters, one per 64-byte line, zero at rest
    double *stats;        // [8] device copy
    double *stats_host;   // [9] pinned: 8 statistics + the sequence word
    double seq;
};

// flat vertex blocks of a polygon mesh: off = exclusive scan of len, xy = the len[r] CCW-normalised vertices of face perm[r]
// (perm == nullptr: r) from the raw mesh (xr_mesh_front.hip)
void ragged_fill(xr_mesh *mesh, const int32_t *perm, const uint8_t *len, DevBuf<int32_t> &off, DevBuf<double> &xy);

} // namespace xr
