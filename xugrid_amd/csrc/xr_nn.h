// xr_nn.h -- the exact nearest-point search on a uniform grid (built and queried in xr_sample.hip; read by the handle's entry
// points there and by the nearest fill in xr_fill.hip)
#pragma once
#include "xr_objects.h"

namespace xr {
struct SampleGrid {
    double x0, y0, inv_h, h;
    int nx, ny;
};
} // namespace xr

// Nearest-neighbour index over a fixed set of points (include/xugrid_amd.h)
struct xr_nn {
    int64_t n = 0;             // points indexed
    xr::SampleGrid grid{};
    xr::DevBuf<int32_t> start; // [n_cell + 1]
    xr::DevBuf<double2> xy;    // [n] coordinates in cell order
    xr::DevBuf<int32_t> id;    // [n] caller's id of the point stored at each position
    int64_t n_cell() const { return (int64_t)grid.nx * grid.ny; }
};

namespace xr {

#if defined(__HIPCC__)
// the cell of a coordinate: the one rule behind the index's build, its queries and every kernel that walks its cells
// (comparisons written so that a NaN coordinate lands in cell 0)
__device__ __forceinline__ int sp_cell_x(const SampleGrid &g, double x) {
    const double t = (x - g.x0) * g.inv_h;
    return !(t >= 0.0) ? 0 : t >= (double)(g.nx - 1) ? g.nx - 1 : (int)t;
}
__device__ __forceinline__ int sp_cell_y(const SampleGrid &g, double y) {
    const double t = (y - g.y0) * g.inv_h;
    return !(t >= 0.0) ? 0 : t >= (double)(g.ny - 1) ? g.ny - 1 : (int)t;
}
__device__ __forceinline__ int64_t sp_cell(const SampleGrid &g, double2 p) {
    return (int64_t)sp_cell_y(g, p.y) * g.nx + sp_cell_x(g, p.x);
}
#endif

// What a build indexes: the bounding box (xmin, xmax, ymin, ymax) and the number of the points that take part
struct NnExtent {
    double box[4];
    int64_t n;
};

// cell size for about two points per cell from the box, degenerate boxes included; at most 4 n + 16 cells, 1 << 15 per axis
SampleGrid size_grid(const double box[4], int64_t n);

// values_dev (optional, [n]) selects a subset in all three: a point whose value is NaN is not indexed, and only points whose
// value is NaN are looked up.  Ids stay positions in the caller's arrays either way.
NnExtent nn_extent(const double *xy_dev, int64_t n, const double *values_dev = nullptr);
xr_nn *nn_build(const double *xy_dev, int64_t n, const double *values_dev, const NnExtent &extent);
inline xr_nn *nn_build(const double *xy_dev, int64_t n) { return nn_build(xy_dev, n, nullptr, nn_extent(xy_dev, n)); }
// out_dev[q] = id of the indexed point nearest to query q strictly below max_distance, or -1.  With values_dev ([n_query])
// only the queries whose value is NaN are served, in index-cell order, and out_dev of the others is left alone; n_lookup is
// their exact number (n_query less the NnExtent::n of the same values).
void nn_query(const xr_nn *nn, const double *query_xy_dev, int64_t n_query, double max_distance, int64_t *out_dev,
              const double *values_dev = nullptr, int64_t n_lookup = 0);

} // namespace xr
