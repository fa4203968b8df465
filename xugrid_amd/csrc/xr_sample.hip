// xr_sample.hip -- reading mesh data at points and along lines on the device: the nearest-entity search behind
// Ugrid2d.locate_nearest_node / _edge / _face (xugrid/ugrid/ugridbase.py:1261-1303, ugrid2d.py:1007-1027: a scipy KDTree
// query per facet), the point gather of sel_points (ugridbase.py:1125-1259: obj.isel + where) and the section coordinates of
// intersect_line / intersect_linestring (ugridbase.py:1438-1452, selection_utils.py:27-32).
//
// Nearest: xr_nn is a uniform grid over a fixed set of points (about two per cell) that keeps its OWN copy of the coordinates
// in cell order next to the caller's ids, so a query that walks a cell reads consecutive 16-byte pairs.  One lane per query
// walks rings of cells around the query's cell (exact f64 squared distances, strictly below max_distance, lowest id among
// equidistant points).  From NN_SORT_MIN_QUERIES queries on the queries are first binned by index cell (counting sort) and
// searched in that order: neighbouring lanes then walk the same cells.  The answers do not depend on either order.  The
// nearest fill (xr_fill.hip) is the second caller: it indexes the valid points of a slice and looks up the null ones, both
// picked by the slice's values (xr_nn.h).
#include <algorithm>
#include <cmath>
#include <vector>

#include "xr_nn.h"
#include "xr_prims.h"

namespace xr {

static constexpr int SB = 256; // threads per block

// Queries from which on the search runs in index-cell order (option nn_query_sort = -1; 0 / 1 force caller / cell order).
// MI355X, 1M-face Delaunay mesh of bench.py, face index, uniformly random queries over the node bounds, whole call, median
// of 20 (profiles/sample_run.py, "query_sweep"), ms in caller order / in cell order:
//    16 000: 0.042 / 0.058    64 000: 0.054 / 0.069    256 000: 0.078 / 0.093    384 000: 0.110 / 0.107
//   512 000: 0.150 / 0.120   768 000: 0.200 / 0.161  1 000 000: 0.262 / 0.189
// The two extra launches and the scan of the sort cost ~0.015 ms whatever the size; the search gains more than that from
// about 384 000 queries on (even there, a fifth faster at 512 000), so the constant sits at the first size the sort clearly wins.
static constexpr int64_t NN_SORT_MIN_QUERIES = 1 << 19;

// the subset a pass works on: every point without `values`, else the points whose value is NaN (want_nan) or is not
__device__ __forceinline__ bool sp_takes_part(const double *__restrict__ values, bool want_nan, int64_t i) {
    return !values || (values[i] != values[i]) == want_nan;
}

// per block: the bounding box of its points that take part and their number -> partial[b * 5 ..] = xmin, xmax, ymin, ymax,
// count (NaN coordinates are passed over by the box and counted).  The count of a WAVE is a ballot, so the block reduction is
// taken in its two steps: the kernel lives on its cross-lane operations (12.4 us for 1M points with the four box values, 15.1 us
// with a fifth value in the butterfly).
__global__ void __launch_bounds__(SB)
k_sp_bbox(const double2 *__restrict__ xy, const double *__restrict__ values, int64_t n, double *__restrict__ partial) {
    __shared__ double lds[5 * (SB / 64)];
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    const bool mine = i < n && sp_takes_part(values, false, i);
    if (mine) {
        const double2 p = xy[i];
        x0 = fmin(x0, p.x), x1 = fmax(x1, p.x), y0 = fmin(y0, p.y), y1 = fmax(y1, p.y);
    }
    double v[5] = {wave_reduce<OpMin>(x0), wave_reduce<OpMax>(x1), wave_reduce<OpMin>(y0), wave_reduce<OpMax>(y1),
                   (double)__popcll(__ballot(mine))};
    block_fold_waves<false, SB, OpMin, OpMax, OpMin, OpMax, OpSum>(lds, v);
    if (threadIdx.x == 0)
        for (int u = 0; u < 5; u++) partial[(int64_t)blockIdx.x * 5 + u] = v[u];
}

// counting sort by grid cell of the points that take part, used for the indexed points and for the queries alike: histogram,
// scan, scatter
__global__ void __launch_bounds__(SB)
k_sp_count(const double2 *__restrict__ xy, const double *__restrict__ values, bool want_nan, int64_t n, SampleGrid g,
           int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i < n && sp_takes_part(values, want_nan, i)) atomicAdd(&count[sp_cell(g, xy[i])], 1);
}

// id_out[position] = point; xy_out (index build only): the point's coordinates beside it.  The order inside a cell is the
// order in which the lanes arrive; no answer depends on it (the search compares ids on equal distances).
__global__ void __launch_bounds__(SB)
k_sp_scatter(const double2 *__restrict__ xy, const double *__restrict__ values, bool want_nan, int64_t n, SampleGrid g,
             const int32_t *__restrict__ start, int32_t *__restrict__ cursor, double2 *__restrict__ xy_out,
             int32_t *__restrict__ id_out) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i >= n || !sp_takes_part(values, want_nan, i)) return;
    const double2 p = xy[i];
    const int64_t c = sp_cell(g, p);
    const int32_t pos = start[c] + atomicAdd(&cursor[c], 1);
    if (xy_out) xy_out[pos] = p;
    id_out[pos] = (int32_t)i;
}

// One lane per query (lane i serves query order[i], or i without an order): rings of cells around the query's cell.  After
// ring R every indexed point within the block of cells [cx - R, cx + R] x [cy - R, cy + R] has been seen; an unseen point is at
// least as far as the nearest side of that block.  The inner loop reads the cell's coordinates in storage order and touches
// the ids only for a candidate that ties or beats the best so far.
__global__ void __launch_bounds__(SB)
k_sp_search(const double2 *__restrict__ pxy, const int32_t *__restrict__ pid, const int32_t *__restrict__ start, SampleGrid g,
            const double2 *__restrict__ qxy, const int32_t *__restrict__ order, int64_t n_query, double md2, double max_distance,
            int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i >= n_query) return;
    const int64_t q = order ? order[i] : i;
    const double2 p = qxy[q];
    if (p.x != p.x || p.y != p.y) {
        out[q] = -1;
        return;
    }
    const int cx = sp_cell_x(g, p.x), cy = sp_cell_y(g, p.y);
    const int rmax = max(g.nx, g.ny);
    double best = INFINITY;
    int32_t bj = -1;
    for (int R = 0; R <= rmax; R++) {
        const int ylo = cy - R, yhi = cy + R, xlo = cx - R, xhi = cx + R;
        for (int yy = max(ylo, 0); yy <= min(yhi, g.ny - 1); yy++) {
            const bool edge_row = yy == ylo || yy == yhi;
            // the ring's cells of this row: all of it on the two edge rows (one run of storage), its two ends elsewhere
            if (edge_row) {
                const int64_t c0 = (int64_t)yy * g.nx + max(xlo, 0), c1 = (int64_t)yy * g.nx + min(xhi, g.nx - 1);
                for (int e = start[c0]; e < start[c1 + 1]; e++) {
                    const double2 s = pxy[e];
                    const double dx = s.x - p.x, dy = s.y - p.y;
                    const double d2 = dx * dx + dy * dy;
                    if (d2 < md2 && d2 <= best) {
                        const int32_t j = pid[e];
                        if (d2 < best || j < bj) best = d2, bj = j;
                    }
                }
            } else {
                for (int side = 0; side < 2; side++) {
                    const int xx = side ? xhi : xlo;
                    if (xx < 0 || xx >= g.nx) continue;
                    const int64_t c = (int64_t)yy * g.nx + xx;
                    for (int e = start[c]; e < start[c + 1]; e++) {
                        const double2 s = pxy[e];
                        const double dx = s.x - p.x, dy = s.y - p.y;
                        const double d2 = dx * dx + dy * dy;
                        if (d2 < md2 && d2 <= best) {
                            const int32_t j = pid[e];
                            if (d2 < best || j < bj) best = d2, bj = j;
                        }
                    }
                }
            }
        }
        // distance from the query to the outside of the block seen so far
        const double lx = p.x - (g.x0 + (double)(cx - R) * g.h), hx = g.x0 + (double)(cx + R + 1) * g.h - p.x;
        const double ly = p.y - (g.y0 + (double)(cy - R) * g.h), hy = g.y0 + (double)(cy + R + 1) * g.h - p.y;
        const double lb = fmax(0.0, fmin(fmin(lx, hx), fmin(ly, hy)));
        if (lb * lb > best || lb >= max_distance) break;
    }
    out[q] = bj;
}

// flag = 1 if an index lies outside [lo, n): the one validation pass of a gather / section call
__global__ void __launch_bounds__(SB)
k_sp_index_check(const int64_t *__restrict__ index, int64_t count, int64_t lo, int64_t n, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    const bool bad = i < count && (index[i] >= n || index[i] < lo);
    wave_flag(bad, flag);
}

// out[k, p] = index[p] >= 0 ? in[k, index[p]] : fill; slice k = blockIdx.y of this tile
template <typename SRC>
__global__ void __launch_bounds__(SB)
k_sp_gather(const SRC *__restrict__ in, int64_t n, const int64_t *__restrict__ index, int64_t n_point, double fill,
            double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (p >= n_point) return;
    const int64_t k = blockIdx.y, j = index[p];
    out[k * n_point + p] = j >= 0 ? (double)in[k * n + j] : fill;
}

// mid = 0.5 (p0 + p1); s = |mid - start of the piece's segment| + length of the segments in front of it
__global__ void __launch_bounds__(SB)
k_sp_section(const double *__restrict__ pieces, const int64_t *__restrict__ piece_segment, int64_t n_piece,
             const double *__restrict__ segment_xy, const double *__restrict__ cumulative, double *__restrict__ mid_xy,
             double *__restrict__ s) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i >= n_piece) return;
    const double *p = pieces + 4 * i;
    const int64_t seg = piece_segment[i];
    const double mx = 0.5 * (p[0] + p[2]), my = 0.5 * (p[1] + p[3]);
    const double dx = mx - segment_xy[4 * seg], dy = my - segment_xy[4 * seg + 1];
    mid_xy[2 * i] = mx;
    mid_xy[2 * i + 1] = my;
    s[i] = sqrt(dx * dx + dy * dy) + cumulative[seg];
}

} // namespace xr

namespace xr {

static bool index_in_range(const int64_t *index_dev, int64_t count, int64_t lo, int64_t n) {
    if (count == 0) return true;
    DevBuf<int32_t> flag(1);
    fill_i32(flag.get(), 0, 1);
    XR_LAUNCH("sample_index_check", k_sp_index_check, dim3(div_up(count, SB)), dim3(SB), 0, index_dev, count, lo, n, flag.get());
    return read_scalar(flag.get()) == 0;
}

SampleGrid size_grid(const double box[4], int64_t n) {
    SampleGrid g{};
    const bool finite = std::isfinite(box[0]) && std::isfinite(box[1]) && std::isfinite(box[2]) && std::isfinite(box[3]);
    const double w = finite ? std::max(box[1] - box[0], 0.0) : 0.0, ht = finite ? std::max(box[3] - box[2], 0.0) : 0.0;
    const double target = std::max<double>(1.0, (double)n / 2.0);
    double cell = std::sqrt(std::max(w * ht, 0.0) / target);
    if (!(cell > 0.0)) cell = std::max(std::max(w, ht) / target, 0.0);
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    int64_t nx = std::min<int64_t>((int64_t)(w / cell) + 1, 1 << 15), ny = std::min<int64_t>((int64_t)(ht / cell) + 1, 1 << 15);
    while (nx * ny > 4 * n + 16) { // (degenerate boxes)
        cell *= 1.5;
        nx = (int64_t)(w / cell) + 1;
        ny = (int64_t)(ht / cell) + 1;
    }
    g.x0 = finite ? box[0] : 0.0, g.y0 = finite ? box[2] : 0.0, g.h = cell, g.inv_h = 1.0 / cell, g.nx = (int)nx, g.ny = (int)ny;
    return g;
}

NnExtent nn_extent(const double *xy_dev, int64_t n, const double *values_dev) {
    XR_REQUIRE(n < INT32_MAX, XR_ERR_LIMIT, "xr_nn: more than 2^31 points");
    NnExtent ext{{INFINITY, -INFINITY, INFINITY, -INFINITY}, 0};
    if (n <= 0) return ext;
    const unsigned nb = div_up(n, SB);
    TwoStageReduce<SB, double, OpMin, OpMax, OpMin, OpMax, OpSum> box("sample_bbox_final", nb, [&](double *partial) {
        XR_LAUNCH("sample_bbox", k_sp_bbox, dim3(nb), dim3(SB), 0, reinterpret_cast<const double2 *>(xy_dev), values_dev, n, partial);
    });
    double h[5];
    box.read(h);
    std::copy(h, h + 4, ext.box);
    ext.n = (int64_t)h[4];
    return ext;
}

xr_nn *nn_build(const double *xy_dev, int64_t n, const double *values_dev, const NnExtent &extent) {
    XR_REQUIRE(extent.n > 0, XR_ERR_INVALID, "xr_nn: no points to index.");
    const double2 *xy = reinterpret_cast<const double2 *>(xy_dev);
    Building<xr_nn> nn(OnFailure::WaitFirst);
    const unsigned nb = div_up(n, SB);
    nn->n = extent.n;
    nn->grid = size_grid(extent.box, extent.n);
    const int64_t nc = nn->n_cell();
    DevBuf<int32_t> count_cursor(2 * (size_t)nc);
    nn->start.alloc((size_t)nc + 1);
    nn->xy.alloc((size_t)extent.n);
    nn->id.alloc((size_t)extent.n);
    fill_i32(count_cursor.get(), 0, 2 * nc);
    XR_LAUNCH("sample_count", k_sp_count, dim3(nb), dim3(SB), 0, xy, values_dev, false, n, nn->grid, count_cursor.get());
    exclusive_scan_i32(count_cursor.get(), nn->start.get(), nc);
    XR_LAUNCH("sample_scatter", k_sp_scatter, dim3(nb), dim3(SB), 0, xy, values_dev, false, n, nn->grid, nn->start.get(),
              count_cursor.get() + nc, nn->xy.get(), nn->id.get());
    return nn.release();
}

void nn_query(const xr_nn *nn, const double *query_xy_dev, int64_t n_query, double max_distance, int64_t *out_dev,
              const double *values_dev, int64_t n_lookup) {
    const double2 *qxy = reinterpret_cast<const double2 *>(query_xy_dev);
    const unsigned nb = div_up(n_query, SB);
    const int64_t mode = option(OPT_NN_QUERY_SORT);
    const bool sorted = values_dev || mode > 0 || (mode < 0 && n_query >= NN_SORT_MIN_QUERIES); // (a subset is served as a list)
    const int64_t n_search = values_dev ? n_lookup : n_query;
    if (n_search <= 0) return;
    DevBuf<int32_t> order;
    if (sorted) {
        const int64_t nc = nn->n_cell();
        DevBuf<int32_t> count_cursor(2 * (size_t)nc), qstart((size_t)nc + 1);
        order.alloc((size_t)n_search);
        fill_i32(count_cursor.get(), 0, 2 * nc);
        XR_LAUNCH("sample_query_count", k_sp_count, dim3(nb), dim3(SB), 0, qxy, values_dev, true, n_query, nn->grid,
                  count_cursor.get());
        exclusive_scan_i32(count_cursor.get(), qstart.get(), nc);
        XR_LAUNCH("sample_query_scatter", k_sp_scatter, dim3(nb), dim3(SB), 0, qxy, values_dev, true, n_query, nn->grid,
                  qstart.get(), count_cursor.get() + nc, (double2 *)nullptr, order.get());
    }
    const double md2 = std::isinf(max_distance) ? INFINITY : max_distance * max_distance;
    XR_LAUNCH(sorted ? "sample_search_sorted" : "sample_search", k_sp_search, dim3(div_up(n_search, SB)), dim3(SB), 0,
              nn->xy.get(), nn->id.get(), nn->start.get(), nn->grid, qxy, sorted ? order.get() : (const int32_t *)nullptr, n_search,
              md2, max_distance, out_dev);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_nn_create_dev(const double *xy_dev, int64_t n, xr_nn **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (xy_dev || n == 0), XR_ERR_INVALID, "xr_nn_create_dev: NULL argument");
    *out = nn_build(xy_dev, n);
    dev_call_done();
    XR_API_END
}

int xr_nn_create_mesh(xr_mesh *mesh, int facet, xr_nn **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out, XR_ERR_INVALID, "xr_nn_create_mesh: NULL argument");
    XR_REQUIRE(facet == XR_FACET_NODE || facet == XR_FACET_FACE, XR_ERR_INVALID,
               "xr_nn_create_mesh: facet must be XR_FACET_NODE or XR_FACET_FACE");
    if (facet == XR_FACET_NODE) {
        *out = nn_build(mesh->node_xy.get(), mesh->n_node);
    } else {
        XR_REQUIRE(mesh->n_face > 0, XR_ERR_INVALID, "xr_nn: no points to index.");
        const auto c = mesh_centroids_shared(mesh);
        *out = nn_build(c->get(), mesh->n_face);
    }
    stream_sync();
    XR_API_END
}

int xr_nn_info(const xr_nn *index, int64_t *n, int64_t *n_cell) {
    XR_API_BEGIN
    XR_REQUIRE(index, XR_ERR_INVALID, "xr_nn_info: NULL handle");
    if (n) *n = index->n;
    if (n_cell) *n_cell = index->n_cell();
    XR_API_END
}

int xr_nn_destroy(xr_nn *index) {
    XR_API_BEGIN
    if (index) {
        release_point();
        delete index;
    }
    XR_API_END
}

int xr_nn_query_dev(const xr_nn *index, const double *query_xy_dev, int64_t n_query, double max_distance, int64_t *index_out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(index, XR_ERR_INVALID, "xr_nn_query_dev: NULL handle");
    XR_REQUIRE(n_query >= 0 && n_query < INT32_MAX, XR_ERR_LIMIT, "xr_nn_query_dev: n_query must be in [0, 2^31)");
    XR_REQUIRE((query_xy_dev && index_out_dev) || n_query == 0, XR_ERR_INVALID, "xr_nn_query_dev: NULL argument");
    XR_REQUIRE(max_distance >= 0.0, XR_ERR_INVALID, "xr_nn_query_dev: max_distance must be non-negative");
    if (n_query > 0) nn_query(index, query_xy_dev, n_query, max_distance, index_out_dev);
    dev_call_done();
    XR_API_END
}

int xr_gather_points_dev(const void *in_dev, int dtype, int64_t K, int64_t n, const int64_t *index_dev, int64_t n_point,
                         double fill_value, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(K >= 0 && n >= 0 && n_point >= 0, XR_ERR_INVALID, "xr_gather_points_dev: negative size");
    XR_REQUIRE((in_dev || n == 0 || K == 0) && ((index_dev && out_dev) || n_point == 0 || K == 0), XR_ERR_INVALID,
               "xr_gather_points_dev: NULL argument");
    if (K > 0 && n_point > 0) {
        XR_REQUIRE(index_in_range(index_dev, n_point, INT64_MIN, n), XR_ERR_INVALID,
                   "xr_gather_points_dev: index out of range (the data has %lld entries)", (long long)n);
        with_source_type(dtype, [&](auto tag) {
            using SRC = decltype(tag);
            const SRC *in = static_cast<const SRC *>(in_dev);
            for (int64_t k0 = 0; k0 < K; k0 += 65535) { // (slices on gridDim.y)
                const int64_t cnt = std::min<int64_t>(65535, K - k0);
                XR_LAUNCH("sample_gather", k_sp_gather<SRC>, dim3(div_up(n_point, SB), (unsigned)cnt), dim3(SB), 0, in + k0 * n, n,
                          index_dev, n_point, fill_value, out_dev + k0 * n_point);
            }
        });
    } else {
        with_source_type(dtype, [](auto) {});
    }
    dev_call_done();
    XR_API_END
}

int xr_section_coords_dev(const double *pieces_dev, const int64_t *piece_segment_dev, int64_t n_piece, const double *segment_xy_dev,
                          int64_t n_segment, double *mid_xy_out_dev, double *s_out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(n_piece >= 0 && n_segment >= 0, XR_ERR_INVALID, "xr_section_coords_dev: negative size");
    XR_REQUIRE((pieces_dev && piece_segment_dev && mid_xy_out_dev && s_out_dev) || n_piece == 0, XR_ERR_INVALID,
               "xr_section_coords_dev: NULL argument");
    XR_REQUIRE(segment_xy_dev || n_segment == 0, XR_ERR_INVALID, "xr_section_coords_dev: NULL argument");
    if (n_piece > 0) {
        XR_REQUIRE(index_in_range(piece_segment_dev, n_piece, 0, n_segment), XR_ERR_INVALID,
                   "xr_section_coords_dev: piece_segment out of range (the line has %lld segments)", (long long)n_segment);
        // exclusive prefix sum of the segments' lengths, on the host: a line has a few segments
        std::vector<double> seg((size_t)n_segment * 4), cumulative((size_t)n_segment);
        d2h(seg.data(), segment_xy_dev, sizeof(double) * seg.size());
        double total = 0.0;
        for (int64_t i = 0; i < n_segment; i++) {
            cumulative[(size_t)i] = total;
            const double dx = seg[4 * i + 2] - seg[4 * i], dy = seg[4 * i + 3] - seg[4 * i + 1];
            total += std::sqrt(dx * dx + dy * dy);
        }
        DevBuf<double> cum_dev((size_t)n_segment);
        h2d(cum_dev.get(), cumulative.data(), sizeof(double) * cumulative.size());
        XR_LAUNCH("sample_section", k_sp_section, dim3(div_up(n_piece, SB)), dim3(SB), 0, pieces_dev, piece_segment_dev, n_piece,
                  segment_xy_dev, cum_dev.get(), mid_xy_out_dev, s_out_dev);
    }
    dev_call_done();
    XR_API_END
}

} // extern "C"
