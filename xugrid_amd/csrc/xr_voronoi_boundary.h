// xr_voronoi_boundary.h -- the one host step of xr_voronoi.hip: the cells of the boundary nodes (voronoi.py:59-327).
// Plain C++ over the few KB the device gathered (boundary nodes, their rows of node -> face, the exterior edges), no HIP: the
// same function is compiled into a stand-alone program for the host sanitizers (tests/native/voronoi_boundary_main.cpp).
//
// A LOCAL problem (boundary nodes 0..nb-1, the faces around them, both ascending like their global ids, so every grouping and
// stable sort sees the order it would see globally).  O(boundary) items in a dozen dependent steps (sorts, a scan, a per-cell
// convexity choice): tens of microseconds here; as device kernels each step would be a launch plus a round trip.  The
// arithmetic follows xugrid_amd/voronoi.py (_boundary_records) operation for operation, including numpy's pairwise summation
// in the polygon areas: on a straight boundary the two candidate areas of the convexity choice differ by rounding only.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

namespace xr {

struct VoronoiBoundaryIn {
    int64_t n_face = 0;          // generator points of the mesh: vertex ids [0, n_face)
    int64_t nb = 0, ne = 0;      // boundary nodes, exterior edges
    const int64_t *nodes = nullptr;       // [nb] global ids, ascending
    const int64_t *row_ptr = nullptr;     // [nb + 1] rows of the boundary nodes in faces / face_xy
    const int64_t *faces = nullptr;       // faces around each boundary node, ascending per node
    const double *face_xy = nullptr;      // generator point of every listed face
    const double *node_xy = nullptr;      // [nb * 2] coordinates of the boundary nodes
    const int64_t *edge_lo = nullptr, *edge_hi = nullptr, *edge_face = nullptr; // [ne] exterior edges, lexicographic (lo, hi)
    const double *edge_face_xy = nullptr; // [ne * 2] generator point of every exterior edge's face
    bool add_vertices = true;  // one extra corner per boundary node, between the node's two projections
    bool skip_concave = true;  // the true boundary node replaces that corner only where the cell's area does not shrink
};

struct VoronoiBoundaryOut {
    std::vector<double> extra_xy;  // vertices behind the n_face generator points: kept projections, then one per boundary node
    std::vector<int64_t> cells;    // [n_cell][m] global vertex ids, -1 padded, counter-clockwise
    int64_t n_cell = 0, m = 0;
    std::vector<int64_t> tail;     // source face of every added vertex (-1: the per-node extras)
    std::vector<int64_t> interp;   // [n_extra][2] the two projection vertex ids an extra corner sits between
    int64_t n_record = 0;
    double ms_setup = 0.0, ms_sort = 0.0, ms_cells = 0.0;
};

static constexpr int VORONOI_BOUNDARY_OK = 0;
static constexpr int VORONOI_BOUNDARY_ID_RANGE = 1;    // vertex ids would leave the int32 range
static constexpr int VORONOI_BOUNDARY_CELL_CORNERS = 2; // a cell has more than VORONOI_BOUNDARY_MAX_CORNERS corners (out.m)
static constexpr int64_t VORONOI_BOUNDARY_MAX_CORNERS = 128;

inline double np_pairwise_sum(const double *a, int64_t n) { // numpy's DOUBLE_pairwise_sum for n <= 128
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; i++) res += a[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}

inline int voronoi_boundary_cells(const VoronoiBoundaryIn &in, VoronoiBoundaryOut &out) {
    const auto tk0 = std::chrono::steady_clock::now();
    const int64_t nb = in.nb, ne = in.ne, n_face = in.n_face;
    const bool add_vertices = in.add_vertices, skip_concave = in.skip_concave;
    out = VoronoiBoundaryOut();
    if (ne == 0) return VORONOI_BOUNDARY_OK; // closed surface: nothing to add
    if (!(n_face + 3 * ne < ((int64_t)1 << 31))) return VORONOI_BOUNDARY_ID_RANGE;
    // Vertex ids are GLOBAL from the start (generator point f -> f, kept projection r -> n_face + r, extra corner k ->
    // n_face + n_proj + k): the local renumbering of the numpy restatement only exists to keep its arrays small; every
    // record carries its corner's coordinates, so no vertex table is needed either.  Cell keys are local node ranks
    // (ascending like the global node ids).
    struct Rec {
        int64_t key, id;
        double x, y, angle;
    };
    std::vector<Rec> rec;
    rec.reserve((size_t)in.row_ptr[nb] + 3 * (size_t)ne);
    for (int64_t i = 0; i < nb; i++) // corners that are generator points: nodes shared by several faces ...
        if (in.row_ptr[i + 1] - in.row_ptr[i] > 1)
            for (int64_t r = in.row_ptr[i]; r < in.row_ptr[i + 1]; r++)
                rec.push_back({i, in.faces[r], in.face_xy[2 * r], in.face_xy[2 * r + 1], 0.0});
    for (int64_t i = 0; i < nb; i++) // ... then corner nodes owned by exactly one face
        if (in.row_ptr[i + 1] - in.row_ptr[i] == 1) {
            const int64_t r = in.row_ptr[i];
            rec.push_back({i, in.faces[r], in.face_xy[2 * r], in.face_xy[2 * r + 1], 0.0});
        }
    // projections of the adjacent generator point on every exterior edge
    auto local_node = [&](int64_t g) { return (int64_t)(std::lower_bound(in.nodes, in.nodes + nb, g) - in.nodes); };
    const double *nxy = in.node_xy;
    const double merge_tol = 1.0e-8 * 1.0e-8;
    std::vector<int64_t> e_n0((size_t)ne), e_n1((size_t)ne), kept_rank((size_t)ne, -1);
    std::vector<double> proj_all((size_t)ne * 2);
    int64_t n_proj = 0;
    for (int64_t e = 0; e < ne; e++) {
        e_n0[(size_t)e] = local_node(in.edge_lo[e]);
        e_n1[(size_t)e] = local_node(in.edge_hi[e]);
        const double ax = nxy[2 * e_n0[(size_t)e]], ay = nxy[2 * e_n0[(size_t)e] + 1];
        const double bx = nxy[2 * e_n1[(size_t)e]], by = nxy[2 * e_n1[(size_t)e] + 1];
        const double cx = in.edge_face_xy[2 * e], cy = in.edge_face_xy[2 * e + 1];
        const double vx = bx - ax, vy = by - ay, ux = cx - ax, uy = cy - ay;
        const double sc = (ux * vx + uy * vy) / (vx * vx + vy * vy);
        const double px = ax + sc * vx, py = ay + sc * vy;
        proj_all[2 * (size_t)e] = px;
        proj_all[2 * (size_t)e + 1] = py;
        const double dx = px - cx, dy = py - cy;
        if (std::sqrt(dx * dx + dy * dy) > merge_tol) kept_rank[(size_t)e] = n_proj++;
    }
    const int64_t first_new = n_face + n_proj; // id of the first extra corner
    for (int64_t e = 0; e < ne; e++)
        if (kept_rank[(size_t)e] >= 0) { // both end nodes use the projection
            const int64_t id = n_face + kept_rank[(size_t)e];
            rec.push_back({e_n0[(size_t)e], id, proj_all[2 * (size_t)e], proj_all[2 * (size_t)e + 1], 0.0});
            rec.push_back({e_n1[(size_t)e], id, proj_all[2 * (size_t)e], proj_all[2 * (size_t)e + 1], 0.0});
            out.tail.push_back(in.edge_face[e]);
        }
    // add_vertices: one extra corner per boundary node, between the node's two projections: the (edge, end) records sorted by
    // node id (stable), paired off two by two; the interpolation map refers to the UNFILTERED projection numbering exactly as
    // the reference does
    const int64_t n_extra = add_vertices ? ne : 0; // (2 ne records, two per extra corner)
    std::vector<double> extra_xy((size_t)n_extra * 2), true_corner((size_t)n_extra * 2);
    if (add_vertices) {
        std::vector<int64_t> by_node((size_t)(2 * ne));
        for (int64_t j = 0; j < 2 * ne; j++) by_node[(size_t)j] = j;
        auto flat_node = [&](int64_t j) { return (j & 1) ? e_n1[(size_t)(j >> 1)] : e_n0[(size_t)(j >> 1)]; };
        std::stable_sort(by_node.begin(), by_node.end(), [&](int64_t a, int64_t b) { return flat_node(a) < flat_node(b); });
        out.interp.resize((size_t)n_extra * 2);
        for (int64_t k = 0; k < n_extra; k++) {
            const int64_t p0 = by_node[(size_t)(2 * k)] >> 1, p1 = by_node[(size_t)(2 * k + 1)] >> 1;
            extra_xy[2 * (size_t)k] = 0.5 * (proj_all[2 * (size_t)p0] + proj_all[2 * (size_t)p1]);
            extra_xy[2 * (size_t)k + 1] = 0.5 * (proj_all[2 * (size_t)p0 + 1] + proj_all[2 * (size_t)p1 + 1]);
            const int64_t node = flat_node(by_node[(size_t)(2 * k)]);
            rec.push_back({node, first_new + k, extra_xy[2 * (size_t)k], extra_xy[2 * (size_t)k + 1], 0.0});
            out.interp[2 * (size_t)k] = p0 + n_face;
            out.interp[2 * (size_t)k + 1] = p1 + n_face;
            true_corner[2 * (size_t)k] = nxy[2 * node];
            true_corner[2 * (size_t)k + 1] = nxy[2 * node + 1];
        }
        out.tail.insert(out.tail.end(), (size_t)n_extra, (int64_t)-1);
    }
    const auto tk1 = std::chrono::steady_clock::now();
    // ---- counter-clockwise order about the mean of each cell's corners (sums in record order, as np.bincount)
    const int64_t n_rec = (int64_t)rec.size();
    std::vector<double> sx((size_t)nb, 0.0), sy((size_t)nb, 0.0), cnt((size_t)nb, 0.0);
    for (const Rec &r : rec) {
        sx[(size_t)r.key] += r.x;
        sy[(size_t)r.key] += r.y;
        cnt[(size_t)r.key] += 1.0;
    }
    for (Rec &r : rec) {
        const double px = sx[(size_t)r.key] / cnt[(size_t)r.key], py = sy[(size_t)r.key] / cnt[(size_t)r.key];
        r.angle = std::atan2(r.y - py, r.x - px);
    }
    std::stable_sort(rec.begin(), rec.end(), [](const Rec &a, const Rec &b) {
        if (a.key != b.key) return a.key < b.key;
        return a.angle < b.angle;
    });
    const auto tk2 = std::chrono::steady_clock::now();
    // ---- dense table: one row per distinct key (ascending), -1 padded
    std::vector<int64_t> row_start;
    for (int64_t r = 0; r < n_rec; r++)
        if (r == 0 || rec[(size_t)r].key != rec[(size_t)r - 1].key) row_start.push_back(r);
    const int64_t n_cell = (int64_t)row_start.size();
    row_start.push_back(n_rec);
    int64_t m = 0;
    for (int64_t c = 0; c < n_cell; c++) m = std::max(m, row_start[(size_t)c + 1] - row_start[(size_t)c]);
    out.n_record = n_rec;
    if (m > VORONOI_BOUNDARY_MAX_CORNERS) {
        out.m = m;
        return VORONOI_BOUNDARY_CELL_CORNERS;
    }
    std::vector<int64_t> cells((size_t)(n_cell * m), -1);
    for (int64_t c = 0; c < n_cell; c++) {
        const Rec *row = rec.data() + row_start[(size_t)c];
        const int64_t len = row_start[(size_t)c + 1] - row_start[(size_t)c];
        for (int64_t j = 0; j < len; j++) cells[(size_t)(c * m + j)] = row[j].id;
    }
    if (add_vertices && !skip_concave) {
        // the true boundary node always replaces the substitute corner: no area comparison
        extra_xy = true_corner;
    } else if (add_vertices) {
        // ---- keep the true boundary node where it does not make the cell concave: the cell's area with the true node against
        // its area with the midpoint substitute (closed polygon: fill slots and the closing slot repeat corner 0)
        std::vector<double> term((size_t)m);
        for (int64_t c = 0; c < n_cell; c++) {
            const Rec *row = rec.data() + row_start[(size_t)c];
            const int64_t len = row_start[(size_t)c + 1] - row_start[(size_t)c];
            auto vertex = [&](int64_t j, bool use_true, double &x, double &y) { // corner j of the closed polygon
                const Rec &r = row[j < len ? j : 0];
                if (use_true && r.id >= first_new) {
                    x = true_corner[2 * (size_t)(r.id - first_new)];
                    y = true_corner[2 * (size_t)(r.id - first_new) + 1];
                } else {
                    x = r.x;
                    y = r.y;
                }
            };
            double area[2];
            for (int t = 0; t < 2; t++) {
                double x0, y0;
                vertex(0, t == 1, x0, y0);
                for (int64_t i = 0; i < m; i++) { // closed[i], closed[i + 1] with closed[m] = corner 0
                    double xa, ya, xb, yb;
                    vertex(i, t == 1, xa, ya);
                    vertex(i + 1 < m ? i + 1 : len, t == 1, xb, yb);
                    const double a0 = xa - x0, a1 = ya - y0, b0 = xb - x0, b1 = yb - y0;
                    term[(size_t)i] = a0 * b1 - a1 * b0;
                }
                area[t] = 0.5 * std::fabs(np_pairwise_sum(term.data(), m));
            }
            if (area[1] >= area[0])
                for (int64_t j = 0; j < len; j++)
                    if (row[j].id >= first_new) {
                        const int64_t k = row[j].id - first_new;
                        extra_xy[2 * (size_t)k] = true_corner[2 * (size_t)k];
                        extra_xy[2 * (size_t)k + 1] = true_corner[2 * (size_t)k + 1];
                    }
        }
    }
    const auto tk3 = std::chrono::steady_clock::now();
    out.ms_setup = std::chrono::duration<double, std::milli>(tk1 - tk0).count();
    out.ms_sort = std::chrono::duration<double, std::milli>(tk2 - tk1).count();
    out.ms_cells = std::chrono::duration<double, std::milli>(tk3 - tk2).count();
    out.cells = std::move(cells);
    out.n_cell = n_cell;
    out.m = m;
    out.extra_xy.resize((size_t)(n_proj + n_extra) * 2);
    for (int64_t e = 0; e < ne; e++)
        if (kept_rank[(size_t)e] >= 0) {
            out.extra_xy[2 * (size_t)kept_rank[(size_t)e]] = proj_all[2 * (size_t)e];
            out.extra_xy[2 * (size_t)kept_rank[(size_t)e] + 1] = proj_all[2 * (size_t)e + 1];
        }
    std::copy(extra_xy.begin(), extra_xy.end(), out.extra_xy.begin() + 2 * n_proj);
    return VORONOI_BOUNDARY_OK;
}

} // namespace xr
