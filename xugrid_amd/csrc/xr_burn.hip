// xr_burn.hip -- writing vector geometry into the faces of a mesh on the device: xugrid.burn_vector_geometry
// (xugrid/ugrid/burn.py:57-262).  The reference triangulates every polygon on the host (earcut) and searches the triangles
// one polygon at a time; here a face is in a polygon iff its centroid passes the per-segment rule of xr_point_in_face.h
// over ALL ring segments of the polygon, exterior and holes together (even-odd) -- no triangulation.
//
// Polygons: one lane per face walks the ring segments that can matter to its centroid.  Those come from a STRIP INDEX: the
// y-extent of the segments is cut into S strips and a segment is listed in every strip its y-range, widened by a pad of
// two tolerances plus the rounding of the coordinates, touches (so the on-edge test still sees a horizontal segment lying
// just across a strip border).  A strip's list is ordered by segment id -- hence by polygon id -- so the lane keeps one
// parity bit, settles a polygon where the id changes, and the last polygon settled "in" is the winner (the reference's
// sequential loop: later polygons overwrite earlier ones).  The list order comes from counts, not from the arrival of
// lanes: segments are taken in chunks of STRIP_CHUNK, count[strip][chunk] is scanned strip-major, and inside a chunk a
// segment's rank in a strip is the number of earlier segments of the chunk that touch it.
//
// all_touched polygons and lines reuse the segment clipper of the network gridder (xr_edge_length_csr_dev: faces x
// segments with a piece of positive length); k_burn_row_max folds the geometry ids of a face's row into its winner.  For
// polygons a ring segment drawn exactly along an edge of a face does not make that face "touched": the clipper reports such
// a piece to BOTH neighbours, the reference (triangles against faces, strict separating axes) to neither, and the face on
// the polygon's side is found through its centroid or another segment anyway.
// Points go through the locate kernel and a per-face atomicMax of the point index.  Every precedence is a maximum of
// ids, so no result depends on scheduling; k_burn_combine turns the three winners into values.
#include <algorithm>
#include <cmath>

#include "xr_objects.h"
#include "xr_point_in_face.h"
#include "xr_prims.h"

namespace xr {

static constexpr int BB = 256;          // threads per block
static constexpr int STRIP_CHUNK = 256; // segments per chunk of the ordered fill (one block)
static constexpr int64_t STRIP_MATRIX_MAX = (int64_t)16 << 20; // words of count[strip][chunk] (64 MB)
static constexpr int64_t STRIPS_AUTO_MAX = 1 << 16, STRIPS_FORCED_MAX = 1 << 20;

struct Strips {
    double y0, inv_h, lo, hi, pad; // strip of y: (y - y0) * inv_h; centroids outside [lo, hi] meet no segment
    int n;
};

// monotone non-decreasing in y; NaN lands in strip 0
__device__ __forceinline__ int strip_of(const Strips &s, double y) {
    const double t = (y - s.y0) * s.inv_h;
    return !(t >= 0.0) ? 0 : t >= (double)(s.n - 1) ? s.n - 1 : (int)t;
}

// flag = 1 unless off[0] == 0, off[n_off - 1] == total and off never decreases
__global__ void __launch_bounds__(BB)
k_burn_check_offsets(const int64_t *__restrict__ off, int64_t n_off, int64_t total, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    bool bad = false;
    if (i < n_off) {
        const int64_t v = off[i];
        bad = (i == 0 && v != 0) || (i == n_off - 1 && v != total) || (i > 0 && v < off[i - 1]);
    }
    wave_flag(bad, flag);
}

// the last r in [0, n) with off[r] <= i (off ascending, off[0] <= i)
__device__ __forceinline__ int64_t offset_owner(const int64_t *__restrict__ off, int64_t n, int64_t i) {
    int64_t lo = 0, hi = n; // off[lo] <= i < off[hi] (off[n] = total > i)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Segment i starts at vertex i and ends at the next vertex of its part (a ring or a line); the last vertex of a ring is
// joined to the ring's first (cyclic: the closing segment of an open ring; of a closed ring it has zero length), the last
// vertex of a line to itself (zero length: every rule passes it over).  key[i]: the geometry the segment belongs to --
// group_off == nullptr: the part itself (lines), else the group of the part (the polygon of a ring).
__global__ void __launch_bounds__(BB)
k_burn_segments(const double2 *__restrict__ xy, int64_t n_vertex, const int64_t *__restrict__ part_off, int64_t n_part,
                const int64_t *__restrict__ group_off, int64_t n_group, int cyclic, double4 *__restrict__ seg,
                int32_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (i >= n_vertex) return;
    const int64_t r = offset_owner(part_off, n_part, i);
    const int64_t end = part_off[r + 1];
    const int64_t nxt = i + 1 < end ? i + 1 : cyclic ? part_off[r] : i;
    const double2 a = xy[i], b = xy[nxt];
    seg[i] = make_double4(a.x, a.y, b.x, b.y);
    key[i] = (int32_t)(group_off ? offset_owner(group_off, n_group, r) : r);
}

// per block: ymin, ymax, the largest |coordinate| and the summed |dy| of the segments that count (len2 > 0); the |dy| of a
// block are summed in the order of block_reduce, the blocks' sums in that of k_fold_partials (xr_prims.h)
__global__ void __launch_bounds__(BB) k_burn_extent(const double4 *__restrict__ seg, int64_t n, double *__restrict__ partial) {
    __shared__ double lds[4 * (BB / 64)];
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    double y0 = INFINITY, y1 = -INFINITY, am = 0.0, dy = 0.0;
    if (i < n) {
        const double4 s = seg[i];
        const double wx = s.z - s.x, wy = s.w - s.y;
        if (wx * wx + wy * wy > 0) {
            y0 = fmin(s.y, s.w), y1 = fmax(s.y, s.w);
            am = fmax(fmax(fabs(s.x), fabs(s.z)), fmax(fabs(s.y), fabs(s.w)));
            dy = fabs(wy);
        }
    }
    block_reduce<BB, OpMin, OpMax, OpMax, OpSum>(lds, y0, y1, am, dy);
    if (threadIdx.x == 0) {
        double *out = partial + (int64_t)blockIdx.x * 4;
        out[0] = y0, out[1] = y1, out[2] = am, out[3] = dy;
    }
}

// span[i] = (first, last) strip of segment i, (1, 0) for a segment no rule reads; count[strip * n_chunk + chunk] += 1 for
// every strip of the span (the counts do not depend on the order of the additions); total += length of the span
__global__ void __launch_bounds__(BB)
k_burn_strip_count(const double4 *__restrict__ seg, int64_t n, Strips st, int n_chunk, int2 *__restrict__ span,
                   int32_t *__restrict__ count, unsigned long long *__restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (i >= n) return;
    const double4 s = seg[i];
    const double wx = s.z - s.x, wy = s.w - s.y;
    int2 sp = make_int2(1, 0);
    if (wx * wx + wy * wy > 0) sp = make_int2(strip_of(st, fmin(s.y, s.w) - st.pad), strip_of(st, fmax(s.y, s.w) + st.pad));
    span[i] = sp;
    if (sp.y < sp.x) return;
    const int64_t chunk = i / STRIP_CHUNK;
    for (int k = sp.x; k <= sp.y; k++) atomicAdd(&count[(int64_t)k * n_chunk + chunk], 1);
    atomicAdd(total, (unsigned long long)(sp.y - sp.x + 1));
}

// entry[start[strip * n_chunk + chunk] + rank] = segment, rank = earlier segments of the chunk that touch the strip: the
// list of a strip holds its segments in ascending id whatever order the lanes run in.  One block per chunk; the lanes of a
// wave read the same earlier span at the same time (a broadcast).
__global__ void __launch_bounds__(STRIP_CHUNK)
k_burn_strip_fill(const int2 *__restrict__ span, int64_t n, int n_chunk, const int32_t *__restrict__ start,
                  int32_t *__restrict__ entry) {
    __shared__ int2 sh[STRIP_CHUNK];
    const int64_t i = (int64_t)blockIdx.x * STRIP_CHUNK + threadIdx.x;
    const int2 sp = i < n ? span[i] : make_int2(1, 0);
    sh[threadIdx.x] = sp;
    __syncthreads();
    for (int k = sp.x; k <= sp.y; k++) {
        int rank = 0;
        for (int j = 0; j < (int)threadIdx.x; j++) rank += (sh[j].x <= k) & (k <= sh[j].y);
        entry[start[(int64_t)k * n_chunk + blockIdx.x] + rank] = (int32_t)i;
    }
}

// One lane per face: the centroid against the segments of its strip, polygon by polygon.  winner[f] = the last (highest)
// polygon whose segments put the centroid on an edge or give an odd crossing number, -1 for none.
__global__ void __launch_bounds__(BB)
k_burn_polygons(const double2 *__restrict__ centroid, int64_t n_face, Strips st, int n_chunk, const int32_t *__restrict__ start,
                const int32_t *__restrict__ entry, const double4 *__restrict__ seg, const int32_t *__restrict__ seg_polygon,
                double tol, int32_t *__restrict__ winner) {
    const int64_t f = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (f >= n_face) return;
    const double2 c = centroid[f];
    int32_t win = -1;
    if (c.y >= st.lo && c.y <= st.hi) {
        const int64_t s = strip_of(st, c.y);
        const P2 p{c.x, c.y};
        int32_t cur = -1;
        bool odd = false, on_edge = false;
        for (int32_t e = start[s * n_chunk], e1 = start[(s + 1) * n_chunk]; e < e1; e++) {
            const int32_t id = entry[e], g = seg_polygon[id];
            if (g != cur) {
                if (on_edge || odd) win = cur;
                cur = g, odd = false, on_edge = false;
            }
            const double4 v = seg[id];
            point_vs_segment(P2{v.x, v.y}, P2{v.z, v.w}, p, tol, on_edge, odd);
        }
        if (on_edge || odd) win = cur;
    }
    winner[f] = win;
}

// The segment lies on the line of an edge of the convex face: whatever piece of it the face holds runs along the face's
// boundary (exact arithmetic on purpose: it is the segments drawn along mesh lines that both neighbours would report)
__device__ __forceinline__ bool along_face_edge(const double *__restrict__ poly, int n, double4 s) {
    P2 a = load_p2(poly, n - 1);
    for (int i = 0; i < n; i++) {
        const P2 b = load_p2(poly, i);
        const double ex = b.x - a.x, ey = b.y - a.y;
        if ((ex != 0 || ey != 0) && ex * (s.y - a.y) - ey * (s.x - a.x) == 0 && ex * (s.w - a.y) - ey * (s.z - a.x) == 0) return true;
        a = b;
    }
    return false;
}

// winner[f] = max(winner[f], key of every column stored in row f); with fxy (the faces' vertex blocks): of every column
// whose segment does not run along an edge of face f
__global__ void __launch_bounds__(BB)
k_burn_row_max(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n_row,
               const int32_t *__restrict__ key, const double *__restrict__ fxy, const uint8_t *__restrict__ len,
               const int32_t *__restrict__ off, int m, const double4 *__restrict__ seg, int32_t *__restrict__ winner) {
    const int64_t f = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (f >= n_row) return;
    int32_t w = winner[f];
    for (int32_t e = indptr[f], e1 = indptr[f + 1]; e < e1; e++) {
        const int32_t column = indices[e], k = key[column];
        if (k > w && !(fxy && along_face_edge(fxy + 2 * face_vertex_base(off, f, m), len[f], seg[column]))) w = k;
    }
    winner[f] = w;
}

// winner[face of point i] = max(.., i): the highest point index of a face, whatever order the lanes arrive in
__global__ void __launch_bounds__(BB)
k_burn_point_max(const int64_t *__restrict__ face, int64_t n_point, int64_t n_face, int32_t *__restrict__ winner) {
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (i >= n_point) return;
    const int64_t f = face[i];
    if (f >= 0 && f < n_face) atomicMax(&winner[f], (int32_t)i);
}

// points over lines over polygons; a missing winner array means no geometry of that kind, missing values mean 1.0
__global__ void __launch_bounds__(BB)
k_burn_combine(int64_t n_face, const int32_t *__restrict__ w_polygon, const double *__restrict__ v_polygon,
               const int32_t *__restrict__ w_line, const double *__restrict__ v_line, const int32_t *__restrict__ w_point,
               const double *__restrict__ v_point, double fill, double *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (f >= n_face) return;
    const int32_t wt = w_point ? w_point[f] : -1, wl = w_line ? w_line[f] : -1, wg = w_polygon ? w_polygon[f] : -1;
    double v = fill;
    if (wt >= 0) v = v_point ? v_point[wt] : 1.0;
    else if (wl >= 0) v = v_line ? v_line[wl] : 1.0;
    else if (wg >= 0) v = v_polygon ? v_polygon[wg] : 1.0;
    out[f] = v;
}

static void require_offsets(const char *what, const int64_t *off_dev, int64_t n_part, int64_t total) {
    DevBuf<int32_t> flag(1);
    fill_i32(flag.get(), 0, 1);
    XR_LAUNCH("burn_check_offsets", k_burn_check_offsets, dim3(div_up(n_part + 1, BB)), dim3(BB), 0, off_dev, n_part + 1, total,
              flag.get());
    XR_REQUIRE(read_scalar(flag.get()) == 0, XR_ERR_INVALID,
               "%s must start at 0, end at %lld and never decrease", what, (long long)total);
}

// winner[f] = max(winner[f], key[segment]) over the segments with a piece of positive length in face f; interior_only: a
// piece that runs along the boundary of the face does not count
static void touched_max(xr_mesh *mesh, const double4 *seg, int64_t n_seg, const int32_t *key, bool interior_only, int32_t *winner) {
    xr_csr *csr = nullptr;
    const int rc = xr_edge_length_csr_dev(mesh, reinterpret_cast<const double *>(seg), n_seg, &csr);
    if (rc != XR_OK) throw Failure{rc};
    std::unique_ptr<xr_csr> keep(csr);
    if (csr->nnz > 0) {
        if (interior_only) {
            mesh_prepare(mesh, true);
            mesh_face_coords(mesh);
        }
        XR_LAUNCH("burn_row_max", k_burn_row_max, dim3(div_up(csr->n, BB)), dim3(BB), 0, csr->indptr.get(), csr->indices.get(),
                  csr->n, key, interior_only ? mesh->prep.fxy.get() : (const double *)nullptr, mesh->prep.len.get(), mesh->caller_off(),
                  mesh->m, seg, winner);
    }
    stream_sync(); // (the matrix goes back to the pool behind its reader)
}

static void burn_polygons(xr_mesh *mesh, const double *coords_dev, int64_t n_vertex, const int64_t *ring_off, int64_t n_ring,
                          const int64_t *polygon_off, int64_t n_polygon, bool all_touched, int32_t *winner) {
    const int64_t F = mesh->n_face;
    if (F == 0) return;
    fill_i32(winner, -1, F);
    if (n_polygon == 0) return;
    require_offsets("ring_offsets", ring_off, n_ring, n_vertex);
    require_offsets("polygon_offsets", polygon_off, n_polygon, n_ring);
    if (n_vertex == 0) return;
    mesh_prepare(mesh, false);
    mesh_read_stats(mesh, /*need_exact=*/true);
    const double tol = 1e-12 * mesh->stats.h[stat::MAX_DIAGONAL]; // the default tolerance of xr_locate_points
    const int64_t n_seg = n_vertex;
    DevBuf<double4> seg((size_t)n_seg);
    DevBuf<int32_t> seg_polygon((size_t)n_seg);
    XR_LAUNCH("burn_segments", k_burn_segments, dim3(div_up(n_seg, BB)), dim3(BB), 0, reinterpret_cast<const double2 *>(coords_dev),
              n_vertex, ring_off, n_ring, polygon_off, n_polygon, 1, seg.get(), seg_polygon.get());
    // ---- the strips: extent of the segments, then their number from the mean y-range of a segment
    const unsigned nb = div_up(n_seg, BB);
    TwoStageReduce<BB, double, OpMin, OpMax, OpMax, OpSum> extent("burn_extent_final", nb, [&](double *partial) {
        XR_LAUNCH("burn_extent", k_burn_extent, dim3(nb), dim3(BB), 0, seg.get(), n_seg, partial);
    });
    double ext[4]; // ymin, ymax, largest |coordinate|, sum |dy|
    extent.read(ext);
    const bool any = std::isfinite(ext[0]) && std::isfinite(ext[1]) && ext[1] >= ext[0];
    if (any) {
        const int n_chunk = (int)div_up(n_seg, STRIP_CHUNK);
        const double height = ext[1] - ext[0];
        // (a list is read by every face of its strip: about two strips per segment keep the lists short without repeating
        // the segments more than twice over)
        int64_t n_strip = option(OPT_BURN_STRIPS) > 0 ? std::min<int64_t>(option(OPT_BURN_STRIPS), STRIPS_FORCED_MAX)
                          : ext[3] > 0 && height > 0
                              ? (int64_t)std::min<double>(2.0 * (double)n_seg * height / ext[3], (double)std::min(n_seg, STRIPS_AUTO_MAX))
                              : 1;
        n_strip = std::max<int64_t>(1, std::min(n_strip, STRIP_MATRIX_MAX / n_chunk));
        if (!(height > 0) || !std::isfinite(height)) n_strip = 1;
        Strips st{};
        st.n = (int)n_strip;
        st.y0 = ext[0];
        st.inv_h = n_strip > 1 ? (double)n_strip / height : 0.0;
        st.pad = 2.0 * tol + 1e-14 * (std::isfinite(ext[2]) ? ext[2] : 0.0);
        st.lo = ext[0] - st.pad, st.hi = ext[1] + st.pad;
        const int64_t n_word = n_strip * n_chunk;
        DevBuf<int2> span((size_t)n_seg);
        DevBuf<int32_t> count((size_t)n_word), start((size_t)n_word + 1);
        DevBuf<unsigned long long> total_dev(1);
        fill_i32(count.get(), 0, n_word);
        fill_i32(reinterpret_cast<int32_t *>(total_dev.get()), 0, 2);
        XR_LAUNCH("burn_strip_count", k_burn_strip_count, dim3(nb), dim3(BB), 0, seg.get(), n_seg, st, n_chunk, span.get(),
                  count.get(), total_dev.get());
        const unsigned long long total = read_scalar(total_dev.get());
        XR_REQUIRE(total < (unsigned long long)INT32_MAX, XR_ERR_LIMIT,
                   "xr_burn_polygons_dev: %llu strip entries for %lld ring segments exceed the int32 range", total, (long long)n_seg);
        if (total > 0) {
            exclusive_scan_i32(count.get(), start.get(), n_word);
            DevBuf<int32_t> entry((size_t)total);
            XR_LAUNCH("burn_strip_fill", k_burn_strip_fill, dim3(n_chunk), dim3(STRIP_CHUNK), 0, span.get(), n_seg, n_chunk,
                      start.get(), entry.get());
            const auto centroids = mesh_centroids_shared(mesh);
            XR_LAUNCH("burn_polygons", k_burn_polygons, dim3(div_up(F, BB)), dim3(BB), 0,
                      reinterpret_cast<const double2 *>(centroids->get()), F, st, n_chunk, start.get(), entry.get(), seg.get(),
                      seg_polygon.get(), tol, winner);
            stream_sync(); // (the index goes back to the pool behind its reader)
        }
    }
    if (all_touched) touched_max(mesh, seg.get(), n_seg, seg_polygon.get(), /*interior_only=*/true, winner);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_burn_polygons_dev(xr_mesh *mesh, const double *coords_dev, int64_t n_vertex, const int64_t *ring_offsets_dev,
                         int64_t n_ring, const int64_t *polygon_offsets_dev, int64_t n_polygon, int all_touched,
                         int32_t *winner_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (winner_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_burn_polygons_dev: NULL argument");
    XR_REQUIRE(n_vertex >= 0 && n_ring >= 0 && n_polygon >= 0, XR_ERR_INVALID, "xr_burn_polygons_dev: negative size");
    XR_REQUIRE(n_vertex < ((int64_t)1 << 30) && n_ring < INT32_MAX && n_polygon < INT32_MAX, XR_ERR_LIMIT,
               "xr_burn_polygons_dev: too many vertices, rings or polygons");
    XR_REQUIRE((coords_dev || n_vertex == 0) && ((ring_offsets_dev && polygon_offsets_dev) || n_polygon == 0), XR_ERR_INVALID,
               "xr_burn_polygons_dev: NULL argument");
    try {
        burn_polygons(mesh, coords_dev, n_vertex, ring_offsets_dev, n_ring, polygon_offsets_dev, n_polygon, all_touched != 0,
                      winner_dev);
    } catch (const Failure &) {
        try {
            stream_sync(); // (nothing in flight still reads the caller's arrays)
        } catch (const Failure &) {
        }
        throw;
    }
    dev_call_done();
    XR_API_END
}

int xr_burn_lines_dev(xr_mesh *mesh, const double *coords_dev, int64_t n_vertex, const int64_t *line_offsets_dev, int64_t n_line,
                      int32_t *winner_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (winner_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_burn_lines_dev: NULL argument");
    XR_REQUIRE(n_vertex >= 0 && n_line >= 0, XR_ERR_INVALID, "xr_burn_lines_dev: negative size");
    XR_REQUIRE(n_vertex < ((int64_t)1 << 30) && n_line < INT32_MAX, XR_ERR_LIMIT, "xr_burn_lines_dev: too many vertices or lines");
    XR_REQUIRE((coords_dev || n_vertex == 0) && (line_offsets_dev || n_line == 0), XR_ERR_INVALID,
               "xr_burn_lines_dev: NULL argument");
    const int64_t F = mesh->n_face;
    try {
        if (F > 0) {
            fill_i32(winner_dev, -1, F);
            if (n_line > 0) {
                require_offsets("line_offsets", line_offsets_dev, n_line, n_vertex);
                if (n_vertex > 0) {
                    DevBuf<double4> seg((size_t)n_vertex);
                    DevBuf<int32_t> seg_line((size_t)n_vertex);
                    XR_LAUNCH("burn_segments", k_burn_segments, dim3(div_up(n_vertex, BB)), dim3(BB), 0,
                              reinterpret_cast<const double2 *>(coords_dev), n_vertex, line_offsets_dev, n_line,
                              (const int64_t *)nullptr, (int64_t)0, 0, seg.get(), seg_line.get());
                    touched_max(mesh, seg.get(), n_vertex, seg_line.get(), /*interior_only=*/false, winner_dev);
                }
            }
        }
    } catch (const Failure &) {
        try {
            stream_sync();
        } catch (const Failure &) {
        }
        throw;
    }
    dev_call_done();
    XR_API_END
}

int xr_burn_points_dev(xr_mesh *mesh, const double *coords_dev, int64_t n_point, int32_t *winner_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (winner_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_burn_points_dev: NULL argument");
    XR_REQUIRE(n_point >= 0 && (coords_dev || n_point == 0), XR_ERR_INVALID, "xr_burn_points_dev: bad arguments");
    XR_REQUIRE(n_point < INT32_MAX, XR_ERR_LIMIT, "xr_burn_points_dev: too many points");
    const int64_t F = mesh->n_face;
    try {
        if (F > 0) {
            fill_i32(winner_dev, -1, F);
            if (n_point > 0) {
                DevBuf<int64_t> face((size_t)n_point);
                locate_points_dev(mesh, coords_dev, n_point, -1.0, face.get());
                XR_LAUNCH("burn_point_max", k_burn_point_max, dim3(div_up(n_point, BB)), dim3(BB), 0, face.get(), n_point, F,
                          winner_dev);
                stream_sync();
            }
        }
    } catch (const Failure &) {
        try {
            stream_sync();
        } catch (const Failure &) {
        }
        throw;
    }
    dev_call_done();
    XR_API_END
}

int xr_burn_combine_dev(int64_t n_face, const int32_t *polygon_winner_dev, const double *polygon_values_dev,
                        const int32_t *line_winner_dev, const double *line_values_dev, const int32_t *point_winner_dev,
                        const double *point_values_dev, double fill, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(n_face >= 0 && (out_dev || n_face == 0), XR_ERR_INVALID, "xr_burn_combine_dev: bad arguments");
    if (n_face > 0)
        XR_LAUNCH("burn_combine", k_burn_combine, dim3(div_up(n_face, BB)), dim3(BB), 0, n_face, polygon_winner_dev,
                  polygon_values_dev, line_winner_dev, line_values_dev, point_winner_dev, point_values_dev, fill, out_dev);
    dev_call_done();
    XR_API_END
}

} // extern "C"
