// xr_polygonize.hip -- regions of equal face value -> polygon rings, on the device (xugrid.polygonize,
// xugrid/ugrid/polygonize.py; semantics: DESIGN section 12).  Reads the face nodes of the mesh and edge_face / face_edge /
// node -> face of its topology where they are; the output has the layout xr_burn_polygons_dev reads.
//
// Route:
//   1. per face: the value as float64, valid (not NaN), the sign of the shoelace sum in the caller's node order.
//   2. region labels by hook-and-compress: a hook launch over the edges joins the roots of the two faces of every connecting edge
//      (atomicMin of the larger root's parent), a compress launch points every face at its root; until a hook changes nothing.
//      Parents only decrease and stay inside the region, so a stale read inside a launch costs a round at most; the fixed point
//      -- every face points at the smallest face of its region -- is reached across kernel boundaries only.
//   3. regions numbered by flag / scan / rank over the roots (as k_comp_flag / k_comp_number, valid faces only).
//   4. boundary half-edges (face, slot) flagged and compacted in (face, slot) order.
//   5. successor of every half-edge by the fan walk about its end node through the region: a permutation whose cycles are the rings.
//   6. cycle leader (smallest half-edge) and distance to the end of the cycle by pointer doubling, ceil(log2(n)) launches each.
//   7. rings numbered by leader; length, polygon and shoelace sign per ring; half-edges listed ring by ring.
//   8. the ring table (three int32 per ring) goes to the host, which puts the rings of every polygon in canonical order
//      (xr_polygonize_order.h) and sends back one place per ring and the two offset arrays.
//   9. one launch writes the coordinates, the closing vertex of every ring included.
#include <algorithm>
#include <vector>

#include "xr_polygonize_order.h"
#include "xr_prims.h"
#include "xr_topology.h"

struct xr_polygons {
    int64_t n_face = 0, n_polygon = 0, n_ring = 0, n_vertex = 0, n_halfedge = 0, label_rounds = 0, readbacks = 0;
    xr::DevBuf<double> coords;            // [n_vertex*2]
    xr::DevBuf<int64_t> ring_offsets;     // [n_ring+1]
    xr::DevBuf<int64_t> polygon_offsets;  // [n_polygon+1]
    xr::DevBuf<double> values;            // [n_polygon]
    xr::DevBuf<int64_t> face_polygon;     // [n_face]
};

namespace xr {

static constexpr int PB = 256;
enum PgFlag : int { PG_DEGENERATE = 0, PG_WALK = 1, PG_CHANGED = 2, PG_PERMUTATION = 3, PG_COUNT = 4 };

// real nodes of a face: the fill (-1) trails
__device__ __forceinline__ int pg_face_len(const int32_t *__restrict__ face, int m) {
    int n = 0;
    while (n < m && face[n] >= 0) n++;
    return n;
}

// the edge of slot s (node s -> its successor, the two different): face_edge is compacted over the slots that are edges
// (k_topo_face_edge), so the slot's place is its rank among them
__device__ __forceinline__ int pg_slot_edge(const int32_t *__restrict__ face, const int32_t *__restrict__ face_edge_row, int s) {
    int rank = 0;
    for (int j = 0; j < s; j++) rank += face[j] != face[j + 1];
    return face_edge_row[rank];
}

// the face on the other side of edge e seen from f, -1: none
__device__ __forceinline__ int pg_across(const int32_t *__restrict__ edge_face, int e, int f) {
    const int a = edge_face[2 * (int64_t)e], b = edge_face[2 * (int64_t)e + 1];
    return a == f ? b : a;
}

// node a half-edge (slot i of the flat face table) starts at, the face on its left
__device__ __forceinline__ int pg_start_node(const int32_t *__restrict__ faces, int m, const int8_t *__restrict__ orient, int i) {
    const int f = i / m, s = i - f * m;
    const int32_t *face = faces + (int64_t)f * m;
    if (orient[f] > 0) return face[s];
    const int L = pg_face_len(face, m);
    return face[s + 1 == L ? 0 : s + 1];
}

// 1: value, validity and orientation of every face; parent = self
template <typename T>
__global__ void __launch_bounds__(PB)
k_pg_prepare(const T *__restrict__ data, const int32_t *__restrict__ faces, int m, const double *__restrict__ node_xy, int64_t n_face,
             double *__restrict__ val, int8_t *__restrict__ orient, int32_t *__restrict__ parent, int32_t *__restrict__ flags) {
    const int64_t f = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (f >= n_face) return;
    const double v = (double)data[f];
    val[f] = v;
    parent[f] = (int32_t)f;
    int8_t o = 0;
    if (v == v) {
        const int32_t *face = faces + f * m;
        const int L = pg_face_len(face, m);
        double s = 0.0;
        for (int k = 0; k < L; k++) {
            const int64_t a = face[k], b = face[k + 1 == L ? 0 : k + 1];
            s += node_xy[2 * a] * node_xy[2 * b + 1] - node_xy[2 * b] * node_xy[2 * a + 1];
        }
        o = s > 0.0 ? 1 : -1;
        if (s == 0.0 || !(fabs(s) <= 1.7976931348623157e308)) atomicAdd(&flags[PG_DEGENERATE], 1); // (rare: an error follows)
    }
    orient[f] = o;
}

// 2a: hook.  parent[x] <= x always, so the walk to a root ends; with a stale read it ends at a member that WAS a root.
__global__ void __launch_bounds__(PB)
k_pg_hook(const int32_t *__restrict__ edge_face, int64_t n_edge, const double *__restrict__ val, const int8_t *__restrict__ orient,
          int32_t *parent, int32_t *__restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= n_edge) return;
    const int a = edge_face[2 * e], b = edge_face[2 * e + 1];
    if (a < 0 || b < 0 || !orient[a] || !orient[b] || !(val[a] == val[b])) return;
    int ra = a, rb = b, p;
    while ((p = parent[ra]) < ra) ra = p;
    while ((p = parent[rb]) < rb) rb = p;
    if (ra == rb) return;
    const int hi = max(ra, rb), lo = min(ra, rb);
    if (atomicMin(&parent[hi], lo) > lo) flags[PG_CHANGED] = 1;
}

// 2b: compress.  Only thread x stores parent[x]; what other threads read meanwhile is the old or the new ancestor.
__global__ void __launch_bounds__(PB) k_pg_compress(int32_t *parent, int64_t n_face) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x >= n_face) return;
    int r = (int)x, p;
    while ((p = parent[r]) < r) r = p;
    if (r < (int)x) parent[x] = r;
}

// 3: roots of valid faces; then the number of every face and the value of every region
__global__ void __launch_bounds__(PB)
k_pg_region_flag(const int32_t *__restrict__ parent, const int8_t *__restrict__ orient, int64_t n_face, int32_t *__restrict__ flag) {
    const int64_t f = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (f < n_face) flag[f] = orient[f] != 0 && parent[f] == (int32_t)f;
}
__global__ void __launch_bounds__(PB)
k_pg_region_number(const int32_t *__restrict__ parent, const int8_t *__restrict__ orient, const int32_t *__restrict__ rank,
                   const double *__restrict__ val, int64_t n_face, int32_t *__restrict__ region, int64_t *__restrict__ face_polygon,
                   double *__restrict__ values) {
    const int64_t f = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (f >= n_face) return;
    const int r = orient[f] ? rank[parent[f]] : -1;
    region[f] = r;
    face_polygon[f] = r;
    if (orient[f] && parent[f] == (int32_t)f) values[r] = val[f];
}

// 4: one thread per slot: a boundary half-edge?
__global__ void __launch_bounds__(PB)
k_pg_halfedge_flag(const int32_t *__restrict__ faces, int64_t n_face, int m, const int32_t *__restrict__ face_edge,
                   const int32_t *__restrict__ edge_face, const int32_t *__restrict__ region, int32_t *__restrict__ hflag,
                   int32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n_face * m) return;
    const int64_t f = i / m;
    const int s = (int)(i - f * m);
    int flag = 0;
    if (region[f] >= 0) {
        const int32_t *face = faces + f * m;
        const int L = pg_face_len(face, m);
        if (s < L && face[s] != face[s + 1 == L ? 0 : s + 1]) {
            const int e = pg_slot_edge(face, face_edge + f * m, s);
            if (e < 0) flags[PG_WALK] = 1; // (a slot that is an edge has one)
            else {
                const int g = pg_across(edge_face, e, (int)f);
                flag = g < 0 || region[g] != region[f];
            }
        }
    }
    hflag[i] = flag;
}

// 5: successor of half-edge h = a -> b of face f: in f the slot that leaves b; a boundary half-edge is the answer, else across it
// and again.  The walk visits a face about b once, so it ends within the faces that name b (nf_ptr); anything else is a broken
// table and is reported (the half-edge then succeeds itself, which keeps every later index in range).
__global__ void __launch_bounds__(PB)
k_pg_successor(const int32_t *__restrict__ he_slot, int64_t n_he, const int32_t *__restrict__ faces, int m,
               const int32_t *__restrict__ face_edge, const int32_t *__restrict__ edge_face, const int8_t *__restrict__ orient,
               const int32_t *__restrict__ hflag, const int32_t *__restrict__ hpos, const int32_t *__restrict__ nf_ptr,
               int32_t *__restrict__ succ, int32_t *__restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    const int i = he_slot[h];
    int f = i / m;
    const int s = i - f * m;
    const int32_t *face = faces + (int64_t)f * m;
    int L = pg_face_len(face, m);
    const int b = orient[f] > 0 ? face[s + 1 == L ? 0 : s + 1] : face[s];
    const int limit = nf_ptr[b + 1] - nf_ptr[b];
    int out = -1;
    for (int step = 0; step <= limit; step++) {
        face = faces + (int64_t)f * m;
        L = pg_face_len(face, m);
        const bool ccw = orient[f] > 0;
        int t = -1;
        for (int k = 0; k < L && t < 0; k++) {
            const int from = ccw ? face[k] : face[k + 1 == L ? 0 : k + 1], to = ccw ? face[k + 1 == L ? 0 : k + 1] : face[k];
            if (from == b && to != b) t = k;
        }
        if (t < 0) break;
        const int64_t idx = (int64_t)f * m + t;
        if (hflag[idx]) {
            out = hpos[idx];
            break;
        }
        const int e = pg_slot_edge(face, face_edge + (int64_t)f * m, t);
        if (e < 0) break;
        const int g = pg_across(edge_face, e, f);
        if (g < 0) break;
        f = g;
    }
    if (out < 0) {
        flags[PG_WALK] = 1;
        out = (int)h;
    }
    succ[h] = out;
}

// the successor must be a permutation: every half-edge is entered once
__global__ void __launch_bounds__(PB) k_pg_indegree(const int32_t *__restrict__ succ, int64_t n_he, int32_t *__restrict__ indeg) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h < n_he) atomicAdd(&indeg[succ[h]], 1);
}
__global__ void __launch_bounds__(PB)
k_pg_leader_init(const int32_t *__restrict__ indeg, const int32_t *__restrict__ succ, int64_t n_he, int32_t *__restrict__ nxt,
                 int32_t *__restrict__ mn, int32_t *__restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    if (indeg[h] != 1) flags[PG_PERMUTATION] = 1;
    nxt[h] = succ[h];
    mn[h] = (int32_t)h;
}
// 6a: one doubling round of the cycle minimum: (nxt, mn) cover 2^k half-edges from h on
__global__ void __launch_bounds__(PB)
k_pg_leader_round(const int32_t *__restrict__ nxt, const int32_t *__restrict__ mn, int64_t n_he, int32_t *__restrict__ nxt_out,
                  int32_t *__restrict__ mn_out) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    const int n = nxt[h];
    mn_out[h] = min(mn[h], mn[n]);
    nxt_out[h] = nxt[n];
}
// 6b: the cycle cut open in front of its leader: steps from h to the last half-edge of the ring
__global__ void __launch_bounds__(PB)
k_pg_dist_init(const int32_t *__restrict__ succ, const int32_t *__restrict__ leader, int64_t n_he, int32_t *__restrict__ nxt,
               int32_t *__restrict__ dist) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    const bool last = succ[h] == leader[h];
    nxt[h] = last ? (int32_t)h : succ[h];
    dist[h] = last ? 0 : 1;
}
__global__ void __launch_bounds__(PB)
k_pg_dist_round(const int32_t *__restrict__ nxt, const int32_t *__restrict__ dist, int64_t n_he, int32_t *__restrict__ nxt_out,
                int32_t *__restrict__ dist_out) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    const int n = nxt[h];
    dist_out[h] = dist[h] + dist[n];
    nxt_out[h] = nxt[n];
}

// 7: rings by leader
__global__ void __launch_bounds__(PB) k_pg_ring_flag(const int32_t *__restrict__ leader, int64_t n_he, int32_t *__restrict__ flag) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h < n_he) flag[h] = leader[h] == (int32_t)h;
}
__global__ void __launch_bounds__(PB)
k_pg_ring_table(const int32_t *__restrict__ leader, const int32_t *__restrict__ ring_rank, const int32_t *__restrict__ dist,
                const int32_t *__restrict__ he_slot, const int32_t *__restrict__ region, int m, int64_t n_he,
                int32_t *__restrict__ ring_len, int32_t *__restrict__ ring_poly) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he || leader[h] != (int32_t)h) return;
    const int r = ring_rank[h];
    ring_len[r] = dist[h] + 1;
    ring_poly[r] = region[he_slot[h] / m];
}
// half-edges ring by ring, each ring from its leader on
__global__ void __launch_bounds__(PB)
k_pg_ring_list(const int32_t *__restrict__ leader, const int32_t *__restrict__ ring_rank, const int32_t *__restrict__ dist,
               const int32_t *__restrict__ ring_start, int64_t n_he, int32_t *__restrict__ listed, int32_t *__restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    const int l = leader[h], r = ring_rank[l];
    const int pos = dist[l] - dist[h];
    if (pos < 0 || pos >= ring_start[r + 1] - ring_start[r]) { // (cannot happen on a permutation)
        flags[PG_PERMUTATION] = 1;
        return;
    }
    listed[ring_start[r] + pos] = (int32_t)h;
}
// sign of the shoelace sum of every ring, coordinates relative to its first vertex: one wave per ring, lanes stride over its
// segments, butterfly in fixed order (the same bits on every run; only the sign is kept)
__global__ void __launch_bounds__(PB)
k_pg_ring_sign(const int32_t *__restrict__ listed, const int32_t *__restrict__ ring_start, int64_t n_ring,
               const int32_t *__restrict__ he_slot, const int32_t *__restrict__ faces, int m, const int8_t *__restrict__ orient,
               const double *__restrict__ node_xy, int32_t *__restrict__ ring_sign) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (PB / 64) + (threadIdx.x >> 6);
    if (r >= n_ring) return; // (whole waves leave together)
    const int base = ring_start[r], n = ring_start[r + 1] - base;
    const int64_t v0 = pg_start_node(faces, m, orient, he_slot[listed[base]]);
    const double x0 = node_xy[2 * v0], y0 = node_xy[2 * v0 + 1];
    double sum = 0.0;
    for (int k = lane; k < n; k += 64) {
        const int64_t a = pg_start_node(faces, m, orient, he_slot[listed[base + k]]);
        const int64_t b = pg_start_node(faces, m, orient, he_slot[listed[base + (k + 1 == n ? 0 : k + 1)]]);
        const double ax = node_xy[2 * a] - x0, ay = node_xy[2 * a + 1] - y0, bx = node_xy[2 * b] - x0, by = node_xy[2 * b + 1] - y0;
        sum += ax * by - bx * ay;
    }
    sum = wave_reduce<OpSum>(sum); // (a sum of doubles: the order of xr_prims.h)
    if (lane == 0) ring_sign[r] = sum > 0.0 ? 1 : sum < 0.0 ? -1 : 0;
}

// 9: every half-edge writes its start vertex at its place in its ring; the leader also closes the ring
__global__ void __launch_bounds__(PB)
k_pg_gather(const int32_t *__restrict__ leader, const int32_t *__restrict__ ring_rank, const int32_t *__restrict__ dist,
            const int32_t *__restrict__ new_pos, const int64_t *__restrict__ ring_offsets, const int32_t *__restrict__ he_slot,
            const int32_t *__restrict__ faces, int m, const int8_t *__restrict__ orient, const double *__restrict__ node_xy,
            int64_t n_he, double *__restrict__ coords) {
    const int64_t h = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (h >= n_he) return;
    const int l = leader[h];
    const int ring = new_pos[ring_rank[l]];
    const int64_t first = ring_offsets[ring], end = ring_offsets[ring + 1];
    const int64_t at = first + (dist[l] - dist[h]);
    if (at < first || at >= end - 1) return; // (cannot happen: the ring has end - first - 1 half-edges)
    const int64_t v = pg_start_node(faces, m, orient, he_slot[h]);
    const double x = node_xy[2 * v], y = node_xy[2 * v + 1];
    coords[2 * at] = x, coords[2 * at + 1] = y;
    if (at == first) coords[2 * (end - 1)] = x, coords[2 * (end - 1) + 1] = y;
}

__global__ void __launch_bounds__(PB) k_pg_fill_i64(int64_t *__restrict__ p, int64_t v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i < n) p[i] = v;
}

static int doubling_rounds(int64_t n) {
    int k = 0;
    while (((int64_t)1 << k) < n) k++;
    return k;
}

// no region at all: empty arrays, offsets [0]
static void polygons_empty(xr_polygons *p) {
    p->n_polygon = p->n_ring = p->n_vertex = p->n_halfedge = 0;
    p->coords.alloc(1), p->ring_offsets.alloc(1), p->polygon_offsets.alloc(1);
    if (!p->values.get()) p->values.alloc(1);
    XR_LAUNCH("pg_fill_i64", k_pg_fill_i64, dim3(1), dim3(PB), 0, p->ring_offsets.get(), (int64_t)0, (int64_t)1);
    XR_LAUNCH("pg_fill_i64", k_pg_fill_i64, dim3(1), dim3(PB), 0, p->polygon_offsets.get(), (int64_t)0, (int64_t)1);
}

static void polygonize(xr_topology *t, const void *data_dev, int dtype, xr_polygons *p) {
    const xr_mesh *mesh = t->mesh;
    const int64_t F = t->n_face, E = t->n_edge;
    const int m = t->m;
    const int64_t n_slot = F * m;
    const int32_t *faces = mesh->faces_raw.get();
    const double *node_xy = mesh->node_xy.get();
    p->n_face = F;
    p->face_polygon.alloc((size_t)std::max<int64_t>(F, 1));
    if (F == 0) return polygons_empty(p);
    const unsigned fb = div_up(F, PB);

    // 1
    DevBuf<double> val((size_t)F);
    DevBuf<int8_t> orient((size_t)F);
    DevBuf<int32_t> parent((size_t)F), flags(PG_COUNT);
    fill_i32(flags.get(), 0, PG_COUNT);
    if (dtype == XR_F64)
        XR_LAUNCH("pg_prepare", k_pg_prepare<double>, dim3(fb), dim3(PB), 0, (const double *)data_dev, faces, m, node_xy, F, val.get(),
                  orient.get(), parent.get(), flags.get());
    else if (dtype == XR_F32)
        XR_LAUNCH("pg_prepare", k_pg_prepare<float>, dim3(fb), dim3(PB), 0, (const float *)data_dev, faces, m, node_xy, F, val.get(),
                  orient.get(), parent.get(), flags.get());
    else
        XR_LAUNCH("pg_prepare", k_pg_prepare<int32_t>, dim3(fb), dim3(PB), 0, (const int32_t *)data_dev, faces, m, node_xy, F,
                  val.get(), orient.get(), parent.get(), flags.get());

    // 2 (one read-back of the flag words per round)
    int32_t h_flags[PG_COUNT];
    for (;;) {
        fill_i32(flags.get() + PG_CHANGED, 0, 1);
        if (E > 0)
            XR_LAUNCH("pg_hook", k_pg_hook, dim3(div_up(E, PB)), dim3(PB), 0, t->edge_face.get(), E, val.get(), orient.get(),
                      parent.get(), flags.get());
        XR_LAUNCH("pg_compress", k_pg_compress, dim3(fb), dim3(PB), 0, parent.get(), F);
        p->label_rounds++;
        d2h(h_flags, flags.get(), sizeof(h_flags));
        p->readbacks++;
        XR_REQUIRE(h_flags[PG_DEGENERATE] == 0, XR_ERR_INVALID,
                   "xr_polygonize_dev: degenerate face: %d faces with data have a shoelace sum that is zero or not finite",
                   (int)h_flags[PG_DEGENERATE]);
        if (!h_flags[PG_CHANGED]) break;
    }

    // 3
    DevBuf<int32_t> flag((size_t)std::max<int64_t>(n_slot, F)), rank((size_t)F + 1), region((size_t)F);
    XR_LAUNCH("pg_region_flag", k_pg_region_flag, dim3(fb), dim3(PB), 0, parent.get(), orient.get(), F, flag.get());
    exclusive_scan_i32(flag.get(), rank.get(), F);
    const int64_t P = read_scalar(rank.get() + F);
    p->readbacks++;
    p->n_polygon = P;
    p->values.alloc((size_t)std::max<int64_t>(P, 1));
    XR_LAUNCH("pg_region_number", k_pg_region_number, dim3(fb), dim3(PB), 0, parent.get(), orient.get(), rank.get(), val.get(), F,
              region.get(), p->face_polygon.get(), p->values.get());
    if (P == 0) return polygons_empty(p);

    // 4
    DevBuf<int32_t> hpos((size_t)n_slot + 1);
    XR_LAUNCH("pg_halfedge_flag", k_pg_halfedge_flag, dim3(div_up(n_slot, PB)), dim3(PB), 0, faces, F, m, t->face_edge.get(),
              t->edge_face.get(), region.get(), flag.get(), flags.get());
    exclusive_scan_i32(flag.get(), hpos.get(), n_slot);
    const int64_t H = read_scalar(hpos.get() + n_slot);
    p->readbacks++;
    XR_REQUIRE(H > 0, XR_ERR_INVALID, "xr_polygonize_dev: internal error: %lld regions without a boundary", (long long)P);
    p->n_halfedge = H;
    const unsigned hb = div_up(H, PB);
    DevBuf<int32_t> he_slot((size_t)H), succ((size_t)H);
    XR_LAUNCH("pg_compact", k_compact_ids<int32_t>, dim3(div_up(n_slot, PB)), dim3(PB), 0, flag.get(), hpos.get(), n_slot, he_slot.get());

    // 5
    XR_LAUNCH("pg_successor", k_pg_successor, dim3(hb), dim3(PB), 0, he_slot.get(), H, faces, m, t->face_edge.get(),
              t->edge_face.get(), orient.get(), flag.get(), hpos.get(), t->nf_ptr.get(), succ.get(), flags.get());

    // 6 (no read-back per round: the number of rounds follows from H)
    const int rounds = doubling_rounds(H);
    DevBuf<int32_t> nxt_a((size_t)H), nxt_b((size_t)H), acc_a((size_t)H), acc_b((size_t)H), leader((size_t)H), dist((size_t)H);
    {
        DevBuf<int32_t> indeg((size_t)H);
        fill_i32(indeg.get(), 0, H);
        XR_LAUNCH("pg_indegree", k_pg_indegree, dim3(hb), dim3(PB), 0, succ.get(), H, indeg.get());
        XR_LAUNCH("pg_leader_init", k_pg_leader_init, dim3(hb), dim3(PB), 0, indeg.get(), succ.get(), H, nxt_a.get(), acc_a.get(),
                  flags.get());
    }
    int32_t *nxt = nxt_a.get(), *nxt_o = nxt_b.get(), *acc = acc_a.get(), *acc_o = acc_b.get();
    for (int k = 0; k < rounds; k++) {
        XR_LAUNCH("pg_leader_round", k_pg_leader_round, dim3(hb), dim3(PB), 0, nxt, acc, H, nxt_o, acc_o);
        std::swap(nxt, nxt_o), std::swap(acc, acc_o);
    }
    XR_HIP(hipMemcpyAsync(leader.get(), acc, sizeof(int32_t) * (size_t)H, hipMemcpyDeviceToDevice, launch_stream()));
    XR_LAUNCH("pg_dist_init", k_pg_dist_init, dim3(hb), dim3(PB), 0, succ.get(), leader.get(), H, nxt, acc);
    for (int k = 0; k < rounds; k++) {
        XR_LAUNCH("pg_dist_round", k_pg_dist_round, dim3(hb), dim3(PB), 0, nxt, acc, H, nxt_o, acc_o);
        std::swap(nxt, nxt_o), std::swap(acc, acc_o);
    }
    XR_HIP(hipMemcpyAsync(dist.get(), acc, sizeof(int32_t) * (size_t)H, hipMemcpyDeviceToDevice, launch_stream()));

    // 7
    DevBuf<int32_t> ring_rank((size_t)H + 1);
    XR_LAUNCH("pg_ring_flag", k_pg_ring_flag, dim3(hb), dim3(PB), 0, leader.get(), H, nxt_o);
    exclusive_scan_i32(nxt_o, ring_rank.get(), H);
    int32_t h_ring[2];
    d2h(h_ring, ring_rank.get() + H, sizeof(int32_t));
    d2h(h_flags, flags.get(), sizeof(h_flags));
    p->readbacks += 2;
    const int64_t R = h_ring[0];
    XR_REQUIRE(!h_flags[PG_WALK] && !h_flags[PG_PERMUTATION], XR_ERR_INVALID,
               "xr_polygonize_dev: internal error: the boundary half-edges do not close into rings (walk %d, permutation %d)",
               (int)h_flags[PG_WALK], (int)h_flags[PG_PERMUTATION]);
    XR_REQUIRE(R > 0 && R <= H, XR_ERR_INVALID, "xr_polygonize_dev: internal error: %lld rings of %lld half-edges", (long long)R,
               (long long)H);
    p->n_ring = R;
    p->n_vertex = H + R;
    DevBuf<int32_t> ring_len((size_t)R), ring_poly((size_t)R), ring_sign((size_t)R), ring_start((size_t)R + 1), listed((size_t)H);
    XR_LAUNCH("pg_ring_table", k_pg_ring_table, dim3(hb), dim3(PB), 0, leader.get(), ring_rank.get(), dist.get(), he_slot.get(),
              region.get(), m, H, ring_len.get(), ring_poly.get());
    exclusive_scan_i32(ring_len.get(), ring_start.get(), R);
    fill_i32(listed.get(), 0, H); // (on a permutation every entry is written; a broken one must still leave the sign kernel in range)
    XR_LAUNCH("pg_ring_list", k_pg_ring_list, dim3(hb), dim3(PB), 0, leader.get(), ring_rank.get(), dist.get(), ring_start.get(), H,
              listed.get(), flags.get());
    XR_LAUNCH("pg_ring_sign", k_pg_ring_sign, dim3(div_up(R, PB / 64)), dim3(PB), 0, listed.get(), ring_start.get(), R, he_slot.get(),
              faces, m, orient.get(), node_xy, ring_sign.get());

    // 8: the ring table to the host and its order back
    std::vector<int32_t> h_poly((size_t)R), h_sign((size_t)R), h_len((size_t)R), h_pos((size_t)R);
    std::vector<int64_t> h_ring_offsets((size_t)R + 1), h_polygon_offsets((size_t)P + 1);
    d2h(h_poly.data(), ring_poly.get(), sizeof(int32_t) * (size_t)R);
    d2h(h_sign.data(), ring_sign.get(), sizeof(int32_t) * (size_t)R);
    d2h(h_len.data(), ring_len.get(), sizeof(int32_t) * (size_t)R);
    d2h(h_flags, flags.get(), sizeof(h_flags));
    p->readbacks += 4;
    XR_REQUIRE(!h_flags[PG_PERMUTATION], XR_ERR_INVALID, "xr_polygonize_dev: internal error: a half-edge lies outside its ring");
    const int64_t bad = polygonize_order_rings(R, P, h_poly.data(), h_sign.data(), h_len.data(), h_pos.data(), h_ring_offsets.data(),
                                               h_polygon_offsets.data());
    XR_REQUIRE(bad >= 0, XR_ERR_INVALID, "xr_polygonize_dev: internal error: ring %lld has no polygon or no segment", (long long)(-1 - bad));
    XR_REQUIRE(bad == 0, XR_ERR_INVALID, "xr_polygonize_dev: internal error: region %lld has other than exactly one exterior ring",
               (long long)(bad - 1));
    XR_REQUIRE(h_ring_offsets[(size_t)R] == H + R, XR_ERR_INVALID, "xr_polygonize_dev: internal error: ring lengths do not sum up");
    DevBuf<int32_t> new_pos((size_t)R);
    p->ring_offsets.alloc((size_t)R + 1), p->polygon_offsets.alloc((size_t)P + 1), p->coords.alloc(2 * (size_t)(H + R));
    h2d(new_pos.get(), h_pos.data(), sizeof(int32_t) * (size_t)R);
    h2d(p->ring_offsets.get(), h_ring_offsets.data(), sizeof(int64_t) * ((size_t)R + 1));
    h2d(p->polygon_offsets.get(), h_polygon_offsets.data(), sizeof(int64_t) * ((size_t)P + 1));

    // 9
    XR_LAUNCH("pg_gather", k_pg_gather, dim3(hb), dim3(PB), 0, leader.get(), ring_rank.get(), dist.get(), new_pos.get(),
              p->ring_offsets.get(), he_slot.get(), faces, m, orient.get(), node_xy, H, p->coords.get());
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_polygonize_dev(xr_topology *topology, const void *data_dev, int dtype, xr_polygons **out) {
    XR_API_BEGIN
    XR_REQUIRE(topology && out, XR_ERR_INVALID, "xr_polygonize_dev: NULL argument");
    XR_REQUIRE(topology->n_nonmanifold == 0, XR_ERR_INVALID, "xr_polygonize_dev: the mesh has %lld edges with more than two faces",
               (long long)topology->n_nonmanifold);
    XR_REQUIRE(dtype == XR_F64 || dtype == XR_F32 || dtype == XR_I32, XR_ERR_INVALID, "xr_polygonize_dev: unsupported dtype id %d", dtype);
    XR_REQUIRE(data_dev || topology->n_face == 0, XR_ERR_INVALID, "xr_polygonize_dev: NULL data");
    Building<xr_polygons> p(OnFailure::WaitFirst);
    polygonize(topology, data_dev, dtype, p.get());
    stream_sync(); // (the scratch goes back to the pool behind its readers)
    *out = p.release();
    XR_API_END
}

int xr_polygons_info(const xr_polygons *p, int64_t *n_polygon, int64_t *n_ring, int64_t *n_vertex, int64_t *n_halfedge,
                     int64_t *label_rounds) {
    XR_API_BEGIN
    XR_REQUIRE(p, XR_ERR_INVALID, "xr_polygons_info: NULL handle");
    if (n_polygon) *n_polygon = p->n_polygon;
    if (n_ring) *n_ring = p->n_ring;
    if (n_vertex) *n_vertex = p->n_vertex;
    if (n_halfedge) *n_halfedge = p->n_halfedge;
    if (label_rounds) *label_rounds = p->label_rounds;
    XR_API_END
}

int xr_polygons_readbacks(const xr_polygons *p, int64_t *readbacks) {
    XR_API_BEGIN
    XR_REQUIRE(p && readbacks, XR_ERR_INVALID, "xr_polygons_readbacks: NULL argument");
    *readbacks = p->readbacks;
    XR_API_END
}

int xr_polygons_copy_dev(const xr_polygons *p, double *coords_dev, int64_t *ring_offsets_dev, int64_t *polygon_offsets_dev,
                         double *values_dev, int64_t *face_polygon_dev) {
    XR_API_BEGIN
    XR_REQUIRE(p, XR_ERR_INVALID, "xr_polygons_copy_dev: NULL handle");
    const auto copy = [](void *dst, const void *src, size_t bytes) {
        if (dst && bytes) XR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, launch_stream()));
    };
    copy(coords_dev, p->coords.get(), sizeof(double) * 2 * (size_t)p->n_vertex);
    copy(ring_offsets_dev, p->ring_offsets.get(), sizeof(int64_t) * ((size_t)p->n_ring + 1));
    copy(polygon_offsets_dev, p->polygon_offsets.get(), sizeof(int64_t) * ((size_t)p->n_polygon + 1));
    copy(values_dev, p->values.get(), sizeof(double) * (size_t)p->n_polygon);
    copy(face_polygon_dev, p->face_polygon.get(), sizeof(int64_t) * (size_t)p->n_face);
    dev_call_done();
    XR_API_END
}

int xr_polygons_destroy(xr_polygons *p) {
    XR_API_BEGIN
    if (p) {
        release_point();
        delete p;
    }
    XR_API_END
}

} // extern "C"
