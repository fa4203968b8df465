// xr_clip.h -- device code the clips of both weight-build pipelines use (xr_overlap_general.hip: k_clip, k_clip_small,
// k_clip_tri; xr_overlap_fused.hip: k_clip_tri_queue) and the f32 box test the search shares with them (xr_overlap.hip):
// the reference's pre-clip tests for rounding dust, the Sutherland-Hodgman primitives, the register / LDS clip of small
// polygons and the end of every one-pair-per-thread clip kernel.  (The flag / compaction clip of triangles: xr_clip_tri.h.)
//
// The clip arithmetic mirrors oracle/xr_oracle.c (clip_polygons / sh_polygon_area) operation
// for operation; both are built with -ffp-contract=off, so areas agree bit for bit.
#pragma once
#include "xr_objects.h"
#include "xr_clip_tri.h"
#include "xr_prims.h"

namespace xr {

__device__ __forceinline__ bool rec_hit(float4 b, float qx0, float qx1, float qy0, float qy1) {
    return box_gap(b, qx0, qx1, qy0, qy1) < 0.0f;
}

// ---------------------------------------------------------------------------------------------
// What the reference does with a candidate pair BEFORE it clips (numba_celltree, restated in oracle/xr_oracle.c): the two
// faces' exact boxes must overlap STRICTLY (boxes_intersect, :530) and the separating-axis test must not separate them
// (sat_intersect, :757; touching counts as intersecting).  For faces that overlap properly both tests pass and the engine
// skips them.  They matter where faces merely touch or are degenerate: there the clip returns slivers of 1e-20 ... 1e-36
// that the reference never computes --
//   * a mesh against itself (or a mesh sharing its nodes): neighbours across a corner have boxes that touch, not overlap
//     (23 pairs of 60 394 on a 60k-face Delaunay mesh; the engine's float boxes are supersets and let them through),
//   * zero-area and needle source faces: the clip of a target by a segment leaves rounding dust the SAT rejects.
// A pair that fails either test has faces whose interiors are disjoint up to a penetration of a few ulp(coordinate), so the
// clip's area for it is at most ~1e-15 * |coordinate| * perimeter.  overlap_dust_threshold() bounds that for EVERY pair of
// the two meshes (largest coordinate x the smaller mesh's largest face extent, with a factor of four to spare); the clip kernels run the two
// tests -- on the float64 vertices, fetched again -- only for the lanes whose area is positive and below it: a handful
// per million pairs on unrelated meshes, the touching neighbours on related ones.  The tests' arithmetic is the oracle's
// (order and orientation of the vertices do not enter: min / max of the same products).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pair_passes_box_and_sat(const double2 *__restrict__ a, int na, const double2 *__restrict__ b, int nb) {
    double ax0 = INFINITY, ax1 = -INFINITY, ay0 = INFINITY, ay1 = -INFINITY, bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
    for (int j = 0; j < na; j++) {
        const double2 q = a[j];
        ax0 = fmin(ax0, q.x), ax1 = fmax(ax1, q.x), ay0 = fmin(ay0, q.y), ay1 = fmax(ay1, q.y);
    }
    for (int j = 0; j < nb; j++) {
        const double2 q = b[j];
        bx0 = fmin(bx0, q.x), bx1 = fmax(bx1, q.x), by0 = fmin(by0, q.y), by1 = fmax(by1, q.y);
    }
    if (!(ax0 < bx1 && bx0 < ax1 && ay0 < by1 && by0 < ay1)) return false;
    for (int pass = 0; pass < 2; pass++) {
        const double2 *p = pass ? b : a;
        const int np = pass ? nb : na;
        for (int i = 0; i < np; i++) {
            const double2 v0 = p[i], v1 = p[i + 1 < np ? i + 1 : 0];
            const double nx = -(v1.y - v0.y), ny = v1.x - v0.x; // edge normal
            if (nx == 0 && ny == 0) continue;
            double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
            for (int j = 0; j < na; j++) {
                const double2 q = a[j];
                const double d = nx * q.x + ny * q.y;
                amin = d < amin ? d : amin;
                amax = d > amax ? d : amax;
            }
            for (int j = 0; j < nb; j++) {
                const double2 q = b[j];
                const double d = nx * q.x + ny * q.y;
                bmin = d < bmin ? d : bmin;
                bmax = d > bmax ? d : bmax;
            }
            if (amax < bmin || bmax < amin) return false;
        }
    }
    return true;
}
// -> the pair's area after the reference's pre-clip tests: unchanged, or 0 for rounding dust of a pair they reject
__device__ __forceinline__ double confirm_dust(double area, double dust, bool active, const double2 *__restrict__ a, int na,
                                               const double2 *__restrict__ b, int nb) {
    const bool suspicious = active && area > 0 && area <= dust;
    if (__any(suspicious)) {
        if (suspicious && !pair_passes_box_and_sat(a, na, b, nb)) area = 0.0;
    }
    return area;
}

// ---------------------------------------------------------------------------------------------
// Sutherland-Hodgman clip + fan area.  LDS: two polygon buffers per thread, [vertex][thread].
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sh_inside(P2 p, P2 r, P2 U) { return U.x * (p.y - r.y) > U.y * (p.x - r.x); }

__device__ __forceinline__ bool sh_intersection(P2 a, P2 V, P2 r, P2 N, P2 &out) {
    const double wx = r.x - a.x, wy = r.y - a.y;
    const double nw = N.x * wx + N.y * wy;
    const double nv = N.x * V.x + N.y * V.y;
    if (nv != 0) {
        const double tt = nw / nv;
        out.x = a.x + tt * V.x;
        out.y = a.y + tt * V.y;
        return true;
    }
    return false;
}

static constexpr double AREA_OVERFLOW = -1.0; // sentinel: polygon buffer too small, redo with MAXV=64

// The end of every one-pair-per-thread clip kernel (every lane of the wave must get here): `area` is pair c's clipped area
// or an overflow sentinel, t its target face (-1 in a lane without a pair), tf / sf the two faces' vertices.  Rounding dust is
// confirmed, an overflow counted, the area stored, and the survivors are added to their rows' counts: the pairs of one target
// face are contiguous, so a wave holds a few runs of equal t.
__device__ __forceinline__ void clip_epilogue(double area, double dust, bool active, int64_t c, int t, const double2 *__restrict__ tf,
                                              int nt, const double2 *__restrict__ sf, int ns, double *__restrict__ cand_area,
                                              int32_t *__restrict__ overflow_count, int32_t *__restrict__ nnz_row) {
    area = confirm_dust(area, dust, active, tf, nt, sf, ns);
    if (active) {
        if (area == TRI_AREA_OVERFLOW) {
            area = AREA_OVERFLOW;
            atomicAdd(overflow_count, 1);
        }
        cand_area[c] = area;
    }
    wave_run_add(t, active && area > 0, nnz_row);
}

// Small-polygon variant (query + tree vertices <= MAXV, i.e. triangles / quads): the subject
// polygon lives in REGISTERS (statically indexed, loops fully unrolled and predicated on the
// current length); only the output polygon, whose write index is data dependent, is staged in
// LDS ([vertex][thread]).  Half the LDS of the generic kernel -> twice the resident waves.
// The arithmetic and its order are those of k_clip / the oracle.
// -> the pair's area (AREA_OVERFLOW: more than MAXV vertices; before the confirmation of rounding dust); `out` = the
// thread's LDS column, out[j * BLOCK]
template <int MAXV, int BLOCK>
__device__ __forceinline__ double clip_small_pair(const double2 *__restrict__ tf, int nt, const double *__restrict__ sf, int ns,
                                                  double2 *out) {
    double area = 0.0;
    P2 in[MAXV];
    P2 last{0.0, 0.0};
#pragma unroll
    for (int j = 0; j < MAXV; j++) {
        if (j < nt) {
            const double2 v = tf[j];
            in[j] = P2{v.x, v.y};
            last = in[j];
        }
    }
    int length = nt;
    bool overflow = false, empty = false;
    P2 r = load_p2(sf, ns - 1);
#pragma unroll
    for (int i = 0; i < XR_MAX_FACE_NODES; i++) {
        if (i >= ns) break;
        const P2 sv = load_p2(sf, i);
        const P2 U{sv.x - r.x, sv.y - r.y};
        if (U.x == 0 && U.y == 0) continue;
        const P2 N{-U.y, U.x};
        int n_output = 0;
        P2 a = last;
        bool a_inside = sh_inside(a, r, U);
#pragma unroll
        for (int j = 0; j < MAXV; j++) {
            if (j < length) {
                // flat body: the only nested divergent region is the division of a crossing
                const P2 b = in[j];
                const P2 V{b.x - a.x, b.y - a.y};
                const bool live = !(V.x == 0 && V.y == 0);
                bool b_inside = sh_inside(b, r, U);
                const bool cross = live && (b_inside != a_inside);
                P2 pt{0.0, 0.0};
                bool have_pt = false;
                if (cross) have_pt = sh_intersection(a, V, r, N, pt);
                // S-H emission: entering -> [pt] b ; inside -> b ; leaving -> pt, or (parallel-edge
                // quirk) b, which then counts as inside
                const bool quirk = cross && !b_inside && !have_pt;
                if (cross && have_pt) {
                    out[(n_output < MAXV ? n_output : MAXV) * BLOCK] = make_double2(pt.x, pt.y);
                    n_output++;
                    last = pt;
                }
                b_inside = b_inside || quirk;
                if (live && b_inside) {
                    out[(n_output < MAXV ? n_output : MAXV) * BLOCK] = make_double2(b.x, b.y);
                    n_output++;
                    last = b;
                }
                if (live) {
                    a = b;
                    a_inside = b_inside;
                }
            }
        }
        overflow = n_output > MAXV;
        if (overflow) break;
        if (n_output < 3) {
            empty = true;
            break;
        }
        length = n_output;
#pragma unroll
        for (int j = 0; j < MAXV; j++) {
            if (j < length) {
                const double2 v = out[j * BLOCK];
                in[j] = P2{v.x, v.y};
            }
        }
        r = sv;
    }
    if (overflow) return AREA_OVERFLOW;
    if (!empty) {
        const P2 a0 = in[0];
        double ux = in[1].x - a0.x, uy = in[1].y - a0.y;
#pragma unroll
        for (int i = 2; i < MAXV; i++) {
            if (i < length) {
                const double vx = a0.x - in[i].x, vy = a0.y - in[i].y;
                area += fabs(ux * vy - uy * vx);
                ux = vx;
                uy = vy;
            }
        }
        area = 0.5 * area;
    }
    return area;
}

} // namespace xr
