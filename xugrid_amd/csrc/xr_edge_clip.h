// xr_edge_clip.h -- the Cyrus-Beck clip of a segment against one convex face: the ONE copy of the piece arithmetic.  xr_edges.hip
// (the weights of NetworkGridder, intersect_edges) and xr_snapgrid.hip (snap_to_grid) both recompute pieces with it, so their
// end points agree bit for bit with each other and with oracle/xr_oracle.c (cyrus_beck_clip).
#pragma once
#include "xr_geom.h"

namespace xr {

// a + t (b - a), t in [0, 1], against every half-plane of the CCW polygon.  -> length of the clipped piece, or -1;
// its end points in c / d when asked for
__device__ __forceinline__ double cyrus_beck_length(const double *__restrict__ poly, int n, P2 a, P2 b,
                                                    P2 *c = nullptr, P2 *d = nullptr) {
    const double sx = b.x - a.x, sy = b.y - a.y;
    double t0 = 0.0, t1 = 1.0;
    P2 v0 = load_p2(poly, 0);
    for (int i = 0; i < n; i++) {
        const P2 v1 = load_p2(poly, (i + 1 < n) ? i + 1 : 0);
        const double wx = v1.x - v0.x, wy = v1.y - v0.y;
        if (wx != 0.0 || wy != 0.0) {
            const double nx = -wy, ny = wx; // inward normal of a CCW polygon
            const double den = nx * sx + ny * sy;
            const double num = nx * (v0.x - a.x) + ny * (v0.y - a.y);
            if (den == 0.0) {
                if (num > 0.0) return -1.0; // parallel and outside
            } else {
                const double t = num / den;
                if (den > 0.0) {
                    if (t > t0) t0 = t;
                } else {
                    if (t < t1) t1 = t;
                }
            }
        }
        v0 = v1;
    }
    if (!(t0 < t1)) return -1.0;
    const double cx = a.x + t0 * sx, cy = a.y + t0 * sy;
    const double dx = a.x + t1 * sx, dy = a.y + t1 * sy;
    if (c) {
        *c = P2{cx, cy};
        *d = P2{dx, dy};
    }
    const double ex = dx - cx, ey = dy - cy;
    return sqrt(ex * ex + ey * ey);
}

} // namespace xr
