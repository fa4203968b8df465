// xr_mesh_derived.hip -- quantities and meshes derived from a mesh's raw arrays, in the caller's vertex order: centroids (cached
// on the handle), CCW-normalised connectivity, circumcenters, perimeter, face bounds, the fan triangulation, and the
// rectilinear mesh generated from two vertex arrays.  None of it is on the regridding step's hot path.
#include <algorithm>
#include <cmath>
#include <memory>

#include "xr_mesh.h"
#include "xr_prims.h"

namespace xr {

// CCW-normalised connectivity (xr_mesh_faces; not on the hot path)
__global__ void __launch_bounds__(256) k_faces_ccw(const double *__restrict__ node_xy,
                                                  const int32_t *__restrict__ faces_raw, int64_t n_face, int m,
                                                  int64_t *__restrict__ out, bool caller_order) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int face[XR_MAX_FACE_NODES];
    for (int j = 0; j < m; j++) face[j] = faces_raw[f * m + j];
    int n;
    bool flip;
    face_shape<XR_MAX_FACE_NODES>(node_xy, face, m, n, flip);
    if (caller_order) flip = false; // (fill normalised to -1, vertex order untouched)
    for (int j = 0; j < m; j++) out[f * m + j] = (flip && j < n) ? face[n - 1 - j] : face[j];
}

// ---------------------------------------------------------------------------------------------
// centroids -- connectivity.centroids (connectivity.py:636-664) on the caller's vertex order
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_centroids(const double *__restrict__ node_xy,
                                                  const int32_t *__restrict__ faces_raw, int64_t n_face, int m,
                                                  double *__restrict__ cxy) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const int32_t *face = faces_raw + f * m;
    if (m == 3) {
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < 3; i++) {
            const P2 p = load_p2(node_xy, face[i]);
            sx += p.x;
            sy += p.y;
        }
        cxy[2 * f] = sx / 3.0;
        cxy[2 * f + 1] = sy / 3.0;
        return;
    }
    const int f0 = face[0];
    const P2 p0 = load_p2(node_xy, f0);
    double det = 0.0, sx = 0.0, sy = 0.0;
    for (int i = 0; i < m; i++) {
        const int ia = face[i] < 0 ? f0 : face[i];
        int ib = f0;
        if (i + 1 < m) ib = face[i + 1] < 0 ? f0 : face[i + 1];
        const P2 a = load_p2(node_xy, ia), b = load_p2(node_xy, ib);
        const double ax = a.x - p0.x, ay = a.y - p0.y, bx = b.x - p0.x, by = b.y - p0.y;
        const double d = ax * by - ay * bx;
        det += d;
        sx += (ax + bx) * d;
        sy += (ay + by) * d;
    }
    const double aw = 1.0 / (3.0 * det);
    cxy[2 * f] = aw * sx + p0.x;
    cxy[2 * f + 1] = aw * sy + p0.y;
}

// device-resident variants used by other translation units (no host copy)
void mesh_centroids_dev(xr_mesh *mesh, double *cxy_dev) {
    if (mesh->n_face > 0)
        XR_LAUNCH("centroids", k_centroids, dim3(div_up(mesh->n_face, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), mesh->n_face, mesh->m, cxy_dev);
}

std::shared_ptr<DevBuf<double>> mesh_centroids_shared(xr_mesh *mesh) {
    hipStream_t st = launch_stream();
    if (!mesh->centroids.dev) {
        auto c = std::make_shared<DevBuf<double>>((size_t)std::max<int64_t>(mesh->n_face, 1) * 2);
        mesh_centroids_dev(mesh, c->get());
        if (!mesh->centroids.event) XR_HIP(hipEventCreateWithFlags(&mesh->centroids.event, hipEventDisableTiming));
        XR_HIP(hipEventRecord(mesh->centroids.event, st));
        mesh->centroids.stream = st;
        mesh->centroids.dev = std::move(c);
    } else if (st != mesh->centroids.stream) {
        // (filled on another stream -- a points handle launches on the side stream --: this stream's work comes behind it)
        XR_HIP(hipStreamWaitEvent(st, mesh->centroids.event, 0));
    }
    return mesh->centroids.dev;
}

void mesh_faces_ccw_dev(xr_mesh *mesh, int64_t *faces_dev, bool caller_order) {
    if (mesh->n_face > 0)
        XR_LAUNCH("faces_ccw", k_faces_ccw, dim3(div_up(mesh->n_face, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), mesh->n_face, mesh->m, faces_dev, caller_order);
}

// Ugrid2d.from_structured_bounds -> _from_intervals_helper (xugrid/ugrid/ugrid2d.py:1973-2034, :1894-1912) on the
// device: the (ny + 1) x (nx + 1) vertices of a rectilinear grid (node id = j * (nx + 1) + i, the meshgrid order) and
// one quad per cell (face id = j * nx + i), corners lower-left, lower-right, upper-right, upper-left with "left" and
// "lower" following the direction of the vertex arrays (a descending axis swaps them).
__global__ void __launch_bounds__(256)
k_rect_nodes(const double *__restrict__ xv, const double *__restrict__ yv, int64_t nx1, int64_t n_node,
             double *__restrict__ node_xy) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_node) return;
    const int64_t j = v / nx1, i = v - j * nx1;
    reinterpret_cast<double2 *>(node_xy)[v] = make_double2(xv[i], yv[j]);
}

__global__ void __launch_bounds__(256)
k_rect_faces(int64_t nx, int64_t n_face, bool flip_x, bool flip_y, int32_t *__restrict__ faces) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const int64_t j = f / nx, i = f - j * nx;
    const int64_t left = flip_x ? i + 1 : i, right = flip_x ? i : i + 1;
    const int64_t lower = flip_y ? j + 1 : j, upper = flip_y ? j : j + 1;
    const int64_t nx1 = nx + 1;
    reinterpret_cast<int4 *>(faces)[f] = make_int4((int)(lower * nx1 + left), (int)(lower * nx1 + right),
                                                   (int)(upper * nx1 + right), (int)(upper * nx1 + left));
}

// ---------------------------------------------------------------------------------------------
// quantities and meshes derived from a mesh: fan triangulation (connectivity.py:704-788), circumcenters (:667-701),
// perimeter (:600-612), face bounds (ugrid2d.py:597-619).  All in the caller's vertex order (faces_raw).
// ---------------------------------------------------------------------------------------------
// nodes of a face in faces_raw: up to the first fill value from slot 3 on (mesh creation rejects shorter faces)
__device__ __forceinline__ int raw_face_len(const int32_t *__restrict__ face, int m) {
    int n = m;
    for (int i = m - 1; i >= 3; i--)
        if (face[i] < 0) n = i;
    return n;
}

__global__ void __launch_bounds__(256)
k_tri_count(const int32_t *__restrict__ faces_raw, int64_t n_face, int m, int32_t *__restrict__ count) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f < n_face) count[f] = raw_face_len(faces_raw + f * m, m) - 2;
}

// One thread per slot of the PADDED output (face f, word s of its up to 3 (m - 2) triangle words): the lanes of a wave write
// consecutive words of the triangle table, as k_vor_cells does for the cell table.  Triangle t of a face with k nodes is
// (n0, n[t + 1], n[t + 2]); its k - 2 is read off the scan (off[f + 1] - off[f]), not counted again.  off == nullptr: every
// face is a triangle (off[f] = f).
__global__ void __launch_bounds__(256)
k_tri_scatter(const int32_t *__restrict__ faces_raw, int64_t n_face, int m, const int32_t *__restrict__ off,
              int32_t *__restrict__ triangles, int32_t *__restrict__ tri_face) {
    const int w = 3 * (m - 2);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_face * w) return;
    const int64_t f = i / w;
    const int s = (int)(i - f * w);
    const int t = s / 3, c = s - 3 * t;
    const int32_t *face = faces_raw + f * m;
    const int64_t first = off ? off[f] : f;
    if (t >= (off ? off[f + 1] - (int)first : 1)) return;
    triangles[3 * first + s] = c == 0 ? face[0] : face[t + c];
    if (c == 0) tri_face[first + t] = (int32_t)f;
}

// connectivity._circumcenters_triangle, operation for operation (the library is built with -ffp-contract=off)
__global__ void __launch_bounds__(256)
k_circumcenters(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n_face,
                double *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const P2 a = load_p2(node_xy, faces_raw[3 * f]), b = load_p2(node_xy, faces_raw[3 * f + 1]),
             c = load_p2(node_xy, faces_raw[3 * f + 2]);
    const double a_x = a.x, a_y = a.y, b_x = b.x, b_y = b.y, c_x = c.x, c_y = c.y;
    const double D_inv = 0.5 / (a_y * c_x + b_y * a_x - b_y * c_x - a_y * b_x - c_y * a_x + c_y * b_x);
    const double x = ((a_x - c_x) * (a_x + c_x) + (a_y - c_y) * (a_y + c_y)) * (b_y - c_y) -
                     ((b_x - c_x) * (b_x + c_x) + (b_y - c_y) * (b_y + c_y)) * (a_y - c_y);
    const double y = ((b_x - c_x) * (b_x + c_x) + (b_y - c_y) * (b_y + c_y)) * (a_x - c_x) -
                     ((a_x - c_x) * (a_x + c_x) + (a_y - c_y) * (a_y + c_y)) * (b_x - c_x);
    reinterpret_cast<double2 *>(out)[f] = make_double2(D_inv * x, D_inv * y);
}

// connectivity.perimeter: the closed polygon relative to its first vertex (fill slots and the closing slot repeat vertex 0),
// differences of consecutive slots, sqrt(dx * dx + dy * dy) summed in slot order
__global__ void __launch_bounds__(256)
k_perimeter(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n_face, int m,
            double *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const int32_t *face = faces_raw + f * m;
    const P2 p0 = load_p2(node_xy, face[0]);
    double px = p0.x - p0.x, py = p0.y - p0.y, sum = 0.0;
    for (int j = 1; j <= m; j++) {
        const int v = j < m ? face[j] : -1;
        const P2 q = v < 0 ? p0 : load_p2(node_xy, v);
        const double qx = q.x - p0.x, qy = q.y - p0.y;
        const double dx = qx - px, dy = qy - py;
        sum += sqrt(dx * dx + dy * dy);
        px = qx;
        py = qy;
    }
    out[f] = sum;
}

// Ugrid2d.face_bounds: (min x, min y, max x, max y) over the real nodes
__global__ void __launch_bounds__(256)
k_face_bounds(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n_face, int m,
              double *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const int32_t *face = faces_raw + f * m;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int j = 0; j < m; j++) {
        const int v = face[j];
        if (v < 0) continue;
        const P2 p = load_p2(node_xy, v);
        xmin = fmin(xmin, p.x);
        xmax = fmax(xmax, p.x);
        ymin = fmin(ymin, p.y);
        ymax = fmax(ymax, p.y);
    }
    reinterpret_cast<double4 *>(out)[f] = make_double4(xmin, ymin, xmax, ymax);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_mesh_create_rectilinear(const double *x_vertices, int64_t nx, const double *y_vertices, int64_t ny,
                               xr_mesh **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && x_vertices && y_vertices, XR_ERR_INVALID, "xr_mesh_create_rectilinear: NULL argument");
    XR_REQUIRE(nx >= 1 && ny >= 1, XR_ERR_INVALID, "xr_mesh_create_rectilinear: at least one cell per axis expected");
    const int64_t n_node = (nx + 1) * (ny + 1), n_face = nx * ny;
    XR_REQUIRE((nx + 1) < ((int64_t)1 << 31) / (ny + 1) && n_face * 4 < ((int64_t)1 << 31), XR_ERR_LIMIT,
               "xr_mesh_create_rectilinear: mesh exceeds the int32 index range");
    for (int64_t i = 0; i <= nx; i++)
        XR_REQUIRE(x_vertices[i] == x_vertices[i], XR_ERR_INVALID, "xr_mesh_create_rectilinear: NaN x vertex %lld", (long long)i);
    for (int64_t j = 0; j <= ny; j++)
        XR_REQUIRE(y_vertices[j] == y_vertices[j], XR_ERR_INVALID, "xr_mesh_create_rectilinear: NaN y vertex %lld", (long long)j);
    engine();
    Building<xr_mesh> mesh = new_raw_mesh(n_node, n_face, 4);
    DevBuf<double> xv((size_t)nx + 1), yv((size_t)ny + 1);
    h2d(xv.get(), x_vertices, sizeof(double) * (size_t)(nx + 1));
    h2d(yv.get(), y_vertices, sizeof(double) * (size_t)(ny + 1));
    XR_LAUNCH("rect_nodes", k_rect_nodes, dim3(div_up(n_node, 256)), dim3(256), 0, xv.get(), yv.get(), nx + 1, n_node,
              mesh->node_xy.get());
    // (ugrid2d.py:1904-1909: the tests read the flattened vertex arrays; see _from_intervals_helper in ugrid2d.py)
    XR_LAUNCH("rect_faces", k_rect_faces, dim3(div_up(n_face, 256)), dim3(256), 0, nx, n_face,
              x_vertices[1] < x_vertices[0], y_vertices[1] < y_vertices[0], mesh->faces_raw.get());
    stream_sync();
    *out = mesh.release();
    XR_API_END
}

int xr_mesh_centroids(xr_mesh *mesh, double *centroids_out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && centroids_out, XR_ERR_INVALID, "xr_mesh_centroids: NULL argument");
    const int64_t F = mesh->n_face;
    if (F > 0) {
        const auto c = mesh_centroids_shared(mesh);
        d2h(centroids_out, c->get(), sizeof(double) * 2 * (size_t)F);
        stream_sync();
    }
    XR_API_END
}

int xr_mesh_centroids_dev(xr_mesh *mesh, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (out_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_mesh_centroids_dev: NULL argument");
    if (mesh->n_face > 0) {
        const auto c = mesh_centroids_shared(mesh);
        XR_HIP(hipMemcpyAsync(out_dev, c->get(), sizeof(double) * 2 * (size_t)mesh->n_face, hipMemcpyDeviceToDevice, launch_stream()));
    }
    dev_call_done();
    XR_API_END
}

int xr_mesh_circumcenters_dev(xr_mesh *mesh, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (out_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_mesh_circumcenters_dev: NULL argument");
    XR_REQUIRE(mesh->m == 3, XR_ERR_INVALID, "Circumcenters are only supported for triangular grids");
    if (mesh->n_face > 0)
        XR_LAUNCH("circumcenters", k_circumcenters, dim3(div_up(mesh->n_face, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), mesh->n_face, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_mesh_perimeter_dev(xr_mesh *mesh, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (out_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_mesh_perimeter_dev: NULL argument");
    if (mesh->n_face > 0)
        XR_LAUNCH("perimeter", k_perimeter, dim3(div_up(mesh->n_face, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), mesh->n_face, mesh->m, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_mesh_face_bounds_dev(xr_mesh *mesh, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && (out_dev || mesh->n_face == 0), XR_ERR_INVALID, "xr_mesh_face_bounds_dev: NULL argument");
    if (mesh->n_face > 0)
        XR_LAUNCH("face_bounds", k_face_bounds, dim3(div_up(mesh->n_face, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), mesh->n_face, mesh->m, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_mesh_triangulate(xr_mesh *mesh, xr_mesh **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out, XR_ERR_INVALID, "xr_mesh_triangulate: NULL argument");
    const int64_t F = mesh->n_face, N = mesh->n_node;
    const int m = mesh->m;
    int64_t n_triangle = F;
    DevBuf<int32_t> off;
    if (m != 3 && F > 0) { // count, scan, one counter read back
        DevBuf<int32_t> count((size_t)F);
        off.alloc((size_t)F + 1);
        XR_LAUNCH("tri_count", k_tri_count, dim3(div_up(F, 256)), dim3(256), 0, mesh->faces_raw.get(), F, m, count.get());
        exclusive_scan_i32(count.get(), off.get(), F);
        n_triangle = read_scalar(off.get() + F);
    }
    XR_REQUIRE(n_triangle >= 0 && 3 * n_triangle < ((int64_t)1 << 31), XR_ERR_LIMIT,
               "xr_mesh_triangulate: %lld triangles exceed the int32 index range", (long long)n_triangle);
    Building<xr_mesh> tri = new_raw_mesh(N, n_triangle, 3);
    tri->is_triangulation = true;
    tri->tri_face.alloc((size_t)n_triangle); // (kept whether or not the index is asked for: 4 bytes per triangle)
    if (N > 0) // (the handle owns its arrays)
        XR_HIP(hipMemcpyAsync(tri->node_xy.get(), mesh->node_xy.get(), sizeof(double) * 2 * (size_t)N, hipMemcpyDeviceToDevice,
                              launch_stream()));
    if (n_triangle > 0)
        XR_LAUNCH("tri_scatter", k_tri_scatter, dim3(div_up(F * 3 * (m - 2), 256)), dim3(256), 0, mesh->faces_raw.get(), F, m,
                  m == 3 ? (const int32_t *)nullptr : off.get(), tri->faces_raw.get(), tri->tri_face.get());
    stream_sync();
    *out = tri.release();
    XR_API_END
}

int xr_mesh_triangle_face_dev(const xr_mesh *triangles, int64_t *index_dev) {
    XR_API_BEGIN
    XR_REQUIRE(triangles && (index_dev || triangles->n_face == 0), XR_ERR_INVALID, "xr_mesh_triangle_face_dev: NULL argument");
    XR_REQUIRE(triangles->is_triangulation, XR_ERR_INVALID, "xr_mesh_triangle_face_dev: the mesh was not made by xr_mesh_triangulate");
    widen_dev(triangles->tri_face.get(), triangles->n_face, index_dev);
    dev_call_done();
    XR_API_END
}

int xr_mesh_faces(xr_mesh *mesh, int64_t *faces_out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && faces_out, XR_ERR_INVALID, "xr_mesh_faces: NULL argument");
    const int64_t n = mesh->n_face * mesh->m;
    if (n > 0) {
        DevBuf<int64_t> wide((size_t)n);
        XR_LAUNCH("faces_ccw", k_faces_ccw, dim3(div_up(mesh->n_face, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), mesh->n_face, mesh->m, wide.get(), false);
        d2h(faces_out, wide.get(), sizeof(int64_t) * (size_t)n);
        stream_sync();
    }
    XR_API_END
}

} // extern "C"
