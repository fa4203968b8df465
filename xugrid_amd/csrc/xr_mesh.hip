// xr_mesh.hip -- the mesh handle (struct xr_mesh, xr_objects.h): creation from host or device arrays with the ingest of the
// connectivity, sizes, device bytes, invalidation, downloads.  What is computed from a handle lives in the other units of the
// mesh: xr_mesh_front.hip (statistics, preparation), xr_mesh_order.hip (query order, tree index), xr_mesh_derived.hip.
#include <atomic>
#include <vector>

#include "xr_mesh.h"

namespace xr {

Building<xr_mesh> new_raw_mesh(int64_t n_node, int64_t n_face, int m, OnFailure rule) {
    Building<xr_mesh> mesh(rule);
    mesh->n_node = n_node;
    mesh->n_face = n_face;
    mesh->m = m;
    mesh->node_xy.alloc((size_t)n_node * 2);
    mesh->faces_raw.alloc((size_t)n_face * m);
    return mesh;
}

// ingest of the caller's connectivity (xr_mesh_create): fill -> -1, narrow to int32, validate
// err: [0] first face with fewer than 3 nodes, [1] first face with a node id out of range; NO_FACE at launch
static constexpr int64_t NO_FACE = INT64_MAX; // (above every face index for the kernel's unsigned atomicMin as well)
template <typename I>
__global__ void __launch_bounds__(256)
k_ingest_faces(const I *__restrict__ raw, int64_t cnt, int m, int64_t fill_value, int64_t n_node,
               int32_t *__restrict__ out, int64_t *__restrict__ err) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= cnt) return;
    const int64_t v = (int64_t)raw[k];
    const int64_t f = k / m;
    const int j = (int)(k - f * m);
    if (v == fill_value || v == -1) {
        if (j < 3) atomicMin(reinterpret_cast<unsigned long long *>(err), (unsigned long long)f);
        out[k] = -1;
    } else {
        if (v < 0 || v >= n_node) atomicMin(reinterpret_cast<unsigned long long *>(err + 1), (unsigned long long)f);
        out[k] = (int32_t)v;
    }
}

// what xr_mesh_create and xr_mesh_create_dev (`fn`: the one that reports) ask of their arguments
static void check_create_args(const char *fn, const void *node_xy, int64_t n_node, const void *faces, int faces_itemsize,
                              int64_t n_face, int64_t n_max_node, xr_mesh **out) {
    XR_REQUIRE(out != nullptr, XR_ERR_INVALID, "%s: out is NULL", fn);
    XR_REQUIRE(n_node >= 0 && n_face >= 0, XR_ERR_INVALID, "%s: negative sizes", fn);
    XR_REQUIRE(n_max_node >= 3 && n_max_node <= XR_MAX_FACE_NODES, XR_ERR_LIMIT,
               "%s: n_max_node_per_face must be in [3, %d], got %lld", fn, XR_MAX_FACE_NODES, (long long)n_max_node);
    XR_REQUIRE(faces_itemsize == 4 || faces_itemsize == 8, XR_ERR_INVALID, "%s: faces_itemsize must be 4 or 8", fn);
    XR_REQUIRE(n_node < ((int64_t)1 << 31) && n_face * n_max_node < ((int64_t)1 << 31), XR_ERR_LIMIT,
               "%s: mesh exceeds the int32 index range", fn);
    XR_REQUIRE((node_xy && faces) || n_face == 0, XR_ERR_INVALID, "%s: NULL arrays", fn);
}

// the first offending face of an ingest, too short before out of range
static void report_bad_face(const char *fn, int64_t first_short, int64_t first_node, int64_t n_node) {
    XR_REQUIRE(first_short == NO_FACE, XR_ERR_INVALID, "%s: face %lld has fewer than 3 nodes", fn, (long long)first_short);
    XR_REQUIRE(first_node == NO_FACE, XR_ERR_INVALID, "%s: face %lld references a node outside [0,%lld)", fn,
               (long long)first_node, (long long)n_node);
}

// device-side ingest: the caller's connectivity in device memory -> mesh->faces_raw, validated (waits for the verdict)
static void ingest_faces_dev(const char *fn, xr_mesh *mesh, const void *raw_dev, int faces_itemsize, int64_t fill_value) {
    const int64_t cnt = mesh->n_face * mesh->m;
    DevBuf<int64_t> err(2);
    const int64_t none[2] = {NO_FACE, NO_FACE};
    h2d(err.get(), none, sizeof(none));
    const auto launch = [&](auto *raw) {
        XR_LAUNCH("ingest_faces", k_ingest_faces<std::remove_cv_t<std::remove_pointer_t<decltype(raw)>>>, dim3(div_up(cnt, 256)),
                  dim3(256), 0, raw, cnt, mesh->m, fill_value, mesh->n_node, mesh->faces_raw.get(), err.get());
    };
    if (faces_itemsize == 8) launch(static_cast<const int64_t *>(raw_dev));
    else launch(static_cast<const int32_t *>(raw_dev));
    int64_t h_err[2];
    d2h(h_err, err.get(), sizeof(h_err));
    report_bad_face(fn, h_err[0], h_err[1], mesh->n_node);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_mesh_create(const double *node_xy, int64_t n_node, const void *faces, int faces_itemsize, int64_t n_face,
                   int64_t n_max_node, int64_t fill_value, xr_mesh **out) {
    XR_API_BEGIN
    check_create_args("xr_mesh_create", node_xy, n_node, faces, faces_itemsize, n_face, n_max_node, out);
    engine();
    // Ingest on the way to the device.  Both arrays go through the pinned staging buffers in pieces, filled by the host
    // thread pool while the previous piece is in flight (pageable numpy arrays handed to hipMemcpy move at a third of the
    // link rate).  The connectivity is NARROWED while it is copied: fill value -> -1, int64 -> int32 (half the bytes over
    // PCIe), validated (every face has at least three nodes, every node id is inside [0, n_node)); the first offending
    // face is reported.  Nothing waits for the last DMA: the arrays are consumed, later work is stream-ordered behind it.
    const size_t cnt = (size_t)n_face * (size_t)n_max_node;
    // (Meshes of less than 1 MB take the device-side ingest: two plain copies and a kernel, no pinned staging buffers --
    // those are 2 x 64 MiB of pinned host memory, allocated on first use.)
    const bool device_ingest = cnt * (size_t)faces_itemsize + sizeof(double) * 2 * (size_t)n_node < ((size_t)1 << 20);
    Building<xr_mesh> mesh = new_raw_mesh(n_node, n_face, (int)n_max_node);
    if (device_ingest) {
        h2d_big(mesh->node_xy.get(), node_xy, sizeof(double) * 2 * (size_t)n_node);
    } else {
        const char *xy_bytes = reinterpret_cast<const char *>(node_xy);
        h2d_staged(mesh->node_xy.get(), sizeof(double) * 2 * (size_t)n_node, [=](char *dst, size_t off, size_t n) {
            parallel_ranges(n, 64, [=](size_t b, size_t e) { memcpy(dst + b, xy_bytes + off + b, e - b); });
        });
    }
    if (cnt > 0 && !device_ingest) {
        std::atomic<int64_t> bad_short(NO_FACE), bad_node(NO_FACE);
        const int m = (int)n_max_node;
        auto narrow = [&](auto *raw) {
            h2d_staged(mesh->faces_raw.get(), cnt * sizeof(int32_t), [&, raw](char *dst, size_t off, size_t n) {
                int32_t *out32 = reinterpret_cast<int32_t *>(dst);
                const size_t k0 = off / sizeof(int32_t), nk = n / sizeof(int32_t);
                parallel_ranges(nk, 16, [&, raw, out32, k0](size_t b, size_t e) {
                    int64_t first_short = NO_FACE, first_node = NO_FACE;
                    for (size_t i = b; i < e; i++) {
                        const size_t k = k0 + i;
                        const int64_t v = (int64_t)raw[k];
                        if (v == fill_value || v == -1) {
                            if ((int)(k % (size_t)m) < 3 && first_short == NO_FACE) first_short = (int64_t)(k / (size_t)m);
                            out32[i] = -1;
                        } else {
                            if ((v < 0 || v >= n_node) && first_node == NO_FACE) first_node = (int64_t)(k / (size_t)m);
                            out32[i] = (int32_t)v;
                        }
                    }
                    int64_t cur = bad_short.load();
                    while (first_short < cur && !bad_short.compare_exchange_weak(cur, first_short)) {}
                    cur = bad_node.load();
                    while (first_node < cur && !bad_node.compare_exchange_weak(cur, first_node)) {}
                });
            });
        };
        if (faces_itemsize == 8) narrow(static_cast<const int64_t *>(faces));
        else narrow(static_cast<const int32_t *>(faces));
        if (bad_short.load() != NO_FACE || bad_node.load() != NO_FACE) stream_sync(); // (the handle is dropped below)
        report_bad_face("xr_mesh_create", bad_short.load(), bad_node.load(), n_node);
    } else if (cnt > 0) {
        DevBuf<char> raw(cnt * (size_t)faces_itemsize);
        h2d_big(raw.get(), faces, cnt * (size_t)faces_itemsize);
        ingest_faces_dev("xr_mesh_create", mesh.get(), raw.get(), faces_itemsize, fill_value);
    }
    *out = mesh.release();
    XR_API_END
}

int xr_mesh_create_dev(const double *node_xy_dev, int64_t n_node, const void *faces_dev, int faces_itemsize, int64_t n_face,
                       int64_t n_max_node, int64_t fill_value, xr_mesh **out) {
    XR_API_BEGIN
    check_create_args("xr_mesh_create_dev", node_xy_dev, n_node, faces_dev, faces_itemsize, n_face, n_max_node, out);
    engine();
    Building<xr_mesh> mesh = new_raw_mesh(n_node, n_face, (int)n_max_node);
    if (n_node > 0)
        XR_HIP(hipMemcpyAsync(mesh->node_xy.get(), node_xy_dev, sizeof(double) * 2 * (size_t)n_node, hipMemcpyDeviceToDevice,
                              launch_stream()));
    if (n_face > 0) ingest_faces_dev("xr_mesh_create_dev", mesh.get(), faces_dev, faces_itemsize, fill_value);
    else stream_sync();
    *out = mesh.release();
    XR_API_END
}

int xr_mesh_destroy(xr_mesh *mesh) {
    XR_API_BEGIN
    if (mesh) {
        flush_pending_points_of(mesh); // (an xr_points handle made from this mesh whose kernels have not been launched yet)
        release_point();
        delete mesh;
    }
    XR_API_END
}

int xr_mesh_info(const xr_mesh *mesh, int64_t *n_node, int64_t *n_face, int64_t *n_max_node) {
    XR_API_BEGIN
    XR_REQUIRE(mesh, XR_ERR_INVALID, "xr_mesh_info: NULL mesh");
    if (n_node) *n_node = mesh->n_node;
    if (n_face) *n_face = mesh->n_face;
    if (n_max_node) *n_max_node = mesh->m;
    XR_API_END
}

int xr_mesh_device_bytes(const xr_mesh *mesh, int64_t *bytes) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && bytes, XR_ERR_INVALID, "xr_mesh_device_bytes: NULL argument");
    // (not counted, as ever: the statistics' arrival counters, stats.done, and the barycentric cache, bary.ids / bary.cell_flag)
    *bytes = (int64_t)(mesh->MeshRaw::bytes() + mesh->stats.bytes() + mesh->prep.bytes() + mesh->qo.bytes() + mesh->index.bytes() +
                       mesh->centroids.bytes());
    XR_API_END
}

int xr_mesh_invalidate(xr_mesh *mesh) {
    XR_API_BEGIN
    XR_REQUIRE(mesh, XR_ERR_INVALID, "xr_mesh_invalidate: NULL mesh");
    // (the blocks go back to the pool, which hands them out again in stream order on the one main stream: in asynchronous
    // mode nothing has to wait here)
    flush_pending_points_of(mesh); // (an xr_points handle made from this mesh whose kernels have not been launched yet)
    release_point();
    // (what describes the raw mesh stays: the provenance arrays, the barycentric cache)
    mesh->stats.release();
    mesh->prep.release();
    mesh->qo.release();
    mesh->index.release();
    mesh->centroids.release();
    XR_API_END
}

int xr_mesh_download(xr_mesh *mesh, double *node_xy_out, int64_t *faces_out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh, XR_ERR_INVALID, "xr_mesh_download: NULL handle");
    if (node_xy_out && mesh->n_node > 0) d2h(node_xy_out, mesh->node_xy.get(), sizeof(double) * 2 * (size_t)mesh->n_node);
    const int64_t n = mesh->n_face * mesh->m;
    if (faces_out && n > 0) {
        std::vector<int32_t> raw((size_t)n);
        d2h(raw.data(), mesh->faces_raw.get(), sizeof(int32_t) * (size_t)n);
        for (int64_t i = 0; i < n; i++) faces_out[i] = raw[(size_t)i];
    }
    XR_API_END
}

} // extern "C"
