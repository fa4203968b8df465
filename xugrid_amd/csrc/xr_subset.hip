// xr_subset.hip -- cutting a sub-mesh out of a device mesh (Ugrid2d.topology_subset, ugrid2d.py:1138-1216; isel, :1228-1288;
// clip_box, :1218-1226) and the index arithmetic around it, where the mesh is.  DESIGN section 14.
//
// The rule (restated in include/xugrid_amd.h): the faces of the sub-mesh are faces[index] in the order given, the table keeps
// its width and the caller's vertex order; its nodes are the distinct nodes of those faces in ascending old id, renumbered by
// their dense rank; coordinates are copied.  No sort: "distinct, ascending" is a flag per old node (every writer stores the
// same 1), an exclusive scan of the flags (the dense rank) and a compaction -- the one pattern behind every index this unit
// hands out (`index_from_flags`).  No float atomics; the only atomics are one integer add per WAVE that saw a bad or a
// repeated id, i.e. none on a valid call.
//
// Nothing is read through an id before the id has been compared with its range: the kernels that follow the marking pass
// repeat the comparison instead of trusting a verdict the host has not seen yet (they are enqueued behind the read-back).
#include <algorithm>

#include "xr_index.h"
#include "xr_objects.h"
#include "xr_prims.h"
#include "xr_topology.h"

namespace xr {

enum SubsetStatus : int { SS_RANGE = 0, SS_REPEAT = 1, SS_MOVED = 2, SS_COUNT = 3 };

// 1: one thread per i.  pos[index[i]] = i + 1 (pos is zero at the start: 0 = not selected; of a repeated id one writer wins,
// the others find out in the next pass); ids outside [0, size) are counted, never used; status[SS_MOVED] = 1 when some
// index[i] != i (every writer stores the same value).
__global__ void __launch_bounds__(256)
k_subset_mark(const int64_t *__restrict__ index, int64_t n, int64_t size, int32_t *__restrict__ pos, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const int64_t f = index[i];
        bad = f < 0 || f >= size;
        if (!bad) pos[f] = (int32_t)(i + 1);
        if (f != i) status[SS_MOVED] = 1;
    }
    wave_count(bad, status + SS_RANGE);
}

// i lost the race for pos[index[i]]: its id occurs more than once
__device__ __forceinline__ bool subset_repeated(const int64_t *__restrict__ index, int64_t i, int64_t size, const int32_t *__restrict__ pos) {
    const int64_t f = index[i];
    return f >= 0 && f < size && pos[f] != (int32_t)(i + 1);
}

// 1b (an index that selects no faces by itself -- a node or an edge indexer): the repeats, one thread per i
__global__ void __launch_bounds__(256)
k_subset_repeats(const int64_t *__restrict__ index, int64_t n, int64_t size, const int32_t *__restrict__ pos, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    wave_count(i < n && subset_repeated(index, i, size, pos), status + SS_REPEAT);
}

// 2: one thread per (i, slot): the slot-0 thread counts a repeat; every real slot flags its node (all writers store 1)
__global__ void __launch_bounds__(256)
k_subset_flag_nodes(const int64_t *__restrict__ index, int64_t n, int64_t n_face, int m, const int32_t *__restrict__ faces_raw,
                    const int32_t *__restrict__ pos, int32_t *__restrict__ node_flag, int32_t *__restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool repeat = false;
    if (t < n * m) {
        const int64_t i = t / m;
        const int slot = (int)(t - i * m);
        const int64_t f = index[i];
        if (f >= 0 && f < n_face) {
            if (slot == 0) repeat = pos[f] != (int32_t)(i + 1);
            const int v = faces_raw[f * m + slot];
            if (v >= 0) node_flag[v] = 1;
        }
    }
    wave_count(repeat, status + SS_REPEAT);
}

// 4: one thread per old node: a flagged node goes to its dense rank with its 16 bytes of coordinates
__global__ void __launch_bounds__(256)
k_subset_nodes(const int32_t *__restrict__ node_flag, const int32_t *__restrict__ node_new, int64_t n_node,
               const double *__restrict__ node_xy, int32_t *__restrict__ sub_node, double *__restrict__ sub_xy) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_node || !node_flag[v]) return;
    const int j = node_new[v];
    sub_node[j] = (int32_t)v;
    reinterpret_cast<double2 *>(sub_xy)[j] = reinterpret_cast<const double2 *>(node_xy)[v];
}

// 5: one thread per (i, slot) of the new table: consecutive lanes write consecutive words
__global__ void __launch_bounds__(256)
k_subset_faces(const int64_t *__restrict__ index, int64_t n, int64_t n_face, int m, const int32_t *__restrict__ faces_raw,
               const int32_t *__restrict__ node_new, int32_t *__restrict__ sub_faces) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * m) return;
    const int64_t i = t / m;
    const int64_t f = index[i];
    if (f < 0 || f >= n_face) return; // (the call fails: the table is never handed out)
    const int v = faces_raw[f * m + (t - i * m)];
    sub_faces[t] = v < 0 ? -1 : node_new[v];
}

// ---- flags of the other selections
__global__ void __launch_bounds__(256) k_mask_flags(const uint8_t *__restrict__ mask, int64_t n, int32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = mask[i] != 0;
}

// the four comparisons of locate_bounding_box; a NaN centroid fails them
__global__ void __launch_bounds__(256)
k_box_flags(const double *__restrict__ cxy, int64_t n_face, double xmin, double ymin, double xmax, double ymax, int32_t *__restrict__ flags) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    const double2 c = reinterpret_cast<const double2 *>(cxy)[f];
    flags[f] = c.x >= xmin && c.x < xmax && c.y >= ymin && c.y < ymax;
}

// one thread per (i, slot) of face_edge[index]: the edges of the selected faces
__global__ void __launch_bounds__(256)
k_edge_flags(const int64_t *__restrict__ index, int64_t n, int64_t n_face, int m, const int32_t *__restrict__ face_edge,
             int32_t *__restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * m) return;
    const int64_t i = t / m;
    const int64_t f = index[i];
    if (f < 0 || f >= n_face) return;
    const int e = face_edge[f * m + (t - i * m)];
    if (e >= 0) flags[e] = 1;
}

// one thread per face: a face with a flagged node
__global__ void __launch_bounds__(256)
k_faces_of_nodes(const int32_t *__restrict__ faces_raw, int64_t n_face, int m, const int32_t *__restrict__ node_flag,
                 int32_t *__restrict__ flags) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int hit = 0;
    for (int k = 0; k < m; k++) {
        const int v = faces_raw[f * m + k];
        if (v >= 0) hit |= node_flag[v];
    }
    flags[f] = hit != 0;
}

// one thread per selected edge: both columns of edge_face (flags zero at the start)
__global__ void __launch_bounds__(256)
k_faces_of_edges(const int64_t *__restrict__ index, int64_t n, int64_t n_edge, const int32_t *__restrict__ edge_face,
                 int32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t e = index[i];
    if (e < 0 || e >= n_edge) return;
    const int a = edge_face[2 * e], b = edge_face[2 * e + 1];
    if (a >= 0) flags[a] = 1;
    if (b >= 0) flags[b] = 1;
}

__global__ void __launch_bounds__(256)
k_index_mismatch(const int64_t *__restrict__ a, const int64_t *__restrict__ b, int64_t n, int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    wave_count(i < n && a[i] != b[i], count);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_mesh_subset_dev(xr_mesh *mesh, const int64_t *face_index_dev, int64_t n, xr_mesh **out, int *is_identity, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out && is_identity && problems && (face_index_dev || n == 0), XR_ERR_INVALID, "xr_mesh_subset_dev: NULL argument");
    const int64_t F = mesh->n_face, N = mesh->n_node;
    const int m = mesh->m;
    XR_REQUIRE(n >= 0 && n <= F, XR_ERR_INVALID, "index size %lld is larger than dimension size: %lld", (long long)n, (long long)F);
    XR_REQUIRE(n * m < ((int64_t)1 << 31), XR_ERR_LIMIT, "xr_mesh_subset_dev: %lld face slots exceed the int32 index range", (long long)(n * m));
    *out = nullptr;
    *is_identity = 0;
    problems[0] = problems[1] = 0;
    Building<xr_mesh> sub(OnFailure::WaitFirst);
    sub->m = m;
    sub->is_subset = true;
    int32_t h[1 + SS_COUNT] = {0, 0, 0, 0}; // node total, then the status words
    if (n > 0) {
        // one block: [node_new: N + 1][status: SS_COUNT][.. to a multiple of 4 words][node_flag: N][pos: F]; everything behind
        // node_new starts as zero (one fill), node_new[N] and the status words come back in one copy
        const int64_t flag_at = (N + 1 + SS_COUNT + 3) / 4 * 4;
        DevBuf<int32_t> work((size_t)(flag_at + N + F));
        int32_t *node_new = work.get(), *status = work.get() + N + 1, *node_flag = work.get() + flag_at, *pos = node_flag + N;
        fill_i32(status, 0, flag_at - (N + 1) + N + F);
        XR_LAUNCH("subset_mark", k_subset_mark, dim3(div_up(n, 256)), dim3(256), 0, face_index_dev, n, F, pos, status);
        XR_LAUNCH("subset_flag_nodes", k_subset_flag_nodes, dim3(div_up(n * m, 256)), dim3(256), 0, face_index_dev, n, F, m,
                  mesh->faces_raw.get(), pos, node_flag, status);
        exclusive_scan_i32(node_flag, node_new, N);
        sub->faces_raw.alloc((size_t)(n * m));
        // (the new table needs the ranks, not their number: it is written while the number travels)
        d2h(h, node_new + N, sizeof(h), [&] {
            XR_LAUNCH("subset_faces", k_subset_faces, dim3(div_up(n * m, 256)), dim3(256), 0, face_index_dev, n, F, m,
                      mesh->faces_raw.get(), node_new, sub->faces_raw.get());
        });
        problems[0] = h[1 + SS_RANGE];
        problems[1] = h[1 + SS_REPEAT];
        if (problems[0] || problems[1] || (n == F && !h[1 + SS_MOVED])) {
            *is_identity = !problems[0] && !problems[1];
            stream_sync();
            return XR_OK; // (`sub` is freed on the way out)
        }
        const int64_t Nn = h[0];
        sub->n_node = Nn;
        sub->n_face = n;
        sub->node_xy.alloc((size_t)Nn * 2);
        sub->sub_node.alloc((size_t)Nn);
        XR_LAUNCH("subset_nodes", k_subset_nodes, dim3(div_up(N, 256)), dim3(256), 0, node_flag, node_new, N, mesh->node_xy.get(),
                  sub->sub_node.get(), sub->node_xy.get());
        stream_sync(); // (`work` goes back to the pool behind its readers)
    } else {
        *is_identity = F == 0;
        if (*is_identity) return XR_OK;
        sub->node_xy.alloc(0), sub->faces_raw.alloc(0), sub->sub_node.alloc(0); // the empty grid: nothing is launched
    }
    *out = sub.release();
    XR_API_END
}

int xr_mesh_subset_node_index_dev(const xr_mesh *subset, int64_t *index_dev) {
    XR_API_BEGIN
    XR_REQUIRE(subset && (index_dev || subset->n_node == 0), XR_ERR_INVALID, "xr_mesh_subset_node_index_dev: NULL argument");
    XR_REQUIRE(subset->is_subset, XR_ERR_INVALID, "xr_mesh_subset_node_index_dev: the mesh was not made by xr_mesh_subset_dev");
    widen_dev(subset->sub_node.get(), subset->n_node, index_dev);
    dev_call_done();
    XR_API_END
}

int xr_index_check_dev(const int64_t *index_dev, int64_t n, int64_t size, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(problems && (index_dev || n == 0) && n >= 0 && size >= 0, XR_ERR_INVALID, "xr_index_check_dev: bad argument");
    XR_REQUIRE(size < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), XR_ERR_LIMIT, "xr_index_check_dev: sizes exceed the int32 index range");
    problems[0] = problems[1] = 0;
    if (n > 0) {
        DevBuf<int32_t> work((size_t)(4 + size)); // [status: SS_COUNT, one word unused][pos: size], zero at the start
        int32_t *status = work.get(), *pos = work.get() + 4;
        fill_i32(work.get(), 0, 4 + size);
        XR_LAUNCH("subset_mark", k_subset_mark, dim3(div_up(n, 256)), dim3(256), 0, index_dev, n, size, pos, status);
        XR_LAUNCH("subset_repeats", k_subset_repeats, dim3(div_up(n, 256)), dim3(256), 0, index_dev, n, size, pos, status);
        int32_t h[SS_COUNT];
        d2h(h, status, sizeof(h));
        problems[0] = h[SS_RANGE], problems[1] = h[SS_REPEAT];
        stream_sync();
    }
    XR_API_END
}

int xr_index_mismatch_dev(const int64_t *a_dev, const int64_t *b_dev, int64_t n, int64_t *count) {
    XR_API_BEGIN
    XR_REQUIRE(count && ((a_dev && b_dev) || n == 0) && n >= 0, XR_ERR_INVALID, "xr_index_mismatch_dev: bad argument");
    *count = 0;
    if (n > 0) {
        DevBuf<int32_t> word(1);
        fill_i32(word.get(), 0, 1);
        XR_LAUNCH("subset_mismatch", k_index_mismatch, dim3(div_up(n, 256)), dim3(256), 0, a_dev, b_dev, n, word.get());
        *count = read_scalar(word.get());
        stream_sync();
    }
    XR_API_END
}

int xr_index_from_mask_dev(const uint8_t *mask_dev, int64_t n, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (mask_dev || n == 0) && n >= 0, XR_ERR_INVALID, "xr_index_from_mask_dev: bad argument");
    XR_REQUIRE(n < ((int64_t)1 << 31), XR_ERR_LIMIT, "xr_index_from_mask_dev: the mask exceeds the int32 index range");
    DevBuf<int32_t> flags((size_t)n);
    if (n > 0) XR_LAUNCH("subset_mask_flags", k_mask_flags, dim3(div_up(n, 256)), dim3(256), 0, mask_dev, n, flags.get());
    *out = index_from_flags(flags.get(), n);
    XR_API_END
}

int xr_mesh_box_faces_dev(xr_mesh *mesh, double xmin, double ymin, double xmax, double ymax, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out, XR_ERR_INVALID, "xr_mesh_box_faces_dev: NULL argument");
    const int64_t F = mesh->n_face;
    DevBuf<int32_t> flags((size_t)F);
    if (F > 0) {
        const auto c = mesh_centroids_shared(mesh);
        XR_LAUNCH("subset_box_flags", k_box_flags, dim3(div_up(F, 256)), dim3(256), 0, c->get(), F, xmin, ymin, xmax, ymax, flags.get());
    }
    *out = index_from_flags(flags.get(), F);
    XR_API_END
}

int xr_mesh_faces_of_nodes_dev(xr_mesh *mesh, const int64_t *node_index_dev, int64_t n, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out && (node_index_dev || n == 0) && n >= 0, XR_ERR_INVALID, "xr_mesh_faces_of_nodes_dev: bad argument");
    const int64_t F = mesh->n_face, N = mesh->n_node;
    DevBuf<int32_t> flags((size_t)F), node_flag((size_t)N);
    fill_i32(node_flag.get(), 0, N);
    if (n > 0) XR_LAUNCH("subset_flag_ids", k_flag_ids, dim3(div_up(n, 256)), dim3(256), 0, node_index_dev, n, N, node_flag.get());
    if (F > 0)
        XR_LAUNCH("subset_faces_of_nodes", k_faces_of_nodes, dim3(div_up(F, 256)), dim3(256), 0, mesh->faces_raw.get(), F, mesh->m,
                  node_flag.get(), flags.get());
    *out = index_from_flags(flags.get(), F);
    XR_API_END
}

int xr_topology_faces_of_edges_dev(const xr_topology *t, const int64_t *edge_index_dev, int64_t n, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(t && out && (edge_index_dev || n == 0) && n >= 0, XR_ERR_INVALID, "xr_topology_faces_of_edges_dev: bad argument");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_faces_of_edges_dev: the mesh has edges with more than two faces");
    const int64_t F = t->n_face;
    DevBuf<int32_t> flags((size_t)F);
    fill_i32(flags.get(), 0, F);
    if (n > 0 && F > 0)
        XR_LAUNCH("subset_faces_of_edges", k_faces_of_edges, dim3(div_up(n, 256)), dim3(256), 0, edge_index_dev, n, t->n_edge,
                  t->edge_face.get(), flags.get());
    *out = index_from_flags(flags.get(), F);
    XR_API_END
}

int xr_topology_subset_edges_dev(const xr_topology *t, const int64_t *face_index_dev, int64_t n, xr_index **out) {
    XR_API_BEGIN
    XR_REQUIRE(t && out && (face_index_dev || n == 0) && n >= 0, XR_ERR_INVALID, "xr_topology_subset_edges_dev: bad argument");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_subset_edges_dev: the mesh has edges with more than two faces");
    XR_REQUIRE(n * t->m < ((int64_t)1 << 31), XR_ERR_LIMIT, "xr_topology_subset_edges_dev: face slots exceed the int32 index range");
    const int64_t E = t->n_edge;
    DevBuf<int32_t> flags((size_t)E);
    fill_i32(flags.get(), 0, E);
    if (n > 0 && E > 0)
        XR_LAUNCH("subset_edge_flags", k_edge_flags, dim3(div_up(n * t->m, 256)), dim3(256), 0, face_index_dev, n, t->n_face, t->m,
                  t->face_edge.get(), flags.get());
    *out = index_from_flags(flags.get(), E);
    XR_API_END
}

int xr_index_info(const xr_index *index, int64_t *n) {
    XR_API_BEGIN
    XR_REQUIRE(index && n, XR_ERR_INVALID, "xr_index_info: NULL argument");
    *n = index->n;
    XR_API_END
}

int xr_index_copy_dev(const xr_index *index, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(index && (out_dev || index->n == 0), XR_ERR_INVALID, "xr_index_copy_dev: NULL argument");
    widen_dev(index->ids.get(), index->n, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_index_destroy(xr_index *index) {
    XR_API_BEGIN
    if (index) {
        release_point();
        delete index;
    }
    XR_API_END
}

} // extern "C"
