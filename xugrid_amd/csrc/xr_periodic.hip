// xr_periodic.hip -- folding the right column of a device mesh onto the left one and cutting that seam open again
// (Ugrid2d.to_periodic, ugrid2d.py:1392-1462; Ugrid2d.to_nonperiodic, :1464-1572), where the mesh is.  DESIGN section 16.
//
// The wrap asks the question of xr_merge.hip -- "which rows are equal, and which of them came first" -- of ONE mesh's node
// coordinates after every right node was given x = xmin in a working copy: the key table of xr_key_table.h answers it, and the
// flag -> exclusive scan -> compaction pattern around it turns the answer into ids.  The kept nodes take their coordinates
// from the ORIGINAL array, not from the working copy (the reference's quirk).  The unwrap needs no table:
// "distinct, ascending" is a mark per node (every writer stores the same 1), a scan and a compaction, as in xr_subset.hip.
//
// The two boundary sets of the wrap are O(boundary): they are compacted, read back, sorted and compared on the host.  Nothing
// is sorted on the device; there are no float atomics (the bounds are a two-launch reduction with fmin / fmax, exact in any
// order); the only atomics outside the key table are one atomicMin per old edge (the smallest id wins: deterministic) and one
// integer add per wave that saw a miss.  Ids are int32 in HBM and nothing is read through an id that has not been compared
// with its range.
#include <algorithm>
#include <cmath>
#include <vector>

#include "xr_objects.h"
#include "xr_prims.h"
#include "xr_topology.h"

#include "xr_key_table.h"

struct xr_periodic {
    xr_mesh *mesh = nullptr;          // the new mesh until xr_periodic_take_mesh hands it out
    bool wrapped = false;             // made by xr_periodic_wrap_dev (else by xr_periodic_unwrap_dev)
    int64_t n_node_old = 0, n_node_new = 0, n_face = 0, n_edge_index = -1;
    xr::DevBuf<int32_t> node_index;   // [n_node_new] the old node of every new node
    xr::DevBuf<int32_t> node_inverse; // [n_node_old] wrap only: the new node of every old node
    xr::DevBuf<int32_t> edge_index;   // [n_edge_index] after xr_periodic_edges_dev: the old edge of every new edge
    ~xr_periodic() { delete mesh; }
};

namespace xr {

static constexpr int PERIODIC_RANGE_BLOCKS = 1024; // partial results of the bounds reduction (one block folds them)
static constexpr int PERIODIC_REGS = 8;            // faces up to this width are kept in registers
static constexpr double CLOSE_ATOL = 1e-8, CLOSE_RTOL = 1e-5; // np.isclose / np.allclose defaults

// ---- bounds: smallest and largest x (fmin / fmax skip a NaN)
// partial[2 b], partial[2 b + 1] = min, max of the x that block b strides over
__global__ void __launch_bounds__(256) k_periodic_x_range(const double2 *__restrict__ xy, int64_t n, double *__restrict__ partial) {
    __shared__ double lds[2 * 4];
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = xy[i].x;
        lo = fmin(lo, x), hi = fmax(hi, x);
    }
    block_reduce<256, OpMin, OpMax>(lds, lo, hi);
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = lo, partial[2 * blockIdx.x + 1] = hi;
}

// ---- wrap
__device__ __forceinline__ bool is_close(double a, double b) { return fabs(a - b) <= CLOSE_ATOL + CLOSE_RTOL * fabs(b); }

// flags[i] = node i is a left node, flags[n + i] = it is a right node (one array: ONE scan ranks both sets)
__global__ void __launch_bounds__(256)
k_periodic_boundary_flags(const double2 *__restrict__ xy, int64_t n, double xmin, double xmax, int32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = xy[i].x;
    flags[i] = is_close(x, xmin);
    flags[n + i] = is_close(x, xmax);
}

// counts[0], counts[1] = left nodes, left + right nodes: the scan at the two set boundaries, for one read-back
__global__ void k_periodic_boundary_counts(const int32_t *__restrict__ rank, int64_t n, int32_t *__restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counts[0] = rank[n], counts[1] = rank[2 * n];
}

// the y of the left nodes in node order, then the y of the right nodes in node order
__global__ void __launch_bounds__(256)
k_periodic_boundary_y(const double2 *__restrict__ xy, int64_t n, const int32_t *__restrict__ flags, const int32_t *__restrict__ rank,
                      double *__restrict__ ys) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= 2 * n || !flags[j]) return;
    ys[rank[j]] = xy[j < n ? j : j - n].y;
}

// the working copy: every right node at x = xmin
__global__ void __launch_bounds__(256)
k_periodic_working_copy(const double2 *__restrict__ xy, int64_t n, const int32_t *__restrict__ is_right, double xmin, double2 *__restrict__ work) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double2 p = xy[i];
    if (is_right[i]) p.x = xmin;
    work[i] = p;
}

// one thread per slot: a real slot through `inverse`, anything else (the fill) stays -1
__global__ void __launch_bounds__(256)
k_periodic_wrap_faces(const int32_t *__restrict__ faces, int64_t n_slot, int64_t n_node, const int32_t *__restrict__ inverse,
                      int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_slot) return;
    const int32_t v = faces[t];
    out[t] = v >= 0 && v < n_node ? inverse[v] : -1;
}

// ---- unwrap
// one thread per face: top = the largest x over its real slots (np.nanmax: fmax skips a NaN); slot k is periodic when
// top - x > half, strictly (false for a fill slot and for a NaN x); the node of a periodic slot is marked (every writer stores the
// same 1).  M > 0: the row lives in registers (every index is a constant after unrolling); M == 0: any width m, read twice.
template <int M>
__global__ void __launch_bounds__(256)
k_periodic_face_flags(const int32_t *__restrict__ faces, int64_t n_face, int m, const double2 *__restrict__ xy, int64_t n_node, double half,
                      uint8_t *__restrict__ slot_flag, int32_t *__restrict__ node_mark) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    double top = -INFINITY;
    if constexpr (M > 0) {
        int32_t v[M];
        double x[M];
#pragma unroll
        for (int k = 0; k < M; k++) {
            v[k] = faces[f * M + k];
            x[k] = v[k] >= 0 && v[k] < n_node ? xy[v[k]].x : NAN;
            top = fmax(top, x[k]);
        }
#pragma unroll
        for (int k = 0; k < M; k++) {
            const bool periodic = top - x[k] > half;
            slot_flag[f * M + k] = periodic;
            if (periodic) node_mark[v[k]] = 1;
        }
    } else {
        for (int k = 0; k < m; k++) {
            const int32_t v = faces[f * m + k];
            if (v >= 0 && v < n_node) top = fmax(top, xy[v].x);
        }
        for (int k = 0; k < m; k++) {
            const int32_t v = faces[f * m + k];
            const bool periodic = v >= 0 && v < n_node && top - xy[v].x > half;
            slot_flag[f * m + k] = periodic;
            if (periodic) node_mark[v] = 1;
        }
    }
}

// one thread per slot: a periodic slot names the copy of its node, everything else stays (the fill included)
__global__ void __launch_bounds__(256)
k_periodic_unwrap_faces(const int32_t *__restrict__ faces, const uint8_t *__restrict__ slot_flag, int64_t n_slot, int64_t n_node,
                        const int32_t *__restrict__ node_rank, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_slot) return;
    const int32_t v = faces[t];
    out[t] = slot_flag[t] ? (int32_t)n_node + node_rank[v] : v; // (a flagged slot holds an id in range: k_periodic_face_flags)
}

// one thread per old node: its 16 bytes stay where they are; a marked node also goes to n_node + rank as (xmax, y)
__global__ void __launch_bounds__(256)
k_periodic_append_nodes(const double2 *__restrict__ xy, int64_t n_node, const int32_t *__restrict__ node_mark,
                        const int32_t *__restrict__ node_rank, double xmax, double2 *__restrict__ out_xy, int32_t *__restrict__ node_index) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_node) return;
    const double2 p = xy[i];
    out_xy[i] = p;
    node_index[i] = (int32_t)i;
    if (node_mark[i]) {
        const int64_t j = n_node + node_rank[i];
        out_xy[j] = make_double2(xmax, p.y);
        node_index[j] = (int32_t)i;
    }
}

// ---- edges
// the id of edge (a, b) in a topology: row min(a, b) of its node -> node CSR, whose data is the edge id; -1: no such edge
__device__ __forceinline__ int32_t edge_of_pair(int32_t a, int32_t b, int64_t n_node, const int32_t *__restrict__ nn_ptr,
                                                const int32_t *__restrict__ nn_idx, const int32_t *__restrict__ nn_dat) {
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    int32_t id = -1;
    if (lo >= 0 && hi < n_node)
        for (int k = nn_ptr[lo]; k < nn_ptr[lo + 1]; k++)
            if (nn_idx[k] == hi) id = nn_dat[k];
    return id;
}

__device__ __forceinline__ int32_t mapped_node(int32_t v, int64_t n, const int32_t *__restrict__ map) { return v >= 0 && v < n ? map[v] : -1; }

// wrap, one thread per OLD edge: its pair through `inverse` is an edge of the new mesh; index[that edge] = the smallest such old id
// (index starts as INT32_MAX)
__global__ void __launch_bounds__(256)
k_periodic_wrap_edges(const int32_t *__restrict__ edge_node, int64_t n_edge, int64_t n_node_old, const int32_t *__restrict__ inverse,
                      int64_t n_node_new, int64_t n_edge_new, const int32_t *__restrict__ nn_ptr, const int32_t *__restrict__ nn_idx,
                      const int32_t *__restrict__ nn_dat, int32_t *__restrict__ index) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edge) return;
    const int32_t a = mapped_node(edge_node[2 * e], n_node_old, inverse), b = mapped_node(edge_node[2 * e + 1], n_node_old, inverse);
    const int32_t id = edge_of_pair(a, b, n_node_new, nn_ptr, nn_idx, nn_dat);
    if (id >= 0 && id < n_edge_new) atomicMin(index + id, (int32_t)e);
}

// ... and the new edges no old edge came to
__global__ void __launch_bounds__(256) k_periodic_unfilled(const int32_t *__restrict__ index, int64_t n, int32_t *__restrict__ misses) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    wave_count(e < n && index[e] == INT32_MAX, misses);
}

// unwrap, one thread per NEW edge: the old edge of its pair through node_index (-1 and counted when there is none)
__global__ void __launch_bounds__(256)
k_periodic_unwrap_edges(const int32_t *__restrict__ edge_node, int64_t n_edge, int64_t n_node_new, const int32_t *__restrict__ node_index,
                        int64_t n_node_old, int64_t n_edge_old, const int32_t *__restrict__ nn_ptr, const int32_t *__restrict__ nn_idx,
                        const int32_t *__restrict__ nn_dat, int32_t *__restrict__ index, int32_t *__restrict__ misses) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool miss = false;
    if (e < n_edge) {
        const int32_t a = mapped_node(edge_node[2 * e], n_node_new, node_index), b = mapped_node(edge_node[2 * e + 1], n_node_new, node_index);
        int32_t id = edge_of_pair(a, b, n_node_old, nn_ptr, nn_idx, nn_dat);
        if (id >= n_edge_old) id = -1;
        miss = id < 0;
        index[e] = id;
    }
    wave_count(miss, misses);
}

__global__ void __launch_bounds__(256) k_periodic_iota(int64_t n, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = i;
}

// ---- host side
// -> xmin, xmax of the nodes (n_node > 0); one read-back
static void node_x_range(const xr_mesh *mesh, double &xmin, double &xmax) {
    const int64_t N = mesh->n_node;
    const int blocks = (int)std::min<int64_t>(div_up(N, 256), PERIODIC_RANGE_BLOCKS);
    const double2 *xy = reinterpret_cast<const double2 *>(mesh->node_xy.get());
    TwoStageReduce<256, double, OpMin, OpMax> range("periodic_x_range_fold", blocks, [&](double *partial) {
        XR_LAUNCH("periodic_x_range", k_periodic_x_range, dim3(blocks), dim3(256), 0, xy, N, partial);
    });
    double h[2];
    range.read(h);
    xmin = h[0], xmax = h[1];
}

static void face_flags(const xr_mesh *mesh, double half, uint8_t *slot_flag, int32_t *node_mark) {
    const int64_t F = mesh->n_face;
    auto launch = [&](auto tag) {
        constexpr int M = decltype(tag)::value;
        XR_LAUNCH("periodic_face_flags", k_periodic_face_flags<M>, dim3(div_up(F, 256)), dim3(256), 0, mesh->faces_raw.get(), F, mesh->m,
                  reinterpret_cast<const double2 *>(mesh->node_xy.get()), mesh->n_node, half, slot_flag, node_mark);
    };
    switch (mesh->m <= PERIODIC_REGS ? mesh->m : 0) {
    case 3: launch(std::integral_constant<int, 3>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 5: launch(std::integral_constant<int, 5>()); break;
    case 6: launch(std::integral_constant<int, 6>()); break;
    case 7: launch(std::integral_constant<int, 7>()); break;
    case 8: launch(std::integral_constant<int, 8>()); break;
    default: launch(std::integral_constant<int, 0>()); break;
    }
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_periodic_wrap_dev(xr_mesh *mesh, xr_periodic **out, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out && problems, XR_ERR_INVALID, "xr_periodic_wrap_dev: NULL argument");
    const int64_t N = mesh->n_node, F = mesh->n_face;
    const int m = mesh->m;
    XR_REQUIRE(N > 0, XR_ERR_INVALID, "xr_periodic_wrap_dev: the mesh has no nodes");
    XR_REQUIRE(2 * N < INT32_MAX && F * m < INT32_MAX, XR_ERR_LIMIT, "xr_periodic_wrap_dev: %lld nodes / %lld face slots exceed the int32 index range",
               (long long)N, (long long)(F * m));
    *out = nullptr;
    problems[0] = problems[1] = 0;
    const double2 *xy = reinterpret_cast<const double2 *>(mesh->node_xy.get());
    double xmin, xmax;
    node_x_range(mesh, xmin, xmax);

    // the two boundary sets: flags, one scan over both, their y compacted; counts first, then the values
    DevBuf<int32_t> side_flag((size_t)2 * N), side_rank((size_t)2 * N + 1), counts(2);
    DevBuf<double> ys((size_t)2 * N);
    XR_LAUNCH("periodic_boundary_flags", k_periodic_boundary_flags, dim3(div_up(N, 256)), dim3(256), 0, xy, N, xmin, xmax, side_flag.get());
    exclusive_scan_i32(side_flag.get(), side_rank.get(), 2 * N);
    XR_LAUNCH("periodic_boundary_counts", k_periodic_boundary_counts, dim3(1), dim3(64), 0, side_rank.get(), N, counts.get());
    int32_t h_counts[2];
    d2h(h_counts, counts.get(), sizeof(h_counts), [&] {
        XR_LAUNCH("periodic_boundary_y", k_periodic_boundary_y, dim3(div_up(2 * N, 256)), dim3(256), 0, xy, N, side_flag.get(), side_rank.get(),
                  ys.get());
    });
    const int64_t n_left = h_counts[0], n_right = (int64_t)h_counts[1] - h_counts[0];
    XR_REQUIRE(n_left >= 0 && n_right >= 0 && n_left + n_right <= 2 * N, XR_ERR_HIP, "xr_periodic_wrap_dev: boundary counts out of range");
    std::vector<double> h_ys((size_t)(n_left + n_right));
    if (!h_ys.empty()) d2h(h_ys.data(), ys.get(), h_ys.size() * sizeof(double));
    if (n_left != n_right) problems[0] = 1;
    else {
        std::sort(h_ys.begin(), h_ys.begin() + n_left);
        std::sort(h_ys.begin() + n_left, h_ys.end());
        for (int64_t k = 0; k < n_left; k++) {
            const double l = h_ys[(size_t)k], r = h_ys[(size_t)(n_left + k)];
            if (!(std::fabs(l - r) <= CLOSE_ATOL + CLOSE_RTOL * std::fabs(r))) problems[1]++;
        }
    }
    if (problems[0] || problems[1]) {
        stream_sync();
        return XR_OK;
    }

    // nodes: the working copy, first occurrences, rank, inverse; the faces follow while the kept count travels
    Building<xr_periodic> periodic(OnFailure::WaitFirst);
    periodic->wrapped = true;
    periodic->n_node_old = N, periodic->n_face = F;
    DevBuf<double> work((size_t)N * 2);
    DevBuf<int32_t> rep((size_t)N), flag((size_t)N), rank((size_t)N + 1);
    periodic->node_inverse.alloc((size_t)N);
    XR_LAUNCH("periodic_working_copy", k_periodic_working_copy, dim3(div_up(N, 256)), dim3(256), 0, xy, N, side_flag.get() + N, xmin,
              reinterpret_cast<double2 *>(work.get()));
    table_first_occurrence(XYRows{reinterpret_cast<const double2 *>(work.get())}, N, rep.get(), flag.get());
    rank_of_flags(flag.get(), rank.get(), N);
    Building<xr_mesh> wrapped;
    wrapped->m = m, wrapped->n_face = F;
    wrapped->faces_raw.alloc((size_t)(F * m));
    const int64_t Nn = read_scalar(rank.get() + N, [&] {
        XR_LAUNCH("periodic_inverse", k_merge_inverse, dim3(div_up(N, 256)), dim3(256), 0, rep.get(), rank.get(), N, periodic->node_inverse.get());
        if (F > 0)
            XR_LAUNCH("periodic_wrap_faces", k_periodic_wrap_faces, dim3(div_up(F * m, 256)), dim3(256), 0, mesh->faces_raw.get(), F * m, N,
                      periodic->node_inverse.get(), wrapped->faces_raw.get());
    });
    XR_REQUIRE(Nn > 0 && Nn <= N, XR_ERR_HIP, "xr_periodic_wrap_dev: kept node count out of range");
    wrapped->n_node = Nn, periodic->n_node_new = Nn;
    wrapped->node_xy.alloc((size_t)Nn * 2);
    periodic->node_index.alloc((size_t)Nn);
    // (the ORIGINAL coordinates of the kept nodes: the overwrite of the working copy never reaches the result)
    XR_LAUNCH("periodic_compact_xy", k_merge_compact_xy, dim3(div_up(N, 256)), dim3(256), 0, flag.get(), rank.get(), N, xy,
              periodic->node_index.get(), reinterpret_cast<double2 *>(wrapped->node_xy.get()));
    stream_sync(); // (the work arrays go back to the pool behind their readers)
    periodic->mesh = wrapped.release();
    *out = periodic.release();
    XR_API_END
}

int xr_periodic_unwrap_dev(xr_mesh *mesh, double xmax, xr_periodic **out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && out, XR_ERR_INVALID, "xr_periodic_unwrap_dev: NULL argument");
    const int64_t N = mesh->n_node, F = mesh->n_face;
    const int m = mesh->m;
    XR_REQUIRE(N > 0, XR_ERR_INVALID, "xr_periodic_unwrap_dev: the mesh has no nodes");
    XR_REQUIRE(2 * N < INT32_MAX && F * m < INT32_MAX, XR_ERR_LIMIT, "xr_periodic_unwrap_dev: %lld nodes / %lld face slots exceed the int32 index range",
               (long long)N, (long long)(F * m));
    *out = nullptr;
    const double2 *xy = reinterpret_cast<const double2 *>(mesh->node_xy.get());
    double xleft, xright;
    node_x_range(mesh, xleft, xright);
    const double half = 0.5 * (xright - xleft);

    Building<xr_periodic> periodic(OnFailure::WaitFirst);
    periodic->n_node_old = N, periodic->n_face = F;
    DevBuf<uint8_t> slot_flag((size_t)(F * m));
    DevBuf<int32_t> node_mark((size_t)N), node_rank((size_t)N + 1);
    fill_i32(node_mark.get(), 0, N);
    if (F > 0) face_flags(mesh, half, slot_flag.get(), node_mark.get());
    exclusive_scan_i32(node_mark.get(), node_rank.get(), N);
    Building<xr_mesh> unwrapped;
    unwrapped->m = m, unwrapped->n_face = F;
    unwrapped->faces_raw.alloc((size_t)(F * m));
    // (the new table needs the ranks, not their number: it is written while the number travels)
    const int64_t U = read_scalar(node_rank.get() + N, [&] {
        if (F > 0)
            XR_LAUNCH("periodic_unwrap_faces", k_periodic_unwrap_faces, dim3(div_up(F * m, 256)), dim3(256), 0, mesh->faces_raw.get(),
                      slot_flag.get(), F * m, N, node_rank.get(), unwrapped->faces_raw.get());
    });
    XR_REQUIRE(U >= 0 && U <= N, XR_ERR_HIP, "xr_periodic_unwrap_dev: new node count out of range");
    const int64_t Nn = N + U;
    unwrapped->n_node = Nn, periodic->n_node_new = Nn;
    unwrapped->node_xy.alloc((size_t)Nn * 2);
    periodic->node_index.alloc((size_t)Nn);
    XR_LAUNCH("periodic_append_nodes", k_periodic_append_nodes, dim3(div_up(N, 256)), dim3(256), 0, xy, N, node_mark.get(), node_rank.get(), xmax,
              reinterpret_cast<double2 *>(unwrapped->node_xy.get()), periodic->node_index.get());
    stream_sync();
    periodic->mesh = unwrapped.release();
    *out = periodic.release();
    XR_API_END
}

int xr_periodic_edges_dev(xr_periodic *periodic, const xr_topology *old_topology, const xr_topology *new_topology, int64_t *misses) {
    XR_API_BEGIN
    XR_REQUIRE(periodic && old_topology && new_topology && misses, XR_ERR_INVALID, "xr_periodic_edges_dev: NULL argument");
    const xr_topology *o = old_topology, *t = new_topology;
    XR_REQUIRE(o->n_nonmanifold == 0 && o->n_node == periodic->n_node_old, XR_ERR_INVALID,
               "xr_periodic_edges_dev: the old topology is non-manifold or not of the converted mesh");
    XR_REQUIRE(t->n_nonmanifold == 0 && t->n_node == periodic->n_node_new, XR_ERR_INVALID,
               "xr_periodic_edges_dev: the new topology is non-manifold or not of the new mesh");
    const int64_t E_old = o->n_edge, E_new = t->n_edge;
    *misses = 0;
    periodic->n_edge_index = -1;
    DevBuf<int32_t> index((size_t)E_new), count(1);
    fill_i32(count.get(), 0, 1);
    if (E_new > 0) {
        if (periodic->wrapped) {
            fill_i32(index.get(), INT32_MAX, E_new);
            if (E_old > 0)
                XR_LAUNCH("periodic_wrap_edges", k_periodic_wrap_edges, dim3(div_up(E_old, 256)), dim3(256), 0, o->edge_node.get(), E_old, o->n_node,
                          periodic->node_inverse.get(), t->n_node, E_new, t->nn_ptr.get(), t->nn_idx.get(), t->nn_dat.get(), index.get());
            XR_LAUNCH("periodic_unfilled", k_periodic_unfilled, dim3(div_up(E_new, 256)), dim3(256), 0, index.get(), E_new, count.get());
        } else {
            XR_LAUNCH("periodic_unwrap_edges", k_periodic_unwrap_edges, dim3(div_up(E_new, 256)), dim3(256), 0, t->edge_node.get(), E_new, t->n_node,
                      periodic->node_index.get(), o->n_node, E_old, o->nn_ptr.get(), o->nn_idx.get(), o->nn_dat.get(), index.get(), count.get());
        }
        *misses = read_scalar(count.get());
    }
    stream_sync();
    if (*misses == 0) {
        periodic->edge_index = std::move(index);
        periodic->n_edge_index = E_new;
    }
    XR_API_END
}

int xr_periodic_info(const xr_periodic *periodic, int64_t *n_index) {
    XR_API_BEGIN
    XR_REQUIRE(periodic && n_index, XR_ERR_INVALID, "xr_periodic_info: NULL argument");
    n_index[0] = periodic->n_node_new, n_index[1] = periodic->n_edge_index, n_index[2] = periodic->n_face;
    XR_API_END
}

int xr_periodic_take_mesh(xr_periodic *periodic, xr_mesh **mesh) {
    XR_API_BEGIN
    XR_REQUIRE(periodic && mesh && periodic->mesh, XR_ERR_INVALID, "xr_periodic_take_mesh: no mesh to hand out");
    *mesh = periodic->mesh;
    periodic->mesh = nullptr;
    XR_API_END
}

int xr_periodic_index_copy_dev(const xr_periodic *periodic, int facet, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(periodic && facet >= 0 && facet < 3 && (facet != 1 || periodic->n_edge_index >= 0), XR_ERR_INVALID,
               "xr_periodic_index_copy_dev: bad argument");
    const int64_t n = facet == 0 ? periodic->n_node_new : facet == 1 ? periodic->n_edge_index : periodic->n_face;
    XR_REQUIRE(out_dev || n == 0, XR_ERR_INVALID, "xr_periodic_index_copy_dev: NULL argument");
    if (facet == 2) {
        if (n > 0) XR_LAUNCH("periodic_iota", k_periodic_iota, dim3(div_up(n, 256)), dim3(256), 0, n, out_dev);
    } else {
        widen_dev((facet == 0 ? periodic->node_index : periodic->edge_index).get(), n, out_dev);
    }
    dev_call_done();
    XR_API_END
}

int xr_periodic_node_inverse_copy_dev(const xr_periodic *periodic, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(periodic && periodic->wrapped && out_dev, XR_ERR_INVALID, "xr_periodic_node_inverse_copy_dev: not the result of a wrap");
    widen_dev(periodic->node_inverse.get(), periodic->n_node_old, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_periodic_destroy(xr_periodic *periodic) {
    XR_API_BEGIN
    if (periodic) {
        release_point();
        delete periodic;
    }
    XR_API_END
}

} // extern "C"
