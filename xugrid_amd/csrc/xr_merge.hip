// xr_merge.hip -- joining device meshes (Ugrid2d.merge_partitions, partitioning.py:81-148), matching two point sets
// (connectivity.index_like, connectivity.py:38-61) and splitting by label (partitioning.py:16-27), where the meshes are.
// DESIGN section 15.
//
// Everything here asks one question of a set of rows: "which rows are equal, and which of them came first".  No sort answers
// it: an open-addressing KEY TABLE in HBM does.  Slots are int32 ids of rows, -1 when empty; the capacity is a power of two
// strictly greater than the number of rows (key_table_capacity), probing is linear with wrap-around.  A row is compared by
// reading it through the id in the slot: coordinate pairs with == on doubles (-0.0 == 0.0; a NaN equals nothing, itself
// included), faces and edges by their ascending-sorted ints.
//
// The table, its insert and look-up kernels and why every key ends with its smallest id are in xr_key_table.h, which
// xr_periodic.hip shares.
//
// Around the table sits the pattern of xr_subset.hip: flag (rep[i] == i) -> exclusive_scan_i32 (the dense rank) -> compaction.
// The per-partition indexes come out of the same scan: its values at the partitions' boundaries are the offsets.  Ids are
// int32 in HBM; nothing is read through an id that has not been compared with its range.
#include <algorithm>
#include <vector>

#include "xr_objects.h"
#include "xr_prims.h"
#include "xr_topology.h"

#include "xr_key_table.h"

namespace xr {

// the rows kept of a concatenation of P segments: their ids in the concatenation, ascending, and where each segment's part starts
struct KeptRows {
    DevBuf<int32_t> keep;            // [bound[P]]
    std::vector<int64_t> off, bound; // [P + 1]: first row of segment p in the concatenation / in `keep`
};

} // namespace xr

struct xr_merge {
    xr_mesh *mesh = nullptr;           // the merged mesh until xr_merge_take_mesh hands it out
    xr::KeptRows rows[3];              // by facet id: 0 nodes, 1 edges (after xr_merge_edges_dev), 2 faces
    xr::DevBuf<int32_t> node_inverse;  // [sum n_node] merged id of every concatenated node
    xr::DevBuf<int32_t> edge_position; // [kept edges] the merged mesh's own id of every kept edge
    bool has_edges = false;
    ~xr_merge() { delete mesh; }
};

// the order of the labels: ids grouped by label, ascending inside a label
struct xr_label_order {
    int64_t n = 0;
    xr::DevBuf<int32_t> ids; // [n]
};

namespace xr {

static constexpr int MERGE_SORT_REGS = 8; // rows up to this width are sorted in registers

// faces of one partition, one thread per face: the row widened to M slots with -1, real slots through node_inverse (with the
// partition's node offset), as given into all_rows and ascending into sorted_rows.  M > 0: the row lives in registers (every
// index is a constant after unrolling); M == 0: any width m, sorted where it lies.
template <int M>
__global__ void __launch_bounds__(256)
k_merge_face_rows(const int32_t *__restrict__ faces, int64_t n_face, int mp, int64_t n_node, int64_t node_off,
                  const int32_t *__restrict__ inverse, int m, int32_t *__restrict__ all_rows, int32_t *__restrict__ sorted_rows) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    if constexpr (M > 0) {
        int32_t v[M];
#pragma unroll
        for (int k = 0; k < M; k++) {
            const int32_t node = k < mp ? faces[f * mp + k] : -1;
            v[k] = node >= 0 && node < n_node ? inverse[node_off + node] : -1;
        }
#pragma unroll
        for (int k = 0; k < M; k++) all_rows[f * M + k] = v[k];
        key_sort_row(v);
#pragma unroll
        for (int k = 0; k < M; k++) sorted_rows[f * M + k] = v[k];
    } else {
        for (int k = 0; k < m; k++) {
            const int32_t node = k < mp ? faces[f * mp + k] : -1;
            const int32_t v = node >= 0 && node < n_node ? inverse[node_off + node] : -1;
            all_rows[f * m + k] = v;
            sorted_rows[f * m + k] = v;
        }
        key_sort_row_inplace(sorted_rows + f * m, m);
    }
}

// edges of one partition, one thread per edge: (lower, higher) merged node
__global__ void __launch_bounds__(256)
k_merge_edge_rows(const int32_t *__restrict__ edge_node, int64_t n_edge, int64_t n_node, int64_t node_off,
                  const int32_t *__restrict__ inverse, int32_t *__restrict__ rows) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edge) return;
    const int32_t a = edge_node[2 * e], b = edge_node[2 * e + 1];
    const int32_t u = a >= 0 && a < n_node ? inverse[node_off + a] : -1, v = b >= 0 && b < n_node ? inverse[node_off + b] : -1;
    rows[2 * e] = u < v ? u : v;
    rows[2 * e + 1] = u < v ? v : u;
}

// one thread per (row, slot) of the concatenation: consecutive lanes read consecutive words
__global__ void __launch_bounds__(256)
k_merge_compact_rows(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n, int m,
                     const int32_t *__restrict__ rows, int32_t *__restrict__ keep, int32_t *__restrict__ out_rows) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * m) return;
    const int64_t i = t / m;
    if (!flag[i]) return;
    const int slot = (int)(t - i * m);
    const int64_t j = rank[i];
    if (slot == 0) keep[j] = (int32_t)i;
    out_rows[j * m + slot] = rows[t];
}

// a kept edge goes to its rank with the merged mesh's own id of its node pair: row `lower` of the node -> node CSR, whose
// data is the edge id (-1 if the merged mesh has no such edge: cannot happen for edges of its own faces)
__global__ void __launch_bounds__(256)
k_merge_compact_edges(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n, const int32_t *__restrict__ rows,
                      int64_t n_node, const int32_t *__restrict__ nn_ptr, const int32_t *__restrict__ nn_idx,
                      const int32_t *__restrict__ nn_dat, int32_t *__restrict__ keep, int32_t *__restrict__ position) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int j = rank[i];
    keep[j] = (int32_t)i;
    const int32_t lo = rows[2 * i], hi = rows[2 * i + 1];
    int32_t id = -1;
    if (lo >= 0 && lo < n_node)
        for (int k = nn_ptr[lo]; k < nn_ptr[lo + 1]; k++)
            if (nn_idx[k] == hi) id = nn_dat[k];
    position[j] = id;
}

// ---- index_like
__global__ void __launch_bounds__(256) k_like_keys(const double *__restrict__ xy, int64_t n2, double tolerance, double *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) keys[i] = rint(xy[i] / tolerance); // (np.round: half to even, as rint in the default rounding mode)
}

__global__ void __launch_bounds__(256) k_like_repeats(const int32_t *__restrict__ flag, int64_t n, int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    wave_count(i < n && !flag[i], count);
}

enum LikeStatus : int { LS_REPEAT = 0, LS_MISS = 1, LS_COUNT = 2 };

// one thread per row i of b: the row j of a with b's key, checked against the tolerance on both axes; hit[j] counts the takers
__global__ void __launch_bounds__(256)
k_like_lookup(const double2 *__restrict__ key_a, const double2 *__restrict__ key_b, const double2 *__restrict__ a,
              const double2 *__restrict__ b, int64_t n, double tolerance, const int32_t *__restrict__ table, uint32_t mask,
              int32_t *__restrict__ hit, int64_t *__restrict__ index, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool miss = false, repeat = false;
    if (i < n) {
        const double2 q = key_b[i];
        uint32_t h = key_hash_xy(q.x, q.y) & mask;
        int32_t j = -1;
        for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
            const int32_t occ = table[h];
            if (occ < 0) break;
            if ((int64_t)occ >= n) continue;
            const double2 p = key_a[occ];
            if (p.x == q.x && p.y == q.y) {
                j = occ;
                break;
            }
        }
        if (j >= 0) {
            const double2 p = a[j], r = b[i];
            if (!(fabs(p.x - r.x) <= tolerance && fabs(p.y - r.y) <= tolerance)) j = -1;
        }
        miss = j < 0;
        if (!miss) repeat = atomicExch(hit + j, 1) != 0;
        index[i] = j;
    }
    wave_count(repeat, status + LS_REPEAT);
    wave_count(miss, status + LS_MISS);
}

// ---- labels
enum LabelStatus : int { LB_MIN = 0, LB_MAX = 1 };
// smallest and largest label: the block's (block_reduce, xr_prims.h), then one atomic pair per BLOCK (a million
// atomics on two words would queue up behind each other)
__global__ void __launch_bounds__(256) k_label_range(const int64_t *__restrict__ labels, int64_t n, int32_t *__restrict__ status) {
    __shared__ int32_t lds[2 * 4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t lo = INT32_MAX, hi = -1;
    if (i < n) lo = hi = (int32_t)std::min<int64_t>(std::max<int64_t>(labels[i], -1), INT32_MAX); // (clamped: the host only asks "negative?" and "too many?")
    block_reduce<256, OpMin, OpMax>(lds, lo, hi);
    if (threadIdx.x == 0) {
        atomicMin(status + LB_MIN, lo);
        atomicMax(status + LB_MAX, hi);
    }
}

// flags[l * n + i] = (labels[i] == l): label-major, so ONE scan ranks every id behind the ids of smaller labels and behind the
// smaller ids of its own -- the stable placement, without atomics
__global__ void __launch_bounds__(256)
k_label_flags(const int64_t *__restrict__ labels, int64_t n, int64_t n_label, int32_t *__restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * n_label) return;
    const int64_t l = t / n;
    flags[t] = labels[t - l * n] == l;
}

__global__ void __launch_bounds__(256)
k_label_place(const int64_t *__restrict__ labels, int64_t n, int64_t n_label, const int32_t *__restrict__ rank, int32_t *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = labels[i];
    if (l >= 0 && l < n_label) ids[rank[l * n + i]] = (int32_t)i;
}

__global__ void k_label_bounds(const int32_t *__restrict__ rank, int64_t n, int64_t n_label, int32_t *__restrict__ out) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l <= n_label) out[l] = rank[l * n];
}

// ---- host side
static void face_rows(const xr_mesh *part, int64_t node_off, const int32_t *inverse, int m, int32_t *all_rows, int32_t *sorted_rows) {
    const int64_t F = part->n_face;
    if (F == 0) return;
    auto launch = [&](auto tag) {
        constexpr int M = decltype(tag)::value;
        XR_LAUNCH("merge_face_rows", k_merge_face_rows<M>, dim3(div_up(F, 256)), dim3(256), 0, part->faces_raw.get(), F, part->m,
                  part->n_node, node_off, inverse, m, all_rows, sorted_rows);
    };
    switch (m <= MERGE_SORT_REGS ? m : 0) {
    case 3: launch(std::integral_constant<int, 3>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 5: launch(std::integral_constant<int, 5>()); break;
    case 6: launch(std::integral_constant<int, 6>()); break;
    case 7: launch(std::integral_constant<int, 7>()); break;
    case 8: launch(std::integral_constant<int, 8>()); break;
    default: launch(std::integral_constant<int, 0>()); break;
    }
}

static void set_offsets(KeptRows &rows, const std::vector<int64_t> &sizes) {
    rows.off.assign(sizes.size() + 1, 0);
    for (size_t p = 0; p < sizes.size(); p++) rows.off[p + 1] = rows.off[p] + sizes[p];
    rows.bound.assign(sizes.size() + 1, 0);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_merge_meshes_dev(xr_mesh *const *parts, int64_t n_part, xr_merge **out) {
    XR_API_BEGIN
    XR_REQUIRE(parts && out && n_part >= 1, XR_ERR_INVALID, "xr_merge_meshes_dev: bad argument");
    const int P = (int)n_part;
    std::vector<int64_t> n_node(P), n_face(P);
    int m = 3; // (no mesh is narrower: xr_mesh_create)
    for (int p = 0; p < P; p++) {
        XR_REQUIRE(parts[p], XR_ERR_INVALID, "xr_merge_meshes_dev: NULL mesh");
        n_node[p] = parts[p]->n_node, n_face[p] = parts[p]->n_face;
        m = std::max(m, parts[p]->m);
    }
    Building<xr_merge> merge(OnFailure::WaitFirst);
    KeptRows &nodes = merge->rows[0], &faces = merge->rows[2];
    set_offsets(nodes, n_node), set_offsets(faces, n_face);
    const int64_t N = nodes.off[P], F = faces.off[P];
    XR_REQUIRE(N < INT32_MAX && F * m < INT32_MAX, XR_ERR_LIMIT,
               "xr_merge_meshes_dev: %lld nodes / %lld face slots in all exceed the int32 index range", (long long)N, (long long)(F * m));

    // nodes: concatenate, first occurrences, rank, inverse
    DevBuf<double> all_xy((size_t)N * 2);
    for (int p = 0; p < P; p++)
        if (n_node[p] > 0)
            XR_HIP(hipMemcpyAsync(all_xy.get() + 2 * nodes.off[p], parts[p]->node_xy.get(), (size_t)n_node[p] * 16, hipMemcpyDeviceToDevice,
                                  launch_stream()));
    DevBuf<int32_t> node_rep((size_t)N), node_flag((size_t)N), node_rank((size_t)N + 1);
    merge->node_inverse.alloc((size_t)N);
    if (N > 0) table_first_occurrence(XYRows{reinterpret_cast<const double2 *>(all_xy.get())}, N, node_rep.get(), node_flag.get());
    rank_of_flags(node_flag.get(), node_rank.get(), N);
    if (N > 0)
        XR_LAUNCH("merge_inverse", k_merge_inverse, dim3(div_up(N, 256)), dim3(256), 0, node_rep.get(), node_rank.get(), N,
                  merge->node_inverse.get());

    // faces: widened, remapped rows and their sorted copies; the same table on the sorted rows
    DevBuf<int32_t> all_faces((size_t)(F * m)), sorted_faces((size_t)(F * m)), face_rep((size_t)F), face_flag((size_t)F),
        face_rank((size_t)F + 1);
    for (int p = 0; p < P; p++)
        face_rows(parts[p], nodes.off[p], merge->node_inverse.get(), m, all_faces.get() + faces.off[p] * m, sorted_faces.get() + faces.off[p] * m);
    if (F > 0) table_first_occurrence(IntRows{sorted_faces.get(), m}, F, face_rep.get(), face_flag.get());
    rank_of_flags(face_flag.get(), face_rank.get(), F);

    // the one read-back: both scans at the partitions' boundaries (the last of each is its total)
    std::vector<int32_t> at(2 * (P + 1)), h(2 * (P + 1));
    for (int p = 0; p <= P; p++) at[p] = (int32_t)nodes.off[p], at[P + 1 + p] = (int32_t)faces.off[p];
    DevBuf<int32_t> words((size_t)4 * (P + 1));
    h2d(words.get(), at.data(), at.size() * sizeof(int32_t));
    XR_LAUNCH("merge_bounds", k_merge_bounds, dim3(div_up(2 * (P + 1), 256)), dim3(256), 0, node_rank.get(), face_rank.get(), words.get(),
              P + 1, P + 1, words.get() + 2 * (P + 1));
    d2h(h.data(), words.get() + 2 * (P + 1), h.size() * sizeof(int32_t));
    for (int p = 0; p <= P; p++) nodes.bound[p] = h[p], faces.bound[p] = h[P + 1 + p];
    const int64_t Nn = nodes.bound[P], Fn = faces.bound[P];

    Building<xr_mesh> mesh = new_raw_mesh(Nn, Fn, m);
    nodes.keep.alloc((size_t)Nn), faces.keep.alloc((size_t)Fn);
    if (Nn > 0)
        XR_LAUNCH("merge_compact_xy", k_merge_compact_xy, dim3(div_up(N, 256)), dim3(256), 0, node_flag.get(), node_rank.get(), N,
                  reinterpret_cast<const double2 *>(all_xy.get()), nodes.keep.get(), reinterpret_cast<double2 *>(mesh->node_xy.get()));
    if (Fn > 0)
        XR_LAUNCH("merge_compact_faces", k_merge_compact_rows, dim3(div_up(F * m, 256)), dim3(256), 0, face_flag.get(), face_rank.get(), F, m,
                  all_faces.get(), faces.keep.get(), mesh->faces_raw.get());
    stream_sync(); // (the work arrays go back to the pool behind their readers)
    merge->mesh = mesh.release();
    *out = merge.release();
    XR_API_END
}

int xr_merge_edges_dev(xr_merge *merge, const xr_topology *const *parts, int64_t n_part, const xr_topology *merged) {
    XR_API_BEGIN
    XR_REQUIRE(merge && parts && merged, XR_ERR_INVALID, "xr_merge_edges_dev: NULL argument");
    const int P = (int)n_part;
    KeptRows &nodes = merge->rows[0], &edges = merge->rows[1];
    XR_REQUIRE((size_t)P + 1 == nodes.off.size(), XR_ERR_INVALID, "xr_merge_edges_dev: one topology per merged partition expected");
    XR_REQUIRE(merged->n_nonmanifold == 0 && merged->n_node == nodes.bound[P], XR_ERR_INVALID,
               "xr_merge_edges_dev: the merged topology is non-manifold or not the merged mesh's");
    std::vector<int64_t> n_edge(P);
    for (int p = 0; p < P; p++) {
        XR_REQUIRE(parts[p] && parts[p]->n_nonmanifold == 0 && parts[p]->n_node == nodes.off[p + 1] - nodes.off[p], XR_ERR_INVALID,
                   "xr_merge_edges_dev: topology %d is non-manifold or not of partition %d", p, p);
        n_edge[p] = parts[p]->n_edge;
    }
    set_offsets(edges, n_edge);
    const int64_t E = edges.off[P];
    XR_REQUIRE(2 * E < INT32_MAX, XR_ERR_LIMIT, "xr_merge_edges_dev: %lld edges in all exceed the int32 index range", (long long)E);
    DevBuf<int32_t> rows((size_t)E * 2), rep((size_t)E), flag((size_t)E), rank((size_t)E + 1);
    for (int p = 0; p < P; p++)
        if (n_edge[p] > 0)
            XR_LAUNCH("merge_edge_rows", k_merge_edge_rows, dim3(div_up(n_edge[p], 256)), dim3(256), 0, parts[p]->edge_node.get(), n_edge[p],
                      parts[p]->n_node, nodes.off[p], merge->node_inverse.get(), rows.get() + 2 * edges.off[p]);
    if (E > 0) table_first_occurrence(IntRows{rows.get(), 2}, E, rep.get(), flag.get());
    rank_of_flags(flag.get(), rank.get(), E);
    std::vector<int32_t> at(P + 1), h(P + 1);
    for (int p = 0; p <= P; p++) at[p] = (int32_t)edges.off[p];
    DevBuf<int32_t> words((size_t)2 * (P + 1));
    h2d(words.get(), at.data(), at.size() * sizeof(int32_t));
    XR_LAUNCH("merge_bounds", k_merge_bounds, dim3(div_up(P + 1, 256)), dim3(256), 0, rank.get(), rank.get(), words.get(), P + 1, 0,
              words.get() + (P + 1));
    d2h(h.data(), words.get() + (P + 1), h.size() * sizeof(int32_t));
    for (int p = 0; p <= P; p++) edges.bound[p] = h[p];
    const int64_t En = edges.bound[P];
    edges.keep.alloc((size_t)En), merge->edge_position.alloc((size_t)En);
    if (En > 0)
        XR_LAUNCH("merge_compact_edges", k_merge_compact_edges, dim3(div_up(E, 256)), dim3(256), 0, flag.get(), rank.get(), E, rows.get(),
                  merged->n_node, merged->nn_ptr.get(), merged->nn_idx.get(), merged->nn_dat.get(), edges.keep.get(),
                  merge->edge_position.get());
    stream_sync();
    merge->has_edges = true;
    XR_API_END
}

int xr_merge_info(const xr_merge *merge, int64_t *n_part, int64_t *n_node_all, int64_t *n_face_all) {
    XR_API_BEGIN
    XR_REQUIRE(merge && n_part && n_node_all && n_face_all, XR_ERR_INVALID, "xr_merge_info: NULL argument");
    *n_part = (int64_t)merge->rows[0].off.size() - 1;
    *n_node_all = merge->rows[0].off.back(), *n_face_all = merge->rows[2].off.back();
    XR_API_END
}

int xr_merge_take_mesh(xr_merge *merge, xr_mesh **mesh) {
    XR_API_BEGIN
    XR_REQUIRE(merge && mesh && merge->mesh, XR_ERR_INVALID, "xr_merge_take_mesh: no mesh to hand out");
    *mesh = merge->mesh;
    merge->mesh = nullptr;
    XR_API_END
}

int xr_merge_index_info(const xr_merge *merge, int facet, int64_t part, int64_t *n) {
    XR_API_BEGIN
    XR_REQUIRE(merge && n && facet >= 0 && facet < 3 && (facet != 1 || merge->has_edges), XR_ERR_INVALID, "xr_merge_index_info: bad argument");
    const KeptRows &rows = merge->rows[facet];
    XR_REQUIRE(part >= -1 && part + 1 < (int64_t)rows.off.size(), XR_ERR_INVALID, "xr_merge_index_info: no partition %lld", (long long)part);
    *n = part < 0 ? rows.bound.back() : rows.bound[part + 1] - rows.bound[part];
    XR_API_END
}

int xr_merge_index_copy_dev(const xr_merge *merge, int facet, int64_t part, int position, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(merge && facet >= 0 && facet < 3 && (facet != 1 || merge->has_edges) && (!position || facet == 1), XR_ERR_INVALID,
               "xr_merge_index_copy_dev: bad argument");
    const KeptRows &rows = merge->rows[facet];
    XR_REQUIRE(part >= -1 && part + 1 < (int64_t)rows.off.size(), XR_ERR_INVALID, "xr_merge_index_copy_dev: no partition %lld", (long long)part);
    const int64_t first = part < 0 ? 0 : rows.bound[part], n = (part < 0 ? rows.bound.back() : rows.bound[part + 1]) - first;
    XR_REQUIRE(out_dev || n == 0, XR_ERR_INVALID, "xr_merge_index_copy_dev: NULL argument");
    const int32_t *src = (position ? merge->edge_position.get() : rows.keep.get()) + first;
    widen_dev(src, n, out_dev, position || part < 0 ? 0 : rows.off[part]);
    dev_call_done();
    XR_API_END
}

int xr_merge_node_inverse_copy_dev(const xr_merge *merge, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(merge, XR_ERR_INVALID, "xr_merge_node_inverse_copy_dev: NULL argument");
    const int64_t n = merge->rows[0].off.back();
    XR_REQUIRE(out_dev || n == 0, XR_ERR_INVALID, "xr_merge_node_inverse_copy_dev: NULL argument");
    widen_dev(merge->node_inverse.get(), n, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_merge_destroy(xr_merge *merge) {
    XR_API_BEGIN
    if (merge) {
        release_point();
        delete merge;
    }
    XR_API_END
}

int xr_index_like_dev(const double *a_dev, const double *b_dev, int64_t n, double tolerance, int64_t *index_out_dev, int64_t *problems) {
    XR_API_BEGIN
    XR_REQUIRE(problems && ((a_dev && b_dev && index_out_dev) || n == 0) && n >= 0, XR_ERR_INVALID, "xr_index_like_dev: bad argument");
    XR_REQUIRE(n < INT32_MAX / 2, XR_ERR_LIMIT, "xr_index_like_dev: %lld rows exceed the int32 index range", (long long)n);
    XR_REQUIRE(tolerance >= 0.0, XR_ERR_INVALID, "xr_index_like_dev: the tolerance must not be negative");
    problems[0] = problems[1] = 0;
    if (n > 0) {
        DevBuf<double> keys;
        const double *key_a = a_dev, *key_b = b_dev;
        if (tolerance != 0.0) {
            keys.alloc((size_t)n * 4);
            XR_LAUNCH("like_keys", k_like_keys, dim3(div_up(2 * n, 256)), dim3(256), 0, a_dev, 2 * n, tolerance, keys.get());
            XR_LAUNCH("like_keys", k_like_keys, dim3(div_up(2 * n, 256)), dim3(256), 0, b_dev, 2 * n, tolerance, keys.get() + 2 * n);
            key_a = keys.get(), key_b = keys.get() + 2 * n;
        }
        // [status: LS_COUNT, two words unused][hit: n][rep: n][flag: n]; status and hit start as zero
        DevBuf<int32_t> work((size_t)(4 + 3 * n));
        int32_t *status = work.get(), *hit = work.get() + 4, *rep = hit + n, *flag = rep + n;
        fill_i32(work.get(), 0, 4 + n);
        KeyTable table(n);
        const XYRows rows{reinterpret_cast<const double2 *>(key_a)};
        XR_LAUNCH("merge_insert", k_table_insert<XYRows>, dim3(div_up(n, 256)), dim3(256), 0, rows, n, table.slots.get(), table.mask);
        XR_LAUNCH("merge_rep", k_table_rep<XYRows>, dim3(div_up(n, 256)), dim3(256), 0, rows, n, table.slots.get(), table.mask, rep, flag);
        XR_LAUNCH("like_repeats", k_like_repeats, dim3(div_up(n, 256)), dim3(256), 0, flag, n, status + LS_REPEAT);
        XR_LAUNCH("like_lookup", k_like_lookup, dim3(div_up(n, 256)), dim3(256), 0, reinterpret_cast<const double2 *>(key_a),
                  reinterpret_cast<const double2 *>(key_b), reinterpret_cast<const double2 *>(a_dev),
                  reinterpret_cast<const double2 *>(b_dev), n, tolerance, table.slots.get(), table.mask, hit, index_out_dev, status);
        int32_t h[LS_COUNT];
        d2h(h, status, sizeof(h));
        problems[0] = h[LS_REPEAT], problems[1] = h[LS_MISS];
        stream_sync();
    }
    XR_API_END
}

int xr_labels_range_dev(const int64_t *labels_dev, int64_t n, int64_t *min_label, int64_t *max_label) {
    XR_API_BEGIN
    XR_REQUIRE(min_label && max_label && (labels_dev || n == 0) && n >= 0, XR_ERR_INVALID, "xr_labels_range_dev: bad argument");
    *min_label = 0, *max_label = -1;
    if (n > 0) {
        DevBuf<int32_t> status(2);
        const int32_t start[2] = {INT32_MAX, -1};
        h2d(status.get(), start, sizeof(start));
        XR_LAUNCH("label_range", k_label_range, dim3(div_up(n, 256)), dim3(256), 0, labels_dev, n, status.get());
        int32_t h[2];
        d2h(h, status.get(), sizeof(h));
        *min_label = h[LB_MIN], *max_label = h[LB_MAX];
        stream_sync();
    }
    XR_API_END
}

int xr_labels_order_dev(const int64_t *labels_dev, int64_t n, int64_t n_label, xr_label_order **out, int64_t *bounds) {
    XR_API_BEGIN
    XR_REQUIRE(out && bounds && (labels_dev || n == 0) && n >= 0 && n_label >= 0, XR_ERR_INVALID, "xr_labels_order_dev: bad argument");
    XR_REQUIRE(n * n_label < INT32_MAX && n_label < (1 << 20), XR_ERR_LIMIT,
               "xr_labels_order_dev: %lld ids x %lld labels exceed the int32 index range", (long long)n, (long long)n_label);
    Building<xr_label_order> order(OnFailure::WaitFirst);
    order->n = n;
    order->ids.alloc((size_t)n);
    for (int64_t l = 0; l <= n_label; l++) bounds[l] = 0;
    if (n > 0 && n_label > 0) {
        const int64_t T = n * n_label;
        DevBuf<int32_t> flags((size_t)T), rank((size_t)T + 1), words((size_t)n_label + 1);
        XR_LAUNCH("label_flags", k_label_flags, dim3(div_up(T, 256)), dim3(256), 0, labels_dev, n, n_label, flags.get());
        exclusive_scan_i32(flags.get(), rank.get(), T);
        XR_LAUNCH("label_bounds", k_label_bounds, dim3(div_up(n_label + 1, 256)), dim3(256), 0, rank.get(), n, n_label, words.get());
        std::vector<int32_t> h((size_t)n_label + 1);
        d2h(h.data(), words.get(), h.size() * sizeof(int32_t), [&] {
            XR_LAUNCH("label_place", k_label_place, dim3(div_up(n, 256)), dim3(256), 0, labels_dev, n, n_label, rank.get(), order->ids.get());
        });
        for (int64_t l = 0; l <= n_label; l++) bounds[l] = h[(size_t)l];
        stream_sync();
    }
    *out = order.release();
    XR_API_END
}

int xr_label_order_copy_dev(const xr_label_order *order, int64_t first, int64_t count, int64_t *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(order && first >= 0 && count >= 0 && first + count <= order->n && (out_dev || count == 0), XR_ERR_INVALID,
               "xr_label_order_copy_dev: bad argument");
    widen_dev(order->ids.get() + first, count, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_label_order_destroy(xr_label_order *order) {
    XR_API_BEGIN
    if (order) {
        release_point();
        delete order;
    }
    XR_API_END
}

int xr_dev_copy_columns(void *dst_dev, int64_t dst_row_bytes, const void *src_dev, int64_t src_row_bytes, int64_t rows) {
    XR_API_BEGIN
    XR_REQUIRE(rows >= 0 && src_row_bytes >= 0 && dst_row_bytes >= src_row_bytes && ((dst_dev && src_dev) || rows * src_row_bytes == 0),
               XR_ERR_INVALID, "xr_dev_copy_columns: bad argument");
    if (rows > 0 && src_row_bytes > 0)
        XR_HIP(hipMemcpy2DAsync(dst_dev, (size_t)dst_row_bytes, src_dev, (size_t)src_row_bytes, (size_t)src_row_bytes, (size_t)rows,
                                hipMemcpyDeviceToDevice, launch_stream()));
    dev_call_done();
    XR_API_END
}

} // extern "C"
