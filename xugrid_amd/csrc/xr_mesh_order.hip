// xr_mesh_order.hip -- the two spatial orderings of a mesh's faces: the query order (Morton order of coarse cells) and the tree
// index (hierarchical grid), both one counting sort fused with the permutation of the per-face arrays.  What the host decides
// from the statistics beforehand -- grid levels, Morton cover, whether the caller's numbering is kept -- is xr_mesh_plan.h.
//
// Replaces, on the device, what the reference does when it constructs
// numba_celltree.CellTree2d(node_coordinates, face_node_connectivity, -1)
// (xugrid/ugrid/ugrid2d.py:908-921).  The index is NOT a port of the
// cell tree: a bounding-interval hierarchy is a pointer-chasing structure; on CDNA4 a
// counting-sorted hierarchical grid gives contiguous, coalescable record runs per query row.
#include <algorithm>
#include <cmath>

#include "xr_mesh.h"
#include "xr_mesh_plan.h"
#include "xr_agg.h"

namespace xr {

// ---------------------------------------------------------------------------------------------
// spatial ordering = counting sort of the faces by a small integer key (the ONLY sort the engine
// needs), fused with the permutation of the per-face arrays:
//   pass 1 (k_spatial_count)   key of every face (Morton code of a coarse cell / grid cell of the
//                              tree index) + bucket histogram (global atomics)
//   scan                       bucket offsets (= cell_start for the tree index)
//   pass 2 (k_spatial_scatter) slot = offset + atomic cursor; the face's vertex block, length,
//                              bbox (f64, or the conservative f32 record bbox) are read
//                              coalesced in the caller's order and written to the slot
// Order inside a bucket follows the atomics, i.e. is unspecified -- every consumer is written
// so that final results do not depend on it.
// ---------------------------------------------------------------------------------------------

// (KeyTable / agg_insert -- one global atomic per DISTINCT key of a block -- live in xr_agg.h: the edge kernels use them too)

// (`lv` = the per-level grid sizes in LDS, [0..L) nx, [L..2L) ny, [2L..3L) base: the level differs from lane to lane, and
// indexing the kernel ARGUMENT g.nx[l] with it compiles to three dependent global loads per face)
__device__ __forceinline__ int face_cell(const GridParams &g, const int32_t *lv, double4 bb) {
    const double e = fmax(bb.y - bb.x, bb.w - bb.z);
    const int l = level_of_extent(g, e);
    const double inv_h = level_inv_h(g, l);
    const int nx = lv[l], ny = lv[MAX_LEVELS + l], base = lv[2 * MAX_LEVELS + l];
    const int cx = cell_coord(bb.x, g.x0, inv_h, nx);
    const int cy = cell_coord(bb.z, g.y0, inv_h, ny);
    return base + cy * nx + cx;
}

// (the bbox comes from the raw mesh, like in the scatter pass: node gathers hit the L2-resident node array)
template <bool INDEX, int MC>
__global__ void __launch_bounds__(256)
k_spatial_count(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n, int m_rt,
                GridParams g, MortonParams mp, int32_t *__restrict__ key, int32_t *__restrict__ count,
                const double *__restrict__ bbox_opt = nullptr /* caller-order boxes of a prepared mesh (polygon meshes) */) {
    constexpr int MA = MC > 0 ? MC : XR_MAX_FACE_NODES;
    const int m = MC > 0 ? MC : m_rt;
    __shared__ int32_t sh_lv[3 * MAX_LEVELS];
    if (INDEX) {
        if (threadIdx.x < MAX_LEVELS) {
            sh_lv[threadIdx.x] = g.nx[threadIdx.x];
            sh_lv[MAX_LEVELS + threadIdx.x] = g.ny[threadIdx.x];
            sh_lv[2 * MAX_LEVELS + threadIdx.x] = g.base[threadIdx.x];
        }
        __syncthreads();
    }
    __shared__ KeyTable sh_tab;
    agg_clear(sh_tab);
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f < n) {
        double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        if (MC == 0 && bbox_opt) {
            const double4 b = reinterpret_cast<const double4 *>(bbox_opt)[f];
            xmin = b.x, xmax = b.y, ymin = b.z, ymax = b.w;
        } else {
            bool open = true;
#pragma unroll
            for (int j = 0; j < MA; j++) {
                if (j < m) {
                    const int v = faces_raw[f * m + j];
                    open = open && !(j >= 3 && v < 0); // polygon_length: stop at the first fill value
                    if (open) {
                        const P2 p = load_p2(node_xy, v);
                        xmin = fmin(xmin, p.x);
                        xmax = fmax(xmax, p.x);
                        ymin = fmin(ymin, p.y);
                        ymax = fmax(ymax, p.y);
                    }
                }
            }
        }
        const double4 bb = make_double4(xmin, xmax, ymin, ymax);
        const int k = INDEX ? face_cell(g, sh_lv, bb) : morton_key(mp, bb);
        key[f] = k;
        int rank;
        agg_insert(sh_tab, k, rank);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < AGG_SLOTS; s += 256)
        if (sh_tab.key[s] >= 0) atomicAdd(&count[sh_tab.key[s]], sh_tab.cnt[s]);
}

// The face's CCW-normalised vertex block and its bbox are recomputed from the raw mesh (node gathers hit the
// L2-resident node array) instead of being copied from the caller-order arrays: a mesh that is only ever the
// TREE never materialises `fxy`, and the scatter reads 17 bytes per face instead of 97.
template <bool INDEX, int MC>
__global__ void __launch_bounds__(256)
k_spatial_scatter(const int32_t *__restrict__ key, int64_t n, int m_rt, const int32_t *__restrict__ start,
                  int32_t *__restrict__ cursor, const double *__restrict__ node_xy,
                  const int32_t *__restrict__ faces_raw, int32_t *__restrict__ perm, double *__restrict__ o_fxy,
                  uint8_t *__restrict__ o_len, double *__restrict__ o_bbox, float *__restrict__ o_recbb, double x0,
                  double y0, const double *__restrict__ bbox_opt = nullptr, const uint8_t *__restrict__ len_opt = nullptr) {
    constexpr int MA = MC > 0 ? MC : XR_MAX_FACE_NODES;
    const int m = MC > 0 ? MC : m_rt;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // Slots: `cursor` still holds the bucket histogram of the count pass and is handed out from the top down (the order inside
    // a bucket is unspecified anyway), which leaves every bucket at zero for the next build.  One returning atomic per DISTINCT
    // key of the block, as in the count pass (device-scope atomics are executed at the memory side of the fabric, ~40 G/s: one
    // per face was half of this kernel); a face's slot inside the block's stretch is its rank in the LDS table.
    __shared__ KeyTable sh_tab;
    agg_clear(sh_tab);
    const bool valid = f < n;
    const bool stored_only = MC == 0 && bbox_opt && len_opt && !o_fxy;
    // (the face's node ids go out together with the key, in front of the barriers: their gathers follow the slot computation
    // without a further round trip)
    int face[MA];
    if (valid && !stored_only) {
#pragma unroll
        for (int j = 0; j < MA; j++)
            if (j < m) face[j] = faces_raw[f * m + j];
    }
    const int k = valid ? key[f] : -1;
    __syncthreads();
    int tab_slot = 0, rank = 0;
    if (valid) tab_slot = agg_insert(sh_tab, k, rank);
    __syncthreads();
    for (int s = threadIdx.x; s < AGG_SLOTS; s += 256)
        if (sh_tab.key[s] >= 0) sh_tab.base[s] = start[sh_tab.key[s]] + atomicSub(&cursor[sh_tab.key[s]], sh_tab.cnt[s]) - sh_tab.cnt[s];
    __syncthreads();
    if (!valid) return;
    const int64_t r = (int64_t)sh_tab.base[tab_slot] + rank;
    if (stored_only) {
        // a prepared polygon mesh (its vertex blocks are written by ragged_fill): the record is the stored box and length
        const double4 b = reinterpret_cast<const double4 *>(bbox_opt)[f];
        perm[r] = (int32_t)f;
        o_len[r] = len_opt[f];
        if (INDEX)
            reinterpret_cast<float4 *>(o_recbb)[r] = make_float4(f32_below(b.x - x0), f32_above(b.y - x0), f32_below(b.z - y0), f32_above(b.w - y0));
        else
            reinterpret_cast<double4 *>(o_bbox)[r] = b;
        return;
    }
    int nl;
    bool flip;
    face_shape<MA>(node_xy, face, m, nl, flip);
    constexpr bool PREFETCH = MC > 0; // (general polygons, up to 32 nodes: gathered in the loop below, not held in registers)
    P2 pts[PREFETCH ? MA : 1];
    if (PREFETCH) {
#pragma unroll
        for (int j = 0; j < MA; j++)
            if (j < nl) pts[j] = load_p2(node_xy, face[j]);
    }
    perm[r] = (int32_t)f;
    o_len[r] = (uint8_t)nl;
    double2 *dst = reinterpret_cast<double2 *>(o_fxy) + r * m;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
#pragma unroll
    for (int j = 0; j < MA; j++) {
        if (j < nl) {
            const P2 p = PREFETCH ? pts[PREFETCH ? j : 0] : load_p2(node_xy, face[j]);
            xmin = fmin(xmin, p.x);
            xmax = fmax(xmax, p.x);
            ymin = fmin(ymin, p.y);
            ymax = fmax(ymax, p.y);
            if (o_fxy) dst[flip ? nl - 1 - j : j] = make_double2(p.x, p.y); // (ragged meshes: ragged_fill writes them)
        }
    }
    if (INDEX) {
        reinterpret_cast<float4 *>(o_recbb)[r] =
            make_float4(f32_below(xmin - x0), f32_above(xmax - x0), f32_below(ymin - y0), f32_above(ymax - y0));
    } else if (o_bbox) {
        reinterpret_cast<double4 *>(o_bbox)[r] = make_double4(xmin, xmax, ymin, ymax);
    }
}

template <bool INDEX>
static void spatial_sort(xr_mesh *mesh, const GridParams &g, const MortonParams &mp, int64_t n_buckets,
                         int32_t *bucket_start, int32_t *perm, double *o_fxy, uint8_t *o_len, double *o_bbox,
                         float *o_recbb) {
    const int64_t F = mesh->n_face;
    // (polygon meshes are always prepared with their caller-order boxes and lengths, mesh_prepare; both null for triangles and
    // quadrilaterals, whose kernels read the vertices instead)
    const double *boxes = mesh->prep.has_attrs && mesh->m != 3 && mesh->m != 4 ? mesh->prep.bbox.get() : nullptr;
    const uint8_t *lens = boxes ? mesh->prep.len.get() : nullptr;
    // The histogram lives in the engine's zero-at-rest scratch: the count pass raises it, the scatter pass hands the slots
    // out from the top down -- every bucket is back at zero when the scatter has run, so the next build needs no memset
    // (one launch, or two when the length is odd: 9 us + gaps of a 0.56 ms step).
    DevBuf<int32_t> key((size_t)F), count_own;
    int32_t *count = zero_scratch(0, (size_t)n_buckets);
    const bool cached = count != nullptr;
    if (!cached) {
        count_own.alloc((size_t)n_buckets);
        count = count_own.get();
        XR_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * (((size_t)n_buckets + 3) & ~(size_t)3), launch_stream())); // (blocks are >= 4 KB: one fill kernel)
    }
    if (F > 0) {
        const char *name = INDEX ? "index_count" : "order_count";
        const dim3 grid(div_up(F, 256)), block(256);
        with_nodes_per_face(mesh->m, [&](auto mc) {
            XR_LAUNCH(name, (k_spatial_count<INDEX, mc()>), grid, block, 0, mesh->node_xy.get(), mesh->faces_raw.get(), F,
                      mesh->m, g, mp, key.get(), count, boxes);
        });
    }
    exclusive_scan_i32(count, bucket_start, n_buckets);
    if (F > 0) {
        const char *name = INDEX ? "index_scatter" : "order_scatter";
        const dim3 grid(div_up(F, 256)), block(256);
        with_nodes_per_face(mesh->m, [&](auto mc) {
            XR_LAUNCH(name, (k_spatial_scatter<INDEX, mc()>), grid, block, 0, key.get(), F, mesh->m, bucket_start, count,
                      mesh->node_xy.get(), mesh->faces_raw.get(), perm, o_fxy, o_len, o_bbox, o_recbb, g.x0, g.y0, boxes, lens);
        });
    }
    if (cached) zero_scratch_done(0);
}

void mesh_query_order(xr_mesh *mesh) {
    if (mesh->qo.ready) return;
    mesh_read_stats(mesh, /*need_exact=*/true); // (the ordering heuristic reads sums over ALL faces: sampled statistics are redone)
    const int64_t F = mesh->n_face;
    const int m = mesh->m;
    mesh->qo.identity = numbering_coherent(mesh->stats.h, F);
    if (mesh->qo.identity) {
        mesh_face_coords(mesh); // the caller-order vertex blocks ARE the query-order ones (no-op if prepared with them)
        mesh->qo.ready = true;
        return;
    }
    mesh->qo.perm.alloc((size_t)F);
    if (!mesh->ragged()) mesh->qo.fxy.alloc((size_t)F * m * 2);
    mesh->qo.len.alloc((size_t)F);
    if (mesh->ragged()) mesh->qo.bbox.alloc((size_t)F * 4); // (dense meshes: query_face_box)
    if (F > 0) {
        const MortonParams mp = morton_cover(mesh->stats.h, F, 2.0, 1, 10); // two mean extents per coarse cell
        const int64_t n_keys = (int64_t)mp.n_side * mp.n_side;
        GridParams g{};
        DevBuf<int32_t> start((size_t)n_keys + 1);
        spatial_sort<false>(mesh, g, mp, n_keys, start.get(), mesh->qo.perm.get(),
                            mesh->ragged() ? (double *)nullptr : mesh->qo.fxy.get(), mesh->qo.len.get(), mesh->qo.bbox.get(),
                            nullptr);
    }
    if (mesh->ragged()) ragged_fill(mesh, mesh->qo.perm.get(), mesh->qo.len.get(), mesh->qo.off, mesh->qo.fxy);
    mesh->qo.ready = true;
}

void mesh_build_index(xr_mesh *mesh) {
    if (mesh->index.ready) return;
    mesh_read_stats(mesh);
    const int64_t F = mesh->n_face;
    const int m = mesh->m;
    XR_REQUIRE(F < (int64_t)1 << 31, XR_ERR_LIMIT, "mesh has too many faces for int32 indices");
    GridParams g{};
    XR_REQUIRE(index_grid(mesh->stats.h, F, mesh->stats.sampled, g), XR_ERR_LIMIT, "spatial index too large");
    mesh->index.grid = g;

    mesh->index.cell_start.alloc((size_t)g.n_cells + 1);
    mesh->index.rec_bb.alloc(((size_t)F + MeshIndex::REC_BB_PAD) * 4);
    mesh->index.rec_face.alloc((size_t)F);
    if (!mesh->ragged()) mesh->index.rec_fxy.alloc((size_t)F * m * 2);
    mesh->index.rec_len.alloc((size_t)F);
    MortonParams mp{};
    spatial_sort<true>(mesh, g, mp, g.n_cells, mesh->index.cell_start.get(), mesh->index.rec_face.get(),
                       mesh->ragged() ? (double *)nullptr : mesh->index.rec_fxy.get(), mesh->index.rec_len.get(), nullptr,
                       mesh->index.rec_bb.get());
    if (mesh->ragged()) ragged_fill(mesh, mesh->index.rec_face.get(), mesh->index.rec_len.get(), mesh->index.rec_off, mesh->index.rec_fxy);
    mesh->index.ready = true;
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_mesh_build_index(xr_mesh *mesh) {
    XR_API_BEGIN
    XR_REQUIRE(mesh, XR_ERR_INVALID, "xr_mesh_build_index: NULL mesh");
    mesh_build_index(mesh);
    stream_sync();
    XR_API_END
}

} // extern "C"
