// xr_mesh_front.hip -- the front of everything a mesh is used for: the statistics of its faces (kernels, the in-kernel tail,
// the hand-off to the host: MeshStatsBox) and the per-face preparation in the caller's order (fill/length/CCW/bbox/vertex
// gather, one launch for both meshes of a weight build: mesh_prepare_pair), areas, the flat vertex blocks of polygon meshes.
//
// Replaces, on the device, what intersect_faces does to the query mesh (cast, counter-clockwise normalisation, bounding
// boxes; xugrid/ugrid/ugrid2d.py:908-921).
#include <algorithm>
#include <cmath>
#include <memory>

#include "xr_mesh.h"
#include "xr_prims.h"

namespace xr {

static constexpr int PREP_BLOCK = 256;

// The eight statistics of a mesh, in the order of stat::Slot (xr_geom.h): a block's partial record.  Their
// operators are named here once; the order of every reduction is that of xr_prims.h, so the results are deterministic.
// lds: 8 * BLOCK / 64 doubles; the results are in thread 0.
template <int BLOCK, typename... OPS> struct StatsReduce {
    // one value per thread and statistic -> the block's
    __device__ __forceinline__ static void block(double *lds, double (&v)[8]) { block_reduce_array<false, BLOCK, OPS...>(lds, v); }
    // the nb partial records the blocks of a statistics kernel left -> the mesh's
    __device__ __forceinline__ static void partials(double *lds, const double *__restrict__ partial, int nb, double (&v)[8]) {
        block_fold_partials<false, BLOCK, OPS...>(lds, partial, nb, v);
    }
};
template <int BLOCK> using MeshStats = StatsReduce<BLOCK, OpMin, OpMax, OpMin, OpMax, OpSum, OpMax, OpMax, OpSum>;

// ---------------------------------------------------------------------------------------------
// per-face preparation.  MC > 0: compile-time vertices per face; MC == 0: runtime m <= 32.
// connectivity.area on the caller's order (connectivity.py:372-382, 615-633): fill slots and the closing slot
// repeat node 0; everything relative to node 0.  Only `relative` overlap weights and xr_mesh_area read it, so it
// is computed on demand (mesh_area) and not by the preparation pass.
template <int MC>
__global__ void __launch_bounds__(256)
k_face_area(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n_face, int m_rt,
            double *__restrict__ area) {
    constexpr int MA = MC > 0 ? MC : XR_MAX_FACE_NODES;
    const int m = MC > 0 ? MC : m_rt;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_face) return;
    int face[MA];
#pragma unroll
    for (int j = 0; j < MA; j++)
        if (j < m) face[j] = faces_raw[f * m + j];
    const P2 p0 = load_p2(node_xy, face[0]);
    double det = 0.0;
#pragma unroll
    for (int i = 0; i < MA; i++) {
        if (i < m) {
            const int ia = face[i] < 0 ? face[0] : face[i];
            int ib = face[0];
            if (i + 1 < m) ib = face[i + 1] < 0 ? face[0] : face[i + 1];
            const P2 a = load_p2(node_xy, ia), b = load_p2(node_xy, ib);
            const double ax = a.x - p0.x, ay = a.y - p0.y;
            const double bx = b.x - p0.x, by = b.y - p0.y;
            det += ax * by - ay * bx;
        }
    }
    area[f] = 0.5 * fabs(det);
}

// Tail of the two statistics kernels: the block's partial goes to HBM with agent-scope (sc1) stores, a counter says how
// many blocks have done so, and the LAST block to arrive reduces all partials -- in the fixed order of k_reduce_stats, so the
// result does not depend on which block that is -- and publishes the eight numbers: device copy, pinned host copy and,
// behind them, the host's sequence word (system scope), which the host polls (mesh_read_stats).  One launch and one
// cross-queue hop less per mesh than a separate one-block reduction kernel, and no event on the stream.
// Hand-off: 8-byte agent-scope atomics on both sides (MI355X_MICROARCH.md, inter-workgroup visibility) + an agent acquire
// in the one reducing block; the counter is zero at rest (the last block clears it).
// (StatsTail: xr_mesh.h)
// (bid / nb: the block's index among the nb blocks that share the tail -- the whole grid, or one part of the paired k_prepare_faces')
__device__ __forceinline__ void stats_tail(const StatsTail &t, const double (&a)[8], double *lds, int64_t bid, int64_t nb) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        double *p = t.partials + bid * 8;
#pragma unroll
        for (int i = 0; i < 8; i++) __hip_atomic_store(&p[i], a[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // Two-level arrival count: thousands of returning atomics on ONE address serialise (~10 ns each: 3900 blocks that
        // finish together = 40 us, measured); STATS_SHARDS counters on lines of their own take 1/STATS_SHARDS of the blocks
        // each, and only the last arrival of a shard goes on to the second-level word.
        const int shard = (int)(bid % STATS_SHARDS);
        const unsigned in_shard = (unsigned)((nb - shard + STATS_SHARDS - 1) / STATS_SHARDS);
        unsigned *first = t.done + 16 * (1 + shard);
        bool last = false;
        if (__hip_atomic_fetch_add(first, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_shard - 1) {
            __hip_atomic_store(first, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned shards = (unsigned)(nb < STATS_SHARDS ? nb : STATS_SHARDS);
            last = __hip_atomic_fetch_add(t.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1;
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) {
        __hip_atomic_store(t.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    // (the strided step of block_fold_partials, spelled out for the agent-scope loads)
    double r[8] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nb; i += PREP_BLOCK) {
        const double *p = t.partials + i * 8;
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = __hip_atomic_load(&p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r[0] = fmin(r[0], v[0]); r[1] = fmax(r[1], v[1]); r[2] = fmin(r[2], v[2]); r[3] = fmax(r[3], v[3]);
        r[4] += v[4]; r[5] = fmax(r[5], v[5]); r[6] = fmax(r[6], v[6]); r[7] += v[7];
    }
    __syncthreads(); // (lds still holds the block's own wave partials for thread 0 above)
    MeshStats<PREP_BLOCK>::block(lds, r);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            t.stats[k] = r[k];
            t.stats_host[k] = r[k];
        }
        __threadfence_system();
        __hip_atomic_store(&t.stats_host[8], t.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// (The end of a statistics block -- store the partial record for k_reduce_stats, or stats_tail -- is spelled out in both block
// functions below.  Behind one more inlined function, in every form tried, the polygon form k_prepare_faces<0, .> keeps its
// node ids in scalars instead of a register array and takes 92 / 76 instead of 62 VGPRs: profiles/r11_mesh_stages_ab.txt.)
// LIGHT: statistics only (a mesh that is only ever the TREE: its records are built from the raw mesh by
// k_spatial_scatter, nothing reads caller-order per-face arrays)
// (block bid of nb: the body of k_prepare_faces, which its paired form runs too)
template <int MC, bool LIGHT>
__device__ __forceinline__ void prepare_faces_block(int64_t bid, int64_t nb, const double *__restrict__ node_xy,
                                                    const int32_t *__restrict__ faces_raw, int64_t n_face, int m_rt,
                                                    double *__restrict__ fxy, uint8_t *__restrict__ len_out,
                                                    double *__restrict__ bbox, double *__restrict__ partials, const StatsTail &tail) {
    constexpr int MA = MC > 0 ? MC : XR_MAX_FACE_NODES;
    const int m = MC > 0 ? MC : m_rt;
    const int64_t f = bid * PREP_BLOCK + threadIdx.x;

    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, ext = 0.0, diag = 0.0, jump = 0.0;
    if (f < n_face) {
        int face[MA];
#pragma unroll
        for (int j = 0; j < MA; j++)
            if (j < m) face[j] = faces_raw[f * m + j];

        int n;
        bool flip;
        face_shape<MA>(node_xy, face, m, n, flip);
        if (!LIGHT) len_out[f] = (uint8_t)n;
        double2 *fx = reinterpret_cast<double2 *>(fxy) + f * m;
#pragma unroll
        for (int j = 0; j < MA; j++) {
            if (j < n) {
                const P2 p = load_p2(node_xy, face[j]);
                xmin = fmin(xmin, p.x);
                xmax = fmax(xmax, p.x);
                ymin = fmin(ymin, p.y);
                ymax = fmax(ymax, p.y);
                if (!LIGHT && fxy) fx[flip ? n - 1 - j : j] = make_double2(p.x, p.y);
            }
        }
        if (!LIGHT && bbox) reinterpret_cast<double4 *>(bbox)[f] = make_double4(xmin, xmax, ymin, ymax); // (polygon meshes only)
        ext = fmax(xmax - xmin, ymax - ymin);
        const double dx = xmax - xmin, dy = ymax - ymin;
        diag = sqrt(dx * dx + dy * dy);
    }

    // numbering coherence: distance between the bbox centres of consecutive faces (within a wave)
    const int lane = threadIdx.x & 63;
    {
        const double cx = 0.5 * (xmin + xmax), cy = 0.5 * (ymin + ymax);
        const double px = __shfl_up(cx, 1, 64), py = __shfl_up(cy, 1, 64);
        if (lane > 0 && f < n_face) jump = fmax(fabs(cx - px), fabs(cy - py));
    }
    // block partials (only thread 0's `a` is the block's)
    __shared__ double lds[8 * (PREP_BLOCK / 64)];
    double a[8] = {xmin, xmax, ymin, ymax, ext, ext, diag, jump};
    MeshStats<PREP_BLOCK>::block(lds, a);
    if (tail.done == nullptr) { // (separate reduction kernel behind this one)
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) partials[bid * 8 + k] = a[k];
        }
    } else {
        stats_tail(tail, a, lds, bid, nb);
    }
}

template <int MC, bool LIGHT>
__global__ void __launch_bounds__(PREP_BLOCK)
k_prepare_faces(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n_face,
                int m_rt, double *__restrict__ fxy, uint8_t *__restrict__ len_out, double *__restrict__ bbox,
                double *__restrict__ partials, StatsTail tail) {
    prepare_faces_block<MC, LIGHT>(blockIdx.x, gridDim.x, node_xy, faces_raw, n_face, m_rt, fxy, len_out, bbox, partials, tail);
}

// Statistics of a mesh that is only ever the TREE, from a SAMPLE of its faces: the index only needs the bounds (exact:
// taken from the node array, a coalesced stream) and the mean bbox extent (to choose the cell size: every `stride`-th block
// of 256 faces is looked at).  Block b reads faces [b * stride * 256, + 256) and its slice of the nodes; partials in the
// layout of k_prepare_faces with [7] = faces sampled.  Nothing the RESULTS depend on comes from the sample: the grid is an
// accelerator (any cell size gives the same pairs), the number of levels is then derived from the domain size, and the one
// statistic with a meaning outside the index -- the largest bbox diagonal behind the default tolerance -- is recomputed over
// all faces when somebody asks for it (mesh_read_stats(need_exact)).
template <int MC>
__device__ __forceinline__ void sample_stats_block(int64_t bid, int64_t nb, const double *__restrict__ node_xy, int64_t n_node,
                                                   const int32_t *__restrict__ faces_raw, int64_t n_face, int m_rt, int stride,
                                                   double *__restrict__ partials, const StatsTail &tail) {
    constexpr int MA = MC > 0 ? MC : XR_MAX_FACE_NODES;
    const int m = MC > 0 ? MC : m_rt;
    const int64_t f = (bid * stride) * PREP_BLOCK + threadIdx.x;
    double ext = 0.0, diag = 0.0, cnt = 0.0;
    if (f < n_face) {
        double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        bool open = true;
#pragma unroll
        for (int j = 0; j < MA; j++) {
            if (j < m) {
                const int v = faces_raw[f * m + j];
                open = open && !(j >= 3 && v < 0);
                if (open) {
                    const P2 p = load_p2(node_xy, v);
                    xmin = fmin(xmin, p.x);
                    xmax = fmax(xmax, p.x);
                    ymin = fmin(ymin, p.y);
                    ymax = fmax(ymax, p.y);
                }
            }
        }
        const double dx = xmax - xmin, dy = ymax - ymin;
        ext = fmax(dx, dy);
        diag = sqrt(dx * dx + dy * dy);
        cnt = 1.0;
    }
    // this block's slice of the node array
    double nx0 = INFINITY, nx1 = -INFINITY, ny0 = INFINITY, ny1 = -INFINITY;
    const int64_t per = (n_node + nb - 1) / nb;
    const int64_t i0 = bid * per, i1 = i0 + per < n_node ? i0 + per : n_node;
    const double2 *nodes = reinterpret_cast<const double2 *>(node_xy);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += PREP_BLOCK) {
        const double2 p = nodes[i];
        nx0 = fmin(nx0, p.x);
        nx1 = fmax(nx1, p.x);
        ny0 = fmin(ny0, p.y);
        ny1 = fmax(ny1, p.y);
    }
    __shared__ double lds[8 * (PREP_BLOCK / 64)];
    double a[8] = {nx0, nx1, ny0, ny1, ext, ext, diag, cnt};
    MeshStats<PREP_BLOCK>::block(lds, a);
    if (tail.done == nullptr) { // (separate reduction kernel behind this one)
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) partials[bid * 8 + k] = a[k];
        }
    } else {
        stats_tail(tail, a, lds, bid, nb);
    }
}

template <int MC>
__global__ void __launch_bounds__(PREP_BLOCK)
k_sample_stats(const double *__restrict__ node_xy, int64_t n_node, const int32_t *__restrict__ faces_raw, int64_t n_face,
               int m_rt, int stride, double *__restrict__ partials, StatsTail tail) {
    sample_stats_block<MC>(blockIdx.x, gridDim.x, node_xy, n_node, faces_raw, n_face, m_rt, stride, partials, tail);
}

// One front launch for a weight build (mesh_prepare_pair): the first nb_sample blocks are k_sample_stats of the TREE with its
// tail -- dispatched first, they run BESIDE the blocks behind them, which are k_prepare_faces of the QUERY.  The sampled pass is
// latency (a tenth of the bytes of the query's pass, on a grid that fills two of every three CUs once): alone it costs a launch of
// its own at the head of the chain, 17.5 + 30.6 us against 33.5 us for this kernel (1M x 1M step).  Beside
// the first generation of the query's blocks the sampling blocks take longer than alone: the host has the tree's statistics near
// the end of the launch (it waits ~12 us where it waited for nothing) and still reaches the index build earlier than before.
// The two parts share nothing: partials, counters and sequence words are each mesh's own.
struct SampleArgs {
    const double *node_xy;
    int64_t n_node;
    const int32_t *faces_raw;
    int64_t n_face;
    int stride;
    double *partials;
    StatsTail tail;
};
// (An overload of k_prepare_faces, told apart by its third template argument MT, the tree's nodes per face: the kernel tables
// of the profiles know the query's preparation by that name, and this is the form it takes in a weight build.)
template <int MC, bool LIGHT, int MT>
__global__ void __launch_bounds__(PREP_BLOCK)
k_prepare_faces(int nb_sample, SampleArgs t, const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw,
                int64_t n_face, double *__restrict__ fxy, uint8_t *__restrict__ len_out, double *__restrict__ partials, StatsTail tail) {
    if ((int)blockIdx.x < nb_sample) // (block-uniform)
        sample_stats_block<MT>(blockIdx.x, nb_sample, t.node_xy, t.n_node, t.faces_raw, t.n_face, MT, t.stride, t.partials, t.tail);
    else
        prepare_faces_block<MC, LIGHT>((int64_t)blockIdx.x - nb_sample, (int64_t)gridDim.x - nb_sample, node_xy, faces_raw, n_face, MC,
                                       fxy, len_out, nullptr, partials, tail);
}

// the second launch of the statistics where the kernel's last block does not reduce the partials itself (stats_tail)
__global__ void __launch_bounds__(256) k_reduce_stats(const double *__restrict__ partials, int64_t nb,
                                                     double *__restrict__ stats, double *stats_host, double seq) {
    __shared__ double lds[8 * 4];
    double a[8];
    MeshStats<256>::partials(lds, partials, (int)nb, a);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            stats[k] = a[k];
            stats_host[k] = a[k];
        }
        // the host polls the sequence word (mesh_read_stats): behind the statistics, system scope
        __threadfence_system();
        __hip_atomic_store(&stats_host[8], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- flat vertex blocks of polygon meshes (m > DENSE_MAX_NODES): offsets = exclusive scan of the lengths, then one
// pass writes the len[r] CCW-normalised vertices of face perm[r] (perm == nullptr: r) from the raw mesh
__global__ void __launch_bounds__(256) k_widen_len(const uint8_t *__restrict__ len, int64_t n, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = len[i];
}

// The vertex blocks of a block's 256 faces are one contiguous stretch of the output: they are staged in LDS and written
// out as whole lines (a thread writing its own 16-byte vertices at a stride of ~100 bytes touched 64 lines per store
// instruction: 0.15 ms for the 3M vertices of a Voronoi tessellation).  The node ids are read where they are needed
// (no 32-entry private copy of the row); orientation as face_shape(): the first non-collinear vertex triple decides.
static constexpr int RAGGED_STAGE = 2048; // vertices one block stages (32 KiB: five blocks per CU; a tessellation's typical block holds 1536); fuller blocks write directly

__global__ void __launch_bounds__(256)
k_fill_ragged(const double *__restrict__ node_xy, const int32_t *__restrict__ faces_raw, int64_t n_face, int m,
              const int32_t *__restrict__ perm, const uint8_t *__restrict__ len, const int32_t *__restrict__ off,
              double *__restrict__ out_xy) {
    __shared__ double2 sh_xy[RAGGED_STAGE];
    const int64_t r0 = (int64_t)blockIdx.x * 256, r = r0 + threadIdx.x;
    const int64_t r1 = r0 + 256 < n_face ? r0 + 256 : n_face;
    const int base = off[r0], total = off[r1] - base;
    const bool staged = total <= RAGGED_STAGE;
    if (r < n_face) {
        const int64_t f = perm ? perm[r] : r;
        const int32_t *face = faces_raw + f * m;
        const int n = len[r];
        bool flip = false;
        for (int i = 0; i < n; i++) {
            const int ia = face[i >= 2 ? i - 2 : i + n - 2], ib = face[i >= 1 ? i - 1 : n - 1], ic = face[i];
            const P2 a = load_p2(node_xy, ia), b = load_p2(node_xy, ib), c = load_p2(node_xy, ic);
            const double ux = b.x - a.x, uy = b.y - a.y, vx = c.x - a.x, vy = c.y - a.y;
            const double prod = ux * vy - uy * vx;
            if (prod == 0) continue;
            flip = prod < 0;
            break;
        }
        double2 *dst = staged ? sh_xy + (off[r] - base) : reinterpret_cast<double2 *>(out_xy) + off[r];
        // eight corners at a time as two rounds of independent loads (ids, then coordinates) instead of a chain of dependent pairs
        for (int j0 = 0; j0 < n; j0 += 8) {
            int id[8];
            P2 p[8];
#pragma unroll
            for (int u = 0; u < 8; u++) id[u] = face[j0 + u < n ? j0 + u : n - 1];
#pragma unroll
            for (int u = 0; u < 8; u++) p[u] = load_p2(node_xy, id[u]);
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (j0 + u < n) dst[flip ? n - 1 - (j0 + u) : j0 + u] = make_double2(p[u].x, p[u].y);
        }
    }
    if (!staged) return; // (uniform)
    __syncthreads();
    double2 *out = reinterpret_cast<double2 *>(out_xy) + base;
    for (int k = threadIdx.x; k < total; k += 256) out[k] = sh_xy[k];
}

void ragged_fill(xr_mesh *mesh, const int32_t *perm, const uint8_t *len, DevBuf<int32_t> &off, DevBuf<double> &xy) {
    const int64_t F = mesh->n_face;
    off.alloc((size_t)F + 1);
    DevBuf<int32_t> len32((size_t)std::max<int64_t>(F, 1));
    if (F > 0) XR_LAUNCH("widen_len", k_widen_len, dim3(div_up(F, 256)), dim3(256), 0, len, F, len32.get());
    exclusive_scan_i32(len32.get(), off.get(), F);
    const int64_t total = F > 0 ? read_scalar(off.get() + F) : 0;
    XR_REQUIRE(total >= 0, XR_ERR_LIMIT, "mesh has too many face vertices for int32 offsets");
    xy.alloc((size_t)std::max<int64_t>(total, 1) * 2);
    if (F > 0)
        XR_LAUNCH("fill_ragged", k_fill_ragged, dim3(div_up(F, 256)), dim3(256), 0, mesh->node_xy.get(),
                  mesh->faces_raw.get(), F, mesh->m, perm, len, off.get(), xy.get());
}

void mesh_face_coords(xr_mesh *mesh) {
    mesh_prepare(mesh, true);
    if (mesh->prep.fxy_valid) return;
    ragged_fill(mesh, nullptr, mesh->prep.len.get(), mesh->prep.fxy_off, mesh->prep.fxy); // (dense blocks are written by the prepare pass)
    mesh->prep.fxy_valid = true;
}

static constexpr int64_t SAMPLE_MIN_FACES = 1 << 17; // smaller meshes: the full pass costs a launch either way
static constexpr int SAMPLE_STRIDE = 8;              // every 8th block of 256 faces

// May the last block of a statistics kernel of nb blocks reduce the partials itself (stats_tail)?  Up to STATS_TAIL_MAX_BLOCKS
// blocks (beyond that a separate reduction kernel, as until round 3; "never" / "always" were measured behind a switch in
// round 4), and only on the engine's own main stream.  Every block pays ~3 us at its end for the hand-off (agent-scope stores,
// their acknowledgement, a returning atomic): nothing for the 490 blocks of sample_stats, whose result the host is waiting
// for (16 instead of 12 + 10 + 20 us until the tree's statistics are there), but +15 us for the 3900 blocks of
// prepare_faces, whose statistics are only read after the index build -- those keep the one-block kernel on the side
// stream (measured, 1M x 1M step: never 0.507, always 0.520, default see DESIGN section 5).
static constexpr int64_t STATS_TAIL_MAX_BLOCKS = 1024;
static bool stats_tail_in_kernel(int64_t nb) {
    return nb <= STATS_TAIL_MAX_BLOCKS && !(stream_override() || current_lane() || engine().on_side);
}

StatsTail MeshStatsBox::begin(double *partials, int64_t nb) {
    if (!host) { // pinned statistics page + the event of the two-launch form
        void *p = nullptr;
        XR_HIP(hipHostMalloc(&p, sizeof(double) * 16, hipHostMallocCoherent));
        host = static_cast<double *>(p);
        memset(host, 0, sizeof(double) * 16);
        XR_HIP(hipEventCreateWithFlags(&event, hipEventDisableTiming | hipEventReleaseToSystem));
    }
    seq += 1.0;
    polled = true; // (both forms end with the sequence word)
    if (!stats_tail_in_kernel(nb)) return StatsTail{partials, nullptr, nullptr, nullptr, seq};
    if (!done.get()) { // the hand-off words of the in-kernel reduction
        done.alloc(16 * (1 + STATS_SHARDS));
        XR_HIP(hipMemsetAsync(done.get(), 0, sizeof(unsigned) * 16 * (1 + STATS_SHARDS), launch_stream()));
    }
    return StatsTail{partials, done.get(), dev.get(), host, seq};
}

void MeshStatsBox::enqueued(const double *partials, int64_t nb, const StatsTail &tail, bool on_side) {
    if (!tail.done) {
        // (a one-block kernel that ends with writes to pinned host memory: ~10 us, which only the host waits for)
        std::unique_ptr<SideScope> side;
        if (on_side) side.reset(new SideScope);
        XR_LAUNCH("reduce_stats", k_reduce_stats, dim3(1), dim3(256), 0, partials, nb, dev.get(), host, tail.seq);
        XR_HIP(hipEventRecord(event, launch_stream()));
    }
    event_pending = !tail.done;
    launched = true;
    valid = false;
}

void MeshStatsBox::read() {
    if (valid) return;
    // the reducing block / kernel stores the sequence word behind the statistics: poll it (bounded), else wait for the
    // event behind the reduction kernel or drain the stream
    if (!(polled && poll_pinned_f64(host + 8, seq))) {
        if (event_pending) XR_HIP(hipEventSynchronize(event));
        else XR_HIP(hipStreamSynchronize(engine().stream));
        XR_REQUIRE(!polled || host[8] == seq, XR_ERR_HIP, "mesh statistics did not arrive");
    }
    for (int i = 0; i < stat::N_SLOTS; i++) h[i] = host[i];
    valid = true;
}

// the caller-order arrays of a preparation as a QUERY, by raggedness, and the flags that say so
static void alloc_query_depth(xr_mesh *mesh) {
    const int64_t F = mesh->n_face;
    const bool dense = !mesh->ragged(); // (ragged: flat vertex blocks, filled on demand by mesh_face_coords)
    if (dense) mesh->prep.fxy.alloc((size_t)F * mesh->m * 2);
    mesh->prep.len.alloc((size_t)F);
    // (dense meshes keep no box array: whoever needs a face's box takes it from the vertices, query_face_box in xr_geom.h --
    // 32 of the prepare kernel's 81 bytes per triangle, and the overlap kernels were the only readers)
    if (!dense) mesh->prep.bbox.alloc((size_t)F * 4);
    mesh->prep.fxy_valid = dense;
    mesh->prep.has_attrs = true;
}

void mesh_prepare(xr_mesh *mesh, bool want_fxy, bool stats_on_side, bool allow_sampled) {
    // two depths: statistics only (want_fxy = false: the mesh is used as a tree) or statistics + the caller-order
    // len / bbox / vertex blocks a query needs.  A mesh prepared light and later used as a query is prepared again;
    // so is one whose statistics come from a sample when exact ones are asked for.
    if (mesh->stats.launched && (mesh->prep.has_attrs || !want_fxy) && (!mesh->stats.sampled || allow_sampled)) return;
    const int64_t F = mesh->n_face;
    const int m = mesh->m;
    // Polygon (ragged) meshes always keep len / bbox: the index build then reads one coalesced 32-byte box per face instead
    // of gathering the face's 6-20 vertices again in both of its passes (Voronoi tessellation of 1M triangles:
    // index_count 0.134 -> see DESIGN, index_scatter 0.067 ms).
    if (mesh->ragged()) want_fxy = true;
    if (!want_fxy && allow_sampled && F >= SAMPLE_MIN_FACES && !mesh->prep.has_attrs) {
        mesh->stats.dev.alloc(8);
        const int64_t nb_all = (F + PREP_BLOCK - 1) / PREP_BLOCK;
        const int64_t nb = (nb_all + SAMPLE_STRIDE - 1) / SAMPLE_STRIDE;
        DevBuf<double> partials((size_t)nb * 8);
        dim3 grid((unsigned)nb), block(PREP_BLOCK);
        const StatsTail tail = mesh->stats.begin(partials.get(), nb);
        with_nodes_per_face(m, [&](auto mc) {
            XR_LAUNCH("sample_stats", k_sample_stats<mc()>, grid, block, 0, mesh->node_xy.get(), mesh->n_node, mesh->faces_raw.get(),
                      F, m, SAMPLE_STRIDE, partials.get(), tail);
        });
        mesh->stats.enqueued(partials.get(), nb, tail, stats_on_side);
        mesh->stats.sampled = true;
        return;
    }
    mesh->stats.sampled = false;
    if (want_fxy) alloc_query_depth(mesh);
    else mesh->prep.fxy_valid = mesh->prep.has_attrs = false;
    mesh->stats.dev.alloc(8);
    const int64_t nb = std::max<int64_t>(1, (F + PREP_BLOCK - 1) / PREP_BLOCK);
    DevBuf<double> partials((size_t)nb * 8);
    dim3 grid((unsigned)nb), block(PREP_BLOCK);
    const StatsTail tail = mesh->stats.begin(partials.get(), nb);
    with_nodes_per_face(m, [&](auto mc) {
        if (want_fxy)
            XR_LAUNCH("prepare_faces", (k_prepare_faces<mc(), false>), grid, block, 0, mesh->node_xy.get(), mesh->faces_raw.get(), F,
                      m, mesh->ragged() ? (double *)nullptr : mesh->prep.fxy.get(), mesh->prep.len.get(), mesh->prep.bbox.get(), partials.get(), tail);
        else
            XR_LAUNCH("prepare_stats", (k_prepare_faces<mc(), true>), grid, block, 0, mesh->node_xy.get(), mesh->faces_raw.get(), F,
                      m, (double *)nullptr, (uint8_t *)nullptr, (double *)nullptr, partials.get(), tail);
    });
    mesh->stats.enqueued(partials.get(), nb, tail, stats_on_side);
}

// The front of a weight build in ONE launch (k_prepare_faces<., ., MT>): the tree's sampled statistics lead the query's preparation.
// Taken where mesh_prepare(tree, false, true, true) would run k_sample_stats with its in-kernel tail and
// mesh_prepare(query, true, true) k_prepare_faces of a dense mesh; every other pair gets exactly those two calls.  The state both
// meshes end in is written by what those calls use too: alloc_query_depth, MeshStatsBox::begin / enqueued.
void mesh_prepare_pair(xr_mesh *tree, xr_mesh *query) {
    const int64_t S = tree->n_face, T = query->n_face;
    const int64_t nb_sample = div_up(div_up(S, (int64_t)PREP_BLOCK), (int64_t)SAMPLE_STRIDE);
    const int64_t nb_query = std::max<int64_t>(1, div_up(T, (int64_t)PREP_BLOCK));
    const auto tri_or_quad = [](const xr_mesh *mesh) { return mesh->m == 3 || mesh->m == 4; }; // (the dense meshes there are)
    const bool pair = option(OPT_FRONT_FUSED) != 0 && tree != query && tri_or_quad(tree) && tri_or_quad(query) &&
                      !tree->stats.launched && S >= SAMPLE_MIN_FACES && !tree->prep.has_attrs && stats_tail_in_kernel(nb_sample) &&
                      !(query->stats.launched && query->prep.has_attrs && !query->stats.sampled) &&
                      nb_sample + nb_query < ((int64_t)1 << 31);
    if (!pair) {
        mesh_prepare(tree, false, /*stats_on_side=*/true, /*allow_sampled=*/true); // (bounds exact, mean extent sampled)
        host_stamp(1);
        mesh_prepare(query, true, /*stats_on_side=*/true); // (its statistics are first read by mesh_query_order)
        return;
    }
    tree->stats.dev.alloc(8);
    DevBuf<double> t_partials((size_t)nb_sample * 8);
    const StatsTail t_tail = tree->stats.begin(t_partials.get(), nb_sample); // (in-kernel: the conditions above are its own)
    query->stats.sampled = false;
    alloc_query_depth(query);
    query->stats.dev.alloc(8);
    DevBuf<double> q_partials((size_t)nb_query * 8);
    const StatsTail q_tail = query->stats.begin(q_partials.get(), nb_query);
    const SampleArgs sample{tree->node_xy.get(), tree->n_node, tree->faces_raw.get(), S, SAMPLE_STRIDE, t_partials.get(), t_tail};
    const dim3 grid((unsigned)(nb_sample + nb_query)), block(PREP_BLOCK);
    const auto launch = [&](auto mt, auto mq) {
        XR_LAUNCH("prepare_faces", (k_prepare_faces<mq(), false, mt()>), grid, block, 0, (int)nb_sample, sample, query->node_xy.get(),
                  query->faces_raw.get(), T, query->prep.fxy.get(), query->prep.len.get(), q_partials.get(), q_tail);
    };
    const std::integral_constant<int, 3> m3;
    const std::integral_constant<int, 4> m4;
    if (tree->m == 3) query->m == 3 ? launch(m3, m3) : launch(m3, m4);
    else query->m == 3 ? launch(m4, m3) : launch(m4, m4);
    tree->stats.enqueued(t_partials.get(), nb_sample, t_tail, true);
    tree->stats.sampled = true;
    host_stamp(1);
    query->stats.enqueued(q_partials.get(), nb_query, q_tail, true);
}

const double *mesh_area(xr_mesh *mesh) {
    if (mesh->prep.area_valid) return mesh->prep.area.get();
    const int64_t F = mesh->n_face;
    mesh->prep.area.alloc((size_t)F);
    if (F > 0) {
        const dim3 grid(div_up(F, 256)), block(256);
        with_nodes_per_face(mesh->m, [&](auto mc) {
            XR_LAUNCH("face_area", k_face_area<mc()>, grid, block, 0, mesh->node_xy.get(), mesh->faces_raw.get(), F, mesh->m,
                      mesh->prep.area.get());
        });
    }
    mesh->prep.area_valid = true;
    return mesh->prep.area.get();
}

void mesh_read_stats(xr_mesh *mesh, bool need_exact) {
    if (!mesh->stats.launched) mesh_prepare(mesh, false);
    else if (need_exact && mesh->stats.sampled) mesh_prepare(mesh, mesh->prep.has_attrs, false, false); // over all faces this time
    mesh->stats.read();
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_mesh_prepare(xr_mesh *mesh) {
    XR_API_BEGIN
    XR_REQUIRE(mesh, XR_ERR_INVALID, "xr_mesh_prepare: NULL mesh");
    mesh_prepare(mesh);
    stream_sync();
    XR_API_END
}

int xr_mesh_area(xr_mesh *mesh, double *area_out) {
    XR_API_BEGIN
    XR_REQUIRE(mesh && area_out, XR_ERR_INVALID, "xr_mesh_area: NULL argument");
    const double *area = mesh_area(mesh);
    if (mesh->n_face > 0) {
        d2h(area_out, area, sizeof(double) * (size_t)mesh->n_face);
    }
    stream_sync();
    XR_API_END
}

} // extern "C"
