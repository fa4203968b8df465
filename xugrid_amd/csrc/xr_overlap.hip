// xr_overlap.hip -- OverlapRegridder weight construction on the device.
//
// Replaces numba_celltree.CellTree2d.intersect_faces as called from
// UnstructuredGrid2d.overlap (xugrid/regrid/unstructured.py:109-135), the relative
// normalisation (:133-134) and MatrixCSR.from_triplet (xugrid/regrid/regridder.py:433-435,
// xugrid/core/sparse.py:61-78).
//
// Two pipelines.  Dense meshes of at most 4 nodes per face (triangle x triangle: the benchmark) take overlap_tri(),
// xr_overlap_fused.hip: search -> persistent clip -> per-block scan -> assembly, big faces on a side stream, ONE host round
// trip.  Everything else takes the general chain, overlap_general() in xr_overlap_general.hip (all on the engine stream):
//   search         one thread per query (target) face walks the tree mesh's hierarchical grid and
//                  parks the bbox-overlapping tree records in 16 LDS slots; the block reserves its
//                  stretch of the candidate-pair queue with one atomic and writes it compacted
//                                               -> cand_off/cand_count[T], cand_tgt/src[C]
//   search_big     faces with too many rows / records / hits: block per face, count -> reserve -> fill
//   clip           one thread per candidate pair: Sutherland-Hodgman clip of the query polygon
//                  by the tree polygon, polygon buffers staged in LDS ([vertex][thread] layout,
//                  conflict-free 16-byte accesses), fan area                 -> cand_area[C]
//                  per-row counts of pairs with area > 0 by wave-aggregated atomics -> nnz_row[T]
//   scan           -> indptr[T+1]
//   row_fill       per query face: rank the surviving pairs by tree face id and write the CSR
//                  row (indices, data); data /= tree face area if relative.  Rows with many
//                  candidates go to one block each (all-pairs or LDS bitmap rank, k_row_fill_long).
// Query faces whose bbox spans many grid rows/records are searched by one block each
// (k_search_big) instead of one thread.
//
// THIS unit holds what both pipelines use -- k_search, k_search_big, k_row_fill_long and their launchers (declared in
// xr_overlap.h), the dust threshold, the rows' tiling keys -- and the entry points.  Device code of the clips: xr_clip.h.
#include "xr_overlap.h"
#include "xr_mesh_plan.h"
#include "xr_apply.h"
#include "xr_clip.h"

namespace xr {

// ---------------------------------------------------------------------------------------------
// candidate search
// ---------------------------------------------------------------------------------------------
// A query face is "big" when its bbox spans many grid rows or many records (hull slivers of a
// Delaunay mesh, coarse target cells over a fine source): one thread would serialise thousands
// of tests, so those faces are queued and handled by one block each (k_search_big).
static constexpr int BIG_VISITS = 160; // records visited by one thread before it gives up

static constexpr int TILE_RUN = 16; // rows per run in the tiling hint (128-byte output stores per variable).  Measured, K = 256 on
                                    // the benchmark matrix: runs of 64 rows / tiles of 24 extents 2.10 ms, 16 / 12: 1.72 ms (a qhull-numbered
                                    // target: long runs of consecutive ids are not compact); a lattice-numbered pair 0.99 ms either way

// Level split: the walk only visits the grid levels that hold the bulk of the records.  The records of the upper
// levels (a Delaunay hull's slivers: a few hundred of a million) are the TAIL of the record arrays (levels are
// concatenated); when that tail is short (<= BIGREC_MAX) every block filters it against its own bounding box once
// (coalesced) and its faces test the few survivors from LDS, instead of every face walking 5-6 all but empty levels:
// the dependent cell_start -> record round trips of those levels were most of the search time.
static constexpr int WALK_PAD = MeshIndex::REC_BB_PAD; // records of padding behind rec_bb: the walk's unclamped loads
static constexpr int BIGREC_MAX = 1024;  // records of the upper grid levels handled as a list
static constexpr int BIGREC_BLOCK = 64;  // ... of which at most this many may touch one block's bounding box

// PACK: the owning thread of a parked candidate rides in the top 8 bits of the record id (trees of at most 2^24 faces) instead
// of a byte array of its own: 19.5 instead of 23.5 KB of LDS per block = 8 instead of 6 resident blocks per CU for a
// kernel that is a chain of dependent loads.
// (The f32 box test of a step through subtract / max, 62 vector instructions per step of four records.  Two cheaper forms --
// compares combined on the scalar unit: 37 + 28 scalar; packed adds: 47 + 10 -- were measured in round 5 and changed nothing:
// the kernel waits on memory.  They are gone.)
// MC: nodes per query face (3, 4: the face's box comes from its vertices, query_face_box; 0: a polygon mesh's stored box).
template <bool PACK, int MC>
__global__ void __launch_bounds__(256)
k_search(const double *__restrict__ q_bbox, const double *__restrict__ q_fxy, const uint8_t *__restrict__ q_len,
         int64_t n_query, GridParams g, int64_t n_tree,
         const int32_t *__restrict__ cell_start,
         const float *__restrict__ rec_bb, int32_t *__restrict__ cand_count, int32_t *__restrict__ cand_off,
         int32_t *__restrict__ cand_tgt, int32_t *__restrict__ cand_src, int32_t *__restrict__ queue_cursor,
         int2 *__restrict__ block_seg, uint8_t *__restrict__ is_big, int32_t *__restrict__ big_list,
         int32_t *__restrict__ n_big, MortonParams tile, int32_t *__restrict__ tile_key, int32_t *__restrict__ nnz_row,
         bool remap, int32_t *__restrict__ blk_rows = nullptr /* optional: regular (non-big) faces per block, written */,
         int32_t *__restrict__ blk_surv = nullptr /* optional: the clip's survivor count of the block, cleared here */,
         int region_cap = 0 /* > 0: EIGHT queue regions of this many pairs with a cursor each (queue_cursor[0..7]), one per XCD */) {
    __shared__ __attribute__((aligned(16))) int32_t sh_slots[SLOTS + 1][256]; // [slot][thread]: conflict-free; + trash row
    __shared__ uint8_t sh_owner[PACK ? 1 : SLOTS * 256];
    __shared__ __attribute__((aligned(16))) float4 sh_bigbb[BIGREC_BLOCK];
    __shared__ int32_t sh_bigrec[BIGREC_BLOCK];
    __shared__ float sh_box[4][4];
    __shared__ int32_t sh_nbig;
    __shared__ int32_t sh_wave[4];
    __shared__ int32_t sh_base;
    const int64_t n_blocks = (n_query + 255) / 256;
    const int64_t lb = xcd_block(n_blocks, remap);
    if (threadIdx.x == 0 && blk_surv) blk_surv[lb] = 0; // (every hardware block owns one word, also the idle ones of the rounded grid)
    if (lb >= n_blocks) {
        if (threadIdx.x == 0 && blk_rows) blk_rows[lb] = 0;
        return;
    }
    const int64_t t = lb * 256 + threadIdx.x;
    const float4 *__restrict__ rbb = reinterpret_cast<const float4 *>(rec_bb);
    // ---- level split (uniform: scalar loads)
    int l_split = g.n_levels, big0 = (int)n_tree;
    for (int l = g.n_levels - 1; l >= 1; l--) {
        const int first = cell_start[g.base[l]];
        if ((int)n_tree - first > BIGREC_MAX) break;
        l_split = l;
        big0 = first;
    }
    double4 bb = make_double4(0, 0, 0, 0);
    float qx0 = INFINITY, qx1 = -INFINITY, qy0 = INFINITY, qy1 = -INFINITY;
    if (t < n_query) {
        bb = query_face_box<MC>(q_bbox, q_fxy, q_len, t);
        qx0 = f32_below(bb.x - g.x0), qx1 = f32_above(bb.y - g.x0);
        qy0 = f32_below(bb.z - g.y0), qy1 = f32_above(bb.w - g.y0);
    }
    // Sparse levels in between (round 4): from the lowest level on whose tail holds at most 1/64 of the records (the 1M benchmark:
    // levels 2-4, 0.6 % of the records, ~0.05 per face -- but every face paid their cell bounds: three of its ~15 dependent
    // round trips and 11 % of its instructions), the levels [l_coop, l_split) are walked ONCE PER BLOCK: thread i takes grid
    // row i of the block's box on one of those levels, and the records that touch the box join the LDS list below.
    int l_coop = l_split;
    for (int l = l_split - 1; l >= 1; l--) {
        const int first = cell_start[g.base[l]];
        if (((int64_t)big0 - first) * 64 > n_tree) break;
        l_coop = l;
    }
    if (threadIdx.x == 0) sh_nbig = 0;
    if (big0 < (int)n_tree || l_coop < l_split) {
        // the block's bounding box, then one coalesced pass over the big records
        float bx0 = wave_reduce<OpMin>(qx0), bx1 = wave_reduce<OpMax>(qx1), by0 = wave_reduce<OpMin>(qy0), by1 = wave_reduce<OpMax>(qy1);
        if ((threadIdx.x & 63) == 0) {
            const int w = threadIdx.x >> 6;
            sh_box[w][0] = bx0; sh_box[w][1] = bx1; sh_box[w][2] = by0; sh_box[w][3] = by1;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; w++) {
            bx0 = fminf(bx0, sh_box[w][0]); bx1 = fmaxf(bx1, sh_box[w][1]);
            by0 = fminf(by0, sh_box[w][2]); by1 = fmaxf(by1, sh_box[w][3]);
        }
        for (int r = big0 + threadIdx.x; r < (int)n_tree; r += 256) {
            const float4 rb = rbb[r];
            if (rec_hit(rb, bx0, bx1, by0, by1)) {
                const int k = atomicAdd(&sh_nbig, 1);
                if (k < BIGREC_BLOCK) {
                    sh_bigrec[k] = r;
                    sh_bigbb[k] = rb;
                }
            }
        }
        if (l_coop < l_split) {
            // level-0 cells of the box's corners (the float box is a superset of every face's box; same monotone cell function
            // and the same shifts as the per-thread walk below)
            const int bcx0 = cell_coord((double)bx0 + g.x0, g.x0, g.inv_h0, g.nx[0]), bcx1 = cell_coord((double)bx1 + g.x0, g.x0, g.inv_h0, g.nx[0]);
            const int bcy0 = cell_coord((double)by0 + g.y0, g.y0, g.inv_h0, g.ny[0]), bcy1 = cell_coord((double)by1 + g.y0, g.y0, g.inv_h0, g.ny[0]);
            int n_items = 0;
            for (int l = l_coop; l < l_split; l++) n_items += (bcy1 >> (l * LEVEL_SHIFT)) - max((bcy0 >> (l * LEVEL_SHIFT)) - 1, 0) + 1;
            if (n_items > 256) {
                l_coop = l_split; // (a block spanning too many grid rows: its faces walk these levels themselves)
            } else if ((int)threadIdx.x < n_items) {
                int it = threadIdx.x, l = l_coop;
                for (;; l++) {
                    const int rows = (bcy1 >> (l * LEVEL_SHIFT)) - max((bcy0 >> (l * LEVEL_SHIFT)) - 1, 0) + 1;
                    if (it < rows) break;
                    it -= rows;
                }
                const int sh = l * LEVEL_SHIFT, nx = g.nx[l], base = g.base[l];
                const int cy = max((bcy0 >> sh) - 1, 0) + it;
                const int cx0 = max((bcx0 >> sh) - 1, 0), cx1 = bcx1 >> sh;
                const int r0 = cell_start[base + cy * nx + cx0], r1 = cell_start[base + cy * nx + cx1 + 1];
                for (int r = r0; r < r1; r++) {
                    const float4 rb = rbb[r];
                    if (rec_hit(rb, bx0, bx1, by0, by1)) {
                        const int k = atomicAdd(&sh_nbig, 1);
                        if (k < BIGREC_BLOCK) {
                            sh_bigrec[k] = r;
                            sh_bigbb[k] = rb;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (sh_nbig > BIGREC_BLOCK) { // too many for the list: this block walks every level
            l_split = g.n_levels;
            l_coop = l_split;
            __syncthreads();
            if (threadIdx.x == 0) sh_nbig = 0;
        }
    }
    __syncthreads();
    const int n_bigblk = sh_nbig;
    int count = 0;
    bool big = false;
    if (t < n_query) {
        nnz_row[t] = 0; // the clip kernel counts the surviving pairs of the row into it
        if (tile_key) {
            // row tiling hint for the many-variable apply: all rows of a run of TILE_RUN consecutive ids share the
            // key of the run's middle row, so runs stay contiguous (long output stores) and neighbouring runs meet
            const int64_t mid = (t & ~(int64_t)(tile.n_run - 1)) + tile.n_run / 2;
            tile_key[t] = morton_key(tile, query_face_box<MC>(q_bbox, q_fxy, q_len, mid < n_query ? mid : n_query - 1));
        }
        // Level-0 cells of the bbox corners, once; the level-l cell of x is (level-0 cell) >> l exactly (cell
        // sizes are power-of-two multiples and the clamped ranges nest), and the cell of x - h_l is that minus one:
        // no per-level floating-point cell arithmetic.  (A record that can overlap has xmin > q.xmin - 0.999 h_l,
        // so its cell is >= cell(q.xmin) - 1 for the same monotone cell function the index was built with.)
        const int c_x0 = cell_coord(bb.x, g.x0, g.inv_h0, g.nx[0]), c_x1 = cell_coord(bb.y, g.x0, g.inv_h0, g.nx[0]);
        const int c_y0 = cell_coord(bb.z, g.y0, g.inv_h0, g.ny[0]), c_y1 = cell_coord(bb.w, g.y0, g.inv_h0, g.ny[0]);
        constexpr int WALK_LOADS = 4;
        int visited = 0, n_rows = 0;
        for (int l = 0; l < l_coop; l++)
            n_rows += (c_y1 >> (l * LEVEL_SHIFT)) - max((c_y0 >> (l * LEVEL_SHIFT)) - 1, 0) + 1;
        big = n_rows > 8 * l_coop + 8;
        for (int l = 0; l < l_coop && !big; l++) {
            const int nx = g.nx[l], base = g.base[l];
            const int sh = l * LEVEL_SHIFT;
            const int cx0 = max((c_x0 >> sh) - 1, 0), cx1 = c_x1 >> sh;
            const int cy0 = max((c_y0 >> sh) - 1, 0), cy1 = c_y1 >> sh;
            for (int cyb = cy0; cyb <= cy1 && !big; cyb += 4) {
                // fetch the record runs of up to four grid rows before walking them
                int r0[4], r1[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int cy = cyb + k <= cy1 ? cyb + k : cy1;
                    r0[k] = cell_start[base + cy * nx + cx0];
                    r1[k] = cyb + k <= cy1 ? cell_start[base + cy * nx + cx1 + 1] : r0[k];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    visited += r1[k] - r0[k];
                    if (visited > BIG_VISITS) big = true;
                    if (!big) {
                        for (int r = r0[k]; r < r1[k]; r += WALK_LOADS) {
                            // WALK_LOADS independent 16-byte loads in flight per step (6 and 8 measured in round 4: no faster)
                            const int last = r1[k] - 1;
                            float4 bx[WALK_LOADS];
                            static_assert(WALK_LOADS - 1 <= WALK_PAD, "rec_bb padding");
                            // (no clamp of the index: rec_bb is padded by WALK_PAD records, a load beyond the run reads the next
                            // run or the padding and is masked below; PACK: ONE 32-bit byte offset from the uniform base per step --
                            // at most 2^24 records of 16 bytes -- and the records behind it through the instruction's immediate offset)
                            const char *step_base = reinterpret_cast<const char *>(rbb) + ((uint32_t)r << 4);
#pragma unroll
                            for (int u = 0; u < WALK_LOADS; u++)
                                bx[u] = PACK ? *reinterpret_cast<const float4 *>(step_base + 16 * u) : rbb[r + u];
                            // branch-free parking: the slot is written unconditionally and only kept (count advances) on a hit;
                            // beyond SLOTS everything lands in a trash row
#pragma unroll
                            for (int u = 0; u < WALK_LOADS; u++) {
                                sh_slots[count < SLOTS ? count : SLOTS][threadIdx.x] = r + u;
                                count += fmaxf(box_gap(bx[u], qx0, qx1, qy0, qy1), r + u <= last ? -INFINITY : 1.0f) < 0.0f ? 1 : 0;
                            }
                        }
                    }
                }
            }
        }
        // the big records that touch the block (from LDS)
        for (int k = 0; k < n_bigblk && !big; k++) {
            const bool h = rec_hit(sh_bigbb[k], qx0, qx1, qy0, qy1);
            sh_slots[count < SLOTS ? count : SLOTS][threadIdx.x] = sh_bigrec[k];
            count += h ? 1 : 0;
        }
        if (count > SLOTS) big = true;
        is_big[t] = big ? 1 : 0;
        if (big) big_list[atomicAdd(n_big, 1)] = (int32_t)t;
    }
    // The block's candidates go straight into the pair queue: block-level exclusive scan of the counts, ONE
    // atomic reservation per block, then the entries -- compacted in LDS -- are written as whole lines.  No
    // slot array, no global scan, no compaction pass; blocks land in the queue in arbitrary order (nothing
    // downstream depends on it: rows are re-ranked by tree face id), the rows of one block stay contiguous.
    const int mine = (t < n_query && !big) ? count : 0;
    if (blk_rows) {
        const int n_regular = __syncthreads_count(t < n_query && !big);
        if (threadIdx.x == 0) blk_rows[lb] = n_regular;
    }
    int own[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; j++) own[j] = j < mine ? sh_slots[j][threadIdx.x] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(mine);
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads(); // (also: every thread has read its slots)
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) woff += sh_wave[w];
        total += sh_wave[w];
    }
    const int lo = woff + incl - mine;
    // One returning atomic per block on ONE word is served at the memory side at ~10 M a second when thousands of blocks queue up
    // for it (10 us of this kernel, measured by giving every block a fixed stretch instead).  With region_cap > 0 the queue is
    // eight dense regions, one per XCD (hardware block b runs on XCD b mod 8, and with the XCD-aware block order that XCD owns a
    // contiguous eighth of the target faces): eight words share the traffic, and the persistent clip deals its chunks per
    // region anyway.
    if (threadIdx.x == 0) {
        const int x = region_cap > 0 ? (int)(blockIdx.x & 7) : 0;
        sh_base = (total > 0 ? atomicAdd(&queue_cursor[x * QCUR_STRIDE], total) : 0) + x * region_cap;
    }
    int32_t *flat = &sh_slots[0][0];
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        if (j < mine) {
            flat[lo + j] = PACK ? (own[j] | (int32_t)(threadIdx.x << 24)) : own[j];
            if (!PACK) sh_owner[lo + j] = (uint8_t)threadIdx.x;
        }
    }
    __syncthreads();
    const int base = sh_base;
    if (t < n_query && !big) { // big faces get their offset and count from k_search_big<false>
        cand_off[t] = base + lo;
        cand_count[t] = mine;
    }
    if (threadIdx.x == 0) block_seg[lb] = make_int2(base, total);
    const int32_t t0 = (int32_t)(lb * 256);
    for (int i = threadIdx.x; i < total; i += 256) {
        const int32_t v = flat[i];
        cand_tgt[base + i] = t0 + (PACK ? (int32_t)((uint32_t)v >> 24) : (int32_t)sh_owner[i]);
        cand_src[base + i] = PACK ? (v & 0xffffff) : v;
    }
}

// One block per big query face.  The face is scan-converted against the grid: for grid row cy of
// level l only the cells under the polygon's x-extent inside the y-slab of that row are visited
// (a thin hull sliver touches O(length) cells instead of the O(length^2) cells of its bbox).
// Lanes take one grid row each (64 rows per batch, batches dealt round-robin to the block's four
// waves); runs longer than LONG_RUN records are processed by the whole wave in 64-record chunks.
//
// Superset argument: a tree face s on level l with positive-area intersection has a point p in
// both polygons; its record sits in the cell of (xmin_s, ymin_s) with p.x - h < xmin_s <= p.x and
// p.y - h < ymin_s <= p.y (extent <= 0.999 h).  So for row cy the relevant points have
// y in [Y(cy), Y(cy) + 2h) and the record's cell column lies in [cell(xlo - h), cell(xhi)], with
// [xlo, xhi] the polygon's x-extent inside that slab (inflated by 1e-6 h against rounding).
static constexpr int LONG_RUN = 128;

// FUSED: ONE walk parks the face's candidates in LDS (up to BIG_STAGE of them); the block then reserves the face's
// stretch of the pair queue with one atomic and copies them out.  Faces with more candidates than the stage holds
// walk a second time and write straight to the queue (the first walk has counted them); faces whose stretch does
// not fit the queue as currently allocated are listed and filled by a second launch (FUSED = false) after the host
// regrew it.  (The two-walk version -- count, reserve, fill -- took twice as long per face, and a big face is a
// chain of dependent phases: the kernel's duration is the slowest face's.)
static constexpr int BIG_STAGE = 5120; // size of the stage (dynamic LDS; 3072 / 2048 / 1024 / 512 measured in round 5: no gain)
static constexpr int BIG_RANK_MAX = 1 << 16; // big faces ranked by id (all-pairs, inside k_search_big); longer lists keep their order

template <bool FUSED>
__global__ void __launch_bounds__(256)
k_search_big(const double *__restrict__ q_bbox, const double *__restrict__ q_fxy,
             const uint8_t *__restrict__ q_len, const int32_t *__restrict__ q_off, int q_m, GridParams g,
             const int32_t *__restrict__ cell_start, const float *__restrict__ rec_bb,
             const int32_t *__restrict__ rec_face, const int32_t *__restrict__ big_list,
             const int32_t *__restrict__ n_big, int32_t *__restrict__ cand_off, int32_t *__restrict__ cand_count,
             int32_t *__restrict__ cand_tgt, int32_t *__restrict__ cand_src, int32_t *__restrict__ queue_cursor,
             int64_t capacity, int32_t *__restrict__ pending_list, int32_t *__restrict__ n_pending,
             int big_stage /* entries of the LDS stage (FUSED) */,
             int32_t *__restrict__ slot_face = nullptr /* optional: the listed faces in ascending id order, written */) {
    __builtin_amdgcn_s_setprio(3); // side-stream kernel: its waves go first in the SIMDs' issue arbitration (see overlap_tri)
    // one BLOCK per big face: its four waves take the 64-row batches round-robin; candidates are
    // appended through a per-face cursor in LDS (their order inside the row is irrelevant: rows are
    // ranked by tree face id afterwards)
    __shared__ double2 sh_poly[XR_MAX_FACE_NODES];
    __shared__ double4 sh_bb;
    extern __shared__ int32_t sh_stage[]; // [big_stage] (FUSED) / [1]
    __shared__ int sh_cursor;
    __shared__ int sh_out0;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nb = *n_big;
    const float4 *__restrict__ rbb = reinterpret_cast<const float4 *>(rec_bb);
    const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    __shared__ int32_t sh_rankw[4];
    for (int bi = blockIdx.x; bi < nb; bi += gridDim.x) {
        const int t = big_list[bi];
        const int np = q_len[t];
        if (slot_face) {
            // the face's rank among the listed ones by face id (k_search lists them in finishing order; ranking makes the
            // stored matrix the same from run to run).  Lists beyond BIG_RANK_MAX faces keep the order they were found in.
            int c = 0;
            if (nb <= BIG_RANK_MAX)
                for (int j = threadIdx.x; j < nb; j += 256) c += big_list[j] < t ? 1 : 0;
            c = wave_reduce<OpSum>(c);
            if (lane == 0) sh_rankw[wv] = c;
        }
        __syncthreads();
        if (slot_face && threadIdx.x == 0)
            slot_face[nb <= BIG_RANK_MAX ? sh_rankw[0] + sh_rankw[1] + sh_rankw[2] + sh_rankw[3] : bi] = t;
        if (threadIdx.x < np) sh_poly[threadIdx.x] = reinterpret_cast<const double2 *>(q_fxy)[face_vertex_base(q_off, t, q_m) + threadIdx.x];
        if (threadIdx.x == 0) {
            sh_cursor = 0;
            sh_bb = query_face_box_rt(q_bbox, q_fxy, q_len, q_m, t); // (dense meshes store no box)
        }
        __syncthreads();
        const double2 *poly = sh_poly;
        const double4 bb = sh_bb;
        const float qx0 = f32_below(bb.x - g.x0), qx1 = f32_above(bb.y - g.x0);
        const float qy0 = f32_below(bb.z - g.y0), qy1 = f32_above(bb.w - g.y0);
        for (int pass = FUSED ? 0 : 1; pass < 2; pass++) {
        const bool STAGE = pass == 0; // first walk: park in LDS (and count); second walk: write to the queue
        if (!STAGE) {
            if (FUSED) {
                // (the first walk left the face's total in sh_cursor)
                __syncthreads();
                const int n = sh_cursor;
                __syncthreads();
                if (threadIdx.x == 0) {
                    const int base = atomicAdd(queue_cursor, n);
                    cand_count[t] = n;
                    cand_off[t] = base;
                    const bool fits = (int64_t)base + n <= capacity && base >= 0;
                    if (!fits) pending_list[atomicAdd(n_pending, 1)] = t;
                    sh_out0 = fits ? base : -1;
                    sh_cursor = 0;
                }
                __syncthreads();
                const int out = sh_out0;
                if (out < 0) break;
                if (n <= big_stage) { // everything is parked: copy it out, no second walk
                    for (int i = threadIdx.x; i < n; i += 256) {
                        cand_tgt[out + i] = t;
                        cand_src[out + i] = sh_stage[i];
                    }
                    break;
                }
            } else {
                if (threadIdx.x == 0) sh_out0 = cand_off[t];
                __syncthreads();
            }
            if (sh_out0 < 0) break;
        }
        const int out0 = STAGE ? 0 : sh_out0;
        for (int l = 0; l < g.n_levels; l++) {
            const double h = level_h(g, l), inv_h = level_inv_h(g, l);
            const double eps = 1e-6 * h;
            const int nx = g.nx[l], ny = g.ny[l], base = g.base[l];
            const int cy0 = cell_coord(bb.z - h, g.y0, inv_h, ny), cy1 = cell_coord(bb.w, g.y0, inv_h, ny);
            int batch_id = 0;
            for (int cyb = cy0; cyb <= cy1; cyb += 64, batch_id++) {
                if (((batch_id + l) & 3) != wv) continue;
                const int cy = cyb + lane;
                int r0 = 0, r1 = 0;
                // (the record test uses the polygon's x-extent INSIDE the row's slab, not the face's whole box: a record of this
                // row lies inside the slab in y, so a common point with the polygon has its x inside that extent -- the same
                // argument that lets the walk skip the cells beside it.  For a diagonal sliver this is the difference between
                // "every record of every visited cell" and the records along the sliver: the longest face of the 1M benchmark
                // went from ~4000 candidates, 763 of them real, to a third.)
                float rx0 = qx0, rx1 = qx1;
                if (cy <= cy1) {
                    // polygon x-extent inside the slab [ya, yb] of this grid row
                    const double ya = g.y0 + (double)cy * h - eps, yb = g.y0 + (double)(cy + 2) * h + eps;
                    double xlo = INFINITY, xhi = -INFINITY;
                    double2 p = poly[np - 1];
                    for (int k = 0; k < np; k++) {
                        const double2 q = poly[k];
                        const double ylo = fmin(p.y, q.y), yhi = fmax(p.y, q.y);
                        if (yhi >= ya && ylo <= yb) {
                            double xa = p.x, xb = q.x;
                            if (yhi > ylo) {
                                // clip the edge to the slab (parameter along p -> q)
                                const double inv = 1.0 / (q.y - p.y);
                                double t0 = (ya - p.y) * inv, t1 = (yb - p.y) * inv;
                                if (t0 > t1) { const double tmp = t0; t0 = t1; t1 = tmp; }
                                t0 = fmax(t0, 0.0);
                                t1 = fmin(t1, 1.0);
                                xa = p.x + t0 * (q.x - p.x);
                                xb = p.x + t1 * (q.x - p.x);
                            }
                            xlo = fmin(xlo, fmin(xa, xb));
                            xhi = fmax(xhi, fmax(xa, xb));
                        }
                        p = q;
                    }
                    if (xhi >= xlo) {
                        xlo = fmax(xlo - eps, bb.x);
                        xhi = fmin(xhi + eps, bb.y);
                        const int cx0 = cell_coord(xlo - h, g.x0, inv_h, nx), cx1 = cell_coord(xhi, g.x0, inv_h, nx);
                        r0 = cell_start[base + cy * nx + cx0];
                        r1 = cell_start[base + cy * nx + cx1 + 1];
                        rx0 = fmaxf(qx0, f32_below(xlo - g.x0));
                        rx1 = fminf(qx1, f32_above(xhi - g.x0));
                    }
                }
                const int len = r1 - r0;
                // (1) long runs: the whole wave, 64 records at a time
                unsigned long long long_mask = __ballot(len > LONG_RUN);
                while (long_mask) {
                    const int src_lane = __ffsll((long long)long_mask) - 1;
                    long_mask &= long_mask - 1;
                    const int R0 = __shfl(r0, src_lane, 64), R1 = __shfl(r1, src_lane, 64);
                    const float X0 = __shfl(rx0, src_lane, 64), X1 = __shfl(rx1, src_lane, 64);
                    for (int rb = R0; rb < R1; rb += 64) {
                        const int r = rb + lane;
                        const bool hit = r < R1 && rec_hit(rbb[r], X0, X1, qy0, qy1);
                        const unsigned long long mask = __ballot(hit);
                        const int n = __popcll(mask);
                        if (n > 0) {
                            int slot0 = 0;
                            if (lane == 0) slot0 = atomicAdd(&sh_cursor, n);
                            slot0 = __shfl(slot0, 0, 64);
                            if (hit) {
                                const int slot = slot0 + __popcll(mask & lt_mask);
                                if (STAGE) {
                                    if (slot < big_stage) sh_stage[FUSED ? slot : 0] = r;
                                } else {
                                    cand_tgt[out0 + slot] = t;
                                    cand_src[out0 + slot] = r;
                                }
                            }
                        }
                    }
                }
                // (2) short runs: one lane per grid row
                const int my_r1 = len > LONG_RUN ? r0 : r1;
                int cnt = 0;
                for (int r = r0; r < my_r1; r++) cnt += rec_hit(rbb[r], rx0, rx1, qy0, qy1) ? 1 : 0;
                const int excl = wave_incl_scan(cnt) - cnt;
                const int batch = __shfl(excl + cnt, 63, 64);
                if (batch > 0) {
                    int slot0 = 0;
                    if (lane == 0) slot0 = atomicAdd(&sh_cursor, batch);
                    slot0 = __shfl(slot0, 0, 64);
                    int pos = slot0 + excl;
                    for (int r = r0; r < my_r1; r++) {
                        if (rec_hit(rbb[r], rx0, rx1, qy0, qy1)) {
                            if (STAGE) {
                                if (pos < big_stage) sh_stage[FUSED ? pos : 0] = r;
                            } else {
                                cand_tgt[out0 + pos] = t;
                                cand_src[out0 + pos] = r;
                            }
                            pos++;
                        }
                    }
                }
            }
        }
        } // pass
    }
}

// Rows that do not fit the packed short-row path (candidates > ROW_SHORT) are listed by k_row_fill and
// finished by ONE kernel, one block per row: up to ROW_BLOCK candidates by an all-pairs rank (ids staged in
// LDS, 16-byte broadcast reads: a few microseconds), longer rows by the bitmap rank below.  (Separate
// wave-per-row / block-per-row / bitmap kernels were each pure latency on a few hundred rows: 14 + 21 + 26 us
// back to back.)
static constexpr int ROW_BLOCK = 512;

// Long rows: one block per row ranks the survivors by tree face id with an LDS bitmap.
// The id space [0, S) is processed in chunks of BM_BITS ids (one chunk covers a million tree faces): set one
// bit per survivor, count the bits of each thread's segment of BM_SEG words (rotated start -> bank-conflict
// free), scan the 256 segment totals, rank = (survivors in earlier chunks) + segment base + popcounts of
// the segment's words below + popc(bits below).  O(n + S/32) per row instead of O(n^2); any row length,
// any number of tree faces.  The row is read from HBM once, four candidates in flight per thread, and
// parked in LDS (survivor id or -1) for the later passes: the kernel is a chain of dependent phases on a
// handful of rows, i.e. pure latency.
static constexpr int BM_WORDS = 32768;          // 128 KiB of bitmap
static constexpr int BM_BITS = BM_WORDS * 32;   // ids per chunk
static constexpr int BM_SEG = BM_WORDS / 256;   // words per thread segment
static constexpr int BM_STAGE = 4096;           // candidates parked in LDS (16 KiB); longer rows re-read HBM
static constexpr size_t ROW_FILL_LIGHT_LDS = sizeof(int32_t) * (16 + BM_STAGE); // LDS of a k_row_fill_long launch with row_class = 1
static constexpr size_t ROW_FILL_LONG_LDS =                                    // ... of any other: + segment bases, bitmap, group counts
    ROW_FILL_LIGHT_LDS + sizeof(uint32_t) * (256 + BM_WORDS) + sizeof(uint16_t) * (BM_WORDS / 8);

// LIST: the launch also writes the apply's list of long rows (apply_long_rows, listed, n_stored; scan_nnz mode).  A template
// parameter, so that the launches that do not list -- the bitmap rows' is the one the weight build waits for -- carry none of it.
template <bool LIST>
__global__ void __launch_bounds__(256)
k_row_fill_long(const int32_t *__restrict__ cand_off, const int32_t *__restrict__ cand_count,
                const int32_t *__restrict__ cand_sid,
                const double *__restrict__ cand_area, const int32_t *__restrict__ indptr,
                const double *__restrict__ src_area, bool relative, int64_t n_tree, int32_t *__restrict__ indices,
                double *__restrict__ data, const int32_t *__restrict__ long_rows,
                const int32_t *__restrict__ n_long, int64_t row_base /* >= 0: list entry li is stored row row_base + li */,
                const int32_t *__restrict__ skip_if /* optional: nothing is done when this device word is > 0 */,
                const int32_t *__restrict__ scan_nnz = nullptr /* optional: row lengths per FACE; the offsets of the listed rows
                                                                  are then computed here (exclusive scan in list order) */,
                int32_t *__restrict__ scan_indptr = nullptr /* [n_long + 1], written */,
                int32_t *__restrict__ scan_total = nullptr /* total entries, written */,
                int row_class = 0 /* 0: every listed row; 1: only rows of at most ROW_BLOCK candidates -- the launch then needs
                                     ROW_FILL_LIGHT_LDS bytes of LDS instead of 150 KB, so its blocks find room beside other
                                     kernels and every row gets a block of its own; 2: only the rows beyond ROW_BLOCK */,
                int32_t *__restrict__ apply_long_rows = nullptr /* optional (scan_nnz mode): the listed rows of more than
                                                                   XR_APPLY_LONG_ROW entries are written to the apply's list
                                                                   as STORED rows n_stored - n_long + li, counted in `listed` */,
                FusedCounters *listed = nullptr, int64_t n_stored = 0) {
    __builtin_amdgcn_s_setprio(3); // side-stream kernel: its waves go first in the SIMDs' issue arbitration (see overlap_tri)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // (scratch and stage first: a row_class = 1 launch allocates nothing behind them)
    int32_t *red = reinterpret_cast<int32_t *>(smem);           // [16] scratch
    int32_t *stage = red + 16;                                  // [BM_STAGE]
    uint32_t *tbase = reinterpret_cast<uint32_t *>(stage + BM_STAGE); // [256] exclusive over thread segments
    uint32_t *bm = tbase + 256;                                 // [BM_WORDS]
    uint16_t *gcnt = reinterpret_cast<uint16_t *>(bm + BM_WORDS); // [BM_WORDS / 8] bits per 8 words -> prefix in segment
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (skip_if && *skip_if > 0) return;
    const int nl = *n_long;
    // block-wide sum of the lengths of the listed rows [k0, k1) (scan_nnz mode); *n_longer: how many of them the apply reduces
    // cooperatively (more than XR_APPLY_LONG_ROW entries), *longest: the longest of them
    auto length_sum = [&](int k0, int k1, int *n_longer, int *longest) -> long long {
        long long v = 0;
        int c = 0, m = 0;
        for (int k = k0 + tid; k < k1; k += 256) {
            const int len = scan_nnz[long_rows[k]];
            v += len;
            if (LIST) {
                c += len > XR_APPLY_LONG_ROW ? 1 : 0;
                m = len > m ? len : m;
            }
        }
        v = wave_reduce<OpSum>(v);
        if (LIST) {
            c = wave_reduce<OpSum>(c);
            m = wave_reduce<OpMax>(m);
        }
        __syncthreads();
        if (lane == 0) {
            red[wave] = (int32_t)(v > 0x7fffffffll ? 0x7fffffff : v);
            if (LIST) {
                red[4 + wave] = c;
                red[8 + wave] = m;
            }
        }
        __syncthreads();
        if (LIST) {
            *n_longer = red[4] + red[5] + red[6] + red[7];
            const int m01 = red[8] > red[9] ? red[8] : red[9], m23 = red[10] > red[11] ? red[10] : red[11];
            *longest = m01 > m23 ? m01 : m23;
        }
        return (long long)red[0] + red[1] + red[2] + red[3];
    };
    long long scan_base = 0; // offset of row blockIdx.x, advanced by gridDim.x rows per trip
    int list_base = 0;       // ... its place among the listed rows of more than XR_APPLY_LONG_ROW entries
    int list_max = 0;        // ... and the longest row in front of it
    if (scan_nnz) {
        scan_base = length_sum(0, blockIdx.x < nl ? (int)blockIdx.x : nl, &list_base, &list_max);
        if (blockIdx.x == 0 && nl == 0 && tid == 0) {
            scan_indptr[0] = 0;
            *scan_total = 0;
        }
    }
    for (int li = blockIdx.x; li < nl; li += gridDim.x) {
        const int t = long_rows[li];
        const int c0 = cand_off[t], n = cand_count[t];
        int base;
        if (scan_nnz) {
            const long long capped = scan_base > 0x7fffffffll ? 0x7fffffffll : scan_base;
            base = (int)capped;
            int len_t = 0; // (thread 0: the row's own length, fetched beside the loads of the sum below)
            if (tid == 0) {
                scan_indptr[li] = base;
                if (LIST || li == nl - 1) len_t = scan_nnz[t];
            }
            const int next = li + (int)gridDim.x;
            int longer = 0, longest = 0;
            scan_base += length_sum(li, next < nl ? next : nl, &longer, &longest);
            if (tid == 0) {
                if (LIST) {
                    // The apply's list of long rows, without an atomic (a thousand on one address are microseconds of the
                    // big faces' chain): the row's place in it is the number of long rows in front of it in the list, and its
                    // stored row is known without the assembly -- the listed rows go behind all others, in list order.  The
                    // block of the last row has seen every row: it leaves their number and the longest one's length.
                    // (The regular rows never have more than SLOTS entries: nobody else lists.)
                    if (len_t > XR_APPLY_LONG_ROW) apply_long_rows[list_base] = (int32_t)(n_stored - nl + li);
                    if (li == nl - 1) {
                        const int n_listed = list_base + (len_t > XR_APPLY_LONG_ROW ? 1 : 0);
                        listed->n_apply_long = n_listed;
                        if (n_listed > 0) listed->max_row = len_t > list_max ? len_t : list_max;
                    }
                }
                if (li == nl - 1) { // the last listed row closes the offsets
                    const long long all = capped + len_t;
                    scan_indptr[nl] = (int32_t)(all > 0x7fffffffll ? 0x7fffffff : all);
                    *scan_total = scan_indptr[nl];
                }
            }
            list_base += longer;
            list_max = longest > list_max ? longest : list_max;
        } else {
            base = row_base >= 0 ? indptr[row_base + li] : indptr[t];
        }
        __syncthreads();
        if (row_class != 0 && (row_class == 1) != (n <= ROW_BLOCK)) continue; // (uniform) the other launch's row
        // park the row: survivor id or -1 (four independent pairs of loads per thread and trip)
        for (int i0 = tid; i0 < n && i0 < BM_STAGE; i0 += 4 * 256) {
            double a[4];
            int sd[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * 256;
                const bool in = i < n && i < BM_STAGE;
                a[u] = in ? cand_area[c0 + i] : 0.0;
                sd[u] = in ? cand_sid[c0 + i] : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * 256;
                if (i < n && i < BM_STAGE) stage[i] = a[u] > 0 ? sd[u] : -1;
            }
        }
        if (n <= ROW_BLOCK) { // all-pairs rank; dead candidates compare as +inf
            __syncthreads();
            const int n4 = (n + 3) & ~3;
            if (tid < n4 - n) stage[n + tid] = -1;
            __syncthreads();
            const int4 *quad = reinterpret_cast<const int4 *>(stage);
            for (int i = tid; i < n; i += 256) {
                const int sd = stage[i];
                if (sd < 0) continue;
                int rank = 0;
                for (int j = 0; j < n4 / 4; j++) {
                    const int4 q = quad[j];
                    rank += ((unsigned)q.x < (unsigned)sd) + ((unsigned)q.y < (unsigned)sd) + ((unsigned)q.z < (unsigned)sd) +
                            ((unsigned)q.w < (unsigned)sd);
                }
                const double a = cand_area[c0 + i];
                indices[base + rank] = sd;
                data[base + rank] = relative ? a / src_area[sd] : a;
            }
            continue;
        }
        auto survivor = [&](int i) -> int { // tree face id of candidate i of the row, -1 if its area is not positive
            if (i < BM_STAGE) return stage[i];
            return cand_area[c0 + i] > 0 ? cand_sid[c0 + i] : -1;
        };
        int running = 0;
        for (int64_t cb64 = 0; cb64 < n_tree; cb64 += BM_BITS) {
            const int cb = (int)cb64;
            __syncthreads();
            {
                uint4 *bm4 = reinterpret_cast<uint4 *>(bm);
                for (int w = tid; w < BM_WORDS / 4; w += 256) bm4[w] = make_uint4(0u, 0u, 0u, 0u);
            }
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                const int s = survivor(i) - cb;
                if (s >= 0 && s < BM_BITS) atomicOr(&bm[s >> 5], 1u << (s & 31));
            }
            __syncthreads();
            // bits per group of 8 words (coalesced 32-byte reads), then an exclusive prefix over the 16 groups
            // of each thread's segment
            for (int g = tid; g < BM_WORDS / 8; g += 256) {
                const uint4 x = reinterpret_cast<const uint4 *>(bm)[2 * g], y = reinterpret_cast<const uint4 *>(bm)[2 * g + 1];
                gcnt[g] = (uint16_t)(__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w) + __popc(y.x) + __popc(y.y) +
                                     __popc(y.z) + __popc(y.w));
            }
            __syncthreads();
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < BM_SEG / 8; k++) {
                const uint32_t c = gcnt[tid * (BM_SEG / 8) + k];
                gcnt[tid * (BM_SEG / 8) + k] = (uint16_t)acc;
                acc += c;
            }
            // block exclusive scan of the per-thread totals
            const uint32_t incl = wave_incl_scan(acc);
            if (lane == 63) red[wave] = (int32_t)incl;
            __syncthreads();
            uint32_t woff = 0, chunk_total = 0;
            for (int w = 0; w < 4; w++) {
                if (w < wave) woff += (uint32_t)red[w];
                chunk_total += (uint32_t)red[w];
            }
            tbase[tid] = woff + incl - acc;
            __syncthreads();
            if (chunk_total != 0) {
                for (int i = tid; i < n; i += 256) {
                    const int sid = survivor(i);
                    const int s = sid - cb;
                    if (sid >= 0 && s >= 0 && s < BM_BITS) {
                        const int w = s >> 5;
                        int rank = running + (int)tbase[w / BM_SEG] + (int)gcnt[w >> 3] +
                                   __popc(bm[w] & ((1u << (s & 31)) - 1u));
                        for (int k = w & ~7; k < w; k++) rank += __popc(bm[k]);
                        const double a = cand_area[c0 + i];
                        indices[base + rank] = sid;
                        data[base + rank] = relative ? a / src_area[sid] : a;
                    }
                }
            }
            running += (int)chunk_total;
        }
        __syncthreads();
    }
}

// Upper bound, for every pair of faces of the two meshes, of the area the clip can return for a pair the reference's pre-clip
// tests reject (pair_passes_box_and_sat).  Such a pair's true intersection is at most ~3 ulp(coordinate) deep (the SAT's
// projections) and the clip's crossing points are off by a few ulp(coordinate) more: a sliver of width <= ~8 eps |coordinate|
// along at most half the perimeter of the smaller face.  With perimeter <= 4 extents: 16 eps M ext; the threshold is four
// times that (64 eps = 1.4e-14), M the largest coordinate magnitude, ext the smaller of the two meshes' largest face extents
// (both statistics are on the host when the clip is launched; a sampled tree statistic is bounded by the domain).  The
// smaller the threshold the fewer lanes fetch their vertices again: on the 1M benchmark 1e-12 M ext cost the clip 7 us.
double overlap_dust_threshold(const xr_mesh *tree, const xr_mesh *query) {
    double mag = 0.0, ext = INFINITY;
    for (const xr_mesh *m : {tree, query}) {
        const double *h = m->stats.h;
        mag = std::max(mag, std::max(std::max(fabs(h[stat::XMIN]), fabs(h[stat::XMAX])),
                                     std::max(fabs(h[stat::YMIN]), fabs(h[stat::YMAX]))));
        ext = std::min(ext, m->stats.sampled ? std::max(h[stat::XMAX] - h[stat::XMIN], h[stat::YMAX] - h[stat::YMIN])
                                             : h[stat::MAX_EXTENT]);
    }
    return option(OPT_DUST) == 0 ? 0.0 : 5.7e-14 * mag * ext; // (option "dust" = 0: measurement switch, no confirmation)
}

// ---- launches both pipelines share (declared in xr_overlap.h) ------------------------------------------------------------
void launch_search(const xr_mesh *tree, const xr_mesh *query, const SearchLists &l, const PairQueue &q, int32_t *n_big,
                   const MortonParams &tile, int32_t *tile_key, int32_t *blk_rows, int32_t *blk_surv) {
    const int64_t T = query->n_face;
    const dim3 grid(xcd_grid(div_up(T, 256), REMAP_SEARCH));
    auto launch = [&](auto packed) {
        with_nodes_per_face(query->m, [&](auto mc) {
            XR_LAUNCH("search", (k_search<decltype(packed)::value, mc()>), grid, dim3(256), 0, query->qo_bbox(), query->qo_fxy(),
                      query->qo_len(), T, tree->index.grid, tree->n_face, tree->index.cell_start.get(), tree->index.rec_bb.get(), l.cand_count.get(),
                      l.cand_off.get(), q.tgt, q.src, q.cursor, l.block_seg.get(), l.is_big.get(), l.big_list.get(), n_big, tile,
                      tile_key, l.nnz_row.get(), REMAP_SEARCH, blk_rows, blk_surv, blk_rows ? (int)q.capacity : 0);
        });
    };
    if (tree->n_face <= ((int64_t)1 << 24)) launch(std::true_type());
    else launch(std::false_type());
}

void launch_search_big(const xr_mesh *tree, const xr_mesh *query, const SearchLists &l, const PairQueue &q, const int32_t *n_big,
                       int32_t *n_pending, int32_t *slot_face) {
    XR_LAUNCH("search_big", k_search_big<true>, dim3(engine().num_cu * 8), dim3(256), sizeof(int32_t) * (size_t)BIG_STAGE,
              query->qo_bbox(), query->qo_fxy(), query->qo_len(), query->qo_off(), query->m, tree->index.grid, tree->index.cell_start.get(),
              tree->index.rec_bb.get(), tree->index.rec_face.get(), l.big_list.get(), n_big, l.cand_off.get(), l.cand_count.get(), q.tgt,
              q.src, q.cursor, q.capacity, l.pending.get(), n_pending, BIG_STAGE, slot_face);
}

void launch_search_big_fill(const xr_mesh *tree, const xr_mesh *query, const SearchLists &l, const PairQueue &q,
                            const int32_t *n_pending) {
    XR_LAUNCH("search_big_fill", k_search_big<false>, dim3(engine().num_cu * 8), dim3(256), sizeof(int32_t), query->qo_bbox(),
              query->qo_fxy(), query->qo_len(), query->qo_off(), query->m, tree->index.grid, tree->index.cell_start.get(), tree->index.rec_bb.get(),
              tree->index.rec_face.get(), l.pending.get(), n_pending, l.cand_off.get(), l.cand_count.get(), q.tgt, q.src,
              (int32_t *)nullptr, q.capacity, (int32_t *)nullptr, (int32_t *)nullptr, 0);
}

void launch_row_fill_long(int row_class, const xr_mesh *tree, const SearchLists &l, const double *tree_area, bool relative,
                          const LongRows &r) {
    const bool light = row_class == 1;
    // (both classes' launches walk the whole list for its offsets; ONE of them, not the bitmap rows', lists for the apply)
    auto launch = [&](auto list) {
        allow_dynamic_lds<&k_row_fill_long<list()>>(ROW_FILL_LONG_LDS);
        XR_LAUNCH(row_class == 2 ? "row_fill_huge" : "row_fill_long", k_row_fill_long<list()>, dim3(engine().num_cu * (light ? 6 : 1)),
                  dim3(256), light ? ROW_FILL_LIGHT_LDS : ROW_FILL_LONG_LDS, l.cand_off.get(), l.cand_count.get(), r.cand_sid,
                  r.cand_area, r.indptr, tree_area, relative, tree->n_face, r.indices, r.data, r.long_rows, r.n_long, r.row_base,
                  r.skip_if, r.scan_nnz, r.scan_indptr, r.scan_total, row_class, r.apply_long_rows, r.listed, r.n_stored);
    };
    if (light && r.apply_long_rows && r.scan_nnz) launch(std::true_type());
    else launch(std::false_type());
}

// Rows kept in the caller's (coherent, but typically strip-like) numbering get a coarse Morton key each: tiles of 12-24 mean
// target extents, runs of TILE_RUN consecutive rows kept together.  A Morton-sorted query order is tiled already.
// -> the key's parameters; csr->tiling.key allocated, csr->tiling.pending / key_range set
static MortonParams tile_key_params(const xr_mesh *query, xr_csr *csr) {
    MortonParams tile{};
    csr->tiling.pending = false;
    if (!query->qo.identity) return tile;
    const int64_t T = query->n_face;
    // tile edge <= 12 mean extents (the side count is a power of two): about one block of 256 triangles per tile
    tile = morton_cover(query->stats.h, T, 12.0, 0, 12);
    tile.n_run = TILE_RUN;
    csr->tiling.key.alloc((size_t)T);
    csr->tiling.key_range = (int64_t)tile.n_side * tile.n_side;
    csr->tiling.pending = tile.n_side > 1;
    return tile;
}

static void overlap(xr_mesh *tree, xr_mesh *query, bool relative, xr_csr *csr, EarlyApply *early = nullptr) {
    // (the query side on the side stream next to the tree side was measured: the prepare kernels are bandwidth bound and
    // just slow each other down, 0.684 -> 0.706 ms per step)
    // the tree side only needs its records (built from the raw mesh).  Its statistics go to the host through a one-block
    // kernel that ends with writes to pinned memory (~20 us): on the side stream as well, beside the preparation of the
    // query mesh, which is what the host waits behind anyway
    // (that was the tree's FULL statistics pass; its sampled pass is latency, a tenth of the query side's bytes, and leads the
    // query's grid in one launch: mesh_prepare_pair.  The query's statistics are first read by mesh_query_order below)
    mesh_prepare_pair(tree, query);
    host_stamp(2);
    mesh_build_index(tree);
    host_stamp(3);
    mesh_query_order(query);
    host_stamp(4);
    const double *tree_area = relative ? mesh_area(tree) : nullptr;
    const int64_t T = query->n_face, S = tree->n_face;
    XR_REQUIRE(T < ((int64_t)1 << 31) - 1, XR_ERR_LIMIT, "too many query faces for int32 row offsets");
    csr->n = T;
    csr->m = S;
    csr->nnz = 0;
    csr->indptr.alloc((size_t)T + 1);
    tree->last_candidates = 0;
    if (T == 0 || S == 0) {
        XR_HIP(hipMemsetAsync(csr->indptr.get(), 0, sizeof(int32_t) * ((size_t)T + 1), launch_stream()));
        csr->indices.alloc(0);
        csr->data.alloc(0);
        return;
    }
    const MortonParams tile = tile_key_params(query, csr);
    // dense meshes of at most 4 nodes per face: the single-round-trip pipeline of xr_overlap_fused.hip (option "overlap_fused"
    // = 0: test / measurement switch back to the general kernel chain)
    const bool fused = option(OPT_OVERLAP_FUSED) != 0 && tree->m <= DENSE_MAX_NODES && query->m <= DENSE_MAX_NODES &&
                       (T + 8 * FB) * SLOTS < ((int64_t)1 << 31);
    if (fused && overlap_tri(tree, query, tree_area, relative, csr, tile, early)) return;
    overlap_general(tree, query, tree_area, relative, csr, tile);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_overlap(xr_mesh *tree, xr_mesh *query, int relative, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(tree && query && out, XR_ERR_INVALID, "xr_overlap: NULL argument");
    Building<xr_csr> csr;
    overlap(tree, query, relative != 0, csr.get());
    stream_sync();
    *out = csr.release();
    XR_API_END
}

int xr_overlap_apply_dev(xr_mesh *tree, xr_mesh *query, int relative, int method, double percentile, const void *source_dev,
                         int source_dtype, int64_t K, double *out_dev, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(tree && query && out, XR_ERR_INVALID, "xr_overlap_apply_dev: NULL argument");
    XR_REQUIRE(K >= 0 && (source_dev || tree->n_face == 0 || K == 0) && (out_dev || query->n_face == 0 || K == 0), XR_ERR_INVALID,
               "xr_overlap_apply_dev: NULL data argument");
    XR_REQUIRE(source_dtype == XR_F64 || source_dtype == XR_F32, XR_ERR_INVALID, "unsupported source dtype id %d", source_dtype);
    host_stamp(0);
    Building<xr_csr> csr(OnFailure::WaitFirst);
    EarlyApply early;
    early.fn = [&](const xr_csr *c, const ApplyContext *ctx) { csr_apply_dev(c, method, percentile, source_dev, source_dtype, K, out_dev, ctx); };
    // one variable and a streaming reducer: the apply is one launch that needs no size on the host
    const bool can_early = K == 1 && method != XR_MODE && method != XR_PERCENTILE;
    early.takes_tail = can_early;
    overlap(tree, query, relative != 0, csr.get(), can_early ? &early : nullptr);
    host_stamp(8);
    if (!early.done && K > 0) csr_apply_dev(csr.get(), method, percentile, source_dev, source_dtype, K, out_dev);
    dev_call_done(); // (xr_set_async(1): returns with the apply in flight)
    host_stamp(9);
    *out = csr.release();
    XR_API_END
}

int xr_overlap_partial_dev(xr_mesh *tree, xr_mesh *query, int relative, int method, const void *source_dev, int source_dtype,
                           int64_t K, double *out_dev, int rows_layout, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(tree && query && out, XR_ERR_INVALID, "xr_overlap_partial_dev: NULL argument");
    XR_REQUIRE(K >= 0 && (source_dev || tree->n_face == 0 || K == 0) && (out_dev || query->n_face == 0 || K == 0), XR_ERR_INVALID,
               "xr_overlap_partial_dev: NULL data argument");
    // (checked BEFORE the weight build: inside it they would fire in the early apply's callback, half-way through the build)
    XR_REQUIRE(xr_partial_components(method) > 0, XR_ERR_INVALID, "xr_overlap_partial_dev: method %d has no partial state", method);
    XR_REQUIRE(source_dtype == XR_F32 || source_dtype == XR_F64, XR_ERR_INVALID, "xr_overlap_partial_dev: source_dtype must be XR_F32 or XR_F64");
    XR_REQUIRE(K < 65536, XR_ERR_LIMIT, "xr_overlap_partial_dev: at most 65535 variables per call");
    Building<xr_csr> csr(OnFailure::WaitFirst);
    EarlyApply early;
    early.fn = [&](const xr_csr *c, const ApplyContext *ctx) { csr_partial_dev(c, method, source_dev, source_dtype, K, out_dev, rows_layout, ctx); };
    const bool can_early = K == 1; // (one variable: the wave-window kernel needs no size on the host)
    overlap(tree, query, relative != 0, csr.get(), can_early ? &early : nullptr);
    if (!early.done && K > 0) csr_partial_dev(csr.get(), method, source_dev, source_dtype, K, out_dev, rows_layout);
    dev_call_done();
    *out = csr.release();
    XR_API_END
}

int xr_overlap_stats(const xr_mesh *tree, int64_t *n_candidates) {
    XR_API_BEGIN
    XR_REQUIRE(tree && n_candidates, XR_ERR_INVALID, "xr_overlap_stats: NULL argument");
    *n_candidates = tree->last_candidates;
    XR_API_END
}

} // extern "C"
