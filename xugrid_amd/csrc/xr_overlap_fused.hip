// xr_overlap_fused.hip -- dense meshes of at most 4 nodes per face without the host in the loop: the fused pipeline of the
// weight construction, its kernels and its host side, overlap_tri (the other two units: xr_overlap.hip, xr_overlap_general.hip;
// reference seam: CellTree2d.intersect_faces + weights /= area + MatrixCSR.from_triplet, xugrid/regrid/unstructured.py:109-135,
// xugrid/regrid/regridder.py:433-435).
//
// The general kernel chain search -> [host: C] -> clip (+ row counts by global atomics) -> scan (2 launches) -> [host: nnz]
// -> row_fill needs the host twice.  For triangle meshes:
//   k_search / k_search_big   as before, big faces into their own queue
//   k_clip_tri_queue          persistent clip over the regular pair queue; its length is read from device memory, so
//                             the launch does not wait for the host; chunks software-pipelined
//   k_assemble_scan           the search leaves the number of regular faces per block of 256 target faces, the clip the
//                             number of surviving pairs per block (one atomic per wave): ONE small block scans the few
//                             thousand (rows, entries) pairs into every block's first stored row and CSR base
//   k_assemble                the block that owns 256 consecutive target faces counts its survivors per row in LDS, ranks
//                             every survivor among its row and writes the final CSR at its base.  No row counters in
//                             HBM.  (xr_csr::stored.row_order maps stored rows to the caller's faces.)  Up to 8192 blocks every
//                             block sums the counts of the blocks in front of it itself instead of k_assemble_scan
//   big faces (hull slivers, > SLOTS hits; 0.1 % of the faces, but their block-per-face kernels are chains of dependent
//   phases: 15 % of the step when run in line) on a SIDE STREAM, forked behind k_search: k_search_big -> k_clip_tri_queue on
//   their own pair queue -> k_row_fill_long (rows in face order as ranked by k_search_big; scans their lengths itself) into a small
//   CSR of their own; joined behind k_assemble, k_place_big copies those rows BEHIND the regular ones.
//   [host: sizes + error bits: ONE round trip for the whole weight matrix]
// Measured and discarded on the way (MI355X, benchmark pair): a fully fused search + clip + assembly block (pairs never
// leave LDS): correct, but the grid walk is a chain of dependent loads that needs ~7 waves per SIMD, the LDS staging
// allows 2 -- 0.68 ms against 0.31 ms for separate kernels; clip + assembly in one kernel: the clip is FP64-issue bound
// and needs 5 waves per SIMD, the staging leaves 3 -- 0.33 ms against 0.25 ms (and with the look-back inside, 1 ... 16
// clip rounds per block make every generation of resident blocks last as long as its slowest member); rows of the
// assembly placed by ONE returning 64-bit atomic per block instead of the look-back: 4000 atomics on one address cost
// 30 us (and a "last block done" counter another 27 us).
#include "xr_overlap.h"
#include "xr_clip.h"

namespace xr {

// (FusedCounters, the control block's words -- CtlWord --, the verdict on an attempt and the gate of an apply enqueued behind the
// build: xr_overlap_tail.h, shared with the apply that takes the tail of the build into its own launch; FB, SLOTS: xr_overlap.h)
// Mailbox record k_publish_all leaves for the host (pinned memory, engine().mailbox), indexed by MailSlot.
enum MailSlot : int {
    MAIL_REG_PAIRS = 0,      // = CTL_REG_CURSOR ... the first five control words as they are
    MAIL_BIG_PAIRS = 1,
    MAIL_N_BIG = 2,
    MAIL_N_PENDING = 3,
    MAIL_BIG_OVERFLOW = 4,   // (reserved, like its control word)
    MAIL_ERROR = 5,          // the FusedCounters fields in the order the host reads them
    MAIL_ROWS_REGULAR = 6,
    MAIL_N_APPLY_LONG = 7,
    MAIL_P_REGULAR = 8,
    MAIL_P_BIG = 9,
    MAIL_MAX_ROW = 10,
    MAIL_REGION_LEN = 11,    // [8] the regions' own lengths (read by the `debug` option's line only)
    MAIL_FUSED_SLOTS = MAIL_REGION_LEN + 8
};
static_assert(MAIL_BIG_OVERFLOW - MAIL_REG_PAIRS == CTL_BIG_OVERFLOW - CTL_REG_CURSOR && MAIL_FUSED_SLOTS <= MAIL_SEQ_SLOT,
              "the first control words map to the first mailbox slots one to one");

// Persistent triangle x triangle clip over the regular pair queue: the number of pairs is read from device memory
// (the search's queue cursor), so the launch needs no host round trip; every block walks chunks of 256 pairs.  Chunks are dealt so that every XCD works on one contiguous eighth of the queue (the order
// k_search wrote it in: the vertex blocks are in that XCD's L2).
// COUNT: which survivor counts the kernel keeps (two instantiations: both paths in one kernel cost registers -> scratch)
//   0 none, 1 per block of FB target faces (regular queue: blk_surv), 2 per target face (big faces' queue: nnz_row)
//   (the LDS columns are lane-major, 7 consecutive slots per lane; slot-major columns were measured in round 3 and lost)
// KIND 1 (round 5): dense meshes of up to 4 nodes per face on either side (quadrilaterals, mixed triangle / quadrilateral
// meshes with fill values -- the usual D-Flow FM mesh, a raster paired with a triangle mesh): the register / LDS clip of
// k_clip_small<8> (the oracle's arithmetic in the oracle's order) inside the same persistent loop, so that these pairs take
// the one-round-trip pipeline too.  q_len / s_len / q_m / s_m are only read then.
// (waves per SIMD: the persistent grid is sized for five resident blocks per CU -- four for KIND 1 -- and a single register beyond
// 96 would leave only four: the block that does not fit runs BEHIND the others, +40 % on the kernel -- measured when one crept in)
template <int BLOCK, int COUNT, int KIND = 0>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(KIND == 0 ? 5 : 4)))
k_clip_tri_queue(const double *__restrict__ q_fxy, const double *__restrict__ rec_fxy,
                 const int32_t *__restrict__ rec_face, const int32_t *cand_tgt,
                 const int32_t *cand_src, const int32_t *__restrict__ n_cand_dev, int64_t capacity,
                 double *__restrict__ cand_area, int32_t *__restrict__ cand_sid, int32_t *__restrict__ error_bits,
                 int32_t *__restrict__ nnz_row /* optional: survivors per target face, counted by atomics */,
                 const int32_t *__restrict__ skip_if /* optional: nothing is done when this device word is > 0 */,
                 int32_t *__restrict__ blk_surv = nullptr /* optional: survivors per BLOCK of 256 target faces (k_assemble_scan) */,
                 double dust = 0.0 /* areas up to this are confirmed by the reference's pre-clip tests (xr_clip.h: confirm_dust) */,
                 const uint8_t *__restrict__ q_len = nullptr, const uint8_t *__restrict__ s_len = nullptr, int q_m = 3, int s_m = 3) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CS = 1; // (stride between a lane's slots)
    constexpr int SMALL_MAXV = 8;
    double2 *col = reinterpret_cast<double2 *>(smem) + (KIND == 1 ? threadIdx.x : threadIdx.x * (TRI_MAXV + 1)); // the lane's slots
    __shared__ uint2 sh_lut[KIND == 1 ? 1 : TRI_LUT];
    if (skip_if) __builtin_amdgcn_s_setprio(3); // (the big faces' queue, on the side stream: issue priority over the main clip)
    if (skip_if && *skip_if > 0) return; // (big faces that did not fit their queue: the host redoes everything)
    if (KIND == 0) {
        tri_lut_init(sh_lut);
        __syncthreads();
    }
    // capacity > 0: ONE dense queue of *n_cand_dev pairs, its chunks dealt so that every XCD works on a contiguous eighth;
    // capacity < 0: EIGHT dense regions of -capacity pairs each (region x filled by the search blocks of XCD x, n_cand_dev[x] pairs):
    // slot j is chunk j / 8 of region j mod 8 -- the same dealing, the regions' own lengths
    const bool regions = capacity < 0;
    const int64_t region_cap = regions ? -capacity : 0;
    int64_t n_cand = 0, per_xcd;
    auto region_len = [&](int x) -> int64_t { // (uniform: a scalar load; a region that overflowed is redone by the host)
        const int64_t n = n_cand_dev[x * QCUR_STRIDE];
        return n < region_cap ? n : region_cap;
    };
    if (regions) {
        int64_t longest = 0;
#pragma unroll
        for (int x = 0; x < 8; x++) longest = region_len(x) > longest ? region_len(x) : longest;
        per_xcd = (longest + BLOCK - 1) / BLOCK;
    } else {
        n_cand = *n_cand_dev < capacity ? *n_cand_dev : capacity; // (a queue that overflowed is redone by the host)
        per_xcd = ((n_cand + BLOCK - 1) / BLOCK + 7) >> 3;
    }
    const int64_t n_slots = per_xcd * 8; // chunk slots incl. the empty ones of the shorter eighths
    // j-th slot -> index of its first pair; *end = one behind the last pair the slot's stretch may hold
    auto slot_first = [&](int64_t j, int64_t *end) -> int64_t {
        if (regions) {
            const int x = (int)(j & 7);
            *end = (int64_t)x * region_cap + region_len(x);
            return (int64_t)x * region_cap + (j >> 3) * BLOCK;
        }
        *end = n_cand;
        return ((j & 7) * per_xcd + (j >> 3)) * BLOCK;
    };
    const double2 *tfx = reinterpret_cast<const double2 *>(q_fxy);
    const double2 *sfx = reinterpret_cast<const double2 *>(rec_fxy);
    const int tid = threadIdx.x;
    // the pair indices of the NEXT chunk are fetched while a chunk is clipped (its vertex gathers then start at once;
    // prefetching the vertex blocks as well costs 36 more registers = a wave per SIMD, and the clip is issue bound)
    int n_tq = 0, n_s = 0;
    auto load_idx = [&](int64_t slot, int &tq, int &s) {
        tq = 0;
        s = 0;
        if (slot < n_slots) {
            int64_t end;
            const int64_t c = slot_first(slot, &end) + tid;
            if (c < end) {
                tq = cand_tgt[c];
                s = cand_src[c];
            }
        }
    };
    const int64_t stride = gridDim.x;
    int64_t slot = blockIdx.x;
    load_idx(slot, n_tq, n_s);
    bool overflow = false;
    for (; slot < n_slots; slot += stride) {
        int64_t c_end;
        const int64_t c = slot_first(slot, &c_end) + tid;
        const bool active = c < c_end;
        int sid = 0;
        const int cur_tq = n_tq;
        double area = 0.0;
        if (KIND == 1) {
            const int cur_s = n_s;
            int nt = 0, ns = 0;
            if (active) {
                sid = rec_face[cur_s];
                nt = q_len[cur_tq];
                ns = s_len[cur_s];
            }
            load_idx(slot + stride, n_tq, n_s);
            const double2 *tf = tfx + (int64_t)cur_tq * q_m;
            const double2 *sf = sfx + (int64_t)cur_s * s_m;
            if (active) area = clip_small_pair<SMALL_MAXV, BLOCK>(tf, nt, reinterpret_cast<const double *>(sf), ns, col);
            area = confirm_dust(area, dust, active, tf, nt, sf, ns);
        } else {
            P2 tv[3] = {{0, 0}, {0, 0}, {0, 0}}, sv[3] = {{0, 0}, {0, 0}, {0, 0}};
            if (active) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const double2 a = tfx[(int64_t)n_tq * 3 + j], b2 = sfx[(int64_t)n_s * 3 + j];
                    tv[j] = P2{a.x, a.y};
                    sv[j] = P2{b2.x, b2.y};
                }
                sid = rec_face[n_s];
            }
            load_idx(slot + stride, n_tq, n_s);
            // (rounding dust of a pair the reference's pre-clip tests reject: the few lanes concerned fetch their vertices again --
            // confirm_dust spelled out, because the source id is read again too: holding it costs a register)
            area = tri_clip_area<CS>(tv, sv, col, sh_lut, active);
            const bool suspicious = active && area > 0 && area <= dust;
            if (__any(suspicious)) {
                if (suspicious && !pair_passes_box_and_sat(tfx + (int64_t)cur_tq * 3, 3, sfx + (int64_t)cand_src[c] * 3, 3)) area = 0.0;
            }
        }
        const int tq_now = active ? cur_tq : -1;
        if (active) {
            overflow = overflow || area == TRI_AREA_OVERFLOW;
            cand_area[c] = area;
            cand_sid[c] = area > 0 ? sid : 0x7fffffff;
        }
        if (COUNT == 1) {
            // survivors per block of FB target faces.  The pairs of a block are one stretch of the queue (1700 on average):
            // most waves see a single block -- one atomic by lane 0; the others add per run of equal block ids
            const int lane = tid & 63;
            const int blk_now = active ? (cur_tq >> 8) : -1;
            const unsigned long long surv = __ballot(active && area > 0);
            const int blk_first = __builtin_amdgcn_readfirstlane(blk_now), blk_last = __shfl(blk_now, 63, 64);
            if (blk_first == blk_last) { // (uniform)
                if (lane == 0 && blk_first >= 0 && surv) atomicAdd(&blk_surv[blk_first], __popcll(surv));
            } else {
                wave_run_add(blk_now, active && area > 0, blk_surv);
            }
        }
        // pairs of one target face are contiguous: the head lane of each run of equal faces adds the run's survivors
        if (COUNT == 2) wave_run_add(tq_now, active && area > 0, nnz_row);
    }
    if (overflow) atomicOr(error_bits, 1);
}

// CSR assembly for the regular faces: the block that owns 256 consecutive target faces stages the source ids of its
// (k_assemble_scan: the blocks' first stored row and CSR base from counts the search and the clip left per block -- one
// block scans the few thousand (rows, entries) pairs in the order the assembly assigns stored rows, i.e. hardware block
// order; replaces the look-back chain inside k_assemble when those counts exist)
__global__ void __launch_bounds__(1024)
k_assemble_scan(const int32_t *__restrict__ blk_rows, const int32_t *__restrict__ blk_surv, int64_t n_blocks, int n_chain,
                bool remap, int32_t *__restrict__ base_rows, int32_t *__restrict__ base_nnz, FusedCounters *counters,
                int32_t *__restrict__ indptr) {
    __shared__ long long sh_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0; // (rows, entries) of the chunks in front, in every thread
    const int64_t per_xcd = (n_blocks + 7) >> 3;
    for (int b0 = 0; b0 < n_chain; b0 += 1024) {
        const int b = b0 + tid;
        long long v = 0;
        if (b < n_chain) {
            const int64_t lb = remap ? (int64_t)(b & 7) * per_xcd + (b >> 3) : b;
            if (lb < n_blocks) v = ((long long)blk_rows[lb] << 31) | (long long)blk_surv[lb];
        }
        // (the block level stays spelled out: block_excl_scan<1024, long long> unrolls its sixteen 64-bit reads and takes the
        // kernel from 56 to 72 registers, over the 64-register occupancy step)
        const long long incl = wave_incl_scan(v);
        if (lane == 63) sh_w[wave] = incl;
        __syncthreads();
        long long woff = 0, tot = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) woff += sh_w[w];
            tot += sh_w[w];
        }
        const long long excl = carry + woff + incl - v;
        if (b < n_chain) {
            base_nnz[b] = (int32_t)(excl & 0x7fffffffll);
            base_rows[b] = (int32_t)(excl >> 31);
        }
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        const long long entries = carry & 0x7fffffffll, rows = carry >> 31;
        counters->p_regular = (int32_t)entries; // entries of all regular rows
        counters->rows_regular = (int32_t)rows;
        indptr[rows] = (int32_t)entries;        // (= indptr[T] when there are no big faces)
    }
}

// stretch of the pair queue in LDS ("dead" for area <= 0), counts the survivors per face (LDS atomics), reserves its
// rows and entries with ONE atomic, ranks every survivor among its row and writes it to its final CSR position.
__global__ void __launch_bounds__(FB, 2)
k_assemble(const double *__restrict__ q_bbox, const double *__restrict__ q_fxy, const uint8_t *__restrict__ q_len, int q_m,
           const int32_t *__restrict__ q_perm, int64_t n_query,
           const int32_t *__restrict__ cand_tgt, const int32_t *__restrict__ cand_off,
           const int32_t *__restrict__ cand_count, const int2 *__restrict__ block_seg,
           const uint8_t *__restrict__ is_big, const double *__restrict__ cand_area,
           const int32_t *__restrict__ cand_sid, const double *__restrict__ src_area, bool relative, MortonParams tile,
           int32_t *__restrict__ tile_key, FusedCounters *__restrict__ counters,
           int32_t *__restrict__ indptr, int32_t *__restrict__ indices, double *__restrict__ data, int32_t *__restrict__ row_order,
           int64_t csr_capacity, bool remap,
           const int32_t *__restrict__ base_rows = nullptr, const int32_t *__restrict__ base_nnz = nullptr,
           const int32_t *__restrict__ blk_rows = nullptr, const int32_t *__restrict__ blk_surv = nullptr) {
    __shared__ int32_t sh_stage[SLOTS * FB];
    __shared__ int32_t sh_nnz[FB];     // survivors of the face (LDS atomics)
    __shared__ uint16_t sh_lo[FB];     // offset of the face's pairs inside the stretch
    __shared__ uint16_t sh_rowoff[FB]; // CSR offset of the face's row inside the block
    __shared__ uint8_t sh_cnt[FB];     // pairs of the face (0 for big faces)
    __shared__ int32_t sh_wave[FWAVES];
    __shared__ long long sh_base;
    const int tid = threadIdx.x;
    const int64_t n_blocks = (n_query + FB - 1) / FB;
    const int64_t lb = xcd_block(n_blocks, remap); // (blocks beyond n_blocks carry no faces but stay in the chain)
    const bool valid_block = lb < n_blocks;
    sh_nnz[tid] = 0;
    const int64_t t0 = lb * FB;
    const int64_t t = t0 + tid;
    const bool in_range = valid_block && t < n_query;
    const int2 seg = valid_block ? block_seg[lb] : make_int2(0, 0);
    const int total = seg.y;
    bool regular = false;
    int my_cnt = 0;
    if (in_range) {
        regular = !is_big[t];
        my_cnt = regular ? cand_count[t] : 0;
        sh_lo[tid] = (uint16_t)(regular ? cand_off[t] - seg.x : 0);
    } else {
        sh_lo[tid] = 0;
    }
    sh_cnt[tid] = (uint8_t)my_cnt;
    __syncthreads();
    // (the kernel is latency bound -- 84 % of its wave cycles wait, PMC -- so both entry loops keep the loads of four
    // steps in flight instead of one)
    for (int i0 = tid; i0 < total; i0 += 4 * FB) {
        int s[4], row[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * FB;
            const int64_t c = (int64_t)seg.x + (i < total ? i : total - 1);
            s[u] = cand_sid[c];
            row[u] = cand_tgt[c] - (int)t0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * FB;
            if (i < total) {
                sh_stage[i] = s[u];
                if (s[u] != 0x7fffffff) atomicAdd(&sh_nnz[row[u]], 1);
            }
        }
    }
    __syncthreads();
    const int my_nnz = regular ? sh_nnz[tid] : 0;
    int block_nnz = 0, block_rows = 0;
    const int rowoff = block_excl_scan<FB>(my_nnz, &block_nnz, sh_wave);
    const int rowidx = block_excl_scan<FB>(regular ? 1 : 0, &block_rows, sh_wave);
    sh_rowoff[tid] = (uint16_t)rowoff;
    const int b = (int)blockIdx.x, n_chain = (int)gridDim.x;
    if (blk_surv) {
        // The search left the regular faces, the clip the surviving pairs of every block of FB target faces: this block
        // sums the (rows, entries) of the blocks in front of it itself -- in the order the assembly assigns stored rows,
        // i.e. hardware block order.  A few thousand pairs of words that all blocks read from L2 (b / 256 loads per thread,
        // issued together, while the block's own entry loads are in flight): no scan kernel, no launch in between.
        const int64_t per_xcd = (n_blocks + 7) >> 3;
        long long acc = 0;
        for (int hb = tid; hb < b; hb += FB) {
            const int64_t plb = remap ? (int64_t)(hb & 7) * per_xcd + (hb >> 3) : hb;
            if (plb < n_blocks) acc += ((long long)blk_rows[plb] << 31) | (long long)blk_surv[plb];
        }
        acc = wave_reduce<OpSum>(acc);
        __shared__ long long sh_part[FWAVES];
        if ((tid & 63) == 0) sh_part[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            long long tot = 0;
#pragma unroll
            for (int w = 0; w < FWAVES; w++) tot += sh_part[w];
            sh_base = tot;
        }
    } else { // scanned beforehand (k_assemble_scan)
        if (tid == 0) sh_base = ((long long)base_rows[b] << 31) | (long long)base_nnz[b];
    }
    __syncthreads();
    const long long base = sh_base & 0x7fffffffll, row_base = sh_base >> 31;
    if (!base_nnz && b == n_chain - 1 && tid == 0) { // (own prefix: the last block of the chain knows the totals)
        const long long entries = base + block_nnz, rows = row_base + block_rows;
        counters->p_regular = (int32_t)entries; // entries of all regular rows
        counters->rows_regular = (int32_t)rows;
        indptr[rows] = (int32_t)entries;        // (= indptr[T] when there are no big faces)
    }
    if (regular) {
        const long long r = row_base + rowidx; // stored row of the face
        indptr[r] = (int32_t)(base + rowoff);
        row_order[r] = q_perm ? q_perm[t] : (int32_t)t;
        if (tile_key) {
            const int64_t mid = (t & ~(int64_t)(tile.n_run - 1)) + tile.n_run / 2;
            tile_key[r] = morton_key(tile, query_face_box_rt(q_bbox, q_fxy, q_len, q_m, mid < n_query ? mid : n_query - 1));
        }
    }
    bool overflow_cap = false;
    for (int i0 = tid; i0 < total; i0 += 4 * FB) {
        double area[4];
        int row[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * FB;
            const int64_t c = (int64_t)seg.x + (i < total ? i : total - 1);
            area[u] = cand_area[c];
            row[u] = cand_tgt[c] - (int)t0; // (read again -- an L2 hit -- rather than kept in LDS)
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * FB;
            if (i >= total) continue;
            const int s = sh_stage[i];
            if (s == 0x7fffffff) continue;
            const int a0 = sh_lo[row[u]], a1 = a0 + sh_cnt[row[u]];
            int rank = 0;
            for (int j = a0; j < a1; j++) rank += sh_stage[j] < s ? 1 : 0;
            const long long pos = base + sh_rowoff[row[u]] + rank;
            if (pos < csr_capacity) {
                indices[pos] = s;
                data[pos] = relative ? area[u] / src_area[s] : area[u];
            } else {
                overflow_cap = true;
            }
        }
    }
    if (overflow_cap) atomicOr(&counters->error, 4);
}

// ---- the big faces' rows (side stream) -------------------------------------------------------------------------------
// Their order (by face id) is established inside k_search_big (slot_face), their offsets inside k_row_fill_long (scan_nnz
// mode): the chain search_big -> clip -> row_fill_long is the critical path of the weight build, every launch less counts.

// The finished rows of the big faces go BEHIND the regular ones (place_big_rows, xr_overlap_tail.h): as a launch of its own
// wherever no K = 1 apply is enqueued behind the build -- that apply's launch takes these blocks in front of its own.
__global__ void __launch_bounds__(256) k_place_big(PlaceBig p) { place_big_rows<false>(p, (int)blockIdx.x, (int)gridDim.x); }

// sizes, error bits and the long-row count -> host mailbox / device word of the matrix (after everything else)
// ... and clears all of them behind itself: the counter words are the engine's zero-at-rest scratch (the next xr_overlap
// starts without a memset).  One wave.
__global__ void k_publish_all(int32_t *c /* the control block (CtlWord) */, FusedCounters *fc,
                              int32_t *__restrict__ n_apply_long_out, int32_t *mail /* MailSlot */, int32_t seq, int64_t cap,
                              int64_t big_capacity) {
    // one load per lane (the CTL_LINE words are one line), so the host's wait is one round trip long
    const int t = threadIdx.x;
    int32_t w = 0;
    if (t < CTL_LINE) w = c[t];
    // (the cursors of the eight regions of the regular pair queue, a line each, read by the eight lanes behind: their sum is the
    // number of regular pairs, which takes the place of the single cursor CTL_REG_CURSOR)
    const bool region_lane = t >= CTL_LINE && t < CTL_LINE + 8;
    const int32_t cur = region_lane ? c[CTL_REGION_CURSOR + (t - CTL_LINE) * QCUR_STRIDE] : 0;
    const int32_t c_reg_sum = wave_reduce<OpSum>(cur);
    if (t == CTL_REG_CURSOR) w = c_reg_sum;
    int slot = -1; // mailbox slot of control word t
    if (t <= CTL_BIG_OVERFLOW) slot = MAIL_REG_PAIRS + t;
    else if (t == XR_CTL_COUNTER(error)) slot = MAIL_ERROR;
    else if (t == XR_CTL_COUNTER(rows_regular)) slot = MAIL_ROWS_REGULAR;
    else if (t == XR_CTL_COUNTER(n_apply_long)) slot = MAIL_N_APPLY_LONG;
    else if (t == XR_CTL_COUNTER(p_regular)) slot = MAIL_P_REGULAR;
    else if (t == XR_CTL_COUNTER(p_big)) slot = MAIL_P_BIG;
    else if (t == XR_CTL_COUNTER(max_row)) slot = MAIL_MAX_ROW;
    if (slot >= 0) mail[slot] = w;
    if (region_lane) mail[MAIL_REGION_LEN + (t - CTL_LINE)] = cur;
    if (t == XR_CTL_COUNTER(n_apply_long)) n_apply_long_out[TAIL_N_LONG] = w;
    if (t == CTL_N_BIG) n_apply_long_out[TAIL_N_BIG] = w; // (for an apply that takes the place of k_place_big behind this kernel)
    if (t == XR_CTL_COUNTER(p_regular)) n_apply_long_out[TAIL_P_REGULAR] = w;
    if (t == 0) {
        // gate of an apply enqueued right behind this kernel: open only if THIS attempt produced the final matrix -- the
        // verdict the host reaches from the mailbox with the same function (fused_outcome, xr_overlap_tail.h)
        const FusedOutcome verdict = fused_outcome(c_reg_sum, c[CTL_BIG_CURSOR], c[CTL_N_PENDING], c[XR_CTL_COUNTER(error)],
                                                   c[XR_CTL_COUNTER(p_regular)], c[XR_CTL_COUNTER(p_big)], cap, big_capacity);
        n_apply_long_out[TAIL_GATE] = verdict == FUSED_FINAL ? 1 : 0;
    }
    __builtin_amdgcn_s_waitcnt(0); // (every load above has returned before the words are cleared)
    if (t < CTL_LINE) c[t] = 0;
    if (region_lane) c[CTL_REGION_CURSOR + (t - CTL_LINE) * QCUR_STRIDE] = 0;
    (void)fc;
    // the host polls the sequence word (mailbox_wait_seq): it goes out BEHIND the words above (one wave: a system-scope
    // release covers the stores of all its lanes)
    __threadfence_system();
    if (t == 0) __hip_atomic_store(&mail[MAIL_SEQ_SLOT], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

static bool debug_fused() { return (option(OPT_DEBUG) & 1) != 0; }

// ---- the host side ------------------------------------------------------------------------------------------------------
// overlap_tri() enqueues one ATTEMPT at the matrix -- sized for per_face entries per target face and big_capacity pairs of
// the big faces -- reads the mailbox once, and decides with fused_outcome (xr_overlap_tail.h), the function k_publish_all
// set the gate with.  The stages of an attempt are the functions below, in the order the loop of overlap_tri calls them.

// What one build is given, the sizes that follow from it, and the buffers that survive its attempts.
struct FusedBuild {
    xr_mesh *const tree, *const query;
    const double *const tree_area;
    const bool relative;
    xr_csr *const csr;
    const MortonParams &tile;
    int32_t *const tile_key;
    const int64_t T = query->n_face, n_blocks = div_up(T, FB);
    const bool remap = REMAP_SEARCH;
    const unsigned grid = xcd_grid(n_blocks, remap);
    // the regular pair queue: eight regions (one per XCD) of region_cap pairs each -- every block of 256 faces parks at most
    // 256 x SLOTS pairs and an XCD takes ceil(n_blocks / 8) blocks
    const int64_t region_cap = div_up(div_up(T, FB), 8) * FB * SLOTS;
    const int64_t reg_capacity = 8 * region_cap;
    // Row bases of the assembly: every assembly block sums the counts of the blocks in front of it itself (scan_mode 2) -- it reads
    // b words in block b, O(blocks^2) L2 reads in total: fine for a few thousand blocks (1M faces: 62 MB), 6 GB for the 39k blocks
    // of a 10M-face target (measured: 10M -> 10M 4.39 -> 4.89 ms) -- so from 8192 blocks on a one-block scan kernel between clip and
    // assembly provides them (scan_mode 1, as until round 3).  (Until round 5 a decoupled look-back inside k_assemble was a third
    // form, behind a switch; it lost in round 3 and is gone.)
    const int scan_mode = grid <= 8192 ? 2 : 1;
    // (launch_clip_queue) KIND 0, triangle x triangle; KIND 1, any other pair of dense meshes
    const bool tri_pair = tree->m == 3 && query->m == 3;
    const double dust = overlap_dust_threshold(tree, query);
    // Behind the control words (CtlWord, xr_overlap_tail.h), per block of 256 target faces: survivors (clip), regular faces
    // (search) -- k_search clears its block's survivor count: no memset in front of the search.
    DevBuf<int32_t> ctl_tail{2 * (size_t)grid}, ctl_own; // (ctl_own: the control words, where the engine's scratch is taken)
    int32_t *const blk_surv = ctl_tail.get(), *const blk_rows = blk_surv + grid;
    DevBuf<int32_t> blk_base{2 * (size_t)grid}; // first stored row / CSR base of every hardware block (k_assemble_scan)
    SearchLists l{T};
    DevBuf<int32_t> slot_face{(size_t)T}, big_indptr{(size_t)T + 1};
    // (measured and removed: the clip writing only its survivors, compacted in place over the queue -- the HBM bytes drop, but the
    // assembly becomes three passes of dependent loads, 0.066 -> 0.087 ms, DESIGN_HISTORY.md round 3)
    DevBuf<int32_t> cand_tgt{(size_t)reg_capacity}, cand_src{(size_t)reg_capacity}, cand_sid{(size_t)reg_capacity};
    DevBuf<double> cand_area{(size_t)reg_capacity};
};

// What one attempt allocates for its capacities, and the control block it runs on.
struct FusedAttempt {
    int64_t cap = 0, big_capacity = 0; // entries the CSR / pairs the big faces' queue have room for
    DevBuf<int32_t> big_tgt, big_src, big_sid, big_indices;
    DevBuf<double> big_area, big_data;
    // The control words (CtlWord) come from the engine's zero-at-rest scratch (k_publish_all clears them again after copying
    // them to the mailbox)
    int32_t *ctl = nullptr;
    bool ctl_cached = false;
    FusedCounters *fc = nullptr;
    int32_t *n_big_dev = nullptr, *n_pending_dev = nullptr;
    PairQueue reg_queue{}, big_queue{};
};

// what k_publish_all left in the mailbox (MailSlot)
struct FusedMail {
    int32_t c_reg, c_big, n_big, n_pending, err, rows_regular, n_apply_long, p_regular, p_big, max_row;
};

// k_clip_tri_queue, persistent, over a pair queue.  KIND 0, triangle x triangle: the flag / compaction clip of xr_clip_tri.h;
// KIND 1, any other pair of dense meshes (<= 4 nodes per face: quadrilaterals, mixed meshes with fill values, a raster
// against triangles): the register / LDS clip of k_clip_small<8>, which also reads the faces' lengths.
// COUNT 2: the big faces' queue, survivors per face; COUNT 1: the regular queue's eight regions, survivors per block.
template <int COUNT>
static void launch_clip_queue(const FusedBuild &b, const char *name, int blocks_per_cu, const PairQueue &q, double *area,
                              int32_t *sid, int32_t *error, int32_t *nnz_row, const int32_t *skip_if, int32_t *blk_surv) {
    constexpr int BLOCK = 256;
    const int64_t capacity = COUNT == 1 ? -q.capacity : q.capacity; // (< 0: eight regions of that many pairs)
    auto launch = [&](auto kind, size_t maxv, const uint8_t *q_len, const uint8_t *s_len) {
        XR_LAUNCH(name, (k_clip_tri_queue<BLOCK, COUNT, kind()>), dim3(engine().num_cu * blocks_per_cu), dim3(BLOCK),
                  (maxv + 1) * BLOCK * sizeof(double2), b.query->qo_fxy(), b.tree->index.rec_fxy.get(), b.tree->index.rec_face.get(), q.tgt, q.src,
                  q.cursor, capacity, area, sid, error, nnz_row, skip_if, blk_surv, b.dust, q_len, s_len, b.query->m, b.tree->m);
    };
    if (b.tri_pair) launch(std::integral_constant<int, 0>(), TRI_MAXV, nullptr, nullptr);
    else launch(std::integral_constant<int, 1>(), 8, b.query->qo_len(), b.tree->index.rec_len.get());
}

// (1) the matrix and the big faces' buffers sized for this attempt's capacities; a control block that is zero
static void attempt_allocate(FusedBuild &b, FusedAttempt &a, int64_t per_face, int64_t big_capacity) {
    a.big_capacity = big_capacity;
    a.cap = per_face * b.T + big_capacity;
    XR_REQUIRE(a.cap < ((int64_t)1 << 31), XR_ERR_LIMIT, "nnz exceeds the int32 range");
    b.csr->indices.alloc((size_t)a.cap);
    b.csr->data.alloc((size_t)a.cap);
    b.csr->longs.rows.alloc((size_t)(a.cap / XR_APPLY_LONG_ROW + 1));
    for (DevBuf<int32_t> *buf : {&a.big_tgt, &a.big_src, &a.big_sid, &a.big_indices}) buf->alloc((size_t)big_capacity);
    a.big_area.alloc((size_t)big_capacity);
    a.big_data.alloc((size_t)big_capacity);
    a.ctl = zero_scratch(1, CTL_WORDS);
    a.ctl_cached = a.ctl != nullptr;
    if (!a.ctl_cached) {
        b.ctl_own.alloc(CTL_WORDS);
        a.ctl = b.ctl_own.get();
        XR_HIP(hipMemsetAsync(a.ctl, 0, CTL_WORDS * sizeof(int32_t), launch_stream()));
    }
    a.fc = reinterpret_cast<FusedCounters *>(a.ctl + CTL_COUNTERS);
    a.n_big_dev = a.ctl + CTL_N_BIG;
    a.n_pending_dev = a.ctl + CTL_N_PENDING;
    a.reg_queue = PairQueue{b.cand_tgt.get(), b.cand_src.get(), a.ctl + CTL_REGION_CURSOR, b.region_cap};
    a.big_queue = PairQueue{a.big_tgt.get(), a.big_src.get(), a.ctl + CTL_BIG_CURSOR, big_capacity};
}

// (2) the search: regular faces into the eight regions of the regular queue, big faces listed
static void enqueue_search(const FusedBuild &b, const FusedAttempt &a) {
    launch_search(b.tree, b.query, b.l, a.reg_queue, a.n_big_dev, b.tile, nullptr, b.blk_rows, b.blk_surv);
}

// (3) side streams: everything about the big faces except their final placement
static void enqueue_big_chain(const FusedBuild &b, const FusedAttempt &a) {
    SideScope side;
    launch_search_big(b.tree, b.query, b.l, a.big_queue, a.n_big_dev, a.n_pending_dev, b.slot_face.get());
    // (pairs of a face that did not fit are missing: the error is seen at the end and everything is redone)
    launch_clip_queue<2>(b, "clip_big", 1, a.big_queue, a.big_area.get(), a.big_sid.get(), &a.fc->error, b.l.nnz_row.get(),
                         a.n_pending_dev, nullptr);
    // (rows in face order: ranked inside search_big; their offsets: scanned inside row_fill_long -- two launches less
    // in what is the critical path of the whole weight build)
    // Two launches: the rows of at most ROW_BLOCK candidates (all but a handful) with 16 KB of LDS per block -- a block
    // per row, resident beside the clip and the assembly -- and the few longer ones with the bitmap (150 KB, a CU per
    // block).  As ONE launch every block needed a whole CU: it could not start before the clip's blocks had left and
    // then walked ~5 rows in turn -- 54-64 us, ending after the assembly (round-4 timeline).
    // (round 6: the two launches are independent -- each scans the row lengths itself and fills only its own class of
    // rows -- so the bitmap rows go to a SECOND side stream and run beside the light ones: the big faces' chain
    // behind the clip is one launch shorter where it is the step's critical path, 0.506 -> 0.500 ms in an A/B)
    const LongRows big_rows{a.big_sid.get(), a.big_area.get(), b.big_indptr.get(), a.big_indices.get(), a.big_data.get(),
                            b.slot_face.get(), a.n_big_dev, 0, a.n_pending_dev, b.l.nnz_row.get(), b.big_indptr.get(), &a.fc->p_big,
                            b.csr->longs.rows.get(), a.fc, b.T};
    SideForkScope fork;
    launch_row_fill_long(2, b.tree, b.l, b.tree_area, b.relative, big_rows);
    fork.end_launches();
    launch_row_fill_long(1, b.tree, b.l, b.tree_area, b.relative, big_rows);
}

// (4) main stream: the persistent clip over the regular queue, then the assembly of the regular rows
static void enqueue_regular(const FusedBuild &b, const FusedAttempt &a) {
    // Persistent blocks per CU: five fill the LDS and the register files (best for the clip alone).  The big faces' chain
    // on the side stream then gets few wave slots while the clip runs; with its kernels at raised wave priority and only
    // three launches long (search_big -> clip -> row_fill_long) it still ends about when k_assemble does: 3, 4 and 5
    // blocks per CU all give the same step (0.635 ms) -- measured after the chain lost two launches; before, 3 was
    // 4 % faster because the chain was the critical path.
    // (KIND 1: k_clip_small's LDS columns are 36 KB per block, four persistent blocks per CU)
    launch_clip_queue<1>(b, b.tri_pair ? "clip_tri" : "clip_small", b.tri_pair ? 5 : 4, a.reg_queue, b.cand_area.get(),
                         b.cand_sid.get(), &a.fc->error, nullptr, nullptr, b.blk_surv);
    const xr_mesh *query = b.query;
    xr_csr *csr = b.csr;
    const unsigned grid = b.grid;
    if (b.scan_mode == 1)
        XR_LAUNCH("assemble_scan", k_assemble_scan, dim3(1), dim3(1024), 0, b.blk_rows, b.blk_surv, (int64_t)b.n_blocks, (int)grid,
                  b.remap, b.blk_base.get(), b.blk_base.get() + grid, a.fc, csr->indptr.get());
    XR_LAUNCH("assemble", k_assemble, dim3(grid), dim3(FB), 0, query->qo_bbox(), query->qo_fxy(), query->qo_len(), query->m,
              query->qo_perm(), b.T, b.cand_tgt.get(), b.l.cand_off.get(), b.l.cand_count.get(), b.l.block_seg.get(), b.l.is_big.get(),
              b.cand_area.get(), b.cand_sid.get(), b.tree_area, b.relative, b.tile, b.tile_key, a.fc, csr->indptr.get(),
              csr->indices.get(), csr->data.get(), csr->stored.row_order.get(), a.cap, b.remap,
              b.scan_mode == 1 ? b.blk_base.get() : (const int32_t *)nullptr,
              b.scan_mode == 1 ? b.blk_base.get() + grid : (const int32_t *)nullptr,
              b.scan_mode == 2 ? b.blk_rows : (const int32_t *)nullptr, b.scan_mode == 2 ? b.blk_surv : (const int32_t *)nullptr);
}

// (5) The tail.  Behind the join the big faces' rows lie complete in their own small CSR, and the list of long rows is final.
// An apply that can read them THERE (K = 1, xr_overlap_apply_dev) does not wait for their copy behind the regular rows:
// its launch leads with the blocks that make the copy (k_apply_tail1), one launch and one kernel boundary less between
// the assembly and the apply.  It stays BEHIND k_publish_all, which hands it n_big and the regular rows' entries with
// the gate (TailWord): the host's read-back and its enqueueing of the next build stay hidden behind the apply.
// (The apply in front of k_publish_all, on the control block itself, was measured: the host then learns the sizes
// one apply later and the device idles for its ~30 us of enqueueing, 0.469 -> 0.488 ms per step.)
// -> what places the big rows: k_place_big here (!tail_fused), or the apply's launch
static PlaceBig enqueue_tail(const FusedBuild &b, const FusedAttempt &a, bool tail_fused) {
    side_join();
    const xr_mesh *query = b.query;
    xr_csr *csr = b.csr;
    const PlaceBig place{a.n_big_dev, b.slot_face.get(), b.big_indptr.get(), a.big_indices.get(), a.big_data.get(), b.T,
                         query->qo_perm(), query->qo_bbox(), query->qo_fxy(), query->qo_len(), query->m, b.tile, b.tile_key, a.fc,
                         csr->indptr.get(), csr->indices.get(), csr->data.get(), csr->stored.row_order.get(), a.cap, a.n_pending_dev};
    if (!tail_fused) XR_LAUNCH("place_big", k_place_big, dim3(TAIL_PLACE_BLOCKS), dim3(256), 0, place);
    return place;
}

// (6) publish -- sizes and error bits to the mailbox, the gate and the tail's words to the matrix, the control block zero
// again -- then the early apply, gated by the word k_publish_all has just set.  -> the sequence number the mailbox will show
static int32_t enqueue_publish_and_apply(const FusedBuild &b, const FusedAttempt &a, const PlaceBig &place, bool tail_fused,
                                         EarlyApply *early) {
    host_stamp(5);
    const int32_t seq = mailbox_next_seq();
    XR_LAUNCH("publish", k_publish_all, dim3(1), dim3(64), 0, a.ctl, a.fc, b.csr->longs.n_dev.get(), const_cast<int32_t *>(engine().mailbox),
              seq, a.cap, a.big_capacity);
    if (a.ctl_cached) zero_scratch_done(1); // (the counters are zero again behind k_publish_all)
    if (early) {
        const ApplyTail tail{place, b.csr->longs.n_dev.get()};
        const ApplyContext ctx{b.csr->longs.n_dev.get() + TAIL_GATE, tail_fused ? &tail : nullptr};
        early->fn(b.csr, &ctx);
    }
    host_stamp(6);
    return seq;
}

// (7) the one host round trip of the build
static FusedMail read_back(int32_t seq) {
    mailbox_wait_seq(seq);
    host_stamp(7);
    const int32_t *mail = const_cast<const int32_t *>(engine().mailbox);
    return FusedMail{mail[MAIL_REG_PAIRS], mail[MAIL_BIG_PAIRS], mail[MAIL_N_BIG], mail[MAIL_N_PENDING], mail[MAIL_ERROR],
                     mail[MAIL_ROWS_REGULAR], mail[MAIL_N_APPLY_LONG], mail[MAIL_P_REGULAR], mail[MAIL_P_BIG], mail[MAIL_MAX_ROW]};
}

bool overlap_tri(xr_mesh *tree, xr_mesh *query, const double *tree_area, bool relative, xr_csr *csr, const MortonParams &tile,
                 EarlyApply *early) {
    FusedBuild b{tree, query, tree_area, relative, csr, tile, csr->tiling.pending ? csr->tiling.key.get() : nullptr};
    const int64_t T = b.T;
    // (CsrLongRows::begin is not used on this timed path: the list is sized per attempt (attempt_allocate), the words once, and
    // k_publish_all writes them -- no clear)
    csr->longs.n_dev.alloc(TAIL_WORDS); // (TailWord: the rows of more than XR_APPLY_LONG_ROW entries, the gate of an apply enqueued behind the build ...)
    csr->stored.row_order.alloc((size_t)T);
    csr->stored.has_row_order = true;
    const bool tail_fused = early && early->takes_tail && option(OPT_TAIL_FUSED) != 0;
    const int64_t margin_opt = option(OPT_QUEUE_MARGIN); // test hook: a tiny margin forces the regrow path
    int64_t big_capacity = margin_opt > 0 ? margin_opt : ((int64_t)4 << 20);
    int64_t per_face = 8; // CSR entries reserved per target face (+ the big queue); regrown if the matrix is denser
    for (int attempt = 0;; attempt++) {
        XR_REQUIRE(attempt < 8, XR_ERR_LIMIT, "xr_overlap: the weight matrix does not fit the device buffers");
        FusedAttempt a;
        attempt_allocate(b, a, per_face, big_capacity);
        enqueue_search(b, a);
        enqueue_big_chain(b, a);
        enqueue_regular(b, a);
        const PlaceBig place = enqueue_tail(b, a, tail_fused);
        const int32_t seq = enqueue_publish_and_apply(b, a, place, tail_fused, early);
        const FusedMail m = read_back(seq);
        const FusedOutcome verdict = fused_outcome(m.c_reg, m.c_big, m.n_pending, m.err, m.p_regular, m.p_big, a.cap, a.big_capacity);
        XR_REQUIRE(verdict != FUSED_LIMIT, XR_ERR_LIMIT, "candidate pair count exceeds the int32 range");
        if (debug_fused()) {
            const int32_t *len = const_cast<const int32_t *>(engine().mailbox) + MAIL_REGION_LEN;
            fprintf(stderr, "[tri] T=%lld C=%d big: %d faces %d pairs (%d pending) p_regular=%d p_big=%d err=%d rows=%d long=%d regions %d %d %d %d %d %d %d %d of %lld\n",
                    (long long)T, m.c_reg, m.n_big, m.c_big, m.n_pending, m.p_regular, m.p_big, m.err, m.rows_regular, m.n_apply_long, len[0],
                    len[1], len[2], len[3], len[4], len[5], len[6], len[7], (long long)b.region_cap);
        }
        switch (verdict) {
        case FUSED_GENERAL:
            csr->stored.has_row_order = false; // (the general pipeline stores the rows in query order)
            return false;
        case FUSED_GROW_BIG: // some big faces needed more room than the margin
            big_capacity = (int64_t)m.c_big + 1024;
            continue;
        case FUSED_GROW_CSR:
            per_face *= 2;
            continue;
        default: // FUSED_FINAL
            break;
        }
        XR_REQUIRE(m.rows_regular == T - m.n_big, XR_ERR_INVALID, "xr_overlap: internal row count mismatch");
        tree->last_candidates = (int64_t)m.c_reg + m.c_big;
        csr->nnz = (int64_t)m.p_regular + m.p_big;
        csr->longs.end(m.n_apply_long); // rows of more than XR_APPLY_LONG_ROW entries (none: the apply skips their kernels)
        csr->longs.max_row_len = m.n_apply_long > 0 ? m.max_row : XR_APPLY_LONG_ROW;
        if (early) early->done = true; // (the apply enqueued in THIS attempt saw the final matrix)
        return true;
    }
}

} // namespace xr
