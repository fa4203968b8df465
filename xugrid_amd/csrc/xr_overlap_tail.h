// xr_overlap_tail.h -- what the fused weight build (xr_overlap_fused.hip) and the K = 1 apply enqueued behind it
// (xr_apply_stream.hip: k_apply_tail1, xr_partial.hip) share: the control block's words, the verdict on an attempt -- ONE function,
// evaluated by k_publish_all for the gate and by overlap_tri after its read-back --, the context an apply enqueued behind the
// build is handed, and the placement of the big faces' rows behind the regular ones -- a launch of its own (k_place_big) or
// the leading blocks of the apply's launch.
#pragma once
#include <cstddef>

#include "xr_geom.h"

namespace xr {

static constexpr int QCUR_STRIDE = 32; // words between the cursors of the regular queue's eight regions: a 128-byte line each

struct FusedCounters {                    // device words, zeroed before the launch
    int32_t n_apply_long;                 // rows with more than XR_APPLY_LONG_ROW entries
    int32_t error;                        // bit 0 (1): clip buffer overflow, bit 2 (4): CSR capacity -- no other bit is ever set
    int32_t p_regular;                    // entries of all regular rows (k_assemble)
    int32_t rows_regular;                 // regular rows
    int32_t p_big;                        // entries of the big faces' rows (k_big_order)
    int32_t pad0;                         // (unused)
    int32_t max_row;                      // entries of the longest row (atomicMax)
    int32_t pad2;
};

// ---- the words device and host share: ONE description, used by the kernels' launches, k_publish_all and overlap_tri ----
// Control block of a fused build: CTL_WORDS device words, zero at rest (the engine's zero-at-rest scratch; k_publish_all
// clears what the build raised), indexed by CtlWord.
enum CtlWord : int {
    CTL_REG_CURSOR = 0,     // pairs of the regular queue; the eight region cursors below count them, k_publish_all puts their sum here
    CTL_BIG_CURSOR = 1,     // pairs in the big faces' queue (k_search_big)
    CTL_N_BIG = 2,          // big faces (k_search)
    CTL_N_PENDING = 3,      // big faces whose pairs did not fit their queue: > 0 makes the side-stream kernels skip, the host regrows
    CTL_BIG_OVERFLOW = 4,   // clip overflows among the big pairs (reserved: they are reported through FusedCounters::error)
    CTL_COUNTERS = 8,       // FusedCounters
    CTL_LINE = 16,          // words [0, CTL_LINE) are one 64-byte stretch that k_publish_all fetches with one load per lane
    CTL_REGION_CURSOR = 32, // cursors of the regular queue's eight regions (one per XCD), QCUR_STRIDE words = a 128-byte line apart
    CTL_WORDS = CTL_REGION_CURSOR + 8 * QCUR_STRIDE
};
#define XR_CTL_COUNTER(field) (xr::CTL_COUNTERS + (int)(offsetof(xr::FusedCounters, field) / sizeof(int32_t))) // control word of a FusedCounters field
static_assert(CTL_COUNTERS + sizeof(FusedCounters) / sizeof(int32_t) <= CTL_LINE && CTL_BIG_OVERFLOW < CTL_COUNTERS &&
                  CTL_LINE <= CTL_REGION_CURSOR && CTL_LINE + 8 <= 64,
              "the counters lie inside the line k_publish_all's one wave fetches, the region cursors behind it");

// The verdict on one attempt of the fused build, from the words k_publish_all sends to the mailbox.  ONE function for both
// sides: k_publish_all opens the gate of an apply enqueued behind the build only on FUSED_FINAL, and overlap_tri switches on
// the same value after its read-back -- so the host never declares a step done whose apply left at a closed gate.  A failed
// attempt leaves row pointers no kernel may follow.  c_reg: the pairs of the regular queue (the sum of its eight regions'
// cursors), c_big: those of the big faces' queue, cap / big_capacity: entries the CSR / the big faces' queue have room for.
enum FusedOutcome : int {
    FUSED_FINAL = 0, // the attempt produced the final matrix
    FUSED_LIMIT,     // a pair count left the int32 range: XR_ERR_LIMIT
    FUSED_GENERAL,   // a clip needed more vertices than its buffer holds (error bit 0): the general chain
    FUSED_GROW_BIG,  // big faces' pairs did not fit their queue: again with a longer one
    FUSED_GROW_CSR   // the matrix is denser than the CSR reserved (error bit 2, or the big rows found no room): per_face doubles
};
__host__ __device__ inline FusedOutcome fused_outcome(int32_t c_reg, int32_t c_big, int32_t n_pending, int32_t err, int32_t p_regular,
                                                      int32_t p_big, int64_t cap, int64_t big_capacity) {
    if (c_reg < 0 || c_big < 0) return FUSED_LIMIT;
    if (err & 1) return FUSED_GENERAL;
    if (n_pending > 0 || (int64_t)c_big > big_capacity) return FUSED_GROW_BIG;
    if ((err & 4) || (int64_t)p_regular + p_big > cap) return FUSED_GROW_CSR;
    return FUSED_FINAL;
}

// The finished rows of the big faces (ranked by k_row_fill_long into big_indices / big_data on the side stream) go
// BEHIND the regular rows: stored row T - n_big + slot.
struct PlaceBig {
    const int32_t *n_big_dev, *slot_face, *big_indptr, *big_indices;
    const double *big_data;
    int64_t n_query;
    const int32_t *q_perm;
    const double *q_bbox, *q_fxy;
    const uint8_t *q_len;
    int q_m;
    MortonParams tile;
    int32_t *tile_key;
    FusedCounters *counters;
    int32_t *indptr, *indices;
    double *data;
    int32_t *row_order;
    int64_t csr_capacity;
    const int32_t *skip_if;
};

#ifdef __HIPCC__
// Grid-stride over rows and entries, by block `block` of `n_blocks` blocks of 256 threads.  (Which of these rows the apply
// reduces cooperatively is listed where their lengths are first known, by k_row_fill_long.)
// IN_TAIL: the blocks run beside blocks that read the regular rows' pointers up to indptr[T - n_big] -- the word the assembly
// stored, and the one word of the regular rows this function would store again (same value): left alone there, so that no
// block of that launch reads what another one writes.
template <bool IN_TAIL>
__device__ __forceinline__ void place_big_copy(const PlaceBig &p, int n_big, int64_t p_regular, int64_t p_big, int block, int n_blocks) {
    const int64_t t_reg = p.n_query - n_big;
    const int64_t i0 = (int64_t)block * 256 + threadIdx.x, stride = (int64_t)n_blocks * 256;
    for (int64_t k = i0; k < n_big; k += stride) {
        const int f = p.slot_face[k];
        const int64_t r = t_reg + k;
        if (!(IN_TAIL && k == 0)) p.indptr[r] = (int32_t)(p_regular + p.big_indptr[k]);
        p.row_order[r] = p.q_perm ? p.q_perm[f] : f;
        if (p.tile_key) {
            const int64_t mid = ((int64_t)f & ~(int64_t)(p.tile.n_run - 1)) + p.tile.n_run / 2;
            p.tile_key[r] = morton_key(p.tile, query_face_box_rt(p.q_bbox, p.q_fxy, p.q_len, p.q_m, mid < p.n_query ? mid : p.n_query - 1));
        }
    }
    for (int64_t e = i0; e < p_big; e += stride) {
        p.indices[p_regular + e] = p.big_indices[e];
        p.data[p_regular + e] = p.big_data[e];
    }
    if (i0 == 0) p.indptr[p.n_query] = (int32_t)(p_regular + p_big);
}
// ... behind the checks on the control block's words: nothing to place, big faces that did not fit their queue (the host redoes
// everything), a matrix that does not fit the CSR (error bit 2: the host regrows)
template <bool IN_TAIL>
__device__ __forceinline__ void place_big_rows(const PlaceBig &p, int block, int n_blocks) {
    const int n_big = *p.n_big_dev;
    if (n_big == 0 || *p.skip_if > 0) return;
    const int64_t p_regular = p.counters->p_regular, p_big = p.big_indptr[n_big];
    if (p_regular + p_big > p.csr_capacity) {
        if (block == 0 && threadIdx.x == 0) atomicOr(&p.counters->error, 4);
        return;
    }
    place_big_copy<IN_TAIL>(p, n_big, p_regular, p_big, block, n_blocks);
}
#endif

// What the K = 1 apply's launch needs to take the place of k_place_big and to read the big rows from the big faces' own CSR.
struct ApplyTail {
    PlaceBig place;
    const int32_t *words; // what k_publish_all left in the matrix' own words (xr_csr::longs.n_dev), indexed by TailWord
};
// What overlap_tri hands an apply it enqueues behind an attempt, before the host has read the attempt's sizes back
// (csr_apply_dev, csr_partial_dev; callers with a finished matrix pass none).  The sizes of the matrix are then not known on
// the host: the apply assumes long rows of any length -- that only adds blocks which look at the device-side list of long rows
// and find it short or empty; results do not depend on it.
struct ApplyContext {
    const int32_t *gate;   // the build's gate word (TAIL_GATE): every block of the apply leaves unless the attempt was final
    const ApplyTail *tail; // the apply's launch places the big rows itself (k_apply_tail1), or null
    bool has_long = true;     // (in place of xr_csr::longs.any / longs.max_row_len: long rows possible, of any length)
    int64_t max_row_len = -1;
};
// xr_csr::longs.n_dev of a matrix of the fused build, written by k_publish_all
enum TailWord : int { TAIL_N_LONG = 0, TAIL_GATE = 1, TAIL_N_BIG = 2, TAIL_P_REGULAR = 3, TAIL_WORDS = 4 };
static constexpr int TAIL_PLACE_BLOCKS = 64; // leading blocks of the apply's launch that place the big rows (k_place_big's grid)

} // namespace xr
