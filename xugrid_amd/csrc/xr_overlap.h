// xr_overlap.h -- what the three units of the weight construction share: xr_overlap.hip (the search, the long rows' kernel,
// the entry points), xr_overlap_general.hip (the general chain) and xr_overlap_fused.hip (the fused pipeline).  The sizes and
// the block order every unit's kernels agree on, the host structs the shared launchers take, and the functions one unit
// defines for the others.  (Device code both pipelines' clips use: xr_clip.h; the seam to the apply: xr_overlap_tail.h.)
#pragma once
#include <functional>

#include "xr_objects.h"
#include "xr_overlap_tail.h"

namespace xr {

// One traversal per query face: hits are parked in SLOTS LDS slots per face and counted; the block
// then compacts them into its stretch of the candidate-pair queue.  Faces with more than SLOTS
// hits, too many grid rows or too many visited records are "big" and go to the block-per-face
// kernel instead.
static constexpr int SLOTS = 16;
static_assert(SLOTS <= XR_APPLY_LONG_ROW, "a regular row is never one of the apply's long rows: only k_row_fill_long lists");
static constexpr int FB = 256;            // faces (= threads) per block: the block granularity of k_search's queue stretches
static constexpr int FWAVES = FB / 64;

// XCD-aware block order (launch the grid rounded up to a multiple of 8): hardware block b runs on XCD b % 8; every
// XCD gets a CONTIGUOUS range of logical blocks (= one spatial region of the Morton-ordered work list), so that the
// lines shared by neighbouring blocks stay in one L2.  -> logical block (>= n_blocks: nothing to do)
__device__ __forceinline__ int64_t xcd_block(int64_t n_blocks, bool remap) {
    if (!remap) return blockIdx.x;
    const int64_t per_xcd = (n_blocks + 7) >> 3;
    return (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
}
// Which kernels take the XCD-aware block order (xcd_block): clip + search fetch 15 % fewer HBM bytes with it (PMC: clip
// 161 -> 130 MB, search 56 -> 48 MB per launch) at an unchanged clip time and a 5 % shorter search; row_fill loses more on
// the then interleaved queue than it gains.
static constexpr bool REMAP_CLIP = true, REMAP_SEARCH = true, REMAP_ROW_FILL = false;
static unsigned xcd_grid(int64_t n_blocks, bool remap) { return (unsigned)(remap ? (n_blocks + 7) / 8 * 8 : n_blocks); }

// ---- launches both pipelines share --------------------------------------------------------------------------------------
// what the search leaves per target face and per block of 256 of them
struct SearchLists {
    DevBuf<int32_t> cand_count, cand_off, big_list, pending, nnz_row;
    DevBuf<uint8_t> is_big;
    DevBuf<int2> block_seg;
    explicit SearchLists(int64_t T)
        : cand_count((size_t)T), cand_off((size_t)T + 1), big_list((size_t)T), pending((size_t)T), nnz_row((size_t)T),
          is_big((size_t)T), block_seg((size_t)div_up(T, 256)) {}
};
// the pair queue a kernel appends to
struct PairQueue {
    int32_t *tgt, *src, *cursor;
    int64_t capacity; // (of one region where the queue is the fused pipeline's eight regions with a cursor each)
};

// k_row_fill_long over one class of the listed rows: 0 every row; 1 the rows of at most ROW_BLOCK candidates (16 KB of LDS:
// six blocks per CU, resident beside other kernels); 2 the longer ones (the bitmap: a CU per block).
struct LongRows { // (the kernel's arguments of the same names)
    const int32_t *cand_sid;
    const double *cand_area;
    const int32_t *indptr;
    int32_t *indices;
    double *data;
    const int32_t *long_rows, *n_long;
    int64_t row_base;
    const int32_t *skip_if = nullptr, *scan_nnz = nullptr;
    int32_t *scan_indptr = nullptr, *scan_total = nullptr;
    int32_t *apply_long_rows = nullptr; // (scan_nnz mode) the apply's list of long rows, FusedCounters that count it, stored rows
    FusedCounters *listed = nullptr;
    int64_t n_stored = 0;
};

// An apply the caller wants right behind the weight build (xr_overlap_apply_dev).  The triangle pipeline enqueues it BEFORE
// the host has read the sizes back -- the K = 1 apply kernel takes everything it needs from device memory -- so the one host
// round trip of the build is hidden behind the apply instead of standing between the two.
struct EarlyApply {
    std::function<void(const xr_csr *, const ApplyContext *)> fn; // (the context goes through to csr_apply_dev / csr_partial_dev)
    bool takes_tail = false; // fn enqueues the K = 1 kernel that places the big rows itself (ApplyContext::tail)
    bool done = false;
};

// ---- xr_overlap.hip
double overlap_dust_threshold(const xr_mesh *tree, const xr_mesh *query); // areas up to this are confirmed by the reference's pre-clip tests
// k_search over every target face.  PACKED: the owner byte rides in the record id's top byte where the tree has at most
// 2^24 faces.  blk_rows / blk_surv: the fused pipeline's per-block counts; its queue is then eight regions.
void launch_search(const xr_mesh *tree, const xr_mesh *query, const SearchLists &l, const PairQueue &q, int32_t *n_big,
                   const MortonParams &tile, int32_t *tile_key, int32_t *blk_rows = nullptr, int32_t *blk_surv = nullptr);
// k_search_big<true>: the listed big faces, one block each, into `q`; faces that do not fit it are listed in l.pending
void launch_search_big(const xr_mesh *tree, const xr_mesh *query, const SearchLists &l, const PairQueue &q, const int32_t *n_big,
                       int32_t *n_pending, int32_t *slot_face = nullptr);
// k_search_big<false>: the faces of l.pending (n_pending: their device count) into the stretches they reserved in a regrown `q`
void launch_search_big_fill(const xr_mesh *tree, const xr_mesh *query, const SearchLists &l, const PairQueue &q,
                            const int32_t *n_pending);
void launch_row_fill_long(int row_class, const xr_mesh *tree, const SearchLists &l, const double *tree_area, bool relative,
                          const LongRows &r);
// ---- xr_overlap_fused.hip
// Dense meshes of at most 4 nodes per face: search -> persistent clip -> assembly, the big faces of the search (hull slivers
// ...) on a side stream, their rows stored behind the regular ones; ONE host round trip at the very end (sizes + error bits).
// -> false if the pair has to go through the general pipeline after all (a clip that needs more vertices than its buffer
// holds: floating-point degenerate input).
bool overlap_tri(xr_mesh *tree, xr_mesh *query, const double *tree_area, bool relative, xr_csr *csr, const MortonParams &tile,
                 EarlyApply *early);
// ---- xr_overlap_general.hip
// The general kernel chain, all on the engine stream: two host round trips, rows in query order.
void overlap_general(xr_mesh *tree, xr_mesh *query, const double *tree_area, bool relative, xr_csr *csr, const MortonParams &tile);

} // namespace xr
