// xr_apply.h -- what the units of the sparse apply share besides the reducers (xr_reduce.h): xr_apply.hip (the entry points
// and the dispatch of the full apply) with its three pipelines -- xr_apply_stream.hip (the streamed reducers),
// xr_apply_plan.hip (the many-variable plan), xr_apply_workspace.hip (mode and percentiles) --, xr_partial.hip (the partial
// states of the source-sharded apply), xr_csr.hip (the MatrixCSR handle) and xr_outer.hip (the separable weights).
// Constants, a few host helpers, and the functions one of these units defines for the others: plain functions that take the
// reducer and dtype ids -- every unit dispatches to the kernels it owns itself, no template crosses a unit boundary.
#pragma once
#include "xr_objects.h"
#include "xr_overlap_tail.h"

namespace xr {

static constexpr int AP_BLOCK = 256;

// Rows longer than APPLY_LONG entries are not reduced by one thread: a coarse target cell over a fine source
// has tens to thousands of entries, and a thread walking such a row alone reads its CSR entries uncoalesced and
// waits one memory latency per entry.  They are reduced by one WAVE each (lanes stride the row: coalesced
// entries, neighbouring columns gathered together) or, beyond APPLY_WAVE entries, by a whole block: strided
// partial states merged in a fixed butterfly order -> deterministic, but the summation order differs from
// the reference's sequential loop (agreement ~1e-15 relative instead of bit-exact).
static constexpr int APPLY_LONG = XR_APPLY_LONG_ROW;
static constexpr int APPLY_WAVE = XR_APPLY_WAVE_ROW;
// ... by a group of 16 lanes up to APPLY_GROUP16 entries, by all 64 beyond (apply_row_group, xr_apply_stream.hip; the row pass of
// the adjoint walks the same way, xr_adjoint.hip)
static constexpr int APPLY_GROUP16 = 512;

// the wave window of the K = 1 kernels (k_apply_rows1, k_apply_partial_w1)
static constexpr int W1_CAP = 384; // entries per wave window: 64 rows x 4 entries (the mean of a triangle pair) + slack for the tail
                                   // (measured on the 1M x 1M matrix: 256 / 320 / 384 / 448 entries -> kernel 31 / 30 / 27 / 27 us)

// K >= PLAN_KT variables go through the apply plan (ensure_plan, k_apply_plan)
static constexpr int PLAN_KT = 8; // source variables per pipeline stage (LDS: PLAN_KT * PLAN_UMAX doubles)

static inline const int32_t *row_order_of(const xr_csr *csr) {
    return (csr->stored.has_row_order && !csr->stored.output_stored) ? csr->stored.row_order.get() : nullptr;
}

// (with_source_type, the table of the source dtypes, is in xr_internal.h)
static size_t source_size(int dtype) {
    size_t size = 0;
    with_source_type(dtype, [&](auto tag) { size = sizeof(tag); });
    return size;
}
// ... and back: the dtype id of an element type, for a call into another unit
template <typename SRC> constexpr int source_dtype = sizeof(SRC) == sizeof(double) ? XR_F64 : XR_F32;

// the caller's source block into the stored column order: dst[k][j] = src[k][col_of[j]] (every source line is read once;
// the columns of a line are spatial neighbours, so they are consumed within a short stretch of j: L2 hits)
// (`static`, as the kernels of xr_prims.h: every unit that launches it through stored_source gets its own copy)
template <typename SRC>
static __global__ void __launch_bounds__(256)
k_permute_source(const SRC *__restrict__ src, const int32_t *__restrict__ col_of, int64_t S, SRC *__restrict__ dst) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t k = blockIdx.y;
    if (j < S) dst[k * S + j] = src[k * S + col_of[j]];
}

// -> the source block in the STORED column order (the caller's block itself unless the columns were renumbered)
template <typename SRC>
static const SRC *stored_source(const xr_csr *csr, const SRC *src, int64_t K, DevBuf<char> &permuted) {
    if (!(csr->cols.permuted && !csr->cols.source_permuted && K > 0 && csr->m > 0)) return src;
    permuted.alloc((size_t)K * (size_t)csr->m * sizeof(SRC));
    SRC *dst = reinterpret_cast<SRC *>(permuted.get());
    for (int64_t k0 = 0; k0 < K; k0 += 65535) {
        const int64_t kc = std::min<int64_t>(K - k0, 65535);
        dim3 grid(div_up(csr->m, 256), (unsigned)kc);
        XR_LAUNCH("permute_source", k_permute_source<SRC>, grid, dim3(256), 0, src + k0 * csr->m, csr->cols.col_of.get(), csr->m,
                  dst + k0 * csr->m);
    }
    return dst;
}

// A host-array apply: the stacked variables go through the device in chunks of at most ~4 GiB of staging (n_src source
// elements of esz bytes + n_out float64 results per variable), so any K works whatever the size of HBM; every variable is
// independent, results do not depend on the chunking.  chunk(k0, kc, src, dst) moves and applies variables k0 ... k0 + kc.
template <typename F> static void staged_chunks(int64_t K, int64_t n_src, size_t esz, int64_t n_out, F &&chunk) {
    const size_t per_k = (size_t)n_src * esz + (size_t)n_out * sizeof(double);
    const int64_t chunk_opt = option(OPT_APPLY_CHUNK_BYTES); // test hook
    const size_t budget = chunk_opt > 0 ? (size_t)chunk_opt : ((size_t)4 << 30);
    int64_t kchunk = per_k > 0 ? (int64_t)(budget / per_k) : K;
    if (kchunk < 1) kchunk = 1;
    if (kchunk > K) kchunk = K;
    DevBuf<char> src((size_t)kchunk * (size_t)n_src * esz);
    DevBuf<double> dst((size_t)kchunk * (size_t)n_out);
    for (int64_t k0 = 0; k0 < K; k0 += kchunk) {
        chunk(k0, (K - k0) < kchunk ? (K - k0) : kchunk, src.get(), dst.get());
        stream_sync();
    }
}

// xr_csr.hip
void upload_narrow(const int64_t *host, int64_t n, int32_t *dev); // host int64 -> device int32 (sizes checked by the caller)
// the matrix as the caller numbers it (what xr_csr_download copies out): the stored arrays, or copies the view owns
struct CallerView {
    const int32_t *indptr = nullptr, *indices = nullptr;
    const double *data = nullptr;
    DevBuf<int32_t> c_indptr, c_indices, c_columns;
    DevBuf<double> c_data;
};
void caller_view(const xr_csr *csr, CallerView &view, bool want_columns = true);
void ensure_tiled(const xr_csr *csr);                             // the row tiling, if keys are pending (exclusive scope)
int prepare_for_apply(const xr_csr *csr, int64_t K);              // row tiling + apply plan in front of a shared-scope apply
// xr_apply_plan.hip
void ensure_plan(const xr_csr *csr);                              // the apply plan of the many-variable kernels (exclusive scope)
// the planned row blocks of a matrix whose plan is built ("apply_plan"; the unplanned blocks and the long rows: launch_stream)
void apply_planned(const xr_csr *csr, int method, const void *src_dev, int dtype, int64_t K, double *out_dev);
// xr_apply_stream.hip, xr_apply_workspace.hip: the two halves of apply_dispatch -- the streamed reducers (which place
// apply_planned in their launch sequence) and mode / percentiles.  src_dev is in the STORED column order (stored_source)
void apply_stream(const xr_csr *csr, int method, const void *src_dev, int dtype, int64_t K, double *out_dev, const ApplyContext *ctx);
void apply_workspace(const xr_csr *csr, int method, double percentile, const void *src_dev, int dtype, int64_t K, double *out_dev);
// the apply of a finished matrix on the calling thread's launch stream (xr_apply.hip) and its partial states for the
// source-sharded apply (xr_partial.hip).  ctx: the apply is enqueued behind a weight build the host has not confirmed yet (K = 1,
// overlap_tri) -- it obeys the build's gate and may take the build's tail into its launch (ApplyContext, xr_overlap_tail.h)
void csr_apply_dev(const xr_csr *csr, int method, double percentile, const void *src_dev, int dtype, int64_t K, double *out_dev,
                   const ApplyContext *ctx = nullptr);
void csr_partial_dev(const xr_csr *csr, int method, const void *src_dev, int dtype, int64_t K, double *out_dev, int rows_layout,
                     const ApplyContext *ctx = nullptr);

// xr_adjoint.hip
void ensure_transposed(const xr_csr *csr);                        // the transposed weights of the adjoint (exclusive scope)
int prepare_for_adjoint(const xr_csr *csr, int method);           // ... in front of a shared-scope adjoint (checks the reducer first)
// the adjoint of csr_apply_dev for the reducers that are linear in the source (src_dev may be NULL: no NaN in the source)
void csr_adjoint_dev(const xr_csr *csr, int method, const void *src_dev, int dtype, const double *grad_dev, int64_t K,
                     double *out_dev);

} // namespace xr
