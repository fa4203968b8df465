// xr_csr.hip -- the MatrixCSR handle: upload, download, assembly from sorted triplets, the row and column keys with
// the row tiling they ask for, and the stored orders a caller may read.
//
// Replaces MatrixCSR.from_triplet / MatrixCOO.to_csr (xugrid/core/sparse.py:61-78,119-127).
// CSR = indptr i32[T+1], indices i32[nnz], data f64[nnz] (xr_objects.h).
#include <vector>

#include "xr_apply.h"
#include "xr_prims.h"

namespace xr {

__global__ void k_narrow_i64(const int64_t *__restrict__ in, int32_t *__restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int32_t)in[i];
}
__global__ void k_bincount(const int32_t *__restrict__ row, int64_t nnz, int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nnz) atomicAdd(&count[row[i]], 1);
}

__global__ void k_gather_i32(const int32_t *__restrict__ table, const int32_t *__restrict__ idx, int64_t n,
                             int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = table[idx[i]];
}
__global__ void k_scatter_iota_i32(const int32_t *__restrict__ perm, int64_t n, int32_t *__restrict__ inverse) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) inverse[perm[i]] = (int32_t)i;
}
__global__ void k_relabel_i32(const int32_t *__restrict__ table, int32_t *__restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = table[idx[i]];
}

// stored row r -> caller row row_order[r]
__global__ void k_unpermute_len(const int32_t *__restrict__ indptr, const int32_t *__restrict__ row_order, int64_t n,
                                int32_t *__restrict__ len) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) len[row_order[r]] = indptr[r + 1] - indptr[r];
}
// one wave per stored row
__global__ void k_unpermute_rows(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                 const double *__restrict__ data, const int32_t *__restrict__ row_order, int64_t n,
                                 const int32_t *__restrict__ c_indptr, int32_t *__restrict__ c_indices,
                                 double *__restrict__ c_data) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const int s = indptr[r], e = indptr[r + 1], d = c_indptr[row_order[r]];
    for (int j = s + lane; j < e; j += 64) {
        c_indices[d + (j - s)] = indices[j];
        c_data[d + (j - s)] = data[j];
    }
}

void upload_narrow(const int64_t *host, int64_t n, int32_t *dev) {
    if (n <= 0) return;
    DevBuf<int64_t> wide((size_t)n);
    h2d(wide.get(), host, sizeof(int64_t) * (size_t)n);
    XR_LAUNCH("narrow_i64", k_narrow_i64, dim3(div_up(n, 256)), dim3(256), 0, wide.get(), dev, n);
}

// The matrix in the CALLER's row and column ids whatever order it is stored in: rows stored in query order are put back
// (stored row r is the caller's row row_order[r]) and renumbered columns are translated, into copies the view owns; a matrix
// stored as the caller numbers it is viewed in place.  want_columns = false leaves the stored column ids.
void caller_view(const xr_csr *csr, CallerView &v, bool want_columns) {
    v.indptr = csr->indptr.get(), v.indices = csr->indices.get(), v.data = csr->data.get();
    if (csr->stored.has_row_order && csr->n > 0) {
        DevBuf<int32_t> len((size_t)csr->n);
        v.c_indptr.alloc((size_t)csr->n + 1);
        v.c_indices.alloc((size_t)csr->nnz);
        v.c_data.alloc((size_t)csr->nnz);
        XR_LAUNCH("unpermute_len", k_unpermute_len, dim3(div_up(csr->n, 256)), dim3(256), 0, csr->indptr.get(),
                  csr->stored.row_order.get(), csr->n, len.get());
        exclusive_scan_i32(len.get(), v.c_indptr.get(), csr->n);
        XR_LAUNCH("unpermute_rows", k_unpermute_rows, dim3(div_up(csr->n * 64, 256)), dim3(256), 0, csr->indptr.get(),
                  csr->indices.get(), csr->data.get(), csr->stored.row_order.get(), csr->n, v.c_indptr.get(), v.c_indices.get(),
                  v.c_data.get());
        v.indptr = v.c_indptr.get(), v.indices = v.c_indices.get(), v.data = v.c_data.get();
    }
    if (want_columns && csr->cols.permuted && csr->nnz > 0) { // stored column ids -> the caller's
        v.c_columns.alloc((size_t)csr->nnz);
        XR_LAUNCH("col_ids", k_gather_i32, dim3(div_up(csr->nnz, 256)), dim3(256), 0, csr->cols.col_of.get(), v.indices, csr->nnz,
                  v.c_columns.get());
        v.indices = v.c_columns.get();
    }
}

// the long rows as the host found them in the caller's arrays: the list and its count are uploaded, no kernel lists them
static void set_long_rows(xr_csr *csr, const std::vector<int32_t> &longs) {
    if (longs.empty()) return;
    const int32_t count = (int32_t)longs.size();
    csr->longs.begin(longs.size());
    h2d(csr->longs.rows.get(), longs.data(), sizeof(int32_t) * longs.size());
    h2d(csr->longs.n_dev.get(), &count, sizeof(int32_t));
    csr->longs.end(count);
}

// ---------------------------------------------------------------------------------------------
// Row tiling for many source variables.  The stored row order is free (row_order maps stored -> caller
// rows), and with K >= 8 variables the apply is bound by HBM traffic: a block of 256 stored rows that is a
// long strip of targets (consecutive ids of a lattice-numbered mesh) touches a few source values in each
// of very many cache lines, a compact 2-D tile touches long runs (measured on the 1M -> 1M benchmark,
// K = 256: 1.42 -> 1.06 ms).  Rows are regrouped once, by the coarse Morton key xr_overlap attached
// (stable: ascending stored row inside a tile), before the plan is built.
// ---------------------------------------------------------------------------------------------
__global__ void k_tile_scatter(const int32_t *__restrict__ key, int64_t n, const int32_t *__restrict__ start,
                               int32_t *__restrict__ cursor, int32_t *__restrict__ members) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) members[start[key[r]] + atomicAdd(&cursor[key[r]], 1)] = (int32_t)r;
}
// position i of the unordered member list -> its rank inside the tile by ascending row id
__global__ void k_tile_rank(const int32_t *__restrict__ key, const int32_t *__restrict__ start,
                            const int32_t *__restrict__ members, int64_t n, int32_t *__restrict__ perm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = members[i];
    const int s = start[key[r]], e = start[key[r] + 1];
    int rank = 0;
    for (int j = s; j < e; j++) rank += members[j] < r;
    perm[s + rank] = r;
}
__global__ void k_tile_len(const int32_t *__restrict__ indptr, const int32_t *__restrict__ perm, int64_t n,
                           int32_t *__restrict__ len) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) len[r] = indptr[perm[r] + 1] - indptr[perm[r]];
}
// one wave per new stored row
__global__ void k_tile_rows(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                            const double *__restrict__ data, const int32_t *__restrict__ row_order,
                            const int32_t *__restrict__ perm, int64_t n, const int32_t *__restrict__ t_indptr,
                            int32_t *__restrict__ t_indices, double *__restrict__ t_data,
                            int32_t *__restrict__ t_row_order, int32_t *__restrict__ long_rows,
                            int32_t *__restrict__ n_long) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const int old = perm[r];
    const int s = indptr[old], e = indptr[old + 1], d = t_indptr[r];
    for (int j = s + lane; j < e; j += 64) {
        t_indices[d + (j - s)] = indices[j];
        t_data[d + (j - s)] = data[j];
    }
    if (lane == 0) {
        t_row_order[r] = row_order ? row_order[old] : old;
        if (e - s > APPLY_LONG) long_rows[atomicAdd(n_long, 1)] = (int32_t)r;
    }
}

void ensure_tiled(const xr_csr *ccsr) {
    xr_csr *csr = const_cast<xr_csr *>(ccsr); // like the plan: a cache-friendly re-layout of the same matrix
    if (!csr->tiling.pending) return;
    // (a re-layout of the matrix: only under the exclusive scope -- the apply entry points call prepare_for_apply first,
    // so that the concurrent, shared part of an apply finds this done)
    XR_REQUIRE(exclusive_held(), XR_ERR_INVALID, "internal: row tiling requested outside the exclusive scope");
    csr->tiling.pending = false;
    const int64_t n = csr->n, R = csr->tiling.key_range;
    if (n == 0 || R <= 1) {
        csr->tiling.release();
        return;
    }
    DevBuf<int32_t> hist((size_t)R + 1), start((size_t)R + 1), members((size_t)n), perm((size_t)n), len((size_t)n);
    fill_i32(hist.get(), 0, R + 1);
    XR_LAUNCH("bincount", k_bincount, dim3(div_up(n, 256)), dim3(256), 0, csr->tiling.key.get(), n, hist.get());
    exclusive_scan_i32(hist.get(), start.get(), R);
    fill_i32(hist.get(), 0, R + 1);
    XR_LAUNCH("tile_scatter", k_tile_scatter, dim3(div_up(n, 256)), dim3(256), 0, csr->tiling.key.get(), n, start.get(),
              hist.get(), members.get());
    XR_LAUNCH("tile_rank", k_tile_rank, dim3(div_up(n, 256)), dim3(256), 0, csr->tiling.key.get(), start.get(),
              members.get(), n, perm.get());
    XR_LAUNCH("tile_len", k_tile_len, dim3(div_up(n, 256)), dim3(256), 0, csr->indptr.get(), perm.get(), n, len.get());
    DevBuf<int32_t> t_indptr((size_t)n + 1), t_indices((size_t)csr->nnz), t_row_order((size_t)n);
    DevBuf<double> t_data((size_t)csr->nnz);
    CsrLongRows t_longs; // (the rows keep their lengths; their stored positions are listed anew)
    t_longs.max_row_len = csr->longs.max_row_len;
    exclusive_scan_i32(len.get(), t_indptr.get(), n);
    t_longs.begin((size_t)(csr->nnz / APPLY_LONG + 1));
    XR_LAUNCH("tile_rows", k_tile_rows, dim3(div_up(n * 64, 256)), dim3(256), 0, csr->indptr.get(), csr->indices.get(),
              csr->data.get(), csr->stored.has_row_order ? csr->stored.row_order.get() : (const int32_t *)nullptr, perm.get(), n,
              t_indptr.get(), t_indices.get(), t_data.get(), t_row_order.get(), t_longs.rows.get(), t_longs.n_dev.get());
    t_longs.end();
    csr->indptr = std::move(t_indptr);
    csr->indices = std::move(t_indices);
    csr->data = std::move(t_data);
    csr->stored.row_order = std::move(t_row_order);
    csr->stored.has_row_order = true;
    csr->longs = std::move(t_longs);
    csr->rows_regrouped();
    csr->tiling.release();
}

// The row tiling of the many-variable apply is PART of the stored order.  It is normally deferred to the first apply with
// K >= 8; whoever is told the stored order (xr_csr_row_order) or asks for results in it (xr_csr_output_stored_order) gets
// it settled right away, whatever K the coming applies have -- otherwise a later apply would regroup the rows under a
// permutation the caller has already read, and every result after that would be silently mis-ordered.
static void settle_row_layout(const xr_csr *csr) {
    if (csr && csr->n > 0 && csr->tiling.pending) {
        ensure_tiled(csr);
        stream_sync();
    }
}

// Everything an apply may build lazily inside the matrix (row tiling, apply plan) is built here, under the EXCLUSIVE
// scope; the apply proper then only reads the matrix and runs under the shared scope next to other threads' applies.
int prepare_for_apply(const xr_csr *csr, int64_t K) {
    XR_API_BEGIN
    if (csr && csr->n > 0 && K >= PLAN_KT && option(OPT_APPLY_PLAN) != 0 && (csr->tiling.pending || !csr->plan.ready)) {
        ensure_tiled(csr);
        ensure_plan(csr);
        stream_sync();
    }
    XR_API_END
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_csr_info(const xr_csr *csr, int64_t *n, int64_t *m, int64_t *nnz) {
    XR_API_BEGIN
    XR_REQUIRE(csr, XR_ERR_INVALID, "xr_csr_info: NULL csr");
    if (n) *n = csr->n;
    if (m) *m = csr->m;
    if (nnz) *nnz = csr->nnz;
    XR_API_END
}

int xr_csr_download(const xr_csr *csr, double *data, int64_t *indices, int64_t *indptr) {
    XR_API_BEGIN
    XR_REQUIRE(csr, XR_ERR_INVALID, "xr_csr_download: NULL csr");
    CallerView v;
    caller_view(csr, v, indices != nullptr);
    const int32_t *d_indptr = v.indptr, *d_indices = v.indices;
    const double *d_data = v.data;
    if (data && csr->nnz > 0) {
        d2h(data, d_data, sizeof(double) * (size_t)csr->nnz);
    }
    DevBuf<int64_t> wide;
    if (indices || indptr) wide.alloc((size_t)std::max(csr->nnz, csr->n + 1));
    download_wide(d_indices, csr->nnz, indices, wide);
    download_wide(d_indptr, csr->n + 1, indptr, wide);
    stream_sync();
    XR_API_END
}

int xr_csr_upload(const double *data, const int64_t *indices, const int64_t *indptr, int64_t n, int64_t m,
                  int64_t nnz, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && indptr && (nnz == 0 || (data && indices)), XR_ERR_INVALID, "xr_csr_upload: NULL argument");
    XR_REQUIRE(n >= 0 && m >= 0 && nnz >= 0, XR_ERR_INVALID, "xr_csr_upload: negative sizes");
    XR_REQUIRE(n < ((int64_t)1 << 31) - 1 && m < ((int64_t)1 << 31) && nnz < ((int64_t)1 << 31), XR_ERR_LIMIT,
               "xr_csr_upload: matrix exceeds the int32 index range");
    XR_REQUIRE(indptr[0] == 0 && indptr[n] == nnz, XR_ERR_INVALID, "xr_csr_upload: indptr does not span [0, nnz]");
    for (int64_t i = 0; i < n; i++)
        XR_REQUIRE(indptr[i + 1] >= indptr[i], XR_ERR_INVALID,
                   "xr_csr_upload: indptr is not non-decreasing at row %lld", (long long)i);
    for (int64_t i = 0; i < nnz; i++)
        XR_REQUIRE(indices[i] >= 0 && indices[i] < m, XR_ERR_INVALID,
                   "xr_csr_upload: column index %lld outside [0,%lld)", (long long)indices[i], (long long)m);
    Building<xr_csr> csr;
    csr->n = n; csr->m = m; csr->nnz = nnz;
    csr->indptr.alloc((size_t)n + 1);
    csr->indices.alloc((size_t)nnz);
    csr->data.alloc((size_t)nnz);
    upload_narrow(indptr, n + 1, csr->indptr.get());
    upload_narrow(indices, nnz, csr->indices.get());
    h2d(csr->data.get(), data, sizeof(double) * (size_t)nnz);
    std::vector<int32_t> longs;
    for (int64_t i = 0; i < n; i++)
        if (indptr[i + 1] - indptr[i] > APPLY_LONG) longs.push_back((int32_t)i);
    set_long_rows(csr.get(), longs);
    stream_sync();
    *out = csr.release();
    XR_API_END
}

int xr_csr_from_triplet(const int64_t *row, const int64_t *col, const double *data, int64_t nnz, int64_t n,
                        int64_t m, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(out && (nnz == 0 || (row && col && data)), XR_ERR_INVALID, "xr_csr_from_triplet: NULL argument");
    XR_REQUIRE(n >= 0 && m >= 0 && nnz >= 0, XR_ERR_INVALID, "xr_csr_from_triplet: negative sizes");
    XR_REQUIRE(n < ((int64_t)1 << 31) - 1 && m < ((int64_t)1 << 31) && nnz < ((int64_t)1 << 31), XR_ERR_LIMIT,
               "xr_csr_from_triplet: matrix exceeds the int32 index range");
    for (int64_t i = 0; i < nnz; i++) {
        XR_REQUIRE(row[i] >= 0 && row[i] < n && col[i] >= 0 && col[i] < m, XR_ERR_INVALID,
                   "xr_csr_from_triplet: entry %lld outside the %lld x %lld matrix", (long long)i, (long long)n,
                   (long long)m);
        XR_REQUIRE(i == 0 || row[i] >= row[i - 1], XR_ERR_INVALID,
                   "xr_csr_from_triplet: rows must be sorted (core/sparse.py:65)");
    }
    Building<xr_csr> csr;
    csr->n = n; csr->m = m; csr->nnz = nnz;
    csr->indptr.alloc((size_t)n + 1);
    csr->indices.alloc((size_t)nnz);
    csr->data.alloc((size_t)nnz);
    DevBuf<int32_t> row32((size_t)nnz), count((size_t)(n > 0 ? n : 1));
    upload_narrow(row, nnz, row32.get());
    upload_narrow(col, nnz, csr->indices.get());
    h2d(csr->data.get(), data, sizeof(double) * (size_t)nnz);
    XR_HIP(hipMemsetAsync(count.get(), 0, sizeof(int32_t) * (size_t)(n > 0 ? n : 1), launch_stream()));
    if (nnz > 0) XR_LAUNCH("bincount", k_bincount, dim3(div_up(nnz, 256)), dim3(256), 0, row32.get(), nnz, count.get());
    exclusive_scan_i32(count.get(), csr->indptr.get(), n);
    std::vector<int32_t> longs;
    for (int64_t i = 0, j = 0; i < nnz; i = j) { // rows are sorted: run lengths
        while (j < nnz && row[j] == row[i]) j++;
        if (j - i > APPLY_LONG) longs.push_back((int32_t)row[i]);
    }
    set_long_rows(csr.get(), longs);
    stream_sync();
    *out = csr.release();
    XR_API_END
}

int xr_csr_set_row_keys(xr_csr *csr, const int64_t *keys, int64_t key_range) {
    XR_API_BEGIN
    XR_REQUIRE(csr && (keys || csr->n == 0), XR_ERR_INVALID, "xr_csr_set_row_keys: NULL argument");
    XR_REQUIRE(key_range >= 1 && key_range <= ((int64_t)1 << 24), XR_ERR_INVALID,
               "xr_csr_set_row_keys: key_range must be in [1, 2^24]");
    // With the output in stored order the stored order is part of what the caller has been told (xr_csr_row_order): new
    // keys would regroup the rows under every result that is read through the old permutation.
    XR_REQUIRE(!csr->stored.output_stored, XR_ERR_INVALID,
               "xr_csr_set_row_keys: the matrix delivers its output in stored order -- its row order is frozen; call "
               "xr_csr_output_stored_order(csr, 0) first, set the keys, switch it on again and re-read xr_csr_row_order");
    for (int64_t i = 0; i < csr->n; i++)
        XR_REQUIRE(keys[i] >= 0 && keys[i] < key_range, XR_ERR_INVALID, "xr_csr_set_row_keys: key %lld outside [0,%lld)",
                   (long long)keys[i], (long long)key_range);
    if (csr->n > 0) {
        csr->tiling.key.alloc((size_t)csr->n);
        if (csr->stored.has_row_order) {
            // rows already stored in another order (built by xr_overlap, or tiled before): the keys are per CALLER row, the
            // regrouping works on stored rows -- key of stored row r = keys[row_order[r]]; the permutations compose
            DevBuf<int32_t> by_caller((size_t)csr->n);
            upload_narrow(keys, csr->n, by_caller.get());
            XR_LAUNCH("gather_keys", k_gather_i32, dim3(div_up(csr->n, 256)), dim3(256), 0, by_caller.get(),
                      csr->stored.row_order.get(), csr->n, csr->tiling.key.get());
        } else {
            upload_narrow(keys, csr->n, csr->tiling.key.get());
        }
        stream_sync();
        csr->keys_changed();
        csr->tiling.key_range = key_range;
        csr->tiling.pending = key_range > 1;
    }
    XR_API_END
}

int xr_csr_set_col_keys(xr_csr *csr, const int64_t *keys, int64_t key_range) {
    XR_API_BEGIN
    XR_REQUIRE(csr && (keys || csr->m == 0), XR_ERR_INVALID, "xr_csr_set_col_keys: NULL argument");
    XR_REQUIRE(key_range >= 1 && key_range <= ((int64_t)1 << 24), XR_ERR_INVALID,
               "xr_csr_set_col_keys: key_range must be in [1, 2^24]");
    XR_REQUIRE(!csr->cols.permuted, XR_ERR_INVALID, "xr_csr_set_col_keys: the columns of this matrix are renumbered already");
    for (int64_t i = 0; i < csr->m; i++)
        XR_REQUIRE(keys[i] >= 0 && keys[i] < key_range, XR_ERR_INVALID, "xr_csr_set_col_keys: key %lld outside [0,%lld)",
                   (long long)keys[i], (long long)key_range);
    const int64_t m = csr->m;
    if (m > 0 && key_range > 1) {
        // stable counting sort of the columns by key (the tiling kernels of the rows): col_of[new] = caller's column
        DevBuf<int32_t> key((size_t)m), hist((size_t)key_range + 1), start((size_t)key_range + 1), members((size_t)m),
            rank((size_t)m);
        upload_narrow(keys, m, key.get());
        fill_i32(hist.get(), 0, key_range + 1);
        XR_LAUNCH("bincount", k_bincount, dim3(div_up(m, 256)), dim3(256), 0, key.get(), m, hist.get());
        exclusive_scan_i32(hist.get(), start.get(), key_range);
        fill_i32(hist.get(), 0, key_range + 1);
        XR_LAUNCH("tile_scatter", k_tile_scatter, dim3(div_up(m, 256)), dim3(256), 0, key.get(), m, start.get(), hist.get(),
                  members.get());
        csr->cols.col_of.alloc((size_t)m);
        XR_LAUNCH("tile_rank", k_tile_rank, dim3(div_up(m, 256)), dim3(256), 0, key.get(), start.get(), members.get(), m,
                  csr->cols.col_of.get());
        XR_LAUNCH("col_inverse", k_scatter_iota_i32, dim3(div_up(m, 256)), dim3(256), 0, csr->cols.col_of.get(), m, rank.get());
        if (csr->nnz > 0)
            XR_LAUNCH("col_relabel", k_relabel_i32, dim3(div_up(csr->nnz, 256)), dim3(256), 0, rank.get(),
                      csr->indices.get(), csr->nnz);
        stream_sync();
        csr->cols.permuted = true;
        csr->keys_changed();
    }
    XR_API_END
}

int xr_csr_col_order(const xr_csr *csr, int64_t *order_out) {
    XR_API_BEGIN
    XR_REQUIRE(csr && (order_out || csr->m == 0), XR_ERR_INVALID, "xr_csr_col_order: NULL argument");
    if (csr->cols.permuted) {
        DevBuf<int64_t> wide((size_t)csr->m);
        download_wide(csr->cols.col_of.get(), csr->m, order_out, wide);
        stream_sync();
    } else {
        for (int64_t i = 0; i < csr->m; i++) order_out[i] = i;
    }
    XR_API_END
}

int xr_csr_expect_permuted(xr_csr *csr, int permuted) {
    XR_API_BEGIN
    XR_REQUIRE(csr, XR_ERR_INVALID, "xr_csr_expect_permuted: NULL argument");
    csr->cols.source_permuted = permuted != 0;
    XR_API_END
}

int xr_csr_output_stored_order(xr_csr *csr, int stored) {
    XR_API_BEGIN
    XR_REQUIRE(csr, XR_ERR_INVALID, "xr_csr_output_stored_order: NULL argument");
    if (stored) settle_row_layout(csr); // from here on the order is frozen (xr_csr_set_row_keys refuses)
    csr->stored.output_stored = stored != 0;
    XR_API_END
}

int xr_csr_row_order(const xr_csr *csr, int64_t K_hint, int64_t *order_out) {
    XR_API_BEGIN
    (void)K_hint; // (kept in the signature; the layout is settled whatever K is)
    XR_REQUIRE(csr && (order_out || csr->n == 0), XR_ERR_INVALID, "xr_csr_row_order: NULL argument");
    settle_row_layout(csr);
    if (csr->stored.has_row_order) {
        DevBuf<int64_t> wide((size_t)csr->n);
        download_wide(csr->stored.row_order.get(), csr->n, order_out, wide);
        stream_sync();
    } else {
        for (int64_t i = 0; i < csr->n; i++) order_out[i] = i;
    }
    XR_API_END
}

int xr_csr_long_rows(const xr_csr *csr, int64_t capacity, int64_t *rows_out, int64_t *n_out) {
    XR_API_BEGIN
    XR_REQUIRE(csr && n_out && (rows_out || capacity == 0) && capacity >= 0, XR_ERR_INVALID, "xr_csr_long_rows: invalid argument");
    stream_sync();
    const int64_t n = csr->longs.n_dev.get() ? read_scalar(csr->longs.n_dev.get()) : 0;
    *n_out = n;
    const int64_t take = n < capacity ? n : capacity;
    if (take > 0) {
        DevBuf<int64_t> wide((size_t)take);
        download_wide(csr->longs.rows.get(), take, rows_out, wide);
        stream_sync();
    }
    XR_API_END
}

int xr_csr_destroy(xr_csr *csr) {
    XR_API_BEGIN
    if (csr) {
        release_point();
        delete csr;
    }
    XR_API_END
}

} // extern "C"
