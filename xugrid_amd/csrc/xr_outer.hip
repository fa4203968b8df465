// xr_outer.hip -- separable (rectilinear) weights: the two per-axis sparse matrices of a raster pair (xr_outer), their
// matrix-free apply, and the CSR of their outer product for whoever needs the entries side by side
// (xugrid/regrid/structured.py:503-601).
#include <memory>
#include <vector>

#include "xr_apply.h"
#include "xr_reduce.h"

namespace xr {

// ---- matrix-free apply of separable weights: one thread per target cell walks the c_y x c_x entries of its row
// (y-major, x-minor = the order of the materialised CSR row and of the reference's loop) and forms each weight
// w_y * w_x on the fly.  Neighbouring threads are neighbouring x-targets, whose x-lists are adjacent source columns:
// the gathers are coalesced whatever the coarsening ratio, so even rows of thousands of entries are reduced
// sequentially -- bit-identical to the reference order -- and the P entries of the product are never stored or read.
template <int METHOD, typename SRC, int KTILE, int CX>
__global__ void __launch_bounds__(AP_BLOCK)
k_apply_outer(const int32_t *__restrict__ ipy, const int32_t *__restrict__ sy, const double *__restrict__ wy,
              const int32_t *__restrict__ ipx, const int32_t *__restrict__ sx, const double *__restrict__ wx, int64_t nty,
              int64_t ntx, int64_t nsx, int64_t S, int rows_per_block, const SRC *__restrict__ source, int64_t K,
              double *__restrict__ out) {
    // blockIdx.x: 256 adjacent x-targets; blockIdx.y: a run of target rows (everything about a y-list is wave-uniform,
    // i.e. scalar loads); blockIdx.z: tile of KTILE source variables.  CX > 0: every x-list has at most CX entries
    // and lives in registers for all rows of the run; the CX x KTILE gathers of one source row are then independent
    // loads issued back to back (lanes past the end of their list re-read their last column and discard it).
    const int64_t it = (int64_t)blockIdx.x * AP_BLOCK + threadIdx.x;
    if (it >= ntx) return;
    const int64_t T = nty * ntx;
    const int x0 = ipx[it], x1 = ipx[it + 1];
    const int nx = x1 - x0;
    constexpr int CXR = CX > 0 ? CX : 1;
    int sxr[CXR];
    double wxr[CXR];
    if (CX > 0) {
#pragma unroll
        for (int c = 0; c < CXR; c++) {
            const int b = c < nx ? x0 + c : (nx > 0 ? x1 - 1 : 0);
            sxr[c] = nx > 0 ? sx[b] : 0;
            wxr[c] = nx > 0 ? wx[b] : 0.0;
        }
    }
    const int64_t k0 = (int64_t)blockIdx.z * KTILE;
    const int kn = (int)((K - k0) < KTILE ? (K - k0) : KTILE);
    const SRC *src = source + k0 * S;
    const int64_t j0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t j1 = (j0 + rows_per_block) < nty ? (j0 + rows_per_block) : nty;
    for (int64_t jt = j0; jt < j1; jt++) {
        const int y0 = ipy[jt], y1 = ipy[jt + 1];
        double normsum = 0.0;
        if (METHOD == XR_GEOMETRIC_MEAN)
            for (int a = y0; a < y1; a++)
                for (int b = x0; b < x1; b++) normsum += wy[a] * wx[b];
        Red<METHOD> red[KTILE];
        for (int a = y0; a < y1; a++) {
            const int64_t rowbase = (int64_t)sy[a] * nsx;
            const double wa = wy[a];
            if (CX > 0) {
                double v[CXR][KTILE];
#pragma unroll
                for (int c = 0; c < CXR; c++)
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++)
                        v[c][kk] = ld_src(src, (int64_t)(kk < kn ? kk : 0) * S + rowbase + sxr[c]);
#pragma unroll
                for (int c = 0; c < CXR; c++) {
                    if (c < nx) {
                        const double w = wa * wxr[c];
#pragma unroll
                        for (int kk = 0; kk < KTILE; kk++) red[kk].add(v[c][kk], w, normsum);
                    }
                }
            } else {
                for (int b = x0; b < x1; b++) {
                    const int64_t col = rowbase + sx[b];
                    const double w = wa * wx[b];
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++)
                        if (kk < kn) red[kk].add(ld_src(src, (int64_t)kk * S + col), w, normsum);
                }
            }
        }
        const bool empty = y1 == y0 || nx == 0;
        const int64_t t = jt * ntx + it;
#pragma unroll
        for (int kk = 0; kk < KTILE; kk++) {
            if (kk < kn) {
                double r = NAN;
                if (!empty) {
                    r = red[kk].fin();
                    if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) r = NAN;
                }
                out[(k0 + kk) * T + t] = r;
            }
        }
    }
}

template <int METHOD, typename SRC, int KT, int CX>
static void launch_outer_kt(const xr_outer *o, const SRC *src, int64_t K, double *out) {
    const int rpb = (int)std::max<int64_t>(4, div_up(o->nty, 65535));
    const dim3 grid((unsigned)div_up(o->ntx, AP_BLOCK), (unsigned)div_up(o->nty, rpb), (unsigned)div_up(K, KT));
    XR_LAUNCH("apply_outer", (k_apply_outer<METHOD, SRC, KT, CX>), grid, dim3(AP_BLOCK), 0, o->ipy.get(), o->sy.get(),
              o->wy.get(), o->ipx.get(), o->sx.get(), o->wx.get(), o->nty, o->ntx, o->nsx, o->nsy * o->nsx, rpb, src, K,
              out);
}

template <int METHOD, typename SRC, int KT>
static void launch_outer_cx(const xr_outer *o, const SRC *src, int64_t K, double *out) {
    if (o->max_cx <= 2) launch_outer_kt<METHOD, SRC, KT, 2>(o, src, K, out);
    else if (o->max_cx <= 4) launch_outer_kt<METHOD, SRC, KT, 4>(o, src, K, out);
    else launch_outer_kt<METHOD, SRC, KT, 0>(o, src, K, out);
}

template <int METHOD, typename SRC>
static void launch_outer(const xr_outer *o, const SRC *src, int64_t K, double *out) {
    if (o->nty * o->ntx == 0 || K == 0) return;
    if (o->Py == 0 || o->Px == 0) { // no entries at all (e.g. an empty source grid): every row is empty
        fill_f64(out, NAN, K * o->nty * o->ntx);
        return;
    }
    XR_REQUIRE(div_up(K, 4) <= 65535, XR_ERR_LIMIT, "apply: too many source variables in one call (%lld)", (long long)K);
    if (K == 1) launch_outer_cx<METHOD, SRC, 1>(o, src, K, out);
    else if (K == 2) launch_outer_cx<METHOD, SRC, 2>(o, src, K, out);
    else launch_outer_cx<METHOD, SRC, 4>(o, src, K, out);
}

// ---- separable (rectilinear) weights: CSR of the outer product of two per-axis sparse matrices.
// Row (jt, it) of the product holds cy(jt) * cx(it) entries, y-major / x-minor, i.e. ascending in the
// column id sy * n_source_x + sx when both axis rows are ascending.  The entries of one jt form a
// contiguous slab of cy * Px entries (Px = nnz of the x axis) that starts at indptr_y[jt] * Px, and
// entry e of the slab belongs to the x-target that owns x-entry floor(e / cy): offsets have a closed
// form, so there is no sort and no scan (the reference argsorts the broadcast triplets,
// xugrid/regrid/structured.py:527).
__global__ __launch_bounds__(256) void
k_outer_indptr(const int32_t *__restrict__ ipy, const int32_t *__restrict__ ipx, int64_t nty, int64_t ntx, int64_t Px,
               int64_t nnz, int32_t *__restrict__ indptr, int32_t *__restrict__ long_rows,
               int32_t *__restrict__ n_long) {
    const int64_t T = nty * ntx;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) indptr[T] = (int32_t)nnz;
    if (t >= T) return;
    const int64_t jt = t / ntx, it = t - jt * ntx;
    const int64_t cy = ipy[jt + 1] - ipy[jt], cx = ipx[it + 1] - ipx[it];
    indptr[t] = (int32_t)((int64_t)ipy[jt] * Px + cy * ipx[it]);
    if (cy * cx > XR_APPLY_LONG_ROW) long_rows[atomicAdd(n_long, 1)] = (int32_t)t;
}

__global__ __launch_bounds__(256) void
k_outer_fill(const int32_t *__restrict__ ipy, const int32_t *__restrict__ sy, const double *__restrict__ wy,
             const int32_t *__restrict__ ipx, const int32_t *__restrict__ sx, const double *__restrict__ wx,
             const int32_t *__restrict__ tx_of_entry, int64_t nty, int64_t nsx, int64_t Px,
             int32_t *__restrict__ indices, double *__restrict__ data) {
    for (int64_t jt = blockIdx.y; jt < nty; jt += gridDim.y) {
        const int y0 = ipy[jt], cy = ipy[jt + 1] - y0;
        if (cy == 0) continue;
        const int64_t slab = (int64_t)y0 * Px, n = (int64_t)cy * Px;
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
            const int it = tx_of_entry[e / cy];
            const int x0 = ipx[it], cx = ipx[it + 1] - x0;
            const int r = (int)(e - (int64_t)cy * x0);
            const int a = r / cx, b = r - a * cx;
            indices[slab + e] = (int32_t)((int64_t)sy[y0 + a] * nsx + sx[x0 + b]);
            data[slab + e] = wy[y0 + a] * wx[x0 + b];
        }
    }
}

} // namespace xr

using namespace xr;

static void check_axis(const char *name, const int64_t *indptr, const int64_t *source, const double *weight,
                       int64_t n_target, int64_t n_source) {
    XR_REQUIRE(indptr, XR_ERR_INVALID, "xr_csr_from_outer: NULL indptr (%s axis)", name);
    XR_REQUIRE(n_target >= 0 && n_source >= 0, XR_ERR_INVALID, "xr_csr_from_outer: negative size (%s axis)", name);
    XR_REQUIRE(indptr[0] == 0, XR_ERR_INVALID, "xr_csr_from_outer: indptr[0] != 0 (%s axis)", name);
    for (int64_t i = 0; i < n_target; i++)
        XR_REQUIRE(indptr[i + 1] >= indptr[i], XR_ERR_INVALID, "xr_csr_from_outer: indptr decreases at %lld (%s axis)",
                   (long long)i, name);
    const int64_t nnz = indptr[n_target];
    XR_REQUIRE(nnz == 0 || (source && weight), XR_ERR_INVALID, "xr_csr_from_outer: NULL entries (%s axis)", name);
    for (int64_t i = 0; i < nnz; i++)
        XR_REQUIRE(source[i] >= 0 && source[i] < n_source, XR_ERR_INVALID,
                   "xr_csr_from_outer: source index %lld outside [0,%lld) (%s axis)", (long long)source[i],
                   (long long)n_source, name);
}

static xr_outer *outer_create(const int64_t *indptr_y, const int64_t *source_y, const double *weight_y, int64_t n_target_y,
                              int64_t n_source_y, const int64_t *indptr_x, const int64_t *source_x, const double *weight_x,
                              int64_t n_target_x, int64_t n_source_x) {
    check_axis("y", indptr_y, source_y, weight_y, n_target_y, n_source_y);
    check_axis("x", indptr_x, source_x, weight_x, n_target_x, n_source_x);
    const int64_t Py = indptr_y[n_target_y], Px = indptr_x[n_target_x];
    const int64_t lim = ((int64_t)1 << 31) - 1;
    XR_REQUIRE(n_target_y == 0 || n_target_x < lim / n_target_y, XR_ERR_LIMIT,
               "separable weights: target grid exceeds the int32 index range");
    XR_REQUIRE(n_source_y == 0 || n_source_x <= lim / n_source_y, XR_ERR_LIMIT,
               "separable weights: source grid exceeds the int32 index range");
    Building<xr_outer> o;
    o->nty = n_target_y; o->nsy = n_source_y; o->ntx = n_target_x; o->nsx = n_source_x; o->Py = Py; o->Px = Px;
    o->ipy.alloc((size_t)n_target_y + 1); o->ipx.alloc((size_t)n_target_x + 1);
    o->sy.alloc((size_t)Py); o->sx.alloc((size_t)Px); o->tx.alloc((size_t)Px);
    o->wy.alloc((size_t)Py); o->wx.alloc((size_t)Px);
    upload_narrow(indptr_y, n_target_y + 1, o->ipy.get());
    upload_narrow(indptr_x, n_target_x + 1, o->ipx.get());
    upload_narrow(source_y, Py, o->sy.get());
    upload_narrow(source_x, Px, o->sx.get());
    h2d(o->wy.get(), weight_y, sizeof(double) * (size_t)Py);
    h2d(o->wx.get(), weight_x, sizeof(double) * (size_t)Px);
    std::vector<int32_t> owner((size_t)Px);
    for (int64_t it = 0; it < n_target_x; it++)
        for (int64_t q = indptr_x[it]; q < indptr_x[it + 1]; q++) owner[(size_t)q] = (int32_t)it;
    h2d(o->tx.get(), owner.data(), sizeof(int32_t) * (size_t)Px);
    for (int64_t j = 0; j < n_target_y; j++) o->max_cy = std::max(o->max_cy, indptr_y[j + 1] - indptr_y[j]);
    for (int64_t i = 0; i < n_target_x; i++) o->max_cx = std::max(o->max_cx, indptr_x[i + 1] - indptr_x[i]);
    stream_sync();
    return o.release();
}

// the CSR of the outer product, assembled on the device (closed-form offsets: no sort, no scan)
static xr_csr *outer_materialise(const xr_outer *o) {
    const int64_t lim = ((int64_t)1 << 31) - 1;
    XR_REQUIRE(o->Py == 0 || o->Px < lim / o->Py, XR_ERR_LIMIT, "separable weights: %lld x %lld entries exceed the int32 range",
               (long long)o->Py, (long long)o->Px);
    const int64_t n = o->nty * o->ntx, m = o->nsy * o->nsx, nnz = o->Py * o->Px;
    Building<xr_csr> csr;
    csr->n = n; csr->m = m; csr->nnz = nnz;
    csr->indptr.alloc((size_t)n + 1);
    csr->indices.alloc((size_t)nnz);
    csr->data.alloc((size_t)nnz);
    csr->longs.begin((size_t)(nnz / XR_APPLY_LONG_ROW + 1));
    XR_LAUNCH("outer_indptr", k_outer_indptr, dim3(div_up(n + 1, 256)), dim3(256), 0, o->ipy.get(), o->ipx.get(), o->nty,
              o->ntx, o->Px, nnz, csr->indptr.get(), csr->longs.rows.get(), csr->longs.n_dev.get());
    if (nnz > 0) {
        const int64_t gx = std::min<int64_t>(div_up(o->max_cy * o->Px, 256), 1 << 16);
        const int64_t gy = std::min<int64_t>(o->nty, 32768);
        XR_LAUNCH("outer_fill", k_outer_fill, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, o->ipy.get(), o->sy.get(),
                  o->wy.get(), o->ipx.get(), o->sx.get(), o->wx.get(), o->tx.get(), o->nty, o->nsx, o->Px,
                  csr->indices.get(), csr->data.get());
    }
    csr->longs.end();
    return csr.release();
}

// x-lists of at most 4 entries (similar resolutions, refinement, any coarsening along y only): matrix-free.  Longer
// x-lists make neighbouring lanes gather columns that lie a whole list apart; there the stored product with its
// cooperative long-row kernels is the faster engine (and the only one for mode / percentiles, which need a row's
// values side by side).  Products too large to store (>= 2^31 entries) stay matrix-free.
static bool outer_matrix_free(const xr_outer *o) {
    const int64_t force = option(OPT_OUTER_APPLY); // test hook: 1 "free" | 2 "csr"
    const bool fits = o->Py == 0 || o->Px < (((int64_t)1 << 31) - 1) / o->Py;
    if (!fits) return true;
    if (force == 1) return true;
    if (force == 2) return false;
    return o->max_cx <= 4;
}

static void apply_outer_dev(xr_outer *o, int method, double p, const void *src, int dtype, int64_t K, double *out) {
    with_source_type(dtype, [&](auto tag) {
        using SRC = decltype(tag);
        with_reducer(method, [&](auto m) {
            constexpr int METHOD = decltype(m)::value;
            if constexpr (streamed_reducer<METHOD>) {
                if (outer_matrix_free(o)) {
                    launch_outer<METHOD, SRC>(o, static_cast<const SRC *>(src), K, out);
                    return;
                }
            }
            if (!o->csr) o->csr = outer_materialise(o);
            csr_apply_dev(o->csr, METHOD, p, src, dtype, K, out);
        });
    });
}

extern "C" {

int xr_csr_from_outer(const int64_t *indptr_y, const int64_t *source_y, const double *weight_y, int64_t n_target_y,
                      int64_t n_source_y, const int64_t *indptr_x, const int64_t *source_x, const double *weight_x,
                      int64_t n_target_x, int64_t n_source_x, xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(out, XR_ERR_INVALID, "xr_csr_from_outer: NULL argument");
    const std::unique_ptr<xr_outer> o(outer_create(indptr_y, source_y, weight_y, n_target_y, n_source_y, indptr_x, source_x,
                                                   weight_x, n_target_x, n_source_x));
    *out = outer_materialise(o.get());
    XR_API_END
}

int xr_outer_create(const int64_t *indptr_y, const int64_t *source_y, const double *weight_y, int64_t n_target_y,
                    int64_t n_source_y, const int64_t *indptr_x, const int64_t *source_x, const double *weight_x,
                    int64_t n_target_x, int64_t n_source_x, xr_outer **out) {
    XR_API_BEGIN
    XR_REQUIRE(out, XR_ERR_INVALID, "xr_outer_create: NULL argument");
    *out = outer_create(indptr_y, source_y, weight_y, n_target_y, n_source_y, indptr_x, source_x, weight_x, n_target_x,
                        n_source_x);
    XR_API_END
}

int xr_outer_info(const xr_outer *o, int64_t *n, int64_t *m, int64_t *nnz) {
    XR_API_BEGIN
    XR_REQUIRE(o, XR_ERR_INVALID, "xr_outer_info: NULL handle");
    if (n) *n = o->nty * o->ntx;
    if (m) *m = o->nsy * o->nsx;
    if (nnz) *nnz = o->Py * o->Px;
    XR_API_END
}

int xr_outer_csr(xr_outer *o, const xr_csr **out) {
    XR_API_BEGIN
    XR_REQUIRE(o && out, XR_ERR_INVALID, "xr_outer_csr: NULL argument");
    if (!o->csr) o->csr = outer_materialise(o);
    *out = o->csr;
    XR_API_END
}

int xr_outer_destroy(xr_outer *o) {
    XR_API_BEGIN
    if (o) {
        stream_sync();
        delete o;
    }
    XR_API_END
}

int xr_apply_outer_dev(xr_outer *o, int method, double percentile, const void *source_dev, int source_dtype, int64_t K,
                       double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(o && (source_dev || K == 0) && (out_dev || K == 0), XR_ERR_INVALID, "xr_apply_outer_dev: NULL argument");
    XR_REQUIRE(K >= 0, XR_ERR_INVALID, "xr_apply_outer_dev: negative K");
    apply_outer_dev(o, method, percentile, source_dev, source_dtype, K, out_dev);
    dev_call_done();
    XR_API_END
}

// the adjoint of the apply (xr_adjoint.hip) needs the entries of a column side by side: through the materialised CSR
int xr_apply_outer_adjoint_dev(xr_outer *o, int method, const void *source_dev, int source_dtype, const double *grad_dev,
                               int64_t K, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(o && K >= 0 && ((grad_dev && out_dev) || K == 0), XR_ERR_INVALID, "xr_apply_outer_adjoint_dev: invalid argument");
    if (const int rc = prepare_for_adjoint(o->csr, method)) return rc; // (the reducer is checked before anything is built)
    if (!o->csr) o->csr = outer_materialise(o);
    ensure_transposed(o->csr);
    csr_adjoint_dev(o->csr, method, source_dev, source_dtype, grad_dev, K, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_apply_outer(xr_outer *o, int method, double percentile, const void *source, int source_dtype, int64_t K, double *out) {
    XR_API_BEGIN
    XR_REQUIRE(o && (source || K == 0) && (out || K == 0), XR_ERR_INVALID, "xr_apply_outer: NULL argument");
    XR_REQUIRE(K >= 0, XR_ERR_INVALID, "xr_apply_outer: negative K");
    const size_t esz = source_size(source_dtype);
    const int64_t n = o->nty * o->ntx, m = o->nsy * o->nsx;
    staged_chunks(K, m, esz, n, [&](int64_t k0, int64_t kc, char *src, double *dst) {
        h2d(src, static_cast<const char *>(source) + (size_t)k0 * (size_t)m * esz, (size_t)kc * (size_t)m * esz);
        apply_outer_dev(o, method, percentile, src, source_dtype, kc, dst);
        d2h(out + (size_t)k0 * (size_t)n, dst, (size_t)kc * (size_t)n * sizeof(double));
    });
    XR_API_END
}

} // extern "C"
