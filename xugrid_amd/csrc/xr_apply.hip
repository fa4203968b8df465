// xr_apply.hip -- the sparse weight x data apply: its entry points and the dispatch to the three pipelines.
//
// Replaces make_regrid(func)._regrid (xugrid/regrid/regridder.py:41-67) with one kernel
// specialisation per reducer of xugrid/regrid/reduce.py, and CentroidLocatorRegridder._regrid
// (regridder.py:400-409).  The pipelines are units of their own: the streamed reducers in xr_apply_stream.hip, the
// many-variable plan in xr_apply_plan.hip, mode and percentiles in xr_apply_workspace.hip.  The reducers themselves are in
// xr_reduce.h; the MatrixCSR handle with its row tiling is in xr_csr.hip, the partial states of the source-sharded apply in
// xr_partial.hip, the separable weights in xr_outer.hip; what these units share is in xr_apply.h.
//
// Reducer semantics are those of reduce.py line by line; entries of a
// row are consumed in CSR order by one thread per (row, k-tile), so that results are
// bit-identical to the reference loop on the same CSR (except exp/log in geometric_mean).
//
// HBM layout: source (K, S) row-major, out (K, T) row-major (regridder.py:163, :44);
// CSR = indptr i32[T+1], indices i32[nnz], data f64[nnz].
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xr_apply.h"
#include "xr_reduce.h"
#include "xr_prims.h"

namespace xr {

template <typename SRC>
__global__ void k_apply_coo(const int32_t *__restrict__ row, const int32_t *__restrict__ col, int64_t nnz, int64_t T,
                            int64_t S, const SRC *__restrict__ source, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int64_t k = blockIdx.y;
    out[k * T + row[i]] = ld_src(source + k * S, col[i]);
}

static void apply_dispatch(const xr_csr *csr, int method, double p, const void *src, int dtype, int64_t K, double *out,
                           const ApplyContext *ctx) {
    if (csr->n == 0 || K == 0) return;
    // (Until round 4 many variables were walked in host-side groups of 128; since round 5 the many-variable kernel orders its
    // own work by groups of 64 variables -- k_apply_plan, L2-blocked order.)
    with_reducer(method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        if constexpr (streamed_reducer<METHOD>) {
            apply_stream(csr, METHOD, src, dtype, K, out, ctx);
        } else {
            XR_REQUIRE(!ctx, XR_ERR_INVALID, "internal: a gated apply is a streaming reducer");
            if (METHOD == XR_PERCENTILE)
                XR_REQUIRE(p >= 0.0 && p <= 100.0, XR_ERR_INVALID,
                           "percentile must be in the range [0, 100], received: %g", p);
            apply_workspace(csr, METHOD, p, src, dtype, K, out);
        }
    });
}

static void apply_dev(const xr_csr *csr, int method, double p, const void *src, int dtype, int64_t K, double *out,
                      const ApplyContext *ctx = nullptr) {
    with_source_type(dtype, [&](auto tag) {
        using SRC = decltype(tag);
        DevBuf<char> permuted; // (goes back to the pool at return; the pool hands blocks out in stream order)
        apply_dispatch(csr, method, p, stored_source(csr, static_cast<const SRC *>(src), K, permuted), dtype, K, out, ctx);
    });
}

void csr_apply_dev(const xr_csr *csr, int method, double percentile, const void *src_dev, int dtype, int64_t K, double *out_dev,
                   const ApplyContext *ctx) {
    apply_dev(csr, method, percentile, src_dev, dtype, K, out_dev, ctx);
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_apply_csr_dev(const xr_csr *csr, int method, double percentile, const void *source_dev, int source_dtype,
                     int64_t K, double *out_dev) {
    {
        const int rc = prepare_for_apply(csr, K);
        if (rc != XR_OK) return rc;
    }
    XR_API_BEGIN_SHARED
    XR_REQUIRE(csr && (source_dev || csr->m == 0 || K == 0) && (out_dev || csr->n == 0 || K == 0), XR_ERR_INVALID,
               "xr_apply_csr_dev: NULL argument");
    XR_REQUIRE(K >= 0, XR_ERR_INVALID, "xr_apply_csr_dev: negative K");
    apply_dev(csr, method, percentile, source_dev, source_dtype, K, out_dev);
    dev_call_done();
    XR_API_END
}

int xr_apply_csr(const xr_csr *csr, int method, double percentile, const void *source, int source_dtype, int64_t K,
                 double *out) {
    {
        const int rc = prepare_for_apply(csr, K);
        if (rc != XR_OK) return rc;
    }
    XR_API_BEGIN_SHARED
    XR_REQUIRE(csr && (source || csr->m == 0 || K == 0) && (out || csr->n == 0 || K == 0), XR_ERR_INVALID,
               "xr_apply_csr: NULL argument");
    XR_REQUIRE(K >= 0, XR_ERR_INVALID, "xr_apply_csr: negative K");
    const size_t esz = source_size(source_dtype);
    staged_chunks(K, csr->m, esz, csr->n, [&](int64_t k0, int64_t kc, char *src, double *dst) {
        const size_t n_src = (size_t)kc * (size_t)csr->m, n_out = (size_t)kc * (size_t)csr->n;
        h2d_big(src, static_cast<const char *>(source) + (size_t)k0 * (size_t)csr->m * esz, n_src * esz);
        apply_dev(csr, method, percentile, src, source_dtype, kc, dst);
        if (n_out > 0) d2h_big(out + (size_t)k0 * (size_t)csr->n, dst, n_out * sizeof(double));
    });
    XR_API_END
}

int xr_apply_coo(const int64_t *row, const int64_t *col, int64_t nnz, int64_t T, const void *source, int source_dtype,
                 int64_t K, int64_t S, double *out) {
    XR_API_BEGIN
    XR_REQUIRE(nnz >= 0 && T >= 0 && K >= 0 && S >= 0, XR_ERR_INVALID, "xr_apply_coo: negative sizes");
    const size_t esz = source_size(source_dtype);
    XR_REQUIRE(T < ((int64_t)1 << 31) && S < ((int64_t)1 << 31) && K < 65536, XR_ERR_LIMIT, "xr_apply_coo: too large");
    for (int64_t i = 0; i < nnz; i++)
        XR_REQUIRE(row[i] >= 0 && row[i] < T && col[i] >= 0 && col[i] < S, XR_ERR_INVALID,
                   "xr_apply_coo: entry %lld out of range", (long long)i);
    const size_t n_src = (size_t)K * (size_t)S, n_out = (size_t)K * (size_t)T;
    DevBuf<char> src(n_src * esz);
    DevBuf<double> dst(n_out);
    DevBuf<int32_t> r32((size_t)nnz), c32((size_t)nnz);
    h2d(src.get(), source, n_src * esz);
    upload_narrow(row, nnz, r32.get());
    upload_narrow(col, nnz, c32.get());
    fill_f64(dst.get(), NAN, (int64_t)n_out);
    if (nnz > 0 && K > 0) {
        dim3 grid(div_up(nnz, 256), (unsigned)K);
        with_source_type(source_dtype, [&](auto tag) {
            using SRC = decltype(tag);
            XR_LAUNCH("apply_coo", k_apply_coo<SRC>, grid, dim3(256), 0, r32.get(), c32.get(), nnz, T, S,
                      reinterpret_cast<const SRC *>(src.get()), dst.get());
        });
    }
    if (n_out > 0) {
        XR_HIP(hipMemcpyAsync(out, dst.get(), n_out * sizeof(double), hipMemcpyDeviceToHost, launch_stream()));
    }
    stream_sync();
    XR_API_END
}

} // extern "C"
