// xr_fill.hip -- filling the NaN entries of mesh data on the device: the Laplace fill of
// xugrid/ugrid/interpolate.py:207-330 (UgridDataArrayAccessor.laplace_interpolate) and the nearest fill of
// UgridDataArrayAccessor.interpolate_na (method "nearest").
//
// Laplace: a symmetric adjacency (xr_graph: CSR, optional weights, connected-component labels) and a batched masked
// conjugate gradient.  Slice k of the K data slices has its own unknown set U_k (NaN entries of components that hold at
// least one value); the system is the reference's diagonally scaled one, A = S L[U,U] S, b = S (-L[U,K] data[K]) with
// S = diag(1/sqrt(D)), solved by plain CG (no ILU0: DESIGN section 7) with scipy's stopping rule.  All K slices iterate
// together, four launches per iteration (spmv + p.q partials, alpha, update + r.r partials, beta / stopping rule); every
// dot product is a block partial combined in a fixed order, so results are bit-identical run to run and independent of K.
// A slice that stops freezes; the host enqueues chunks of iterations and reads the K active words once per chunk.
//
// Nearest: the null points of a slice are looked up in an xr_nn index of its valid points (xr_nn.h: exact f64 squared
// distances, lowest index among equidistant candidates).  Slices with the same NaN mask as slice 0 share one search.
#include <algorithm>
#include <cmath>
#include <vector>

#include "xr_nn.h"
#include "xr_objects.h"
#include "xr_prims.h"
#include "xr_topology.h"

namespace xr {

enum FillStatus : int { FILL_CONVERGED = 0, FILL_MAXITER = 1, FILL_BREAKDOWN = 2, FILL_NODATA = 3 };

static constexpr int FB = 256; // threads per block of the row kernels (one row per thread)

// Every sum over rows here is the fixed-order block reduction of xr_prims.h (wave64 butterfly, then the four wave sums in wave
// order), and every sum over blocks its fold of the partials.

// ---------------------------------------------------------------------------------------------
// graph construction
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FB) k_label_init(int32_t *__restrict__ lab, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i < n) lab[i] = (int32_t)i;
}

// one round of minimum-label propagation over the rows, then a pointer jump.  Labels only decrease and every label is a
// node id of the same component, so the fixed point -- the smallest id of each component -- does not depend on the order
// in which lanes see each other's stores.  `changed` is written with a plain store (any lane that lowers a label).
__global__ void __launch_bounds__(FB)
k_label_round(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n, int32_t *lab,
              int32_t *__restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= n) return;
    int32_t m = lab[i];
    for (int e = indptr[i]; e < indptr[i + 1]; e++) m = min(m, lab[indices[e]]);
    m = min(m, lab[m]);
    if (m < lab[i]) {
        lab[i] = m;
        *changed = 1;
    }
}

// ---------------------------------------------------------------------------------------------
// Laplace fill: set-up
// ---------------------------------------------------------------------------------------------
// comp_valid[k, label] = 1 for every component of slice k that holds a value; has_valid / has_null per slice
__global__ void __launch_bounds__(FB)
k_fill_mark(const double *__restrict__ in, const int32_t *__restrict__ lab, int64_t n, uint8_t *__restrict__ comp_valid,
            uint8_t *__restrict__ has_valid, uint8_t *__restrict__ has_null) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    const int64_t k = blockIdx.y;
    if (i >= n) return;
    const double v = in[k * n + i];
    if (v == v) {
        comp_valid[k * n + lab[i]] = 1;
        has_valid[k] = 1;
    } else {
        has_null[k] = 1;
    }
}

// out = in; unknown flag; scale s = 1/sqrt(D); b = s * sum_{j known} w_ij in_j; x = 0, r = b, p = 0; partial b.b
__global__ void __launch_bounds__(FB)
k_fill_setup(const double *__restrict__ in, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
             const double *__restrict__ data, int use_weights, const int32_t *__restrict__ lab,
             const uint8_t *__restrict__ comp_valid, int64_t n, double *__restrict__ out, uint8_t *__restrict__ unknown,
             double *__restrict__ scale, double *__restrict__ x, double *__restrict__ r, double *__restrict__ p0,
             double *__restrict__ p1, double *__restrict__ partial) {
    __shared__ double sh[FB / 64];
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    const int64_t k = blockIdx.y;
    double bb = 0.0;
    if (i < n) {
        const int64_t o = k * n + i;
        const double v = in[o];
        out[o] = v;
        const bool u = v != v && comp_valid[k * n + lab[i]];
        unknown[o] = u;
        double b = 0.0, s = 0.0;
        if (u) {
            double D = 0.0;
            for (int e = indptr[i]; e < indptr[i + 1]; e++) {
                const double w = use_weights ? data[e] : 1.0;
                D += w;
                const double dj = in[k * n + indices[e]];
                if (dj == dj) b += w * dj;
            }
            s = D > 0.0 ? 1.0 / sqrt(D) : 1.0; // (an unknown row always has a neighbour: its component holds a value)
            b *= s;
        }
        scale[o] = s;
        x[o] = 0.0;
        r[o] = b;
        p0[o] = 0.0;
        p1[o] = 0.0;
        bb = b * b;
    }
    block_reduce_all<FB, OpSum>(sh, bb);
    if (threadIdx.x == 0) partial[k * gridDim.x + blockIdx.x] = bb;
}

// per-slice state, one record per slice
struct CgState {
    double rho, alpha, beta, tol;
    int64_t iter;
    int32_t active, status;
};

// the nb block partials of a slice in the fixed order of block_fold_partials (xr_prims.h), in every thread
__device__ __forceinline__ double slice_total(const double *__restrict__ part, int nb, double *sh) {
    double t[1];
    block_fold_partials<true, FB, OpSum>(sh, part, nb, t);
    return t[0];
}

// one block per slice: the scipy 1.15 `cg` prologue (bnrm2, atol = max(atol, rtol * bnrm2), bnrm2 == 0 -> x = 0)
__global__ void __launch_bounds__(FB)
k_cg_start(const double *__restrict__ partial, int nb, const uint8_t *__restrict__ has_valid,
           const uint8_t *__restrict__ has_null, double atol, double rtol, int64_t maxiter, CgState *__restrict__ st,
           int32_t *__restrict__ active_out) {
    __shared__ double sh[FB / 64];
    const int64_t k = blockIdx.x;
    const double rr = slice_total(partial + k * nb, nb, sh);
    if (threadIdx.x) return;
    CgState s{};
    s.rho = rr;
    s.tol = fmax(atol, rtol * sqrt(rr));
    s.iter = 0;
    s.active = 0;
    s.status = FILL_CONVERGED;
    if (!has_valid[k]) s.status = FILL_NODATA;
    else if (!has_null[k] || rr == 0.0 || maxiter <= 0) s.status = FILL_CONVERGED;
    else if (!(sqrt(rr) < s.tol)) s.active = 1;
    st[k] = s;
    active_out[k] = s.active;
}

// q = A p_new with p_new = r + beta p_old computed on the fly for every gathered row (p_old is never rewritten here), and
// the block partial of p_new . q
__global__ void __launch_bounds__(FB)
k_cg_spmv(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
          int use_weights, int64_t n, const uint8_t *__restrict__ unknown, const double *__restrict__ scale,
          const double *__restrict__ r, const double *__restrict__ p_old, double *__restrict__ p_new,
          double *__restrict__ q, const CgState *__restrict__ st, double *__restrict__ partial) {
    __shared__ double sh[FB / 64];
    const int64_t k = blockIdx.y;
    if (!st[k].active) return;
    const double beta = st[k].beta;
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    double pq = 0.0;
    if (i < n && unknown[k * n + i]) {
        const int64_t o = k * n + i;
        const double si = scale[o];
        const double pi = r[o] + beta * p_old[o];
        double D = 0.0, acc = 0.0;
        for (int e = indptr[i]; e < indptr[i + 1]; e++) {
            const double w = use_weights ? data[e] : 1.0;
            D += w;
            const int64_t oj = k * n + indices[e];
            if (unknown[oj]) acc += w * scale[oj] * (r[oj] + beta * p_old[oj]);
        }
        const double qi = si * (D * si * pi - acc);
        p_new[o] = pi;
        q[o] = qi;
        pq = pi * qi;
    }
    block_reduce_all<FB, OpSum>(sh, pq);
    if (threadIdx.x == 0) partial[k * gridDim.x + blockIdx.x] = pq;
}

__global__ void __launch_bounds__(FB)
k_cg_alpha(const double *__restrict__ partial, int nb, CgState *__restrict__ st, int32_t *__restrict__ active_out) {
    __shared__ double sh[FB / 64];
    const int64_t k = blockIdx.x;
    if (!st[k].active) return;
    const double pq = slice_total(partial + k * nb, nb, sh);
    if (threadIdx.x) return;
    if (!(pq > 0.0) || !isfinite(pq)) {
        st[k].active = 0;
        st[k].status = FILL_BREAKDOWN;
        active_out[k] = 0;
        return;
    }
    st[k].alpha = st[k].rho / pq;
}

__global__ void __launch_bounds__(FB)
k_cg_update(int64_t n, const uint8_t *__restrict__ unknown, const double *__restrict__ p, const double *__restrict__ q,
            double *__restrict__ x, double *__restrict__ r, const CgState *__restrict__ st, double *__restrict__ partial) {
    __shared__ double sh[FB / 64];
    const int64_t k = blockIdx.y;
    if (!st[k].active) return;
    const double alpha = st[k].alpha;
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    double rr = 0.0;
    if (i < n && unknown[k * n + i]) {
        const int64_t o = k * n + i;
        x[o] += alpha * p[o];
        const double ri = r[o] - alpha * q[o];
        r[o] = ri;
        rr = ri * ri;
    }
    block_reduce_all<FB, OpSum>(sh, rr);
    if (threadIdx.x == 0) partial[k * gridDim.x + blockIdx.x] = rr;
}

// the top of scipy's next loop pass: stop when ||r|| < tol -- unless this was the last allowed iteration (scipy then
// leaves the loop without the test and reports maxiter)
__global__ void __launch_bounds__(FB)
k_cg_beta(const double *__restrict__ partial, int nb, int64_t maxiter, CgState *__restrict__ st,
          int32_t *__restrict__ active_out) {
    __shared__ double sh[FB / 64];
    const int64_t k = blockIdx.x;
    if (!st[k].active) return;
    const double rr = slice_total(partial + k * nb, nb, sh);
    if (threadIdx.x) return;
    CgState s = st[k];
    s.iter += 1;
    if (s.iter >= maxiter) {
        s.active = 0;
        s.status = FILL_MAXITER;
    } else if (sqrt(rr) < s.tol) {
        s.active = 0;
        s.status = FILL_CONVERGED;
    } else {
        s.beta = rr / s.rho;
        s.rho = rr;
    }
    st[k] = s;
    active_out[k] = s.active;
}

__global__ void __launch_bounds__(FB)
k_fill_finish(int64_t n, int64_t total, const uint8_t *__restrict__ unknown, const double *__restrict__ scale,
              const double *__restrict__ x, double *__restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (o < total && unknown[o]) out[o] = scale[o] * x[o];
}

__global__ void k_cg_report(const CgState *__restrict__ st, int64_t K, int64_t *__restrict__ iters, int32_t *__restrict__ status) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) {
        iters[k] = st[k].iter;
        status[k] = st[k].status;
    }
}

// ---------------------------------------------------------------------------------------------
// nearest fill
// ---------------------------------------------------------------------------------------------
// mismatch[k] = 1 if the NaN mask of slice k differs from slice 0's
__global__ void __launch_bounds__(FB)
k_nn_mask_cmp(const double *__restrict__ in, int64_t n, uint8_t *__restrict__ mismatch) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    const int64_t k = blockIdx.y + 1;
    if (i >= n) return;
    const double a = in[i], b = in[k * n + i];
    if ((a != a) != (b != b)) mismatch[k] = 1;
}

// a valid entry keeps its own value; a null one takes the value at src (the search's answer, read for null entries only)
__global__ void __launch_bounds__(FB)
k_nn_gather(const double *__restrict__ in, int64_t n, const int64_t *__restrict__ src, const int64_t *__restrict__ slices,
            double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= n) return;
    const int64_t k = slices[blockIdx.y];
    double v = in[k * n + i];
    if (v != v) {
        const int64_t j = src[i];
        v = j >= 0 ? in[k * n + j] : NAN;
    }
    out[k * n + i] = v;
}

// the slices share the NaN mask of slices[0]: an index of its valid points (xr_nn.h), one search for its null points
static void nearest_group(const double *xy, int64_t n, const double *in, double *out, const std::vector<int64_t> &slices,
                          double max_distance) {
    const double *v = in + slices[0] * n;
    const NnExtent valid = nn_extent(xy, n, v);
    XR_REQUIRE(valid.n > 0, XR_ERR_INVALID, "All values are NA.");
    DevBuf<int64_t> src((size_t)n);
    std::unique_ptr<xr_nn> nn;
    if (valid.n < n) { // (without a null entry there is nothing to build or search)
        nn.reset(nn_build(xy, n, v, valid));
        nn_query(nn.get(), xy, n, max_distance, src.get(), v, n - valid.n);
    }
    const unsigned nb = div_up(n, FB);
    DevBuf<int64_t> sl(slices.size());
    h2d(sl.get(), slices.data(), sizeof(int64_t) * slices.size());
    for (size_t s0 = 0; s0 < slices.size(); s0 += 65535) {
        const size_t cnt = std::min<size_t>(65535, slices.size() - s0);
        XR_LAUNCH("nn_gather", k_nn_gather, dim3(nb, (unsigned)cnt), dim3(FB), 0, in, n, src.get(), sl.get() + s0, out);
    }
}

// labels = the smallest member id of every component: rounds of k_label_round until none lowers a label
void label_components(xr_graph *g) {
    const int64_t n = g->n;
    if (n <= 0) return;
    DevBuf<int32_t> changed(1);
    XR_LAUNCH("label_init", k_label_init, dim3(div_up(n, FB)), dim3(FB), 0, g->labels.get(), n);
    for (;;) {
        fill_i32(changed.get(), 0, 1);
        XR_LAUNCH("label_round", k_label_round, dim3(div_up(n, FB)), dim3(FB), 0, g->indptr.get(), g->indices.get(), n,
                  g->labels.get(), changed.get());
        g->label_rounds++;
        if (!read_scalar(changed.get())) break;
    }
}

static void laplace_fill(const xr_graph *g, const double *in_dev, double *out_dev, int64_t K, int use_weights, double atol,
                         double rtol, int64_t maxiter, int64_t chunk, int64_t *iterations_out, int *status_out);
static void nearest_fill(const double *xy_dev, int64_t n, const double *in_dev, double *out_dev, int64_t K, double max_distance);

} // namespace xr

using namespace xr;

extern "C" {

int xr_graph_from_csr(const int64_t *indptr, const int64_t *indices, const double *data, int64_t n, int64_t nnz,
                      const int64_t *labels, xr_graph **out) {
    XR_API_BEGIN
    XR_REQUIRE(indptr && out && (indices || nnz == 0), XR_ERR_INVALID, "xr_graph_from_csr: NULL argument");
    XR_REQUIRE(n >= 0 && nnz >= 0, XR_ERR_INVALID, "xr_graph_from_csr: negative size");
    XR_REQUIRE(n < INT32_MAX && nnz < INT32_MAX, XR_ERR_LIMIT, "xr_graph_from_csr: more than 2^31 rows or entries");
    XR_REQUIRE(indptr[0] == 0 && indptr[n] == nnz, XR_ERR_INVALID, "xr_graph_from_csr: indptr does not span the entries");
    std::vector<int32_t> ip((size_t)n + 1), ix((size_t)nnz), lb;
    for (int64_t i = 0; i <= n; i++) {
        XR_REQUIRE(i == 0 || indptr[i] >= indptr[i - 1], XR_ERR_INVALID, "xr_graph_from_csr: indptr is not ascending");
        ip[(size_t)i] = (int32_t)indptr[i];
    }
    for (int64_t e = 0; e < nnz; e++) {
        XR_REQUIRE(indices[e] >= 0 && indices[e] < n, XR_ERR_INVALID, "xr_graph_from_csr: column index out of range");
        ix[(size_t)e] = (int32_t)indices[e];
    }
    if (labels) {
        lb.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            XR_REQUIRE(labels[i] >= 0 && labels[i] < n, XR_ERR_INVALID, "xr_graph_from_csr: component label out of range");
            lb[(size_t)i] = (int32_t)labels[i];
        }
    }
    std::unique_ptr<xr_graph> g(new xr_graph());
    g->n = n, g->nnz = nnz, g->has_data = data != nullptr;
    g->indptr.alloc((size_t)n + 1);
    g->indices.alloc((size_t)nnz);
    g->data.alloc((size_t)nnz);
    g->labels.alloc((size_t)n);
    h2d(g->indptr.get(), ip.data(), sizeof(int32_t) * ip.size());
    if (nnz) h2d(g->indices.get(), ix.data(), sizeof(int32_t) * ix.size());
    if (nnz) {
        if (data) h2d(g->data.get(), data, sizeof(double) * (size_t)nnz);
        else fill_f64(g->data.get(), 1.0, nnz);
    }
    if (labels) {
        if (n) h2d(g->labels.get(), lb.data(), sizeof(int32_t) * lb.size());
    } else if (n) {
        label_components(g.get());
    }
    stream_sync();
    *out = g.release();
    XR_API_END
}

int xr_graph_info(const xr_graph *g, int64_t *n, int64_t *nnz) {
    XR_API_BEGIN
    XR_REQUIRE(g, XR_ERR_INVALID, "xr_graph_info: NULL handle");
    if (n) *n = g->n;
    if (nnz) *nnz = g->nnz;
    XR_API_END
}

int xr_graph_download(const xr_graph *g, int64_t *indptr, int64_t *indices, double *data, int64_t *labels) {
    XR_API_BEGIN
    XR_REQUIRE(g, XR_ERR_INVALID, "xr_graph_download: NULL handle");
    std::vector<int32_t> t((size_t)std::max(g->n + 1, g->nnz));
    if (indptr) {
        d2h(t.data(), g->indptr.get(), sizeof(int32_t) * (size_t)(g->n + 1));
        for (int64_t i = 0; i <= g->n; i++) indptr[i] = t[(size_t)i];
    }
    if (indices && g->nnz) {
        d2h(t.data(), g->indices.get(), sizeof(int32_t) * (size_t)g->nnz);
        for (int64_t e = 0; e < g->nnz; e++) indices[e] = t[(size_t)e];
    }
    if (data && g->nnz) d2h(data, g->data.get(), sizeof(double) * (size_t)g->nnz);
    if (labels && g->n) {
        d2h(t.data(), g->labels.get(), sizeof(int32_t) * (size_t)g->n);
        for (int64_t i = 0; i < g->n; i++) labels[i] = t[(size_t)i];
    }
    XR_API_END
}

int xr_graph_destroy(xr_graph *g) {
    XR_API_BEGIN
    if (g) {
        release_point();
        delete g;
    }
    XR_API_END
}

int xr_graph_laplace_fill_dev(const xr_graph *g, const double *in_dev, double *out_dev, int64_t K, int use_weights,
                              double atol, double rtol, int64_t maxiter, int64_t chunk, int64_t *iterations_out,
                              int *status_out) {
    XR_API_BEGIN
    XR_REQUIRE(g && iterations_out && status_out, XR_ERR_INVALID, "xr_graph_laplace_fill_dev: NULL argument");
    XR_REQUIRE(K >= 0 && K < 65536, XR_ERR_INVALID, "xr_graph_laplace_fill_dev: K must be in [0, 65536)");
    const int64_t n = g->n;
    XR_REQUIRE((in_dev && out_dev) || n == 0 || K == 0, XR_ERR_INVALID, "xr_graph_laplace_fill_dev: NULL data");
    XR_REQUIRE(!use_weights || g->has_data, XR_ERR_INVALID, "xr_graph_laplace_fill_dev: the graph has no weights");
    if (K > 0) laplace_fill(g, in_dev, out_dev, K, use_weights, atol, rtol, maxiter, chunk, iterations_out, status_out);
    XR_API_END
}

} // extern "C"

namespace xr {
static void laplace_fill(const xr_graph *g, const double *in_dev, double *out_dev, int64_t K, int use_weights, double atol,
                         double rtol, int64_t maxiter, int64_t chunk, int64_t *iterations_out, int *status_out) {
    const int64_t n = g->n;
    if (chunk <= 0) chunk = 24;
    const int64_t total = n * K;
    const unsigned nb = div_up(std::max<int64_t>(n, 1), FB);
    DevBuf<uint8_t> flags((size_t)total * 2 + 2 * (size_t)K); // comp_valid, unknown, has_valid, has_null
    uint8_t *comp_valid = flags.get(), *unknown = flags.get() + total, *has_valid = unknown + total, *has_null = has_valid + K;
    DevBuf<double> work((size_t)total * 6), partial((size_t)K * nb);
    double *scale = work.get(), *x = scale + total, *r = x + total, *p[2] = {r + total, r + 2 * total}, *q = r + 3 * total;
    DevBuf<CgState> st((size_t)K);
    DevBuf<int32_t> active((size_t)K);
    DevBuf<int64_t> iters((size_t)K);
    DevBuf<int32_t> status((size_t)K);
    XR_HIP(hipMemsetAsync(flags.get(), 0, flags.bytes(), launch_stream()));
    const dim3 rows(nb, (unsigned)K);
    if (n) {
        XR_LAUNCH("fill_mark", k_fill_mark, rows, dim3(FB), 0, in_dev, g->labels.get(), n, comp_valid, has_valid, has_null);
        XR_LAUNCH("fill_setup", k_fill_setup, rows, dim3(FB), 0, in_dev, g->indptr.get(), g->indices.get(), g->data.get(),
                  use_weights, g->labels.get(), comp_valid, n, out_dev, unknown, scale, x, r, p[0], p[1], partial.get());
    } else {
        fill_f64(partial.get(), 0.0, (int64_t)K * nb);
    }
    XR_LAUNCH("cg_start", k_cg_start, dim3((unsigned)K), dim3(FB), 0, partial.get(), (int)nb, has_valid, has_null, atol, rtol,
              maxiter, st.get(), active.get());
    std::vector<int32_t> h_active((size_t)K);
    d2h(h_active.data(), active.get(), sizeof(int32_t) * (size_t)K);
    int64_t done = 0;
    int parity = 0;
    auto any_active = [&]() { return std::any_of(h_active.begin(), h_active.end(), [](int32_t a) { return a != 0; }); };
    while (any_active() && done < maxiter) {
        const int64_t steps = std::min(chunk, maxiter - done);
        for (int64_t s = 0; s < steps; s++) {
            XR_LAUNCH("cg_spmv", k_cg_spmv, rows, dim3(FB), 0, g->indptr.get(), g->indices.get(), g->data.get(), use_weights, n,
                      unknown, scale, r, p[parity], p[parity ^ 1], q, st.get(), partial.get());
            XR_LAUNCH("cg_alpha", k_cg_alpha, dim3((unsigned)K), dim3(FB), 0, partial.get(), (int)nb, st.get(), active.get());
            XR_LAUNCH("cg_update", k_cg_update, rows, dim3(FB), 0, n, unknown, p[parity ^ 1], q, x, r, st.get(), partial.get());
            XR_LAUNCH("cg_beta", k_cg_beta, dim3((unsigned)K), dim3(FB), 0, partial.get(), (int)nb, maxiter, st.get(), active.get());
            parity ^= 1;
        }
        done += steps;
        d2h(h_active.data(), active.get(), sizeof(int32_t) * (size_t)K);
    }
    if (total) XR_LAUNCH("fill_finish", k_fill_finish, dim3(div_up(total, FB)), dim3(FB), 0, n, total, unknown, scale, x, out_dev);
    XR_LAUNCH("cg_report", k_cg_report, dim3(div_up(K, 64)), dim3(64), 0, st.get(), K, iters.get(), status.get());
    d2h(iterations_out, iters.get(), sizeof(int64_t) * (size_t)K);
    d2h(status_out, status.get(), sizeof(int32_t) * (size_t)K);
}
} // namespace xr

extern "C" {

int xr_nearest_fill_dev(const double *xy_dev, int64_t n, const double *in_dev, double *out_dev, int64_t K, double max_distance) {
    XR_API_BEGIN
    XR_REQUIRE(K >= 0 && K < 65536, XR_ERR_INVALID, "xr_nearest_fill_dev: K must be in [0, 65536)");
    XR_REQUIRE((xy_dev && in_dev && out_dev) || n == 0 || K == 0, XR_ERR_INVALID, "xr_nearest_fill_dev: NULL argument");
    XR_REQUIRE(n < INT32_MAX, XR_ERR_LIMIT, "xr_nearest_fill_dev: more than 2^31 points");
    XR_REQUIRE(max_distance >= 0.0, XR_ERR_INVALID, "xr_nearest_fill_dev: max_distance must be non-negative");
    if (n > 0 && K > 0) nearest_fill(xy_dev, n, in_dev, out_dev, K, max_distance);
    dev_call_done();
    XR_API_END
}

} // extern "C"

namespace xr {
static void nearest_fill(const double *xy_dev, int64_t n, const double *in_dev, double *out_dev, int64_t K, double max_distance) {
    std::vector<uint8_t> mismatch((size_t)K, 0);
    if (K > 1) {
        DevBuf<uint8_t> mm((size_t)K);
        XR_HIP(hipMemsetAsync(mm.get(), 0, (size_t)K, launch_stream()));
        XR_LAUNCH("nn_mask_cmp", k_nn_mask_cmp, dim3(div_up(n, FB), (unsigned)(K - 1)), dim3(FB), 0, in_dev, n, mm.get());
        d2h(mismatch.data(), mm.get(), (size_t)K);
    }
    std::vector<int64_t> same;
    for (int64_t k = 0; k < K; k++)
        if (!mismatch[(size_t)k]) same.push_back(k);
    nearest_group(xy_dev, n, in_dev, out_dev, same, max_distance);
    for (int64_t k = 1; k < K; k++)
        if (mismatch[(size_t)k]) nearest_group(xy_dev, n, in_dev, out_dev, std::vector<int64_t>{k}, max_distance);
}
} // namespace xr

// ---------------------------------------------------------------------------------------------
// graphs from the device topology; graph operations
// ---------------------------------------------------------------------------------------------
namespace xr {

// d[e] = distance between the points of row i and column indices[e] (ugridbase.py:962-970: sqrt(dx*dx + dy*dy) of col - row);
// block partial of their sum
__global__ void __launch_bounds__(FB)
k_graph_distance(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ xy, int64_t n,
                 double *__restrict__ d, double *__restrict__ partial) {
    __shared__ double sh[FB / 64];
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    double sum = 0.0;
    if (i < n) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        for (int e = indptr[i]; e < indptr[i + 1]; e++) {
            const int64_t j = indices[e];
            const double dx = xy[2 * j] - x, dy = xy[2 * j + 1] - y;
            const double v = sqrt(dx * dx + dy * dy);
            d[e] = v;
            sum += v;
        }
    }
    block_reduce_all<FB, OpSum>(sh, sum);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// d -> mean(d) / d
__global__ void __launch_bounds__(FB) k_graph_weights(double *__restrict__ d, int64_t nnz, const double *__restrict__ total) {
    const int64_t e = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (e < nnz) d[e] = (total[0] / (double)nnz) / d[e];
}

__global__ void __launch_bounds__(FB) k_comp_flag(const int32_t *__restrict__ lab, int64_t n, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i < n) flag[i] = lab[i] == (int32_t)i;
}
// rank[i] = components whose smallest member lies below i; a member's number is the rank of its label
__global__ void __launch_bounds__(FB)
k_comp_number(const int32_t *__restrict__ lab, const int32_t *__restrict__ rank, int64_t n, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i < n) out[i] = rank[lab[i]];
}

// one Jacobi step of the binary iteration on a snapshot: in -> out, slice on gridDim.y
__global__ void __launch_bounds__(FB)
k_binary_step(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n, const uint8_t *__restrict__ in,
              uint8_t *__restrict__ out, uint8_t value, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ exterior) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= n) return;
    const uint8_t *src = in + (int64_t)blockIdx.y * n;
    const bool own = src[i] != 0;
    bool differs = false;
    for (int e = indptr[i]; e < indptr[i + 1] && !differs; e++) differs = (src[indices[e]] != 0) != own;
    uint8_t r = differs ? value : (uint8_t)own;
    if (mask && mask[i]) r = !value; // (sic: the reference's `output[mask] = not value`)
    if (exterior && exterior[i]) r = value;
    out[(int64_t)blockIdx.y * n + i] = r;
}

} // namespace xr

extern "C" {

int xr_graph_from_topology(const xr_topology *t, int facet, xr_graph **out) {
    XR_API_BEGIN
    XR_REQUIRE(t && out, XR_ERR_INVALID, "xr_graph_from_topology: NULL argument");
    XR_REQUIRE(facet == XR_FACET_NODE || facet == XR_FACET_FACE, XR_ERR_INVALID,
               "xr_graph_from_topology: facet must be XR_FACET_NODE or XR_FACET_FACE");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_graph_from_topology: the mesh has edges with more than two faces");
    const bool face = facet == XR_FACET_FACE;
    const int64_t n = face ? t->n_face : t->n_node, nnz = face ? t->ff_nnz : t->nn_nnz;
    const int32_t *ptr = face ? t->ff_ptr.get() : t->nn_ptr.get(), *idx = face ? t->ff_idx.get() : t->nn_idx.get();
    Building<xr_graph> g;
    g->n = n, g->nnz = nnz, g->has_data = true;
    g->indptr.alloc((size_t)n + 1);
    g->indices.alloc((size_t)std::max<int64_t>(nnz, 1));
    g->data.alloc((size_t)std::max<int64_t>(nnz, 1));
    g->labels.alloc((size_t)std::max<int64_t>(n, 1));
    XR_HIP(hipMemcpyAsync(g->indptr.get(), ptr, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToDevice, launch_stream()));
    if (nnz > 0) {
        XR_HIP(hipMemcpyAsync(g->indices.get(), idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, launch_stream()));
        const auto centroids = face ? mesh_centroids_shared(t->mesh) : nullptr;
        const double *xy = face ? centroids->get() : t->mesh->node_xy.get();
        const unsigned nb = div_up(n, FB);
        TwoStageReduce<FB, double, OpSum> total("graph_distance_total", nb, [&](double *partial) {
            XR_LAUNCH("graph_distance", k_graph_distance, dim3(nb), dim3(FB), 0, g->indptr.get(), g->indices.get(), xy, n, g->data.get(),
                      partial);
        });
        XR_LAUNCH("graph_weights", k_graph_weights, dim3(div_up(nnz, FB)), dim3(FB), 0, g->data.get(), nnz, total.result());
    }
    label_components(g.get());
    stream_sync();
    *out = g.release();
    XR_API_END
}

int xr_graph_label_rounds(const xr_graph *g, int64_t *rounds) {
    XR_API_BEGIN
    XR_REQUIRE(g && rounds, XR_ERR_INVALID, "xr_graph_label_rounds: NULL argument");
    *rounds = g->label_rounds;
    XR_API_END
}

int xr_graph_components_dev(const xr_graph *g, int64_t *labels_dev, int64_t *n_components) {
    XR_API_BEGIN
    XR_REQUIRE(g && n_components && (labels_dev || g->n == 0), XR_ERR_INVALID, "xr_graph_components_dev: NULL argument");
    const int64_t n = g->n;
    *n_components = 0;
    if (n > 0) {
        DevBuf<int32_t> flag((size_t)n), rank((size_t)n + 1);
        XR_LAUNCH("comp_flag", k_comp_flag, dim3(div_up(n, FB)), dim3(FB), 0, g->labels.get(), n, flag.get());
        exclusive_scan_i32(flag.get(), rank.get(), n);
        XR_LAUNCH("comp_number", k_comp_number, dim3(div_up(n, FB)), dim3(FB), 0, g->labels.get(), rank.get(), n, labels_dev);
        *n_components = read_scalar(rank.get() + n);
    }
    XR_API_END
}

int xr_graph_binary_iterate_dev(const xr_graph *g, const uint8_t *in_dev, uint8_t *out_dev, int64_t K, int value,
                                int64_t iterations, const uint8_t *mask_dev, const uint8_t *exterior_dev) {
    XR_API_BEGIN
    XR_REQUIRE(g, XR_ERR_INVALID, "xr_graph_binary_iterate_dev: NULL handle");
    XR_REQUIRE(K >= 0 && K < 65536, XR_ERR_INVALID, "xr_graph_binary_iterate_dev: K must be in [0, 65536)");
    XR_REQUIRE(iterations >= 1, XR_ERR_INVALID, "xr_graph_binary_iterate_dev: iterations must be at least 1");
    const int64_t n = g->n;
    XR_REQUIRE((in_dev && out_dev) || n == 0 || K == 0, XR_ERR_INVALID, "xr_graph_binary_iterate_dev: NULL data");
    if (n > 0 && K > 0) {
        // ping-pong between out_dev and one scratch buffer so that the last step lands in out_dev; the input is only read
        DevBuf<uint8_t> scratch(iterations > 1 ? (size_t)(n * K) : 1);
        uint8_t *buf[2] = {out_dev, scratch.get()};
        int at = (int)((iterations - 1) & 1); // step s writes buf[(iterations - 1 - s) & 1]
        const uint8_t *src = in_dev;
        const dim3 grid(div_up(n, FB), (unsigned)K);
        for (int64_t s = 0; s < iterations; s++) {
            XR_LAUNCH("binary_step", k_binary_step, grid, dim3(FB), 0, g->indptr.get(), g->indices.get(), n, src, buf[at],
                      (uint8_t)(value != 0), mask_dev, s == 0 ? exterior_dev : nullptr);
            src = buf[at];
            at ^= 1;
        }
        stream_sync(); // (the scratch goes back to the pool behind its last reader)
    }
    dev_call_done();
    XR_API_END
}

} // extern "C"
