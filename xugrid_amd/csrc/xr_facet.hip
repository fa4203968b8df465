// xr_facet.hip -- moving data between the facets of a mesh on the device: UgridDataArray.ugrid.to_node / to_edge / to_face
// (xugrid/core/dataarray_accessor.py:300-416, _to_facet: obj.isel(indexer).where(indexer != -1)) and the reduction over the new
// dimension that always follows it in the reference's documentation (.mean("nmax") and its kin), fused.
//
// A FacetTable is {target}_{source}_connectivity in one of two layouts, int32, read where it is:
//   dense  idx [n_target, width], -1 fill        face_node (the mesh's faces_raw), face_edge, edge_node, edge_face
//   CSR    ptr [n_target + 1], idx [ptr[n_target]]   node_face (nf_ptr / nf_idx), node_edge (nn_ptr / nn_dat); width = widest row
// Raw form:     out[k, t, j] = in[k, table[t, j]], NaN where there is no entry -- one lane per (t, j), so consecutive lanes write
//               consecutive elements of a slice and read consecutive table entries.
// Reduced form: out[k, t] = mean / sum / min / max over the row's non-NaN contributors -- one lane per target, walking the row's
//               entries in table order (THE ORDER IS THE SPECIFICATION of the float64 sum: the same bits on every run).  Rows of
//               any length: the lane loops; nothing is staged, capped or truncated.
// Both forms keep a tile of FACET_TILE slices in the lane: an index is read once per tile, not once per slice; tiles ride on
// gridDim.y (chunked at 65 535 tiles), so the K edge is the tile remainder.  DESIGN section 11 has the measurement.
#include <algorithm>
#include <cmath>

#include "xr_prims.h"
#include "xr_topology.h"

namespace xr {

static constexpr int FB = 256;       // threads per block
static constexpr int FACET_TILE = 8; // slices per lane (option facet_tile = 1: one slice per lane, the A/B of DESIGN section 11)

struct FacetTable {
    const int32_t *ptr; // nullptr: dense
    const int32_t *idx;
    int64_t n_target, n_source;
    int width;
};

// flag = 1 unless every index is below n_source, the row pointers start at 0, never decrease and end at ptr[n_target] (the
// length of idx) and no row is longer than `width`: the one validation pass of a call, before anything is read through an
// index.  A lane reads its row's entries only once the row's own bounds are sane.
__global__ void __launch_bounds__(FB) k_facet_check(FacetTable tb, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    bool bad = false;
    if (tb.ptr) {
        if (i < tb.n_target) {
            const int s = tb.ptr[i], e = tb.ptr[i + 1];
            bad = s < 0 || e < s || e - s > tb.width || e > tb.ptr[tb.n_target] || (i == 0 && s != 0);
            if (!bad)
                for (int r = s; r < e; r++) bad |= tb.idx[r] >= tb.n_source;
        }
    } else if (i < tb.n_target * tb.width) {
        bad = tb.idx[i] >= tb.n_source;
    }
    wave_flag(bad, flag);
}

// widest row of a CSR: one block, any number of rows -> out[0]
__global__ void __launch_bounds__(FB) k_facet_width(const int32_t *__restrict__ ptr, int64_t n, int32_t *__restrict__ out) {
    __shared__ int sh[FB / 64];
    int w = 0;
    for (int64_t i = threadIdx.x; i < n; i += FB) w = max(w, ptr[i + 1] - ptr[i]);
    block_reduce<FB, OpMax>(sh, w);
    if (threadIdx.x == 0) out[0] = w;
}

// one lane per output element (t, j) of a slice; slices [blockIdx.y * KT, ...) of the K of this launch
template <typename SRC, int KT>
__global__ void __launch_bounds__(FB) k_facet_raw(FacetTable tb, const SRC *__restrict__ in, int64_t K, double *__restrict__ out) {
    const int64_t total = tb.n_target * tb.width;
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= total) return;
    int idx;
    if (tb.ptr) {
        const int64_t t = i / tb.width;
        const int j = (int)(i - t * tb.width);
        const int s = tb.ptr[t];
        idx = j < tb.ptr[t + 1] - s ? tb.idx[s + j] : -1;
    } else {
        idx = tb.idx[i];
    }
    const int64_t k0 = (int64_t)blockIdx.y * KT;
    const int kn = (int)min((int64_t)KT, K - k0);
    const SRC *src = in + k0 * tb.n_source;
    double *dst = out + k0 * total + i;
    if (idx < 0) {
        for (int u = 0; u < kn; u++) dst[u * total] = NAN;
    } else if (kn == KT) {
        double v[KT];
#pragma unroll
        for (int u = 0; u < KT; u++) v[u] = (double)src[u * tb.n_source + idx];
#pragma unroll
        for (int u = 0; u < KT; u++) dst[u * total] = v[u];
    } else {
        for (int u = 0; u < kn; u++) dst[u * total] = (double)src[u * tb.n_source + idx];
    }
}

// one lane per target: its row's entries in table order, KT slices at a time.  NaN contributors are passed over; a target
// without a contributor gets 0.0 (sum) or NaN (mean, min, max).
template <typename SRC, int FORM, int KT>
__global__ void __launch_bounds__(FB) k_facet_reduce(FacetTable tb, const SRC *__restrict__ in, int64_t K, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= tb.n_target) return;
    const int64_t s = tb.ptr ? tb.ptr[t] : t * tb.width, e = tb.ptr ? tb.ptr[t + 1] : s + tb.width;
    const int64_t k0 = (int64_t)blockIdx.y * KT;
    const int kn = (int)min((int64_t)KT, K - k0);
    const SRC *src = in + k0 * tb.n_source;
    constexpr bool summing = FORM == XR_FACET_MEAN || FORM == XR_FACET_SUM;
    double acc[KT];
    int cnt[KT];
#pragma unroll
    for (int u = 0; u < KT; u++) acc[u] = summing ? 0.0 : NAN, cnt[u] = 0;
    for (int64_t r = s; r < e; r++) {
        const int idx = tb.idx[r];
        if (idx < 0) continue;
#pragma unroll
        for (int u = 0; u < KT; u++) {
            if (u >= kn) continue;
            const double x = (double)src[u * tb.n_source + idx];
            if (x != x) continue;
            if (summing) acc[u] += x, cnt[u]++;
            else if (FORM == XR_FACET_MIN) acc[u] = fmin(acc[u], x); // (fmin / fmax of NaN and x: x)
            else acc[u] = fmax(acc[u], x);
        }
    }
    double *dst = out + k0 * tb.n_target + t;
#pragma unroll
    for (int u = 0; u < KT; u++) {
        if (u >= kn) continue;
        dst[u * tb.n_target] = FORM == XR_FACET_MEAN ? (cnt[u] > 0 ? acc[u] / (double)cnt[u] : NAN) : acc[u];
    }
}

template <typename SRC, int KT> static void launch_tiles(const FacetTable &tb, int form, const SRC *in, int64_t K, double *out) {
    const int64_t per_slice = form == XR_FACET_RAW ? tb.n_target * tb.width : tb.n_target;
    const unsigned nb = div_up(form == XR_FACET_RAW ? per_slice : tb.n_target, FB);
    const int64_t chunk = (int64_t)65535 * KT; // (tiles on gridDim.y)
    for (int64_t k0 = 0; k0 < K; k0 += chunk) {
        const int64_t cnt = std::min<int64_t>(chunk, K - k0);
        const dim3 grid(nb, div_up(cnt, KT));
        const SRC *src = in + k0 * tb.n_source;
        double *dst = out + k0 * per_slice;
        switch (form) {
        case XR_FACET_RAW: XR_LAUNCH("facet_raw", (k_facet_raw<SRC, KT>), grid, dim3(FB), 0, tb, src, cnt, dst); break;
        case XR_FACET_MEAN: XR_LAUNCH("facet_reduce", (k_facet_reduce<SRC, XR_FACET_MEAN, KT>), grid, dim3(FB), 0, tb, src, cnt, dst); break;
        case XR_FACET_SUM: XR_LAUNCH("facet_reduce", (k_facet_reduce<SRC, XR_FACET_SUM, KT>), grid, dim3(FB), 0, tb, src, cnt, dst); break;
        case XR_FACET_MIN: XR_LAUNCH("facet_reduce", (k_facet_reduce<SRC, XR_FACET_MIN, KT>), grid, dim3(FB), 0, tb, src, cnt, dst); break;
        default: XR_LAUNCH("facet_reduce", (k_facet_reduce<SRC, XR_FACET_MAX, KT>), grid, dim3(FB), 0, tb, src, cnt, dst); break;
        }
    }
}

// the one launcher behind both entry points
static void facet_map(const char *who, const FacetTable &tb, int form, const void *in_dev, int dtype, int64_t K, double *out_dev) {
    XR_REQUIRE(form == XR_FACET_MEAN || form == XR_FACET_SUM || form == XR_FACET_MIN || form == XR_FACET_MAX || form == XR_FACET_RAW,
               XR_ERR_INVALID, "%s: form must be XR_FACET_MEAN, _SUM, _MIN, _MAX or _RAW", who);
    XR_REQUIRE(K >= 0 && tb.n_target >= 0 && tb.n_source >= 0 && tb.width >= 0, XR_ERR_INVALID, "%s: negative size", who);
    XR_REQUIRE(tb.n_target < INT32_MAX && tb.n_source < INT32_MAX, XR_ERR_LIMIT, "%s: more than 2^31 entities", who);
    const int64_t cells = tb.n_target * tb.width; // (both below 2^31)
    XR_REQUIRE(cells < (int64_t)INT32_MAX * FB, XR_ERR_LIMIT, "%s: the table has too many cells", who);
    const int64_t n_out = form == XR_FACET_RAW ? cells : tb.n_target;
    with_source_type(dtype, [](auto) {});
    if (K == 0 || n_out == 0) return;
    XR_REQUIRE(in_dev || tb.n_source == 0, XR_ERR_INVALID, "%s: NULL argument", who);
    XR_REQUIRE(out_dev && (tb.idx || cells == 0) , XR_ERR_INVALID, "%s: NULL argument", who);
    const int64_t n_check = tb.ptr ? tb.n_target : cells;
    if (n_check > 0) {
        DevBuf<int32_t> flag(1);
        fill_i32(flag.get(), 0, 1);
        XR_LAUNCH("facet_check", k_facet_check, dim3(div_up(n_check, FB)), dim3(FB), 0, tb, flag.get());
        XR_REQUIRE(read_scalar(flag.get()) == 0, XR_ERR_INVALID,
                   "%s: the table is not valid (an index beyond the %lld source entries, or rows that are out of order or wider than %d)",
                   who, (long long)tb.n_source, tb.width);
    }
    const bool one = option(OPT_FACET_TILE) == 1;
    with_source_type(dtype, [&](auto tag) {
        using SRC = decltype(tag);
        const SRC *in = static_cast<const SRC *>(in_dev);
        if (one) launch_tiles<SRC, 1>(tb, form, in, K, out_dev);
        else launch_tiles<SRC, FACET_TILE>(tb, form, in, K, out_dev);
    });
}

static bool facet_id(int f) { return f == XR_FACET_NODE || f == XR_FACET_EDGE || f == XR_FACET_FACE; }

// widest rows of the two CSR tables of a topology: one reduction each on first request, then kept
static void topology_widths(xr_topology *t) {
    if (t->nf_width >= 0) return;
    DevBuf<int32_t> w(2);
    XR_LAUNCH("facet_width", k_facet_width, dim3(1), dim3(FB), 0, t->nf_ptr.get(), t->n_node, w.get());
    XR_LAUNCH("facet_width", k_facet_width, dim3(1), dim3(FB), 0, t->nn_ptr.get(), t->n_node, w.get() + 1);
    int32_t h[2];
    d2h(h, w.get(), sizeof(h));
    t->nf_width = h[0], t->nn_width = h[1];
}

static FacetTable topology_table(const char *who, xr_topology *t, int target, int source) {
    XR_REQUIRE(facet_id(target) && facet_id(source), XR_ERR_INVALID, "%s: facets are XR_FACET_NODE, _EDGE or _FACE", who);
    XR_REQUIRE(target != source, XR_ERR_INVALID, "%s: target and source facet are the same", who);
    const int64_t n_of[3] = {t->n_node, t->n_edge, t->n_face};
    FacetTable tb{nullptr, nullptr, n_of[target], n_of[source], 2};
    if (target == XR_FACET_NODE) {
        topology_widths(t);
        const bool face = source == XR_FACET_FACE;
        tb.ptr = face ? t->nf_ptr.get() : t->nn_ptr.get();
        tb.idx = face ? t->nf_idx.get() : t->nn_dat.get();
        tb.width = face ? t->nf_width : t->nn_width;
    } else if (target == XR_FACET_FACE) {
        tb.idx = source == XR_FACET_NODE ? t->mesh->faces_raw.get() : t->face_edge.get();
        tb.width = t->m;
    } else {
        tb.idx = source == XR_FACET_NODE ? t->edge_node.get() : t->edge_face.get();
    }
    return tb;
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_topology_facet_width(xr_topology *t, int target, int source, int64_t *width) {
    XR_API_BEGIN
    XR_REQUIRE(t && width, XR_ERR_INVALID, "xr_topology_facet_width: NULL argument");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_facet_width: the mesh has edges with more than two faces");
    *width = topology_table("xr_topology_facet_width", t, target, source).width;
    XR_API_END
}

int xr_topology_facet_map_dev(xr_topology *t, int target, int source, int form, const void *in_dev, int dtype, int64_t K,
                              double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(t, XR_ERR_INVALID, "xr_topology_facet_map_dev: NULL handle");
    XR_REQUIRE(t->n_nonmanifold == 0, XR_ERR_INVALID, "xr_topology_facet_map_dev: the mesh has edges with more than two faces");
    facet_map("xr_topology_facet_map_dev", topology_table("xr_topology_facet_map_dev", t, target, source), form, in_dev, dtype, K,
              out_dev);
    dev_call_done();
    XR_API_END
}

int xr_facet_map_dev(const int32_t *ptr_dev, const int32_t *idx_dev, int64_t n_target, int64_t width, int64_t n_source, int form,
                     const void *in_dev, int dtype, int64_t K, double *out_dev) {
    XR_API_BEGIN
    XR_REQUIRE(width >= 0 && width < INT32_MAX, XR_ERR_INVALID, "xr_facet_map_dev: width must be in [0, 2^31)");
    facet_map("xr_facet_map_dev", FacetTable{ptr_dev, idx_dev, n_target, n_source, (int)width}, form, in_dev, dtype, K, out_dev);
    dev_call_done();
    XR_API_END
}

} // extern "C"
