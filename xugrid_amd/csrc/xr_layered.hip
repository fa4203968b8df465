// xr_layered.hip -- layered (2-D grid x per-column vertical intervals) overlap weights: from a 2-D weight matrix W and the
// top / bottom of every layer in every column to the 3-D matrix, and the reference's vertical building block overlap_1d_nd
// (xugrid/regrid/overlap_1d.py:162-245) on the same two kernels.
//
// The rule: one entry for every entry (j, i, w) of W and every layer pair (lt, ls) with
//     dz = min(top_s[ls, i], top_t[lt, j]) - max(bottom_s[ls, i], bottom_t[lt, j]) > 0,
// a NaN bound or top <= bottom meaning "no such layer here"; nothing is assumed about the order of the layers.  Weight w * dz,
// relative: w * (dz / (top_s - bottom_s)).  One IEEE operation each: a numpy restatement gives the same bits.
//
// An ITEM is one (entry p of W, target layer lt) -- or one (pair k, target layer) for overlap_1d_nd -- numbered so that the
// items are in the order of the result: q = lt * nnz2d + p for the matrix (rows (lt, j) ascending, W's order of i inside a row),
// q = k * Lt + lt for the pairs.  count pass (entries of item q) -> ONE flat exclusive scan (the offsets, already in result
// order: no sort) -> fill pass (the same walk again, writing from the offset).
//
// One thread holds one entry of W (one pair) and walks ALL its items: the bounds of its source column are gathered once, a
// tile of SOURCE_TILE layers at a time into registers, and every target layer is compared with the tile -- every source layer
// against every target layer, so any layer order is served.  Consecutive lanes hold consecutive entries: W, the counts and the
// offsets are read and written coalesced, the lanes of one row share their target column, and the entries a wave writes are
// neighbours.  Columns of more than SOURCE_TILE layers take one round per tile; an item's count then grows by a plain
// read-modify-write of its own word, and the fill pass carries the item's write position from tile to tile in the words of
// the count array, which the scan has consumed by then.  (A thread per ITEM would gather every source column once per target
// layer: measured at 27 x the count pass's byte floor)
#include "xr_apply.h"
#include "xr_prims.h"

namespace xr {

static constexpr int SOURCE_TILE = 8; // source layers held in registers at a time (32 VGPRs of bounds)

// top / bottom of layer l in column c: base[l * layer_stride + c * col_stride]; (l, c) is numbered l * id_layer + c * id_col
struct Layers {
    const double *top, *bottom;
    int64_t layer_stride, col_stride;
    int64_t id_layer, id_col;
    int n_layer;
};

struct LayeredItems {
    Layers s, t;
    int64_t n_entry;          // entries of W / pairs: one thread each
    int64_t q_layer, q_entry; // item (lt, p) is number lt * q_layer + p * q_entry
    // the matrix
    const int32_t *indices, *row_of;
    const double *data;
    // the pairs
    const int64_t *source_index, *target_index;
    int64_t n_source_col, n_target_col;
};

struct Entry {
    int64_t i, j; // source, target column
    double w;
    bool ok;      // false: a pair that names a column outside its array
};

template <bool PAIRS> __device__ __forceinline__ Entry entry_of(const LayeredItems &v, int64_t p) {
    Entry e;
    if constexpr (PAIRS) {
        e.i = v.source_index[p];
        e.j = v.target_index[p];
        e.w = 1.0;
        e.ok = e.i >= 0 && e.i < v.n_source_col && e.j >= 0 && e.j < v.n_target_col;
    } else {
        e.i = v.indices[p];
        e.j = v.row_of[p];
        e.w = v.data[p];
        e.ok = true;
    }
    return e;
}

// layers ls0 ... ls0 + SOURCE_TILE of source column i; a layer that does not exist there (a NaN bound, top <= bottom, past the
// last one) becomes (-inf, +inf): its dz is -inf against any target layer, so the walk needs no test of its own
struct SourceTile {
    double top[SOURCE_TILE], bottom[SOURCE_TILE];
    __device__ __forceinline__ void load(const Layers &s, int64_t i, int ls0) {
        const double *t = s.top + i * s.col_stride, *b = s.bottom + i * s.col_stride;
#pragma unroll
        for (int k = 0; k < SOURCE_TILE; k++) {
            const bool in = ls0 + k < s.n_layer;
            const double st = in ? t[(ls0 + k) * s.layer_stride] : 0.0, sb = in ? b[(ls0 + k) * s.layer_stride] : 0.0;
            const bool exists = st > sb;
            top[k] = exists ? st : -HUGE_VAL;
            bottom[k] = exists ? sb : HUGE_VAL;
        }
    }
    __device__ __forceinline__ double dz(int k, double tt, double tb) const {
        return (top[k] < tt ? top[k] : tt) - (bottom[k] > tb ? bottom[k] : tb);
    }
};

// total64 != nullptr: the sum of the counts in 64 bits (one atomic per wave), where the int32 scan could wrap
template <bool PAIRS>
__global__ void __launch_bounds__(256)
k_layered_count(LayeredItems v, int32_t *__restrict__ count, int32_t *__restrict__ bad, unsigned long long *__restrict__ total64) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long sum = 0;
    bool ok = true;
    if (p < v.n_entry) {
        const Entry e = entry_of<PAIRS>(v, p);
        ok = e.ok;
        const int64_t at = e.j * v.t.col_stride;
        for (int ls0 = 0; ls0 == 0 || ls0 < v.s.n_layer; ls0 += SOURCE_TILE) {
            SourceTile tile;
            if (ok) tile.load(v.s, e.i, ls0);
            for (int lt = 0; lt < v.t.n_layer; lt++) {
                int n = 0;
                if (ok) {
                    const double tt = v.t.top[lt * v.t.layer_stride + at], tb = v.t.bottom[lt * v.t.layer_stride + at];
                    if (tt > tb) { // (false for a NaN bound)
#pragma unroll
                        for (int k = 0; k < SOURCE_TILE; k++) n += tile.dz(k, tt, tb) > 0;
                    }
                }
                const int64_t q = lt * v.q_layer + p * v.q_entry;
                if (ls0 == 0) count[q] = n;
                else if (n) count[q] += n;
                sum += n;
            }
        }
    }
    if constexpr (PAIRS) wave_flag(!ok, bad);
    if (total64) {
        sum = wave_reduce<OpSum>(sum);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total64, sum);
    }
}

// the matrix: (ls * n_s + i, w * dz) into indices / data; the pairs: the reference's triplets (i * Ls + ls, j * Lt + lt, dz).
// cursor: the words of the count array (one per item), free behind the scan
template <bool PAIRS, bool RELATIVE>
__global__ void __launch_bounds__(256)
k_layered_fill(LayeredItems v, const int32_t *__restrict__ offset, int32_t *__restrict__ cursor, int32_t *__restrict__ indices,
               double *__restrict__ data, int64_t *__restrict__ source_out, int64_t *__restrict__ target_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= v.n_entry) return;
    const Entry e = entry_of<PAIRS>(v, p);
    const int64_t t_at = e.j * v.t.col_stride;
    const bool one_tile = v.s.n_layer <= SOURCE_TILE;
    for (int ls0 = 0; ls0 < v.s.n_layer; ls0 += SOURCE_TILE) {
        SourceTile tile;
        tile.load(v.s, e.i, ls0);
        for (int lt = 0; lt < v.t.n_layer; lt++) {
            const int64_t q = lt * v.q_layer + p * v.q_entry;
            const int32_t end = offset[q + 1];
            int32_t at = ls0 == 0 ? offset[q] : cursor[q];
            if (at == end) { // nothing (left) for this item
                if (ls0 == 0 && !one_tile) cursor[q] = end;
                continue;
            }
            const double tt = v.t.top[lt * v.t.layer_stride + t_at], tb = v.t.bottom[lt * v.t.layer_stride + t_at];
#pragma unroll
            for (int k = 0; k < SOURCE_TILE; k++) {
                const double dz = tile.dz(k, tt, tb);
                if (dz > 0) {
                    const int64_t source_id = (int64_t)(ls0 + k) * v.s.id_layer + e.i * v.s.id_col;
                    if constexpr (PAIRS) {
                        source_out[at] = source_id;
                        target_out[at] = (int64_t)lt * v.t.id_layer + e.j * v.t.id_col;
                        data[at] = dz;
                    } else {
                        indices[at] = (int32_t)source_id;
                        data[at] = RELATIVE ? e.w * (dz / (tile.top[k] - tile.bottom[k])) : e.w * dz;
                    }
                    at++;
                }
            }
            if (!one_tile) cursor[q] = at;
        }
    }
}

__global__ void __launch_bounds__(256)
k_layered_row_of(const int32_t *__restrict__ indptr, int64_t n, int32_t *__restrict__ row_of) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    for (int p = indptr[j], e = indptr[j + 1]; p < e; p++) row_of[p] = (int32_t)j;
}

// row (lt, j) starts where its first item does: indptr3[lt * n_t + j] = offset[lt * nnz2d + indptr2[j]]; is_long[row] = 1 for
// the rows of more than XR_APPLY_LONG_ROW entries
__global__ void __launch_bounds__(256)
k_layered_indptr(const int32_t *__restrict__ indptr2, const int32_t *__restrict__ offset, int64_t n_t, int64_t n_layer_t,
                 int64_t nnz2d, int32_t *__restrict__ indptr3, int32_t *__restrict__ is_long) {
    const int64_t rows = n_layer_t * n_t;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > rows) return;
    if (r == rows) {
        indptr3[r] = offset[n_layer_t * nnz2d];
        return;
    }
    const int64_t lt = r / n_t, j = r - lt * n_t;
    const int32_t s = offset[lt * nnz2d + indptr2[j]], e = offset[lt * nnz2d + indptr2[j + 1]];
    indptr3[r] = s;
    is_long[r] = e - s > XR_APPLY_LONG_ROW;
}

static constexpr int64_t I32_LIMIT = ((int64_t)1 << 31) - 1;

// count -> scan: the offsets of the items (n_item + 1 words) and the number of entries
// (count: the counts, scratch of the fill pass afterwards)
template <bool PAIRS>
static int64_t layered_offsets(const LayeredItems &v, const char *who, DevBuf<int32_t> &count, DevBuf<int32_t> &offset) {
    const int64_t n_item = v.n_entry * v.t.n_layer;
    offset.alloc((size_t)n_item + 1);
    count.alloc((size_t)n_item);
    if (n_item == 0) {
        fill_i32(offset.get(), 0, 1);
        return 0;
    }
    DevBuf<int32_t> bad(1);
    DevBuf<unsigned long long> total64;
    fill_i32(bad.get(), 0, 1);
    // (an item has at most n_layer_s entries: where that bound fits, so does the scan)
    const bool may_wrap = n_item > I32_LIMIT / std::max<int64_t>(v.s.n_layer, 1);
    if (may_wrap) {
        total64.alloc(1);
        XR_HIP(hipMemsetAsync(total64.get(), 0, sizeof(unsigned long long), launch_stream()));
    }
    XR_LAUNCH("layered_count", k_layered_count<PAIRS>, dim3(div_up(v.n_entry, 256)), dim3(256), 0, v, count.get(), bad.get(),
              may_wrap ? total64.get() : (unsigned long long *)nullptr);
    if (PAIRS)
        XR_REQUIRE(read_scalar(bad.get()) == 0, XR_ERR_INVALID, "%s: a pair names a column outside its bounds array", who);
    if (may_wrap) {
        const unsigned long long total = read_scalar(total64.get());
        XR_REQUIRE(total <= (unsigned long long)I32_LIMIT, XR_ERR_LIMIT, "%s: %llu entries exceed the int32 index range", who, total);
    }
    exclusive_scan_i32(count.get(), offset.get(), n_item);
    return read_scalar(offset.get() + n_item);
}

static Layers grid_layers(const double *top, const double *bottom, int64_t n_layer, int64_t col_stride, int64_t n_col) {
    // (n_layer, n_col) arrays, or (n_layer,) taken with a column stride of 0; ids layer * n_col + column
    return Layers{top, bottom, col_stride ? n_col : 1, col_stride, n_col, 1, (int)n_layer};
}

static void check_layers(const char *who, const char *side, const double *top, const double *bottom, int64_t n_layer,
                         int64_t col_stride, int64_t n_col, int64_t limit) {
    XR_REQUIRE(n_layer >= 0, XR_ERR_INVALID, "%s: negative layer count (%s)", who, side);
    XR_REQUIRE(col_stride == 0 || col_stride == 1, XR_ERR_INVALID,
               "%s: column stride must be 1 ((n_layer, n_face) arrays) or 0 ((n_layer,) arrays), received %lld (%s)", who,
               (long long)col_stride, side);
    XR_REQUIRE((top && bottom) || n_layer == 0 || (n_col == 0 && col_stride == 1), XR_ERR_INVALID, "%s: NULL top / bottom (%s)",
               who, side);
    XR_REQUIRE(n_layer == 0 || n_col < limit / n_layer, XR_ERR_LIMIT, "%s: %lld layers x %lld cells exceed the int32 index range (%s)",
               who, (long long)n_layer, (long long)n_col, side);
}

// everything that can be refused is refused here, before anything is uploaded or launched
static void check_layered(const char *who, const xr_csr *w2d, xr_csr **out, const double *top_s, const double *bottom_s,
                          int64_t n_layer_s, int64_t col_stride_s, const double *top_t, const double *bottom_t, int64_t n_layer_t,
                          int64_t col_stride_t) {
    XR_REQUIRE(w2d && out, XR_ERR_INVALID, "%s: NULL argument", who);
    check_layers(who, "source", top_s, bottom_s, n_layer_s, col_stride_s, w2d->m, (int64_t)1 << 31);
    check_layers(who, "target", top_t, bottom_t, n_layer_t, col_stride_t, w2d->n, I32_LIMIT);
    XR_REQUIRE(n_layer_t == 0 || w2d->nnz < I32_LIMIT / n_layer_t, XR_ERR_LIMIT,
               "%s: %lld target layers x %lld entries exceed the int32 index range", who, (long long)n_layer_t, (long long)w2d->nnz);
}

static xr_csr *csr_layered(const xr_csr *w2d, const Layers &s, const Layers &t, bool relative) {
    const char *who = "xr_csr_layered";
    const int64_t n_t = w2d->n, n_s = w2d->m, nnz2d = w2d->nnz;
    Building<xr_csr> csr(OnFailure::WaitFirst); // (the kernels may read the caller's arrays)
    CallerView w;
    caller_view(w2d, w);
    LayeredItems v{};
    v.s = s, v.t = t;
    v.n_entry = nnz2d, v.q_layer = nnz2d, v.q_entry = 1;
    DevBuf<int32_t> row_of((size_t)nnz2d), count, offset;
    if (nnz2d > 0) XR_LAUNCH("layered_row_of", k_layered_row_of, dim3(div_up(n_t, 256)), dim3(256), 0, w.indptr, n_t, row_of.get());
    v.indices = w.indices, v.row_of = row_of.get(), v.data = w.data;
    const int64_t nnz = layered_offsets<false>(v, who, count, offset);

    csr->n = (int64_t)t.n_layer * n_t;
    csr->m = (int64_t)s.n_layer * n_s;
    csr->nnz = nnz;
    csr->indptr.alloc((size_t)csr->n + 1);
    csr->indices.alloc((size_t)nnz);
    csr->data.alloc((size_t)nnz);
    DevBuf<int32_t> is_long((size_t)csr->n + 1), pos((size_t)csr->n + 1);
    XR_LAUNCH("layered_indptr", k_layered_indptr, dim3(div_up(csr->n + 1, 256)), dim3(256), 0, w.indptr, offset.get(), n_t,
              (int64_t)t.n_layer, nnz2d, csr->indptr.get(), is_long.get());
    if (nnz > 0) {
        auto fill = relative ? k_layered_fill<false, true> : k_layered_fill<false, false>;
        XR_LAUNCH("layered_fill", fill, dim3(div_up(nnz2d, 256)), dim3(256), 0, v, offset.get(), count.get(), csr->indices.get(),
                  csr->data.get(), (int64_t *)nullptr, (int64_t *)nullptr);
    }
    // the rows of more than 32 entries, ascending (flags -> scan -> compaction, as the transposed weights list theirs)
    exclusive_scan_i32(is_long.get(), pos.get(), csr->n);
    const int32_t n_long = read_scalar(pos.get() + csr->n);
    if (n_long > 0) { // (counted by the scan: the kernel lists the rows, the count is uploaded)
        csr->longs.begin((size_t)n_long);
        XR_LAUNCH("layered_long_ids", k_compact_ids<int32_t>, dim3(div_up(csr->n, 256)), dim3(256), 0, is_long.get(), pos.get(),
                  csr->n, csr->longs.rows.get());
        h2d(csr->longs.n_dev.get(), &n_long, sizeof(int32_t));
        csr->longs.end(n_long);
    }
    stream_sync();
    return csr.release();
}

} // namespace xr

using namespace xr;

extern "C" {

int xr_csr_layered_dev(const xr_csr *w2d, const double *top_s_dev, const double *bottom_s_dev, int64_t n_layer_s,
                       int64_t col_stride_s, const double *top_t_dev, const double *bottom_t_dev, int64_t n_layer_t,
                       int64_t col_stride_t, int relative, xr_csr **out) {
    XR_API_BEGIN
    check_layered("xr_csr_layered_dev", w2d, out, top_s_dev, bottom_s_dev, n_layer_s, col_stride_s, top_t_dev, bottom_t_dev, n_layer_t,
                  col_stride_t);
    *out = csr_layered(w2d, grid_layers(top_s_dev, bottom_s_dev, n_layer_s, col_stride_s, w2d->m),
                       grid_layers(top_t_dev, bottom_t_dev, n_layer_t, col_stride_t, w2d->n), relative != 0);
    XR_API_END
}

int xr_csr_layered(const xr_csr *w2d, const double *top_s, const double *bottom_s, int64_t n_layer_s, int64_t col_stride_s,
                   const double *top_t, const double *bottom_t, int64_t n_layer_t, int64_t col_stride_t, int relative,
                   xr_csr **out) {
    XR_API_BEGIN
    check_layered("xr_csr_layered", w2d, out, top_s, bottom_s, n_layer_s, col_stride_s, top_t, bottom_t, n_layer_t,
                  col_stride_t);
    const size_t ns = (size_t)n_layer_s * (size_t)(col_stride_s ? w2d->m : 1), nt = (size_t)n_layer_t * (size_t)(col_stride_t ? w2d->n : 1);
    DevBuf<double> ts(ns), bs(ns), tt(nt), bt(nt);
    if (ns > 0) h2d(ts.get(), top_s, ns * sizeof(double)), h2d(bs.get(), bottom_s, ns * sizeof(double));
    if (nt > 0) h2d(tt.get(), top_t, nt * sizeof(double)), h2d(bt.get(), bottom_t, nt * sizeof(double));
    *out = csr_layered(w2d, grid_layers(ts.get(), bs.get(), n_layer_s, col_stride_s, w2d->m),
                       grid_layers(tt.get(), bt.get(), n_layer_t, col_stride_t, w2d->n), relative != 0);
    XR_API_END
}

int xr_overlap_1d_nd_dev(const double *source_bounds_dev, int64_t n, int64_t n_layer_s, const double *target_bounds_dev,
                         int64_t m, int64_t n_layer_t, const int64_t *source_index_dev, const int64_t *target_index_dev,
                         int64_t o, int64_t capacity, int64_t *source_out_dev, int64_t *target_out_dev, double *overlap_out_dev,
                         int64_t *n_out) {
    XR_API_BEGIN
    const char *who = "xr_overlap_1d_nd_dev";
    XR_REQUIRE(n_out && n >= 0 && m >= 0 && n_layer_s >= 0 && n_layer_t >= 0 && o >= 0 && capacity >= 0, XR_ERR_INVALID,
               "%s: invalid argument", who);
    XR_REQUIRE(o == 0 || (source_index_dev && target_index_dev), XR_ERR_INVALID, "%s: NULL index", who);
    XR_REQUIRE((source_bounds_dev || n * n_layer_s == 0) && (target_bounds_dev || m * n_layer_t == 0), XR_ERR_INVALID,
               "%s: NULL bounds", who);
    XR_REQUIRE(capacity == 0 || (source_out_dev && target_out_dev && overlap_out_dev), XR_ERR_INVALID, "%s: NULL output", who);
    XR_REQUIRE(n_layer_t == 0 || o < I32_LIMIT / n_layer_t, XR_ERR_LIMIT, "%s: %lld pairs x %lld target layers exceed the int32 index range",
               who, (long long)o, (long long)n_layer_t);
    XR_REQUIRE(n_layer_s < I32_LIMIT, XR_ERR_LIMIT, "%s: too many source layers", who);
    LayeredItems v{};
    // bounds (column, layer, 2): [.., 0] the lower, [.., 1] the upper bound; ids column * n_layer + layer
    v.s = Layers{source_bounds_dev + 1, source_bounds_dev, 2, 2 * n_layer_s, 1, n_layer_s, (int)n_layer_s};
    v.t = Layers{target_bounds_dev + 1, target_bounds_dev, 2, 2 * n_layer_t, 1, n_layer_t, (int)n_layer_t};
    v.n_entry = o, v.q_layer = 1, v.q_entry = n_layer_t;
    v.source_index = source_index_dev, v.target_index = target_index_dev;
    v.n_source_col = n, v.n_target_col = m;
    DevBuf<int32_t> count, offset;
    struct Drain { // (the kernels read the caller's arrays: nothing in flight when the call returns, error or not)
        ~Drain() {
            try {
                stream_sync();
            } catch (const Failure &) {
            }
        }
    } drain;
    const int64_t total = layered_offsets<true>(v, who, count, offset);
    *n_out = total;
    if (total > 0 && capacity >= total)
        XR_LAUNCH("layered_fill", (k_layered_fill<true, false>), dim3(div_up(o, 256)), dim3(256), 0, v, offset.get(), count.get(),
                  (int32_t *)nullptr, overlap_out_dev, source_out_dev, target_out_dev);
    XR_API_END
}

} // extern "C"
