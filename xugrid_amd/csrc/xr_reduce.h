// xr_reduce.h -- the reducers of xugrid/regrid/reduce.py as the apply units share them: the streaming states `Red<METHOD>` with
// their wave / block / group merges (xr_apply_stream.hip, xr_outer.hip), the partial states of the shard-decomposable reducers
// (xr_partial.hip; their component layout is part of include/xugrid_amd.h) and the tables that turn a run-time reducer id
// into a template argument.  Two codings of the same reducers with different component layouts: they are not interchangeable.
// No kernels and no launches here.
#pragma once
#include <type_traits>

#include "xr_apply.h"

namespace xr {

template <typename SRC> __device__ __forceinline__ double ld_src(const SRC *p, int64_t i) { return (double)p[i]; }

// ---------------------------------------------------------------------------------------------
// streaming reducers: constant-size state per (row, k), one pass over the row
// ---------------------------------------------------------------------------------------------
// State = up to three doubles (a, b, c) so that partial states can be shuffled between lanes and
// merged (long rows are reduced by a whole block, see k_apply_long).
template <int METHOD> struct Red;

template <> struct Red<XR_MEAN> { // reduce.py:16-27   a = sum w v, b = sum w
    double a = 0.0, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        const bool ok = v == v; // select instead of branch: lanes stay converged
        const double na = a + w * v, nb = b + w;
        a = ok ? na : a;
        b = ok ? nb : b;
    }
    __device__ void merge(const Red &o) { a += o.a; b += o.b; }
    __device__ double fin() const { return b == 0 ? NAN : a / b; }
};
template <> struct Red<XR_HARMONIC_MEAN> { // reduce.py:30-42   a = sum w / v, b = sum w
    double a = 0.0, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        if (v != v || v == 0) return;
        if (w > 0) {
            b += w;
            a += w / v;
        }
    }
    __device__ void merge(const Red &o) { a += o.a; b += o.b; }
    __device__ double fin() const { return (a == 0 || b == 0) ? NAN : b / a; }
};
template <> struct Red<XR_GEOMETRIC_MEAN> { // reduce.py:45-72; normsum = sum of ALL row weights
    double a = 0.0, b = 0.0, c = 0.0;        // a = sum wn ln v, b = sum wn, c = 1 if a negative value was seen
    __device__ void add(double v, double w, double normsum) {
        if (c != 0.0) return;
        const double wn = w / normsum;
        if (v > 0 && wn > 0) {
            a += wn * log(fabs(v));
            b += wn;
        } else if (v < 0) {
            c = 1.0;
        }
    }
    __device__ void merge(const Red &o) { a += o.a; b += o.b; if (o.c != 0.0) c = 1.0; }
    __device__ double fin() const { return (c != 0.0 || b == 0) ? NAN : exp((1.0 / b) * a); }
};
template <> struct Red<XR_SUM> { // reduce.py:75-87   a = sum v, b = sum w
    double a = 0.0, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        const bool ok = v == v;
        const double na = a + v, nb = b + w;
        a = ok ? na : a;
        b = ok ? nb : b;
    }
    __device__ void merge(const Red &o) { a += o.a; b += o.b; }
    __device__ double fin() const { return b == 0 ? NAN : a; }
};
template <> struct Red<XR_MINIMUM> { // reduce.py:90-106   a = min v, b = max w
    double a = INFINITY, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        const bool ok = v == v;
        a = (ok && v < a) ? v : a;
        b = (ok && w > b) ? w : b;
    }
    __device__ void merge(const Red &o) { if (o.a < a) a = o.a; if (o.b > b) b = o.b; }
    __device__ double fin() const { return b == 0.0 ? NAN : a; }
};
template <> struct Red<XR_MAXIMUM> { // reduce.py:109-123   a = max v, b = max w
    double a = -INFINITY, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        const bool ok = v == v;
        a = (ok && v > a) ? v : a;
        b = (ok && w > b) ? w : b;
    }
    __device__ void merge(const Red &o) { if (o.a > a) a = o.a; if (o.b > b) b = o.b; }
    __device__ double fin() const { return b == 0.0 ? NAN : a; }
};
template <> struct Red<XR_FIRST_ORDER_CONSERVATIVE> { // reduce.py:206-222   a = sum v w, b = sum w
    double a = 0.0, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        const bool ok = v == v;
        const double na = a + v * w, nb = b + w;
        a = ok ? na : a;
        b = ok ? nb : b;
    }
    __device__ void merge(const Red &o) { a += o.a; b += o.b; }
    __device__ double fin() const { return b == 0 ? NAN : a; }
};
template <> struct Red<XR_MAX_OVERLAP> { // reduce.py:225-238   a = value of the largest weight b
    double a = -INFINITY, b = 0.0, c = 0.0;
    __device__ void add(double v, double w, double) {
        const bool take = (v == v) && ((w > b) || (w == b && v > a));
        b = take ? w : b;
        a = take ? v : a;
    }
    __device__ void merge(const Red &o) {
        if ((o.b > b) || (o.b == b && o.a > a)) {
            b = o.b;
            a = o.a;
        }
    }
    __device__ double fin() const { return b == 0.0 ? NAN : a; }
};

template <> struct Red<XR_SELECT> { // regridder.py:400-409 on CSR rows: the last entry wins, NaN included
    double a = NAN, b = 0.0, c = 0.0;
    __device__ void add(double v, double, double) {
        a = v;
        b = 1.0;
    }
    __device__ void merge(const Red &o) {
        if (o.b != 0.0) {
            a = o.a;
            b = 1.0;
        }
    }
    __device__ double fin() const { return a; }
};

template <int METHOD> __device__ __forceinline__ void wave_merge(Red<METHOD> &r) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        Red<METHOD> o;
        o.a = __shfl_xor(r.a, d, 64);
        o.b = __shfl_xor(r.b, d, 64);
        o.c = __shfl_xor(r.c, d, 64);
        if ((lane & d) == 0) { // lane-independent order: every lane ends with the same value
            r.merge(o);
        } else {
            o.merge(r);
            r = o;
        }
    }
}

template <int METHOD> __device__ __forceinline__ void block_merge(Red<METHOD> &r, double (*lds)[3]) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        Red<METHOD> o;
        o.a = __shfl_xor(r.a, d, 64);
        o.b = __shfl_xor(r.b, d, 64);
        o.c = __shfl_xor(r.c, d, 64);
        // merge in a lane-independent order so that every lane holds the same value
        if ((threadIdx.x & d) == 0) {
            r.merge(o);
        } else {
            o.merge(r);
            r = o;
        }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        lds[wave][0] = r.a;
        lds[wave][1] = r.b;
        lds[wave][2] = r.c;
    }
    __syncthreads();
    Red<METHOD> t;
    t.a = lds[0][0]; t.b = lds[0][1]; t.c = lds[0][2];
#pragma unroll
    for (int w = 1; w < AP_BLOCK / 64; w++) {
        Red<METHOD> o;
        o.a = lds[w][0]; o.b = lds[w][1]; o.c = lds[w][2];
        t.merge(o);
    }
    r = t;
}

// ... by a group of G lanes (apply_row_group, xr_apply_stream.hip)
template <int METHOD, int G> __device__ __forceinline__ void group_merge(Red<METHOD> &r) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) {
        Red<METHOD> o;
        o.a = __shfl_xor(r.a, d, 64);
        o.b = __shfl_xor(r.b, d, 64);
        o.c = __shfl_xor(r.c, d, 64);
        if ((lane & d) == 0) { // lane-independent order: every lane of the group ends with the same value
            r.merge(o);
        } else {
            o.merge(r);
            r = o;
        }
    }
}

// ---- partial states of every shard-decomposable reducer (multi-GPU split over the source faces) ------------------
// (reduce.py:16-123, 206-222; component table in include/xugrid_amd.h)
__host__ __device__ constexpr int partial_components(int method) {
    switch (method) {
    case XR_MEAN: case XR_FIRST_ORDER_CONSERVATIVE: case XR_SUM: case XR_HARMONIC_MEAN: case XR_MINIMUM: case XR_MAXIMUM: return 2;
    case XR_GEOMETRIC_MEAN: return 4;
    default: return 0;
    }
}
__host__ __device__ constexpr bool partial_is_max(int method) { return method == XR_MINIMUM || method == XR_MAXIMUM; }

struct PartialState {
    double c[4];
};
__device__ __forceinline__ PartialState partial_identity(int method) {
    PartialState st{{0.0, 0.0, 0.0, 0.0}};
    if (partial_is_max(method)) st.c[0] = -INFINITY;
    return st;
}
__device__ __forceinline__ void partial_add(int method, PartialState &st, double v, double w) {
    switch (method) {
    case XR_MEAN: case XR_FIRST_ORDER_CONSERVATIVE:
        if (v == v) { st.c[0] += w * v; st.c[1] += w; }
        break;
    case XR_SUM:
        if (v == v) { st.c[0] += v; st.c[1] += w; }
        break;
    case XR_HARMONIC_MEAN:
        if (v == v && v != 0 && w > 0) { st.c[0] += w; st.c[1] += w / v; }
        break;
    case XR_GEOMETRIC_MEAN:
        st.c[0] += w;
        if (v > 0 && w > 0) { st.c[1] += w * log(fabs(v)); st.c[2] += w; }
        else if (v < 0) st.c[3] += 1.0;
        break;
    case XR_MINIMUM:
        if (v == v) { st.c[0] = fmax(st.c[0], -v); st.c[1] = fmax(st.c[1], w); }
        break;
    case XR_MAXIMUM:
        if (v == v) { st.c[0] = fmax(st.c[0], v); st.c[1] = fmax(st.c[1], w); }
        break;
    }
}
__device__ __forceinline__ void partial_combine(int method, PartialState &a, const double *b, int64_t stride, int C) {
    // (static component indices: a loop over the run-time C puts the state into scratch memory)
    if (partial_is_max(method)) {
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < C) a.c[c] = fmax(a.c[c], b[c * stride]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < C) a.c[c] += b[c * stride];
    }
}
__device__ __forceinline__ double partial_finalize(int method, const PartialState &st) {
    switch (method) {
    case XR_MEAN: return st.c[1] == 0 ? NAN : st.c[0] / st.c[1];
    case XR_FIRST_ORDER_CONSERVATIVE: case XR_SUM: return st.c[1] == 0 ? NAN : st.c[0];
    case XR_HARMONIC_MEAN: return (st.c[1] == 0 || st.c[0] == 0) ? NAN : st.c[0] / st.c[1];
    case XR_GEOMETRIC_MEAN:
        // (the reference normalises the weights by their sum first: exp(sum (w / W) ln v / sum (w / W)) -- the same
        // number up to rounding)
        if (st.c[0] == 0 || st.c[3] > 0 || st.c[2] == 0) return NAN;
        return exp((1.0 / (st.c[2] / st.c[0])) * (st.c[1] / st.c[0]));
    case XR_MINIMUM: return st.c[1] == 0 ? NAN : -st.c[0];
    case XR_MAXIMUM: return st.c[1] == 0 ? NAN : st.c[0];
    }
    return NAN;
}

// ---- host dispatch: run-time source dtype and reducer ids -> template arguments.  Every table below is the only one of
// its kind; a reducer a kernel family does not serve is excluded with `if constexpr`, never instantiated.

// (with_source_type, the table of the source dtypes, is in xr_internal.h: xr_sample.hip gathers through it too)

// f(std::integral_constant<int, ID>()) for the ID of IDS that equals `id`; false if there is none
template <int... IDS, typename F> static bool with_id(int id, F &&f) {
    return ((id == IDS && (f(std::integral_constant<int, IDS>()), true)) || ...);
}

// every reducer
template <typename F> static void with_reducer(int method, F &&f) {
    const bool known = with_id<XR_MEAN, XR_HARMONIC_MEAN, XR_GEOMETRIC_MEAN, XR_SUM, XR_MINIMUM, XR_MAXIMUM, XR_MODE,
                               XR_PERCENTILE, XR_FIRST_ORDER_CONSERVATIVE, XR_MAX_OVERLAP, XR_SELECT>(method, f);
    XR_REQUIRE(known, XR_ERR_INVALID, "unknown reducer id %d", method);
}

// mode and percentiles need a row's values side by side (launch_workspace); every other reducer streams over a row
template <int METHOD> constexpr bool streamed_reducer = METHOD != XR_MODE && METHOD != XR_PERCENTILE;

// the reducers whose partial states combine over source shards (partial_components > 0)
template <typename F> static void with_decomposable(int method, F &&f) {
    const bool known = with_id<XR_MEAN, XR_FIRST_ORDER_CONSERVATIVE, XR_SUM, XR_HARMONIC_MEAN, XR_GEOMETRIC_MEAN,
                               XR_MINIMUM, XR_MAXIMUM>(method, f);
    XR_REQUIRE(known, XR_ERR_INVALID, "reducer %d does not decompose over source shards", method);
}

} // namespace xr
