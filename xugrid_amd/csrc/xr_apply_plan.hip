// xr_apply_plan.hip -- the apply plan of the many-variable apply (K >= PLAN_KT): blocked CSR with per-block distinct-column
// lists; its builder, the kernel that applies it, and ensure_plan, which attaches it to a matrix.
//
// A block of 256 spatially adjacent rows references ~5x fewer DISTINCT source faces than it has
// entries.  With many source variables the gathers dominate, so each distinct source value is
// loaded ONCE per (block, variable) -- lanes run over the ascending column list, neighbours share
// cache lines -- into LDS, and the rows are reduced from LDS through 16-bit local indices.
// The blocks the plan cannot take and the long rows stay with the streamed kernels (launch_stream, xr_apply_stream.hip).
#include <vector>

#include "xr_apply.h"
#include "xr_reduce.h"
#include "xr_prims.h"

namespace xr {

static constexpr int PLAN_LMAX = 4096; // entries of a block the builder can sort in LDS
static constexpr int PLAN_UMAX = 512;  // distinct columns per block kept in the plan

// MERGED plan (round 5): ONE distinct-column list per GROUP of PLAN_GROUP neighbouring row blocks.  On a qhull-numbered mesh a
// block of 256 rows uses ~4 of the 16 values of every source line it touches, a group of 512 rows 4.5, of 1024 rows 5 (66 / 52
// lines per 256 rows instead of 85: profiles/r05_experiments/analysis_column_locality.*): the group's workgroup gathers every
// line once for all its row blocks.  (Blocks in lockstep with a list EACH -- XR_PLAN_SUBS -- do not get there: the lines in
// flight, 4 x 85 x 8 variables x 128 bytes, are ten times the L1, the siblings' requests miss again.)  Groups of two and of four
// measured the same on the benchmark matrix (K = 256: 1.64 -> 1.53 / 1.56 ms: what the larger group saves in line fills its
// 16-wave barriers cost); two blocks need 58 KB of LDS (two workgroups per CU) and cost a lattice-numbered matrix 2 %, four 7 %.
static constexpr int PLAN_GROUP = 2;
static constexpr int PLAN_GUMAX = 1024; // distinct columns per group kept in the plan

// The builder: one workgroup per list, GROUP == 1 a list per row block, GROUP == PLAN_GROUP a list per group of row blocks.
// Sorts the columns of the list's entries in LDS, keeps the distinct ones (ucol, nuniq) and gives every entry its 16-bit
// position among them (loc).  A list is planned iff every one of its row blocks has at most entry_cap entries -- the apply
// stages a row block's entries in LDS -- and its distinct columns fit the value table; otherwise nuniq = -1 and every row block
// of the list goes on the unplanned list (k_apply_direct takes those).
// max_entries: [0] entries of the largest planned row block; [2], [3] distinct columns and distinct 128-byte source lines,
// summed over the planned blocks (GROUP == 1 only: they decide whether a merged plan pays, ensure_plan).
template <int GROUP>
__global__ void __launch_bounds__(AP_BLOCK * GROUP)
k_plan_build(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t T,
             int32_t *__restrict__ ucol, int32_t *__restrict__ nuniq, uint16_t *__restrict__ loc,
             int32_t *__restrict__ max_entries, int32_t *__restrict__ unplanned, int32_t *__restrict__ n_unplanned,
             int entry_cap) {
    static_assert(GROUP == 1 || GROUP == PLAN_GROUP, "a list per row block or per group of PLAN_GROUP");
    constexpr int NT = AP_BLOCK * GROUP;                        // threads
    constexpr int KMAX = PLAN_LMAX * GROUP;                     // keys the workgroup can sort
    constexpr int UMAX = GROUP == 1 ? PLAN_UMAX : PLAN_GUMAX;   // distinct columns of a list
    __shared__ int32_t keys[KMAX];
    __shared__ int32_t uniq[UMAX];
    __shared__ int32_t sh_wave[NT / 64];
    const int64_t n_blocks = (T + AP_BLOCK - 1) / AP_BLOCK;
    const int64_t b0 = (int64_t)blockIdx.x * GROUP;
    const int64_t row0 = b0 * AP_BLOCK;
    const int64_t row_end = row0 + NT < T ? row0 + NT : T;
    const int seg0 = indptr[row0], seg1 = indptr[row_end];
    const int n = seg1 - seg0;
    // entries of the list's row block g (0: past the last row block)
    auto block_entries = [&](int g) -> int {
        const int64_t r0 = row0 + (int64_t)g * AP_BLOCK;
        if (r0 >= T) return 0;
        const int64_t r1 = r0 + AP_BLOCK < T ? r0 + AP_BLOCK : T;
        return indptr[r1] - indptr[r0];
    };
    auto give_up = [&]() {
        if (threadIdx.x == 0) {
            nuniq[blockIdx.x] = -1;
            for (int g = 0; g < GROUP; g++)
                if (b0 + g < n_blocks) unplanned[atomicAdd(n_unplanned, 1)] = (int32_t)(b0 + g);
        }
    };
    // every row block of the list has to fit the apply's per-block stage (uniform: every thread looks, all leave together)
    bool too_long = false;
#pragma unroll
    for (int g = 0; g < GROUP; g++) too_long |= block_entries(g) > entry_cap;
    if (too_long || n > KMAX) { // (n > KMAX: a guard; it cannot fire while entry_cap <= PLAN_LMAX)
        give_up();
        return;
    }
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += NT) keys[i] = i < n ? indices[seg0 + i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1) { // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // unique: each thread owns a contiguous slice of the sorted keys
    const int per = (n + NT - 1) / NT;
    const int a0 = threadIdx.x * per < n ? threadIdx.x * per : n, a1 = a0 + per < n ? a0 + per : n;
    int cnt = 0;
    for (int i = a0; i < a1; i++) cnt += (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(cnt);
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        if (w < wave) woff += sh_wave[w];
        total += sh_wave[w];
    }
    if (total > UMAX) {
        give_up();
        return;
    }
    int pos = woff + incl - cnt;
    for (int i = a0; i < a1; i++)
        if (i == 0 || keys[i] != keys[i - 1]) uniq[pos++] = keys[i];
    __syncthreads();
    for (int u = threadIdx.x; u < total; u += NT) ucol[(int64_t)blockIdx.x * UMAX + u] = uniq[u];
    if constexpr (GROUP == 1) {
        // how well the block uses the source lines it touches (16 values of 8 bytes per 128-byte line): the sums over all blocks
        // decide whether a merged plan pays (ensure_plan)
        __shared__ int32_t sh_lines;
        if (threadIdx.x == 0) sh_lines = 0;
        __syncthreads();
        int mine = 0;
        for (int u = threadIdx.x; u < total; u += NT) mine += (u == 0 || (uniq[u] >> 4) != (uniq[u - 1] >> 4)) ? 1 : 0;
        if (mine) atomicAdd(&sh_lines, mine);
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(max_entries + 2, total);
            atomicAdd(max_entries + 3, sh_lines);
        }
    }
    // the apply kernel sizes its per-block stage for the largest planned block
    if ((int)threadIdx.x < GROUP && b0 + threadIdx.x < n_blocks) atomicMax(max_entries, block_entries((int)threadIdx.x));
    if (threadIdx.x == 0) nuniq[blockIdx.x] = total;
    for (int i = threadIdx.x; i < n; i += NT) { // local index of every entry: binary search in the distinct list
        const int c = indices[seg0 + i];
        int lo = 0, hi = total - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (uniq[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        loc[seg0 + i] = (uint16_t)lo;
    }
}

// One block = 256 stored rows, ALL variables: the block's CSR entries (weight + 16-bit local column)
// are staged in LDS once, then the block walks the variables in tiles of KTILE.  Software pipeline
// (global -> registers -> LDS): the distinct source values of tile i+1 are requested into registers
// before tile i is reduced, and written to LDS after it -- HBM latency overlaps the reduction, so one
// resident block per CU is enough to keep its share of the memory system busy.
// SUBS > 1 (round 5): one workgroup = SUBS neighbouring row blocks (SUBS x 256 threads, every sub-block with its own plan and its
// own LDS region) that walk the variable tiles in LOCKSTEP -- the group's barriers are the workgroup's.  On a mesh whose
// numbering is coherent but not compact (qhull) a row block uses ~4 of the 16 source values of a 128-byte line and its
// neighbours use the rest: as separate workgroups they drift apart and every one of them fetches the line on its own -- the L1
// of a CU holds 256 lines, the L2 of an XCD four microseconds of traffic --, in lockstep on ONE CU the requests for a line meet
// in that CU's L1.
// FAST (round 6; opt-in for `mean` / `first_order_conservative`: option "apply_contract"): on NaN-free tiles the
// products are CONTRACTED into the running sums (one fused multiply-add per entry and variable instead of a multiplication and
// an addition) and the mean is the sum times ONE reciprocal of the row's weight sum (computed once per row, outside the loop
// over the variable tiles) instead of an IEEE division per variable -- the reduction was the kernel's floor (0.71-0.81 ms of
// vector work per K = 256 apply against 0.52 ms of memory time).  The results then differ from the reference's sequential
// loop (regridder.py:41-67) by the roundings of at most n products (n = entries of the row, 4 on average) and one
// multiplication: <= (n + 2) ulp of sum |w v| / sum w -- measured at full size 8e-16 of the field's range, but 1e-9 RELATIVE where a
// mean of mixed-sign data cancels to ~1e-7 of that range.  What it buys (profiles/r06_apply_fast_ab.txt): K = 256 on the
// lattice-numbered pair 1.01 -> 0.92 ms (50 -> 56 % of HBM), on the qhull-numbered benchmark matrix 1.57 -> 1.53 ms (that one is
// bound by its line fills, not by the reduction).  The default stays the reference's operation order, bit for bit.
// The staged tile of distinct source values in LDS is VARIABLE-minor (round 6): the KTILE values of a column in KTILE / 2 consecutive
// 16-byte slots, read with ds_read_b128 (which reaches its rate from one wave per SIMD; ds_read_b64 needs ~4 and the kernel has 3) --
// the slot of a pair XOR-swizzled with the column so that, for a fixed pair, the columns spread over all 16 slot positions of a
// 256-byte LDS row.  Until round 5 it was variable-MAJOR (vals[kk][u]: a ds_read_b64 at a random column per variable).  Same values,
// same arithmetic; measured with gathers and stores off (option plan_dbg = 3, the reduction's floor): merged plan 0.785 -> 0.685 ms,
// per-block plan 0.588 -> 0.502 ms per K = 256 apply; whole kernel - 1.5 ... 2 % (profiles/r06_experiments/apply_lds_layout_ab.txt).
template <int KTILE> __device__ __forceinline__ int plan_slot(int u, int k2) {
    static_assert(KTILE == 8 || KTILE == 4, "tiles of 4 or 8 variables");
    return KTILE == 8 ? u * 4 + (k2 ^ ((u >> 2) & 3)) : u * 2 + (k2 ^ ((u >> 3) & 1));
}
// the KTILE staged values of local column l
template <int KTILE> __device__ __forceinline__ void plan_read(const double *vals, int l, double (&v)[KTILE]) {
#pragma unroll
    for (int k2 = 0; k2 < KTILE / 2; k2++) {
        const double2 t2 = reinterpret_cast<const double2 *>(vals)[plan_slot<KTILE>(l, k2)];
        v[2 * k2] = t2.x;
        v[2 * k2 + 1] = t2.y;
    }
}
template <int METHOD, typename SRC, int KTILE, int SUBS, bool MERGE = false, bool FAST = false>
__global__ void __launch_bounds__(AP_BLOCK * SUBS)
k_apply_plan(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
             const int32_t *__restrict__ ucol, const int32_t *__restrict__ nuniq, const uint16_t *__restrict__ loc,
             const int32_t *__restrict__ row_order, bool skip_long, int64_t T, int64_t S,
             const SRC *__restrict__ source, int64_t K, double *__restrict__ out, int lmax, int super_blocks, int item_tiles, int dbg) {
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const int sub = SUBS > 1 ? (int)threadIdx.x / AP_BLOCK : 0, tid = SUBS > 1 ? (int)threadIdx.x % AP_BLOCK : (int)threadIdx.x;
    // MERGE: ONE value table for the workgroup (the group's distinct columns), the entries of every row block behind it
    static_assert(!MERGE || SUBS == PLAN_GROUP, "a merged plan is built for groups of PLAN_GROUP row blocks");
    constexpr int UMAX = MERGE ? PLAN_GUMAX : PLAN_UMAX;                  // columns of the value table
    constexpr int GATHERERS = MERGE ? AP_BLOCK * SUBS : AP_BLOCK;         // threads that share a list
    const size_t stage_bytes = ((sizeof(double) * (size_t)lmax + sizeof(uint16_t) * (size_t)lmax) + 15) / 16 * 16;
    char *smem = MERGE ? smem_all
                       : smem_all + (size_t)sub * (((sizeof(double) * (KTILE * PLAN_UMAX + lmax) + sizeof(uint16_t) * lmax) + 15) / 16 * 16);
    double *vals = reinterpret_cast<double *>(smem);                      // [UMAX][KTILE / 2] 16-byte slots, swizzled (plan_slot)
    double *sh_w = MERGE ? reinterpret_cast<double *>(smem_all + sizeof(double) * KTILE * UMAX + (size_t)sub * stage_bytes)
                         : vals + KTILE * PLAN_UMAX;                      // [lmax] = entries of the largest planned block
    uint16_t *sh_loc = reinterpret_cast<uint16_t *>(sh_w + lmax);         // [lmax]
    constexpr int UPT = UMAX / GATHERERS;                                 // distinct columns per thread
    const int gtid = MERGE ? (int)threadIdx.x : tid;                      // index among the threads that share the list
    // XCD-aware block order: hardware block b runs on XCD b % 8; give every XCD a CONTIGUOUS range of
    // row blocks (= one spatial region), so that lines shared by neighbouring blocks stay in one L2
    const int64_t n_blocks = (T + AP_BLOCK - 1) / AP_BLOCK;           // row blocks
    const int64_t n_groups = (n_blocks + SUBS - 1) / SUBS;            // workgroups' worth of them
    const int64_t per_xcd = (n_groups + 7) / 8;
    int64_t lg = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    int64_t k_begin = 0, k_end = K;
    if (super_blocks > 0) {
        // L2-blocked order (round 5).  A block of 256 rows uses ~4 of the 16 source values of every 128-byte line it touches
        // (a qhull-numbered mesh: spatial neighbours are not id neighbours); the rest of the line belongs to NEIGHBOURING row
        // blocks, and a block that walks all K variables on its own drifts away from them -- the line comes from HBM once per
        // block (PMC, K = 128: 24 M fabric reads against 7 M for a lattice-numbered pair).  Here a work item is one row block x
        // `item_tiles` variable tiles, and an XCD's items are ordered (super tile of `super_blocks` neighbouring row blocks) ->
        // (variable item) -> (row block): the blocks resident on an XCD at any time share one super tile and one variable
        // item, whose source lines (~1.4 MB for 64 blocks x 8 variables) stay in that XCD's 4 MB L2.
        const int64_t n_items = (K + (int64_t)KTILE * item_tiles - 1) / ((int64_t)KTILE * item_tiles);
        const int64_t i = blockIdx.x >> 3;
        const int64_t per_super = (int64_t)super_blocks * n_items;
        const int64_t sup = i / per_super, rem = i - sup * per_super;
        const int64_t item = rem / super_blocks, b = rem - item * super_blocks;
        const int64_t local = sup * super_blocks + b;
        if (local >= per_xcd) return;
        lg = (int64_t)(blockIdx.x & 7) * per_xcd + local;
        k_begin = item * KTILE * item_tiles;
        k_end = k_begin + (int64_t)KTILE * item_tiles < K ? k_begin + (int64_t)KTILE * item_tiles : K;
    }
    if (lg >= n_groups) return; // (uniform over the workgroup)
    const int64_t lb = lg * SUBS + sub;
    // (a sub-block without work -- past the last row block, or unplanned: too many entries / distinct columns, k_apply_direct takes
    // those over its block list -- stays for the workgroup's barriers; SUBS == 1: it leaves)
    const int64_t row0 = (lb < n_blocks ? lb : 0) * AP_BLOCK;
    const int nu = MERGE ? nuniq[lg] : (lb < n_blocks ? nuniq[lb] : -1);
    if ((SUBS == 1 || MERGE) && nu < 0) return; // (uniform over the workgroup)
    const bool active = nu >= 0 && lb < n_blocks;
    const int64_t t = active ? row0 + tid : T;
    const int64_t row_end = row0 + AP_BLOCK < T ? row0 + AP_BLOCK : T;
    int s = 0, e = 0;
    if (t < T) {
        s = indptr[t];
        e = indptr[t + 1];
    }
    const bool is_long = skip_long && (e - s > APPLY_LONG); // reduced by k_apply_long
    const int64_t t_out = (t < T && row_order) ? (int64_t)row_order[t] : t;
    // stage the block's entries once
    const int seg0 = indptr[row0], seg1 = active ? indptr[row_end] : seg0;
    for (int j = seg0 + tid; j < seg1; j += AP_BLOCK) {
        sh_w[j - seg0] = data[j];
        sh_loc[j - seg0] = loc[j];
    }
    // this thread's distinct columns
    int64_t mycol[UPT];
#pragma unroll
    for (int q = 0; q < UPT; q++) {
        const int u = q * GATHERERS + gtid;
        mycol[q] = (u < nu && !(dbg & 1)) ? (int64_t)ucol[(MERGE ? lg : lb) * UMAX + u] : -1; // (dbg: measurement switches, XR_PLAN_DBG)
    }
    __syncthreads();
    double normsum = 0.0;
    if (METHOD == XR_GEOMETRIC_MEAN && !is_long)
        for (int j = s; j < e; j++) normsum += sh_w[j - seg0];
    double wsum_row = 0.0; // sum of the row's weights in entry order (= Red::b when no value is NaN)
    if (!is_long)
        for (int j = s; j < e; j++) wsum_row += sh_w[j - seg0];
    const double inv_wsum = FAST ? 1.0 / wsum_row : 0.0; // (FAST: one division per row for all K variables)
    // prologue: request tile 0
    double stage[UPT][KTILE];
    {
        const int kn = (int)(k_end - k_begin < KTILE ? k_end - k_begin : KTILE);
        const SRC *src0 = source + k_begin * S;
#pragma unroll
        for (int q = 0; q < UPT; q++)
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++)
                stage[q][kk] = (mycol[q] >= 0 && kk < kn) ? ld_src(src0, (int64_t)kk * S + mycol[q]) : 0.0;
    }
    for (int64_t k0 = k_begin; k0 < k_end; k0 += KTILE) {
        const int kn = (int)((k_end - k0) < KTILE ? (k_end - k0) : KTILE);
        __syncthreads(); // everybody finished reading the previous tile
        int my_nan = 0;
#pragma unroll
        for (int q = 0; q < UPT; q++) {
            const int u = q * GATHERERS + gtid;
            if (u < nu) {
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++) my_nan |= (stage[q][kk] != stage[q][kk]) ? 1 : 0;
#pragma unroll
                for (int k2 = 0; k2 < KTILE / 2; k2++)
                    reinterpret_cast<double2 *>(vals)[plan_slot<KTILE>(u, k2)] = make_double2(stage[q][2 * k2], stage[q][2 * k2 + 1]);
            }
        }
        // block-uniform: does this tile hold any NaN?  (NaN-free tiles take the short path below)
        const bool tile_has_nan = __syncthreads_or(my_nan) != 0;
        // request the next tile while this one is reduced
        const int64_t k1 = k0 + KTILE;
        if (k1 < k_end) {
            const int kn1 = (int)((k_end - k1) < KTILE ? (k_end - k1) : KTILE);
            const SRC *src1 = source + k1 * S;
#pragma unroll
            for (int q = 0; q < UPT; q++)
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++)
                    stage[q][kk] = (mycol[q] >= 0 && kk < kn1) ? ld_src(src1, (int64_t)kk * S + mycol[q]) : 0.0;
        }
        constexpr bool LINEAR = METHOD == XR_MEAN || METHOD == XR_SUM || METHOD == XR_FIRST_ORDER_CONSERVATIVE;
        if (LINEAR && !tile_has_nan) {
            // no NaN anywhere in the tile: the weight sum of a row is the same for every variable
            // (computed once, wsum_row) and the value sums need no per-entry test.  Same additions
            // in the same order as the general path -> bit-identical results.
            if (t < T && !is_long) {
                double acc[KTILE];
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++) acc[kk] = 0.0;
                for (int j = s - seg0; j < e - seg0; j++) {
                    const int l = sh_loc[j];
                    const double w = sh_w[j];
                    double v[KTILE];
                    plan_read<KTILE>(vals, l, v);
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++) {
                        if (METHOD == XR_SUM) acc[kk] += v[kk];
                        else if (FAST) acc[kk] = fma(w, v[kk], acc[kk]);
                        else if (METHOD == XR_MEAN) acc[kk] += w * v[kk];
                        else acc[kk] += v[kk] * w;
                    }
                }
                if (FAST && METHOD == XR_MEAN) {
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++) acc[kk] *= inv_wsum;
                }
                const bool defined = e > s && wsum_row != 0;
                double *o = out + k0 * T + t_out;
                if (dbg & 2) { // (measurement: no stores -- the compiler must not know)
                    if (acc[0] != 12345.678) continue;
                }
                if (kn == KTILE && !(dbg & 4)) {
                    // whole tile: no per-variable branch around the stores.  Non-temporal: the result is written once and not
                    // read here -- it should not push the source lines that neighbouring row blocks still need out of the L2
                    // (1M x 1M, K = 256: 1.52 -> 1.44 ms qhull-numbered, 1.04 -> 0.99 ms lattice-numbered; XR_PLAN_DBG=4: plain stores)
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++)
                        __builtin_nontemporal_store(defined ? (METHOD == XR_MEAN && !FAST ? acc[kk] / wsum_row : acc[kk]) : NAN, &o[kk * T]);
                } else if (kn == KTILE) {
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++) o[kk * T] = defined ? (METHOD == XR_MEAN && !FAST ? acc[kk] / wsum_row : acc[kk]) : NAN;
                } else {
#pragma unroll
                    for (int kk = 0; kk < KTILE; kk++)
                        if (kk < kn) o[kk * T] = defined ? (METHOD == XR_MEAN && !FAST ? acc[kk] / wsum_row : acc[kk]) : NAN;
                }
            }
        } else if (t < T && !is_long) {
            Red<METHOD> red[KTILE];
            for (int j = s - seg0; j < e - seg0; j++) {
                const int l = sh_loc[j];
                const double w = sh_w[j];
                double v[KTILE];
                plan_read<KTILE>(vals, l, v);
#pragma unroll
                for (int kk = 0; kk < KTILE; kk++)
                    if (kk < kn) red[kk].add(v[kk], w, normsum);
            }
#pragma unroll
            for (int kk = 0; kk < KTILE; kk++) {
                if (kk < kn) {
                    double r = NAN;
                    if (e > s) {
                        r = red[kk].fin();
                        if (METHOD == XR_GEOMETRIC_MEAN && normsum == 0) r = NAN;
                    }
                    out[(k0 + kk) * T + t_out] = r;
                }
            }
        }
    }
}

// option "plan_merge": 1 / 0 force a merged / per-block plan; -1 (default): merged when the blocks use less than PLAN_MERGE_UTIL of the 16
// values of the source lines they touch (measured by the per-block builder: ~4 on a qhull-numbered mesh, ~12 on a
// lattice-numbered one -- there the lockstep of a group costs 2 % and saves nothing)
static constexpr double PLAN_MERGE_UTIL = 6.0;
static int plan_merge_mode() { // (read when a matrix' plan is built, once per matrix: a test can switch between matrices)
    const int64_t e = option(OPT_PLAN_MERGE);
    return e < 0 ? -1 : (e == 1 ? 1 : 0);
}

void ensure_plan(const xr_csr *ccsr) {
    xr_csr *csr = const_cast<xr_csr *>(ccsr); // the plan is a cache attached to the weights
    if (csr->plan.ready) return;
    XR_REQUIRE(exclusive_held(), XR_ERR_INVALID, "internal: apply plan requested outside the exclusive scope");
    const int64_t nb = (csr->n + AP_BLOCK - 1) / AP_BLOCK;
    bool merged = plan_merge_mode() == 1;
    int64_t n_lists = nb;
    csr->plan.loc.alloc((size_t)csr->nnz);
    csr->plan.lmax = 256;
    csr->plan.n_unplanned = 0;
    // The apply sizes its LDS stage for the LARGEST planned block, and that decides how many blocks a CU holds: one block
    // of 4096 entries among thousands of 1000 (a Delaunay hull) costs every block a third of the occupancy (K = 256 on
    // the benchmark matrix: 1.76 -> 1.2 ms).  Blocks beyond 2048 entries (twice the typical triangle-mesh block) go to
    // the direct kernel instead.
    constexpr int plan_cap = 2048;
    if (nb > 0) {
        DevBuf<int32_t> max_entries(4); // [0] largest planned block, [1] number of unplanned blocks, [2] distinct columns, [3] distinct lines (sums over the planned blocks)
        csr->plan.unplanned.alloc((size_t)nb);
        auto build = [&](bool group) {
            n_lists = group ? (nb + PLAN_GROUP - 1) / PLAN_GROUP : nb;
            csr->plan.ucol.alloc((size_t)n_lists * (group ? PLAN_GUMAX : PLAN_UMAX));
            csr->plan.nuniq.alloc((size_t)n_lists);
            fill_i32(max_entries.get(), 0, 4);
            auto builder = group ? k_plan_build<PLAN_GROUP> : k_plan_build<1>;
            XR_LAUNCH("plan_build", builder, dim3((unsigned)n_lists),
                      dim3(AP_BLOCK * (group ? PLAN_GROUP : 1)), 0, csr->indptr.get(), csr->indices.get(), csr->n,
                      csr->plan.ucol.get(), csr->plan.nuniq.get(), csr->plan.loc.get(), max_entries.get(),
                      csr->plan.unplanned.get(), max_entries.get() + 1, plan_cap);
        };
        build(merged);
        int32_t h[4];
        d2h(h, max_entries.get(), sizeof(h));
        if (!merged && plan_merge_mode() < 0 && h[3] > 0 && nb >= 4 * PLAN_GROUP && (double)h[2] / (double)h[3] < PLAN_MERGE_UTIL) {
            // (poor use of the source lines: the group plan gathers a line once for the group's row blocks)
            merged = true;
            build(true);
            d2h(h, max_entries.get(), sizeof(h));
        }
        const int m = h[0];
        csr->plan.n_unplanned = h[1];
        csr->plan.lmax = std::min(PLAN_LMAX, std::max(256, (m + 255) / 256 * 256));
        if (option(OPT_DEBUG) & 2) {
            std::vector<int32_t> nu((size_t)n_lists);
            d2h(nu.data(), csr->plan.nuniq.get(), sizeof(int32_t) * (size_t)n_lists);
            double sum = 0; int cnt = 0, mx = 0;
            for (auto v : nu) if (v >= 0) { sum += v; cnt++; mx = std::max(mx, (int)v); }
            fprintf(stderr, "[plan] %s blocks %lld planned %d unplanned %d lmax %d avg distinct columns %.1f max %d nnz/block %.1f\n", merged ? "merged (a list per group of row blocks)" : "per block", (long long)nb, cnt,
                    csr->plan.n_unplanned, csr->plan.lmax, cnt ? sum / cnt : 0.0, mx, (double)csr->nnz / nb);
        }
    }
    csr->plan.merged = merged;
    csr->plan.ready = true;
}

// k_apply_plan over the matrix's plan: KT variables per tile, SUBS row blocks per workgroup (MERGED: one value table for
// the workgroup's SUBS = PLAN_GROUP row blocks).  LDS is sized for the largest planned block, so typical matrices run
// three blocks per CU instead of two.
// (tuning hooks: row blocks per workgroup, variables per tile, the L2-blocked order of k_apply_plan: super tiles of
// `super_blocks` workgroups x items of `item_tiles` variable tiles)
template <int METHOD, typename SRC, int KT, int SUBS, bool MERGED, bool FAST>
static void launch_plan(const xr_csr *csr, const SRC *src, int64_t K, double *out) {
    // default: items of 64 variables, super tile = the XCD's whole range of row blocks -- every XCD sweeps its row blocks
    // once per 64 variables (the source planes in flight: 0.5 GB instead of all K of them; what the host-side split
    // into groups of 128 variables did until round 4, without its extra launches, forks and joins)
    const int plan_dbg = (int)option(OPT_PLAN_DBG); // measurement: 1 no gathers, 2 no stores, 4 plain instead of non-temporal stores
    // LDS per row block: a tile of distinct source values + the block's entries (weight + 16-bit local column), sized for
    // the largest planned block of the matrix.  4 row blocks per workgroup: tiles of 4 variables (4 x 34 KB)
    auto lds_bytes = [](size_t lmax) -> size_t {
        const size_t sub_bytes = ((sizeof(double) * ((size_t)KT * PLAN_UMAX + lmax) + sizeof(uint16_t) * lmax) + 15) / 16 * 16;
        const size_t stage_bytes = ((sizeof(double) * lmax + sizeof(uint16_t) * lmax) + 15) / 16 * 16;
        return MERGED ? sizeof(double) * (size_t)KT * PLAN_GUMAX + stage_bytes * PLAN_GROUP : sub_bytes * SUBS;
    };
    const size_t shmem = lds_bytes((size_t)csr->plan.lmax);
    XR_REQUIRE(shmem <= (size_t)160 * 1024, XR_ERR_LIMIT, "internal: apply plan needs %zu bytes of LDS", shmem);
    // (dynamic LDS beyond 64 KB has to be allowed per kernel: a permission, granted once for the most this instantiation can
    // ask for -- plan.lmax <= PLAN_LMAX, ensure_plan; the launch's own shmem decides how many workgroups a CU holds.  The whole
    // 160 KB cannot be granted: the kernel's static LDS counts against the same limit and the runtime refuses the attribute)
    allow_dynamic_lds<&k_apply_plan<METHOD, SRC, KT, SUBS, MERGED, FAST>>(lds_bytes(PLAN_LMAX));
    const int64_t n_groups = div_up(div_up(csr->n, AP_BLOCK), SUBS);
    const int item_tiles = 64 / KT;
    const int super_blocks = K > (int64_t)KT * item_tiles ? (int)std::min<int64_t>((n_groups + 7) / 8, 1 << 30) : 0;
    int64_t plan_grid = (n_groups + 7) / 8 * 8;
    if (super_blocks > 0) {
        const int64_t per_xcd = (n_groups + 7) / 8;
        const int64_t n_items = div_up(K, (int64_t)KT * item_tiles);
        plan_grid = 8 * div_up(per_xcd, super_blocks) * super_blocks * n_items;
    }
    XR_LAUNCH("apply_plan", (k_apply_plan<METHOD, SRC, KT, SUBS, MERGED, FAST>), dim3((unsigned)plan_grid), dim3(AP_BLOCK * SUBS),
              shmem, csr->indptr.get(), csr->indices.get(), csr->data.get(), csr->plan.ucol.get(), csr->plan.nuniq.get(),
              csr->plan.loc.get(), row_order_of(csr), csr->longs.any, csr->n, csr->m, src, K, out, csr->plan.lmax, super_blocks,
              item_tiles, plan_dbg);
}

void apply_planned(const xr_csr *csr, int method, const void *src, int dtype, int64_t K, double *out) {
    with_reducer(method, [&](auto m) {
        constexpr int METHOD = decltype(m)::value;
        XR_REQUIRE(streamed_reducer<METHOD>, XR_ERR_INVALID, "internal: reducer %d has no planned apply", METHOD);
        if constexpr (streamed_reducer<METHOD>)
            with_source_type(dtype, [&](auto tag) {
                using SRC = decltype(tag);
                const SRC *s = static_cast<const SRC *>(src);
                // contracted products + one reciprocal per row (k_apply_plan, FAST): opt-in
                constexpr bool FAST_OK = METHOD == XR_MEAN || METHOD == XR_FIRST_ORDER_CONSERVATIVE;
                const bool fast = FAST_OK && option(OPT_APPLY_CONTRACT) != 0;
                if (csr->plan.merged && fast) launch_plan<METHOD, SRC, 4, PLAN_GROUP, true, FAST_OK>(csr, s, K, out);
                else if (csr->plan.merged) launch_plan<METHOD, SRC, 4, PLAN_GROUP, true, false>(csr, s, K, out);
                else if (fast) launch_plan<METHOD, SRC, PLAN_KT, 1, false, FAST_OK>(csr, s, K, out);
                else launch_plan<METHOD, SRC, PLAN_KT, 1, false, false>(csr, s, K, out);
            });
    });
}

} // namespace xr
