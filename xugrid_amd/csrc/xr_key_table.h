// xr_key_table.h -- the key table of DESIGN section 15 and what turns its verdict into ids: shared by xr_merge.hip (joining
// meshes, matching point sets) and xr_periodic.hip (the seam of a periodic mesh).  Kernels are `static`: every translation unit
// that includes this header gets its own copy (as in xr_prims.h).
//
// It asks one question of a set of rows: "which rows are equal, and which of them came first".  Slots are int32 ids of rows, -1
// when empty; the capacity is a power of two strictly greater than the number of rows (key_table_capacity, xr_merge_keys.h),
// probing is linear with wrap-around.  A row is compared by reading it through the id in the slot.
//
// Insert, one thread per row i, at each slot of its probe sequence:
//     old = atomicCAS(slot, -1, i)      empty: the slot is i's, done
//     row[old] == row[i]                the slot is the key's: atomicMin(slot, i), done
//     else                              the slot belongs to another key for good: next slot
// A slot never becomes empty again and never changes its key (atomicMin only ever swaps in an id of the same key), so all
// rows of one key stop at the same slot -- the first of their common probe sequence that was empty or theirs -- and after the
// kernel that slot holds the SMALLEST id of the key, whatever the order of arrival: the reference's "first occurrence",
// deterministic.  A thread makes at most `capacity` probes and capacity > n leaves an empty slot, so it ends; nothing spins
// and no thread waits for another.
//
// Coherence: the L2 caches of the eight XCDs are not coherent with each other, and a plain load may be served from a line the
// own XCD fetched before another XCD's atomic changed the slot.  Inside the insert kernel the content of a slot is therefore
// taken ONLY from the value an atomic returns (atomics are performed at device scope, past the L2 of the issuing XCD).  The rows
// themselves were written by an earlier kernel and are read plainly.  The look-up is a second launch: a kernel boundary
// writes back and invalidates the L2s, so there plain loads see the final table.
#pragma once
#include "xr_internal.h"
#include "xr_merge_keys.h"

namespace xr {

// ---- the two kinds of rows
struct XYRows {
    const double2 *xy;
    __device__ uint32_t hash(int64_t i) const {
        const double2 p = xy[i];
        return key_hash_xy(p.x, p.y);
    }
    __device__ bool equal(int64_t a, int64_t b) const {
        const double2 p = xy[a], q = xy[b];
        return p.x == q.x && p.y == q.y;
    }
};
struct IntRows {
    const int32_t *rows; // [n, m], each row ascending
    int m;
    __device__ uint32_t hash(int64_t i) const { return key_hash_row(rows + i * m, m); }
    __device__ bool equal(int64_t a, int64_t b) const {
        bool same = true;
        for (int k = 0; k < m; k++) same &= rows[a * m + k] == rows[b * m + k];
        return same;
    }
};

// one thread per row (see the head of the file).  `mask` = capacity - 1.
template <typename ROWS>
static __global__ void __launch_bounds__(256) k_table_insert(ROWS rows, int64_t n, int32_t *__restrict__ table, uint32_t mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t h = rows.hash(i) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        const int32_t old = atomicCAS(table + h, -1, (int32_t)i);
        if (old < 0) return;
        if (old == (int32_t)i) return; // (cannot happen: one thread per id)
        if ((int64_t)old < n && rows.equal(old, i)) {
            atomicMin(table + h, (int32_t)i);
            return;
        }
    }
}

// the second launch: rep[i] = the smallest id with i's key (i itself for a row that equals nothing), flag[i] = rep[i] == i
template <typename ROWS>
static __global__ void __launch_bounds__(256)
k_table_rep(ROWS rows, int64_t n, const int32_t *__restrict__ table, uint32_t mask, int32_t *__restrict__ rep, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t h = rows.hash(i) & mask;
    int32_t r = (int32_t)i; // (every row was inserted: the loop finds it)
    for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        const int32_t occ = table[h];
        if (occ < 0) break;
        if (occ == (int32_t)i || ((int64_t)occ < n && rows.equal(occ, i))) {
            r = occ;
            break;
        }
    }
    rep[i] = r;
    flag[i] = r == (int32_t)i;
}

static __global__ void __launch_bounds__(256)
k_merge_inverse(const int32_t *__restrict__ rep, const int32_t *__restrict__ rank, int64_t n, int32_t *__restrict__ inverse) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) inverse[i] = rank[rep[i]];
}

static __global__ void __launch_bounds__(256)
k_merge_compact_xy(const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, int64_t n, const double2 *__restrict__ xy,
                   int32_t *__restrict__ keep, double2 *__restrict__ out_xy) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int j = rank[i];
    keep[j] = (int32_t)i;
    out_xy[j] = xy[i]; // (16 bytes copied: bit for bit, a kept zero keeps its sign)
}

// out[k] = rank[at[k]]: the scan's values at the segment boundaries, gathered for one read-back
static __global__ void k_merge_bounds(const int32_t *__restrict__ rank_a, const int32_t *__restrict__ rank_b, const int32_t *__restrict__ at,
                                      int n_a, int n_b, int32_t *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_a) out[k] = rank_a[at[k]];
    else if (k < n_a + n_b) out[k] = rank_b[at[k]];
}

struct KeyTable {
    DevBuf<int32_t> slots;
    uint32_t mask = 0;
    explicit KeyTable(int64_t n) {
        const int64_t cap = key_table_capacity(n, option(OPT_MERGE_TABLE_SLACK) == 1);
        slots.alloc((size_t)cap);
        mask = (uint32_t)(cap - 1);
        fill_i32(slots.get(), -1, cap);
    }
};

// rep / flag of n rows (n > 0): fill, insert, look up
template <typename ROWS> static void table_first_occurrence(const ROWS &rows, int64_t n, int32_t *rep, int32_t *flag) {
    KeyTable table(n);
    XR_LAUNCH("merge_insert", k_table_insert<ROWS>, dim3(div_up(n, 256)), dim3(256), 0, rows, n, table.slots.get(), table.mask);
    XR_LAUNCH("merge_rep", k_table_rep<ROWS>, dim3(div_up(n, 256)), dim3(256), 0, rows, n, table.slots.get(), table.mask, rep, flag);
    // (the table goes back to the pool here; the pool reuses blocks in stream order)
}

// flag -> rank [n + 1]; n == 0: rank[0] = 0
static void rank_of_flags(const int32_t *flag, int32_t *rank, int64_t n) {
    if (n > 0) exclusive_scan_i32(flag, rank, n);
    else fill_i32(rank, 0, 1);
}

} // namespace xr
