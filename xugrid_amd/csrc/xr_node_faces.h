// xr_node_faces.h -- node -> face inversion of a face table on the device (connectivity.invert_dense_to_sparse,
// ugrid/connectivity.py:247-259): the counting sort shared by the Voronoi pre-step (xr_voronoi.hip) and the edge topology
// (xr_topology.hip).  Kernels are `static`: every translation unit that includes this header gets its own copy.
#pragma once
#include "xr_internal.h"

namespace xr {

// Node -> face inversion = a counting sort of the (node, face) slots by node.  Device-scope atomics are executed at the memory
// side of the fabric on this part (every one of them leaves the XCD's L2: PMC TCC_EA0_ATOMIC = TCC_ATOMIC), ~40 G/s in total:
// one atomic per SLOT made both passes atomic-bound (3M slots of a 1M-triangle mesh: 75 + 82 us).  A block therefore counts
// its 1024 slots per DISTINCT node in an LDS table first (faces arrive spatially coherent: a node's ~6 faces mostly sit in
// the same block) and issues one global atomic per distinct node -- the count pass a plain add, the scatter pass one
// returning add that reserves the block's stretch of the node's row; a slot's place in it is its rank in the table.
static constexpr int VOR_SLOTS = 1024, VOR_TABLE = 2048; // slots per block (4 per thread); open-addressing table, load <= 1/2
struct VorTable {
    int32_t key[VOR_TABLE];
    int32_t cnt[VOR_TABLE];
    int32_t base[VOR_TABLE];
};
__device__ __forceinline__ void vor_table_clear(VorTable &t) {
    for (int s = threadIdx.x; s < VOR_TABLE; s += 256) {
        t.key[s] = -1;
        t.cnt[s] = 0;
    }
}
// -> slot of node v in the table; rank = position of this (node, face) slot among the block's slots of the same node
__device__ __forceinline__ int vor_table_insert(VorTable &t, int v, int &rank) {
    int s = (int)(((unsigned)v * 2654435761u) >> 21) & (VOR_TABLE - 1);
    while (true) {
        const int prev = atomicCAS(&t.key[s], -1, v);
        if (prev == -1 || prev == v) break;
        s = (s + 1) & (VOR_TABLE - 1);
    }
    rank = atomicAdd(&t.cnt[s], 1);
    return s;
}

static __global__ void __launch_bounds__(256)
k_vor_count(const int32_t *__restrict__ faces, int64_t total, int32_t *__restrict__ count) {
    __shared__ VorTable sh;
    vor_table_clear(sh);
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * VOR_SLOTS + threadIdx.x;
    int v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = i0 + u * 256 < total ? faces[i0 + u * 256] : -1;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        int rank;
        if (v[u] >= 0) vor_table_insert(sh, v[u], rank);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < VOR_TABLE; s += 256)
        if (sh.key[s] >= 0) atomicAdd(&count[sh.key[s]], sh.cnt[s]);
}

static __global__ void __launch_bounds__(256)
k_vor_scatter(const int32_t *__restrict__ faces, int64_t total, int m, const int32_t *__restrict__ indptr,
              int32_t *__restrict__ cursor, int32_t *__restrict__ out) {
    __shared__ VorTable sh;
    vor_table_clear(sh);
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * VOR_SLOTS + threadIdx.x;
    int v[4], slot[4], rank[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = i0 + u * 256 < total ? faces[i0 + u * 256] : -1;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        slot[u] = 0, rank[u] = 0;
        if (v[u] >= 0) slot[u] = vor_table_insert(sh, v[u], rank[u]);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < VOR_TABLE; s += 256) {
        const int key = sh.key[s];
        if (key >= 0) sh.base[s] = indptr[key] + atomicAdd(&cursor[key], sh.cnt[s]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (v[u] >= 0) out[sh.base[slot[u]] + rank[u]] = (int32_t)((i0 + u * 256) / m);
}

// ascending face ids per node (the scatter order is arbitrary); rows are short
static __global__ void __launch_bounds__(256)
k_vor_sort_rows(const int32_t *__restrict__ indptr, int64_t n_node, int32_t *__restrict__ rows) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_node) return;
    const int s = indptr[v], e = indptr[v + 1];
    for (int i = s + 1; i < e; i++) {
        const int key = rows[i];
        int j = i - 1;
        while (j >= s && rows[j] > key) {
            rows[j + 1] = rows[j];
            j--;
        }
        rows[j + 1] = key;
    }
}

} // namespace xr
