// xr_index.h -- the ascending index the mesh-operation units hand out (xr_index of include/xugrid_amd.h; its entry points are
// in xr_subset.hip) and the one pattern that makes it: flags -> exclusive scan -> compaction.  Shared by xr_subset.hip and
// xr_netedit.hip.
#pragma once
#include "xr_prims.h"

// ascending int32 ids in HBM; what xr_index_from_mask_dev and its relatives return
struct xr_index {
    int64_t n = 0;
    xr::DevBuf<int32_t> ids; // [n]
};

namespace xr {

// flags[index[i]] = 1 for the ids in range (flags zero at the start)
static __global__ void __launch_bounds__(256)
k_flag_ids(const int64_t *__restrict__ index, int64_t n, int64_t size, int32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t v = index[i];
    if (v >= 0 && v < size) flags[v] = 1;
}

// flags int32[n] of 0 / 1 (the base of a pool block) -> the ascending ids of the ones: scan, one read-back (their number),
// compaction
static xr_index *index_from_flags(const int32_t *flags, int64_t n) {
    Building<xr_index> out(OnFailure::WaitFirst);
    if (n > 0) {
        DevBuf<int32_t> off((size_t)n + 1);
        exclusive_scan_i32(flags, off.get(), n);
        out->n = read_scalar(off.get() + n);
        out->ids.alloc((size_t)out->n);
        if (out->n > 0) XR_LAUNCH("subset_compact", k_compact_ids<int32_t>, dim3(div_up(n, 256)), dim3(256), 0, flags, off.get(), n, out->ids.get());
        stream_sync(); // (the scan's scratch goes back to the pool behind its readers)
    }
    return out.release();
}

} // namespace xr
