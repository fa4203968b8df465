// CPU harness of xugrid_amd/csrc/xr_overlap_tail.h: fused_outcome (test infrastructure).  Reads lines of
// "c_reg c_big n_pending err p_regular p_big cap big_capacity" and prints the verdict's name for each.
#include <cstdio>

#include "xr_overlap_tail.h"

static const char *name_of(xr::FusedOutcome o) {
    switch (o) {
    case xr::FUSED_FINAL: return "final";
    case xr::FUSED_LIMIT: return "limit";
    case xr::FUSED_GENERAL: return "general";
    case xr::FUSED_GROW_BIG: return "grow_big";
    case xr::FUSED_GROW_CSR: return "grow_csr";
    }
    return "?";
}

int main() {
    long long v[8];
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]) == 8)
        puts(name_of(xr::fused_outcome((int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)v[5],
                                       (int64_t)v[6], (int64_t)v[7])));
    return 0;
}
