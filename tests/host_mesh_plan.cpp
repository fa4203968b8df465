// CPU harness of xugrid_amd/csrc/xr_mesh_plan.h (test infrastructure).  Reads one case per line, the eight statistics as hex floats:
//   grid   s0..s7 n_face sampled              -> ok x0 y0 h0 inv_h0 n_levels n_cells {base nx ny} per level   | fail
//   morton s0..s7 n_face extents first max    -> x0 y0 inv_h n_side n_run
//   coherent s0..s7 n_face                    -> 0 | 1
// Integers in decimal, doubles with %a (compared bit for bit by tests/test_mesh_plan_host.py).
#include <cstdio>
#include <cstring>

#include "xr_mesh_plan.h"

int main() {
    char kind[16];
    while (scanf("%15s", kind) == 1) {
        double s[8];
        long long n_face;
        for (double &v : s)
            if (scanf("%la", &v) != 1) return 2;
        if (scanf("%lld", &n_face) != 1) return 2;
        if (!strcmp(kind, "grid")) {
            int sampled;
            if (scanf("%d", &sampled) != 1) return 2;
            xr::GridParams g{};
            if (!xr::index_grid(s, n_face, sampled != 0, g)) {
                puts("fail");
                continue;
            }
            printf("ok %a %a %a %a %d %d", g.x0, g.y0, g.h0, g.inv_h0, g.n_levels, g.n_cells);
            for (int l = 0; l < g.n_levels; l++) printf(" %d %d %d", g.base[l], g.nx[l], g.ny[l]);
            puts("");
        } else if (!strcmp(kind, "morton")) {
            double extents;
            int first, max;
            if (scanf("%la %d %d", &extents, &first, &max) != 3) return 2;
            const xr::MortonParams mp = xr::morton_cover(s, n_face, extents, first, max);
            printf("%a %a %a %d %d\n", mp.x0, mp.y0, mp.inv_h, mp.n_side, mp.n_run);
        } else if (!strcmp(kind, "coherent")) {
            printf("%d\n", xr::numbering_coherent(s, n_face) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
