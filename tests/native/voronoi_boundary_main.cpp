// Stand-alone driver of xugrid_amd/csrc/xr_voronoi_boundary.h for the host sanitizers (tests/test_derive_cpu.py compiles it
// with -fsanitize=address,undefined and runs it on local problems built with numpy).
// stdin:  n_face nb ne n_entry add_vertices skip_concave, then one array per line: nodes [nb], row_ptr [nb + 1],
//         faces [n_entry], face_xy [2 n_entry], node_xy [2 nb], edge_lo [ne], edge_hi [ne], edge_face [ne], edge_face_xy [2 ne]
//         (floats as C hexadecimal literals: exact).
// stdout: the status; then "n_extra_vertex n_cell m n_tail n_map" and extra_xy, cells, tail, interpolation map, one per line.
#include <cstdio>
#include <vector>

#include "../../xugrid_amd/csrc/xr_voronoi_boundary.h"

static bool read_ints(std::vector<int64_t> &a, long long n) {
    a.resize((size_t)n);
    for (long long i = 0; i < n; i++) {
        long long v;
        if (std::scanf("%lld", &v) != 1) return false;
        a[(size_t)i] = v;
    }
    return true;
}

static bool read_floats(std::vector<double> &a, long long n) {
    a.resize((size_t)n);
    for (long long i = 0; i < n; i++)
        if (std::scanf("%la", &a[(size_t)i]) != 1) return false;
    return true;
}

int main() {
    long long n_face = 0, nb = 0, ne = 0, n_entry = 0;
    int add_vertices = 1, skip_concave = 1;
    if (std::scanf("%lld %lld %lld %lld %d %d", &n_face, &nb, &ne, &n_entry, &add_vertices, &skip_concave) != 6) return 2;
    if (n_face < 0 || nb < 0 || ne < 0 || n_entry < 0) return 2;
    std::vector<int64_t> nodes, row_ptr, faces, edge_lo, edge_hi, edge_face;
    std::vector<double> face_xy, node_xy, edge_face_xy;
    if (!read_ints(nodes, nb) || !read_ints(row_ptr, nb + 1) || !read_ints(faces, n_entry) || !read_floats(face_xy, 2 * n_entry) ||
        !read_floats(node_xy, 2 * nb) || !read_ints(edge_lo, ne) || !read_ints(edge_hi, ne) || !read_ints(edge_face, ne) ||
        !read_floats(edge_face_xy, 2 * ne))
        return 2;
    xr::VoronoiBoundaryIn in;
    in.n_face = n_face; in.nb = nb; in.ne = ne;
    in.nodes = nodes.data(); in.row_ptr = row_ptr.data(); in.faces = faces.data(); in.face_xy = face_xy.data();
    in.node_xy = node_xy.data(); in.edge_lo = edge_lo.data(); in.edge_hi = edge_hi.data(); in.edge_face = edge_face.data();
    in.edge_face_xy = edge_face_xy.data();
    in.add_vertices = add_vertices != 0;
    in.skip_concave = skip_concave != 0;
    xr::VoronoiBoundaryOut out;
    const int status = xr::voronoi_boundary_cells(in, out);
    std::printf("%d\n", status);
    if (status != 0) return 0;
    std::printf("%lld %lld %lld %lld %lld\n", (long long)(out.extra_xy.size() / 2), (long long)out.n_cell, (long long)out.m,
                (long long)out.tail.size(), (long long)(out.interp.size() / 2));
    for (double v : out.extra_xy) std::printf("%a ", v);
    std::printf("\n");
    for (int64_t v : out.cells) std::printf("%lld ", (long long)v);
    std::printf("\n");
    for (int64_t v : out.tail) std::printf("%lld ", (long long)v);
    std::printf("\n");
    for (int64_t v : out.interp) std::printf("%lld ", (long long)v);
    std::printf("\n");
    return 0;
}
