// xr_topology.h -- the edge topology of a device mesh (built in xr_topology.hip, read by the graph construction in xr_fill.hip
// and by the facet mapping in xr_facet.hip)
#pragma once
#include "xr_objects.h"

struct xr_topology {
    xr_mesh *mesh = nullptr; // borrowed: the caller keeps the mesh alive
    int64_t n_node = 0, n_face = 0, n_edge = 0, n_exterior = 0, n_nonmanifold = 0, ff_nnz = 0, nn_nnz = 0;
    int m = 0;
    int64_t n_long_nodes = 0;         // nodes whose neighbour list went through the wave-per-node kernel
    xr::DevBuf<int32_t> edge_node;    // [n_edge*2] (lower, higher), lexicographic
    xr::DevBuf<int32_t> face_edge;    // [n_face*m] compacted to the left, -1 trailing
    xr::DevBuf<int32_t> edge_face;    // [n_edge*2] ascending, -1 in column 1 for an exterior edge
    xr::DevBuf<int32_t> ff_ptr, ff_idx, ff_dat; // face -> face CSR, data = (sum of) shared edge id(s)
    xr::DevBuf<int32_t> nn_ptr, nn_idx, nn_dat; // node -> node CSR, data = edge id; (nn_ptr, nn_dat) IS node -> edge, edges ascending
    xr::DevBuf<int32_t> nf_ptr, nf_idx;         // node -> face CSR, faces ascending (one entry per slot of a face that names the node)
    int nf_width = -1, nn_width = -1;           // widest row of node -> face / node -> edge; -1: not asked for yet (xr_facet.hip)
    xr::DevBuf<uint8_t> exterior_edge; // [n_edge]
    xr::DevBuf<uint8_t> exterior_face; // [n_face]
};
