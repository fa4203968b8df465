"""
ctypes binding of ``libxugrid_amd.so`` (the C ABI declared in ``include/xugrid_amd.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C xugrid_amd/csrc``.  There
is no CPU fallback: if the shared object is missing, or no HIP device is present, every compute
entry point raises -- loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# XUGRID_AMD_LIB: measurement hook only -- an A/B build of the same sources with other compiler flags (profiles/fma_ab.sh)
LIB_PATH = os.environ.get("XUGRID_AMD_LIB") or os.path.join(_HERE, "libxugrid_amd.so")

XR_OK = 0
XR_ERR_INVALID = -1
XR_ERR_NO_DEVICE = -2
XR_ERR_HIP = -3
XR_ERR_LIMIT = -4

XR_F64 = 0
XR_F32 = 1
XR_I32 = 2


class XugridAmdError(RuntimeError):
    """HIP runtime failure, missing device or missing shared library."""


c_i64 = ctypes.c_int64
c_f64 = ctypes.c_double
c_int = ctypes.c_int
vp = ctypes.c_void_p
p_i64 = ctypes.POINTER(ctypes.c_int64)
p_f64 = ctypes.POINTER(ctypes.c_double)
p_int = ctypes.POINTER(ctypes.c_int)
p_vp = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes).  Kept in one table so tests can check that every symbol declared
# in include/xugrid_amd.h is exported and bound.
SIGNATURES = {
    "xr_last_error": (ctypes.c_char_p, []),
    "xr_device_count": (c_int, [p_int]),
    "xr_init": (c_int, [c_int]),
    "xr_current_device": (c_int, [p_int]),
    "xr_trim_pool": (c_int, []),
    "xr_version": (c_int, []),
    "xr_set_stream": (c_int, [vp, c_int, c_int]),
    "xr_set_async": (c_int, [c_int]),
    "xr_set_option": (c_int, [ctypes.c_char_p, ctypes.c_int64]),
    "xr_get_option": (c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "xr_host_copy": (c_int, [vp, vp, c_i64]),
    "xr_host_interleave2": (c_int, [vp, c_i64, vp, c_i64, c_i64, vp]),
    "xr_mesh_create": (c_int, [vp, c_i64, vp, c_int, c_i64, c_i64, c_i64, p_vp]),
    "xr_mesh_create_dev": (c_int, [vp, c_i64, vp, c_int, c_i64, c_i64, c_i64, p_vp]),
    "xr_mesh_create_rectilinear": (c_int, [vp, c_i64, vp, c_i64, p_vp]),
    "xr_mesh_destroy": (c_int, [vp]),
    "xr_mesh_info": (c_int, [vp, p_i64, p_i64, p_i64]),
    "xr_mesh_device_bytes": (c_int, [vp, p_i64]),
    "xr_mesh_prepare": (c_int, [vp]),
    "xr_mesh_build_index": (c_int, [vp]),
    "xr_mesh_invalidate": (c_int, [vp]),
    "xr_mesh_area": (c_int, [vp, vp]),
    "xr_mesh_centroids": (c_int, [vp, vp]),
    "xr_mesh_centroids_dev": (c_int, [vp, vp]),
    "xr_mesh_faces": (c_int, [vp, vp]),
    "xr_mesh_download": (c_int, [vp, vp, vp]),
    "xr_mesh_triangulate": (c_int, [vp, p_vp]),
    "xr_mesh_triangle_face_dev": (c_int, [vp, vp]),
    "xr_mesh_circumcenters_dev": (c_int, [vp, vp]),
    "xr_mesh_perimeter_dev": (c_int, [vp, vp]),
    "xr_mesh_face_bounds_dev": (c_int, [vp, vp]),
    "xr_voronoi_create": (c_int, [vp, p_vp]),
    "xr_voronoi_create_flags": (c_int, [vp, c_int, c_int, c_int, vp, p_vp]),
    "xr_voronoi_vertex_info": (c_int, [vp, p_i64, p_i64]),
    "xr_voronoi_info": (c_int, [vp, p_i64, p_i64, p_i64, p_i64, p_i64]),
    "xr_voronoi_download": (c_int, [vp, vp, vp, vp, vp, vp]),
    "xr_voronoi_boundary_info": (c_int, [vp, vp, vp]),
    "xr_voronoi_boundary": (c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "xr_voronoi_mesh": (c_int, [vp, vp, c_i64, vp, c_i64, c_i64, p_vp]),
    "xr_voronoi_mesh_auto": (c_int, [vp, p_vp, p_i64, p_i64]),
    "xr_voronoi_tail": (c_int, [vp, vp, vp]),
    "xr_voronoi_boundary_cells_info": (c_int, [vp, p_i64, p_i64, p_i64]),
    "xr_voronoi_boundary_cells": (c_int, [vp, vp, vp]),
    "xr_voronoi_destroy": (c_int, [vp]),
    "xr_overlap": (c_int, [vp, vp, c_int, p_vp]),
    "xr_overlap_stats": (c_int, [vp, p_i64]),
    "xr_overlap_apply_dev": (c_int, [vp, vp, c_int, c_int, c_f64, vp, c_int, c_i64, vp, p_vp]),
    "xr_overlap_partial_dev": (c_int, [vp, vp, c_int, c_int, vp, c_int, c_i64, vp, c_int, p_vp]),
    "xr_shard_plan_dev": (c_int, [vp, vp, c_i64, c_int, vp, vp, c_i64, c_int, c_int, c_int, c_int, vp, p_i64, vp, p_i64, vp]),
    "xr_locate_points": (c_int, [vp, vp, c_i64, c_f64, vp]),
    "xr_locate_raster": (c_int, [vp, vp, c_i64, vp, c_i64, c_f64, vp]),
    "xr_barycentric": (c_int, [vp, vp, c_i64, c_f64, vp, vp]),
    "xr_locate_csr": (c_int, [vp, vp, vp, c_i64, c_f64, p_vp]),
    "xr_replace_interpolated_weights": (c_int, [vp, c_i64, vp, c_i64, c_i64, vp, vp, c_i64, vp, c_i64]),
    "xr_barycentric_csr": (c_int, [vp, vp, vp, vp, c_i64, c_f64, vp, vp, c_i64, p_vp]),
    "xr_barycentric_csr_tail": (c_int, [vp, vp, vp, vp, c_i64, c_f64, c_i64, vp, vp, c_i64, c_int, p_vp]),
    "xr_locate_flags_begin": (c_int, [vp, vp, vp, c_i64, p_vp]),
    "xr_points_destroy": (c_int, [vp]),
    "xr_barycentric_csr_points": (c_int, [vp, vp, vp, c_f64, c_i64, vp, vp, c_i64, c_int, p_vp]),
    "xr_csr_info": (c_int, [vp, p_i64, p_i64, p_i64]),
    "xr_csr_download": (c_int, [vp, vp, vp, vp]),
    "xr_csr_upload": (c_int, [vp, vp, vp, c_i64, c_i64, c_i64, p_vp]),
    "xr_csr_from_triplet": (c_int, [vp, vp, vp, c_i64, c_i64, c_i64, p_vp]),
    "xr_csr_from_outer": (c_int, [vp, vp, vp, c_i64, c_i64, vp, vp, vp, c_i64, c_i64, p_vp]),
    "xr_outer_create": (c_int, [vp, vp, vp, c_i64, c_i64, vp, vp, vp, c_i64, c_i64, p_vp]),
    "xr_outer_info": (c_int, [vp, vp, vp, vp]),
    "xr_outer_csr": (c_int, [vp, p_vp]),
    "xr_outer_destroy": (c_int, [vp]),
    "xr_csr_layered": (c_int, [vp, vp, vp, c_i64, c_i64, vp, vp, c_i64, c_i64, c_int, p_vp]),
    "xr_csr_layered_dev": (c_int, [vp, vp, vp, c_i64, c_i64, vp, vp, c_i64, c_i64, c_int, p_vp]),
    "xr_overlap_1d_nd_dev": (c_int, [vp, c_i64, c_i64, vp, c_i64, c_i64, vp, vp, c_i64, c_i64, vp, vp, vp, p_i64]),
    "xr_apply_outer": (c_int, [vp, c_int, c_f64, vp, c_int, c_i64, vp]),
    "xr_apply_outer_dev": (c_int, [vp, c_int, c_f64, vp, c_int, c_i64, vp]),
    "xr_edge_length_csr": (c_int, [vp, vp, c_i64, p_vp]),
    "xr_edge_length_csr_dev": (c_int, [vp, vp, c_i64, p_vp]),
    "xr_edge_pieces": (c_int, [vp, vp, vp, c_i64, vp]),
    "xr_csr_set_row_keys": (c_int, [vp, vp, c_i64]),
    "xr_csr_set_col_keys": (c_int, [vp, vp, c_i64]),
    "xr_csr_col_order": (c_int, [vp, vp]),
    "xr_csr_expect_permuted": (c_int, [vp, c_int]),
    "xr_csr_output_stored_order": (c_int, [vp, c_int]),
    "xr_csr_row_order": (c_int, [vp, c_i64, vp]),
    "xr_csr_long_rows": (c_int, [vp, c_i64, vp, vp]),
    "xr_csr_destroy": (c_int, [vp]),
    "xr_apply_csr": (c_int, [vp, c_int, c_f64, vp, c_int, c_i64, vp]),
    "xr_apply_csr_dev": (c_int, [vp, c_int, c_f64, vp, c_int, c_i64, vp]),
    "xr_apply_coo": (c_int, [vp, vp, c_i64, c_i64, vp, c_int, c_i64, c_i64, vp]),
    "xr_csr_transpose": (c_int, [vp, p_vp]),
    "xr_csr_drop_transpose": (c_int, [vp]),
    "xr_apply_csr_adjoint": (c_int, [vp, c_int, vp, c_int, vp, c_i64, vp]),
    "xr_apply_csr_adjoint_dev": (c_int, [vp, c_int, vp, c_int, vp, c_i64, vp]),
    "xr_apply_outer_adjoint_dev": (c_int, [vp, c_int, vp, c_int, vp, c_i64, vp]),
    "xr_partial_components": (c_int, [c_int]),
    "xr_partial_combine_is_max": (c_int, [c_int]),
    "xr_apply_partial_dev": (c_int, [vp, c_int, vp, c_int, c_i64, vp, c_int]),
    "xr_partial_fill_identity_dev": (c_int, [c_int, vp, c_i64, c_i64]),
    "xr_finalize_partial_dev": (c_int, [c_int, vp, c_i64, c_i64, vp]),
    "xr_reduce_partial_rows_dev": (c_int, [c_int, vp, vp, vp, c_i64, c_i64, vp]),
    "xr_graph_from_csr": (c_int, [vp, vp, vp, c_i64, c_i64, vp, p_vp]),
    "xr_graph_info": (c_int, [vp, p_i64, p_i64]),
    "xr_graph_download": (c_int, [vp, vp, vp, vp, vp]),
    "xr_graph_destroy": (c_int, [vp]),
    "xr_graph_laplace_fill_dev": (c_int, [vp, vp, vp, c_i64, c_int, c_f64, c_f64, c_i64, c_i64, vp, vp]),
    "xr_nearest_fill_dev": (c_int, [vp, c_i64, vp, vp, c_i64, c_f64]),
    "xr_network_graph_dev": (c_int, [vp, c_i64, vp, c_i64, c_int, p_vp, p_i64]),
    "xr_graph_nearest_dev": (c_int, [vp, vp, c_i64, c_f64, c_i64, vp, vp, p_i64]),
    "xr_graph_nearest_fill_dev": (c_int, [vp, vp, vp, c_i64, c_f64, c_i64, p_i64]),
    "xr_topology_create": (c_int, [vp, p_vp]),
    "xr_topology_info": (c_int, [vp, p_i64, p_i64, p_i64, p_i64, p_i64]),
    "xr_topology_long_nodes": (c_int, [vp, p_i64]),
    "xr_topology_download": (c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "xr_topology_download_node_tables": (c_int, [vp, vp, vp, vp, vp]),
    "xr_topology_edge_xy_dev": (c_int, [vp, vp]),
    "xr_topology_exterior_face_dev": (c_int, [vp, vp]),
    "xr_topology_destroy": (c_int, [vp]),
    "xr_graph_from_topology": (c_int, [vp, c_int, p_vp]),
    "xr_graph_label_rounds": (c_int, [vp, p_i64]),
    "xr_graph_components_dev": (c_int, [vp, vp, p_i64]),
    "xr_graph_binary_iterate_dev": (c_int, [vp, vp, vp, c_i64, c_int, c_i64, vp, vp]),
    "xr_graph_rcm_dev": (c_int, [vp, vp, p_i64]),
    "xr_mesh_reorder_faces_dev": (c_int, [vp, vp, p_vp]),
    "xr_graph_partition_dev": (c_int, [vp, vp, vp, c_i64, vp, p_i64]),
    "xr_topology_facet_map_dev": (c_int, [vp, c_int, c_int, c_int, vp, c_int, c_i64, vp]),
    "xr_topology_facet_width": (c_int, [vp, c_int, c_int, p_i64]),
    "xr_facet_map_dev": (c_int, [vp, vp, c_i64, c_i64, c_i64, c_int, vp, c_int, c_i64, vp]),
    "xr_nn_create_dev": (c_int, [vp, c_i64, p_vp]),
    "xr_nn_create_mesh": (c_int, [vp, c_int, p_vp]),
    "xr_nn_info": (c_int, [vp, p_i64, p_i64]),
    "xr_nn_destroy": (c_int, [vp]),
    "xr_nn_query_dev": (c_int, [vp, vp, c_i64, c_f64, vp]),
    "xr_gather_points_dev": (c_int, [vp, c_int, c_i64, c_i64, vp, c_i64, c_f64, vp]),
    "xr_section_coords_dev": (c_int, [vp, vp, c_i64, vp, c_i64, vp, vp]),
    "xr_burn_polygons_dev": (c_int, [vp, vp, c_i64, vp, c_i64, vp, c_i64, c_int, vp]),
    "xr_burn_lines_dev": (c_int, [vp, vp, c_i64, vp, c_i64, vp]),
    "xr_burn_points_dev": (c_int, [vp, vp, c_i64, vp]),
    "xr_burn_combine_dev": (c_int, [c_i64, vp, vp, vp, vp, vp, vp, c_f64, vp]),
    "xr_polygonize_dev": (c_int, [vp, vp, c_int, p_vp]),
    "xr_polygons_info": (c_int, [vp, p_i64, p_i64, p_i64, p_i64, p_i64]),
    "xr_polygons_readbacks": (c_int, [vp, p_i64]),
    "xr_polygons_copy_dev": (c_int, [vp, vp, vp, vp, vp, vp]),
    "xr_polygons_destroy": (c_int, [vp]),
    "xr_mesh_subset_dev": (c_int, [vp, vp, c_i64, p_vp, p_int, p_i64]),
    "xr_mesh_subset_node_index_dev": (c_int, [vp, vp]),
    "xr_index_check_dev": (c_int, [vp, c_i64, c_i64, p_i64]),
    "xr_index_mismatch_dev": (c_int, [vp, vp, c_i64, p_i64]),
    "xr_index_from_mask_dev": (c_int, [vp, c_i64, p_vp]),
    "xr_mesh_box_faces_dev": (c_int, [vp, c_f64, c_f64, c_f64, c_f64, p_vp]),
    "xr_mesh_faces_of_nodes_dev": (c_int, [vp, vp, c_i64, p_vp]),
    "xr_topology_faces_of_edges_dev": (c_int, [vp, vp, c_i64, p_vp]),
    "xr_topology_subset_edges_dev": (c_int, [vp, vp, c_i64, p_vp]),
    "xr_index_info": (c_int, [vp, p_i64]),
    "xr_index_copy_dev": (c_int, [vp, vp]),
    "xr_index_destroy": (c_int, [vp]),
    "xr_merge_meshes_dev": (c_int, [vp, c_i64, p_vp]),
    "xr_merge_edges_dev": (c_int, [vp, vp, c_i64, vp]),
    "xr_merge_info": (c_int, [vp, p_i64, p_i64, p_i64]),
    "xr_merge_take_mesh": (c_int, [vp, p_vp]),
    "xr_merge_index_info": (c_int, [vp, c_int, c_i64, p_i64]),
    "xr_merge_index_copy_dev": (c_int, [vp, c_int, c_i64, c_int, vp]),
    "xr_merge_node_inverse_copy_dev": (c_int, [vp, vp]),
    "xr_merge_destroy": (c_int, [vp]),
    "xr_index_like_dev": (c_int, [vp, vp, c_i64, c_f64, vp, p_i64]),
    "xr_labels_range_dev": (c_int, [vp, c_i64, p_i64, p_i64]),
    "xr_labels_order_dev": (c_int, [vp, c_i64, c_i64, p_vp, p_i64]),
    "xr_label_order_copy_dev": (c_int, [vp, c_i64, c_i64, vp]),
    "xr_label_order_destroy": (c_int, [vp]),
    "xr_dev_copy_columns": (c_int, [vp, c_i64, vp, c_i64, c_i64]),
    "xr_periodic_wrap_dev": (c_int, [vp, p_vp, p_i64]),
    "xr_periodic_unwrap_dev": (c_int, [vp, c_f64, p_vp]),
    "xr_periodic_edges_dev": (c_int, [vp, vp, vp, p_i64]),
    "xr_periodic_info": (c_int, [vp, p_i64]),
    "xr_periodic_take_mesh": (c_int, [vp, p_vp]),
    "xr_periodic_index_copy_dev": (c_int, [vp, c_int, vp]),
    "xr_periodic_node_inverse_copy_dev": (c_int, [vp, vp]),
    "xr_periodic_destroy": (c_int, [vp]),
    "xr_network_subset_dev": (c_int, [vp, c_i64, vp, c_i64, vp, c_i64, p_vp, p_int, p_i64]),
    "xr_network_edges_of_nodes_dev": (c_int, [vp, c_i64, c_i64, vp, c_i64, p_vp]),
    "xr_network_box_edges_dev": (c_int, [vp, c_i64, vp, c_i64, c_f64, c_f64, c_f64, c_f64, p_vp]),
    "xr_network_nonloop_edges_dev": (c_int, [vp, c_i64, p_vp]),
    "xr_network_merge_dev": (c_int, [p_vp, p_i64, p_vp, p_i64, c_i64, p_vp]),
    "xr_network_refine_dev": (c_int, [vp, c_i64, vp, c_i64, vp, c_i64, c_f64, p_vp, p_i64]),
    "xr_netedit_info": (c_int, [vp, p_i64]),
    "xr_netedit_copy_dev": (c_int, [vp, c_int, vp]),
    "xr_netedit_part_info": (c_int, [vp, c_int, c_i64, p_i64]),
    "xr_netedit_part_copy_dev": (c_int, [vp, c_int, c_i64, vp]),
    "xr_netedit_destroy": (c_int, [vp]),
    "xr_snap_nodes_dev": (c_int, [vp, vp, c_i64, c_i64, c_f64, p_vp]),
    "xr_snap_info": (c_int, [vp, p_i64, p_i64, p_i64]),
    "xr_snap_copy_dev": (c_int, [vp, c_int, vp]),
    "xr_snap_relabel_dev": (c_int, [vp, vp, c_i64, vp]),
    "xr_snap_destroy": (c_int, [vp]),
    "xr_nn_snap_dev": (c_int, [vp, vp, vp, c_i64, c_i64, c_f64, vp, vp, c_i64, vp, p_i64]),
    "xr_snapgrid_create_dev": (c_int, [vp, vp, vp, vp, c_i64, vp, c_i64, c_f64, c_f64, c_int, p_vp]),
    "xr_snapgrid_info": (c_int, [vp, p_i64, p_i64, p_i64]),
    "xr_snapgrid_copy_dev": (c_int, [vp, c_int, vp]),
    "xr_snapgrid_values_dev": (c_int, [vp, vp, c_i64, vp]),
    "xr_snapgrid_destroy": (c_int, [vp]),
    "xr_unique_xy_dev": (c_int, [vp, c_i64, p_vp]),
    "xr_unique_xy_info": (c_int, [vp, p_i64]),
    "xr_unique_xy_copy_dev": (c_int, [vp, c_int, vp]),
    "xr_unique_xy_destroy": (c_int, [vp]),
    "xr_mesh_from_bounds_dev": (c_int, [vp, vp, c_i64, p_vp, vp, p_i64]),
    "xr_interval_breaks_dev": (c_int, [vp, c_i64, c_i64, c_int, vp, p_i64]),
    "xr_mesh_from_intervals_dev": (c_int, [vp, vp, c_i64, c_i64, p_vp]),
    "xr_mesh_from_rings_dev": (c_int, [vp, c_i64, vp, c_i64, vp, c_i64, p_vp, p_i64]),
    "xr_mesh_ring_offsets_dev": (c_int, [vp, vp, vp, p_i64]),
    "xr_mesh_ring_coords_dev": (c_int, [vp, vp, c_i64, vp]),
    "xr_lines_to_network_dev": (c_int, [vp, c_i64, vp, c_i64, p_vp, vp, p_i64]),
    "xr_dev_alloc": (c_int, [c_i64, p_vp]),
    "xr_dev_free": (c_int, [vp]),
    "xr_dev_upload": (c_int, [vp, vp, c_i64]),
    "xr_dev_download": (c_int, [vp, vp, c_i64]),
    "xr_dev_sync": (c_int, []),
    "xr_prof_enable": (c_int, [c_int]),
    "xr_prof_reset": (c_int, []),
    "xr_prof_count": (c_int, [p_int]),
    "xr_prof_get": (c_int, [c_int, ctypes.c_char_p, c_int, p_i64, p_f64]),
}

_lib = None


def load():
    """Load the shared library (no device needed for this step) and bind every symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XugridAmdError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C xugrid_amd/csrc). "
            "xugrid_amd has no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error():
    msg = load().xr_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc):
    """Map a C status to the exception type the reference would raise for the same mistake."""
    if rc == XR_OK:
        return
    msg = last_error()
    if rc == XR_ERR_INVALID:
        raise ValueError(msg)
    if rc == XR_ERR_LIMIT:
        raise OverflowError(msg)
    raise XugridAmdError(msg or f"libxugrid_amd error {rc}")


def device_count():
    n = c_int(0)
    load().xr_device_count(ctypes.byref(n))
    return n.value
