"""
Yardsticks of the derive tests (tests/test_derive_cpu.py, tests/test_gpu_derive.py): numpy restatements of the fan
triangulation, the circumcenters, the perimeter and the face bounds, written from their descriptions and
pinned to the known answers in tests/golden/derive_known.json; the meshes the tests run on; and the LOCAL problem of the
boundary cells -- the arrays the device gathers for the host step of csrc/xr_voronoi_boundary.h -- built with numpy.
"""
import json
import os

import numpy as np
import scipy.sparse

from xugrid_amd import connectivity, meshgen, voronoi

HERE = os.path.dirname(os.path.abspath(__file__))
FLAG_SETS = ((True, True, False), (True, True, True), (True, False, False), (False, False, False))


def known():
    with open(os.path.join(HERE, "golden", "derive_known.json")) as f:
        return json.load(f)


# ---- restatements ---------------------------------------------------------------------------------------------------------
def triangulate_dense(faces):
    """Triangle t of a face with k nodes is (n0, n[t + 1], n[t + 2]), t = 0 .. k - 3, faces in order; a table of three
    columns is copied.  -> (triangles (n_triangle, 3), triangle_face (n_triangle,))"""
    faces = np.asarray(faces)
    n_face, m = faces.shape
    if m == 3:
        return faces.copy(), np.arange(n_face)
    per_face = (faces != -1).sum(axis=1) - 2
    index = np.repeat(np.arange(n_face), per_face)
    t = np.arange(index.size) - np.repeat(np.cumsum(per_face) - per_face, per_face)
    return np.column_stack([faces[index, 0], faces[index, t + 1], faces[index, t + 2]]), index


def circumcenters(faces, x, y):
    """Circumcenter of every triangle, in the operation order the library evaluates (no fused multiply-add on either side)."""
    faces = np.asarray(faces)
    if faces.shape[1] != 3:
        raise NotImplementedError("Circumcenters are only supported for triangular grids")
    a_x, b_x, c_x = x[faces.T]
    a_y, b_y, c_y = y[faces.T]
    d_inv = 0.5 / (a_y * c_x + b_y * a_x - b_y * c_x - a_y * b_x - c_y * a_x + c_y * b_x)
    sq_a = (a_x - c_x) * (a_x + c_x) + (a_y - c_y) * (a_y + c_y)
    sq_b = (b_x - c_x) * (b_x + c_x) + (b_y - c_y) * (b_y + c_y)
    cx = sq_a * (b_y - c_y) - sq_b * (a_y - c_y)
    cy = sq_b * (a_x - c_x) - sq_a * (b_x - c_x)
    return np.column_stack([d_inv * cx, d_inv * cy])


def perimeter(faces, x, y):
    """Closed polygon relative to its first vertex (fill slots and the closing slot repeat vertex 0), differences of
    consecutive slots, sqrt(dx * dx + dy * dy), summed in slot order."""
    closed, _ = connectivity.close_polygons(np.asarray(faces))
    xy = np.stack([x[closed], y[closed]], axis=-1)
    xy = xy - xy[:, :1]
    d = np.diff(xy, axis=1)
    length = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    total = np.zeros(len(closed))
    for j in range(length.shape[1]):  # slot order
        total = total + length[:, j]
    return total


def face_bounds(faces, x, y):
    faces = np.asarray(faces)
    fill = faces == -1
    fx, fy = x[faces], y[faces]
    return np.column_stack([np.where(fill, np.inf, fx).min(axis=1), np.where(fill, np.inf, fy).min(axis=1),
                            np.where(fill, -np.inf, fx).max(axis=1), np.where(fill, -np.inf, fy).max(axis=1)])


def polygon_area_signed(xy, cells):
    """Signed shoelace area of every -1 padded cell."""
    closed, _ = connectivity.close_polygons(cells)
    p = xy[closed]
    rel = p - p[:, :1]
    a, b = rel[:, :-1], rel[:, 1:]
    return 0.5 * (a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]).sum(axis=1)


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def four_square():
    k = known()["four_triangle_square"]
    return np.array(k["nodes"]), np.array(k["faces"], dtype=np.int64)


def exact_lattice(n=9):
    """Right triangles on an integer lattice: every circumcenter is a half-integer point, computed exactly."""
    xy, faces = meshgen.quad_mesh(np.arange(n + 1.0), np.arange(n + 1.0))
    tri = np.concatenate([faces[:, [0, 1, 2]], faces[:, [0, 2, 3]]])
    return xy, np.ascontiguousarray(tri, dtype=np.int64)


def triangles_in_four_columns():
    xy, faces = meshgen.triangle_mesh(60, 4)
    return xy, np.column_stack([faces, np.full(len(faces), -1, dtype=faces.dtype)])


def clockwise_mesh():
    xy, faces = meshgen.mixed_mesh(49, 5)
    out = faces.copy()
    for f in range(len(faces)):
        k = int((faces[f] != -1).sum())
        out[f, :k] = faces[f, :k][::-1]
    return xy, out


def gon32_mesh():
    """One 32-gon (the most nodes a face may have) fanned about by nothing, beside two triangles."""
    ang = 2.0 * np.pi * np.arange(32) / 32
    xy = np.concatenate([np.column_stack([np.cos(ang), np.sin(ang)]), [[2.0, 0.0], [2.0, 1.0], [3.0, 0.0]]])
    faces = np.full((3, 32), -1, dtype=np.int64)
    faces[0, :3] = [0, 32, 33]
    faces[1] = np.arange(32)
    faces[2, :3] = [32, 34, 33]
    return xy, faces


def mixed_with_faces(n_face):
    """A mixed mesh cut to exactly ``n_face`` faces (the int32 scan's tile holds 2048 items)."""
    xy, faces = meshgen.mixed_mesh(2500, 7)
    assert len(faces) >= n_face
    return xy, np.ascontiguousarray(faces[:n_face])


def strip_mesh(n=6):
    """One row of quads: no node has three faces."""
    return meshgen.quad_mesh(np.arange(n + 1.0), np.arange(2.0))


def compaction_mesh():
    """A 3 x 3 block of quads (its four inner nodes have four faces each) and, first in the face table and joined to the block
    by a single node, a triangle none of whose nodes has three faces: without exterior its centroid is not a vertex, so every
    vertex id is renumbered."""
    xy, faces = meshgen.quad_mesh(np.arange(4.0), np.arange(4.0))
    n = len(xy)
    xy = np.concatenate([xy, [[-1.0, -0.5], [-0.5, -1.0]]])
    tri = np.array([[0, n, n + 1, -1]], dtype=faces.dtype)
    return xy, np.concatenate([tri, faces])


# ---- the host yardstick of a tessellation ------------------------------------------------------------------------------------
def host_connectivity(faces, n_node):
    faces = np.asarray(faces, dtype=np.intp)
    edge_node, face_edge = connectivity.edge_connectivity(faces)
    edge_face = connectivity.invert_dense(face_edge)
    if edge_face.shape[1] < 2:
        edge_face = np.column_stack([edge_face, np.full(len(edge_face), -1, dtype=edge_face.dtype)])
    return connectivity.invert_dense_to_sparse(faces, n_rows=n_node), edge_node, edge_face


def host_tessellation(xy, faces, generators, flags):
    """``voronoi.voronoi_topology`` on the host connectivity -> (vertices, cells, face_index, interpolation_map)."""
    nfc, edge_node, edge_face = host_connectivity(faces, len(xy))
    return voronoi.voronoi_topology(nfc, xy, generators, edge_face, edge_node, *flags)


# ---- the local problem of the boundary cells ------------------------------------------------------------------------------
def local_problem(xy, faces, generators):
    """What the device gathers for the host step: boundary nodes, their rows of node -> face with the generator point of every
    listed face, the exterior edges (lexicographic) with the generator point of each edge's face."""
    nfc, edge_node, edge_face = host_connectivity(faces, len(xy))
    ext = edge_face[:, 1] == -1
    e_nodes, e_face = np.sort(edge_node[ext], axis=1), edge_face[ext, 0]
    order = np.lexsort((e_face, e_nodes[:, 1], e_nodes[:, 0]))
    e_nodes, e_face = e_nodes[order], e_face[order]
    nodes = np.unique(e_nodes)
    rows = nfc.tocsr()[nodes]
    rows.sort_indices()
    return {
        "n_face": len(faces), "nodes": nodes.astype(np.int64), "row_ptr": rows.indptr.astype(np.int64),
        "faces": rows.indices.astype(np.int64), "face_xy": generators[rows.indices], "node_xy": xy[nodes],
        "edge_nodes": e_nodes.astype(np.int64), "edge_face": e_face.astype(np.int64), "edge_face_xy": generators[e_face],
    }


def local_expected(p, add_vertices, skip_concave):
    """``voronoi._boundary_records`` on the local problem, in global vertex ids -> (extra_xy, cells, tail, interp or None)."""
    faces, edge_face = p["faces"], p["edge_face"]
    needed, inverse = np.unique(np.concatenate([faces, edge_face]), return_inverse=True)
    nl = needed.size
    cen = np.empty((nl, 2))
    cen[inverse[: faces.size]] = p["face_xy"]
    cen[inverse[faces.size:]] = p["edge_face_xy"]
    nfc = scipy.sparse.csr_matrix((np.ones(faces.size, dtype=np.int8), inverse[: faces.size], p["row_ptr"]),
                                  shape=(p["nodes"].size, nl))
    table, keys, ids, findex, interp = voronoi._boundary_records(
        nfc, p["node_xy"], cen, np.searchsorted(p["nodes"], p["edge_nodes"]), inverse[faces.size:], add_vertices, skip_concave)
    shift = p["n_face"] - nl
    ids = np.where(ids < nl, needed[np.minimum(ids, nl - 1)], ids + shift)
    tail = findex[nl:]
    tail = np.where(tail >= 0, needed[np.maximum(tail, 0)], -1)
    return table[nl:], voronoi._pack_rows(keys, ids), tail, None if interp is None else interp + shift


def program_input(p, add_vertices, skip_concave):
    """The text tests/native/voronoi_boundary_main.cpp reads: sizes and flags, then one array per line (floats in hex)."""
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).ravel())  # noqa: E731
    hexes = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())  # noqa: E731
    head = f"{p['n_face']} {p['nodes'].size} {p['edge_face'].size} {p['faces'].size} {int(add_vertices)} {int(skip_concave)}"
    lines = [head, ints(p["nodes"]), ints(p["row_ptr"]), ints(p["faces"]), hexes(p["face_xy"]), hexes(p["node_xy"]),
             ints(p["edge_nodes"][:, 0]), ints(p["edge_nodes"][:, 1]), ints(p["edge_face"]), hexes(p["edge_face_xy"])]
    return "\n".join(lines) + "\n"


def program_output(text):
    """-> (status, extra_xy, cells, tail, interp)"""
    lines = text.split("\n")
    status = int(lines[0])
    if status != 0:
        return status, None, None, None, None
    n_extra, n_cell, m, n_tail, n_map = (int(v) for v in lines[1].split())
    extra = np.array([float.fromhex(v) for v in lines[2].split()]).reshape(n_extra, 2)
    cells = np.array(lines[3].split(), dtype=np.int64).reshape(n_cell, m)
    tail = np.array(lines[4].split(), dtype=np.int64)
    interp = np.array(lines[5].split(), dtype=np.int64).reshape(n_map, 2)
    assert tail.size == n_tail
    return status, extra, cells, tail, interp
