"""Shared cases and numpy yardsticks of the topology / graph tests (test_graph_cpu.py, test_gpu_topology.py, test_gpu_graph.py,
topology_worker_gpu.py).  The yardsticks are the project's own host route (xugrid_amd/connectivity.py), scipy, and the few
lines of numpy below, written from the rules of xugrid_amd/graph.py's docstring."""
import math

import numpy as np
from scipy import sparse

from xugrid_amd import connectivity, meshgen


# ---- numpy restatement of the binary iteration
def binary_iterate(conn, a, value, iterations=1, mask=None, exterior=None, border_value=False):
    """One iteration = a Jacobi step on a snapshot: an entry becomes ``value`` iff a neighbour's old state differs from its
    own; then ``mask`` entries become ``not value``; after the first step only, ``exterior`` entries become ``value`` (used
    when ``border_value == value`` only).  ``conn``: symmetric scipy sparse; ``a``: bool (n,); never modified."""
    coo = sparse.coo_matrix(conn)
    out = np.array(a, dtype=bool)
    for it in range(iterations):
        old = out.copy()
        differs = np.zeros(out.size, dtype=bool)
        np.logical_or.at(differs, coo.row, old[coo.row] != old[coo.col])
        out = np.where(differs, value, old)
        if mask is not None:
            out[mask] = not value
        if it == 0 and exterior is not None and bool(border_value) == bool(value):
            out[exterior] = value
    return out


def component_numbers(labels):
    """Smallest-member labels -> the rank of each component's smallest member (the claimed scipy numbering)."""
    labels = np.asarray(labels)
    return np.cumsum(labels == np.arange(labels.size))[labels] - 1


def smallest_member_labels(conn):
    """The smallest node id of every component (what xr_graph keeps), by propagation to a fixed point in numpy."""
    coo = sparse.coo_matrix(conn)
    lab = np.arange(coo.shape[0])
    while True:
        new = lab.copy()
        np.minimum.at(new, coo.row, lab[coo.col])
        if np.array_equal(new, lab):
            return lab
        lab = new


def chain(n=5):
    """The chain 0 - 1 - ... - (n-1), symmetric CSR."""
    i = np.arange(n - 1)
    return sparse.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([i, i + 1]), np.concatenate([i + 1, i]))), shape=(n, n)).tocsr()


# ---- meshes: (name, node_xy, faces)
def _unit_xy(n, seed=0):
    return np.random.default_rng(seed).random((n, 2))


def fan(n_tri=70):
    """n_tri triangles about node 0: more neighbours than a wave has lanes."""
    ang = np.linspace(0.0, 1.9 * np.pi, n_tri + 1)
    xy = np.vstack([[0.0, 0.0], np.column_stack([np.cos(ang), np.sin(ang)])])
    k = np.arange(n_tri)
    return xy, np.column_stack([np.zeros(n_tri, dtype=np.int64), k + 1, k + 2])


def hubs():
    """304 fans side by side: hubs of 17 .. 25 neighbours (more than a thread's list of 16, fewer than a wave's 64 lanes) and
    of 64, 65, 66 and 101; more hubs than the wave-per-node kernel has blocks, so its loop over the list of such nodes takes
    a second turn.  Every other fan is numbered backwards: its hub is then the highest node of its fan and owns no edge."""
    sizes = [16 + i % 9 for i in range(300)] + [63, 64, 65, 100]
    xys, tables, base = [], [], 0
    for i, n_tri in enumerate(sizes):
        xy, faces = fan(n_tri)
        if i % 2:
            xy, faces = xy[::-1], len(xy) - 1 - faces
        xys.append(xy + [3.0 * i, 0.0])
        tables.append(faces + base)
        base += len(xy)
    return np.vstack(xys), np.vstack(tables)


def strip(n=3000):
    """1 x n quads."""
    return meshgen.quad_mesh(np.arange(n + 1, dtype=float), np.array([0.0, 1.0]))


def disconnected():
    """Two separated triangle patches, one isolated triangle, unused node ids in the middle and beyond the highest used."""
    xy1, f1 = meshgen.triangle_mesh(30, 1)
    xy2, f2 = meshgen.triangle_mesh(20, 2)
    gap = 3  # unused ids between the patches
    o2 = len(xy1) + gap
    o3 = o2 + len(xy2)
    xy = np.vstack([xy1, np.full((gap, 2), 9.0), xy2 + [2.0, 0.0], [[4.0, 0.0], [5.0, 0.0], [4.0, 1.0]], np.full((4, 2), 9.0)])
    faces = np.vstack([f1, f2 + o2, [[o3, o3 + 1, o3 + 2]]])
    return xy, faces


_BIG = {}


def big_triangles():
    """~40k triangles (many blocks), qhull numbering; made once."""
    if "mesh" not in _BIG:
        _BIG["mesh"] = meshgen.triangle_mesh(20_000, 0)
    return _BIG["mesh"]


def big_permuted():
    """The same mesh with its faces randomly permuted (incoherent numbering)."""
    if "perm" not in _BIG:
        xy, faces = big_triangles()
        _BIG["perm"] = xy, faces[np.random.default_rng(5).permutation(len(faces))]
    return _BIG["perm"]


# the meshes of test_gpu_topology.py, smallest first: name -> maker of (node_xy, faces); made on first use and kept
_TOPOLOGY_MESHES = {
    "one_triangle": lambda: (_unit_xy(3), np.array([[0, 1, 2]])),
    "two_triangles": lambda: (_unit_xy(4), np.array([[0, 1, 2], [1, 3, 2]])),
    "mixed_tri_quad": lambda: (_unit_xy(7), np.array([[0, 1, 2, -1], [1, 3, 4, 2], [4, 5, 6, -1]])),
    "two_shared_edges": lambda: (np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [3.0, 2.0]]),
                                 np.array([[0, 1, 2, 3], [1, 4, 3, 2]])),
    "fan70": lambda: fan(70),
    "hubs": hubs,
    "unused_nodes": lambda: (_unit_xy(12), np.array([[0, 1, 2], [1, 5, 2], [5, 8, 2]])),
    "mixed900": lambda: meshgen.mixed_mesh(900, 3),
    "triangles40k": big_triangles,
    "permuted40k": big_permuted,
}
TOPOLOGY_MESH_NAMES = tuple(_TOPOLOGY_MESHES)
_MADE = {}


def topology_mesh(name):
    if name not in _MADE:
        _MADE[name] = _TOPOLOGY_MESHES[name]()
    return _MADE[name]


def device_grid(xy, faces, dtype=np.int64):
    """A grid whose mesh lives in HBM only (``Ugrid2d.from_device_arrays``)."""
    import xugrid_amd as xa
    from xugrid_amd import engine

    xy_dev = engine.DeviceArray.from_host(np.ascontiguousarray(xy, dtype=np.float64))
    faces_dev = engine.DeviceArray.from_host(np.ascontiguousarray(faces, dtype=dtype))
    grid = xa.Ugrid2d.from_device_arrays(xy_dev, faces_dev)
    grid._keep = (xy_dev, faces_dev)
    return grid


def host_topology(faces, n_node):
    """The host route on ``faces``: dict of the arrays xr_topology produces.  ``invert_dense`` makes edge_face as wide as the
    busiest edge -- one column where no edge is shared; the device table always has two, so a single column is padded with -1."""
    faces = np.asarray(faces, dtype=np.intp)
    edge_node, face_edge = connectivity.edge_connectivity(faces)
    edge_face = connectivity.invert_dense(face_edge)
    if edge_face.shape[1] < 2:
        edge_face = np.column_stack([edge_face, np.full(len(edge_face), -1, dtype=edge_face.dtype)])
    return {
        "edge_node": edge_node, "face_edge": face_edge, "edge_face": edge_face,
        "face_face": connectivity.face_face_connectivity(edge_face, len(faces)),
        "node_node": connectivity.node_node_connectivity(edge_node, n_node),
    }


def fsum_weights(indptr, indices, xy):
    """mean(d) / d with the mean taken by math.fsum (exact up to one rounding) -> (weights, nnz)."""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    d = xy[indices] - xy[rows]
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return (math.fsum(dist) / dist.size) / dist


# ---- the summation order of the device reductions (csrc/xr_prims.h), restated -------------------------------------------------
def block_sums(values):
    """One value per thread -> one sum per block of 256: in every wave of 64 the xor butterfly over the offsets 32 .. 1,
    then the four wave sums added in ascending wave number."""
    v = np.zeros(-(-len(values) // 256) * 256)
    v[:len(values)] = values
    v = v.reshape(-1, 4, 64)
    lanes = np.arange(64)
    for offset in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ offset]
    wave = v[:, :, 0]
    return ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]


def folded_sum(partials):
    """One block folds the partials: thread t adds the partials t, t + 256, ... to 0.0 in that order, then ``block_sums``."""
    t = np.zeros(256)
    for first in range(0, len(partials), 256):
        piece = partials[first:first + 256]
        t[:len(piece)] += piece
    return block_sums(t)[0]


def ordered_weights(indptr, indices, xy):
    """mean(d) / d as the device computes it, bit for bit: a thread adds the distances of its row in entry order, the rows go
    through ``block_sums`` and the blocks through ``folded_sum``."""
    indptr = np.asarray(indptr, dtype=np.int64)
    degree = np.diff(indptr)
    rows = np.repeat(np.arange(len(degree)), degree)
    d = xy[indices] - xy[rows]
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    row_sum = np.zeros(len(degree))
    for k in range(int(degree.max())):
        has = degree > k
        row_sum[has] += dist[indptr[:-1][has] + k]
    return (folded_sum(block_sums(row_sum)) / dist.size) / dist
