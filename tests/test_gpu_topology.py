"""
GPU (-m gpu): the edge topology built on the device (csrc/xr_topology.hip, xugrid_amd/topology.py).  Every array is compared
with ``np.array_equal`` against the project's host route (xugrid_amd/connectivity.py) on the same faces
(tests/graph_cases.py: host_topology).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial import Delaunay

import graph_cases as gc
import xugrid_amd as xa
from graph_cases import device_grid
from xugrid_amd import _lib

pytestmark = pytest.mark.gpu

class _Meshes:
    """name -> (node_xy, faces), made when a test asks (graph_cases.topology_mesh)."""

    def __getitem__(self, name):
        return gc.topology_mesh(name)


MESHES = _Meshes()


def assert_csr_equal(got, exp):
    assert got.shape == exp.shape
    assert np.array_equal(got.indptr, exp.indptr)
    assert np.array_equal(got.indices, exp.indices)
    assert np.array_equal(got.data, exp.data)


def assert_topology_equal(topology, faces, n_node):
    exp = gc.host_topology(faces, n_node)
    assert topology.manifold
    assert topology.n_edge == len(exp["edge_node"])
    assert np.array_equal(topology.edge_node_connectivity, exp["edge_node"])
    assert np.array_equal(topology.face_edge_connectivity, exp["face_edge"])
    assert np.array_equal(topology.edge_face_connectivity, exp["edge_face"])
    assert_csr_equal(topology.face_face_connectivity, exp["face_face"])
    assert_csr_equal(topology.node_node_connectivity, exp["node_node"])
    exterior = exp["edge_face"][:, 1] == -1
    assert topology.n_exterior_edge == exterior.sum()
    assert np.array_equal(topology.exterior_edges, np.nonzero(exterior)[0])
    assert np.array_equal(topology.exterior_faces, np.unique(exp["edge_face"][exterior, 0]))
    return exp


@pytest.mark.parametrize("name", gc.TOPOLOGY_MESH_NAMES)
def test_topology_equals_host_route(name):
    xy, faces = MESHES[name]
    grid = device_grid(xy, faces)
    exp = assert_topology_equal(grid.device_topology(), faces, len(xy))
    if name == "one_triangle":
        assert grid.device_topology().face_face_nnz == 0 and grid.device_topology().n_exterior_edge == 3
    if name in ("fan70", "hubs"):  # the wave-per-node kernel made these lists
        degree = np.diff(exp["node_node"].indptr)
        assert (degree > 16).sum() == {"fan70": 1, "hubs": 304}[name]
        assert grid.device_topology().n_long_nodes == (degree > 16).sum()
    if name == "two_shared_edges":  # ONE entry per pair of faces, the two edge ids summed
        assert exp["face_face"].nnz == 2 and grid.device_topology().face_face_nnz == 2
    # the grid's properties come from the topology, without a host copy of the mesh
    assert np.array_equal(grid.edge_node_connectivity, exp["edge_node"]) and grid.n_edge == len(exp["edge_node"])
    assert np.array_equal(grid.exterior_edges, np.nonzero(exp["edge_face"][:, 1] == -1)[0])
    assert grid._host is None


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_face_table_dtypes(dtype):
    xy, faces = MESHES["mixed900"]
    assert_topology_equal(device_grid(xy, faces, dtype).device_topology(), faces, len(xy))


def test_host_grid_has_a_device_topology_too():
    xy, faces = MESHES["mixed900"]
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert_topology_equal(grid.device_topology(), faces, len(xy))
    assert np.array_equal(grid.exterior_edges, grid.device_topology().exterior_edges)
    assert np.array_equal(grid.exterior_faces, grid.device_topology().exterior_faces)


def test_non_manifold_edge_takes_the_host_route():
    """Three triangles on the edge (0, 1)."""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0], [0.5, -1.0], [0.5, 0.4]])
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    grid = device_grid(xy, faces)
    topology = grid.device_topology()
    assert topology.n_nonmanifold == 1 and not topology.manifold
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert np.array_equal(grid.edge_node_connectivity, host.edge_node_connectivity)
    assert np.array_equal(grid.edge_face_connectivity, host.edge_face_connectivity)
    assert grid.edge_face_connectivity.shape[1] == 3
    assert grid.n_edge == host.n_edge
    data = np.array([1.0, np.nan, 3.0])
    assert np.array_equal(grid.laplace_interpolate(data), host.laplace_interpolate(data))


@pytest.mark.parametrize("name", ["fan70", "hubs", "mixed900", "permuted40k"])
def test_edge_midpoints_bit_for_bit(name):
    xy, faces = MESHES[name]
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    grid = device_grid(xy, faces)
    assert np.array_equal(grid.device_topology().edge_coordinates_device().download(), host.edge_coordinates)
    assert np.array_equal(grid.edge_coordinates, host.edge_coordinates)


@pytest.mark.parametrize("facet", ["face", "node"])
@pytest.mark.parametrize("name", ["two_shared_edges", "mixed900", "permuted40k"])
def test_graph_weights_against_fsum(name, facet):
    """mean(d) / d: any summation order of nnz positive terms is within nnz * 2^-53 relative of the exact mean (math.fsum);
    sqrt and the divide add at most 2 ulp.  Two builds of the same topology give the same bits."""
    xy, faces = MESHES[name]
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    topology = device_grid(xy, faces).device_topology()
    graph = topology.graph(facet)
    indptr, indices, weights = graph.download()
    conn = host.face_face_connectivity if facet == "face" else host.node_node_connectivity
    assert np.array_equal(indptr, conn.indptr) and np.array_equal(indices, conn.indices)
    exp = gc.fsum_weights(indptr, indices, host.centroids if facet == "face" else host.node_coordinates)
    tol = indices.size * 2.0**-53 + 2 * 2.0**-52
    rel = np.abs(weights - exp) / exp
    print(f"{name} {facet}: nnz {indices.size}, max relative error {rel.max():.3e}, tolerance {tol:.3e}")
    assert rel.max() <= tol
    again = topology.graph(facet).download()[2]
    assert np.array_equal(again.view(np.int64), weights.view(np.int64))
    other = device_grid(xy, faces).device_topology().graph(facet).download()[2]
    assert np.array_equal(other.view(np.int64), weights.view(np.int64))


@pytest.mark.parametrize("n_node,seed", [(250, 250), (256, 256), (257, 257), (65_536, 7), (65_537, 2)])
def test_graph_weights_in_the_order_of_the_reduction(n_node, seed):
    """The mean distance is a sum of doubles in a fixed order (csrc/xr_prims.h): threads, butterfly, waves, then the fold of
    the blocks' partials -- restated in numpy and compared bit for bit.  The rows are the nodes of a Delaunay mesh: less than
    a block, one block, one block and a lane, 256 partials and 257 (thread 0 of the fold takes two).  At these seeds the
    sum in this order differs from the correctly rounded one or from numpy's pairwise one: another order would show."""
    xy = np.random.default_rng(seed).random((n_node, 2))
    faces = Delaunay(xy).simplices.astype(np.int64)
    indptr, indices, weights = device_grid(xy, faces).device_topology().graph("node").download()
    assert len(indptr) == n_node + 1
    expected = gc.ordered_weights(indptr, indices, xy)
    assert np.array_equal(weights.view(np.int64), expected.view(np.int64))


def test_drop_device_caches_drops_the_topology():
    xy, faces = MESHES["mixed900"]
    grid = device_grid(xy, faces)
    first = grid.device_topology()
    assert grid.device_topology() is first
    weights = first.graph("face").download()[2]
    grid.drop_device_caches()
    assert grid.device_topology() is not first
    assert_topology_equal(grid.device_topology(), faces, len(xy))
    # a topology the caller still holds keeps answering: its arrays need the faces alone, the mesh rebuilds its centroids
    assert_topology_equal(first, faces, len(xy))
    assert np.array_equal(first.graph("face").download()[2], weights)


def test_download_accepts_null_pointers():
    xy, faces = MESHES["two_triangles"]
    topology = device_grid(xy, faces).device_topology()
    _lib.check(_lib.load().xr_topology_download(topology._h, *([None] * 11)))
    out = np.empty((topology.n_edge, 2), dtype=np.int64)
    _lib.check(_lib.load().xr_topology_download(topology._h, out.ctypes.data_as(ctypes.c_void_p), *([None] * 10)))
    assert np.array_equal(out, [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]])


def test_no_host_detour_on_a_device_grid():
    """The torch / device-only route, in a child process (torch's HIP runtime has to be up before the engine binds the
    device): fills and components on a DeviceUgrid2d never download the mesh."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "topology_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_TOPOLOGY_OK" in res.stdout
