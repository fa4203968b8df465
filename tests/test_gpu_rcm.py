"""
GPU (-m gpu): renumbering on the device (xugrid_amd/graph.py: reverse_cuthill_mckee; Ugrid2d.reverse_cuthill_mckee; kernels in
csrc/xr_rcm.hip) against tests/rcm_cases.py with ``array_equal``: against scipy and ``sequential`` where no seed is tied (the
precondition is asserted on the fixture), against ``sequential`` alone elsewhere.
"""
import numpy as np
import pytest
from scipy.sparse import block_diag, csr_matrix
from scipy.sparse.csgraph import reverse_cuthill_mckee as scipy_rcm

import graph_cases as gc
import rcm_cases as rc
import xugrid_amd as xa
from graph_cases import device_grid
from network_cases import raster_quads
from xugrid_amd import engine, graph

pytestmark = pytest.mark.gpu

_MADE = {}


def eared():
    """The eared Delaunay mesh of 300 points -> (xy, faces, adjacency, sequential order); made once."""
    if "eared" not in _MADE:
        xy, faces = rc.with_ear(*rc.delaunay(300, 0))
        A = rc.face_graph(faces)
        assert rc.seed_ties(A) == 0
        _MADE["eared"] = xy, faces, A, rc.sequential(A)
    return _MADE["eared"]


def host_grid(xy, faces):
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


def test_chain():
    assert np.array_equal(xa.reverse_cuthill_mckee(gc.chain(5)), [4, 3, 2, 1, 0])


@pytest.mark.parametrize("kind", ["host", "device"])
def test_eared_delaunay(kind):
    xy, faces, A, expected = eared()
    assert np.array_equal(expected, scipy_rcm(A, symmetric_mode=True))
    grid = host_grid(xy, faces) if kind == "host" else device_grid(xy, faces)
    reordered, reordering = grid.reverse_cuthill_mckee()
    assert isinstance(reordering, np.ndarray) and reordering.dtype == np.int64
    assert np.array_equal(reordering, expected)
    assert type(reordered) is type(grid) and reordered.name == grid.name
    assert np.array_equal(reordered.face_node_connectivity, faces[expected])
    assert np.array_equal(reordered.node_coordinates, xy)  # bit for bit
    assert np.array_equal(grid.face_node_connectivity, faces)  # the grid itself is unchanged
    # data (3, n_face): numpy in -> numpy out, torch in -> float64 torch out
    data = np.random.default_rng(3).random((3, len(faces)))
    _, again, moved = grid.reverse_cuthill_mckee(dimension=grid.face_dimension, data=data)
    assert np.array_equal(again, expected)  # a second run: the same permutation
    assert isinstance(moved, np.ndarray) and np.array_equal(moved, data[:, expected])
    # a device array in -> a float64 device array out; return_device: the index stays in HBM for a grid that lives there
    _, index, moved = grid.reverse_cuthill_mckee(data=engine.DeviceArray.from_host(data.astype(np.float32)), return_device=True)
    assert isinstance(moved, engine.DeviceArray) and moved.dtype == np.float64
    assert np.array_equal(moved.download(), data.astype(np.float32)[:, expected].astype(np.float64))
    if kind == "device":
        assert isinstance(index, engine.DeviceArray) and index.dtype == np.int64 and np.array_equal(index.download(), expected)
    else:
        assert isinstance(index, np.ndarray) and np.array_equal(index, expected)


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/rcm_worker_gpu.py): torch data through reverse_cuthill_mckee on both kinds of grid, the index as a tensor
def test_torch_in_torch_out():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rcm_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_RCM_OK" in res.stdout


def test_unused_nodes_are_kept():
    xy, faces = gc.topology_mesh("unused_nodes")
    for grid in (host_grid(xy, faces), device_grid(xy, faces)):
        reordered, reordering = grid.reverse_cuthill_mckee()
        assert np.array_equal(reordering, rc.sequential(rc.face_graph(faces)))
        assert reordered.n_node == len(xy) and np.array_equal(reordered.node_coordinates, xy)
        assert np.array_equal(reordered.face_node_connectivity, faces[reordering])


TIE_HEAVY = {
    "delaunay": lambda: rc.delaunay(300, 0),
    "raster": lambda: raster_quads(np.arange(10.0), np.arange(8.0)),  # 7 x 9 quads: four corners of degree 2
    "mixed": lambda: gc.topology_mesh("mixed900"),
}


@pytest.mark.parametrize("name", list(TIE_HEAVY))
def test_tied_seeds_follow_the_stable_order(name):
    xy, faces = TIE_HEAVY[name]()
    A = rc.face_graph(faces)
    assert rc.seed_ties(A) > 0
    expected = rc.sequential(A)
    for grid in (host_grid(xy, faces), device_grid(xy, faces)):
        reordered, reordering = grid.reverse_cuthill_mckee()
        assert np.array_equal(reordering, expected)
        assert np.array_equal(reordered.face_node_connectivity, np.asarray(faces)[expected])


def test_component_after_an_isolated_face():
    xy, faces, _, _ = eared()
    xy, faces = rc.join((xy, faces), rc.isolated_triangles(1))
    A = rc.face_graph(faces)
    assert rc.seed_ties(A) == 0  # seeds of degree 0, then 1
    expected = scipy_rcm(A, symmetric_mode=True)
    assert np.array_equal(expected, rc.sequential(A))
    for grid in (host_grid(xy, faces), device_grid(xy, faces)):
        assert np.array_equal(grid.reverse_cuthill_mckee()[1], expected)


def test_thousands_of_components():
    xy, faces = rc.join(rc.delaunay(400, 1), rc.isolated_triangles(3000), rc.delaunay(250, 2))
    A = rc.face_graph(faces)
    expected, widths = rc.level_form(A)
    assert np.array_equal(expected, rc.sequential(A))
    assert np.array_equal(device_grid(xy, faces).reverse_cuthill_mckee()[1], expected)
    assert graph.last_levels == len(widths)


def test_wide_frontier():
    xy, faces = rc.delaunay(26_000, 0)
    A = rc.face_graph(faces)
    expected, widths = rc.level_form(A)
    assert max(widths) > 2 * graph.RCM_BLOCK  # a level takes more than two blocks of the level kernels
    assert np.array_equal(expected, rc.sequential(A))
    assert np.array_equal(xa.reverse_cuthill_mckee(A), expected)
    assert graph.last_levels == len(widths)


HUBS = {
    "star": lambda: rc.hub_graph(3000),  # a row longer than a block; every leaf of degree 1
    # leaves of degree 1, 2 (a tail) and 3 (a tail and a diagonal entry) within the one long row; rows with a diagonal entry
    "tails": lambda: rc.hub_graph(3000, tails=[(k, 1 + k % 3) for k in range(3, 3000, 7)], diagonal=[0, 7, 10, 17, 2999]),
    # every leaf with a tail of 1 .. 3: several consecutive levels of 5000 vertices of differing degree, twenty blocks each
    "broom": lambda: rc.hub_graph(5000, tails=[(k, 1 + k % 3) for k in range(1, 5001)]),
    # two components, each with a row longer than a block
    "two_hubs": lambda: block_diag([rc.hub_graph(700, tails=[(k, 2) for k in range(1, 700, 3)]), rc.hub_graph(1200, diagonal=[3])]),
}


@pytest.mark.parametrize("name", list(HUBS))
def test_hub(name):
    A = rc.canonical(HUBS[name]())
    assert np.diff(A.indptr).max() > 2 * graph.RCM_BLOCK
    expected, widths = rc.level_form(A)
    assert np.array_equal(expected, rc.sequential(A))
    assert np.array_equal(xa.reverse_cuthill_mckee(A), expected)
    assert graph.last_levels == len(widths)


def test_level_wider_than_the_grid():
    """A level of more vertices than one turn of the level kernels' grid takes, and a row of as many entries."""
    n_leaves = graph.RCM_GRID * graph.RCM_BLOCK + 7000
    A = rc.hub_graph(n_leaves, tails=[(n_leaves - 3, 2)])
    expected, widths = rc.level_form(A)
    assert max(widths) > graph.RCM_GRID * graph.RCM_BLOCK
    assert np.array_equal(expected, rc.sequential(A))
    assert np.array_equal(xa.reverse_cuthill_mckee(A), expected)


def test_repeated_entries_place_no_vertex_twice():
    """A CSR that stores a column twice in a row, handed over as it is: every vertex is still placed once."""
    A = rc.hub_graph(40, tails=[(3, 2), (9, 1)])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    twice = np.sort(np.concatenate([np.arange(A.nnz), np.arange(0, A.nnz, 3)]))  # every third entry stored twice
    doubled = csr_matrix((np.ones(twice.size), A.indices[twice], np.searchsorted(rows[twice], np.arange(A.shape[0] + 1))), shape=A.shape)
    assert doubled.nnz > A.nnz and not doubled.has_canonical_format
    from xugrid_amd.fill import DeviceGraph

    order = graph.rcm(DeviceGraph(doubled))
    assert np.array_equal(np.sort(order), np.arange(A.shape[0]))
    assert np.array_equal(xa.reverse_cuthill_mckee(doubled), rc.sequential(A))  # the public function sums them first


def test_diagonal_entry_counts_in_the_degree():
    A = rc.hub_graph(3, diagonal=[2])
    assert np.array_equal(xa.reverse_cuthill_mckee(A), [2, 3, 0, 1])


def test_degenerate():
    assert np.array_equal(xa.reverse_cuthill_mckee(csr_matrix((1, 1))), [0])
    xy, faces = gc.topology_mesh("one_triangle")
    for grid in (host_grid(xy, faces), device_grid(xy, faces)):
        reordered, reordering = grid.reverse_cuthill_mckee()
        assert np.array_equal(reordering, [0]) and np.array_equal(reordered.face_node_connectivity, faces)
    xy, faces = rc.isolated_triangles(5)  # faces without neighbours only: seeds in id order, reversed
    for grid in (host_grid(xy, faces), device_grid(xy, faces)):
        assert np.array_equal(grid.reverse_cuthill_mckee()[1], [4, 3, 2, 1, 0])


def test_no_faces_behaves_as_the_sibling_methods():
    grid = host_grid(np.random.default_rng(0).random((3, 2)), np.empty((0, 3), dtype=np.int64))
    try:
        grid.connected_components()
        raised = None
    except Exception as e:  # noqa: BLE001  (whatever the sibling raises is the yardstick)
        raised = type(e)
    if raised is None:
        reordered, reordering = grid.reverse_cuthill_mckee()
        assert reordering.shape == (0,) and reordered.n_face == 0 and reordered.n_node == 3
    else:
        with pytest.raises(raised):
            grid.reverse_cuthill_mckee()


def test_other_dimensions_are_refused():
    xy, faces, _, _ = eared()
    grid = host_grid(xy, faces)
    with pytest.raises(ValueError, match="mesh2d_nFaces"):
        grid.reverse_cuthill_mckee(dimension="mesh2d_nNodes")
    with pytest.raises(ValueError):
        grid.reverse_cuthill_mckee(dimension="mesh2d_nEdges")
    with pytest.raises(ValueError, match="square"):
        xa.reverse_cuthill_mckee(csr_matrix((3, 4)))


def test_levels():
    xy, faces, A, expected = eared()
    widths = rc.level_form(A)[1]
    assert len(widths) > 1
    assert np.array_equal(graph.rcm(graph._graph_of(A)), expected)
    assert graph.last_levels == len(widths)
