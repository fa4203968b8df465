"""
GPU: the network edits (csrc/xr_netedit.hip) behind ``Ugrid1d.topology_subset`` / ``isel`` / ``sel`` / ``clip_box`` /
``remove_self_loops`` / ``merge_partitions`` / ``reindex_like`` / ``refine_by_vertices``.  Yardsticks in tests/netedit_cases.py: numpy
restatements of the reference, pinned to the reference's own output by tests/test_netedit_cpu.py.  Every comparison is exact:
ids are integers and coordinates are copied, so they are compared bit for bit.
"""
import numpy as np
import pytest

import netedit_cases as nc
import xugrid_amd as xa
from xugrid_amd import engine

pytestmark = pytest.mark.gpu


def grid_of(xy, edges):
    return xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges, name="net")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_network(grid, xy, edges):
    assert isinstance(grid, xa.Ugrid1d) and grid.name == "net"
    assert grid.node_coordinates.shape == xy.shape and np.array_equal(bits(grid.node_coordinates), bits(xy))
    assert np.array_equal(grid.edge_node_connectivity, edges.reshape(-1, 2))


def assert_index(got, want):
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)


# ---- subset ---------------------------------------------------------------------------------------------------------------------------
CHAIN = nc.chain(2050)  # 2049 edges: one past the 2048-element scan tile
RANDOM = nc.random_network(2000)
SELECTIONS = {
    "chain_reversed": lambda: CHAIN + (np.arange(2048, -1, -1),),
    "chain_every_other": lambda: CHAIN + (np.arange(0, 2049, 2),),
    "chain_one": lambda: CHAIN + (np.array([1000]),),
    "chain_last": lambda: CHAIN + (np.array([2048]),),
    "random_permuted": lambda: RANDOM + (np.random.default_rng(50).permutation(len(RANDOM[1]))[:1000],),
    "hub300": lambda: nc.hub(300) + (np.random.default_rng(51).permutation(600)[:450],),
    "unused_nodes": lambda: nc.unused_nodes() + (np.random.default_rng(52).permutation(329)[:200],),
}


@pytest.mark.parametrize("name", sorted(SELECTIONS))
def test_topology_subset(hip, name):
    xy, edges, index = SELECTIONS[name]()
    grid = grid_of(xy, edges)
    e_xy, e_edges, e_nodes = nc.subset_ref(xy, edges, index)
    assert_network(grid.topology_subset(index), e_xy, e_edges)
    sub, indexes = grid.topology_subset(index, return_index=True)
    assert_network(sub, e_xy, e_edges)
    assert set(indexes) == {grid.node_dimension, grid.edge_dimension}
    assert_index(indexes[grid.node_dimension], e_nodes)
    assert_index(indexes[grid.edge_dimension], index)
    # ... and the same from a device index
    sub, indexes = grid.topology_subset(engine.DeviceArray.from_host(index.astype(np.int64)), return_index=True)
    assert_network(sub, e_xy, e_edges)
    assert isinstance(indexes[grid.node_dimension], engine.DeviceArray) and np.array_equal(indexes[grid.node_dimension].download(), e_nodes)


def test_topology_subset_edge_selections(hip):
    xy, edges = CHAIN
    grid = grid_of(xy, edges)
    everything = np.arange(2049)
    assert grid.topology_subset(everything) is grid
    same, indexes = grid.topology_subset(everything, return_index=True)
    assert same is grid
    assert_index(indexes[grid.node_dimension], np.arange(2050))
    assert_index(indexes[grid.edge_dimension], everything)
    assert grid.topology_subset(np.ones(2049, dtype=bool)) is grid
    empty, indexes = grid.topology_subset([], return_index=True)
    assert empty.n_node == 0 and empty.n_edge == 0 and empty.edge_node_connectivity.shape == (0, 2)
    assert indexes[grid.node_dimension].size == 0 and indexes[grid.edge_dimension].size == 0
    mask = np.random.default_rng(53).random(2049) < 0.5
    sub, indexes = grid.topology_subset(mask, return_index=True)
    assert_network(sub, *nc.subset_ref(xy, edges, np.flatnonzero(mask))[:2])
    assert_index(indexes[grid.edge_dimension], np.flatnonzero(mask))


def test_topology_subset_refusals_leave_the_grid_usable(hip):
    xy, edges = RANDOM
    grid = grid_of(xy, edges)
    n = grid.n_edge
    device = lambda ids: engine.DeviceArray.from_host(np.asarray(ids, dtype=np.int64))  # noqa: E731
    for make in (np.asarray, device):
        with pytest.raises(ValueError, match="repeated"):
            grid.topology_subset(make([5, 7, 5]))
        with pytest.raises(IndexError):
            grid.topology_subset(make([0, n]))
        with pytest.raises(IndexError):
            grid.topology_subset(make([3, -1]))
        with pytest.raises(ValueError, match="larger than dimension size"):
            grid.topology_subset(make(np.zeros(n + 1, dtype=np.int64)))
    with pytest.raises(TypeError):
        grid.topology_subset(np.array([0.5, 1.0]))
    with pytest.raises(TypeError):
        grid.topology_subset(engine.DeviceArray.from_host(np.array([0.5, 1.0])))
    with pytest.raises(ValueError, match="1d"):
        grid.topology_subset(np.zeros((2, 2), dtype=np.int64))
    index = np.arange(10, 20)
    assert_network(grid.topology_subset(index), *nc.subset_ref(xy, edges, index)[:2])


def test_isel_data_on_both_facets(hip):
    xy, edges = RANDOM
    grid = grid_of(xy, edges)
    index = np.random.default_rng(54).permutation(grid.n_edge)[:700]
    e_xy, e_edges, e_nodes = nc.subset_ref(xy, edges, index)
    rng = np.random.default_rng(55)
    node_data, edge_data = rng.random((2, grid.n_node)), rng.random(grid.n_edge).astype(np.float32)
    sub, values = grid.isel({grid.edge_dimension: index}, data=node_data)
    assert_network(sub, e_xy, e_edges)
    assert np.array_equal(values, node_data[:, e_nodes])
    sub, indexes, values = grid.isel(return_index=True, data=edge_data, **{grid.edge_dimension: index})
    assert np.array_equal(values, edge_data[index])
    assert_index(indexes[grid.node_dimension], e_nodes)
    got = grid.isel({grid.edge_dimension: index}, data=engine.DeviceArray.from_host(edge_data))[1]
    assert isinstance(got, engine.DeviceArray) and got.dtype == np.float64 and np.array_equal(got.download(), edge_data[index].astype(np.float64))


# ---- isel / sel / clip_box ---------------------------------------------------------------------------------------------------------------
def test_isel_by_nodes(hip):
    xy, edges = nc.two_components()
    grid = grid_of(xy, edges)
    component = np.arange(40, 65)
    e_xy, e_edges, _ = nc.subset_ref(xy, edges, np.arange(39, 63))
    sub, indexes = grid.isel({grid.node_dimension: component}, return_index=True)
    assert_network(sub, e_xy, e_edges)
    assert_index(indexes[grid.edge_dimension], np.arange(39, 63))
    assert_index(indexes[grid.node_dimension], component)
    assert_network(grid.isel({grid.node_dimension: component, grid.edge_dimension: np.arange(39, 63)}), e_xy, e_edges)
    with pytest.raises(ValueError, match="results in an invalid topology"):
        grid.isel({grid.node_dimension: component[:-1]})
    with pytest.raises(ValueError, match="UGRID dimensions do not align"):
        grid.isel({grid.node_dimension: component, grid.edge_dimension: np.arange(39, 62)})
    with pytest.raises(ValueError, match="do not exist"):
        grid.isel({"net_nFaces": [0]})
    # the node selection of a device array
    sub = grid.isel({grid.node_dimension: engine.DeviceArray.from_host(component.astype(np.int64))})
    assert_network(sub, e_xy, e_edges)
    assert np.array_equal(nc.edges_of_nodes_ref(edges, len(xy), component), np.arange(39, 63))


def test_sel_and_clip_box(hip):
    # midpoints at x = 0.5, 1.5, .. 9.5 on y = 0; one node with a NaN coordinate
    xy, edges = nc.int_chain(11)
    xy = np.concatenate([xy, [[np.nan, 0.0]]])
    edges = np.concatenate([edges, [[10, 11]]])
    grid = grid_of(xy, edges)
    for box in ((1.5, -1.0, 4.5, 1.0), (0.0, 0.0, 100.0, 1e-300), (-5.0, -5.0, 0.5, 5.0), (2.0, 0.5, 3.0, 1.0)):
        want = nc.box_edges_ref(xy, edges, *box)
        assert_network(grid.clip_box(*box), *nc.subset_ref(xy, edges, want)[:2])
    assert nc.box_edges_ref(xy, edges, 1.5, -1.0, 4.5, 1.0).tolist() == [1, 2, 3]  # (on xmin: in; on xmax: out)
    assert nc.box_edges_ref(xy, edges, 0.0, 0.0, 100.0, 1e-300).tolist() == list(range(10))  # (the NaN midpoint is out)
    sub, indexes = grid.sel(x=slice(None, 3.0), return_index=True)
    assert_index(indexes[grid.edge_dimension], [0, 1, 2])
    sub, indexes = grid.sel(y=slice(-1.0, None), x=slice(7.5, None), return_index=True)
    assert_index(indexes[grid.edge_dimension], [7, 8, 9])
    sub, values = grid.sel(x=slice(2.0, 4.0), data=np.arange(11.0))
    assert sub.n_edge == 2 and np.array_equal(values, [2.0, 3.0])
    sub, values = grid.sel(x=slice(2.0, 4.0), data=np.arange(12.0))
    assert np.array_equal(values, [2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match="does not support steps"):
        grid.sel(x=slice(0.0, 5.0, 2.0))
    assert grid.sel() is not None and grid.sel().n_edge == 10  # (unbounded on every side: all but the NaN edge)


# ---- remove_self_loops ------------------------------------------------------------------------------------------------------------------
def test_remove_self_loops(hip):
    xy, edges = nc.self_loops()
    grid = grid_of(xy, edges)
    e_xy, e_edges, e_nodes, e_index = nc.remove_self_loops_ref(xy, edges)
    assert_network(grid.remove_self_loops(), e_xy, e_edges)
    sub, indexes = grid.remove_self_loops(return_index=True)
    assert sub.n_node == 7  # (node 6, used only by a loop, is gone)
    assert_index(indexes[grid.node_dimension], e_nodes)
    assert_index(indexes[grid.edge_dimension], e_index)
    xy, edges = nc.chain(2050)
    plain = grid_of(xy, edges)
    again = plain.remove_self_loops()
    assert again is not plain and again == plain
    assert_network(grid_of(*nc.unused_nodes()).remove_self_loops(), *nc.subset_ref(*nc.unused_nodes(), np.arange(329))[:2])


# ---- merge -----------------------------------------------------------------------------------------------------------------------------
def check_merge(name):
    parts = nc.MERGE_CASES[name]()
    e = nc.merge_ref(parts)
    grids = [grid_of(xy, edges) for xy, edges in parts]
    assert_network(xa.merge_partitions(grids), e["xy"], e["edges"])
    merged, indexes = xa.Ugrid1d.merge_partitions(grids, return_index=True)
    assert_network(merged, e["xy"], e["edges"])
    for dim, key in ((merged.node_dimension, "node_index"), (merged.edge_dimension, "edge_index")):
        assert len(indexes[dim]) == len(parts)
        for got, want in zip(indexes[dim], e[key]):
            assert_index(got, want)
    return grids, e


@pytest.mark.parametrize("name", sorted(nc.MERGE_CASES))
def test_merge_partitions(hip, name):
    check_merge(name)


@pytest.mark.parametrize("name", ["overlapping", "parts2049", "zeros"])
def test_merge_with_the_smallest_table(hip, name):
    assert engine.get_option("merge_table_slack") == 0
    previous = engine.set_option("merge_table_slack", 1)
    try:
        check_merge(name)
    finally:
        engine.set_option("merge_table_slack", previous)
    assert engine.get_option("merge_table_slack") == 0


def test_merge_data_and_refusals(hip):
    grids, e = check_merge("overlapping")
    rng = np.random.default_rng(56)
    for facet, key in (("node", "node_index"), ("edge", "edge_index")):
        data = [rng.random((2, getattr(g, f"n_{facet}"))) for g in grids]
        want = np.concatenate([d[:, i] for d, i in zip(data, e[key])], axis=1)
        merged, values = xa.merge_partitions(grids, data=data, dim=getattr(grids[0], f"{facet}_dimension"))
        assert np.array_equal(values, want)
        merged, indexes, values = xa.merge_partitions(grids, return_index=True, data=[engine.DeviceArray.from_host(d) for d in data])
        assert isinstance(values, engine.DeviceArray) and np.array_equal(values.download(), want)
    assert xa.merge_partitions(grids[:1]) is grids[0]
    same, indexes = xa.merge_partitions(grids[:1], return_index=True)
    assert same is grids[0]
    assert_index(indexes[same.edge_dimension][0], np.arange(grids[0].n_edge))
    with pytest.raises(ValueError, match="zero partitions"):
        xa.merge_partitions([])
    mesh = xa.Ugrid2d(np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), -1, np.array([[0, 1, 2]]))
    with pytest.raises(TypeError, match="same type"):
        xa.merge_partitions([grids[0], mesh])


# ---- reindex_like ------------------------------------------------------------------------------------------------------------------------
def test_reindex_like(hip):
    xy, edges = nc.random_network(500, 0.1, seed=57)
    rng = np.random.default_rng(58)
    node_order, edge_order = rng.permutation(len(xy)), rng.permutation(len(edges))
    new_id = np.empty(len(xy), dtype=np.int64)
    new_id[node_order] = np.arange(len(xy))
    grid = grid_of(xy, edges)
    other = grid_of(xy[node_order], new_id[edges][edge_order][:, ::-1])
    node_data, edge_data = rng.random((3, len(xy))), rng.random(len(edges))
    assert np.array_equal(grid.reindex_like(other, node_data, dim=grid.node_dimension), node_data[:, node_order])
    assert np.array_equal(grid.reindex_like(other, edge_data), edge_data[edge_order])
    assert np.array_equal(xa.partition.reindex_like(grid, other, edge_data), edge_data[edge_order])
    jittered = grid_of(xy[node_order] + rng.uniform(-1e-9, 1e-9, xy.shape), new_id[edges][edge_order])
    for a, b in ((grid.node_coordinates[node_order], jittered.node_coordinates), (grid.edge_coordinates[edge_order], jittered.edge_coordinates)):
        assert not np.array_equal(a, b) and np.array_equal(np.rint(a / 1e-5), np.rint(b / 1e-5))  # (no key straddles a rounding boundary)
    assert np.array_equal(grid.reindex_like(jittered, edge_data, tolerance=1e-5), edge_data[edge_order])
    assert np.array_equal(grid.reindex_like(jittered, node_data, dim=grid.node_dimension, tolerance=1e-5), node_data[:, node_order])
    moved = xy[node_order].copy()
    moved[17] += 0.25
    with pytest.raises(ValueError, match="not identical"):
        grid.reindex_like(grid_of(moved, new_id[edges][edge_order]), node_data, dim=grid.node_dimension)
    with pytest.raises(ValueError, match="not identical"):
        grid.reindex_like(jittered, edge_data)


def test_split_merge_reindex_round_trip(hip):
    xy, edges = nc.chain(300, seed=59)
    grid = grid_of(xy, edges)
    rng = np.random.default_rng(60)
    labels = rng.integers(0, 4, grid.n_edge)
    node_data, edge_data = rng.random(grid.n_node), rng.random((2, grid.n_edge))
    parts = [grid.isel({grid.edge_dimension: np.flatnonzero(labels == l)}, return_index=True) for l in range(4)]
    grids = [p[0] for p in parts]
    for facet, data in (("node", node_data), ("edge", edge_data)):
        dim = getattr(grid, f"{facet}_dimension")
        pieces = [data[..., p[1][dim]] for p in parts]
        merged, values = xa.merge_partitions(grids, data=pieces, dim=dim)
        assert np.array_equal(merged.reindex_like(grid, values, dim=getattr(merged, f"{facet}_dimension")), data)


# ---- refine -------------------------------------------------------------------------------------------------------------------------------
def check_refine(name, **kw):
    xy, edges, vertices, tolerance, _ = nc.REFINE_CASES[name]()
    e = nc.refine_ref(xy, edges, vertices, tolerance)
    grid = grid_of(xy, edges)
    refined, node_index = grid.refine_by_vertices(vertices, return_index=True, tolerance=tolerance, **kw)
    assert_network(refined, e["xy"], e["edges"])
    assert_index(node_index, e["node_index"])
    return grid, refined, e


@pytest.mark.parametrize("name", sorted(nc.REFINE_CASES))
def test_refine_by_vertices(hip, name):
    grid, refined, e = check_refine(name)
    if name in ("known", "known_offset"):
        assert refined.edge_node_connectivity.tolist() == nc.KNOWN_EDGES and e["node_index"].tolist() == nc.KNOWN_NODE_INDEX
    if name == "none":
        assert refined == grid and refined is not grid
    if name == "twins":  # (an edge of length zero between the two equal vertices)
        assert (refined.edge_length == 0.0).sum() == 2
    if name == "two_edges":
        assert e["parent_edge"].tolist() == [0, 0, 0, 1]


def test_refine_default_tolerance_and_device_vertices(hip):
    xy, edges, vertices, _, _ = nc.REFINE_CASES["chain2049"]()
    e = nc.refine_ref(xy, edges, vertices, 0.0)
    grid = grid_of(xy, edges)
    assert_network(grid.refine_by_vertices(vertices), e["xy"], e["edges"])
    refined, node_index = grid.refine_by_vertices(engine.DeviceArray.from_host(vertices), return_index=True)
    assert_network(refined, e["xy"], e["edges"])
    assert isinstance(node_index, engine.DeviceArray) and np.array_equal(node_index.download(), e["node_index"])


def test_refine_names_the_vertices_on_no_edge(hip):
    xy, edges, vertices = nc.known()
    grid = grid_of(xy, edges)
    off = np.array([[7.5, 5.5], [100.0, -40.0], [np.nan, 1.0]])
    given = np.concatenate([vertices[:2], off[:1], vertices[2:], off[1:]])
    with pytest.raises(ValueError) as info:
        grid.refine_by_vertices(given, tolerance=0.01)
    assert str(info.value) == f"The following vertices are not located on any edge:\n{off}"
    assert_network(grid.refine_by_vertices(vertices), *[nc.refine_ref(xy, edges, vertices, 0.0)[k] for k in ("xy", "edges")])


def test_refine_data_follows_parent_edge(hip):
    xy, edges, vertices, tolerance, _ = nc.REFINE_CASES["diagonal"]()
    e = nc.refine_ref(xy, edges, vertices, tolerance)
    grid = grid_of(xy, edges)
    data = np.random.default_rng(61).random((2, len(edges)))
    refined, values = grid.refine_by_vertices(vertices, tolerance=tolerance, data=data)
    assert np.array_equal(values, data[:, e["parent_edge"]])
    refined, node_index, values = grid.refine_by_vertices(vertices, return_index=True, tolerance=tolerance,
                                                          data=engine.DeviceArray.from_host(data[0].astype(np.float32)))
    assert isinstance(values, engine.DeviceArray) and np.array_equal(values.download(), data[0].astype(np.float32).astype(np.float64)[e["parent_edge"]])
    with pytest.raises(ValueError, match="node data"):
        grid.refine_by_vertices(vertices, data=np.zeros(len(xy)))


def test_a_ring_takes_edge_data_and_dim(hip):
    """n_node == n_edge: the refinement takes the data as edge data, ``isel`` / ``sel`` are told the dimension."""
    xy = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])
    edges = np.array([[0, 1], [1, 2], [2, 3], [3, 0]], dtype=np.int64)
    grid = grid_of(xy, edges)
    data = np.array([10.0, 20.0, 30.0, 40.0])
    refined, values = grid.refine_by_vertices(np.array([[4.0, 1.0], [1.0, 0.0], [4.0, 3.0]]), tolerance=0.0, data=data)
    assert refined.n_edge == 7 and np.array_equal(values, [10.0, 10.0, 20.0, 20.0, 20.0, 30.0, 40.0])
    with pytest.raises(ValueError, match="exactly one"):
        grid.isel({grid.edge_dimension: [2, 0]}, data=data)
    sub, values = grid.isel({grid.edge_dimension: [2, 0]}, data=data, dim=grid.edge_dimension)
    assert np.array_equal(values, [30.0, 10.0])
    sub, values = grid.isel({grid.edge_dimension: [2, 0]}, data=data, dim=grid.node_dimension)
    assert np.array_equal(values, data)  # (the nodes 0, 1, 2, 3 of those two edges)
    sub, values = grid.sel(y=slice(None, 1.0), data=data, dim=grid.edge_dimension)
    assert sub.n_edge == 1 and np.array_equal(values, [10.0])


def test_refine_without_vertices_still_checks_the_edges(hip):
    """The C entry point with an edge that names a node out of range and no vertex: refused, as with vertices."""
    xy = engine.DeviceArray.from_host(np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]]))
    vertices = engine.DeviceArray.from_host(np.array([[0.5, 0.0]]))
    for bad in ([[0, 1], [1, 3]], [[-1, 1], [1, 2]]):
        edges = engine.DeviceArray.from_host(np.array(bad, dtype=np.int64))
        for n_vertex in (0, 1):
            with pytest.raises(ValueError, match="do not exist"):
                engine.DeviceNetEdit.refine(xy.ptr, 3, edges.ptr, 2, vertices.ptr, n_vertex, 0.0)
    edges = engine.DeviceArray.from_host(np.array([[0, 1], [1, 2]], dtype=np.int64))
    net, off = engine.DeviceNetEdit.refine(xy.ptr, 3, edges.ptr, 2, 0, 0, 0.0)
    assert off == 0 and np.array_equal(net.edges().download(), [[0, 1], [1, 2]]) and np.array_equal(net.parent_edge().download(), [0, 1])


def test_a_refined_grid_is_a_network(hip):
    """All lengths are integers: the distances along the refined chain at the old nodes equal the unrefined grid's bit for bit."""
    xy, edges, vertices, _, _ = nc.REFINE_CASES["chain2049"]()
    grid = grid_of(xy, edges)
    refined = grid.refine_by_vertices(vertices)
    sources = np.array([3, 1000, 2049])
    distance, source = grid.network_distance(sources, dim=grid.node_dimension)
    r_distance, r_source = refined.network_distance(sources, dim=refined.node_dimension)
    assert np.array_equal(bits(r_distance[:2050]), bits(distance)) and np.array_equal(r_source[:2050], source)
    grid.drop_device_caches()
    assert "_netedit_cache" not in grid.__dict__
    assert_network(grid.topology_subset([5, 4]), *nc.subset_ref(xy, edges, np.array([5, 4]))[:2])


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/netedit_worker_gpu.py): tensor indexers, tensor data and tensor vertices
def test_torch_in_torch_out():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "netedit_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_NETEDIT_OK" in res.stdout
