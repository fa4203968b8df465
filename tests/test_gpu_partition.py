"""
GPU: joining and matching grids on the device -- ``merge_partitions``, ``labels_to_indices``, ``partition_by_label``,
``Ugrid2d.reindex_like`` and ``connectivity.index_like_device`` -- on host-built grids and on grids whose mesh lives in HBM
only, against the numpy restatements of tests/partition_cases.py (pinned to the reference's own answers by
tests/test_partition_cpu.py).  Everything is integers or copied doubles: every comparison is ``np.array_equal``, coordinates
bit for bit.
"""
import numpy as np
import pytest

import graph_cases
import partition_cases as pc
import subset_cases as sc
import xugrid_amd as xa
from partition_cases import assert_index_lists, assert_merged, to_numpy
from xugrid_amd import engine, meshgen

pytestmark = pytest.mark.gpu
KINDS = ("host", "device")


def make_grid(kind, xy, faces):
    if kind == "host":
        return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert kind == "device"
    return graph_cases.device_grid(xy, faces)


def make_grids(kind, name):
    return [make_grid(kind, xy, faces) for xy, faces in pc.partitions(name)]


def check_merge(kind, name):
    e = pc.expected(name)
    grids = make_grids(kind, name)
    merged, indexes = xa.merge_partitions(grids, return_index=True)
    assert type(merged) is (xa.Ugrid2d if kind == "host" else xa.ugrid2d.DeviceUgrid2d)
    assert_merged(merged, e)
    assert_index_lists(merged, indexes, e, np.ndarray if kind == "host" else engine.DeviceArray)
    assert np.array_equal(merged.edge_node_connectivity, e["edges"])
    # without the indexes: the same grid; the static method is the module function
    assert_merged(xa.Ugrid2d.merge_partitions(grids), e)
    # the partitions are unchanged
    for grid, (xy, faces) in zip(grids, pc.partitions(name)):
        assert np.array_equal(grid.face_node_connectivity, faces) and pc.same_bits(grid.node_coordinates, xy)
    return grids, merged, e


# ---- merge against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pc.PARTITIONS))
def test_merge_partitions(hip, name, kind):
    grids, merged, e = check_merge(kind, name)
    # data on every facet: kept values concatenated (nodes, faces), scattered to their merged edge (edges)
    rng = np.random.default_rng(23)
    dims = {"node": merged.node_dimension, "edge": merged.edge_dimension, "face": merged.face_dimension}
    for facet, sizes in (("node", [len(xy) for xy, _ in pc.partitions(name)]), ("face", [len(f) for _, f in pc.partitions(name)]),
                         ("edge", np.diff(e["edge_slices"]))):
        data = [rng.random((2, int(n))) for n in sizes]
        where = data if kind == "host" else [engine.DeviceArray.from_host(d) for d in data]
        got_grid, values = xa.merge_partitions(grids, data=where, dim=dims[facet])
        assert_merged(got_grid, e)
        assert isinstance(values, np.ndarray if kind == "host" else engine.DeviceArray)
        values = to_numpy(values)
        assert values.dtype == np.float64 and np.array_equal(values, pc.merge_data(e, data, facet)), facet


def test_known_anchor_answer(hip):
    merged, indexes = xa.merge_partitions(make_grids("host", "anchor"), return_index=True)
    assert merged.n_node == 12
    assert [i.tolist() for i in indexes[merged.node_dimension]] == [list(range(10)), [8, 9]]
    assert [i.tolist() for i in indexes[merged.face_dimension]] == [[0, 1, 2, 3], [0, 1]]
    assert merged.face_node_connectivity[-2:].tolist() == [[6, 7, 11, 10], [5, 6, 10, 9]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", pc.SLACK_CASES)
def test_same_answers_with_the_smallest_table(hip, name, kind):
    assert engine.get_option("merge_table_slack") == 0
    previous = engine.set_option("merge_table_slack", 1)
    try:
        check_merge(kind, name)
    finally:
        engine.set_option("merge_table_slack", previous)
    assert engine.get_option("merge_table_slack") == 0


@pytest.mark.parametrize("kind", KINDS)
def test_one_grid_is_itself_and_mixed_lists_are_device(hip, kind):
    grids = make_grids(kind, "anchor")
    assert xa.merge_partitions(grids[:1]) is grids[0]
    same, indexes = xa.merge_partitions(grids[:1], return_index=True)
    assert same is grids[0]
    assert np.array_equal(to_numpy(indexes[same.face_dimension][0]), np.arange(grids[0].n_face))
    assert np.array_equal(to_numpy(indexes[same.edge_dimension][0]), np.arange(grids[0].n_edge))
    # one device-resident grid in the list makes the result device-resident
    mixed = [make_grids("host", "anchor")[0], make_grids("device", "anchor")[1]]
    merged, indexes = xa.merge_partitions(mixed, return_index=True)
    assert isinstance(merged, xa.ugrid2d.DeviceUgrid2d)
    assert_merged(merged, pc.expected("anchor"))
    assert_index_lists(merged, indexes, pc.expected("anchor"), engine.DeviceArray)


def test_nonmanifold_takes_the_host_route(hip):
    xy, faces = sc.three_faces_on_one_edge()
    parts = [pc.cut(xy, faces, [0, 1, 2]), pc.cut(xy, faces, [2, 3])]
    grids = [graph_cases.device_grid(*p) for p in parts]
    assert not grids[0].device_topology().manifold
    e = pc.merge(parts)
    merged, indexes = xa.merge_partitions(grids, return_index=True)
    assert isinstance(merged, xa.ugrid2d.DeviceUgrid2d)
    assert_merged(merged, e)
    assert_index_lists(merged, indexes, e, engine.DeviceArray)


# ---- labels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["numpy", "device"])
def test_labels_to_indices(hip, where):
    rng = np.random.default_rng(29)
    for labels in (np.array([0, 1, 0, 2, 2]), np.array([2, 0, 2]), np.zeros(0, dtype=np.int64), np.zeros(2049, dtype=np.int64),
                   rng.integers(0, 7, size=2049), rng.integers(0, 3, size=300).astype(np.int32)):
        given = labels if where == "numpy" else engine.DeviceArray.from_host(labels.astype(np.int64))
        got = xa.labels_to_indices(given)
        want = pc.labels_to_indices(labels)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert isinstance(g, np.ndarray if where == "numpy" else engine.DeviceArray)
            g = to_numpy(g)
            assert g.dtype == np.int64 and np.array_equal(g, w)
    assert [i.tolist() for i in xa.labels_to_indices([0, 1, 0, 2, 2])] == [[0, 2], [1], [3, 4]]
    with pytest.raises(TypeError, match="labels must have integer dtype"):
        xa.labels_to_indices(np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="non-negative"):
        xa.labels_to_indices(np.array([0, -1]))


# ---- the round trip: partition_by_label -> merge_partitions -> reindex_like ------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_partition_roundtrip(hip, kind):
    xy, faces = meshgen.quad_mesh(np.arange(6.0), np.arange(4.0))  # 5 x 3 quads
    grid = make_grid(kind, xy, faces)
    labels = np.repeat([0, 1, 2], 5)
    want = pc.labels_to_indices(labels)
    parts = [pc.cut(xy, faces, ids) for ids in want]
    e = pc.merge(parts)
    dims = {"node": grid.node_dimension, "edge": grid.edge_dimension, "face": grid.face_dimension}
    merged = None
    for facet in ("node", "edge", "face"):
        data = np.arange(getattr(grid, f"n_{facet}"), dtype=np.float64)
        pieces = grid.partition_by_label(labels, data=data)
        assert len(pieces) == 3
        for (sub, indexes, values), ids, (p_xy, p_faces) in zip(pieces, want, parts):
            assert type(sub) is type(grid)
            sc.assert_grid(sub, p_xy, p_faces)
            assert np.array_equal(to_numpy(indexes[grid.face_dimension]), ids)
            assert np.array_equal(values, data[to_numpy(indexes[dims[facet]])])
        merged, values = xa.merge_partitions([p[0] for p in pieces], data=[p[2] for p in pieces], dim=dims[facet])
        assert type(merged) is type(grid)
        assert_merged(merged, e)
        assert np.array_equal(merged.edge_node_connectivity, e["edges"])
        back = merged.reindex_like(grid, values, dim=dims[facet])
        assert isinstance(back, np.ndarray) and back.dtype == np.float64 and np.array_equal(back, data), facet
        assert np.array_equal(merged.reindex_like(grid, values), data)  # the facet found by the data's size
    without = grid.partition_by_label(labels)
    assert len(without) == 3 and all(len(p) == 2 for p in without)


@pytest.mark.parametrize("kind", KINDS)
def test_merge_partitions_no_duplicates(hip, kind):
    xy, faces = pc.quads(3, 2)
    grid = make_grid(kind, xy, faces)
    face_z = np.arange(6.0) * 10.0
    (a, _, za), (b, _, zb) = (grid.isel({grid.face_dimension: np.array(ids)}, return_index=True, data=face_z)
                              for ids in ([0, 1, 2, 3], [2, 3, 4, 5]))
    merged, z = xa.merge_partitions([a, b], data=[za, zb])
    assert merged.n_face == 6 and np.array_equal(np.sort(z), face_z)  # every face_z once
    assert np.array_equal(merged.reindex_like(grid, z), face_z)


# ---- reindex_like / index_like ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["numpy", "device"])
@pytest.mark.parametrize("name", sorted(pc.like_cases()))
def test_index_like(hip, name, where):
    a, b, tolerance = pc.like_cases()[name]
    want = pc.index_like(a, b, tolerance)
    given = (a, b) if where == "numpy" else (engine.DeviceArray.from_host(a), engine.DeviceArray.from_host(b))
    got = xa.connectivity.index_like_device(*given, tolerance=tolerance)
    assert isinstance(got, np.ndarray if where == "numpy" else engine.DeviceArray)
    got = to_numpy(got)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if name.startswith("known"):
        assert got.tolist() == [3, 1, 0, 2]
    for slack in (1,):
        previous = engine.set_option("merge_table_slack", slack)
        try:
            assert np.array_equal(to_numpy(xa.connectivity.index_like_device(*given, tolerance=tolerance)), want)
        finally:
            engine.set_option("merge_table_slack", previous)


@pytest.mark.parametrize("kind", KINDS)
def test_reindex_like_faces_reversed(hip, kind):
    xy, faces = sc.mesh("mixed36")
    grid = make_grid(kind, xy, faces)
    other = make_grid(kind, xy, faces[::-1].copy())
    data = np.arange(grid.n_face, dtype=np.float64)
    assert np.array_equal(grid.reindex_like(other, data), data[::-1])
    stacked = np.stack([data, -data]).astype(np.float32)
    got = grid.reindex_like(other, engine.DeviceArray.from_host(stacked))
    assert isinstance(got, engine.DeviceArray) and np.array_equal(got.download(), stacked[:, ::-1].astype(np.float64))
    # nodes and edges are in the same order in both grids
    nodes = np.arange(grid.n_node, dtype=np.float64)
    assert np.array_equal(grid.reindex_like(other, nodes, dim=grid.node_dimension), nodes)
    edges = np.arange(grid.n_edge, dtype=np.float64)
    assert np.array_equal(grid.reindex_like(other, edges, dim=grid.edge_dimension), edges)


@pytest.mark.parametrize("kind", KINDS)
def test_reindex_like_tolerance(hip, kind):
    a, b, tolerance = pc.like_cases()["jitter"]
    _, faces = sc.mesh("mixed36")
    order = pc.index_like(a, b, tolerance)  # b[i] ~ a[order[i]]
    grid = make_grid(kind, a, faces)
    other = make_grid(kind, b, np.where(faces == -1, -1, np.argsort(order)[faces]))
    data = np.arange(grid.n_node, dtype=np.float64)
    assert np.array_equal(grid.reindex_like(other, data, dim=grid.node_dimension, tolerance=tolerance), data[order])
    with pytest.raises(ValueError, match="not identical after sorting"):
        grid.reindex_like(other, data, dim=grid.node_dimension)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(hip, kind):
    grids = make_grids(kind, "anchor")
    xy, faces = pc.quads(3, 2)
    grid = make_grid(kind, xy, faces)
    a = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    with pytest.raises(ValueError, match="coordinates do not match in shape"):
        xa.connectivity.index_like_device(a, a[:2])
    moved = a.copy()
    moved[1, 0] = 1.1
    with pytest.raises(ValueError, match="coordinates are not identical after sorting"):
        xa.connectivity.index_like_device(a, moved)
    with pytest.raises(ValueError, match="coordinates are not identical after sorting"):
        xa.connectivity.index_like_device(a, moved, tolerance=0.2)  # rint(1.1 / 0.2) = 6, rint(1.0 / 0.2) = 5: DESIGN section 7
    moved[1, 0] = 1.05  # the same key, 0.05 apart
    assert np.array_equal(xa.connectivity.index_like_device(a, moved, tolerance=0.2), [0, 1, 2])
    with pytest.raises(ValueError, match="coordinates are not identical after sorting"):
        xa.connectivity.index_like_device(a, moved, tolerance=0.0)
    for repeated in ((a[[0, 0, 2]], a[[0, 0, 2]]), (a, a[[0, 0, 2]]), (a[[0, 0, 2]], a)):
        with pytest.raises(ValueError, match="coordinates are not identical after sorting"):
            xa.connectivity.index_like_device(*repeated)
    with pytest.raises(ValueError, match="Cannot merge partitions: zero partitions provided."):
        xa.merge_partitions([])
    with pytest.raises(TypeError, match="labels must have integer dtype"):
        grid.partition_by_label(np.zeros(grid.n_face))
    with pytest.raises(ValueError):
        grid.partition_by_label(np.zeros(grid.n_face + 1, dtype=np.int64))
    with pytest.raises(ValueError, match="one array per partition"):
        xa.merge_partitions(grids, data=[np.zeros(grids[0].n_face)])
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):
        xa.merge_partitions(grids, data=[np.zeros(grids[0].n_face), np.zeros(grids[1].n_node)])
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):
        xa.merge_partitions(grids, data=[np.zeros(g.n_face + 1000) for g in grids])
    with pytest.raises(ValueError, match="exactly one UGRID dimension"):
        xa.merge_partitions(grids, data=[np.zeros(g.n_face) for g in grids], dim=grids[0].node_dimension)
    with pytest.raises(ValueError, match="not a UGRID dimension"):
        xa.merge_partitions(grids, data=[np.zeros(g.n_face) for g in grids], dim="nowhere")
    other = make_grid(kind, xy + 0.25, faces)
    with pytest.raises(ValueError, match="coordinates are not identical after sorting"):
        grid.reindex_like(other, np.zeros(grid.n_face))
    # everything is usable afterwards
    assert_merged(xa.merge_partitions(grids), pc.expected("anchor"))
    assert np.array_equal(grid.reindex_like(grid, np.arange(6.0)), np.arange(6.0))
    assert len(grid.partition_by_label(np.zeros(grid.n_face, dtype=np.int64))) == 1


# ---- the merged grid is a first-class mesh -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_merged_grid_regrids_like_the_whole_grid(hip, kind):
    """Per target cell, bit for bit.  A weighted mean adds its terms in the order of the source faces, so it is compared where
    the merged grid keeps the whole grid's face order (label blocks in order: another node table, the same faces); with halo
    partitions in permuted order the faces are renumbered, and the reducers that do not depend on the order are compared."""
    xy, faces = sc.mesh("mixed36")
    xmin, ymin, xmax, ymax = xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()
    whole = make_grid(kind, xy, faces)
    n = whole.n_face
    raster = xa.Ugrid2d.from_structured_bounds(*(np.column_stack([e[:-1], e[1:]]) for e in (np.linspace(xmin, xmax, 5), np.linspace(ymin, ymax, 4))))
    data = np.random.default_rng(5).random(n)

    def regrid(grid, values, method):
        out = xa.OverlapRegridder(grid, raster, method=method).regrid(values)
        assert not np.isnan(out).all()
        return out

    # label blocks in order: the merged faces are the whole grid's faces in the same order
    labels = np.minimum(np.arange(n) * 3 // n, 2)
    pieces = whole.partition_by_label(labels, data=data)
    merged, merged_data = xa.merge_partitions([p[0] for p in pieces], data=[p[2] for p in pieces])
    assert type(merged) is type(whole) and np.array_equal(merged_data, data)
    assert np.array_equal(merged.reindex_like(whole, merged_data), data)
    for method in ("mean", "sum", "maximum"):
        assert np.array_equal(regrid(merged, merged_data, method), regrid(whole, data, method), equal_nan=True), method
    # halo blocks in permuted order: the faces are renumbered
    blocks = pc.halo_blocks(xy, faces, 3)
    pieces = [whole.isel({whole.face_dimension: ids}, data=data) for ids in (blocks[2], blocks[0], blocks[1])]
    merged, merged_data = xa.merge_partitions([p[0] for p in pieces], data=[p[1] for p in pieces])
    assert merged.n_face == n and merged.n_node == whole.n_node and not np.array_equal(merged_data, data)
    assert np.array_equal(merged.reindex_like(whole, merged_data), data)
    for method in ("maximum", "minimum"):
        assert np.array_equal(regrid(merged, merged_data, method), regrid(whole, data, method), equal_nan=True), method


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/partition_worker_gpu.py): tensor labels, tensor data and tensor indexes, on both kinds of grid
def test_torch_in_torch_out():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "partition_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_PARTITION_OK" in res.stdout
