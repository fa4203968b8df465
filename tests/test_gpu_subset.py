"""
GPU: sub-meshes cut on the device -- ``Ugrid2d.topology_subset`` / ``clip_box`` / ``isel`` and ``sel(return_grid=True)`` -- on
host-built grids and on grids whose mesh lives in HBM only, against the numpy restatements of tests/subset_cases.py (pinned to
the reference's known answers by tests/test_subset_cpu.py).  Everything is integers or copied doubles: every comparison is
``np.array_equal``.
"""
import numpy as np
import pytest

import graph_cases
import subset_cases as sc
import xugrid_amd as xa
from subset_cases import assert_grid, assert_indexes, to_numpy
from xugrid_amd import engine, meshgen

pytestmark = pytest.mark.gpu
KINDS = ("host", "device")


def make_grid(kind, xy, faces):
    if kind == "host":
        return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert kind == "device"
    return graph_cases.device_grid(xy, faces)


_expected = {}


def expected(name, selection):
    """(xy_sub, faces_sub, node_index, edge_index, face ids) of the yardstick, computed once per case."""
    key = (name, selection)
    if key not in _expected:
        xy, faces = sc.mesh(name)
        xy_sub, faces_sub, node_index, ids = sc.topology_subset(xy, faces, sc.selections(name)[selection])
        _expected[key] = xy_sub, faces_sub, node_index, sc.edge_index(faces, ids), ids
    return _expected[key]


# ---- topology_subset against the yardstick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,selection", sc.CASES)
def test_topology_subset(hip, name, selection, kind):
    xy, faces = sc.mesh(name)
    index = sc.selections(name)[selection]
    xy_sub, faces_sub, node_index, edge_index, ids = expected(name, selection)
    grid = make_grid(kind, xy, faces)
    sub, indexes = grid.topology_subset(index, return_index=True)
    index_kind = np.ndarray if kind == "host" else engine.DeviceArray
    if np.array_equal(ids, np.arange(len(faces))):  # every face in order: the grid itself
        assert sub is grid and grid.topology_subset(index) is grid
        assert_indexes(grid, indexes, np.arange(len(xy)), np.arange(grid.n_edge), np.arange(len(faces)), index_kind)
        return
    assert type(sub) is type(grid) and sub is not grid
    assert_grid(sub, xy_sub, faces_sub)
    assert_indexes(grid, indexes, node_index, edge_index, ids, index_kind)
    if len(ids):
        # the sub-grid derives its own edges, and they are the old ones: edge k of the sub-grid is old edge edge_index[k]
        edge_node, _ = sc.host_edges(faces)
        assert np.array_equal(sub.edge_node_connectivity, sc.renumber(edge_node[edge_index], node_index))
        assert np.array_equal(sub.face_edge_connectivity, sc.host_edges(faces_sub)[1])
        assert np.array_equal(sub.area, grid.area[ids])
    # the source is unchanged, and a second call gives the same
    assert np.array_equal(grid.face_node_connectivity, faces) and np.array_equal(grid.node_coordinates, xy)
    again = grid.topology_subset(index)
    assert type(again) is type(grid)
    assert_grid(again, xy_sub, faces_sub)


@pytest.mark.parametrize("kind", KINDS)
def test_known_answers(hip, kind):
    xy, faces = sc.mesh("grid2d")
    grid = make_grid(kind, xy, faces)
    k = sc.known()
    for case in k["topology_subset"]:
        sub, indexes = grid.topology_subset(np.array(case["face_index"]), return_index=True)
        assert np.array_equal(sub.face_node_connectivity, case["faces"])
        assert np.array_equal(sub.node_x, case["x"]) and np.array_equal(sub.node_y, case["y"])
        assert np.array_equal(to_numpy(indexes[grid.node_dimension]), case["node_index"])
        assert np.array_equal(to_numpy(indexes[grid.edge_dimension]), case["edge_index"])
    assert np.array_equal(grid.topology_subset(np.array(k["reversed"]["face_index"])).face_node_connectivity, faces[::-1])
    assert grid.topology_subset(np.array(k["identity"]["face_index"])) is grid
    assert grid.topology_subset(np.array(k["identity"]["mask"])) is grid
    clipped = grid.clip_box(*k["clip_box"]["box"])
    assert clipped.n_face == 2
    assert np.array_equal(clipped.face_node_connectivity, grid.topology_subset(np.array(k["clip_box"]["faces"])).face_node_connectivity)
    assert grid.clip_box(*grid.bounds) is grid
    isel = k["isel"]
    assert grid.isel({grid.node_dimension: np.array(isel["node_identity"])}) is grid
    assert grid.isel({grid.edge_dimension: np.array(isel["edge_identity"])}) is grid
    with pytest.raises(ValueError, match="results in an invalid topology"):
        grid.isel({grid.node_dimension: np.array(isel["node_invalid"])})
    with pytest.raises(ValueError, match="results in an invalid topology"):
        grid.isel({grid.edge_dimension: np.array(isel["edge_invalid"])})
    with pytest.raises(ValueError, match="UGRID dimensions do not align"):
        grid.isel({grid.face_dimension: np.array(isel["misaligned"]["face"]), grid.node_dimension: np.array(isel["misaligned"]["node"])})


def test_rectilinear(hip):
    grid = xa.ugrid2d.RectilinearUgrid2d(np.array([0.0, 1.0, 3.0, 4.0, 6.0]), np.array([0.0, 2.0, 3.0, 5.0]))
    index = np.array([7, 2, 11, 0])
    sub, indexes = grid.topology_subset(index, return_index=True)
    assert isinstance(sub, xa.ugrid2d.DeviceUgrid2d)
    xy_sub, faces_sub, node_index, ids = sc.topology_subset(grid.node_coordinates, grid.face_node_connectivity, index)
    assert_grid(sub, xy_sub, faces_sub)
    assert_indexes(grid, indexes, node_index, sc.edge_index(grid.face_node_connectivity, ids), ids, engine.DeviceArray)
    assert grid.clip_box(*grid.bounds) is grid


# ---- clip_box ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["grid2d", "mixed36", "disconnected", "mixed2049"])
def test_clip_box(hip, name, kind):
    xy, faces = sc.mesh(name)
    grid = make_grid(kind, xy, faces)
    c = grid.centroids
    xmin, ymin, xmax, ymax = grid.bounds
    cx, cy = c[len(c) // 3]
    boxes = [
        (0.5 * (xmin + cx), ymin, xmax, 0.5 * (cy + ymax)),
        (cx, ymin, xmax, ymax),  # an edge exactly on a centroid coordinate: the lower bound holds it ...
        (xmin, ymin, cx, ymax),  # ... the upper bound does not
        (xmin, cy, xmax, ymax),
        (xmin, ymin, xmax, cy),
        (xmax + 1.0, ymin, xmax + 2.0, ymax),  # empty
    ]
    n_selected = []
    for box in boxes:
        index = grid.locate_bounding_box(*box)
        assert np.array_equal(index, sc.box_faces(c, *box))
        n_selected.append(len(index))
        clipped, through_index = grid.clip_box(*box), grid.topology_subset(index)
        assert type(clipped) is type(grid) and clipped.n_face == len(index)
        assert np.array_equal(clipped.face_node_connectivity, through_index.face_node_connectivity)
        assert np.array_equal(clipped.node_coordinates, through_index.node_coordinates)
    assert len(c) // 3 in grid.locate_bounding_box(*boxes[1]) and len(c) // 3 not in grid.locate_bounding_box(*boxes[2])
    assert n_selected[1] + n_selected[2] == len(c) and n_selected[3] + n_selected[4] == len(c) and n_selected[5] == 0
    assert grid.clip_box(xmax + 1.0, ymin, xmax + 2.0, ymax).n_node == 0
    assert grid.clip_box(*grid.bounds) is grid


# ---- isel -------------------------------------------------------------------------------------------------------------------
def _as_data(a, where):
    return a if where == "numpy" else engine.DeviceArray.from_host(a)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["numpy", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_isel(hip, dtype, where, kind):
    xy, faces = sc.mesh("disconnected")
    grid = make_grid(kind, xy, faces)
    n_first = len(meshgen.triangle_mesh(30, 1)[1])
    face_ids = np.arange(n_first, len(faces) - 1)  # the second patch
    xy_sub, faces_sub, node_index, edge_index, ids = sc.isel(xy, faces, face=face_ids)
    by = {"face": ids, "node": node_index, "edge": edge_index}
    dims = {"face": grid.face_dimension, "node": grid.node_dimension, "edge": grid.edge_dimension}
    rng = np.random.default_rng(3)
    data = {f: rng.random((2, getattr(grid, f"n_{f}"))).astype(dtype) for f in by}
    for selector in (("face",), ("node",), ("edge",), ("node", "face"), ("edge", "face"), ("node", "edge", "face")):
        indexers = {dims[f]: by[f] for f in selector}
        for facet in by:
            sub, indexes, values = grid.isel(indexers, return_index=True, data=_as_data(data[facet], where))
            assert type(sub) is type(grid)
            assert_grid(sub, xy_sub, faces_sub)
            assert_indexes(grid, indexes, node_index, edge_index, ids)
            assert isinstance(values, np.ndarray if where == "numpy" else engine.DeviceArray)
            values = to_numpy(values)
            assert values.dtype == np.float64 and np.array_equal(values, data[facet][:, by[facet]].astype(np.float64))
        sub_only = grid.isel(**indexers)
        assert_grid(sub_only, xy_sub, faces_sub)
        sub2, values = grid.isel(indexers, data=_as_data(data["node"], where))
        assert np.array_equal(to_numpy(values), data["node"][:, node_index].astype(np.float64))
    # a mask selects like its nonzero
    mask = np.zeros(len(xy), dtype=bool)
    mask[node_index] = True
    assert_grid(grid.isel({grid.node_dimension: mask}), xy_sub, faces_sub)
    # dimensions that stand for different faces; a node selection that leaves a face incomplete
    last = len(faces) - 1
    with pytest.raises(ValueError, match="UGRID dimensions do not align"):
        grid.isel({grid.face_dimension: face_ids, grid.node_dimension: faces[last]})
    with pytest.raises(ValueError, match="results in an invalid topology"):
        grid.isel({grid.node_dimension: node_index[:-1]})
    with pytest.raises(ValueError, match="results in an invalid topology"):
        grid.isel({grid.edge_dimension: edge_index[1:]})
    with pytest.raises(ValueError, match="exactly one"):
        grid.isel({grid.face_dimension: face_ids}, data=np.zeros(len(faces) + len(xy) + 1000))
    assert grid.isel({grid.face_dimension: np.array([last])}).n_face == 1  # the grid is usable afterwards


@pytest.mark.parametrize("kind", KINDS)
def test_sel_return_grid(hip, kind):
    xy, faces = sc.mesh("mixed36")
    grid = make_grid(kind, xy, faces)
    data = np.arange(grid.n_face, dtype=np.float64)
    xmin, ymin, xmax, ymax = grid.bounds
    x, y = slice(0.5 * (xmin + xmax), None), slice(None, 0.5 * (ymin + ymax))
    values, face_index = grid.sel(data, x=x, y=y)
    with_grid = grid.sel(data, x=x, y=y, return_grid=True)
    assert len(with_grid) == 3 and 0 < len(face_index) < grid.n_face
    assert np.array_equal(with_grid.values, values) and np.array_equal(with_grid.face_index, face_index)
    clipped = grid.clip_box(x.start, ymin, xmax, y.stop)
    assert type(with_grid.grid) is type(grid)
    assert np.array_equal(with_grid.grid.face_node_connectivity, clipped.face_node_connectivity)
    assert np.array_equal(with_grid.grid.node_coordinates, clipped.node_coordinates)
    assert "_topology_cache" not in grid.__dict__  # the face index alone: no edge topology was built for it
    with pytest.raises(ValueError, match="return_grid"):
        grid.sel(data, x=np.array([0.5 * (xmin + xmax)]), y=np.array([0.5 * (ymin + ymax)]), return_grid=True)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _as_index(a, where):
    a = np.asarray(a, dtype=np.int64)
    if where == "numpy":
        return a
    return engine.DeviceArray.from_host(a)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["numpy", "device"])
def test_refusals(hip, where, kind):
    xy, faces = sc.mesh("mixed36")
    grid = make_grid(kind, xy, faces)
    n = grid.n_face
    for bad, error, match in (([3, 5, 3], ValueError, "index contains repeated values; only subsets will result in valid UGRID"),
                              ([0, n], IndexError, "outside"), ([2, -1], IndexError, "outside")):
        with pytest.raises(error, match=match):
            grid.topology_subset(_as_index(bad, where))
        with pytest.raises(error, match=match):
            grid.isel({grid.face_dimension: _as_index(bad, where)})
        with pytest.raises(error, match=match):
            grid.isel({grid.node_dimension: _as_index(bad, where)})
        # the grid is usable afterwards
        xy_sub, faces_sub, _, _ = sc.topology_subset(xy, faces, np.array([5, 3]))
        assert_grid(grid.topology_subset(_as_index([5, 3], where)), xy_sub, faces_sub)
    with pytest.raises(ValueError, match="larger than dimension size"):
        grid.topology_subset(_as_index(np.arange(n + 1), where))
    if where != "numpy":
        with pytest.raises(TypeError):
            grid.topology_subset(engine.DeviceArray.from_host(np.array([0.5])))


# ---- kinds of the indexes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_index_kinds(hip, kind):
    xy, faces = sc.mesh("mixed36")
    grid = make_grid(kind, xy, faces)
    index = sc.selections("mixed36")["permuted_subset"]
    xy_sub, faces_sub, node_index, edge_index, ids = expected("mixed36", "permuted_subset")
    sub, indexes = grid.topology_subset(_as_index(index, "device"), return_index=True)
    assert type(sub) is type(grid)
    assert_grid(sub, xy_sub, faces_sub)
    assert_indexes(grid, indexes, node_index, edge_index, ids, engine.DeviceArray)
    sub, indexes = grid.isel({grid.face_dimension: _as_index(index, "device")}, return_index=True)
    assert_indexes(grid, indexes, node_index, edge_index, ids, engine.DeviceArray)
    # a one-byte device array is a mask
    mask = sc.selections("mixed36")["mask"]
    m_xy, m_faces, m_nodes, m_edges, m_ids = expected("mixed36", "mask")
    for device_mask in (engine.DeviceArray.from_host(mask), engine.DeviceArray.from_host(mask.view(np.uint8))):
        sub, indexes = grid.topology_subset(device_mask, return_index=True)
        assert_grid(sub, m_xy, m_faces)
        assert_indexes(grid, indexes, m_nodes, m_edges, m_ids, engine.DeviceArray)
    assert grid.topology_subset(engine.DeviceArray.from_host(np.ones(grid.n_face, dtype=bool))) is grid
    with pytest.raises(ValueError, match="bool index"):
        grid.topology_subset(engine.DeviceArray.from_host(np.ones(grid.n_face - 1, dtype=bool)))


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/subset_worker_gpu.py): torch indexes, bool tensors as masks and torch data through isel, on both kinds of grid
def test_torch_in_torch_out():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "subset_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_SUBSET_OK" in res.stdout


# ---- the new handle is a first-class mesh -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_subgrid_regrids_like_the_full_grid(hip, kind):
    xy, faces = meshgen.quad_mesh(np.linspace(0.0, 8.0, 9), np.linspace(0.0, 8.0, 9))
    grid = make_grid(kind, xy, faces)
    edges = np.linspace(0.0, 8.0, 6)  # cells of width 1.6: they cut the quads
    bounds = np.column_stack([edges[:-1], edges[1:]])
    raster = xa.Ugrid2d.from_structured_bounds(bounds, bounds)
    selected = np.nonzero(grid.centroids[:, 0] < 4.0)[0]
    sub = grid.clip_box(0.0, 0.0, 4.0, 8.0)
    assert sub.n_face == len(selected) == 32 and type(sub) is type(grid)
    data = np.random.default_rng(5).random(grid.n_face)
    full = xa.OverlapRegridder(grid, raster, method="mean").regrid(data)
    part = xa.OverlapRegridder(sub, raster, method="mean").regrid(data[selected])
    covered = raster.centroids[:, 0] < 3.2  # target cells that end at x = 3.2: only selected faces (x < 4) cover them
    assert covered.sum() == 10 and np.array_equal(part[covered], full[covered])
    assert np.all(np.isnan(part[raster.centroids[:, 0] > 4.8]))  # nothing of the sub-grid lies there


def test_nonmanifold_takes_the_host_route(hip):
    xy, faces = sc.three_faces_on_one_edge()
    grid = graph_cases.device_grid(xy, faces)
    assert not grid.device_topology().manifold
    index = np.array([3, 0])
    sub, indexes = grid.topology_subset(index, return_index=True)
    xy_sub, faces_sub, node_index, ids = sc.topology_subset(xy, faces, index)
    edge_index = sc.edge_index(faces, ids)
    assert isinstance(sub, xa.ugrid2d.DeviceUgrid2d)
    assert_grid(sub, xy_sub, faces_sub)
    assert_indexes(grid, indexes, node_index, edge_index, ids, engine.DeviceArray)
    assert np.array_equal(sub.edge_node_connectivity, sc.renumber(sc.host_edges(faces)[0][edge_index], node_index))
    got = grid.isel({grid.edge_dimension: sc.edge_index(faces, np.array([3]))}, return_index=True)
    assert got[0].n_face == 1 and np.array_equal(to_numpy(got[1][grid.face_dimension]), [3])
