"""
GPU: ``Ugrid2d.to_periodic`` and ``Ugrid2d.to_nonperiodic`` on host-built grids and on grids whose mesh lives in HBM only,
against the numpy restatements of tests/periodic_cases.py (pinned to the reference's own answers by
tests/test_periodic_cpu.py).  Everything is integers or copied doubles: every comparison is ``np.array_equal``, coordinates
bit for bit.
"""
import numpy as np
import pytest

import graph_cases
import periodic_cases as pc
import subset_cases as sc
import xugrid_amd as xa
from periodic_cases import assert_grid, assert_indexes, to_numpy
from xugrid_amd import engine, meshgen

pytestmark = pytest.mark.gpu
KINDS = ("host", "device")


def make_grid(kind, xy, faces):
    if kind == "host":
        return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert kind == "device"
    return graph_cases.device_grid(xy, faces)


def kinds_of(kind):
    return (xa.Ugrid2d, np.ndarray) if kind == "host" else (xa.ugrid2d.DeviceUgrid2d, engine.DeviceArray)


def check_both_directions(kind, name):
    """-> (grid, periodic grid, non-periodic grid of that), each checked against the restatement."""
    xy, faces, xmax = pc.mesh(name)
    wrapped_e, unwrapped_e = pc.expected(name)
    grid_type, index_type = kinds_of(kind)
    grid = make_grid(kind, xy, faces)
    wrapped, indexes = grid.to_periodic(return_index=True)
    assert type(wrapped) is grid_type
    assert_grid(wrapped, wrapped_e)
    assert_indexes(grid, indexes, wrapped_e, index_type)
    assert_grid(grid.to_periodic(), wrapped_e)  # without the indexes: the same grid
    unwrapped, indexes = wrapped.to_nonperiodic(xmax, return_index=True)
    assert type(unwrapped) is grid_type
    assert_grid(unwrapped, unwrapped_e)
    assert_indexes(wrapped, indexes, unwrapped_e, index_type)
    assert_grid(wrapped.to_nonperiodic(xmax), unwrapped_e)
    # the inputs are unchanged
    assert np.array_equal(grid.face_node_connectivity, faces) and pc.same_bits(grid.node_coordinates, xy)
    assert_grid(wrapped, wrapped_e)
    return grid, wrapped, unwrapped


# ---- both directions against the yardstick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pc.MESHES))
def test_both_directions(hip, name, kind):
    check_both_directions(kind, name)


@pytest.mark.parametrize("name", list(pc.RANGE_MESHES))
def test_x_range_at_the_edges_of_its_reduction(hip, name):
    """One block, one block and a lane, 256 and 257 partials, a first stage that strides: both directions, every array."""
    xy, _, _ = pc.mesh(name)
    assert len(xy) == int(name[len("nodes"):])
    check_both_directions("host", name)


def test_anchor_answers(hip):
    xy, faces, xmax = pc.mesh("quads32")
    wrapped, indexes = make_grid("host", xy, faces).to_periodic(return_index=True)
    assert indexes[wrapped.node_dimension].tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 10]
    assert wrapped.face_node_connectivity.tolist() == [[0, 1, 4, 3], [1, 2, 5, 4], [2, 0, 3, 5], [3, 4, 7, 6], [4, 5, 8, 7], [5, 3, 6, 8]]
    assert wrapped.n_node == 9 and set(wrapped.node_x.tolist()) == {0.0, 1.0, 2.0}
    unwrapped, indexes = wrapped.to_nonperiodic(3.0, return_index=True)
    assert unwrapped.n_node == 12 and unwrapped.node_coordinates[9:].tolist() == [[3.0, 0.0], [3.0, 1.0], [3.0, 2.0]]
    assert indexes[wrapped.node_dimension].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 3, 6]
    assert unwrapped.face_node_connectivity.tolist() == [[0, 1, 4, 3], [1, 2, 5, 4], [2, 9, 10, 5], [3, 4, 7, 6], [4, 5, 8, 7],
                                                         [5, 10, 11, 8]]
    # the reproduced quirk: a right node that comes first keeps x = xmax
    xy, faces, _ = pc.mesh("quads32_reversed")
    assert set(make_grid("host", xy, faces).to_periodic().node_x.tolist()) == {1.0, 2.0, 3.0}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pc.MESHES))
def test_same_answers_with_the_smallest_table(hip, name, kind):
    assert engine.get_option("merge_table_slack") == 0
    previous = engine.set_option("merge_table_slack", 1)
    try:
        check_both_directions(kind, name)
    finally:
        engine.set_option("merge_table_slack", previous)
    assert engine.get_option("merge_table_slack") == 0


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_identical_indexes(hip, kind):
    xy, faces, xmax = pc.mesh("big")
    grid = make_grid(kind, xy, faces)
    runs = [grid.to_periodic(return_index=True) for _ in range(2)]
    for dim in runs[0][1]:
        assert np.array_equal(to_numpy(runs[0][1][dim]), to_numpy(runs[1][1][dim])), dim
    again = [runs[0][0].to_nonperiodic(xmax, return_index=True)[1] for _ in range(2)]
    for dim in again[0]:
        assert np.array_equal(to_numpy(again[0][dim]), to_numpy(again[1][dim])), dim


# ---- data on every facet -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["quads32", "shuffled", "mixed", "big"])
def test_data_on_every_facet(hip, name, kind):
    xy, faces, xmax = pc.mesh(name)
    wrapped_e, unwrapped_e = pc.expected(name)
    grid = make_grid(kind, xy, faces)
    wrapped = grid.to_periodic()
    rng = np.random.default_rng(43)
    for source, e, convert in ((grid, wrapped_e, lambda **kw: grid.to_periodic(**kw)),
                               (wrapped, unwrapped_e, lambda **kw: wrapped.to_nonperiodic(xmax, **kw))):
        for facet in ("node", "edge", "face"):
            dim = getattr(source, f"{facet}_dimension")
            for dtype in (np.float64, np.float32):
                data = rng.random((2, getattr(source, f"n_{facet}"))).astype(dtype)
                want = data[..., e[f"{facet}_index"]].astype(np.float64)
                for where in (data, engine.DeviceArray.from_host(data)):
                    new, values = convert(data=where, dim=dim)
                    assert new.n_node == len(e["xy"])
                    assert isinstance(values, np.ndarray if where is data else engine.DeviceArray)
                    values = to_numpy(values)
                    assert values.dtype == np.float64 and np.array_equal(values, want), (facet, dtype)
        # grid, indexes, data in that order; 1-D data, the facet found by its size where only one fits
        data = rng.random(source.n_face)
        if source.n_face not in (source.n_node, source.n_edge):
            new, indexes, values = convert(data=data, return_index=True)
            assert_indexes(source, indexes, e)
            assert np.array_equal(values, data[e["face_index"]])


# ---- the round trip on device grids through reindex_like ---------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CLEAN_CASES)
def test_round_trip_through_reindex_like(hip, name):
    """to_nonperiodic of to_periodic is the grid up to the node numbering, and the data comes back with it."""
    xy, faces, _ = pc.mesh(name)
    xmax = xy[:, 0].max()  # (the column's own x: the copies get the coordinates the right column had)
    grid = graph_cases.device_grid(xy, faces)
    dims = {"node": grid.node_dimension, "edge": grid.edge_dimension, "face": grid.face_dimension}
    rng = np.random.default_rng(47)
    e = pc.to_periodic(xy, faces)
    # what the seam shares must be equal on both of its sides to survive the fold: values per PERIODIC node and edge, spread
    old_edges = np.sort(e["node_inverse"][pc.host_edges(faces)], axis=1)
    edge_inverse = np.searchsorted(e["edges"][:, 0] * len(xy) + e["edges"][:, 1], old_edges[:, 0] * len(xy) + old_edges[:, 1])
    spread = {"node": e["node_inverse"], "edge": edge_inverse, "face": np.arange(len(faces))}
    for facet in ("node", "edge", "face"):
        data = rng.random(int(spread[facet].max()) + 1)[spread[facet]]
        assert len(data) == getattr(grid, f"n_{facet}")
        wrapped, folded = grid.to_periodic(data=data, dim=dims[facet])
        back, unfolded = wrapped.to_nonperiodic(xmax, data=folded, dim=dims[facet])
        assert isinstance(back, xa.ugrid2d.DeviceUgrid2d) and back.n_node == grid.n_node and back.n_face == grid.n_face
        assert np.array_equal(back.reindex_like(grid, unfolded, dim=dims[facet]), data), facet


# ---- the converted grid is a first-class mesh --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nonperiodic_grid_regrids_like_the_grid_built_nonperiodic(hip, kind):
    """Per target cell, bit for bit: the faces keep their order, so the sums run in the same order."""
    x_edges, y_edges = np.linspace(-180.0, 180.0, 13), np.linspace(-60.0, 60.0, 7)
    xy, faces = meshgen.quad_mesh(x_edges, y_edges)
    whole = make_grid(kind, xy, faces)
    periodic_e = pc.to_periodic(xy, faces)
    periodic = make_grid(kind, periodic_e["xy"], periodic_e["faces"])  # arrives periodic: the seam column shares its nodes
    assert periodic.n_node == whole.n_node - len(y_edges)
    data = np.random.default_rng(53).random(whole.n_face)
    converted, values = periodic.to_nonperiodic(180.0, data=data, dim=periodic.face_dimension)
    assert type(converted) is type(whole) and np.array_equal(values, data)
    raster = xa.Ugrid2d.from_structured_bounds(*(np.column_stack([e[:-1], e[1:]]) for e in (np.linspace(-180.0, 180.0, 6), np.linspace(-60.0, 60.0, 4))))
    for method in ("mean", "sum", "maximum"):
        got = xa.OverlapRegridder(converted, raster, method=method).regrid(values)
        want = xa.OverlapRegridder(whole, raster, method=method).regrid(data)
        assert not np.isnan(want).any() and np.array_equal(got, want), method


def test_nonmanifold_takes_the_host_route(hip):
    """Three faces on one edge next to a periodic strip: the device topology keeps no tables, the edges come from numpy."""
    xy, faces, xmax = pc.mesh("tri43")
    extra_xy, extra_faces = sc.three_faces_on_one_edge()
    extra_xy = extra_xy[:5] * 0.25 + np.array([1.25, 1.25])  # inside the strip's x range, away from both boundaries
    all_xy = np.concatenate([xy, extra_xy])
    all_faces = np.concatenate([faces, extra_faces[:3] + len(xy)])
    grid = graph_cases.device_grid(all_xy, all_faces)
    assert not grid.device_topology().manifold
    e = pc.to_periodic(all_xy, all_faces)
    wrapped, indexes = grid.to_periodic(return_index=True)
    assert isinstance(wrapped, xa.ugrid2d.DeviceUgrid2d)
    assert_grid(wrapped, e)
    assert_indexes(grid, indexes, e, engine.DeviceArray)
    e2 = pc.to_nonperiodic(e["xy"], e["faces"], xmax)
    unwrapped, indexes = wrapped.to_nonperiodic(xmax, return_index=True)
    assert_grid(unwrapped, e2)
    assert_indexes(wrapped, indexes, e2, engine.DeviceArray)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(hip, kind):
    xy, faces, xmax = pc.mesh("quads32")
    moved = xy.copy()
    moved[7, 1] += 0.25
    with pytest.raises(ValueError, match="y-coordinates of the left and right boundaries do not match"):
        make_grid(kind, moved, faces).to_periodic()
    more = np.concatenate([xy, [[3.0, 0.5]]])  # one more right node: the counts differ
    with pytest.raises(ValueError, match="y-coordinates of the left and right boundaries do not match"):
        make_grid(kind, more, faces).to_periodic()
    grid = make_grid(kind, xy, faces)
    wrapped = grid.to_periodic()
    for convert in (grid.to_periodic, lambda **kw: wrapped.to_nonperiodic(xmax, **kw)):
        with pytest.raises(ValueError, match="exactly one UGRID dimension"):
            convert(data=np.zeros(1000))
        with pytest.raises(ValueError, match="exactly one UGRID dimension"):
            convert(data=np.zeros(6), dim=grid.node_dimension)
        with pytest.raises(ValueError, match="not a UGRID dimension"):
            convert(data=np.zeros(6), dim="nowhere")
    # everything is usable afterwards
    wrapped_e, unwrapped_e = pc.expected("quads32")
    assert_grid(grid.to_periodic(), wrapped_e)
    assert_grid(wrapped.to_nonperiodic(xmax), unwrapped_e)
    assert np.array_equal(grid.face_node_connectivity, faces)


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/periodic_worker_gpu.py): tensor data and tensor indexes, on both kinds of grid
def test_torch_in_torch_out():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "periodic_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_PERIODIC_OK" in res.stdout
