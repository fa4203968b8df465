"""
GPU: snapping (csrc/xr_snap.hip) behind ``xa.snap_nodes`` / ``xa.snap_to_nodes`` / ``Ugrid2d.snap_to_nodes`` / ``Ugrid1d.snap_to_nodes`` /
``Ugrid1d.snap_nodes``.  Yardsticks in tests/snap_cases.py: numpy / scipy restatements, pinned to the reference's own output by
tests/test_snap_cpu.py; the reference's own test cases are compared with its expected values as well.  Every comparison is exact:
ids are integers and coordinates are copied, so they are compared bit for bit.
"""
import json
import os

import numpy as np
import pytest

import snap_cases as sc
import xugrid_amd as xa
from xugrid_amd import engine

pytestmark = pytest.mark.gpu

KNOWN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "snap_known.json")))
_REFERENCE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_floats(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float64 and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def nodes_ref(name):
    """The restatement's answer for a case, computed once."""
    if name not in _REFERENCE:
        x, y, d = sc.NODES_CASES[name]()
        _REFERENCE[name] = (x, y, d) + sc.snap_nodes_ref(x, y, d)
    return _REFERENCE[name]


def dev(a, dtype=np.float64):
    return engine.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype))


def assert_nodes(result, x, y, e_inverse, e_x, e_y):
    inverse, xs, ys = result
    if e_inverse is None:
        assert inverse is None
    else:
        assert isinstance(inverse, np.ndarray) and inverse.dtype == np.int64 and np.array_equal(inverse, e_inverse)
    assert same_floats(xs, e_x) and same_floats(ys, e_y)
    assert not np.shares_memory(xs, x) and not np.shares_memory(ys, y)


# ---- snap_nodes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.NODES_CASES))
def test_snap_nodes(hip, name):
    x, y, d, e_inverse, _, e_x, e_y = nodes_ref(name)
    x0, y0 = x.copy(), y.copy()
    assert_nodes(xa.snap_nodes(x, y, d), x, y, e_inverse, e_x, e_y)
    assert np.array_equal(bits(x), bits(x0)) and np.array_equal(bits(y), bits(y0))
    # ... the goldens themselves: what the reference returned
    known = KNOWN["snap_nodes"][name]
    inverse, xs, ys = xa.snap_nodes(x, y, d)
    assert (inverse is None) if known["inverse"] is None else sc.equals_known(inverse, known["inverse"])
    assert sc.equals_known(xs, known["x"]) and sc.equals_known(ys, known["y"])


@pytest.mark.parametrize("name", sorted(KNOWN["reference_test"]["snap_nodes"]))
def test_snap_nodes_reference_tests(hip, name):
    x, y, d = sc.NODES_CASES[name]()
    expected = KNOWN["reference_test"]["snap_nodes"][name]
    inverse, xs, ys = xa.snap_nodes(x, y, d)
    assert (inverse is None) if expected["inverse"] is None else np.array_equal(inverse, expected["inverse"])
    assert np.array_equal(xs, expected["x"]) and np.array_equal(ys, expected["y"])


@pytest.mark.parametrize("name", ["lattice2049_0.5", "scattered2049", "apart", "chain70", "coincident_d0", "two_near"])
def test_snap_nodes_device_arrays(hip, name):
    x, y, d, e_inverse, _, e_x, e_y = nodes_ref(name)
    dx, dy = dev(x), dev(y)
    inverse, xs, ys = xa.snap_nodes(dx, dy, d)
    assert isinstance(xs, engine.DeviceArray) and isinstance(ys, engine.DeviceArray)
    assert xs.ptr not in (dx.ptr, dy.ptr) and ys.ptr not in (dx.ptr, dy.ptr)
    if e_inverse is None:
        assert inverse is None
    else:
        assert isinstance(inverse, engine.DeviceArray) and inverse.dtype == np.int64 and np.array_equal(inverse.download(), e_inverse)
    assert same_floats(xs.download(), e_x) and same_floats(ys.download(), e_y)
    assert np.array_equal(bits(dx.download()), bits(x)) and np.array_equal(bits(dy.download()), bits(y))


def merge_of(x, y, d):
    both = dev(np.stack((x, y)))
    return engine.DeviceSnap(both.ptr, both.ptr + 8 * len(x), 1, len(x), d)


def test_chain_rounds(hip):
    """Along a chain numbered in order every decision waits for the one before it, and a launch settles at most SWEEPS of them;
    numbered the other way round the chain is the same chain.  With the even places numbered first nothing waits: the even
    places have no lower-numbered neighbour (round 1) and the odd ones see them at once or in the next launch."""
    n = 2050
    for case in (sc.chain, sc.chain_reversed):
        merged = merge_of(*case(n), 0.25)
        assert merged.n_kept == n // 2 and merged.n_pair == 2 * (n - 1)
        assert n / engine.DeviceSnap.SWEEPS <= merged.rounds <= n
    merged = merge_of(*sc.chain_interleaved(n), 0.25)
    assert merged.n_kept == n // 2 and 1 <= merged.rounds <= 2


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_snap_nodes_not_finite(hip, bad):
    x, y = sc.scattered(100)
    x = x.copy()
    x[37] = bad
    with pytest.raises(ValueError, match="data must be finite"):
        xa.snap_nodes(x, y, 0.5)
    with pytest.raises(ValueError, match="data must be finite"):
        xa.snap_nodes(dev(x), dev(y), 0.5)
    with pytest.raises(ValueError, match="data must be finite"):
        xa.snap_nodes(y, x, 1e-9)


def test_snap_nodes_arguments(hip):
    x, y = sc.scattered(10)
    with pytest.raises(ValueError):
        xa.snap_nodes(x, y, -1.0)
    with pytest.raises(ValueError):
        xa.snap_nodes(x, y[:5], 1.0)
    with pytest.raises(TypeError):
        xa.snap_nodes(dev(x), y, 1.0)


# ---- snap_to_nodes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.TO_CASES))
def test_snap_to_nodes(hip, name):
    x, y, to_x, to_y, d = sc.TO_CASES[name]()
    e_x, e_y, e_index, e_count = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    xs, ys, index = xa.snap_to_nodes(x, y, to_x, to_y, d, tiebreaker="nearest", return_index=True)
    assert same_floats(xs, e_x) and same_floats(ys, e_y)
    assert isinstance(index, np.ndarray) and index.dtype == np.int64 and np.array_equal(index, e_index)
    # the index agrees with the coordinates
    hit = index >= 0
    assert same_floats(xs[hit], np.asarray(to_x)[index[hit]]) and same_floats(xs[~hit], np.asarray(x)[~hit])
    assert same_floats(ys[hit], np.asarray(to_y)[index[hit]]) and same_floats(ys[~hit], np.asarray(y)[~hit])
    assert not np.shares_memory(xs, x) and not np.shares_memory(ys, y)
    known = KNOWN["snap_to_nodes"][name]
    assert sc.equals_known(xs, known["nearest"]["x"]) and sc.equals_known(ys, known["nearest"]["y"])
    if (e_count > 1).any():
        with pytest.raises(ValueError) as error:
            xa.snap_to_nodes(x, y, to_x, to_y, d)
        assert str(error.value) == known["no_tiebreaker"]["raises"]
    else:
        xs, ys = xa.snap_to_nodes(x, y, to_x, to_y, d)
        assert sc.equals_known(xs, known["no_tiebreaker"]["x"]) and sc.equals_known(ys, known["no_tiebreaker"]["y"])


@pytest.mark.parametrize("name", sorted(KNOWN["reference_test"]["snap_to_nodes"]))
def test_snap_to_nodes_reference_tests(hip, name):
    x, y, to_x, to_y, d = sc.TO_CASES[name]()
    expected = KNOWN["reference_test"]["snap_to_nodes"][name]
    xs, ys = xa.snap_to_nodes(x, y, to_x, to_y, d, tiebreaker="nearest")
    assert np.array_equal(xs, expected["x"]) and np.array_equal(ys, expected["y"])


def test_snap_to_nodes_equidistant(hip):
    x, y, to_x, to_y, d = sc.EQUIDISTANT
    e_x, e_y, e_index, _ = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    xs, ys, index = xa.snap_to_nodes(x, y, to_x, to_y, d, tiebreaker="nearest", return_index=True)
    assert index.tolist() == [0, 2] and np.array_equal(index, e_index)
    assert same_floats(xs, e_x) and same_floats(ys, e_y)
    # ... whatever the order the nodes are stored in
    xs, ys, index = xa.snap_to_nodes(x, y, to_x[::-1].copy(), to_y[::-1].copy(), d, tiebreaker="nearest", return_index=True)
    assert index.tolist() == [2, 0]


def test_snap_to_nodes_tiebreaker(hip, monkeypatch):
    x, y, to_x, to_y, d = sc.TO_CASES["ref_take_nearest"]()
    with pytest.raises(ValueError) as error:
        xa.snap_to_nodes(x, y, to_x, to_y, d)
    assert str(error.value) == sc.TIES
    # a bad tiebreaker raises before any device work
    from xugrid_amd import _lib

    def no_device(*args):
        raise AssertionError("the device was used")

    grid = xa.Ugrid1d(to_x, to_y, -1, np.array([[0, 1], [1, 2]]))
    monkeypatch.setattr(_lib, "load", no_device)
    for call in (lambda: xa.snap_to_nodes(x, y, to_x, to_y, d, tiebreaker="first"),
                 lambda: grid.snap_to_nodes(x, y, d, tiebreaker="first")):
        with pytest.raises(ValueError) as error:
            call()
        assert str(error.value) == KNOWN["bad_tiebreaker"]["raises"]


def test_snap_to_nodes_empty(hip):
    x, y, to_x, to_y = sc.random_to(65, 63, 3)
    none = np.empty(0)
    xs, ys, index = xa.snap_to_nodes(x, y, none, none, 1.0, return_index=True)
    assert same_floats(xs, x) and same_floats(ys, y) and not np.shares_memory(xs, x) and np.array_equal(index, np.full(65, -1))
    xs, ys, index = xa.snap_to_nodes(none, none, to_x, to_y, 1.0, return_index=True)
    assert xs.shape == ys.shape == index.shape == (0,) and xs.dtype == np.float64 and index.dtype == np.int64
    xs, ys = xa.snap_to_nodes(none, none, none, none, 1.0)
    assert xs.shape == ys.shape == (0,)
    xs, ys, index = xa.snap_to_nodes(dev(x), dev(y), dev(none), dev(none), 1.0, return_index=True)
    assert same_floats(xs.download(), x) and np.array_equal(index.download(), np.full(65, -1))


def test_snap_to_nodes_not_finite(hip):
    x, y, to_x, to_y = sc.random_to(65, 63, 3)
    for position in (0, 1, 2, 3):
        for bad in (np.nan, np.inf):
            arrays = [a.copy() for a in (x, y, to_x, to_y)]
            arrays[position][11] = bad
            with pytest.raises(ValueError, match="data must be finite"):
                xa.snap_to_nodes(*arrays, 0.3, tiebreaker="nearest")
    with pytest.raises(ValueError, match="data must be finite"):
        xa.snap_to_nodes(np.array([np.nan]), np.array([0.0]), np.empty(0), np.empty(0), 0.3)


@pytest.mark.parametrize("name", ["random2049x300_several", "random300x2049_one", "duplicates_d025"])
def test_snap_to_nodes_device_arrays(hip, name):
    x, y, to_x, to_y, d = sc.TO_CASES[name]()
    e_x, e_y, e_index, _ = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    dx, dy = dev(x), dev(y)
    xs, ys, index = xa.snap_to_nodes(dx, dy, dev(to_x), dev(to_y), d, tiebreaker="nearest", return_index=True)
    assert all(isinstance(a, engine.DeviceArray) for a in (xs, ys, index)) and index.dtype == np.int64
    assert xs.ptr not in (dx.ptr, dy.ptr) and ys.ptr not in (dx.ptr, dy.ptr)
    assert same_floats(xs.download(), e_x) and same_floats(ys.download(), e_y) and np.array_equal(index.download(), e_index)
    with pytest.raises(ValueError) as error:
        xa.snap_to_nodes(dx, dy, dev(to_x), dev(to_y), d)
    assert str(error.value) == sc.TIES


# ---- the grids' methods ---------------------------------------------------------------------------------------------------------------
def test_grid_snap_to_nodes(hip):
    from xugrid_amd import meshgen

    xy, faces = meshgen.triangle_mesh(400, 0)
    x, y, _, _ = sc.random_to(300, 300, 11)
    span = xy.max(axis=0) - xy.min(axis=0)
    x, y = xy[:, 0].min() + x / x.max() * span[0], xy[:, 1].min() + y / y.max() * span[1]
    d = 0.75 * np.sqrt(span[0] * span[1] / len(xy))
    expected = xa.snap_to_nodes(x, y, xy[:, 0].copy(), xy[:, 1].copy(), d, tiebreaker="nearest", return_index=True)
    assert (expected[2] >= 0).any() and (expected[2] < 0).any()
    grid2d = xa.Ugrid2d.from_device_arrays(dev(xy), dev(faces, np.int64))
    edges = np.column_stack([np.arange(len(xy) - 1), np.arange(1, len(xy))])
    grid1d = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)
    for grid in (grid2d, grid1d):
        got = grid.snap_to_nodes(x, y, d, tiebreaker="nearest", return_index=True)
        assert same_floats(got[0], expected[0]) and same_floats(got[1], expected[1]) and np.array_equal(got[2], expected[2])
        got = grid.snap_to_nodes(dev(x), dev(y), d, tiebreaker="nearest")
        assert same_floats(got[0].download(), expected[0]) and same_floats(got[1].download(), expected[1])
        assert grid._nearest_index("node") is grid._nearest_index("node")


def test_network_snap_nodes_two_lines(hip):
    x, y, d = sc.NODES_CASES["ref_two_lines_0.1"]()
    grid = xa.Ugrid1d(x, y, -1, sc.TWO_LINES_EDGES, name="net")
    expected = KNOWN["reference_test"]["snap_nodes"]["ref_two_lines_0.1"]
    snapped, index = grid.snap_nodes(d, return_index=True)
    assert isinstance(snapped, xa.Ugrid1d) and snapped.name == "net"
    assert np.array_equal(snapped.node_x, expected["x"]) and np.array_equal(snapped.node_y, expected["y"])
    assert np.array_equal(snapped.edge_node_connectivity, KNOWN["reference_test"]["two_lines_edges"])
    assert set(index) == {grid.node_dimension} and np.array_equal(index[grid.node_dimension], expected["inverse"])
    # nothing within the distance: the grid itself
    assert grid.snap_nodes(0.001) is grid
    same, index = grid.snap_nodes(0.001, return_index=True)
    assert same is grid and index == {grid.node_dimension: None}
    # self-loops that arise are kept
    looped = grid.snap_nodes(1.5)
    assert looped.n_edge == 2 and (looped.edge_node_connectivity[:, 0] == looped.edge_node_connectivity[:, 1]).any()


def test_network_snap_nodes_doubled(hip):
    xy, edges, d = sc.doubled_network(2000)
    e_inverse, e_ids, e_x, e_y = sc.snap_nodes_ref(xy[:, 0], xy[:, 1], d)
    assert len(e_ids) <= 2000
    grid = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, edges, name="net")
    snapped, index = grid.snap_nodes(d, return_index=True)
    assert snapped.name == "net" and snapped.n_edge == grid.n_edge
    assert same_floats(snapped.node_x, e_x) and same_floats(snapped.node_y, e_y)
    assert np.array_equal(index[grid.node_dimension], e_inverse)
    assert np.array_equal(snapped.edge_node_connectivity, e_inverse[edges])


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/snap_worker_gpu.py): tensors in, tensors out
def test_torch_in_torch_out():
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "snap_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_SNAP_OK" in res.stdout
