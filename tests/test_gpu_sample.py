"""
GPU (-m gpu): reading mesh data at points and along lines on the device -- ``locate_nearest_*``, ``sel_points``, ``sel``,
``intersect_line`` / ``intersect_linestring`` (xugrid_amd/sample.py, csrc/xr_sample.hip).  Known answers of the reference's
own tests (numbers transcribed from tests/test_ugrid2d.py), the nearest search at size against scipy's KDTree and at its
edges against a brute-force search of the kernel's arithmetic, the gather through every input kind, sections at size against
a numpy restatement, and a grid that lives on the device only.
"""
import warnings

import numpy as np
import pytest

import xugrid_amd as xa
from sample_cases import brute_nearest, grid2d_arrays, kdtree_nearest, length_inside_hull, section_numpy
from xugrid_amd import meshgen, sample

pytestmark = pytest.mark.gpu

OOB_X = [-10.0, 0.5, -20.0, 1.5, -30.0]
OOB_Y = [-10.0, 0.5, -20.0, 1.25, -30.0]


@pytest.fixture
def grid(hip):
    xy, faces = grid2d_arrays()
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


@pytest.fixture(scope="module")
def big(hip):
    xy, faces = meshgen.triangle_mesh(100_000, 0)
    assert faces.shape[0] == 199_686
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces), xy


def index_of(points):
    return sample.NearestIndex.from_points(np.ascontiguousarray(points, dtype=np.float64))


# ---- known answers of the reference's tests -----------------------------------------------------------------------------------
def test_locate_nearest_known_answers(grid):
    """tests/test_ugrid2d.py:1891-1905"""
    assert np.array_equal(grid.locate_nearest_node(grid.node_coordinates), [0, 1, 2, 3, 4, 5, 6])
    assert np.array_equal(grid.locate_nearest_edge(grid.edge_coordinates), np.arange(10))
    assert np.array_equal(grid.locate_nearest_face(grid.centroids), [0, 1, 2, 3])
    for locate in (grid.locate_nearest_node, grid.locate_nearest_edge, grid.locate_nearest_face):
        assert np.array_equal(locate([[-10.0, 0.0]], 1.0), [-1])
    net = xa.Ugrid1d(grid.node_x, grid.node_y, -1, grid.edge_node_connectivity)
    assert np.array_equal(net.locate_nearest_node(net.node_coordinates), np.arange(7))
    assert np.array_equal(net.locate_nearest_edge(net.edge_coordinates), np.arange(10))
    assert np.array_equal(net.locate_nearest_edge([[-10.0, 0.0]], 1.0), [-1])


def test_sel_points_known_answers(grid):
    """tests/test_ugrid2d.py:835-890"""
    data = np.array([0.0, 1.0, 2.0, 3.0])
    x, y = [0.5, 1.5], [0.5, 1.25]
    got = grid.sel_points(data, x, y)
    assert np.array_equal(got.values, [0, 3]) and np.array_equal(got.index, [0, 1])
    assert np.array_equal(got.x, x) and np.array_equal(got.y, y)

    with pytest.raises(ValueError, match="Not all points are located on the topology"):
        grid.sel_points(data, OOB_X, OOB_Y, out_of_bounds="raise")
    got = grid.sel_points(data, OOB_X, OOB_Y, out_of_bounds="drop")
    assert np.array_equal(got.values, [0, 3]) and np.array_equal(got.index, [1, 3])
    assert np.array_equal(got.x, [0.5, 1.5]) and np.array_equal(got.y, [0.5, 1.25])
    with pytest.warns(UserWarning, match="Not all points are located on the topology"):
        got = grid.sel_points(data, OOB_X, OOB_Y, out_of_bounds="warn")
    assert np.array_equal(got.values, [np.nan, 0, np.nan, 3, np.nan], equal_nan=True)
    assert np.array_equal(got.index, np.arange(5)) and np.array_equal(got.x, OOB_X)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = grid.sel_points(data, OOB_X, OOB_Y, out_of_bounds="ignore")
        assert np.array_equal(got.values, [np.nan, 0, np.nan, 3, np.nan], equal_nan=True)
        got = grid.sel_points(data, OOB_X, OOB_Y, out_of_bounds="ignore", fill_value=-1)
        assert np.array_equal(got.values, [-1, 0, -1, 3, -1])
        got = grid.sel_points(data, OOB_X, OOB_Y, out_of_bounds="drop", tolerance=11.0)
        assert np.array_equal(got.index, [1, 3])


def test_sel_points_multiple_dims(grid):
    """tests/test_ugrid2d.py:892-925: node (and edge) data take the nearest entity; containment still decides the bounds"""
    node_data, edge_data = np.arange(grid.n_node, dtype=np.float64), np.arange(grid.n_edge, dtype=np.float64)
    got = grid.sel_points(node_data, OOB_X, OOB_Y, dim="node", out_of_bounds="ignore")
    assert np.array_equal(got.values, [np.nan, 0, np.nan, 4, np.nan], equal_nan=True)
    got = grid.sel_points(node_data, OOB_X, OOB_Y, dim=grid.node_dimension, out_of_bounds="drop")
    assert np.array_equal(got.values, [0, 4]) and np.array_equal(got.index, [1, 3])
    pts = np.column_stack([OOB_X, OOB_Y])
    got = grid.sel_points(edge_data, OOB_X, OOB_Y, dim="edge", out_of_bounds="ignore")
    expected = brute_nearest(grid.edge_coordinates, pts).astype(np.float64)
    expected[[0, 2, 4]] = np.nan
    assert np.array_equal(got.values, expected, equal_nan=True)
    # face data with method="nearest": the nearest centroid, out-of-bounds points still filled
    got = grid.sel_points(np.arange(4.0), OOB_X, OOB_Y, method="nearest", out_of_bounds="ignore")
    assert np.array_equal(got.values, [np.nan, 0, np.nan, 3, np.nan], equal_nan=True)


def test_intersect_line_known_answers(grid):
    """tests/test_ugrid2d.py:1153-1187"""
    data = np.array([0.0, 1.0, 2.0, 3.0])
    r2 = np.sqrt(2.0)
    got = grid.intersect_line(data, start=(0.0, 0.0), end=(2.0, 2.0))
    assert np.array_equal(got.values, [0, 3]) and np.array_equal(got.face_index, [0, 3])
    assert np.allclose(got.x, [0.5, 1.25]) and np.allclose(got.y, [0.5, 1.25]) and np.allclose(got.s, [0.5 * r2, 1.25 * r2])
    got = grid.intersect_line(data, start=(2.0, 2.0), end=(0.0, 0.0))
    assert np.array_equal(got.values, [3, 0])
    got = grid.intersect_linestring(data, [[0.5, 0.5], [1.5, 0.5], [1.5, 1.5]])
    assert np.array_equal(got.values, [0, 1, 1, 3])
    assert np.allclose(got.x, [0.75, 1.25, 1.5, 1.5]) and np.allclose(got.y, [0.5, 0.5, 0.75, 1.25])
    assert np.allclose(got.s, [0.25, 0.75, 1.25, 1.75])
    e, f, p = grid.intersect_edges(np.array([[[0.0, 0.0], [2.0, 2.0]]]))
    assert np.array_equal(e, [0, 0]) and np.array_equal(f, [0, 3]) and p.shape == (2, 2, 2)


def test_sel_known_answers(grid):
    """tests/test_ugrid2d.py:1029-1145 (the index and the values; the reference's sub-grid is out of scope)"""
    data = np.array([0.0, 1.0, 2.0, 3.0])

    def box(expected, **kw):
        got = grid.sel(data, **kw)
        assert isinstance(got, sample.BoxSelection)
        assert np.array_equal(got.values, expected) and np.array_equal(got.face_index, expected)

    box([0, 1], x=slice(0.0, 2.0), y=slice(0.0, 1.0))
    box([0, 1], x=slice(None, None), y=slice(None, 1.0))
    box([0, 2], x=slice(0.0, 1.0), y=slice(0.0, 2.0))
    box([0, 2], x=slice(None, 1.0), y=slice(None, None))
    for x, y in zip([None, None, slice(0, 2)], [None, slice(0, 2), None]):
        box([0, 1, 2, 3], x=x, y=y)
    box([0, 1, 2, 3])
    assert np.array_equal(grid.locate_bounding_box(0.0, 0.0, 2.0, 1.0), [0, 1])

    for x, y in ((0.5, 0.5), ([0.5], [0.5])):
        got = grid.sel(data, x=x, y=y)
        assert np.array_equal(got.values, [0]) and np.array_equal(got.x, [0.5]) and np.array_equal(got.y, [0.5])
    with pytest.raises(TypeError, match="Invalid indexer type"):
        grid.sel(data, x=(0.5,), y=[0.5])
    for x in ([0.4, 0.8, 1.2], slice(0.4, 1.5, 0.4)):
        got = grid.sel(data, x=x, y=[0.5, 1.1])
        assert np.array_equal(got.values, [0, 0, 1, 2, 2, 3])
        assert np.allclose(got.x, [0.4, 0.8, 1.2, 0.4, 0.8, 1.2]) and np.allclose(got.y, [0.5, 0.5, 0.5, 1.1, 1.1, 1.1])

    got = grid.sel(data, x=slice(None, None), y=0.5)
    assert np.array_equal(got.values, [0, 1]) and np.allclose(got.x, [0.5, 1.5])
    assert np.allclose(got.y, [0.5, 0.5]) and np.allclose(got.s, [0.5, 1.5])
    got = grid.sel(data, x=0.5, y=slice(None, None))
    assert np.array_equal(got.values, [0, 2]) and np.allclose(got.x, [0.5, 0.5])
    assert np.allclose(got.y, [0.5, 1.25]) and np.allclose(got.s, [0.5, 1.25])


# ---- nearest at size, against scipy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("facet", ["node", "face"])
def test_nearest_at_size_equals_kdtree(big, facet):
    """300 000 random queries over the node bounds widened by 10 % per side: the device index equals KDTree.query's for
    every query whose nearest neighbour is unique in float64.  No query may be left out of the comparison (cap 0: these
    inputs hold no tie)."""
    grid, xy = big
    points = xy if facet == "node" else grid.centroids
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    pad = 0.1 * (hi - lo)
    queries = np.random.default_rng(7).uniform(lo - pad, hi + pad, (300_000, 2))
    locate = grid.locate_nearest_node if facet == "node" else grid.locate_nearest_face
    expected, unique = kdtree_nearest(points, queries)
    left_out = int((~unique).sum())
    print(f"{facet}: {left_out} of {len(queries)} queries have a tied nearest neighbour")
    assert left_out == 0
    got = locate(queries)
    assert got.dtype == np.intp and np.array_equal(got, expected)
    # ... and with the bound at the median nearest distance: about half the answers are -1, and they match exactly
    d = points[expected] - queries
    median = float(np.median(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])))
    expected_md, _ = kdtree_nearest(points, queries, median)
    got = locate(queries, median)
    share = float((expected_md == -1).mean())
    print(f"{facet}: max_distance {median:.3e}, {share:.3f} of the answers are -1")
    assert 0.4 < share < 0.6
    assert np.array_equal(got, expected_md)


# ---- ties and edges, against the brute-force yardstick -------------------------------------------------------------------------
def assert_brute(points, queries, max_distance=np.inf, index=None):
    index = index_of(points) if index is None else index
    got = index.query(queries, max_distance)
    expected = brute_nearest(points, queries, max_distance)
    bad = np.nonzero(got != expected)[0]
    assert bad.size == 0, f"{bad.size} of {len(expected)} queries differ: {bad[:5]} {got[bad[:5]]} {expected[bad[:5]]}"
    return got


@pytest.mark.parametrize("n", [250, 256, 257, 65_536, 65_537, 65_792])
def test_extent_at_the_edges_of_its_reduction(hip, n):
    """The index's bounding box and point count are a two-launch reduction over blocks of 256 points: less than a block, one
    block, one block and a lane, 256 partials, 257 with one point and with a full block.  The LAST point alone stretches the box
    (up and to the right), and a quarter of the queries lie around it."""
    rng = np.random.default_rng(n)
    points = rng.uniform(0.0, 1.0, (n, 2))
    points[-1] = (3.0, 2.5)
    queries = np.concatenate([rng.uniform(-0.2, 1.2, (600, 2)), points[-1] + rng.uniform(-1.5, 1.5, (200, 2))])
    got = assert_brute(points, queries)
    assert (got == n - 1).sum() > 50
    assert_brute(points, queries, 0.05)


def test_ties_take_the_lowest_id(hip):
    """Queries at the nodes of a quad lattice against its face centroids: four equidistant centroids inside, two on the
    sides, one at the corners.  (scipy agrees with the lowest id on about half of such queries: not the yardstick here.)"""
    e = np.arange(51, dtype=np.float64)  # (integer edges: the four squared distances are exactly 0.5)
    xy, faces = meshgen.quad_mesh(e, e)
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    centroids = grid.centroids
    got = grid.locate_nearest_face(xy)
    assert np.array_equal(got, brute_nearest(centroids, xy))
    inner = np.nonzero((xy[:, 0] > 0) & (xy[:, 0] < 50) & (xy[:, 1] > 0) & (xy[:, 1] < 50))[0]
    jx, jy = xy[inner, 0].astype(np.int64), xy[inner, 1].astype(np.int64)
    assert np.array_equal(got[inner], (jy - 1) * 50 + (jx - 1))  # the lower-left of the four faces has the lowest id
    # the same points shuffled: the ids move, the rule stays
    perm = np.random.default_rng(0).permutation(len(centroids))
    assert_brute(centroids[perm], xy)


def test_max_distance_is_exclusive(hip):
    points = np.array([[3.0, 4.0], [30.0, 40.0], [-6.0, 8.0]])
    index = index_of(points)
    q = np.array([[0.0, 0.0]])
    assert index.query(q, 5.0)[0] == -1 and index.query(q, np.nextafter(5.0, 6.0))[0] == 0
    assert index.query(q, 0.0)[0] == -1 and index.query(q)[0] == 0 and index.query(q, None)[0] == 0
    assert index.query(np.array([[3.0, 4.0]]), 1e-150)[0] == 0  # (distance 0; the bound is compared squared)
    rng = np.random.default_rng(5)
    points, queries = rng.random((5000, 2)), rng.uniform(-0.1, 1.1, (3000, 2))
    index = index_of(points)
    for md in (0.001, 0.01, 0.05, 1.0):
        assert_brute(points, queries, md, index)
    with pytest.raises(ValueError, match="non-negative"):
        index.query(q, -1.0)


def test_degenerate_point_sets(hip):
    rng = np.random.default_rng(11)
    queries = np.vstack([rng.uniform(-2.0, 3.0, (2000, 2)), [[0.5, 0.5], [np.nan, 0.5], [0.5, np.nan], [np.nan, np.nan]]])
    # all points in one cell: a tight cluster and one far point stretch the box
    cluster = np.vstack([0.5 + 1e-9 * rng.random((3000, 2)), [[1000.0, 1000.0]]])
    assert_brute(cluster, queries)
    # coincident points: the lowest id
    same = np.tile([[0.25, 0.75]], (100, 1))
    assert np.array_equal(assert_brute(same, queries)[:2000], np.zeros(2000))
    # all points on one line (boxes of no height, no width)
    t = rng.random(4000)
    assert_brute(np.column_stack([t, np.full_like(t, 0.3)]), queries)
    assert_brute(np.column_stack([np.full_like(t, -0.7), t]), queries)
    assert_brute(np.column_stack([t, 2.0 * t]), queries)  # (a diagonal: a full box with empty cells off the line)
    # one indexed point
    got = assert_brute(np.array([[0.1, 0.2]]), queries)
    assert np.array_equal(got[:2001], np.zeros(2001)) and np.array_equal(got[2001:], [-1, -1, -1])
    assert np.array_equal(index_of([[0.1, 0.2]]).query(queries, 0.5), brute_nearest([[0.1, 0.2]], queries, 0.5))


def test_far_queries_nan_queries_and_empty_inputs(hip):
    rng = np.random.default_rng(12)
    points = rng.random((20_000, 2))
    index = index_of(points)
    assert index.n == 20_000 and 0 < index.n_cell <= 4 * index.n + 16
    far = np.array([[10.0, 10.0], [-10.0, 0.5], [0.5, -10.0], [12.0, -11.0], [-9.5, 10.5], [0.25, 10.0], [1e6, 1e6],
                    [-1e9, 0.5], [np.nan, 0.0]])
    got = assert_brute(points, far, index=index)
    assert got[-1] == -1 and (got[:-1] >= 0).all()
    assert_brute(points, far, 9.5, index)
    empty = index.query(np.zeros((0, 2)))
    assert empty.shape == (0,) and empty.dtype == np.intp
    with pytest.raises(ValueError, match="no points to index"):
        index_of(np.zeros((0, 2)))


def test_query_order_does_not_change_the_answers(hip, xr_option):
    """Caller order (option nn_query_sort = 0), index-cell order (1) and the choice by the number of queries (-1), on both
    sides of the threshold: identical output."""
    rng = np.random.default_rng(13)
    points = rng.random((50_000, 2))
    index = index_of(points)
    for n_query in (1000, 600_000):
        queries = rng.uniform(-0.1, 1.1, (n_query, 2))
        queries[::97] = np.nan
        out = {}
        for mode in (0, 1, -1):
            xr_option("nn_query_sort", mode)
            out[mode] = index.query(queries, 0.01 if n_query == 1000 else np.inf)
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[-1])
        head = slice(0, 1500)
        assert np.array_equal(out[0][head], brute_nearest(points, queries[head], 0.01 if n_query == 1000 else np.inf))


# ---- gather and sel_points end to end -----------------------------------------------------------------------------------------
def test_gather_kinds_and_shapes(big):
    grid, _ = big
    rng = np.random.default_rng(21)
    n = grid.n_face
    pts = rng.uniform(-0.05, 1.05, (5000, 2))
    face = grid.locate_points(pts)
    assert (face == -1).any() and (face >= 0).any()
    for dtype in (np.float64, np.float32):
        data = rng.normal(size=(3, 2, n)).astype(dtype)
        before = data.copy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = grid.sel_points(data, pts[:, 0], pts[:, 1])
        # the face indices sel_points uses are those of locate_points
        expected = np.where(face >= 0, data[..., np.maximum(face, 0)].astype(np.float64), np.nan)
        assert got.values.shape == (3, 2, 5000) and got.values.dtype == np.float64
        assert np.array_equal(got.values, expected, equal_nan=True)
        assert np.array_equal(data, before) and np.array_equal(got.index, np.arange(5000))
    # a DeviceArray in, a DeviceArray out
    data = rng.normal(size=(4, n))
    dev = xa.engine.DeviceArray.from_host(data)
    out = sample.gather_points(dev, n, face, -7.0)
    assert isinstance(out, xa.engine.DeviceArray)
    assert np.array_equal(out.download(), np.where(face >= 0, data[:, np.maximum(face, 0)], -7.0))
    assert np.array_equal(dev.download(), data)  # (the input is never modified)
    # no points
    assert sample.gather_points(data, n, np.zeros(0, dtype=np.int64)).shape == (4, 0)


def test_gather_past_one_launch_grid_and_index_errors(grid):
    K = 70_000  # (slices ride on gridDim.y in tiles of 65 535)
    data = np.arange(K * 4, dtype=np.float64).reshape(K, 4)
    got = grid.sel_points(data, [0.5, 1.5, -5.0], [0.5, 1.25, 0.0], out_of_bounds="ignore", fill_value=-2.0)
    assert got.values.shape == (K, 3)
    assert np.array_equal(got.values, np.column_stack([data[:, 0], data[:, 3], np.full(K, -2.0)]))
    for bad in ([0, 4], [2**40, 1], [3, 1, 4, -1]):
        with pytest.raises(ValueError, match="index out of range"):
            sample.gather_points(data[:3], 4, np.array(bad))
    assert np.array_equal(sample.gather_points(data[:2], 4, np.array([3, -1, -5, 0]))[0], [3.0, np.nan, np.nan, 0.0],
                          equal_nan=True)
    with pytest.raises(ValueError, match=r"expected data of shape \(\.\.\., 4\)"):
        grid.sel_points(np.zeros(5), [0.5], [0.5])


# ---- sections at size ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diagonal", "zigzag"])
def test_sections_at_size(big, name):
    grid, xy = big
    line = {"diagonal": [[-0.2, -0.1], [1.2, 1.1]],
            "zigzag": [[0.05, 0.1], [0.3, 0.9], [0.5, 0.2], [0.7, 0.95], [0.95, 0.15]]}[name]
    line = np.array(line)
    segments = np.stack((line[:-1], line[1:]), axis=1)
    data = np.random.default_rng(31).normal(size=(2, grid.n_face))
    got = grid.intersect_linestring(data, line) if name == "zigzag" else grid.intersect_line(data, line[0], line[1])
    n = len(got.s)
    assert n > 500 and got.values.shape == (2, n)
    assert np.all(np.diff(got.s) >= 0.0)
    assert np.array_equal(got.values, data[..., got.face_index])
    # s, x and y equal the numpy restatement of the arithmetic bit for bit
    seg, face, pieces = grid.intersect_edges(segments)
    mid, s = section_numpy(pieces, seg, segments)
    order = np.argsort(s, kind="stable")
    assert np.array_equal(got.face_index, face[order])
    assert np.array_equal(got.s, s[order]) and np.array_equal(got.x, mid[order, 0]) and np.array_equal(got.y, mid[order, 1])
    # the pieces tile the part of the line inside the mesh (its convex hull: a Delaunay triangulation)
    d = pieces[:, 1] - pieces[:, 0]
    total, inside = float(np.hypot(d[:, 0], d[:, 1]).sum()), length_inside_hull(xy, segments)
    print(f"{name}: {n} pieces, summed length {total!r}, inside the hull {inside!r}, relative error {abs(total - inside) / inside:.3e}")
    assert abs(total - inside) <= 1e-12 * inside


# ---- torch tensors and a grid that lives on the device.  torch has to initialise its HIP runtime BEFORE the engine binds the
# device, so these run in a process of their own (tests/sample_worker_gpu.py)
def test_torch_route_and_device_grid():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_SAMPLE_OK" in res.stdout
