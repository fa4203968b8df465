"""
CPU: the host side of the sampling methods -- argument validation before any device call, ``sel``'s dispatch on its
indexer types, the section arithmetic on the reference's known answers, and the host yardsticks of the GPU tests checked
against each other.
"""
import numpy as np
import pytest

import xugrid_amd as xa
from network_cases import line_selection_cases
from sample_cases import brute_nearest, grid2d_arrays, kdtree_nearest, length_inside_hull, section_numpy
from xugrid_amd import sample


def grid2d():
    xy, faces = grid2d_arrays()
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


def test_sel_points_argument_errors():
    """tests/test_ugrid2d.py:835-846: the reference's messages, raised before the device is touched."""
    grid, data = grid2d(), np.arange(4.0)
    x, y = [0.5, 1.5], [0.5, 1.25]
    with pytest.raises(ValueError, match="method must be one of"):
        grid.sel_points(data, x, y, method="nothing")
    with pytest.raises(ValueError, match="out_of_bounds must be one of"):
        grid.sel_points(data, x, y, out_of_bounds="nothing")
    with pytest.raises(ValueError, match="shape of x does not match shape of y"):
        grid.sel_points(data, [0.5, 1.5], [0.5])
    with pytest.raises(ValueError, match="x and y must be 1d"):
        grid.sel_points(data, [x], [y])
    with pytest.raises(TypeError, match="fill_value must be a scalar"):
        grid.sel_points(data, x, y, fill_value=lambda v: v)
    with pytest.raises(TypeError, match="fill_value must be a scalar"):
        grid.sel_points(data, x, y, fill_value=np.zeros(2))
    with pytest.raises(ValueError, match="Expected one of"):
        grid.sel_points(data, x, y, dim="nothing")


def test_line_argument_errors():
    grid, data = grid2d(), np.arange(4.0)
    with pytest.raises(ValueError, match="Start and end coordinate pairs must have length two"):  # test_ugrid2d.py:1147-1151
        grid.intersect_line(data, start=(0.0, 0.0, 0.0), end=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="at least two vertices"):
        grid.intersect_linestring(data, [[0.0, 0.0]])
    with pytest.raises(ValueError, match="at least two vertices"):
        grid.intersect_linestring(data, np.zeros((3, 3)))
    # tests/test_ugrid2d.py:1112-1118
    with pytest.raises(ValueError, match="If x is a slice without steps"):
        grid.sel(data, x=slice(None, None), y=[0.25, 0.75])
    with pytest.raises(ValueError, match="If x is a slice without steps"):
        grid.sel(data, x=slice(None, None), y=slice(0.25, 1.0, 0.25))
    with pytest.raises(ValueError, match="If y is a slice without steps"):
        grid.sel(data, x=[0.25, 0.75], y=slice(None, None))
    with pytest.raises(ValueError, match="take data on the faces"):
        grid.sel(np.arange(7.0), x=slice(None, None), y=0.5, dim="node")


def test_validate_indexer_and_dispatch():
    """tests/test_ugrid2d.py:995-1027 and the dispatch of ugridbase.py:1492-1505."""
    v = sample.validate_indexer
    with pytest.raises(ValueError, match="slice stop should be larger than slice start"):
        v(slice(2, 0))
    with pytest.raises(ValueError, match="step should be None"):
        v(slice(None, 2, 1))
    with pytest.raises(ValueError, match="step should be None"):
        v(slice(0, None, 1))
    with pytest.raises(TypeError, match="Invalid indexer type"):
        v((0, 1, 2))
    with pytest.raises(ValueError, match="index should be 0d or 1d"):
        v(np.zeros((2, 2)))
    assert v(slice(None, None)) == slice(None, None) and v(slice(0, 2)) == slice(0, 2)
    assert np.allclose(v(slice(0, 2, 1)), [0, 1])
    assert np.allclose(v(slice(0.4, 1.5, 0.4)), [0.4, 0.8, 1.2])
    for scalar in (1, 1.0, np.float64(1.0), np.int64(1)):
        out = v(scalar)
        assert isinstance(out, np.ndarray) and np.allclose(out, [1])
    assert np.allclose(v([1, 2]), [1, 2])

    a, s = np.array([0.5]), slice(None, None)
    assert sample.sel_kind(s, s) == "box" and sample.sel_kind(s, a) == "yline"
    assert sample.sel_kind(a, s) == "xline" and sample.sel_kind(a, a) == "points"
    with pytest.raises(TypeError, match="Invalid indexer types"):
        sample.sel_kind(a, "y")


def test_section_arithmetic_known_answers():
    """tests/test_ugrid2d.py:1153-1187 and :1120-1145: the pieces of the lines written out by hand."""
    _, _, (diagonal, bend, along_x, along_y) = line_selection_cases()
    pieces = {
        "diagonal": (np.array([[[0.0, 0.0], [1.0, 1.0]], [[1.0, 1.0], [1.5, 1.5]]]), [0, 0]),
        "bend": (np.array([[[0.5, 0.5], [1.0, 0.5]], [[1.0, 0.5], [1.5, 0.5]], [[1.5, 0.5], [1.5, 1.0]],
                           [[1.5, 1.0], [1.5, 1.5]]]), [0, 0, 1, 1]),
        "along_x": (np.array([[[0.0, 0.5], [1.0, 0.5]], [[1.0, 0.5], [2.0, 0.5]]]), [0, 0]),
        "along_y": (np.array([[[0.5, 0.0], [0.5, 1.0]], [[0.5, 1.0], [0.5, 1.5]]]), [0, 0]),
    }
    for name, case in (("diagonal", diagonal), ("bend", bend), ("along_x", along_x), ("along_y", along_y)):
        segments, _, x, y, s = case
        mid, got_s = section_numpy(*pieces[name], segments)
        assert np.allclose(mid[:, 0], x) and np.allclose(mid[:, 1], y) and np.allclose(got_s, s), name
    # the reversed diagonal measures from the other end
    mid, s = section_numpy(pieces["diagonal"][0][:, ::-1], [0, 0], diagonal[0][:, ::-1])
    r2 = np.sqrt(2.0)
    assert np.allclose(s, [1.5 * r2, 0.75 * r2]) and np.array_equal(np.argsort(s, kind="stable"), [1, 0])


def test_yardsticks_agree():
    rng = np.random.default_rng(3)
    points, queries = rng.random((3000, 2)), rng.uniform(-0.2, 1.2, (2000, 2))
    for md in (np.inf, 0.02):
        kd, unique = kdtree_nearest(points, queries, md)
        assert unique.all()
        assert np.array_equal(brute_nearest(points, queries, md), kd)
    # scipy's distance_upper_bound is exclusive (a 3-4-5 triangle: the distance is exactly 5.0)
    p, q = np.array([[3.0, 4.0], [30.0, 40.0]]), np.array([[0.0, 0.0]])
    for yardstick in (lambda md: brute_nearest(p, q, md), lambda md: kdtree_nearest(p, q, md)[0]):
        assert yardstick(5.0)[0] == -1 and yardstick(np.nextafter(5.0, 6.0))[0] == 0
    # ties: the brute-force yardstick takes the lowest id, and marks of uniqueness catch them
    p = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    assert brute_nearest(p[::-1], [[0.0, 0.0]])[0] == 0 and not kdtree_nearest(p, [[0.0, 0.0]])[1][0]
    assert brute_nearest(p, [[np.nan, 0.0], [0.9, 0.0]]).tolist() == [-1, 0]


def test_length_inside_hull():
    square = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5]])
    assert np.isclose(length_inside_hull(square, [[[-1.0, -1.0], [2.0, 2.0]]]), np.sqrt(2.0), rtol=1e-15)
    assert np.isclose(length_inside_hull(square, [[[0.25, 0.5], [0.75, 0.5]], [[0.75, 0.5], [3.0, 0.5]]]), 0.75, rtol=1e-15)
    assert length_inside_hull(square, [[[2.0, 0.0], [3.0, 1.0]]]) == 0.0


def test_grids_expose_the_sampling_methods_and_drop_their_indices():
    grid = grid2d()
    for name in ("locate_nearest_node", "locate_nearest_edge", "locate_nearest_face", "sel_points", "sel", "intersect_line",
                 "intersect_linestring", "intersect_edges", "locate_bounding_box"):
        assert callable(getattr(grid, name)), name
    marker = object()
    grid.__dict__["_sample_cache"] = marker
    grid.drop_device_caches()
    assert "_sample_cache" not in grid.__dict__
    grid.__dict__["_sample_cache"] = marker
    grid.node_x = grid.node_x + 1.0  # (new coordinates: the indices built from the old ones go)
    assert "_sample_cache" not in grid.__dict__
    net = xa.Ugrid1d(np.array([0.0, 1.0, 2.0]), np.zeros(3), -1, np.array([[0, 1], [1, 2]]))
    assert callable(net.locate_nearest_node) and callable(net.locate_nearest_edge)
    net.__dict__["_sample_cache"] = marker
    net.drop_device_caches()
    assert "_sample_cache" not in net.__dict__
