"""
GPU: meshes from cell geometry (xugrid_amd/geometry.py) against the numpy restatements of
tests/geometry_cases.py, which tests/test_geometry_cpu.py pins to the reference's own answers and to ``np.unique``.  Everything
is integers or copied doubles: every comparison is exact, array for array, coordinates bit for bit.
"""
import ctypes
import warnings

import numpy as np
import pytest

import geometry_cases as gc
import xugrid_amd as xa
from geometry_cases import same_bits
from xugrid_amd import _lib, engine, geometry
from xugrid_amd.engine import DeviceArray
from xugrid_amd.ugrid2d import DeviceUgrid2d, RectilinearUgrid2d

pytestmark = pytest.mark.gpu
KINDS = ("host", "device")


def given(kind, a):
    return a if kind == "host" else DeviceArray.from_host(np.ascontiguousarray(a))


def to_numpy(a):
    return a if isinstance(a, np.ndarray) else engine.download(a)


def assert_mesh(grid, xy, faces):
    assert isinstance(grid, DeviceUgrid2d)
    assert grid.n_node == len(xy) and grid.n_face == len(faces)
    got_xy, got_faces = grid.device_mesh.download()
    assert same_bits(got_xy, xy)
    assert got_faces.shape == faces.shape and np.array_equal(got_faces, faces)


# ---- sorted unique rows ---------------------------------------------------------------------------------------------------------
def check_unique(xy, kind="host"):
    rows, index, inverse = xa.unique_xy(given(kind, xy), return_index=True, return_inverse=True)
    if kind == "device":
        assert all(isinstance(a, DeviceArray) for a in (rows, index, inverse))
    rows, index, inverse = (to_numpy(a) for a in (rows, index, inverse))
    e_rows, e_index, e_inverse = gc.unique_rows(xy)
    assert rows.dtype == np.float64 and index.dtype == np.int64 and inverse.dtype == np.int64
    assert same_bits(rows, e_rows)  # (bit for bit: the kept zero is the first occurrence's)
    assert np.array_equal(index, e_index) and np.array_equal(inverse, e_inverse)
    u, u_index, u_inverse = np.unique(xy + 0.0, axis=0, return_index=True, return_inverse=True)
    assert np.array_equal(rows, u.reshape(-1, 2)) and np.array_equal(index, u_index) and np.array_equal(inverse, np.asarray(u_inverse).ravel())
    only = xa.unique_xy(given(kind, xy))
    assert same_bits(to_numpy(only), e_rows)
    return rows, index, inverse


@pytest.mark.parametrize("name", sorted(gc.unique_cases()))
def test_unique_rows(hip, name):
    check_unique(gc.unique_cases()[name])


@pytest.mark.parametrize("name", ("n2049", "zeros", "sign_bit_only"))
def test_unique_rows_of_a_device_array(hip, name):
    check_unique(gc.unique_cases()[name], "device")


def test_unique_rows_keep_the_first_zero(hip):
    rows, index, inverse = check_unique(np.array([[0.0, 1.0], [-0.0, 1.0], [2.0, -0.0], [2.0, 0.0]]))
    assert index.tolist() == [0, 2] and inverse.tolist() == [0, 0, 1, 1]
    assert np.signbit(rows).tolist() == [[False, False], [False, True]]


@pytest.mark.parametrize("name", gc.SLACK_CASES)
def test_unique_rows_with_the_smallest_table(hip, name):
    with engine.option("merge_table_slack", 1):
        check_unique(gc.unique_cases()[name])


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_unique_rows_refuse_non_finite(hip, bad):
    xy = gc.unique_cases()["n257"].copy()
    xy[100, 1] = bad
    with pytest.raises(ValueError, match="1 row"):
        xa.unique_xy(xy)
    with pytest.raises(ValueError, match="expected an \\(n, 2\\) array"):
        xa.unique_xy(np.zeros((4, 3)))


def test_unique_rows_guard_words_and_reproducibility(hip):
    xy = gc.unique_cases()["n2049"]
    e_rows, e_index, e_inverse = gc.unique_rows(xy)
    GUARD, SENTINEL = 8, -7.0e300
    dev = DeviceArray.from_host(xy)
    seen = []
    for _ in range(2):
        unique = geometry.DeviceUnique.of(dev.ptr, len(xy))
        assert (unique.n, unique.n_unique, unique.n_nonfinite) == (len(xy), len(e_rows), 0)
        assert unique.passes_run + unique.passes_skipped == 16
        got = []
        for what, count, dtype in ((0, 2 * len(e_rows), np.float64), (1, len(e_rows), np.int64), (2, len(xy), np.int64)):
            out = DeviceArray.from_host(np.full(count + GUARD, SENTINEL).view(dtype))
            _lib.check(_lib.load().xr_unique_xy_copy_dev(unique._h, what, ctypes.c_void_p(out.ptr)))
            host = out.download()
            assert same_bits(host[count:].view(np.float64), np.full(GUARD, SENTINEL)), "guard words behind the output were written"
            got.append(host[:count])
        assert same_bits(got[0], e_rows.ravel()) and np.array_equal(got[1], e_index) and np.array_equal(got[2], e_inverse)
        seen.append(got)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*seen))


# ---- (N, M, 4) bounds -----------------------------------------------------------------------------------------------------------
def build_from_bounds(xb, yb, kind="host"):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        grid, index = xa.Ugrid2d.from_structured_bounds(given(kind, xb), given(kind, yb), return_index=True)
    return grid, index, [w for w in caught if issubclass(w.category, UserWarning)]


@pytest.mark.parametrize("name", sorted(gc.BOUNDS_CASES))
def test_bounds(hip, name):
    xb, yb = gc.BOUNDS_CASES[name]()
    e = gc.bounds_topology(xb, yb)
    grid, index, caught = build_from_bounds(xb, yb)
    assert_mesh(grid, e["xy"], e["faces"])
    assert isinstance(index, np.ndarray) and index.dtype == np.bool_ and np.array_equal(index, e["index"])
    assert len(caught) == (1 if e["n_invalid"] else 0)
    if e["n_invalid"]:
        assert f"Your structured bounds contain {e['n_invalid']} invalid faces." in str(caught[0].message)
    assert same_bits(xb, gc.BOUNDS_CASES[name]()[0])  # the input is unchanged


def test_bounds_lattice32_answer(hip):
    grid, index, caught = build_from_bounds(*gc.lattice32())
    assert grid.n_face == 4 and grid.n_node == 11 and index.tolist() == [True, False, True, False, True, True]
    assert len(caught) == 1 and "contain 2 invalid faces" in str(caught[0].message)
    assert (grid.face_node_connectivity[:, 3] == -1).tolist() == [False, True, False, False]
    assert grid.n_max_node_per_face == 4
    plain = xa.Ugrid2d.from_structured_bounds(*gc.quad24())  # without the index: the grid alone
    assert isinstance(plain, DeviceUgrid2d) and plain.n_node == 4


def test_bounds_corner_order_does_not_matter(hip):
    grid, index, caught = build_from_bounds(*gc.quad24())
    faces = grid.face_node_connectivity
    assert grid.n_node == 4 and faces.shape == (24, 4) and (faces == faces[0]).all() and index.all() and not caught


def test_bounds_all_invalid_gives_an_empty_grid(hip):
    grid, index, caught = build_from_bounds(*gc.all_invalid())
    assert grid.n_face == 0 and grid.n_node == 0 and not index.any() and len(caught) == 1
    coords, ring_offsets, polygon_offsets = (to_numpy(a) for a in grid.to_polygons())  # the way back of an empty grid
    assert coords.shape == (0, 2) and ring_offsets.tolist() == [0] and polygon_offsets.tolist() == [0]


@pytest.mark.parametrize("name", ("lattice32", "row257"))
def test_bounds_from_device_arrays(hip, name):
    xb, yb = gc.BOUNDS_CASES[name]()
    e = gc.bounds_topology(xb, yb)
    grid, index, _ = build_from_bounds(xb, yb, "device")
    assert_mesh(grid, e["xy"], e["faces"])
    assert isinstance(index, DeviceArray) and index.dtype == np.bool_
    host_index = index.download()
    assert host_index.dtype == np.bool_ and np.array_equal(host_index, e["index"])


def test_bounds_shape_errors(hip):
    xb, yb = gc.lattice_bounds(2, 3)
    with pytest.raises(ValueError, match="Bounds shapes do not match"):
        xa.Ugrid2d.from_structured_bounds(xb, yb[:1])
    with pytest.raises(ValueError, match="Expected \\(N, M, 4\\) bounds"):
        xa.Ugrid2d.from_structured_bounds(xb[..., :3], yb[..., :3])
    bounds = np.column_stack([np.arange(3.0), np.arange(3.0) + 1.0])
    grid, index = xa.Ugrid2d.from_structured_bounds(bounds, bounds[:2], return_index=True)  # 2-D bounds: the path they always took
    assert type(grid) is xa.Ugrid2d and index == slice(None, None) and grid.n_face == 6


def test_bounds_grid_regrids_like_the_host_built_grid(hip):
    xb, yb = gc.lattice_bounds(6, 5, seed=4)
    xb, yb = xb.copy(), yb.copy()
    xb[2, 3, 0] = np.nan
    e = gc.bounds_topology(xb, yb)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        grid = xa.Ugrid2d.from_structured_bounds(xb, yb)
    host = xa.Ugrid2d(e["xy"][:, 0], e["xy"][:, 1], -1, e["faces"])
    edges = lambda lo, hi, n: np.column_stack([np.linspace(lo, hi, n + 1)[:-1], np.linspace(lo, hi, n + 1)[1:]])  # noqa: E731
    raster = xa.Ugrid2d.from_structured_bounds(edges(9.0, 17.0, 7), edges(-3.5, 4.5, 6))
    data = np.random.default_rng(3).normal(size=host.n_face)
    got = xa.OverlapRegridder(grid, raster, method="mean").regrid(data)
    want = xa.OverlapRegridder(host, raster, method="mean").regrid(data)
    assert np.isfinite(want).any() and same_bits(got, want)


# ---- lattices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(gc.LATTICE_CASES))
def test_intervals2d(hip, name, kind):
    ny, nx, x_dec, y_dec = gc.LATTICE_CASES[name]
    x, y = gc.axis_lattice(ny, nx, x_dec, y_dec)
    xy, faces = gc.lattice_mesh(x, y)
    assert_mesh(xa.Ugrid2d.from_structured_intervals2d(given(kind, x), given(kind, y)), xy, faces)
    helper = xa.Ugrid2d._from_intervals_helper(x.ravel(), y.ravel(), nx, ny, "mesh2d")
    assert np.array_equal(faces, helper.face_node_connectivity)


def test_intervals2d_block_edges(hip):
    x, y = gc.lattice_points(3, 258)  # 774 nodes, 514 faces: more than one block of each
    assert_mesh(xa.Ugrid2d.from_structured_intervals2d(x, y), *gc.lattice_mesh(x, y))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("up_up", "down_up", "up_down", "down_down", "wide_down"))
def test_from_structured_2d_centres(hip, name, kind):
    ny, nx, x_dec, y_dec = gc.LATTICE_CASES[name]
    cx, cy = gc.centres(ny, nx, x_dec, y_dec)
    xv, yv = gc.interval_breaks(gc.interval_breaks(cx, 1), 0), gc.interval_breaks(gc.interval_breaks(cy, 1), 0)
    assert same_bits(geometry.interval_breaks(given(kind, cx), 1).download(), gc.interval_breaks(cx, 1))
    assert same_bits(geometry.interval_breaks(given(kind, cy), 0).download(), gc.interval_breaks(cy, 0))
    assert_mesh(xa.Ugrid2d.from_structured(given(kind, cx), given(kind, cy)), *gc.lattice_mesh(xv, yv))


def test_from_structured_1d_centres(hip):
    x, y = np.array([0.5, 1.5, 3.0, 6.0]), np.array([9.0, 7.0, 6.5])
    grid = xa.Ugrid2d.from_structured(x, y, name="raster")
    xv, yv = gc.interval_breaks(x), gc.interval_breaks(y)
    other = xa.Ugrid2d.from_structured_bounds_device(np.column_stack([xv[:-1], xv[1:]]), np.column_stack([yv[1:], yv[:-1]]))
    assert isinstance(grid, RectilinearUgrid2d) and grid.name == "raster"
    assert same_bits(grid.node_coordinates, other.node_coordinates)
    assert np.array_equal(grid.face_node_connectivity, other.face_node_connectivity)
    same = xa.Ugrid2d.from_structured_intervals1d(DeviceArray.from_host(xv), yv)
    assert same_bits(same.node_coordinates, grid.node_coordinates) and np.array_equal(same.face_node_connectivity, grid.face_node_connectivity)


def test_lattice_errors(hip):
    cx, cy = gc.centres(3, 4)
    bad = cx.copy()
    bad[1, 2] = bad[1, 0] - 1.0
    with pytest.raises(ValueError, match="The input coordinate is not monotonic."):
        xa.Ugrid2d.from_structured(bad, cy)
    with pytest.raises(ValueError, match="The input coordinate is not monotonic."):
        xa.Ugrid2d.from_structured(np.array([0.0, 2.0, 1.0]), np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="The input coordinate is not monotonic."):
        xa.Ugrid2d.from_structured(np.array([0.0, np.nan, 1.0]), np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="Cannot derive spacing of 1-sized coordinate: x"):
        xa.Ugrid2d.from_structured(np.array([0.0]), np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="x and y must be 1D or 2D. Found: 3"):
        xa.Ugrid2d.from_structured(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="Dimensions of intervals must be 2D."):
        xa.Ugrid2d.from_structured_intervals2d(np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError, match="Interval shapes must match. Found: x_intervals: \\(3, 4\\), versus y_intervals: \\(4, 3\\)"):
        xa.Ugrid2d.from_structured_intervals2d(np.zeros((3, 4)), np.zeros((4, 3)))


# ---- polygons and lines -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(gc.polygon_cases()))
def test_from_polygons(hip, name, kind):
    coords, ring_offsets = gc.polygon_cases()[name]
    xy, faces = gc.rings_to_faces(coords, ring_offsets)
    assert_mesh(xa.Ugrid2d.from_polygons((given(kind, coords), given(kind, ring_offsets))), xy, faces)
    polygon_offsets = np.arange(len(ring_offsets), dtype=np.int64)
    values = np.zeros(len(ring_offsets) - 1)
    assert_mesh(xa.Ugrid2d.from_polygons((coords, ring_offsets, polygon_offsets, values)), xy, faces)


def test_from_polygons_answers(hip):
    grid = xa.Ugrid2d.from_polygons(gc.polygon_cases()["triangles"])
    assert grid.n_max_node_per_face == 3 and (grid.face_node_connectivity >= 0).all()  # no fill: the shortcut
    grid = xa.Ugrid2d.from_polygons(gc.polygon_cases()["mixed"])
    assert ((grid.face_node_connectivity >= 0).sum(axis=1)).tolist() == [3, 4, 5, 6, 7, 5, 3]
    grid = xa.Ugrid2d.from_polygons(gc.polygon_cases()["duplicates"])
    faces = grid.face_node_connectivity
    assert grid.n_node == 4 and faces[0].tolist() == faces[2].tolist() and sorted(faces[3].tolist()) == sorted(faces[0].tolist())
    assert xa.Ugrid2d.from_polygons(gc.polygon_cases()["none"]).n_face == 0


def test_from_polygons_refusals(hip):
    coords, ring_offsets = gc.polygon_cases()["shared"]
    with pytest.raises(ValueError, match="holes: 1 polygon"):
        xa.Ugrid2d.from_polygons((coords, ring_offsets, np.array([0, 2, 3])))
    opened = coords.copy()
    opened[4, 0] += 1e-9
    with pytest.raises(ValueError, match="1 ring\\(s\\) are not closed"):
        xa.Ugrid2d.from_polygons((opened, ring_offsets))
    with pytest.raises(ValueError, match="1 ring\\(s\\) have fewer than four vertices"):
        xa.Ugrid2d.from_polygons((coords[:13], np.array([0, 5, 10, 13])))
    with pytest.raises(ValueError, match="offsets must ascend"):
        xa.Ugrid2d.from_polygons((coords, np.array([0, 5, 10])))
    with pytest.raises(ValueError, match="offsets must ascend"):
        xa.Ugrid2d.from_polygons((coords, np.array([0, 10, 5, 14])))
    bad = coords.copy()
    bad[1, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        xa.Ugrid2d.from_polygons((bad, ring_offsets))


@pytest.mark.parametrize("kind", KINDS)
def test_polygons_there_and_back(hip, kind):
    xy, faces = gc.rings_to_faces(*gc.polygon_cases()["mixed"])
    shuffled = np.random.default_rng(8).permutation(len(xy))  # a grid whose nodes are NOT in sorted order
    position = np.argsort(shuffled)
    g_xy, g_faces = xy[shuffled], np.where(faces >= 0, position[faces], -1)
    grid = xa.Ugrid2d(g_xy[:, 0], g_xy[:, 1], -1, g_faces) if kind == "host" else xa.Ugrid2d.from_device_arrays(
        DeviceArray.from_host(g_xy), DeviceArray.from_host(g_faces))
    polygons = grid.to_polygons()
    assert all(isinstance(a, np.ndarray if kind == "host" else DeviceArray) for a in polygons)
    e = gc.faces_to_rings(g_xy, g_faces)
    for got, want in zip(polygons, e):
        assert to_numpy(got).dtype == want.dtype and to_numpy(got).tobytes() == want.tobytes()
    assert_mesh(xa.Ugrid2d.from_polygons(polygons), xy, faces)  # the nodes through the sorted order: `faces` again


def test_polygonize_result_meshes(hip):
    bounds = np.column_stack([np.arange(4.0), np.arange(4.0) + 1.0])
    raster = xa.Ugrid2d.from_structured_bounds(bounds, bounds[:3])
    data = np.array([0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 2.0, 1.0, 3.0, 3.0, 2.0, 2.0])
    polygons = xa.polygonize(raster, data)
    assert len(polygons[1]) == len(polygons[2])  # no holes
    grid = xa.Ugrid2d.from_polygons(polygons)
    xy, faces = gc.rings_to_faces(polygons[0], polygons[1])
    assert_mesh(grid, xy, faces)
    assert grid.n_face == len(polygons[3]) == 4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(gc.line_cases()))
def test_from_lines(hip, name, kind):
    coords, line_offsets = gc.line_cases()[name]
    xy, edges = gc.lines_to_edges(coords, line_offsets)
    net = xa.Ugrid1d.from_lines((given(kind, coords), given(kind, line_offsets)))
    assert isinstance(net, xa.Ugrid1d) and same_bits(net.node_coordinates, xy)
    assert np.array_equal(net.edge_node_connectivity, edges)
    if name == "repeated":
        assert [1, 1] in edges.tolist()  # the self loop the reference gives
    if name == "single_vertex":
        assert len(edges) == 1 + 0 + 2


def test_lines_there_and_back(hip):
    xy, edges = gc.lines_to_edges(*gc.line_cases()["shared"])
    shuffled = np.random.default_rng(2).permutation(len(xy))
    position = np.argsort(shuffled)
    net = xa.Ugrid1d(xy[shuffled, 0], xy[shuffled, 1], -1, position[edges])
    coords, line_offsets = net.to_lines()
    assert line_offsets.tolist() == list(range(0, 2 * len(edges) + 1, 2))
    assert same_bits(coords, net.node_coordinates[net.edge_node_connectivity.ravel()])
    back = xa.Ugrid1d.from_lines((coords, line_offsets))
    assert same_bits(back.node_coordinates, xy) and np.array_equal(back.edge_node_connectivity, edges)
    with pytest.raises(ValueError, match="offsets must ascend"):
        xa.Ugrid1d.from_lines((coords, line_offsets[:-1]))


def test_bounding_polygon(hip):
    # a 5 x 5 raster without its centre cell: one polygon, the hole included
    bounds = np.column_stack([np.arange(5.0), np.arange(5.0) + 1.0])
    raster = xa.Ugrid2d.from_structured_bounds(bounds, bounds)
    ring = raster.isel({raster.face_dimension: np.delete(np.arange(25), 12)})
    coords, ring_offsets = ring.bounding_polygon()
    assert len(ring_offsets) == 3 and ring_offsets[0] == 0 and ring_offsets[-1] == len(coords)
    outer, hole = coords[: ring_offsets[1]], coords[ring_offsets[1]:]
    assert (outer.min(), outer.max(), hole.min(), hole.max()) == (0.0, 5.0, 2.0, 3.0)
    assert same_bits(outer[0], outer[-1]) and same_bits(hole[0], hole[-1])
    # two separate parts: 2 x 1 cells and 3 x 2 cells -> the larger one's outline
    xy, faces = gc.lattice_mesh(*gc.axis_lattice(1, 2))
    xy2, faces2 = gc.lattice_mesh(*gc.axis_lattice(2, 3))
    both_xy, both_faces = np.concatenate([xy, xy2 + 100.0]), np.concatenate([faces, faces2 + len(xy)])
    coords, ring_offsets = xa.Ugrid2d(both_xy[:, 0], both_xy[:, 1], -1, both_faces).bounding_polygon()
    assert ring_offsets.tolist() == [0, len(coords)] and coords.min() > 100.0
    moved = xy2 + 100.0
    assert (coords.min(axis=0).tolist(), coords.max(axis=0).tolist()) == (moved.min(axis=0).tolist(), moved.max(axis=0).tolist())
