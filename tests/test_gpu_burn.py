"""
GPU (-m gpu): burning vector geometry into a mesh on the device -- ``burn_vector_geometry`` / ``locate_polygon``
(xugrid_amd/burn.py, csrc/xr_burn.hip).  Known answers of the reference's tests/test_burn.py on its 3 x 3 grid; at size
against the numpy restatement of the polygon rule (tests/burn_cases.py), compared for EQUALITY over all faces -- the same
float64 arithmetic, built without contraction; every strip count the index can be forced to; the order of the polygons in
a strip; empty and degenerate input; a grid and geometry that live on the device only.
"""
import numpy as np
import pytest

import xugrid_amd as xa
from burn_cases import (
    LOCATE_POLYGON_CASES,
    at_size_polygons,
    burn_numpy,
    closed,
    interior_pairs,
    line_segments,
    mixed_frame,
    polygon_winner_numpy,
    ragged,
    reference_burn_case,
    ring_segments,
    touched_winner,
)
from network_cases import raster_quads
from xugrid_amd import burn, meshgen

pytestmark = pytest.mark.gpu

STRIPS = [0, 1, 5000]  # automatic, one strip, far more strips than segments per strip


def default_tolerance(nodes, faces):
    """1e-12 x the largest bounding-box diagonal of a face (ugridbase.py:1165-1170)."""
    xy = np.where((faces >= 0)[..., None], nodes[np.maximum(faces, 0)], np.nan)
    extent = np.nanmax(xy, axis=1) - np.nanmin(xy, axis=1)
    return 1e-12 * np.sqrt(extent[:, 0] * extent[:, 0] + extent[:, 1] * extent[:, 1]).max()


def make_grid(nodes, faces):
    return xa.Ugrid2d(nodes[:, 0], nodes[:, 1], -1, faces)


@pytest.fixture(scope="module")
def case():
    return reference_burn_case()


@pytest.fixture(scope="module")
def grid3(hip, case):
    return make_grid(case["nodes"], case["faces"])


@pytest.fixture(scope="module")
def at_size(hip, oracle):
    """The mesh, the polygons and the yardstick's answers of the tests at size, computed once."""
    nodes, faces = meshgen.triangle_mesh(20_000, 0)
    grid = make_grid(nodes, faces)
    centroids = grid.centroids
    tol = default_tolerance(nodes, faces)
    tree = oracle.CellTree2d(nodes, faces)
    # a triangle wholly inside one face, away from the face's centroid
    home = int(tree.locate_points(np.array([[0.37, 0.61]]))[0])
    corner = nodes[faces[home, 0]]
    centre = centroids[home] + 0.3 * (corner - centroids[home])
    radius = 0.05 * np.hypot(*(corner - centroids[home]))
    tiny = centre + radius * np.array([[1.0, 0.0], [-0.5, 0.8], [-0.5, -0.8]])
    polygons = ragged(at_size_polygons() + [[tiny]])
    n_polygon = polygons[2].size - 1
    values = np.arange(n_polygon, dtype=np.float64) * 1.5 + 3.0
    segments, owner = ring_segments(*polygons)
    segment_index, face_index, _ = tree.intersect_edges(segments)
    assert set(face_index[owner[segment_index] == n_polygon - 1]) == {home}
    winner = polygon_winner_numpy(centroids, *polygons, tol)
    return dict(grid=grid, nodes=nodes, faces=faces, polygons=polygons, values=values, home=home, winner=winner,
                touched=touched_winner(winner, owner, (segment_index, face_index)), n_polygon=n_polygon)


# ---- known answers of the reference's tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("strips", [0, 1, 100_000])
def test_known_answers(grid3, case, xr_option, strips):
    """tests/test_burn.py:81-195 on the 3 x 3 grid, under every strip count."""
    xr_option("burn_strips", strips)
    for exterior, interiors, inside, touched in LOCATE_POLYGON_CASES:
        assert np.array_equal(xa.locate_polygon(grid3, exterior, interiors, all_touched=False), inside)
        assert np.array_equal(xa.locate_polygon(grid3, exterior, interiors, all_touched=True), touched)
        closed_rings = closed(exterior), [closed(ring) for ring in interiors]
        assert np.array_equal(xa.locate_polygon(grid3, *closed_rings), inside)
    assert np.array_equal(xa.burn_vector_geometry(grid3, points=case["points"], fill=-1.0), case["points_expected"])
    assert np.array_equal(xa.burn_vector_geometry(grid3, lines=case["lines"], fill=-1.0), case["lines_expected"])
    assert np.array_equal(xa.burn_vector_geometry(grid3, polygons=case["polygons"]), case["polygons_expected"])
    polygons, lines, points = mixed_frame(case)
    for all_touched in (False, True):
        got = xa.burn_vector_geometry(grid3, polygons=polygons, lines=lines, points=points, all_touched=all_touched)
        assert np.array_equal(got, case["mixed_expected"]), all_touched
        got = xa.burn_vector_geometry(grid3, polygons=case["polygons"][:3], all_touched=all_touched)  # column=None
        assert np.array_equal(got, np.ones(9))


def test_open_rings_and_argument_errors(grid3, case):
    coords, ring_offsets, polygon_offsets, values = case["polygons"]
    rings = [coords[a:b - 1] for a, b in zip(ring_offsets[:-1], ring_offsets[1:])]
    opened = ragged([[rings[0]], [rings[1]]]) + (values,)
    assert np.array_equal(xa.burn_vector_geometry(grid3, polygons=opened), case["polygons_expected"])
    with pytest.raises(ValueError, match="ring_offsets"):
        xa.burn_vector_geometry(grid3, polygons=(coords, ring_offsets[::-1].copy(), polygon_offsets))
    with pytest.raises(ValueError, match="values"):
        xa.burn_vector_geometry(grid3, polygons=(coords, ring_offsets, polygon_offsets, np.ones(3)))
    with pytest.raises(ValueError, match="finite"):
        xa.burn_vector_geometry(grid3, points=(np.array([[np.nan, 0.0]]),))


# ---- at size, exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strips", STRIPS)
def test_at_size_equals_the_numpy_rule(at_size, xr_option, strips):
    """~40 k triangles; 60 random overlapping polygons, a star of 2000 vertices with two holes, a triangle inside one face:
    winner and values equal the brute-force numpy rule on the grid's own centroids, every face compared."""
    xr_option("burn_strips", strips)
    a = at_size
    grid, polygons, values = a["grid"], a["polygons"], a["values"]
    assert grid.n_face > 39_000
    got = burn.polygon_winner(grid, *polygons)
    assert np.array_equal(got, a["winner"])
    assert (a["winner"] >= 0).sum() > 10_000 and np.unique(a["winner"]).size > 30  # (the case is not trivial)
    burned = xa.burn_vector_geometry(grid, polygons=polygons + (values,), fill=-7.0)
    assert np.array_equal(burned, np.where(a["winner"] >= 0, values[np.maximum(a["winner"], 0)], -7.0))

    touched = burn.polygon_winner(grid, *polygons, all_touched=True)
    assert np.array_equal(touched, a["touched"])
    assert (a["touched"] != a["winner"]).sum() > 500
    # the triangle inside one face, off its centroid: burned only when every touched face counts
    last = a["n_polygon"] - 1
    assert got[a["home"]] != last and touched[a["home"]] == last and (touched == last).sum() == 1
    burned = xa.burn_vector_geometry(grid, polygons=polygons + (values,), all_touched=True)
    assert np.array_equal(burned, np.where(a["touched"] >= 0, values[np.maximum(a["touched"], 0)], np.nan), equal_nan=True)


@pytest.mark.parametrize("n_vertex", [250, 256, 257, 65_536, 65_537, 65_792])
def test_extent_at_the_edges_of_its_reduction(hip, n_vertex):
    """The y-range that places the strips is a two-launch reduction over blocks of 256 segments: less than a block, one block,
    one block and a lane, 256 partials, 257 with one segment and with a full block.  A circle, and as the LAST three vertices
    a triangle above it whose apex comes last: only the last segments reach the top of the range, and faces lie under it."""
    nodes, faces = meshgen.triangle_mesh(400, 0)
    grid = make_grid(nodes, faces)
    angle = 2.0 * np.pi * np.arange(n_vertex - 3) / (n_vertex - 3)
    circle = np.column_stack((0.5 + 0.3 * np.cos(angle), 0.45 + 0.3 * np.sin(angle)))
    polygons = ragged([[circle], [np.array([[0.3, 0.8], [0.7, 0.8], [0.5, 0.99]])]])
    assert len(polygons[0]) == n_vertex
    winner = polygon_winner_numpy(grid.centroids, *polygons, default_tolerance(nodes, faces))
    assert (winner == 0).sum() > 100 and (winner == 1).sum() > 10 and (winner == -1).sum() > 100
    values = np.array([3.0, 4.5])
    burned = xa.burn_vector_geometry(grid, polygons=polygons + (values,), fill=-7.0)
    assert np.array_equal(burned, np.where(winner >= 0, values[np.maximum(winner, 0)], -7.0))


@pytest.mark.parametrize("strips", [0, 1, 2, 5, 10, 50, 100_000])
def test_horizontal_edges_through_a_row_of_centroids(hip, xr_option, strips):
    """An 8 x 8 raster of unit cells (centroids at k + 0.5) and two rectangles whose horizontal edges run exactly through
    rows of centroids; with 5 and 10 strips over the extent [0.5, 5.5] those edges also lie exactly ON strip borders.
    Every centroid on an edge is burned, under every strip count."""
    xr_option("burn_strips", strips)
    nodes, faces = raster_quads(np.arange(9.0), np.arange(9.0))
    grid = make_grid(nodes, faces)
    a = [(1.0, 2.5), (6.0, 2.5), (6.0, 5.5), (1.0, 5.5)]
    b = [(2.0, 0.5), (7.0, 0.5), (7.0, 3.5), (2.0, 3.5)]
    polygons = ragged([[a], [b]])
    expected = np.full((8, 8), -1)
    expected[2:6, 1:6] = 0
    expected[0:4, 2:7] = 1
    got = burn.polygon_winner(grid, *polygons)
    assert np.array_equal(got.reshape(8, 8), expected)
    assert np.array_equal(got, polygon_winner_numpy(grid.centroids, *polygons, default_tolerance(nodes, faces)))


# ---- ordering -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strips", [0, 1])
def test_the_highest_polygon_wins(grid3, case, xr_option, strips):
    """70 nested squares about the centroid of face 4 -- more polygon ids in one strip than a wave has lanes -- with
    ascending values: the innermost (highest id) wins where it reaches; reversed, the outermost does everywhere."""
    xr_option("burn_strips", strips)
    half = 1.45 - 0.02 * np.arange(70)
    squares = [[np.array([[-h, -h], [h, -h], [h, h], [-h, h]]) + 1.5] for h in half]
    values = np.arange(70.0)
    tol = default_tolerance(case["nodes"], case["faces"])
    nested = ragged(squares)
    got = xa.burn_vector_geometry(grid3, polygons=nested + (values,))
    assert got[4] == 69.0 and got[3] == 22.0 and got[0] == 22.0
    assert np.array_equal(got, burn_numpy(grid3.centroids, tol, polygons=nested + (values,)))
    assert np.array_equal(xa.burn_vector_geometry(grid3, polygons=nested + (values,)), got)  # (twice the same)
    got = xa.burn_vector_geometry(grid3, polygons=ragged(squares[::-1]) + (values,))
    assert np.array_equal(got, np.full(9, 69.0))


# ---- empty and degenerate input -------------------------------------------------------------------------------------------------
def test_empty_and_degenerate_input(grid3):
    assert np.isnan(xa.burn_vector_geometry(grid3)).all()
    assert np.array_equal(xa.burn_vector_geometry(grid3, fill=-5.0), np.full(9, -5.0))
    none = (np.zeros((0, 2)), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))
    got = xa.burn_vector_geometry(grid3, polygons=none, lines=none[:2], points=(np.zeros((0, 2)),), fill=-5.0)
    assert np.array_equal(got, np.full(9, -5.0))
    # a ring of repeated vertices ON a centroid: every segment has zero length, nothing is burned
    flat = ragged([[np.full((4, 2), 1.5)]])
    for all_touched in (False, True):
        assert np.isnan(xa.burn_vector_geometry(grid3, polygons=flat, all_touched=all_touched)).all()
    # an empty ring and an empty polygon between real ones
    square = [(0.2, 0.2), (0.8, 0.2), (0.8, 0.8), (0.2, 0.8)]
    coords, ring_offsets, polygon_offsets = ragged([[square, np.zeros((0, 2))], [], [np.array(square) + 2.0]])
    got = xa.burn_vector_geometry(grid3, polygons=(coords, ring_offsets, polygon_offsets, np.array([4.0, 5.0, 6.0])), fill=0.0)
    assert np.array_equal(got, [4.0, 0, 0, 0, 0, 0, 0, 0, 6.0])
    # points outside the mesh burn nothing: the last face keeps the fill (the reference writes them into it)
    points = (np.array([[0.5, 0.5], [10.0, 10.0], [-1.0, 2.0]]), np.array([5.0, 7.0, 8.0]))
    assert np.array_equal(xa.burn_vector_geometry(grid3, points=points, fill=-1.0), [5.0] + [-1.0] * 8)
    # a line of a single vertex has no segment
    lines = (np.array([[0.5, 0.5], [1.5, 1.5], [2.5, 1.5]]), np.array([0, 1, 3]), np.array([1.0, 2.0]))
    assert np.array_equal(xa.burn_vector_geometry(grid3, lines=lines, fill=-1.0), [-1, -1, -1, -1, 2, 2, -1, -1, -1])


@pytest.mark.parametrize("strips", [0, 1])
def test_mixed_mesh_with_padding(hip, oracle, xr_option, strips):
    """Triangles and quadrilaterals in one (F, 4) connectivity, -1 behind the triangles' corners; polygons, lines, points."""
    xr_option("burn_strips", strips)
    nodes, faces = meshgen.mixed_mesh(900, 3)
    assert (faces[:, 3] < 0).any() and (faces[:, 3] >= 0).any()
    grid = make_grid(nodes, faces)
    tree = oracle.CellTree2d(nodes, faces)
    tol = default_tolerance(nodes, faces)
    polygons = ragged(at_size_polygons(11)[:12])
    polygons += (np.arange(12.0),)
    rng = np.random.default_rng(5)
    lines = (rng.uniform(0.0, 1.0, (40, 2)), np.array([0, 7, 7, 25, 40]), np.array([100.0, 101.0, 102.0, 103.0]))
    points = (rng.uniform(-0.1, 1.1, (50, 2)), 200.0 + np.arange(50.0))
    segments, _ = ring_segments(*polygons[:3])
    polygon_pairs = interior_pairs(nodes, faces, segments, tree.intersect_edges(segments)[:2])
    line_pairs = tree.intersect_edges(line_segments(*lines[:2])[0])[:2]
    point_faces = tree.locate_points(points[0])
    assert (point_faces < 0).any()
    for all_touched in (False, True):
        expected = burn_numpy(grid.centroids, tol, -1.0, polygons, polygon_pairs if all_touched else None, lines, line_pairs,
                              points, point_faces)
        got = xa.burn_vector_geometry(grid, polygons=polygons, lines=lines, points=points, fill=-1.0, all_touched=all_touched)
        assert np.array_equal(got, expected), all_touched


# ---- a grid and geometry on the device only.  torch has to initialise its HIP runtime BEFORE the engine binds the device, so
# this runs in a process of its own (tests/burn_worker_gpu.py)
def test_device_grid_and_device_geometry():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "burn_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_BURN_OK" in res.stdout
