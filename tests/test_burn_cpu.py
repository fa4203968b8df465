"""
CPU: the host yardstick of the burn tests (tests/burn_cases.py) on its own reproduces the known answers of the reference's
tests/test_burn.py:81-195, and ``xugrid_amd.burn`` validates its arguments before anything reaches the device.  The
all_touched and line combinations take their (segment, face) pairs from the CPU oracle's ``intersect_edges``, the points
their faces from its ``locate_points``, as tests/test_network_cpu.py does.
"""
import numpy as np
import pytest

from burn_cases import (
    LOCATE_POLYGON_CASES,
    burn_numpy,
    closed,
    line_segments,
    mixed_frame,
    polygon_winner_numpy,
    ragged,
    reference_burn_case,
    ring_segments,
)


@pytest.fixture(scope="module")
def case():
    return reference_burn_case()


@pytest.fixture(scope="module")
def tree(case, oracle):
    tree = oracle.CellTree2d(case["nodes"], case["faces"])
    return tree, oracle.centroids(case["nodes"], case["faces"]), tree.default_tolerance()


def pairs_of(tree, segments):
    segment_index, face_index, _ = tree.intersect_edges(segments)
    return segment_index, face_index


def located(tree, centroids, tol, exterior, interiors, all_touched):
    polygon = ragged([[exterior] + list(interiors)])
    winner = polygon_winner_numpy(centroids, *polygon, tol)
    if all_touched:
        segments, owner = ring_segments(*polygon)
        np.maximum.at(winner, pairs_of(tree, segments)[1], 0)
    return np.nonzero(winner >= 0)[0]


@pytest.mark.parametrize("close", [False, True], ids=["open", "closed"])
@pytest.mark.parametrize("which", range(len(LOCATE_POLYGON_CASES)))
def test_locate_polygon_known_answers(tree, which, close):
    """tests/test_burn.py:81-118, centroids on polygon edges and vertices included; closed and open rings agree."""
    tree, centroids, tol = tree
    exterior, interiors, inside, touched = LOCATE_POLYGON_CASES[which]
    if close:
        exterior, interiors = closed(exterior), [closed(ring) for ring in interiors]
    assert np.array_equal(located(tree, centroids, tol, exterior, interiors, False), inside)
    assert np.array_equal(located(tree, centroids, tol, exterior, interiors, True), touched)


def test_burn_polygons_lines_points_known_answers(case, tree):
    """tests/test_burn.py:120-141"""
    tree, centroids, tol = tree
    assert np.array_equal(burn_numpy(centroids, tol, polygons=case["polygons"]), case["polygons_expected"])
    assert np.array_equal(burn_numpy(centroids, tol, polygons=case["polygons"][:3]), np.ones(9))  # column=None
    lines = case["lines"]
    line_pairs = pairs_of(tree, line_segments(*lines[:2])[0])
    assert np.array_equal(burn_numpy(centroids, tol, -1.0, lines=lines, line_pairs=line_pairs), case["lines_expected"])
    points = case["points"]
    got = burn_numpy(centroids, tol, -1.0, points=points, point_faces=tree.locate_points(points[0]))
    assert np.array_equal(got, case["points_expected"])


def test_open_rings_burn_like_closed_ones(case, tree):
    _, centroids, tol = tree
    coords, ring_offsets, polygon_offsets, values = case["polygons"]
    rings = [coords[a:b - 1] for a, b in zip(ring_offsets[:-1], ring_offsets[1:])]  # (drop the repeated first vertex)
    opened = ragged([[rings[0]], [rings[1]]]) + (values,)
    assert np.array_equal(burn_numpy(centroids, tol, polygons=opened), case["polygons_expected"])


def test_mixed_frame_known_answer(case, tree):
    """tests/test_burn.py:180-191: polygons, then lines, then points."""
    tree, centroids, tol = tree
    polygons, lines, points = mixed_frame(case)
    line_pairs = pairs_of(tree, line_segments(*lines[:2])[0])
    got = burn_numpy(centroids, tol, polygons=polygons, lines=lines, line_pairs=line_pairs, points=points,
                     point_faces=tree.locate_points(points[0]))
    assert np.array_equal(got, case["mixed_expected"])


def test_points_outside_the_mesh_burn_nothing(case, tree):
    tree, centroids, tol = tree
    points = (np.array([[0.5, 0.5], [10.0, 10.0]]), np.array([5.0, 7.0]))
    got = burn_numpy(centroids, tol, -1.0, points=points, point_faces=tree.locate_points(points[0]))
    assert got[0] == 5.0 and (got[1:] == -1.0).all()  # (the reference writes 7.0 into the LAST face: DESIGN section 7)


# ---- argument validation of the public function (raised before the device is touched) -----------------------------------------
class FakeGrid:
    n_face = 9
    device_mesh = object()


def test_argument_validation():
    from xugrid_amd import burn

    square = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    ok = (square, np.array([0, 4]), np.array([0, 1]))
    grid = FakeGrid()
    bad_polygons = [
        (square, np.array([1, 4]), ok[2]),             # does not start at 0
        (square, np.array([0, 3]), ok[2]),             # does not end at n
        (square, np.array([0, 3, 2, 4]), np.array([0, 3])),  # decreases
        (square, ok[1], np.array([0, 2])),             # polygon offsets past the rings
        ok + (np.array([1.0, 2.0]),),                  # two values, one polygon
        (np.array([[0.0, np.nan], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), ok[1], ok[2]),
        (square.ravel(), ok[1], ok[2]),                # not (n, 2)
    ]
    for polygons in bad_polygons:
        with pytest.raises(ValueError):
            burn.burn_vector_geometry(grid, polygons=polygons)
    with pytest.raises(ValueError):
        burn.burn_vector_geometry(grid, lines=(square, np.array([0, 5])))
    with pytest.raises(ValueError):
        burn.burn_vector_geometry(grid, lines=(square, np.array([0, 4]), np.array([1.0, 2.0])))
    with pytest.raises(ValueError):
        burn.burn_vector_geometry(grid, points=(square, np.ones(3)))
    with pytest.raises(ValueError):
        burn.burn_vector_geometry(grid, points=(np.array([[np.inf, 0.0]]),))
    with pytest.raises(TypeError):
        burn.burn_vector_geometry(square, points=(square,))
