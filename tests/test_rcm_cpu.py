"""
CPU: the yardsticks of the renumbering tests against each other and against scipy (tests/rcm_cases.py).  ``sequential`` (scipy's
loop with a stable argsort) equals ``level_form`` (the rule of the device kernels) on every fixture, tie-heavy ones included;
``sequential`` equals scipy itself wherever scipy's answer does not depend on its tie order -- a precondition this module checks
on the fixture before it compares.
"""
import numpy as np
import pytest
from scipy.sparse.csgraph import reverse_cuthill_mckee as scipy_rcm

import graph_cases as gc
import rcm_cases as rc
from network_cases import raster_quads


def eared(n_points=300, seed=0):
    return rc.with_ear(*rc.delaunay(n_points, seed))


def eared_plus_isolated():
    return rc.join(eared(), rc.isolated_triangles(1))


def many_components():
    return rc.join(rc.delaunay(60, 1), rc.isolated_triangles(40), rc.delaunay(45, 2))


TIE_FREE = {
    "eared_delaunay": lambda: rc.face_graph(eared()[1]),
    "eared_delaunay_plus_isolated": lambda: rc.face_graph(eared_plus_isolated()[1]),
    "eared_delaunay_5000": lambda: rc.face_graph(eared(5000, 3)[1]),
}
TIE_HEAVY = {
    "chain": lambda: gc.chain(5),
    "delaunay": lambda: rc.face_graph(rc.delaunay(300, 0)[1]),
    "raster": lambda: rc.face_graph(raster_quads(np.arange(10.0), np.arange(8.0))[1]),
    "mixed": lambda: rc.face_graph(gc.topology_mesh("mixed900")[1]),
    "components": lambda: rc.face_graph(many_components()[1]),
    "isolated": lambda: rc.face_graph(rc.isolated_triangles(7)[1]),
    "star": lambda: rc.hub_graph(300),
    "hub_with_tails": lambda: rc.hub_graph(300, tails=[(5, 1), (9, 2), (200, 1), (299, 3)], diagonal=[0, 7]),
}


@pytest.mark.parametrize("name", list(TIE_FREE) + list(TIE_HEAVY))
def test_sequential_equals_level_form(name):
    A = {**TIE_FREE, **TIE_HEAVY}[name]()
    order, widths = rc.level_form(A)
    assert np.array_equal(rc.sequential(A), order)
    assert sum(widths) == A.shape[0] and np.array_equal(np.sort(order), np.arange(A.shape[0]))


@pytest.mark.parametrize("name", list(TIE_FREE))
def test_sequential_equals_scipy_where_no_seed_is_tied(name):
    A = TIE_FREE[name]()
    assert rc.seed_ties(A) == 0, "the fixture must leave scipy no choice of seed"
    assert np.array_equal(rc.sequential(A), scipy_rcm(A, symmetric_mode=True))


def test_plain_delaunay_has_tied_seeds():
    assert rc.seed_ties(TIE_HEAVY["delaunay"]()) > 0


def test_known_answers():
    assert np.array_equal(rc.sequential(gc.chain(5)), [4, 3, 2, 1, 0])
    A = rc.hub_graph(3, diagonal=[2])  # degrees: hub 3, leaves 1, 3 (diagonal), 1 -> seed 1, hub, then leaves 3, 2
    assert np.array_equal(rc.degrees(A), [3, 1, 3, 1])
    assert np.array_equal(rc.sequential(A), [2, 3, 0, 1])


def test_face_graph_is_the_grid_adjacency():
    xy, faces = gc.topology_mesh("mixed900")
    host = gc.host_topology(faces, len(xy))["face_face"].tocsr()
    host.sort_indices()
    A = rc.face_graph(faces)
    assert np.array_equal(host.indptr, A.indptr) and np.array_equal(host.indices, A.indices)
