"""
CPU: the numpy restatement of the part-label rule (tests/partlabel_cases.py; include/xugrid_amd.h: xr_graph_partition_dev) keeps
its own promises -- the cut never rises, balanced seeds stay balanced, the same input gives the same labels, the curve key is
the Hilbert index -- and the fixtures of test_gpu_partlabel.py have the properties they are used for.  The argument checks of
``label_partitions`` are exercised here too: they need no device.
"""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import partlabel_cases as pc
import rcm_cases as rc
import xugrid_amd as xa


def delaunay_case(n_points, P, w=None):
    xy, faces = rc.delaunay(n_points, 0)
    A = rc.face_graph(faces)
    return A, pc.face_centroids(xy, faces), pc.label(A, pc.face_centroids(xy, faces), P, w)


# ---- the curve key
def test_hilbert_corners():
    N = pc.CELLS - 1
    d = pc.hilbert_index([0, N, N, 0], [0, 0, N, N])
    assert d.tolist() == [0, 2**32 - 1, (2**33 - 2) // 3, (2**32 - 1) // 3]  # first, last, the ends of the second and first third


def test_hilbert_block_of_sixteen():
    # the order-2 curve, written out: position along the curve -> (x, y)
    walk = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 2), (0, 3), (1, 3), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (3, 1), (2, 1), (2, 0), (3, 0)]
    x, y = np.array(walk).T
    assert pc.hilbert_index(x, y).tolist() == list(range(16))
    assert np.all(np.abs(np.diff(x)) + np.abs(np.diff(y)) == 1)  # a curve: consecutive cells share a side


def test_cells_clamp_and_degenerate_extent():
    assert pc.cells([[0.0, 0.0], [1.0, 0.5], [0.5, 1.0]]).tolist() == [[0, 0], [65535, 32768], [32768, 65535]]
    assert pc.cells([[2.0, 3.0]] * 4).tolist() == [[0, 0]] * 4  # no extent at all: every key ties
    assert pc.cells([[1.0, 0.0], [1.0, 2.0]]).tolist() == [[0, 0], [0, 65535]]  # a vertical line


# ---- the rule's promises
CASES = [(300, 4, None), (40, 2, None), (60, 4, None), (300, 4, "half"), (2000, 7, None)]


@pytest.mark.parametrize("n_points,P,weights", CASES)
def test_cut_never_rises_and_balance_holds(n_points, P, weights):
    xy, faces = rc.delaunay(n_points, 0)
    A, c = rc.face_graph(faces), pc.face_centroids(xy, faces)
    w = pc.half_weights(len(faces)) if weights else None
    start = pc.seed(c, w, P)
    labels, k = pc.refine(A, start, w, P)
    assert all(b <= a for a, b in zip(k["cuts"], k["cuts"][1:]))
    assert [a - b for a, b in zip(k["cuts"], k["cuts"][1:])] == k["gains"]  # movers are independent: a move lowers the cut by its gain
    used = pc.used_weights(w, len(faces))
    Lmin, L = pc.bounds(int(used.sum()), P)
    W0, W1 = pc.part_weights(start, used, P), pc.part_weights(labels, used, P)
    assert W0.min() >= Lmin and W0.max() <= L  # the seed is within the bounds ...
    assert W1.min() >= Lmin and W1.max() <= L  # ... and so is the result
    assert k["rounds"] <= pc.MAX_ROUNDS and k["cuts"][-1] == pc.cut(A, labels)
    again, k2 = pc.refine(A, pc.seed(c, w, P), w, P)
    assert np.array_equal(again, labels) and k2 == k


def test_unit_seed_sizes_differ_by_at_most_one():
    for n, P in ((582, 4), (67, 2), (15, 3), (1000, 7), (9, 9)):
        xy = np.random.default_rng(n).random((n, 2))
        counts = np.bincount(pc.seed(xy, None, P), minlength=P)
        assert counts.min() >= 1 and counts.max() - counts.min() <= 1


# ---- the fixtures' preconditions
def test_reference_behaviours():
    xy, faces = pc.generate_mesh_2d(5, 3)
    A, c = rc.face_graph(faces), pc.face_centroids(xy, faces)
    assert np.bincount(pc.label(A, c, 3)[0]).tolist() == [5, 5, 5]
    assert np.bincount(pc.label(A, c, 3, pc.half_weights(15))[0]).tolist() == [4, 7, 4]
    xy, edges = pc.generate_mesh_1d(6)
    A, c = pc.edge_graph(edges), pc.edge_midpoints(xy, edges)
    assert A.nnz == 10 and np.array_equal(A.toarray(), pc.chain_graph(6)[0].toarray())
    assert np.bincount(pc.label(A, c, 3)[0]).tolist() == [2, 2, 2]
    assert np.bincount(pc.label(A, c, 3, pc.half_weights(6))[0]).tolist() == [2, 1, 3]


def test_delaunay_300_takes_several_rounds_to_a_lower_cut():
    A, c, (labels, k) = delaunay_case(300, 4)
    assert A.shape[0] == 582
    assert k["rounds"] == 4 and k["accepted"] == [11, 10, 2, 0]
    assert (k["cuts"][0], k["cuts"][-1]) == (74, 47)


@pytest.mark.parametrize("n_points,P,first,uncapped_first", [(40, 2, 1, 2), (60, 4, 2, 8)])
def test_budgets_reject_movers(n_points, P, first, uncapped_first):
    A, c, (labels, k) = delaunay_case(n_points, P)
    assert sum(k["rejected"]) > 0
    free = pc.refine(A, pc.seed(c, None, P), None, P, capped=False)[1]
    assert k["accepted"][0] == first and free["accepted"][0] == uncapped_first


def test_hub_network_has_rows_beyond_a_thread():
    xy, edges = pc.hub_network()
    A = pc.edge_graph(edges)
    assert np.diff(A.indptr).max() == 40 and (np.diff(A.indptr) > 32).sum() == 40
    labels, k = pc.label(A, pc.edge_midpoints(xy, edges), 4)
    assert sorted(np.unique(labels)) == [0, 1, 2, 3]


# ---- argument checks of the public functions: before anything touches a device
def grids():
    xy, faces = pc.generate_mesh_2d(5, 3)
    nxy, edges = pc.generate_mesh_1d(6)
    return [(xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces), 15), (xa.Ugrid1d(nxy[:, 0], nxy[:, 1], -1, edges), 6)]


def test_weight_errors_are_the_references():
    for grid, n in grids():
        with pytest.raises(ValueError, match="Wrong shape on weights. Expected a 1D array with"):
            grid.label_partitions(3, weights=np.ones(n + 10, dtype=int))
        with pytest.raises(ValueError, match="Wrong shape on weights."):
            grid.label_partitions(3, weights=np.ones((n, 1), dtype=int))
        with pytest.raises(TypeError, match="Wrong type on weights. Expected an integer array, received: float64"):
            grid.label_partitions(3, weights=np.ones(n, dtype=float))
        with pytest.raises(ValueError, match="Wrong values on weights. Weights should be greater or equal to zero."):
            grid.label_partitions(3, weights=-np.ones(n, dtype=int))
        with pytest.raises(ValueError, match="Wrong shape on weights."):
            grid.partition(3, weights=np.ones(n + 1, dtype=int))


def test_n_part_errors():
    for grid, n in grids():
        for bad in (0, -2, n + 1):
            with pytest.raises(ValueError, match="n_part"):
                grid.label_partitions(bad)
        with pytest.raises(TypeError):
            grid.label_partitions(2.5)
        with pytest.raises(ValueError, match="does not fit in int64"):
            grid.label_partitions(3, weights=np.full(n, 2**55, dtype=np.int64))
        with pytest.raises(ValueError, match="does not fit in int64"):
            grid.label_partitions(3, weights=np.full(n, 2**63, dtype=np.uint64))
    A, xy = pc.chain_graph(5)
    with pytest.raises(ValueError, match="n_part"):
        xa.label_partitions(A, xy, 6)
    with pytest.raises(ValueError, match="Wrong shape on weights."):
        xa.label_partitions(A, xy, 2, weights=[1, 1, 1])
    with pytest.raises(ValueError, match="square"):
        xa.label_partitions(csr_matrix((3, 4)), xy[:3], 2)


def test_nothing_to_label_launches_nothing():
    labels = xa.label_partitions(csr_matrix((0, 0)), np.zeros((0, 2)), 3)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int64 and labels.shape == (0,)
    grid = xa.Ugrid1d(np.zeros(2), np.zeros(2), -1, np.zeros((0, 2), dtype=np.int64))
    assert grid.label_partitions(2).shape == (0,)
