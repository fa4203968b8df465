"""
CPU: the numpy yardsticks of the sub-mesh tests (tests/subset_cases.py) against the reference's known answers
(tests/golden/subset_known.json) and their own properties; the argument checks of ``topology_subset`` / ``isel`` / ``sel`` that
need no device; and that every case of tests/test_gpu_subset.py reaches what it was made for.
"""
import numpy as np
import pytest

import subset_cases as sc
import xugrid_amd as xa
from xugrid_amd import connectivity


def grid2d():
    xy, faces = sc.mesh("grid2d")
    return xy, faces, xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


# ---- the yardstick equals the known answers -------------------------------------------------------------------------------
def test_topology_subset_known_answers():
    xy, faces = sc.mesh("grid2d")
    k = sc.known()
    for case in k["topology_subset"]:
        xy_sub, faces_sub, node_index, ids = sc.topology_subset(xy, faces, np.array(case["face_index"]))
        assert np.array_equal(faces_sub, case["faces"])
        assert np.array_equal(xy_sub[:, 0], case["x"]) and np.array_equal(xy_sub[:, 1], case["y"])
        assert np.array_equal(node_index, case["node_index"])
        assert np.array_equal(sc.edge_index(faces, ids), case["edge_index"])
    _, faces_sub, _, _ = sc.topology_subset(xy, faces, np.array(k["reversed"]["face_index"]))
    assert np.array_equal(faces_sub, k["reversed"]["faces"]) and np.array_equal(faces_sub, faces[::-1])
    for identity in (k["identity"]["face_index"], k["identity"]["mask"]):
        xy_sub, faces_sub, node_index, ids = sc.topology_subset(xy, faces, np.array(identity))
        assert np.array_equal(ids, np.arange(4)) and np.array_equal(faces_sub, faces) and np.array_equal(xy_sub, xy)


def test_box_and_inversions_known_answers():
    xy, faces = sc.mesh("grid2d")
    k = sc.known()
    closed, _ = connectivity.close_polygons(faces)
    n = (faces != -1).sum(axis=1)
    centroids = np.array([xy[f[:c]].mean(axis=0) for f, c in zip(faces, n)])  # (squares and triangles: the vertex mean)
    assert np.array_equal(sc.box_faces(centroids, *k["clip_box"]["box"]), k["clip_box"]["faces"])
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    assert np.array_equal(sc.box_faces(centroids, lo[0], lo[1], hi[0], hi[1]), np.arange(4))
    # the half-open rule: an edge exactly on a centroid coordinate
    assert np.array_equal(sc.box_faces(centroids, 0.5, 0.0, 1.5, 1.0), [0])
    assert np.array_equal(sc.box_faces(np.array([[np.nan, 0.5], [0.5, 0.5]]), 0.0, 0.0, 1.0, 1.0), [1])
    for case in k["faces_of_nodes"]:
        assert np.array_equal(sc.faces_of_nodes(faces, case["nodes"]), case["faces"])
    for case in k["faces_of_edges"]:
        assert np.array_equal(sc.faces_of_edges(faces, case["edges"]), case["faces"])


def test_isel_known_answers():
    xy, faces = sc.mesh("grid2d")
    k = sc.known()["isel"]
    for kwargs in ({"node": k["node_identity"]}, {"edge": k["edge_identity"]},
                   {"node": k["node_identity"], "edge": k["edge_identity"], "face": [0, 1, 2, 3]}):
        _, faces_sub, node_index, edge_index, ids = sc.isel(xy, faces, **kwargs)
        assert np.array_equal(faces_sub, faces) and np.array_equal(ids, np.arange(4))
        assert np.array_equal(node_index, np.arange(7)) and np.array_equal(edge_index, np.arange(10))
    with pytest.raises(ValueError, match="invalid topology"):
        sc.isel(xy, faces, node=k["node_invalid"])
    with pytest.raises(ValueError, match="invalid topology"):
        sc.isel(xy, faces, edge=k["edge_invalid"])
    with pytest.raises(ValueError, match="do not align"):
        sc.isel(xy, faces, **k["misaligned"])


# ---- ... and its own properties, on every case ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,selection", sc.CASES)
def test_yardstick_properties(name, selection):
    xy, faces = sc.mesh(name)
    index = sc.selections(name)[selection]
    xy_sub, faces_sub, node_index, ids = sc.topology_subset(xy, faces, index)
    assert np.all(np.diff(node_index) > 0)
    assert np.array_equal(xy_sub, xy[node_index])
    assert faces_sub.shape == (len(ids), faces.shape[1])
    back = np.where(faces_sub == -1, -1, node_index[np.where(faces_sub == -1, 0, faces_sub)] if len(node_index) else -1)
    assert np.array_equal(back, faces[ids])
    # edges are numbered lexicographically and the renumbering is monotone: the sub-mesh's own edges ARE the old ones
    edge_node, _ = sc.host_edges(faces)
    e_index = sc.edge_index(faces, ids)
    sub_edge_node, _ = sc.host_edges(faces_sub)
    assert np.array_equal(sub_edge_node, sc.renumber(edge_node[e_index], node_index))
    # isel by the node index of a subset returns that subset (faces ascending: a node selection stands for them in that order)
    if len(ids) and np.array_equal(sc.faces_of_nodes(faces, node_index), np.sort(ids)):
        _, faces_again, node_again, _, ids_again = sc.isel(xy, faces, node=node_index)
        assert np.array_equal(ids_again, np.sort(ids)) and np.array_equal(node_again, node_index)
        assert np.array_equal(faces_again, sc.topology_subset(xy, faces, np.sort(ids))[1])


def test_isel_by_node_index_of_a_component():
    xy, faces = sc.mesh("disconnected")
    ids = np.arange(len(faces) - 1, len(faces))  # the isolated triangle
    _, faces_sub, node_index, _ = sc.topology_subset(xy, faces, ids)
    e_index = sc.edge_index(faces, ids)
    got = sc.isel(xy, faces, node=node_index)
    assert np.array_equal(got[4], ids) and np.array_equal(got[1], faces_sub) and np.array_equal(got[3], e_index)
    got = sc.isel(xy, faces, edge=e_index, node=node_index, face=ids)
    assert np.array_equal(got[4], ids)


def test_yardstick_refusals():
    xy, faces = sc.mesh("grid2d")
    for bad, error in (([0, 0], ValueError), ([4], IndexError), ([-1], IndexError), ([0.5], TypeError),
                       (np.arange(5), ValueError), (np.ones(3, dtype=bool), ValueError)):
        with pytest.raises(error):
            sc.topology_subset(xy, faces, np.array(bad))


# ---- the cases reach what they were made for --------------------------------------------------------------------------------
def test_cases_reach_their_targets():
    tile = 256 * 8  # items of one tile of the int32 scan
    for name in ("mixed2047", "mixed2048", "mixed2049", "quads2116"):
        xy, faces = sc.mesh(name)
        assert len(xy) > tile  # the scan of the node flags has more than one tile
    assert [len(sc.mesh(n)[1]) for n in ("mixed2047", "mixed2048", "mixed2049")] == [2047, 2048, 2049]  # the mask's scan at the tile
    xy, faces = sc.mesh("quads2116")
    node_index = sc.topology_subset(xy, faces, sc.selections("quads2116")["all_but_one"])[2]
    assert len(xy) == 2116 and len(node_index) == 2115 > tile
    for k in (63, 64, 65, 2048):
        assert len(sc.selections("mixed2049")[f"first{k}"]) == k
    assert np.any(np.diff(sc.selections("mixed2049")["first65"]) < 0)  # unsorted
    xy, faces = sc.mesh("mixed36")
    triangles = sc.selections("mixed36")["triangles_only"]
    assert 0 < len(triangles) < len(faces) and faces.shape[1] == 4
    sub = sc.topology_subset(xy, faces, triangles)[1]
    assert sub.shape[1] == 4 and np.all(sub[:, 3] == -1)  # the width stays although every kept face is a triangle
    xy, faces = sc.mesh("fan70")
    assert np.all(faces[:, 0] == 0) and len(faces) == 70  # one node in 70 selected faces
    xy, faces = sc.mesh("disconnected")
    assert np.unique(faces).size < len(xy)  # unused node ids
    xy, faces = sc.mesh("gon32")
    assert faces.shape[1] == 32
    xy, faces = sc.three_faces_on_one_edge()
    _, face_edge = sc.host_edges(faces)
    assert np.bincount(face_edge[face_edge >= 0]).max() == 3  # an edge with three faces
    for name in sc.MESHES:
        s = sc.selections(name)
        assert np.any(np.diff(s["permuted_subset"]) < 0) or len(s["permuted_subset"]) < 2
        assert s["mask"].dtype == np.bool_ and s["empty"].size == 0


# ---- argument checks that need no device ----------------------------------------------------------------------------------
def test_argument_checks_raise_before_the_device():
    xy, faces, grid = grid2d()
    with pytest.raises(TypeError, match="index should be bool or integer"):
        grid.topology_subset(np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="index size 5 is larger than dimension size: 4"):
        grid.topology_subset(np.arange(5))
    with pytest.raises(ValueError, match="bool index"):
        grid.topology_subset(np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="index contains repeated values; only subsets will result in valid UGRID topology."):
        grid.topology_subset(np.array([1, 1]))
    with pytest.raises(IndexError):
        grid.topology_subset(np.array([4]))
    with pytest.raises(IndexError):
        grid.topology_subset(np.array([-1]))
    with pytest.raises(ValueError, match="do not exist"):
        grid.isel({"mesh2d_nVolumes": np.array([0])})
    with pytest.raises(ValueError, match="do not exist"):
        grid.isel(nowhere=np.array([0]))
    with pytest.raises(TypeError, match="index should be bool or integer"):
        grid.isel({grid.face_dimension: np.array([0.5])})
    with pytest.raises(ValueError, match="return_grid"):
        grid.sel(np.zeros(4), x=[0.5], y=[0.5], return_grid=True)
    with pytest.raises(ValueError, match="return_grid"):
        grid.sel(np.zeros(4), x=slice(None, None), y=0.5, return_grid=True)
