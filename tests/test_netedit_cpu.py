"""
CPU: the yardsticks of the network edits and the host side of their public interface -- every ``*_ref`` of tests/netedit_cases.py
against the reference's own output (tests/golden/netedit_known.json), the refine cases' vertices exactly on their edges, and the
refusals that must not need a device.
"""
import json
import os
import re

import numpy as np
import pytest

import netedit_cases as nc
import xugrid_amd as xa
from xugrid_amd import Ugrid1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "netedit_known.json")))


def grid_of(xy, edges):
    return Ugrid1d(xy[:, 0], xy[:, 1], -1, edges)


def test_the_goldens_cover_the_cases():
    assert set(KNOWN["subset"]) == set(nc.SUBSET_CASES)
    assert set(KNOWN["refine"]) == set(nc.REFINE_CASES)
    assert set(KNOWN["merge"]) == set(nc.MERGE_CASES) - {"nan_node"}


@pytest.mark.parametrize("name", sorted(nc.SUBSET_CASES))
def test_subset_ref_reproduces_the_reference(name):
    xy, edges, index = nc.SUBSET_CASES[name]()
    sub_xy, sub_edges, node_index = nc.subset_ref(xy, edges, index)
    known = KNOWN["subset"][name]
    assert nc.equals_known(sub_xy, known["xy"]) and nc.equals_known(sub_edges, known["edges"])
    assert nc.equals_known(node_index, known["node_index"])


def test_remove_self_loops_ref_reproduces_the_reference():
    sub_xy, sub_edges, node_index, edge_index = nc.remove_self_loops_ref(*nc.self_loops())
    known = KNOWN["remove_self_loops"]
    assert nc.equals_known(sub_xy, known["xy"]) and nc.equals_known(sub_edges, known["edges"])
    assert node_index.tolist() == [0, 1, 2, 3, 4, 5, 7] and edge_index.tolist() == [1, 2, 4, 5, 6, 7]


@pytest.mark.parametrize("name", sorted(nc.REFINE_CASES))
def test_refine_ref_reproduces_the_reference(name):
    xy, edges, vertices, tolerance, _ = nc.REFINE_CASES[name]()
    got = nc.refine_ref(xy, edges, vertices, tolerance)
    known = KNOWN["refine"][name]
    for key in ("xy", "edges", "node_index"):
        assert nc.equals_known(got[key], known[key]), key
    # parent_edge is an addition: every new edge lies between the ends of its parent in the scan's order
    assert np.array_equal(np.bincount(got["parent_edge"], minlength=len(edges)), 1 + np.bincount(
        nc.locate_ref(xy, edges, got["xy"][len(xy):], tolerance), minlength=len(edges)))
    assert np.all(np.diff(got["parent_edge"]) >= 0)


def test_refine_ref_reproduces_the_reference_test():
    t = KNOWN["reference_test"]
    xy, edges, vertices = (np.array(t[k]) for k in ("xy", "edges", "vertices"))
    got = nc.refine_ref(xy, edges, vertices, 0.0)
    assert got["edges"].tolist() == t["expected_edges"] and got["node_index"].tolist() == t["expected_node_index"]
    got = nc.refine_ref(xy, edges, vertices + t["offset"], t["offset_tolerance"])
    assert got["edges"].tolist() == t["expected_edges"] and got["node_index"].tolist() == t["expected_node_index"]
    assert nc.KNOWN_EDGES == t["expected_edges"] and nc.KNOWN_NODE_INDEX == t["expected_node_index"]


@pytest.mark.parametrize("name", sorted(nc.REFINE_CASES))
def test_refine_vertices_lie_exactly_on_their_edges(name):
    """What keeps the GPU comparison from hinging on rounding: at tolerance 0.0 the rule finds every vertex."""
    xy, edges, vertices, tolerance, exact = nc.REFINE_CASES[name]()
    found = nc.locate_ref(xy, edges, vertices, 0.0)
    if exact:
        assert (found >= 0).all() and np.array_equal(found, nc.locate_ref(xy, edges, vertices, tolerance))
    else:  # the two cases that are about the tolerance: some vertex is found only with it
        assert (found == -1).any() and (nc.locate_ref(xy, edges, vertices, tolerance) >= 0).all()


def test_the_diagonal_cases_reach_the_wave_walk():
    """The long edge crosses every row of cells: more than the 8 a lane walks alone, and in the wide case more than the 64 lanes."""
    rows = {name: nc.grid_rows(nc.REFINE_CASES[name]()[2])[1] for name in ("diagonal", "diagonal_wide")}
    assert 8 < rows["diagonal"] <= 64 < rows["diagonal_wide"], rows
    for name in rows:
        xy, edges, vertices, _, _ = nc.REFINE_CASES[name]()
        assert (nc.locate_ref(xy, edges, vertices, 0.0) == 1000).all() and 1000 % 64 != 0  # (the long edge is not its wave's lane 0)


@pytest.mark.parametrize("name", sorted(set(nc.MERGE_CASES) - {"nan_node"}))
def test_merge_ref_reproduces_the_reference(name):
    got = nc.merge_ref(nc.MERGE_CASES[name]())
    known = KNOWN["merge"][name]
    for key in ("xy", "edges", "node_inverse"):
        assert nc.equals_known(got[key], known[key]), key
    for key in ("node_index", "edge_index"):
        assert len(got[key]) == len(known[key]) and all(nc.equals_known(a, k) for a, k in zip(got[key], known[key])), key


def test_merge_ref_keeps_a_nan_node_twice_and_the_first_orientation():
    got = nc.merge_ref(nc.MERGE_CASES["nan_node"]())
    assert len(got["xy"]) == 4 and np.isnan(got["xy"][:, 0]).sum() == 2
    assert got["edges"].tolist() == [[0, 1], [0, 2], [0, 3]]
    parts = nc.MERGE_CASES["overlapping"]()
    got = nc.merge_ref(parts)
    chain_edges = nc.chain(60, seed=40)[1]
    assert got["edges"][:19].tolist() == chain_edges[:19].tolist()  # (the shared edges 14 .. 18 in the first part's direction)
    assert (got["edges"][19:, 0] > got["edges"][19:, 1]).all()  # (the later parts' own edges as they hold them: reversed)
    assert np.array_equal(np.unique(np.sort(got["edges"], axis=1), axis=0), chain_edges)
    assert [len(i) for i in got["edge_index"]] == [19, 20, 20]


def test_header_declares_the_network_symbols():
    from xugrid_amd import _lib

    header = open(os.path.join(ROOT, "include", "xugrid_amd.h")).read()
    declared = set(re.findall(r"\bint (xr_net(?:work|edit)_\w+)\(", header)) - {"xr_network_graph_dev"}  # (of the network fill)
    assert declared == {"xr_network_subset_dev", "xr_network_edges_of_nodes_dev", "xr_network_box_edges_dev", "xr_network_nonloop_edges_dev",
                        "xr_network_merge_dev", "xr_network_refine_dev", "xr_netedit_info", "xr_netedit_copy_dev", "xr_netedit_part_info",
                        "xr_netedit_part_copy_dev", "xr_netedit_destroy"}
    assert declared <= set(_lib.SIGNATURES)


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------
def test_index_refusals():
    grid = grid_of(*nc.chain(12))
    with pytest.raises(ValueError, match="repeated"):
        grid.topology_subset([1, 2, 1])
    for bad in ([0, 11], [-1, 3]):
        with pytest.raises(IndexError):
            grid.topology_subset(bad)
    with pytest.raises(ValueError, match="larger than dimension size"):
        grid.topology_subset(np.zeros(12, dtype=np.int64))
    with pytest.raises(TypeError):
        grid.topology_subset(np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="1d"):
        grid.topology_subset(np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="dimension's size"):
        grid.topology_subset(np.ones(10, dtype=bool))
    with pytest.raises(ValueError, match="do not exist"):
        grid.isel({"network1d_nFaces": [0]})
    with pytest.raises(ValueError, match="both keyword and positional"):
        grid.isel({grid.edge_dimension: [0]}, **{grid.node_dimension: [0]})


def test_sel_refusals():
    grid = grid_of(*nc.chain(12))
    with pytest.raises(ValueError, match="does not support steps"):
        grid.sel(x=slice(0.0, 5.0, 2.0))
    with pytest.raises(ValueError, match="only supports slice"):
        grid.sel(x=3.0)
    with pytest.raises(ValueError, match="smaller than slice stop"):
        grid.sel(y=slice(2.0, 1.0))


def test_merge_refusals():
    with pytest.raises(ValueError, match="zero partitions"):
        Ugrid1d.merge_partitions([])
    with pytest.raises(ValueError, match="zero partitions"):
        xa.merge_partitions([])
    network = grid_of(*nc.chain(5))
    mesh = xa.Ugrid2d(np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), -1, np.array([[0, 1, 2]]))
    for grids in ([network, mesh], [mesh, network]):
        with pytest.raises(TypeError, match="same type"):
            xa.merge_partitions(grids)
    with pytest.raises(ValueError, match="one array per partition"):
        xa.merge_partitions([network, network], data=[np.zeros(5)])
    assert xa.merge_partitions([network]) is network


def test_refine_refusals():
    grid = grid_of(*nc.chain(12))
    with pytest.raises(ValueError, match="non-negative"):
        grid.refine_by_vertices(np.zeros((1, 2)), tolerance=-1e-9)
    with pytest.raises(ValueError, match="non-negative"):
        grid.refine_by_vertices(np.zeros((1, 2)), tolerance=np.nan)
    with pytest.raises(ValueError, match="node data"):
        grid.refine_by_vertices(np.zeros((1, 2)), data=np.zeros(12))
    with pytest.raises(ValueError, match="n_edge"):
        grid.refine_by_vertices(np.zeros((1, 2)), data=np.zeros(5))
    ring = grid_of(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.array([[0, 1], [1, 2], [2, 0]]))
    with pytest.raises(ValueError, match="exactly one"):
        ring.sel(x=slice(0.0, 1.0), data=np.zeros(3))
    with pytest.raises(ValueError, match="not a UGRID dimension"):
        ring.sel(x=slice(0.0, 1.0), data=np.zeros(3), dim="faces")

    class Network(Ugrid1d):
        pass

    sub = Network(np.arange(3.0), np.zeros(3), -1, np.array([[0, 1], [1, 2]]))
    assert xa.merge_partitions([sub]) is sub  # (a subclass is a Ugrid1d: no "same type" refusal)
    assert grid.dims == (grid.edge_dimension,)
