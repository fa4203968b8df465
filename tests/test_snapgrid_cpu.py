"""
CPU: the restatement of tests/snapgrid_cases.py against what the reference's ``snap_to_edges`` gave for the same pieces
(tests/golden/snapgrid_known.json, written by tests/golden/gen_snapgrid.py), and against the expected values of the reference's
own tests (tests/test_snap.py:184-329), which the file carries as data.  Every comparison is exact.
"""
import json
import os

import numpy as np
import pytest

import snapgrid_cases as sg

KNOWN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "snapgrid_known.json")))


def test_every_case_has_a_golden():
    assert set(KNOWN["cases"]) == set(sg.CASES)
    assert set(KNOWN["reference_test"]["line_counts"]) == {name for name in sg.CASES if name.startswith("ref_")}


@pytest.mark.parametrize("name", sorted(sg.CASES))
def test_restatement_equals_reference(oracle, name):
    frame, (line_index, edges, edge_lines), n_edge = sg.expected(oracle, name)
    known = KNOWN["cases"][name]
    for column in sg.COLUMNS:
        assert frame[column].dtype == sg.FRAME_DTYPES[column]
        assert np.array_equal(frame[column], np.asarray(known[column], dtype=sg.FRAME_DTYPES[column])), column
    assert np.array_equal(edges, np.asarray(known["edges"], dtype=np.int64))
    assert np.array_equal(edge_lines, np.asarray(known["edge_lines"], dtype=np.int64))
    assert np.array_equal(np.flatnonzero(~np.isnan(line_index)), edges) and np.array_equal(line_index[edges], edge_lines)


@pytest.mark.parametrize("name", sorted(KNOWN["reference_test"]["line_counts"]))
def test_reference_line_counts(oracle, name):
    """np.unique(uds["line_index"], return_counts=True) of tests/test_snap.py: lines 0 .. k - 1, then NaN."""
    _, (line_index, _, _), n_edge = sg.expected(oracle, name)
    counts = KNOWN["reference_test"]["line_counts"][name]
    values, actual = np.unique(line_index, return_counts=True)
    assert n_edge == 180
    assert np.array_equal(values[:-1], np.arange(len(counts) - 1)) and np.isnan(values[-1])
    assert np.array_equal(actual, counts)


def test_reference_docstring_example(oracle):
    """tests/test_snap.py:290-329: both lines name the same edges in the same order; the sum of [1, 2] per edge is 3."""
    doc = KNOWN["reference_test"]["docstring"]
    frame, _, _ = sg.expected(oracle, doc["case"])
    line, edge = frame["line_index"], frame["edge_index"]
    assert np.array_equal(edge[line == 0], edge[line == 1]) and (line == 0).sum() > 0
    sums = np.bincount(edge, weights=np.asarray(doc["my_variable"])[line])
    assert np.array_equal(np.unique(sums[np.unique(edge)]), [doc["sum_per_edge"]])


def test_random_case_is_contested(oracle):
    """The random case keeps what it is for: edges that several lines name, and winners that are not the first line."""
    frame, _, _ = sg.expected(oracle, "random_triangles")
    many, not_first = sg.contested(frame)
    assert len(many) >= 20 and len(not_first) >= 5


def test_long_bucket_case_is_long(oracle):
    frame, _, _ = sg.expected(oracle, "strip_two_rows")
    assert np.bincount(frame["line_index"]).max() > 256
