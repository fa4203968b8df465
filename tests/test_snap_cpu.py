"""
CPU: the restatements of tests/snap_cases.py against what the reference's ``snap_nodes`` / ``snap_to_nodes`` returned for the same
cases (tests/golden/snap_known.json, written by tests/golden/gen_snap.py), and against the expected values of the reference's own
tests, which the file carries as data.  Every comparison is exact.
"""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import snap_cases as sc

KNOWN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "snap_known.json")))


def test_every_case_has_a_golden():
    assert set(KNOWN["snap_nodes"]) == set(sc.NODES_CASES)
    assert set(KNOWN["snap_to_nodes"]) == set(sc.TO_CASES)


@pytest.mark.parametrize("name", sorted(sc.NODES_CASES))
def test_snap_nodes_restatement(name):
    x, y, d = sc.NODES_CASES[name]()
    inverse, ids, xs, ys = sc.snap_nodes_ref(x, y, d)
    known = KNOWN["snap_nodes"][name]
    if known["inverse"] is None:
        assert inverse is None
    else:
        assert inverse is not None and sc.equals_known(inverse, known["inverse"])
        assert np.array_equal(np.unique(inverse), np.arange(len(ids))) and np.array_equal(inverse[ids], np.arange(len(ids)))
    assert sc.equals_known(xs, known["x"]) and sc.equals_known(ys, known["y"])


@pytest.mark.parametrize("name", sorted(KNOWN["reference_test"]["snap_nodes"]))
def test_snap_nodes_reference_tests(name):
    x, y, d = sc.NODES_CASES[name]()
    inverse, _, xs, ys = sc.snap_nodes_ref(x, y, d)
    expected = KNOWN["reference_test"]["snap_nodes"][name]
    assert (inverse is None) if expected["inverse"] is None else np.array_equal(inverse, expected["inverse"])
    assert np.array_equal(xs, expected["x"]) and np.array_equal(ys, expected["y"])
    if name.startswith("ref_two_lines"):
        assert np.array_equal(inverse[sc.TWO_LINES_EDGES], KNOWN["reference_test"]["two_lines_edges"])


@pytest.mark.parametrize("name", sorted(sc.TO_CASES))
def test_snap_to_nodes_restatement(name):
    x, y, to_x, to_y, d = sc.TO_CASES[name]()
    xs, ys, index, count = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    known = KNOWN["snap_to_nodes"][name]
    assert sc.equals_known(xs, known["nearest"]["x"]) and sc.equals_known(ys, known["nearest"]["y"])
    if (count > 1).any():
        assert known["no_tiebreaker"] == {"raises": sc.TIES}
    else:
        assert sc.equals_known(xs, known["no_tiebreaker"]["x"]) and sc.equals_known(ys, known["no_tiebreaker"]["y"])
    assert np.array_equal(index >= 0, count >= 1)


@pytest.mark.parametrize("name", sorted(KNOWN["reference_test"]["snap_to_nodes"]))
def test_snap_to_nodes_reference_tests(name):
    x, y, to_x, to_y, d = sc.TO_CASES[name]()
    xs, ys, _, _ = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    expected = KNOWN["reference_test"]["snap_to_nodes"][name]
    assert np.array_equal(xs, expected["x"]) and np.array_equal(ys, expected["y"])


def test_messages():
    assert KNOWN["bad_tiebreaker"]["raises"] == sc.BAD_TIEBREAKER.format(KNOWN["bad_tiebreaker"]["tiebreaker"])
    from xugrid_amd import snap

    assert snap.BAD_TIEBREAKER == sc.BAD_TIEBREAKER and snap.TIES == sc.TIES


def test_equidistant_lowest_number():
    x, y, to_x, to_y, d = sc.EQUIDISTANT
    xs, ys, index, count = sc.snap_to_nodes_ref(x, y, to_x, to_y, d)
    assert index.tolist() == [0, 2] and count.tolist() == [2, 2]
    assert xs.tolist() == [2.5, 5.0] and ys.tolist() == [1.0, 1.25]


def test_chain_orders():
    """What the round counts of the device test rest on: along the chain numbered in order (either way) every point has its one
    lower-numbered neighbour right before it; numbered even places first, no point has lower-numbered neighbours on both sides
    that are themselves waiting."""
    for case in (sc.chain, sc.chain_reversed, sc.chain_interleaved):
        x, y = case(70)
        inverse, ids, _, _ = sc.snap_nodes_ref(x, y, 0.25)
        assert len(ids) == 35
    x, _ = sc.chain_interleaved(70)
    assert np.array_equal(np.sort(x[:35]), np.arange(0, 70, 2) * 0.25)


def test_sweeps_constant_matches_header():
    from xugrid_amd import engine

    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "xugrid_amd.h")).read()
    assert int(re.search(r"#define XR_SNAP_SWEEPS (\d+)", header).group(1)) == engine.DeviceSnap.SWEEPS


def test_round_loop_under_sanitizers(tmp_path):
    """tests/native/snap_rounds_main.cpp: the stopping rule of the decision rounds and the guard on the adjacency's size
    (xugrid_amd/csrc/xr_snap_rounds.h), stand-alone."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compiler = next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    out = str(tmp_path / "snap_rounds")
    proc = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", out, os.path.join(root, "tests", "native", "snap_rounds_main.cpp")],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "SNAP_ROUNDS_OK" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
