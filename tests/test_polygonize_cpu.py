"""
CPU: the yardstick of the polygonize tests (tests/polygonize_cases.py) pinned without a device -- against counts known in
advance, against the burn yardstick's round trip (``burn_numpy`` over its polygons returns the data), against area sums
(exact on the integer lattices) -- the argument errors of ``xugrid_amd.polygonize`` that need no device, and the library's one
host step (the ring ordering of csrc/xr_polygonize_order.h) as a stand-alone program under the host sanitizers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import polygonize_cases as pc
import xugrid_amd as xa
from burn_cases import burn_numpy
from xugrid_amd.polygonize import host_data, polygonize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = tuple(n for n in pc.CASE_NAMES if n not in ("permuted40k_bands", "hubs", "strip3000"))  # the round trip is brute force
LATTICE = ("stripe", "hole", "pinch", "checkerboard", "islands", "nested", "diagonal_holes")


@pytest.mark.parametrize("name", sorted(pc.KNOWN_COUNTS))
def test_known_counts(name):
    e = pc.expected(name)
    assert (len(e["polygon_offsets"]) - 1, e["n_ring"], e["n_halfedge"]) == pc.KNOWN_COUNTS[name]


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_layout(name):
    """Offsets span the arrays, rings are closed, n_vertex = n_halfedge + n_ring, the half-edges are those of the edge table,
    every region has exactly one polygon and every polygon one ring of positive area, first."""
    xy, faces, data = pc.case(name)
    e = pc.expected(name)
    coords, ro, po = e["coords"], e["ring_offsets"], e["polygon_offsets"]
    n_polygon = len(po) - 1
    assert ro[0] == 0 and ro[-1] == len(coords) and po[0] == 0 and po[-1] == len(ro) - 1
    assert len(coords) == e["n_halfedge"] + e["n_ring"] and e["n_halfedge"] == e["host_halfedge_count"]
    assert np.array_equal(coords[ro[:-1]], coords[ro[1:] - 1])
    assert n_polygon == (e["face_polygon"].max() + 1 if (e["face_polygon"] >= 0).any() else 0)
    assert np.array_equal(e["face_polygon"] < 0, np.isnan(data))
    if name != "all_nan":
        assert n_polygon >= 1 and np.all(np.diff(po) >= 1)
    areas = pc.ring_areas(e)
    assert np.all(areas[po[:-1]] > 0)
    holes = np.ones(len(areas), dtype=bool)
    holes[po[:-1]] = False
    assert np.all(areas[holes] < 0)
    first = np.array([np.nonzero(e["face_polygon"] == p)[0][0] for p in range(n_polygon)], dtype=np.int64)
    assert np.all(np.diff(first) > 0) and np.array_equal(e["values"], data[first], equal_nan=True)


@pytest.mark.parametrize("name", LATTICE)
def test_area_sums_exact_on_lattices(name):
    e = pc.expected(name)
    areas, po = pc.ring_areas(e), e["polygon_offsets"]
    for p in range(len(po) - 1):
        assert areas[po[p]:po[p + 1]].sum() == e["face_area"][e["face_polygon"] == p].sum()


@pytest.mark.parametrize("name", SMALL)
def test_burn_round_trip(name):
    xy, faces, data = pc.case(name)
    e = pc.expected(name)
    back = burn_numpy(pc.centroids(xy, faces), 1e-12, polygons=(e["coords"], e["ring_offsets"], e["polygon_offsets"], e["values"]))
    assert np.array_equal(back, data, equal_nan=True)


def test_reversed_faces_give_the_same_polygons():
    a, b = pc.expected("mixed900_two"), pc.expected("mixed900_reversed")
    assert np.array_equal(a["face_polygon"], b["face_polygon"]) and np.array_equal(a["polygon_offsets"], b["polygon_offsets"])
    # a reversed face numbers its slots the other way round: a ring may start at another of its vertices, holes may swap
    assert pc.normal_form(a) == pc.normal_form(b)


# ---- argument errors that need no device ----------------------------------------------------------------------------------
def grid3():
    xy, faces = pc.case("stripe")[:2]
    return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)


def test_polygonize_is_exported():
    assert xa.polygonize is polygonize and callable(xa.Ugrid2d.polygonize)


def test_non_face_dimensions_are_refused():
    grid = grid3()
    with pytest.raises(ValueError, match="Cannot polygonize non-face dimension"):
        xa.polygonize(grid, np.zeros((2, 9)))
    with pytest.raises(ValueError, match="Cannot polygonize non-face dimension"):
        grid.polygonize(np.zeros(8))
    with pytest.raises(ValueError, match="Cannot polygonize non-face dimension"):
        grid.polygonize(np.float64(1.0))


def test_host_dtypes():
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        out = host_data(np.arange(9, dtype=dtype), 9)
        assert out.dtype == np.float64 and np.array_equal(out, np.arange(9.0))
    with pytest.raises(ValueError, match="float64 cannot represent"):
        host_data(np.array([0, 2**53 + 1] + [0] * 7, dtype=np.int64), 9)
    with pytest.raises(ValueError, match="float64 cannot represent"):
        host_data(np.array([np.iinfo(np.int64).max] + [0] * 8, dtype=np.int64), 9)
    assert host_data(np.array([2**53, -(2**62)] + [0] * 7, dtype=np.int64), 9)[1] == -(2.0**62)
    with pytest.raises(TypeError):
        host_data(np.zeros(9, dtype=bool), 9)
    with pytest.raises(TypeError, match="Ugrid2d"):
        xa.polygonize(object(), np.zeros(9))


# ---- the host step of the library, stand-alone under the sanitizers ---------------------------------------------------------
@pytest.fixture(scope="module")
def order_program(tmp_path_factory):
    compiler = next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    out = str(tmp_path_factory.mktemp("polygonize_order") / "order")
    source = os.path.join(ROOT, "tests", "native", "polygonize_order_main.cpp")
    proc = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", out, source], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return out


def run_order(program, table, n_polygon):
    text = f"{len(table)} {n_polygon}\n" + "".join(f"{p} {s} {n}\n" for p, s, n in table)
    proc = subprocess.run([program], input=text, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-4000:]
    lines = proc.stdout.split("\n")
    return int(lines[0]), [np.array(line.split(), dtype=np.int64) for line in lines[1:4]]


@pytest.mark.parametrize("name", ["islands", "mixed900_own", "nested", "one_triangle"])
def test_ring_order_program_under_sanitizers(order_program, name):
    e = pc.expected(name)
    status, (new_pos, ring_offsets, polygon_offsets) = run_order(order_program, e["ring_table"], len(e["polygon_offsets"]) - 1)
    assert status == 0
    assert np.array_equal(new_pos, e["ring_new_pos"])
    assert np.array_equal(ring_offsets, e["ring_offsets"]) and np.array_equal(polygon_offsets, e["polygon_offsets"])


def test_ring_order_program_reports_bad_tables(order_program):
    assert run_order(order_program, [(0, 1, 4), (1, -1, 4)], 2)[0] == 2    # polygon 1 has no exterior
    assert run_order(order_program, [(0, 1, 4), (0, 1, 4)], 1)[0] == 1     # polygon 0 has two
    assert run_order(order_program, [(0, 1, 4), (3, 1, 4)], 2)[0] == -2    # ring 1 names no polygon
    assert run_order(order_program, [(0, 1, 0)], 1)[0] == -1               # ring 0 has no segment
    assert run_order(order_program, [], 0)[0] == 0
