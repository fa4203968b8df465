"""
CPU: the numpy yardsticks of the geometry tests (tests/geometry_cases.py) give what the reference's own functions recorded in
tests/golden/geometry_known.json (tests/golden/gen_geometry.py) and what ``np.unique`` gives; the bounds cases keep the angles of
distinct corners apart (where the order of corners could depend on whose atan2 ran: DESIGN section 7); and the host arithmetic
of the radix sort (xugrid_amd/csrc/xr_sort_keys.h) runs stand-alone under the sanitizers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import geometry_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def floats(rows, width=2):
    return np.array(rows, dtype=np.float64).reshape(-1, width)


def values_equal(a, b):
    """Equal as doubles (the reference's np.unique may keep the other zero of a pair)."""
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(gc.unique_cases()))
def test_unique_restatement_is_numpy(name):
    xy = gc.unique_cases()[name]
    rows, index, inverse = gc.unique_rows(xy)
    u, u_index, u_inverse = np.unique(xy + 0.0, axis=0, return_index=True, return_inverse=True)
    assert values_equal(rows, u.reshape(-1, 2))
    assert np.array_equal(index, u_index) and np.array_equal(inverse, np.asarray(u_inverse).ravel())
    assert gc.same_bits(rows, xy[index]) and values_equal(rows[inverse], xy)


def test_unique_restatement_keeps_the_first_zero():
    xy = np.array([[0.0, 1.0], [-0.0, 1.0], [2.0, -0.0], [2.0, 0.0]])
    rows, index, inverse = gc.unique_rows(xy)
    assert index.tolist() == [0, 2] and inverse.tolist() == [0, 0, 1, 1]
    assert gc.same_bits(rows, np.array([[0.0, 1.0], [2.0, -0.0]]))


@pytest.mark.parametrize("name", sorted(gc.BOUNDS_CASES))
def test_bounds_restatement_is_the_reference(name):
    k = gc.known()["bounds"][name]
    xb, yb = gc.BOUNDS_CASES[name]()
    assert gc.angles_apart(xb, yb)
    e = gc.bounds_topology(xb, yb)
    assert values_equal(e["xy"], floats(k["xy"]))
    assert np.array_equal(e["faces"], np.array(k["faces"], dtype=np.int64).reshape(-1, 4))
    assert np.array_equal(e["index"], np.array(k["index"], dtype=bool))
    assert len(k["warnings"]) == (1 if e["n_invalid"] else 0)
    if e["n_invalid"]:
        assert f"contain {e['n_invalid']} invalid faces" in k["warnings"][0]


def test_lattice32_answer():
    e = gc.bounds_topology(*gc.lattice32())
    assert len(e["faces"]) == 4 and len(e["xy"]) == 11 and e["n_invalid"] == 2
    assert e["index"].tolist() == [True, False, True, False, True, True]
    assert (e["faces"][:, 3] == -1).tolist() == [False, True, False, False]  # cell 2 is the triangle


def test_quad24_answer():
    e = gc.bounds_topology(*gc.quad24())
    assert len(e["xy"]) == 4 and (e["faces"] == e["faces"][0]).all()


@pytest.mark.parametrize("name", sorted(gc.known()["breaks"]))
def test_breaks_restatement_is_the_reference(name):
    k = gc.known()["breaks"][name]
    ny, nx, x_dec, y_dec = gc.LATTICE_CASES[name]
    cx, cy = gc.centres(ny, nx, x_dec, y_dec)
    assert gc.is_monotonic(cx, 1) and gc.is_monotonic(gc.interval_breaks(cy, 1), 0)
    assert gc.same_bits(gc.interval_breaks(gc.interval_breaks(cx, 1), 0), floats(k["x"], nx + 1))
    assert gc.same_bits(gc.interval_breaks(gc.interval_breaks(cy, 1), 0), floats(k["y"], nx + 1))
    assert gc.same_bits(gc.interval_breaks(cx[0]), np.array(k["x1d"]))


def test_monotonic_restatement_is_the_reference():
    k = gc.known()["monotonic"]
    assert k["zigzag"] == k["nan"] == "The input coordinate is not monotonic." and k["flat"] is True
    assert not gc.is_monotonic([0.0, 2.0, 1.0]) and not gc.is_monotonic([0.0, np.nan, 1.0]) and gc.is_monotonic([1.0, 1.0, 2.0])
    assert gc.interval_breaks([3.0]).tolist() == [3.0, 3.0]


@pytest.mark.parametrize("name", gc.REFERENCE_LATTICES)
def test_lattice_restatement_is_the_reference(name):
    ny, nx, x_dec, y_dec = gc.LATTICE_CASES[name]
    xy, faces = gc.lattice_mesh(*gc.axis_lattice(ny, nx, x_dec, y_dec))
    assert np.array_equal(faces, np.array(gc.known()["lattices"][name], dtype=np.int64).reshape(-1, 4))


def test_lattice_restatement_is_this_projects_helper():
    import xugrid_amd as xa

    for name, (ny, nx, x_dec, y_dec) in gc.LATTICE_CASES.items():
        x, y = gc.axis_lattice(ny, nx, x_dec, y_dec)
        xy, faces = gc.lattice_mesh(x, y)
        grid = xa.Ugrid2d._from_intervals_helper(x.ravel(), y.ravel(), nx, ny, "mesh2d")
        assert np.array_equal(faces, grid.face_node_connectivity), name
        assert gc.same_bits(xy, grid.node_coordinates)


@pytest.mark.parametrize("name", sorted(gc.known()["polygons"]))
def test_polygon_restatement_is_the_reference(name):
    k = gc.known()["polygons"][name]
    xy, faces = gc.rings_to_faces(*gc.polygon_cases()[name])
    assert values_equal(xy, floats(k["xy"]))
    assert np.array_equal(faces, np.array(k["faces"], dtype=np.int64).reshape(faces.shape))
    coords, ring_offsets, _ = gc.faces_to_rings(xy, faces)
    back_xy, back_faces = gc.rings_to_faces(coords, ring_offsets)
    assert gc.same_bits(back_xy, xy) and np.array_equal(back_faces, faces)


def test_polygon_restatement_without_polygons():
    xy, faces = gc.rings_to_faces(*gc.polygon_cases()["none"])
    assert xy.shape == (0, 2) and faces.shape == (0, 3)


@pytest.mark.parametrize("name", sorted(gc.known()["lines"]))
def test_line_restatement_is_the_reference(name):
    k = gc.known()["lines"][name]
    xy, edges = gc.lines_to_edges(*gc.line_cases()[name])
    assert values_equal(xy, floats(k["xy"]))
    assert np.array_equal(edges, np.array(k["edges"], dtype=np.int64).reshape(-1, 2))


# ---- the host arithmetic of the radix sort, stand-alone under the sanitizers -----------------------------------------------------
@pytest.fixture(scope="module")
def sort_program(tmp_path_factory):
    compiler = next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    out = str(tmp_path_factory.mktemp("sort_keys") / "sort")
    source = os.path.join(ROOT, "tests", "native", "sort_keys_main.cpp")
    proc = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", out, source], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return out


@pytest.mark.parametrize("name", ("zeros", "subnormals", "last_bit_of_y", "sign_bit_only", "all_equal", "n257", "n0"))
def test_sort_arithmetic_under_sanitizers(sort_program, name):
    """The program checks that the key image keeps the order of the doubles, sorts the rows by digits as the device does
    (sequentially, skipping the passes the mask names) and prints the order: np.lexsort's, ties in input order."""
    xy = gc.unique_cases()[name][:300]
    text = f"{len(xy)}\n" + "".join(f"{x!r} {y!r}\n" for x, y in xy.tolist())
    proc = subprocess.run([sort_program], input=text, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = proc.stdout.split("\n")
    order = np.array(lines[0].split(), dtype=np.int64)
    assert np.array_equal(order, np.lexsort((xy[:, 1] + 0.0, xy[:, 0] + 0.0)))
    assert lines[2] == "images ok"
    if name == "all_equal":
        assert lines[1] == "0"  # every pass skipped
    if name == "last_bit_of_y":
        assert int(lines[1], 16) & 0xFF00 == 0  # x is constant: none of its passes runs
