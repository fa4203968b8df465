"""
CPU: the yardsticks of the derive tests (tests/derive_cases.py) pinned to known answers (tests/golden/derive_known.json), the
library's one host step of the tessellations (csrc/xr_voronoi_boundary.h) as a stand-alone program under the host sanitizers
against ``voronoi._boundary_records``, and the argument errors of the new ``Ugrid2d`` methods that need no device.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import derive_cases as dc
import xugrid_amd as xa
from sample_cases import grid2d_arrays
from xugrid_amd import meshgen, voronoi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = dc.known()


# ---- the restatements against known answers -------------------------------------------------------------------------------
def test_triangulate_dense_known():
    k = KNOWN["connectivity"]["triangle_quad"]
    triangles, index = dc.triangulate_dense(np.array(k["faces"]))
    assert np.array_equal(triangles, k["triangles"]) and np.array_equal(index, k["triangle_face"])
    faces3 = np.array(KNOWN["connectivity"]["two_triangles"]["faces"])
    triangles, index = dc.triangulate_dense(faces3)
    assert np.array_equal(triangles, faces3) and triangles is not faces3 and np.array_equal(index, [0, 1])


def test_circumcenters_known():
    k = KNOWN["connectivity"]["two_triangles"]
    nodes = np.array(k["nodes"])
    assert np.allclose(dc.circumcenters(np.array(k["faces"]), nodes[:, 0], nodes[:, 1]), k["circumcenters"])
    with pytest.raises(NotImplementedError):
        dc.circumcenters(np.array(KNOWN["connectivity"]["triangle_quad"]["faces"]), nodes[:, 0], nodes[:, 1])


def test_perimeter_and_bounds_known():
    k = KNOWN["connectivity"]["triangle_quad"]
    faces, x, y = np.array(k["faces"]), np.array(k["node_x"]), np.array(k["node_y"])
    expected = np.array(k["perimeter_minus_sqrt2"]) + np.sqrt(2.0) * np.array(k["perimeter_sqrt2_count"])
    assert np.allclose(dc.perimeter(faces, x, y), expected)
    assert np.array_equal(dc.face_bounds(faces, x, y), [[0.0, 0.0, 1.0, 1.0], [1.0, 0.0, 2.0, 1.0]])


def test_grid2d_known():
    nodes, faces = grid2d_arrays()
    k = KNOWN["grid2d"]
    triangles, index = dc.triangulate_dense(faces)
    assert np.array_equal(triangles, k["triangulation"]["triangles"]) and np.array_equal(index, k["triangulation"]["triangle_face"])
    centroids = np.array([nodes[f[f >= 0]].mean(axis=0) for f in faces])  # (two unit quads under two triangles)
    vertices, cells, face_index, interp = dc.host_tessellation(nodes, faces, centroids, (True, False, False))
    assert interp is None
    assert np.allclose(vertices, np.vstack([centroids, k["voronoi_topology"]["exterior"]]))
    assert np.array_equal(cells, k["voronoi_topology"]["faces"]) and np.array_equal(face_index, k["voronoi_topology"]["face_index"])
    assert np.array_equal(dc.triangulate_dense(cells)[0], k["centroid_triangulation"]["triangles"])
    assert len(dc.host_tessellation(nodes, faces, centroids, (False, False, False))[1]) == k["n_face"]["centroidal_no_exterior"]
    assert len(dc.host_tessellation(nodes, faces, centroids, (True, False, False))[1]) == k["n_face"]["centroidal_no_vertices"]
    assert len(dc.host_tessellation(nodes, faces, centroids, (True, True, False))[1]) == k["n_face"]["centroidal_default"]


def test_four_triangle_square_known():
    k = KNOWN["four_triangle_square"]
    xy, faces = dc.four_square()
    cc = dc.circumcenters(faces, xy[:, 0], xy[:, 1])
    assert np.array_equal(cc, [[1.0, 0.0], [2.0, 1.0], [1.0, 2.0], [0.0, 1.0]])  # each on its boundary edge: exact
    for flags in ((True, True, False), (True, True, True)):
        vertices, cells, face_index, interp = dc.host_tessellation(xy, faces, cc, flags)
        assert np.array_equal(cells, k["circumcenter_cells"]) and len(cells) == k["circumcenter_n_face"]
        assert np.array_equal(face_index, [0, 1, 2, 3, -1, -1, -1, -1])  # every projection is dropped
    assert (dc.host_tessellation(xy, faces, cc, (True, False, False))[1][1:, 2] == -1).all()  # two-corner boundary cells


def test_case_meshes():
    assert dc.gon32_mesh()[1].shape == (3, 32) and len(dc.triangulate_dense(dc.gon32_mesh()[1])[0]) == 32
    for n in (2047, 2048, 2049):
        assert len(dc.mixed_with_faces(n)[1]) == n
    xy, faces = dc.strip_mesh()
    assert np.bincount(faces.ravel()).max() == 2
    xy, faces = dc.compaction_mesh()
    per_node = np.bincount(faces[faces >= 0], minlength=len(xy))
    assert per_node[faces[0, :3]].max() < 3 and (per_node >= 3).sum() == 4
    vertices, cells, face_index, _ = dc.host_tessellation(xy, faces, np.zeros((len(faces), 2)), (False, False, False))
    assert len(vertices) == 9 and cells.max() == 8 and face_index.size == 10  # face 0 unused: every id shifts down by one
    xy, faces = dc.clockwise_mesh()
    assert (dc.polygon_area_signed(xy, faces) < 0).all()


# ---- the host step of the library, stand-alone under the sanitizers ---------------------------------------------------------
@pytest.fixture(scope="module")
def boundary_program(tmp_path_factory):
    compiler = next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    out = str(tmp_path_factory.mktemp("voronoi_boundary") / "boundary")
    source = os.path.join(ROOT, "tests", "native", "voronoi_boundary_main.cpp")
    proc = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", out, source], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return out


def centroids_of(xy, faces):
    closed = np.where(faces < 0, faces[:, :1], faces)
    if faces.shape[1] == 3:
        return xy[faces].mean(axis=1)
    p = xy[np.column_stack([closed, closed[:, 0]])]
    rel = p - p[:, :1]
    a, b = rel[:, :-1], rel[:, 1:]
    det = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    w = 1.0 / (3.0 * det.sum(axis=1))
    return np.column_stack([w * ((a + b)[..., 0] * det).sum(axis=1), w * ((a + b)[..., 1] * det).sum(axis=1)]) + p[:, 0]


def local_cases():
    nodes, faces = grid2d_arrays()
    yield "grid2d", nodes, faces, centroids_of(nodes, faces)
    xy, faces = meshgen.mixed_mesh(36, 3)
    yield "mixed36", xy, faces, centroids_of(xy, faces)
    xy, faces = meshgen.triangle_mesh(200, 1)
    yield "triangles200", xy, faces, centroids_of(xy, faces)
    yield "triangles200_circumcenters", xy, faces, dc.circumcenters(faces, xy[:, 0], xy[:, 1])
    xy, faces = dc.four_square()
    yield "square_circumcenters", xy, faces, dc.circumcenters(faces, xy[:, 0], xy[:, 1])


LOCAL = {name: (xy, faces, gen) for name, xy, faces, gen in local_cases()}


@pytest.mark.parametrize("flags", [(True, True, False), (True, True, True), (True, False, False)])
@pytest.mark.parametrize("name", sorted(LOCAL))
def test_boundary_program_under_sanitizers(boundary_program, name, flags):
    xy, faces, generators = LOCAL[name]
    problem = dc.local_problem(xy, faces, generators)
    proc = subprocess.run([boundary_program], input=dc.program_input(problem, flags[1], flags[2]), capture_output=True, text=True,
                          timeout=120)
    assert proc.returncode == 0, proc.stderr[-4000:]
    status, extra, cells, tail, interp = dc.program_output(proc.stdout)
    assert status == 0
    e_extra, e_cells, e_tail, e_interp = dc.local_expected(problem, flags[1], flags[2])
    assert np.array_equal(extra, e_extra) and np.array_equal(cells, e_cells) and np.array_equal(tail, e_tail)
    if e_interp is None:
        assert interp.shape == (0, 2)
    else:
        assert np.array_equal(interp, e_interp)
    if name == "square_circumcenters":
        assert (tail == -1).all() and cells.shape[1] == (3 if flags[1] else 2)


def test_boundary_program_without_boundary(boundary_program):
    proc = subprocess.run([boundary_program], input="4 0 0 0 1 1\n\n0\n\n\n\n\n\n\n\n", capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-4000:]
    status, extra, cells, tail, interp = dc.program_output(proc.stdout)
    assert status == 0 and extra.shape == (0, 2) and cells.size == 0 and tail.size == 0 and interp.shape == (0, 2)


# ---- argument errors that need no device ----------------------------------------------------------------------------------
def test_methods_exist():
    for name in ("triangulate", "tesselate_centroidal_voronoi", "tesselate_circumcenter_voronoi"):
        assert callable(getattr(xa.Ugrid2d, name))
    for name in ("triangulation", "voronoi_topology", "centroid_triangulation", "circumcenters", "perimeter", "face_bounds"):
        assert isinstance(getattr(xa.Ugrid2d, name), property)
    assert callable(xa.ugrid2d.DeviceUgrid2d.from_device_mesh)


def test_circumcenter_errors_need_no_device(monkeypatch):
    nodes, faces = grid2d_arrays()
    grid = xa.Ugrid2d(nodes[:, 0], nodes[:, 1], -1, faces)

    def no_device(self):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(xa.Ugrid2d, "device_mesh", property(no_device))
    with pytest.raises(NotImplementedError, match="Circumcenters are only supported for triangular grids"):
        grid.circumcenters
    with pytest.raises(NotImplementedError, match="Circumcenters are only supported for triangular grids"):
        grid.tesselate_circumcenter_voronoi()


def test_voronoi_topology_device_keeps_its_defaults():
    import inspect

    sig = inspect.signature(voronoi.voronoi_topology_device)
    assert list(sig.parameters)[:3] == ["grid", "compact", "host_boundary"]
    for name, default in (("add_exterior", True), ("add_vertices", True), ("skip_concave", True), ("generators", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is default
    for name in ("tesselate_centroidal_voronoi", "tesselate_circumcenter_voronoi"):
        defaults = {k: p.default for k, p in inspect.signature(getattr(xa.Ugrid2d, name)).parameters.items() if k != "self"}
        assert defaults == {"add_exterior": True, "add_vertices": True, "skip_concave": False}
