"""
GPU: meshes and per-face geometry derived on the device -- ``Ugrid2d.triangulate`` / ``triangulation``, ``circumcenters``,
``perimeter``, ``face_bounds``, the centroidal and circumcenter Voronoi tessellations for every flag set, ``voronoi_topology``
and ``centroid_triangulation`` -- on host-built grids and on grids whose mesh lives in HBM only, against the numpy
restatements of tests/derive_cases.py and ``voronoi.voronoi_topology`` fed with the generator points the device returned.
"""
import numpy as np
import pytest

import derive_cases as dc
import graph_cases
import xugrid_amd as xa
from sample_cases import grid2d_arrays
from xugrid_amd import engine, meshgen
from xugrid_amd.voronoi import voronoi_topology_device

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KINDS = ("host", "device")


def make_grid(kind, xy, faces):
    if kind == "host":
        return xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    assert kind == "device"
    return graph_cases.device_grid(xy, faces)


def to_numpy(a):
    return a if isinstance(a, np.ndarray) else a.download() if isinstance(a, engine.DeviceArray) else a.cpu().numpy()


# ---- triangulate ----------------------------------------------------------------------------------------------------------
TRIANGULATE = {
    "grid2d": grid2d_arrays,
    "mixed36": lambda: meshgen.mixed_mesh(36, 3),
    "triangles_in_four_columns": dc.triangles_in_four_columns,
    "clockwise": dc.clockwise_mesh,
    "gon32": dc.gon32_mesh,
    "mixed2047": lambda: dc.mixed_with_faces(2047),
    "mixed2048": lambda: dc.mixed_with_faces(2048),
    "mixed2049": lambda: dc.mixed_with_faces(2049),
    "triangles": lambda: meshgen.triangle_mesh(60, 2),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(TRIANGULATE))
def test_triangulate(hip, name, kind):
    xy, faces = TRIANGULATE[name]()
    xy, faces = np.asarray(xy, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    e_triangles, e_index = dc.triangulate_dense(faces)
    grid = make_grid(kind, xy, faces)
    tri, index = grid.triangulate(return_index=True)
    assert type(tri) is type(grid) and type(grid.triangulate()) is type(grid)
    if kind == "host":
        assert isinstance(index, np.ndarray)
    else:
        assert isinstance(index, engine.DeviceArray) and index.dtype == np.int64
    index = to_numpy(index)
    assert tri.n_face == len(e_triangles) and tri.n_max_node_per_face == 3 and tri.n_node == len(xy)
    assert np.array_equal(tri.face_node_connectivity, e_triangles) and np.array_equal(index, e_index)
    assert np.array_equal(tri.node_coordinates, xy)
    # the result is a grid: its areas add up to the source's, face by face (a fan of k - 2 triangles, one rounding each)
    area = grid.area
    k = (faces != -1).sum(axis=1)
    summed = np.bincount(e_index, weights=tri.area, minlength=len(faces))  # (every face here is convex: the fan's areas add up)
    print(name, kind, "area: largest |sum - area| / (eps * area) =", float((np.abs(summed - area) / (EPS * area)).max()),
          "allowed k - 2 =", int((k - 2).max()))
    assert np.all(np.abs(summed - area) <= (k - 2) * EPS * area)
    (x, y, triangles), tfc = grid.triangulation
    assert np.array_equal(x, xy[:, 0]) and np.array_equal(y, xy[:, 1])
    assert np.array_equal(triangles, e_triangles) and np.array_equal(tfc, e_index)
    assert grid.triangulation[0][2] is triangles  # cached
    grid.drop_device_caches()
    assert "_derive_cache" not in grid.__dict__


def test_triangulate_rectilinear(hip):
    xv, yv = np.array([0.0, 1.0, 3.0, 4.0]), np.array([0.0, 2.0, 3.0])
    grid = xa.ugrid2d.RectilinearUgrid2d(xv, yv)
    tri, index = grid.triangulate(return_index=True)
    e_triangles, e_index = dc.triangulate_dense(grid.face_node_connectivity)
    assert isinstance(tri, xa.ugrid2d.DeviceUgrid2d)
    assert np.array_equal(tri.face_node_connectivity, e_triangles) and np.array_equal(to_numpy(index), e_index)
    assert np.array_equal(grid.face_bounds, dc.face_bounds(grid.face_node_connectivity, grid.node_x, grid.node_y))


def test_face_data_reaches_the_triangles(hip):
    xy, faces = meshgen.mixed_mesh(36, 3)
    grid = graph_cases.device_grid(xy, faces)
    tri, index = grid.triangulate(return_index=True)
    data = np.arange(grid.n_face, dtype=np.float64)
    values = xa.sample.gather_points(engine.DeviceArray.from_host(data), grid.n_face, index)
    assert isinstance(values, engine.DeviceArray)
    assert np.array_equal(values.download(), data[dc.triangulate_dense(faces)[1]])


# ---- per-face geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["triangles200", "lattice"])
def test_circumcenters_bit_for_bit(hip, name, kind):
    xy, faces = meshgen.triangle_mesh(200, 1) if name == "triangles200" else dc.exact_lattice()
    grid = make_grid(kind, xy, faces)
    expected = dc.circumcenters(faces, xy[:, 0], xy[:, 1])
    got = grid.circumcenters
    assert got.dtype == np.float64 and got.shape == expected.shape and np.array_equal(got, expected)
    if name == "lattice":
        assert np.array_equal(2.0 * got, np.round(2.0 * got))  # half-integer points, exactly
    assert grid.circumcenters is got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["grid2d", "mixed36", "triangles", "gon32", "clockwise"])
def test_perimeter_and_bounds(hip, name, kind):
    xy, faces = TRIANGULATE[name]()
    xy, faces = np.asarray(xy, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    grid = make_grid(kind, xy, faces)
    assert np.array_equal(grid.face_bounds, dc.face_bounds(faces, xy[:, 0], xy[:, 1]))
    expected = dc.perimeter(faces, xy[:, 0], xy[:, 1])
    got = grid.perimeter
    m = faces.shape[1]
    err = np.abs(got - expected)
    print(name, kind, "perimeter: largest error / (eps * perimeter) =", float((err / (EPS * expected)).max()), "allowed", m - 1)
    assert np.all(err <= (m - 1) * EPS * expected)


def test_circumcenters_of_polygons_raise(hip):
    xy, faces = meshgen.mixed_mesh(36, 3)
    for grid in (make_grid("host", xy, faces), make_grid("device", xy, faces)):
        with pytest.raises(NotImplementedError, match="Circumcenters are only supported for triangular grids"):
            grid.circumcenters
        with pytest.raises(NotImplementedError, match="Circumcenters are only supported for triangular grids"):
            grid.tesselate_circumcenter_voronoi()
        with pytest.raises(NotImplementedError, match="Circumcenters are only supported for triangular grids"):
            grid.device_mesh.circumcenters_dev()


# ---- tessellations --------------------------------------------------------------------------------------------------------
TESSELLATE = {
    "mixed400": (lambda: meshgen.mixed_mesh(400, 3), ("centroids",)),
    "triangles200": (lambda: meshgen.triangle_mesh(200, 1), ("centroids", "circumcenters")),
    "triangles5000": (lambda: meshgen.triangle_mesh(5000, 2), ("centroids", "circumcenters")),
}
TESS_CASES = [(name, gen) for name in sorted(TESSELLATE) for gen in TESSELLATE[name][1]]
_expected = {}


def expected_tessellation(name, gen, flags, xy, faces, generators):
    key = (name, gen, flags)
    if key not in _expected:
        _expected[key] = dc.host_tessellation(xy, faces, generators, flags)
    return _expected[key]


def assert_tessellation(mesh, face_index, interp, expected):
    e_vertices, e_cells, e_face_index, e_interp = expected
    vertices, cells = mesh.download()
    assert vertices.shape == e_vertices.shape and np.array_equal(vertices, e_vertices)
    assert cells.shape == e_cells.shape and np.array_equal(cells, e_cells)
    assert np.array_equal(face_index, e_face_index)
    if e_interp is None:
        assert interp is None
    else:
        assert np.array_equal(interp, e_interp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flags", dc.FLAG_SETS)
@pytest.mark.parametrize("name,gen", TESS_CASES)
def test_tessellation_equals_the_restatement(hip, name, gen, flags, kind):
    xy, faces = TESSELLATE[name][0]()
    grid = make_grid(kind, xy, faces)
    generators = grid.centroids if gen == "centroids" else grid.circumcenters
    generators_dev = None if gen == "centroids" else grid.device_mesh.circumcenters_dev()
    expected = expected_tessellation(name, gen, flags, xy, faces, generators)
    mesh, face_index, interp = voronoi_topology_device(grid, add_exterior=flags[0], add_vertices=flags[1], skip_concave=flags[2],
                                                       generators=generators_dev)
    assert_tessellation(mesh, face_index, interp, expected)
    method = grid.tesselate_centroidal_voronoi if gen == "centroids" else grid.tesselate_circumcenter_voronoi
    tessellation = method(*flags)
    assert type(tessellation) is type(grid) and tessellation.n_face == len(expected[1])
    assert np.array_equal(tessellation.face_node_connectivity, expected[1])
    assert np.array_equal(tessellation.node_coordinates, expected[0])


@pytest.mark.parametrize("kind", KINDS)
def test_four_triangle_square(hip, kind):
    xy, faces = dc.four_square()
    grid = make_grid(kind, xy, faces)
    cells = np.array(dc.known()["four_triangle_square"]["circumcenter_cells"])
    for skip_concave in (False, True):
        tessellation = grid.tesselate_circumcenter_voronoi(True, True, skip_concave)
        assert tessellation.n_face == 5 and np.array_equal(tessellation.face_node_connectivity, cells)
        expected = dc.host_tessellation(xy, faces, grid.circumcenters, (True, True, skip_concave))
        assert np.array_equal(tessellation.node_coordinates, expected[0])
    assert grid.tesselate_circumcenter_voronoi().n_face == 5
    with pytest.raises(ValueError, match="fewer than 3 corners"):
        grid.tesselate_circumcenter_voronoi(True, False, False)


@pytest.mark.parametrize("kind", KINDS)
def test_compaction_renumbers(hip, kind):
    xy, faces = dc.compaction_mesh()
    grid = make_grid(kind, xy, faces)
    expected = dc.host_tessellation(xy, faces, grid.centroids, (False, False, False))
    mesh, face_index, interp = voronoi_topology_device(grid, add_exterior=False, add_vertices=False, skip_concave=False)
    assert_tessellation(mesh, face_index, interp, expected)
    assert mesh.n_node == 9 and face_index.size == 10 and not np.array_equal(mesh.download()[0], grid.centroids[:9])


@pytest.mark.parametrize("kind", KINDS)
def test_strip_without_exterior_raises(hip, kind):
    xy, faces = dc.strip_mesh()
    grid = make_grid(kind, xy, faces)
    with pytest.raises(ValueError, match="three faces"):
        grid.tesselate_centroidal_voronoi(add_exterior=False)
    assert grid.tesselate_centroidal_voronoi().n_face == grid.n_node  # with the exterior every node has a cell


@pytest.mark.parametrize("name", ["mixed400", "triangles400_lattice"])
def test_cells_tile_the_mesh(hip, name):
    """Independent of the restatement: with the default flags and centroids the cells tile the mesh, so the signed cell areas
    add up to the face areas -- within n_cell * eps * total (every cell area is a sum rounded relative to values of the size of
    the cell; meshes without hull slivers only: those make clockwise cells)."""
    xy, faces = meshgen.mixed_mesh(400, 3) if name == "mixed400" else meshgen.triangle_mesh(400, 5, delaunay=False)
    grid = make_grid("device", xy, faces)
    tessellation = grid.tesselate_centroidal_voronoi()
    signed = dc.polygon_area_signed(tessellation.node_coordinates, tessellation.face_node_connectivity)
    total = grid.area.sum()
    diff = abs(signed.sum() - total)
    print(name, "sum of signed cell areas - sum of face areas =", diff, "=", diff / (EPS * total), "eps * total; allowed", len(signed))
    assert diff <= len(signed) * EPS * total
    assert np.allclose(tessellation.area.sum(), total, rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", KINDS)
def test_grid2d_properties_equal_the_known_answers(hip, kind):
    nodes, faces = grid2d_arrays()
    grid = make_grid(kind, nodes, faces)
    k = dc.known()["grid2d"]
    vertices, cells, face_index = grid.voronoi_topology
    assert isinstance(cells, np.ndarray)
    assert np.allclose(vertices, np.vstack([grid.centroids, k["voronoi_topology"]["exterior"]]))
    assert np.array_equal(cells, k["voronoi_topology"]["faces"]) and np.array_equal(face_index, k["voronoi_topology"]["face_index"])
    (x, y, triangles), face_index = grid.centroid_triangulation
    assert np.array_equal(x, vertices[:, 0]) and np.array_equal(y, vertices[:, 1])
    assert np.array_equal(triangles, k["centroid_triangulation"]["triangles"])
    assert np.array_equal(face_index, k["voronoi_topology"]["face_index"])
    assert grid.tesselate_centroidal_voronoi(add_exterior=False).n_face == k["n_face"]["centroidal_no_exterior"]
    assert grid.tesselate_centroidal_voronoi(add_vertices=False).n_face == k["n_face"]["centroidal_no_vertices"]
    assert grid.tesselate_centroidal_voronoi().n_face == k["n_face"]["centroidal_default"]
    (_, _, triangles), tfc = grid.triangulation
    assert np.array_equal(triangles, k["triangulation"]["triangles"]) and np.array_equal(tfc, k["triangulation"]["triangle_face"])


def test_device_tessellation_works_as_a_grid(hip):
    # (a split lattice, not a Delaunay mesh: the hull slivers of those give clockwise cells that overlap their neighbours, so
    # the tessellation is no subdivision of the plane and has no single outline)
    xy, faces = meshgen.triangle_mesh(200, 1, delaunay=False)
    grid = graph_cases.device_grid(xy, faces)
    tessellation = grid.tesselate_centroidal_voronoi()
    assert isinstance(tessellation, xa.ugrid2d.DeviceUgrid2d)
    raster = xa.Ugrid2d.from_structured_bounds(np.column_stack([np.linspace(0, 0.9, 10), np.linspace(0.1, 1, 10)]),
                                               np.column_stack([np.linspace(0, 0.9, 10), np.linspace(0.1, 1, 10)]))
    regridder = xa.OverlapRegridder(tessellation, raster, method="mean")
    out = regridder.regrid(np.ones(tessellation.n_face))
    assert out.shape == (raster.n_face,) and np.nanmax(np.abs(out - 1.0)) == 0.0
    polygons = tessellation.polygonize(np.zeros(tessellation.n_face))
    assert len(to_numpy(polygons[2])) - 1 == 1 and len(to_numpy(polygons[3])) == 1
