"""
GPU (-m gpu): ``polygonize`` (xugrid_amd/polygonize.py, csrc/xr_polygonize.hip) against the Python yardstick of
tests/polygonize_cases.py, element for element: all five outputs, scipy's region numbers, the half-edge count of the host
edge table, the round trip through ``burn_vector_geometry`` on the device (exact, NaN kept) and the same bits on a second
call.  Every case except the all-NaN one has at least one region and every region exactly one polygon.
"""
import numpy as np
import pytest

import graph_cases
import polygonize_cases as pc
import xugrid_amd as xa
from xugrid_amd import engine
from xugrid_amd.polygonize import polygonize_device

pytestmark = pytest.mark.gpu

KEYS = ("coords", "ring_offsets", "polygon_offsets", "values", "face_polygon")


def device_grid(name):
    xy, faces, _ = pc.case(name)
    return graph_cases.device_grid(xy, faces)


def download(arrays):
    return [a if isinstance(a, np.ndarray) else a.download() if isinstance(a, engine.DeviceArray) else a.cpu().numpy() for a in arrays]


def assert_equals_yardstick(out, e):
    for key, got in zip(KEYS, out):
        want = e[key]
        assert got.dtype == want.dtype and got.shape == want.shape, key
        assert np.array_equal(got, want, equal_nan=True), key
    assert np.array_equal(np.signbit(out[3]), np.signbit(e["values"]))


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_case_equals_the_yardstick(hip, name):
    xy, faces, data = pc.case(name)
    e = pc.expected(name)
    grid = device_grid(name)
    data_dev = engine.DeviceArray.from_host(data)
    out_dev = grid.polygonize(data_dev, return_index=True)
    assert all(isinstance(a, engine.DeviceArray) for a in out_dev)
    out = download(out_dev)
    assert_equals_yardstick(out, e)
    assert np.array_equal(data_dev.download(), data, equal_nan=True)  # the input is untouched
    # counts: every region one polygon; the half-edges are those of the host edge table
    info, _ = polygonize_device(grid, data_dev)
    n_region = int(e["face_polygon"].max()) + 1 if (e["face_polygon"] >= 0).any() else 0
    assert info.n_polygon == n_region == len(out[2]) - 1 and (n_region >= 1 or name == "all_nan")
    assert info.n_halfedge == e["host_halfedge_count"] and info.n_ring == e["n_ring"]
    assert info.n_vertex == info.n_halfedge + info.n_ring == len(out[0])
    if name in pc.KNOWN_COUNTS:
        assert (info.n_polygon, info.n_ring, info.n_halfedge) == pc.KNOWN_COUNTS[name]
    # the round trip on the device
    back = xa.burn_vector_geometry(grid, polygons=out_dev[:4])
    assert isinstance(back, engine.DeviceArray)
    assert np.array_equal(back.download(), data, equal_nan=True)
    # the same bits on a second call
    again = download(grid.polygonize(data_dev, return_index=True))
    for a, b in zip(out, again):
        assert a.tobytes() == b.tobytes()


def test_reversed_faces_give_the_same_polygons(hip):
    """Every second face in the opposite node order: nothing but the start of a ring and the order of holes may move."""
    results = []
    for name in ("mixed900_two", "mixed900_reversed"):
        out = device_grid(name).polygonize(pc.case(name)[2], return_index=True)
        results.append(dict(zip(KEYS, out)))
    assert np.array_equal(results[0]["face_polygon"], results[1]["face_polygon"])
    assert pc.normal_form(results[0]) == pc.normal_form(results[1])


def test_negative_zero_joins_zero_and_keeps_its_sign(hip):
    xy, faces = pc.case("stripe")[:2]
    data = np.array([-0.0, 0.0, 0.0, 1, 1, 1, 0.0, -0.0, 0.0])
    out = graph_cases.device_grid(xy, faces).polygonize(data, return_index=True)
    assert_equals_yardstick(out, pc.polygonize_numpy(xy, faces, data))
    assert np.array_equal(np.signbit(out[3]), [True, False, False])


@pytest.mark.parametrize("name", ["islands", "nested"])
def test_host_and_rectilinear_grids(hip, name):
    """A host-built Ugrid2d and the RectilinearUgrid2d of the same lattice give what the device grid gives; numpy in, numpy out."""
    xy, faces, data = pc.case(name)
    e = pc.expected(name)
    host = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    out = host.polygonize(data, return_index=True)
    assert all(isinstance(a, np.ndarray) for a in out)
    assert_equals_yardstick(out, e)
    assert len(xa.polygonize(host, data)) == 4
    edges = np.arange(21, dtype=float)
    bounds = np.column_stack([edges[:-1], edges[1:]])
    rectilinear = xa.Ugrid2d.from_structured_bounds_device(bounds, bounds)
    assert type(rectilinear).__name__ == "RectilinearUgrid2d"
    # (the generated mesh numbers nodes, faces and slots as meshgen.quad_mesh does)
    assert_equals_yardstick(rectilinear.polygonize(data, return_index=True), e)


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_device_dtypes(hip, dtype):
    xy, faces, data = pc.case("islands")
    grid = device_grid("islands")
    out = download(grid.polygonize(engine.DeviceArray.from_host(data.astype(dtype)), return_index=True))
    assert_equals_yardstick(out, pc.expected("islands"))
    host = download(grid.polygonize(data.astype(dtype if dtype != np.int32 else np.int64), return_index=True))
    assert_equals_yardstick(host, pc.expected("islands"))


def test_float32_nan_on_the_device(hip):
    xy, faces, data = pc.case("nested")
    out = download(device_grid("nested").polygonize(engine.DeviceArray.from_host(data.astype(np.float32)), return_index=True))
    assert_equals_yardstick(out, pc.expected("nested"))


# torch has to initialise its HIP runtime BEFORE the engine binds the device, so this runs in a process of its own
# (tests/polygonize_worker_gpu.py)
def test_torch_in_torch_out():
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "polygonize_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_POLYGONIZE_OK" in res.stdout


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_shape_errors(hip):
    grid = device_grid("stripe")
    with pytest.raises(ValueError, match="Cannot polygonize non-face dimension"):
        grid.polygonize(engine.DeviceArray.from_host(np.zeros((1, 9))))
    with pytest.raises(ValueError, match="Cannot polygonize non-face dimension"):
        grid.polygonize(engine.DeviceArray.from_host(np.zeros(10)))
    with pytest.raises(ValueError, match="Cannot polygonize non-face dimension"):
        grid.polygonize(np.zeros(8))
    with pytest.raises(TypeError):
        grid.polygonize(engine.DeviceArray.from_host(np.zeros(9, dtype=np.int64)))


def test_zero_area_face_with_data_is_an_error(hip):
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [2.0, 0.0]])
    faces = np.array([[0, 1, 2], [0, 1, 3]])  # the second face is flat
    grid = graph_cases.device_grid(xy, faces)
    with pytest.raises(ValueError, match="degenerate face"):
        grid.polygonize(np.array([1.0, 1.0]))
    # ... without data it takes no part
    out = grid.polygonize(np.array([1.0, np.nan]), return_index=True)
    assert_equals_yardstick(out, pc.polygonize_numpy(xy, faces, np.array([1.0, np.nan])))


def test_non_manifold_mesh_is_an_error(hip):
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, -1.0]])
    faces = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]])  # three faces on the edge 0 - 1
    for grid in (graph_cases.device_grid(xy, faces), xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)):
        with pytest.raises(ValueError, match="non-manifold"):
            grid.polygonize(np.ones(3))


# ---- the labelling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["strip3000", "permuted40k"])
def test_labelling_takes_fewer_rounds_than_label_propagation(hip, mesh):
    """Constant data: the one region is the component.  Hook-and-compress against the minimum-label propagation of the face
    graph of the same grid, both counted in launches that were followed by a read-back."""
    xy, faces = graph_cases.strip(3000) if mesh == "strip3000" else graph_cases.big_permuted()
    grid = graph_cases.device_grid(xy, faces)
    info, _ = polygonize_device(grid, np.ones(len(faces)))
    propagation = int(grid._graph("face").label_rounds())
    print(f"{mesh}: hook-and-compress {info.label_rounds} rounds, label propagation {propagation} rounds")
    assert info.n_polygon == 1
    assert 1 <= info.label_rounds < propagation
