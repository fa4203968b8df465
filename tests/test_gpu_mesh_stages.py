"""
GPU (-m gpu): the mesh handle as its stages (xugrid_amd/csrc/xr_objects.h: raw, statistics, prepared, query order, tree index,
caches) seen from outside -- the bytes each stage adds and invalidation gives back, the re-preparations the stage flags stand
for (light -> query depth, sampled -> exact statistics), and the three ways a connectivity gets into a handle (device-side
ingest of a small host mesh, narrowing on the way of a large one, device arrays) with their one report of the first bad face.
"""
import numpy as np
import pytest

from xugrid_amd import meshgen

pytestmark = pytest.mark.gpu

SAMPLE_MIN_FACES = 131072  # xr_mesh_front.hip: trees from this size on are sized from a sample of their faces
DEVICE_INGEST_BYTES = 1 << 20  # xr_mesh.hip: host meshes below take two plain copies and the ingest kernel
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


# ---- stage accounting ----------------------------------------------------------------------------------------------------------
def polygon_mesh():
    """42 disjoint convex polygons of 3 to 6 nodes on a 7 x 6 grid inside the unit square, CCW, m = 6"""
    k = 3 + np.arange(42) % 4
    cx, cy = (np.arange(42) % 7 + 0.5) / 7.0, (np.arange(42) // 7 + 0.5) / 6.0
    xy, faces, n = [], np.full((42, 6), -1, dtype=np.int64), 0
    for f in range(42):
        t = 2.0 * np.pi * (np.arange(k[f]) + 0.25 * f) / k[f]
        xy.append(np.column_stack([cx[f] + 0.06 * np.cos(t), cy[f] + 0.06 * np.sin(t)]))
        faces[f, : k[f]] = n + np.arange(k[f])
        n += k[f]
    return np.concatenate(xy), faces


ACCOUNTING = {
    "200 triangles": lambda: meshgen.triangle_mesh(121, 0, delaunay=False),
    "200 quads": lambda: meshgen.quad_mesh(np.linspace(0.0, 1.0, 21), np.linspace(0.0, 1.0, 11)),
    "ragged, m = 6": polygon_mesh,
}


def partner():
    """a tree for the meshes above to be the query of: ~600 triangles over the unit square"""
    return cached("partner", lambda: meshgen.triangle_mesh(300, 3))


def one_round(E, mesh, tree):
    mesh.prepare()
    prepared = mesh.device_bytes()
    mesh.build_index()
    indexed = mesh.device_bytes()
    tree.overlap(mesh)
    return prepared, indexed, mesh.device_bytes()


@pytest.mark.parametrize("name", list(ACCOUNTING))
def test_stage_accounting(hip, name):
    E = hip.engine
    xy, faces = ACCOUNTING[name]()
    n_node, (n_face, m) = xy.shape[0], faces.shape
    assert n_face in (200, 42)
    mesh, tree = E.DeviceMesh(xy, faces), E.DeviceMesh(*partner())
    created = 16 * n_node + 4 * n_face * m
    assert mesh.device_bytes() == created
    first = one_round(E, mesh, tree)
    print(name, "created", created, "prepared, indexed, queried", first)
    if m <= 4:  # vertex blocks, lengths, the eight statistics
        assert first[0] == created + 16 * n_face * m + n_face + 64
    assert created < first[0] < first[1] <= first[2]
    mesh.invalidate()
    assert mesh.device_bytes() == created
    assert one_round(E, mesh, tree) == first
    mesh.invalidate()
    assert mesh.device_bytes() == created


def test_provenance_arrays_are_counted_and_kept(hip):
    E = hip.engine
    xy, faces = meshgen.mixed_mesh(150, 2)
    mesh = E.DeviceMesh(xy, faces)
    tri = mesh.triangulate()
    n_tri = int(((faces >= 0).sum(axis=1) - 2).sum())
    assert tri.n_face == n_tri
    expected = 16 * tri.n_node + 4 * 3 * n_tri + 4 * n_tri  # + the source face of every triangle
    assert tri.device_bytes() == expected
    ids = np.arange(5, 60, dtype=np.int64)
    sub, identity, problems = mesh.subset(E.DeviceArray.from_host(ids).ptr, ids.size)
    assert sub is not None and not identity and problems == (0, 0)
    expected_sub = 16 * sub.n_node + 4 * 4 * ids.size + 4 * sub.n_node  # + the source node of every node
    assert sub.device_bytes() == expected_sub
    tri_face, sub_node = E.download(tri.triangle_face_dev()), E.download(sub.subset_node_index_dev())
    for derived, size in ((tri, expected), (sub, expected_sub)):
        derived.prepare()
        derived.build_index()
        assert derived.device_bytes() > size
        derived.invalidate()
        assert derived.device_bytes() == size
    assert np.array_equal(E.download(tri.triangle_face_dev()), tri_face)
    assert np.array_equal(E.download(sub.subset_node_index_dev()), sub_node)


# ---- what the stage flags stand for ----------------------------------------------------------------------------------------------
def weights(tree, query):
    data, indices, indptr = tree.overlap(query).download()
    return indptr, indices, data


def assert_same_weights(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y))


def test_tree_then_query_and_back(hip):
    E = hip.engine
    a, b = meshgen.triangle_mesh(300, 0), meshgen.triangle_mesh(300, 1, 30.0, 0.7)
    fresh_a_query = weights(E.DeviceMesh(*b), E.DeviceMesh(*a))
    fresh_a_tree = weights(E.DeviceMesh(*a), E.DeviceMesh(*b))
    assert fresh_a_query[0][-1] > 0 and fresh_a_tree[0][-1] > 0
    # light preparation (statistics only) first, query depth second
    A, B = E.DeviceMesh(*a), E.DeviceMesh(*b)
    assert_same_weights(weights(A, B), fresh_a_tree)
    assert_same_weights(weights(B, A), fresh_a_query)
    # ... and the other way round
    A, B = E.DeviceMesh(*a), E.DeviceMesh(*b)
    assert_same_weights(weights(B, A), fresh_a_query)
    assert_same_weights(weights(A, B), fresh_a_tree)


def test_sampled_statistics_are_redone_for_the_default_tolerance(hip, xr_option):
    E = hip.engine
    xy, faces = cached("sampled tree", lambda: meshgen.triangle_mesh(257 * 257, 0, delaunay=False))
    assert faces.shape[0] == SAMPLE_MIN_FACES
    qxy, qfaces = meshgen.triangle_mesh(400, 1, 30.0, 0.6, delaunay=False)
    rng = np.random.default_rng(5)
    corners = xy[faces[rng.integers(0, faces.shape[0], 300)]]
    points = np.concatenate([rng.random((500, 2)), corners[:100, 0], 0.5 * (corners[100:200, 0] + corners[100:200, 1]),
                             corners[200:].mean(axis=1), [[-1.0, 0.5], [0.5, 2.0]]])
    expected = E.DeviceMesh(xy, faces).locate_points(points)
    assert (expected >= 0).sum() > 700 and (expected < 0).sum() >= 2

    xr_option("front_fused", 0)  # (the two-launch front names the tree's statistics kernel)
    tree, query = E.DeviceMesh(xy, faces), E.DeviceMesh(qxy, qfaces[:256])
    with E.KernelTimer() as timer:
        tree.overlap(query)
    launches = {k for k, v in timer.records.items() if v[0]}
    assert "sample_stats" in launches and "prepare_stats" not in launches
    with E.KernelTimer() as timer:
        found = tree.locate_points(points)
    launches = {k for k, v in timer.records.items() if v[0]}
    assert "prepare_stats" in launches and "sample_stats" not in launches  # all faces this time
    assert np.array_equal(found, expected)


# ---- ingest ----------------------------------------------------------------------------------------------------------------------
def with_fill(xy, faces, fill):
    """the mesh with `fill` in its empty slots; a fill value that is a node id gets an unused node of that number first"""
    xy, faces = xy.copy(), faces.copy()
    if 0 <= fill < xy.shape[0]:
        xy = np.insert(xy, fill, [[0.5, 0.5]], axis=0)
        faces[faces >= fill] += 1
    faces[faces < 0] = fill
    return xy, faces


def ingest_arrays(dtype, fill):
    """-> (xy, faces just below the device-ingest threshold, faces at it): one face apart"""

    def make():
        xy, faces = with_fill(*cached("mixed", lambda: meshgen.mixed_mesh(30_000, 7)), fill)
        faces = faces.astype(dtype)
        row = 4 * faces.dtype.itemsize
        n_at = -(-(DEVICE_INGEST_BYTES - 16 * xy.shape[0]) // row)
        assert 100 < n_at <= faces.shape[0]
        assert (n_at - 1) * row + 16 * xy.shape[0] < DEVICE_INGEST_BYTES <= n_at * row + 16 * xy.shape[0]
        return xy, faces[: n_at - 1], faces[:n_at]

    return cached(("ingest", np.dtype(dtype).name, fill), make)


def ingest_paths(E, xy, below, at, fill):
    """name -> (a function that makes the handle, the connectivity it is given)"""
    dev_xy = E.DeviceArray.from_host(xy)

    def from_device(faces):
        dev = E.DeviceArray.from_host(faces)
        return E.DeviceMesh.from_device(dev_xy.ptr, xy.shape[0], dev.ptr, faces.dtype.itemsize, faces.shape[0], 4, fill)

    return {
        "host, below the threshold": (lambda f: E.DeviceMesh(xy, f, fill), below),
        "host, at the threshold": (lambda f: E.DeviceMesh(xy, f, fill), at),
        "device, below": (from_device, below),
        "device, at": (from_device, at),
    }


INGEST = [(np.int32, -1), (np.int32, 999), (np.int64, -1), (np.int64, 999)]


@pytest.mark.parametrize("dtype,fill", INGEST)
def test_ingest_paths_agree(hip, dtype, fill):
    E = hip.engine
    xy, below, at = ingest_arrays(dtype, fill)
    assert (at == fill).any() and (at[:, 3] != fill).any()
    for name, (make, faces) in ingest_paths(E, xy, below, at, fill).items():
        with E.KernelTimer() as timer:
            mesh = make(faces)
        kernel = bool(timer.records.get("ingest_faces", (0, 0.0))[0])
        assert kernel == (name != "host, at the threshold"), name  # (narrowed on the way instead)
        got_xy, got_faces = mesh.download()
        assert np.array_equal(bits(got_xy), bits(xy)), name
        assert np.array_equal(got_faces, np.where(faces == fill, -1, faces).astype(np.int64)), name


@pytest.mark.parametrize("dtype,fill", INGEST)
def test_ingest_reports_the_first_bad_face(hip, dtype, fill):
    E = hip.engine
    xy, below, at = ingest_arrays(dtype, fill)
    n_node = xy.shape[0]

    def broken(faces, short=(), out_of_range=()):
        faces = faces.copy()
        for f in short:
            faces[f, 1] = fill
        for f in out_of_range:
            faces[f, 0] = n_node
        return faces

    cases = [
        (dict(short=(7,), out_of_range=(3,)), "face 7 has fewer than 3 nodes"),  # too short is reported first
        (dict(out_of_range=(3,)), "face 3 references a node outside [0,%d)" % n_node),
        (dict(short=(20, 7)), "face 7 has fewer than 3 nodes"),
        (dict(out_of_range=(9, 3, 50)), "face 3 references"),
    ]
    for kw, message in cases:
        for name, (make, faces) in ingest_paths(E, xy, below, at, fill).items():
            with pytest.raises(ValueError) as err:
                make(broken(faces, **kw))
            assert message in str(err.value), (name, kw, str(err.value))
            assert str(err.value).startswith("xr_mesh_create_dev: " if name.startswith("device") else "xr_mesh_create: "), name
