"""
GPU (-m gpu): the device fills at their edges.  ``test_gpu_fill.py`` checks answers on friendly inputs; here the nearest
fill's chosen source is compared exactly with a brute-force search of the kernel's own arithmetic on the inputs where a
uniform-grid ring search goes wrong (points outside the valid box, degenerate boxes, the cell cap, coincident points,
exact ties, large coordinates, the distance bound); the device component labels are compared with scipy, the CG's
iterates -- not only its answer -- with scipy's loop restated (tests/fill_cases.py); and K runs past one launch grid.
"""
import time
import warnings

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph
from scipy.spatial import Delaunay

import xugrid_amd as xa
from fill_cases import brute_nearest, kdtree_nearest, reference_cg, reference_laplace, scaled_system
from test_gpu_fill import mesh_with_patch
from xugrid_amd import fill, meshgen

pytestmark = pytest.mark.gpu


# ---- nearest: data = index, so the output names the source the kernel chose
def point_grid(xy):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    return xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, np.zeros((0, 2), dtype=np.int64))


def chosen(xy, null, max_distance=None, grid=None):
    """-> (device source per point or -1, brute-force source per point, data)."""
    grid = point_grid(xy) if grid is None else grid
    data = np.arange(len(xy), dtype=np.float64)
    data[null] = np.nan
    out = grid.interpolate_na(data, dim="node", max_distance=max_distance)
    assert np.array_equal(out[~null], data[~null])
    src = np.where(np.isnan(out), -1, out).astype(np.int64)
    return src, brute_nearest(xy, data, np.inf if max_distance is None else max_distance), data


def assert_nearest(xy, null, max_distance=None):
    src, expected, _ = chosen(xy, null, max_distance)
    bad = np.nonzero(src != expected)[0]
    assert bad.size == 0, f"{bad.size} of {int(null.sum())} null points differ: {bad[:5]} {src[bad[:5]]} {expected[bad[:5]]}"
    return src


def test_nulls_outside_the_valid_box_and_far_outliers():
    """Nulls beyond the valid points' bbox are clamped into the edge cells of the search grid."""
    rng = np.random.default_rng(10)
    xy = rng.random((6000, 2))
    null = xy[:, 0] >= 0.5  # valid half / null half
    far = np.array([[10.0, 10.0], [-10.0, 0.5], [0.5, -10.0], [12.0, -11.0], [-9.5, 10.5], [0.25, 10.0], [10.0, 0.3]])
    xy = np.vstack([xy, far])
    null = np.r_[null, np.ones(len(far), dtype=bool)]
    assert_nearest(xy, null)
    # and nulls on all four sides of a valid core
    null = np.r_[np.abs(xy[:-len(far)] - 0.5).max(axis=1) > 0.2, np.ones(len(far), dtype=bool)]
    assert_nearest(xy, null)


@pytest.mark.parametrize("direction", ["horizontal", "vertical", "diagonal"])
def test_collinear_points(direction):
    rng = np.random.default_rng(11)
    t = np.cumsum(rng.uniform(0.1, 1.0, 5000))
    xy = {"horizontal": np.column_stack([t, np.full_like(t, 3.0)]),
          "vertical": np.column_stack([np.full_like(t, -2.0), t]),
          "diagonal": np.column_stack([t, 2.0 * t + 1.0])}[direction]
    null = rng.random(len(t)) < 0.3
    null[:200] = True  # nulls beyond one end of the valid points
    null[-300:] = True  # and beyond the other
    off = np.array([[t[0] - 50.0, xy[0, 1] + 40.0], [t[-1] + 100.0, xy[-1, 1] - 7.0], [0.5 * (t[0] + t[-1]), 1e4]])
    assert_nearest(np.vstack([xy, off]), np.r_[null, np.ones(len(off), dtype=bool)])


def test_long_line_past_the_cell_cap():
    """More than 2^16 valid points on a horizontal line: 1 << 15 cells, the last one holding every point past the cap"""
    rng = np.random.default_rng(12)
    n = 90_000
    x = np.cumsum(rng.uniform(0.5, 1.5, n))
    xy = np.column_stack([x, np.full(n, 7.0)])
    null = rng.random(n) < 0.04
    null[-2000:-1500] = True  # a run of nulls inside the clamped last cell
    null[:100] = True
    assert (~null).sum() > 1 << 16
    xy = np.vstack([xy, [[x[-1] + 3e4, 7.0], [x[-1] * 0.7, 9.0]]])
    null = np.r_[null, True, True]
    grid = point_grid(xy)
    data = np.arange(len(xy), dtype=np.float64)
    data[null] = np.nan
    grid.interpolate_na(data, dim="node")  # the point upload and first-use costs
    t0 = time.perf_counter()
    out = grid.interpolate_na(data, dim="node")
    dt = time.perf_counter() - t0
    src = np.where(np.isnan(out), -1, out).astype(np.int64)
    expected = kdtree_nearest(xy, data)
    assert np.array_equal(src, expected), np.nonzero(src != expected)[0][:10]
    print(f"line of {len(xy)} points, {int(null.sum())} null: nearest fill {dt * 1e3:.1f} ms")


def test_small_valid_sets():
    rng = np.random.default_rng(13)
    xy = rng.random((1000, 2))
    null = np.ones(1000, dtype=bool)
    null[417] = False  # one valid point: every null takes it
    src = assert_nearest(xy, null)
    assert (src == 417).all()
    null = np.zeros(1000, dtype=bool)
    null[3] = True  # exactly one null
    assert_nearest(xy, null)
    assert_nearest(xy[:1], np.zeros(1, dtype=bool))  # a single point, valid
    assert_nearest(xy[:2], np.array([True, False]))
    with pytest.raises(ValueError, match="All values are NA."):
        point_grid(xy[:5]).interpolate_na(np.full(5, np.nan), dim="node")


def test_coincident_points():
    rng = np.random.default_rng(14)
    sites = rng.random((700, 2))
    xy = sites[rng.integers(0, 700, 3000)]  # duplicated coordinates with different values
    null = rng.random(3000) < 0.5  # many nulls coincide with a valid point: distance 0
    src = assert_nearest(xy, null)
    same = np.all(xy[src[null]] == xy[null], axis=1)
    assert same.sum() > 100
    # all valid points on one spot: a zero-size box
    xy = np.vstack([np.full((50, 2), 0.25), rng.random((500, 2))])
    null = np.r_[np.zeros(50, dtype=bool), np.ones(500, dtype=bool)]
    src = assert_nearest(xy, null)
    assert (src[null] == 0).all()


def lattice(kind):
    if kind == "int_cell2":  # 21 x 21 integers, 200 valid: the search cell is exactly 2.0, so ties sit on cell edges
        i, j = np.meshgrid(np.arange(21.0), np.arange(21.0))
        xy = np.column_stack([i.ravel(), j.ravel()])
        null = np.ones(len(xy), dtype=bool)
        null[np.random.default_rng(15).permutation(len(xy))[:200]] = False
        return xy, null
    i, j = np.meshgrid(np.arange(50.0), np.arange(40.0))
    xy = np.column_stack([i.ravel(), j.ravel()])
    if kind == "tenth":
        xy = np.column_stack([i.ravel() * 0.1, j.ravel() * 0.1])
    elif kind == "rot30":
        th = np.radians(30.0)
        xy = xy @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T
    rng = np.random.default_rng(16)
    null = rng.random(len(xy)) < 0.5
    null[np.hypot(xy[:, 0] - xy[:, 0].mean(), xy[:, 1] - xy[:, 1].mean()) < 0.2 * np.ptp(xy[:, 0])] = True
    return xy, null


@pytest.mark.parametrize("kind", ["int", "int_cell2", "tenth", "rot30"])
def test_lattice_ties_every_null_point(kind):
    xy, null = lattice(kind)
    src = assert_nearest(xy, null)
    if kind in ("int", "int_cell2"):  # exact ties: check they are there, and resolved to the lowest index
        valid = np.nonzero(~null)[0]
        ties = 0
        for i in np.nonzero(null)[0]:
            d2 = ((xy[valid] - xy[i]) ** 2).sum(axis=1)
            ties += (d2 == d2.min()).sum() > 1
        assert ties > 50


@pytest.mark.parametrize("offset", [(155_000.0, 463_000.0), (500_000.0, 5_800_000.0)])
def test_large_offsets(offset):
    i, j = np.meshgrid(np.arange(60.0), np.arange(45.0))
    xy = np.column_stack([offset[0] + 0.5 * i.ravel(), offset[1] + 0.5 * j.ravel()])
    rng = np.random.default_rng(17)
    null = rng.random(len(xy)) < 0.5
    null[(i.ravel() > 20) & (i.ravel() < 32) & (j.ravel() > 10) & (j.ravel() < 30)] = True
    assert_nearest(xy, null)
    jittered = xy + rng.uniform(-0.2, 0.2, xy.shape)
    assert_nearest(jittered, null)


def test_max_distance_bound():
    i, j = np.meshgrid(np.arange(31.0), np.arange(31.0))
    xy = np.column_stack([i.ravel(), j.ravel()])
    null = (np.abs(xy[:, 0] - 15) <= 2) & (np.abs(xy[:, 1] - 15) <= 2)  # a 5 x 5 hole
    centre = np.nonzero((xy[:, 0] == 15) & (xy[:, 1] == 15))[0][0]
    grid = point_grid(xy)
    src, expected, _ = chosen(xy, null, 3.0, grid)  # the centre is exactly 3 from the nearest valid point
    assert np.array_equal(src, expected) and src[centre] == -1 and (src[null] >= 0).sum() > 0
    src, expected, _ = chosen(xy, null, np.nextafter(3.0, np.inf), grid)
    assert np.array_equal(src, expected) and src[centre] >= 0 and (src[null] >= 0).all()
    for d in (1.0, np.nextafter(1.0, np.inf), 2.0, np.sqrt(5.0), 2.5):
        src, expected, _ = chosen(xy, null, d, grid)
        assert np.array_equal(src, expected), d
    src, expected, _ = chosen(xy, null, 0.0, grid)  # fills nothing
    assert np.array_equal(src, expected) and (src[null] == -1).all()
    inf, _, _ = chosen(xy, null, np.inf, grid)
    none, _, _ = chosen(xy, null, None, grid)
    assert np.array_equal(inf, none) and (none[null] >= 0).all()


def test_values_are_copied_bit_for_bit():
    rng = np.random.default_rng(18)
    xy = rng.random((400, 2))
    grid = point_grid(xy)
    data = rng.normal(size=400)
    data[::7] = np.inf
    data[3::7] = -np.inf
    data[5::7] = -0.0
    null = rng.random(400) < 0.4
    data[null] = np.nan
    out = grid.interpolate_na(data, dim="node")
    src = brute_nearest(xy, data)
    assert (src >= 0).all()
    np.testing.assert_array_equal(out.view(np.int64), data[src].view(np.int64))
    assert np.signbit(out[np.nonzero(data[src] == 0)[0]]).any()
    f32 = grid.interpolate_na(data.astype(np.float32), dim="node")
    assert f32.dtype == np.float64
    np.testing.assert_array_equal(f32.view(np.int64), data.astype(np.float32).astype(np.float64)[src].view(np.int64))
    empty = grid.interpolate_na(np.zeros((0, 400)), dim="node")
    assert empty.shape == (0, 400) and empty.dtype == np.float64


@pytest.mark.parametrize("slice0_has_nan", [False, True])
def test_slice_grouping(slice0_has_nan):
    rng = np.random.default_rng(19)
    xy = rng.random((2500, 2))
    grid = point_grid(xy)
    data = rng.normal(size=(6, 2500))
    mask_a = rng.random(2500) < 0.3
    mask_b = np.hypot(xy[:, 0] - 0.4, xy[:, 1] - 0.6) < 0.3
    if slice0_has_nan:  # slice 0 masked like 1 and 2; 3 and 5 share another mask; 4 all valid
        masks = [mask_a, mask_a, mask_a, mask_b, None, mask_b]
    else:  # slice 0 all valid; 1 and 2 share a mask; 3 has slice 0's (none); 4 all valid; 5 its own
        masks = [None, mask_a, mask_a, None, None, mask_b]
    for k, m in enumerate(masks):
        if m is not None:
            data[k, m] = np.nan
    out = grid.interpolate_na(data, dim="node")
    for k in range(6):
        single = grid.interpolate_na(data[k], dim="node")
        assert np.array_equal(out[k].view(np.int64), single.view(np.int64)), k
        assert np.array_equal(out[k], data[k][brute_nearest(xy, data[k])]), k


def brute_fill(xy, data, max_distance):
    src = brute_nearest(xy, data, np.inf if max_distance is None else max_distance)
    return np.where(src >= 0, data[np.maximum(src, 0)], np.nan)


def test_nearest_fill_equals_brute_force_bit_for_bit():
    """The whole fill -- index of the valid points, lookup of the null ones, gather -- against the argmin of
    ``dx * dx + dy * dy`` over the valid points (lowest id on ties, strictly below ``max_distance``), from one point to
    several blocks.  The points sit on an integer lattice of about n / 2 sites: neighbours tie and points coincide at
    every size, and with ``max_distance`` one spacing only a coincident valid point may fill."""
    rng = np.random.default_rng(26)
    strict = 0
    for n in (1, 63, 64, 65, 257, 1500):
        side = int(np.ceil(np.sqrt(n / 2)))
        site = rng.integers(0, side * side, n)
        xy = np.column_stack([site % side, site // side]).astype(np.float64)
        assert n == 1 or len(np.unique(site)) < n
        grid = point_grid(xy)
        values = rng.normal(size=(3, n))
        half, other, single = rng.random(n) < 0.5, rng.random(n) < 0.5, np.ones(n, dtype=bool)
        for m in (half, other, single):
            m[rng.integers(0, n)] = False  # (at least one valid point; the only one of `single`)
        masks = {"half": half, "none": np.zeros(n, dtype=bool), "single": single}
        for max_distance in (None, 1.0):
            for name, null in masks.items():
                data = np.where(null, np.nan, values[0])
                out = grid.interpolate_na(data, dim="node", max_distance=max_distance)
                expected = brute_fill(xy, data, max_distance)
                assert np.array_equal(out.view(np.int64), expected.view(np.int64)), (n, name, max_distance)
                if max_distance is not None:  # nulls whose nearest valid point is exactly one spacing away stay null
                    at_bound = null & ~np.isnan(brute_fill(xy, data, None)) & np.isnan(expected)
                    at_bound &= ~np.isnan(brute_fill(xy, data, np.nextafter(1.0, 2.0)))
                    strict += int(at_bound.sum())
            batch = np.where(np.stack([half, other, half]), np.nan, values)  # slices 0 and 2 share a mask, 1 has its own
            out = grid.interpolate_na(batch, dim="node", max_distance=max_distance)
            expected = np.stack([brute_fill(xy, b, max_distance) for b in batch])
            assert np.array_equal(out.view(np.int64), expected.view(np.int64)), (n, "batch", max_distance)
    assert strict > 100
    # two coincident valid points (ids 2 and 4) with different values: the null on them and the null beside them take the
    # lower id's value, each valid point keeps its own
    xy = np.array([[5.0, 5.0], [1.0, 0.0], [0.0, 0.0], [9.0, 2.0], [0.0, 0.0], [0.0, 0.0]])
    data = np.array([1.5, np.nan, 20.0, -3.0, 10.0, np.nan])
    out = point_grid(xy).interpolate_na(data, dim="node")
    assert np.array_equal(out.view(np.int64), np.array([1.5, 20.0, 20.0, -3.0, 10.0, 20.0]).view(np.int64))
    assert np.array_equal(out.view(np.int64), brute_fill(xy, data, None).view(np.int64))


# ---- Laplace: component labels, CG iterates, spsolve on harder systems
def csr(rows, cols, n):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    m = sparse.coo_matrix((np.ones(2 * rows.size), (np.r_[rows, cols], np.r_[cols, rows])), shape=(n, n)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


def label_graphs():
    rng = np.random.default_rng(20)
    n = 200_000
    i = np.arange(n - 1)
    yield "chain reversed", csr(n - 1 - i, n - 2 - i, n)  # node n-1 - node n-2 - ... - node 0
    perm = rng.permutation(n)
    yield "chain permuted", csr(perm[i], perm[i + 1], n)
    # a forest of many small trees (1 - 30 nodes), node ids permuted
    sizes = rng.integers(1, 31, 20_000)
    starts = np.r_[0, np.cumsum(sizes)[:-1]]
    n = int(sizes.sum())
    child = np.arange(n)
    tree = np.repeat(np.arange(sizes.size), sizes)
    parent = starts[tree] + (rng.random(n) * (child - starts[tree])).astype(np.int64)
    keep = child != starts[tree]
    perm = rng.permutation(n)
    yield "forest", csr(perm[child[keep]], perm[parent[keep]], n)
    # isolated nodes among a few edges
    n = 5000
    a = rng.integers(0, n, 800)
    b = rng.integers(0, n, 800)
    yield "isolated", csr(a[a != b], b[a != b], n)
    yield "no edges", csr([], [], 1000)
    n = 50_000
    yield "star", csr(np.full(n - 1, n - 1), np.arange(n - 1), n)  # the centre has the largest id
    grid, _ = mesh_with_patch()
    conn = grid.face_face_connectivity.copy()
    conn.data[:] = 1.0  # (the data are edge ids, 0 among them)
    yield "mesh_with_patch faces", conn


def test_component_labels_match_scipy():
    for name, conn in label_graphs():
        ncomp, lab = csgraph.connected_components(conn, directed=False)
        smallest = np.full(ncomp, conn.shape[0], dtype=np.int64)
        np.minimum.at(smallest, lab, np.arange(conn.shape[0]))
        t0 = time.perf_counter()
        labels = fill.DeviceGraph(conn).labels()
        dt = time.perf_counter() - t0
        assert np.array_equal(labels, smallest[lab]), name
        print(f"labels {name}: {conn.shape[0]} nodes, {ncomp} components, {dt * 1e3:.1f} ms")


def holed_mesh(n_points=1000, seed=0, radius=0.3):
    xy, faces = meshgen.triangle_mesh(n_points, seed)
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    c = grid.centroids
    data = np.sin(3 * c[:, 0]) + np.cos(2 * c[:, 1])
    data[np.hypot(c[:, 0] - 0.45, c[:, 1] - 0.55) < radius] = np.nan
    return grid, data


def fill_recorded(grid, data, **kw):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = grid.laplace_interpolate(data, **kw)
    return out, [w for w in caught if issubclass(w.category, UserWarning)]


# the largest relative difference (max-norm) allowed between a device CG iterate and the host's after the same number of
# iterations.  The summation order of the dot products differs, so the iterates cannot be bit-equal; measured on the
# MI355X: 2.8e-15 at worst over the maxiter values below
ITERATE_RTOL = 1e-13


def test_cg_iterates_match_scipy_loop():
    grid, data = holed_mesh()
    conn = grid.get_connectivity_matrix("face", xy_weights=True)
    A, b, scale, unknown = scaled_system(data, conn, csgraph.connected_components(conn)[1], True)
    assert unknown.sum() > 400
    worst = 0.0
    for maxiter in (1, 2, 5, 23, 24, 25, 48, 49, 500):
        iterates, info, norms, tol = reference_cg(A, b, atol=1e-4, rtol=0.0, maxiter=maxiter)
        out, caught = fill_recorded(grid, data, maxiter=maxiter)
        host_iters, dev_iters = len(iterates) - 1, int(fill.last_iterations[0])
        if dev_iters != host_iters:  # only where the host's deciding residual sits on the tolerance itself
            decide = norms[min(dev_iters, host_iters)]
            assert abs(decide - tol) <= 1e-9 * tol, (maxiter, dev_iters, host_iters, decide, tol)
            continue
        expected = scale * iterates[-1]
        rel = np.abs(out[unknown] - expected).max() / np.abs(expected).max()
        worst = max(worst, rel)
        assert rel <= ITERATE_RTOL, (maxiter, rel)
        assert np.array_equal(out[~unknown], data[~unknown])
        assert len(caught) == (1 if info else 0), (maxiter, [str(w.message) for w in caught])
        if info:
            assert str(caught[0].message) == f"Failed to converge after {maxiter} iterations"
        else:
            assert maxiter == 500 and 49 < host_iters < 500
    print(f"CG iterates: worst relative difference to the host loop {worst:.2e} (bound {ITERATE_RTOL:.0e})")


def test_node_dimension_with_xy_weights_matches_spsolve():
    xy, faces = meshgen.mixed_mesh(3000, 5)
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    p = grid.node_coordinates
    data = np.sin(4 * p[:, 0]) * np.cos(3 * p[:, 1])
    rng = np.random.default_rng(21)
    data[rng.random(len(data)) < 0.2] = np.nan
    data[np.hypot(p[:, 0] - 0.3, p[:, 1] - 0.7) < 0.15] = np.nan
    conn = grid.get_connectivity_matrix("node", xy_weights=True)
    expected = reference_laplace(data, conn, True)
    out = grid.laplace_interpolate(data, dim="node", xy_weights=True, direct_solve=True)
    np.testing.assert_allclose(out, expected, rtol=1e-9, atol=1e-9)


def test_graded_mesh_matches_spsolve():
    """Rings of nodes from r = 1e-4 to 1 (spacing ~ r): cells of every size, weights mean(d)/d over more than 10^3."""
    radii = np.geomspace(1e-4, 1.0, 37)
    theta = np.linspace(0.0, 2 * np.pi, 24, endpoint=False)
    pts = [np.zeros((1, 2))]
    for k, r in enumerate(radii):
        a = theta + (np.pi / 24) * (k % 2)
        pts.append(np.column_stack([r * np.cos(a), r * np.sin(a)]))
    xy = np.vstack(pts)
    faces = Delaunay(xy).simplices.astype(np.int64)
    u, v = xy[faces[:, 1]] - xy[faces[:, 0]], xy[faces[:, 2]] - xy[faces[:, 0]]
    cw = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0] < 0
    faces[cw] = faces[cw][:, ::-1]
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    conn = grid.get_connectivity_matrix("face", xy_weights=True)
    assert conn.data.max() / conn.data.min() >= 1e3
    c = grid.centroids
    r = np.hypot(c[:, 0], c[:, 1])
    data = np.log(r) + c[:, 0]
    data[(r > 3e-4) & (r < 0.3) & (c[:, 1] > -0.5 * r)] = np.nan  # a hole across the grading
    data[np.random.default_rng(22).random(len(data)) < 0.1] = np.nan
    expected = reference_laplace(data, conn, True)
    out = grid.laplace_interpolate(data, xy_weights=True, direct_solve=True)
    np.testing.assert_allclose(out, expected, rtol=1e-9, atol=1e-9)


def branched_network():
    """A tree of three branches, an all-NaN chain, an isolated valid node, an isolated NaN node, and a chain with one
    known value."""
    xy, edges, values = [], [], []

    def chain(points, vals):
        base = len(xy)
        xy.extend(points)
        values.extend(vals)
        edges.extend([base + i, base + i + 1] for i in range(len(points) - 1))
        return base

    rng = np.random.default_rng(23)
    s = np.linspace(0.0, 10.0, 101)
    v = np.cos(s)
    v[rng.random(v.size) < 0.3] = np.nan
    v[40:60] = np.nan
    trunk = chain([(x, 0.0) for x in s], v)
    for at, sign in ((30, 1.0), (70, -1.0)):
        h = np.linspace(0.15, 4.0, 26)
        v = np.sin(h) + sign
        v[rng.random(v.size) < 0.3] = np.nan
        v[-5:] = np.nan  # the branch's free end
        b = chain([(s[at] + 0.3 * t, sign * t) for t in h], v)
        edges.append([trunk + at, b])
    all_nan = chain([(x, 5.0) for x in np.linspace(0.0, 3.0, 10)], [np.nan] * 10)
    iso_valid = chain([(20.0, 20.0)], [4.5])
    iso_nan = chain([(21.0, 20.0)], [np.nan])
    one = chain([(x, -8.0 + 0.1 * x * x) for x in np.linspace(0.0, 5.0, 15)], [np.nan] * 7 + [2.75] + [np.nan] * 7)
    xy = np.array(xy)
    grid = xa.Ugrid1d(xy[:, 0], xy[:, 1], -1, np.array(edges))
    return grid, np.array(values, dtype=np.float64), all_nan, iso_valid, iso_nan, one


def test_branched_network_matches_spsolve():
    grid, data, all_nan, iso_valid, iso_nan, one = branched_network()
    conn = grid.get_connectivity_matrix("node", xy_weights=True)
    assert csgraph.connected_components(conn)[0] == 5
    expected = reference_laplace(data, conn, True)
    out = grid.laplace_interpolate(data, direct_solve=True)
    np.testing.assert_allclose(out, expected, rtol=1e-9, atol=1e-9)
    assert np.isnan(out[all_nan:all_nan + 10]).all() and np.isnan(out[iso_nan])
    assert out[iso_valid] == 4.5
    np.testing.assert_allclose(out[one:one + 15], 2.75, rtol=1e-9)
    assert not np.isnan(out[:all_nan]).any()


def test_mixed_statuses_in_one_batch():
    grid, data = holed_mesh()
    c = grid.centroids
    conn = grid.get_connectivity_matrix("face", xy_weights=True)
    labels = csgraph.connected_components(conn)[1]
    small = np.sin(3 * c[:, 0]) + np.cos(2 * c[:, 1])
    small[np.hypot(c[:, 0] - 0.7, c[:, 1] - 0.3) < 0.08] = np.nan
    counts = {}
    for name, d in (("small", small), ("big", data)):
        A, b, _, _ = scaled_system(d, conn, labels, True)
        counts[name] = len(reference_cg(A, b, atol=1e-4, rtol=0.0, maxiter=1000)[0]) - 1
    assert counts["small"] + 4 < counts["big"], counts
    maxiter = (counts["small"] + counts["big"]) // 2
    zeros = np.where(np.isnan(data), np.nan, 0.0)  # every known value 0: b = 0, x = 0 at once
    batch = np.stack([1.5 + c[:, 0], zeros, small, data])
    out, caught = fill_recorded(grid, batch, maxiter=maxiter)
    iters = fill.last_iterations.copy()
    assert len(caught) == 1 and str(caught[0].message) == f"Failed to converge after {maxiter} iterations"
    assert iters[0] == 0 and iters[1] == 0 and iters[3] == maxiter and 0 < iters[2] < maxiter, (iters, counts)
    assert np.array_equal(out[0], batch[0])
    assert (out[1] == 0.0).all()
    for k in range(4):
        single, w = fill_recorded(grid, batch[k], maxiter=maxiter)
        assert np.array_equal(out[k].view(np.int64), single.view(np.int64)), k
        assert int(fill.last_iterations[0]) == iters[k] and len(w) == (k == 3), k


# ---- more slices than one launch grid holds (the kernels take at most 65 535 per call)
K_BIG = 70_000
OWN_MASK = (5, 33_333, 65_534, 65_536, 69_999)  # slices with a NaN mask of their own (not at a tile's first slice)
SAMPLE = sorted(set(OWN_MASK) | {0, 1, 65_533, 65_535, 65_537} | set(np.random.default_rng(24).integers(0, K_BIG, 10)))


def big_stack(n_points=150):
    xy, faces = meshgen.triangle_mesh(n_points, 3)
    grid = xa.Ugrid2d(xy[:, 0], xy[:, 1], -1, faces)
    c = grid.centroids
    base = np.sin(3 * c[:, 0]) + np.cos(2 * c[:, 1])
    data = base[None, :] + 1e-3 * np.arange(K_BIG, dtype=np.float64)[:, None]
    rng = np.random.default_rng(25)
    mask = np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) < 0.2
    mask |= rng.random(grid.n_face) < 0.1
    data[:, mask] = np.nan
    for k in OWN_MASK:
        data[k, rng.random(grid.n_face) < 0.25] = np.nan
    return grid, data


def test_more_slices_than_one_launch_grid():
    grid, data = big_stack()
    assert grid.n_face > 250
    near = grid.interpolate_na(data)
    lap = grid.laplace_interpolate(data)
    iters = fill.last_iterations
    assert near.shape == lap.shape == data.shape and iters.shape == (K_BIG,)
    assert not np.isnan(near).any() and not np.isnan(lap).any()
    for k in SAMPLE:
        assert np.array_equal(near[k].view(np.int64), grid.interpolate_na(data[k]).view(np.int64)), k
        assert np.array_equal(lap[k].view(np.int64), grid.laplace_interpolate(data[k]).view(np.int64)), k
        assert iters[k] == fill.last_iterations[0], k
