"""
GPU (-m gpu): the layered (3-D) overlap weights built on the device (csrc/xr_layered.hip through ``DeviceCSR.layered``,
``LayeredOverlapRegridder`` and ``overlap_1d_nd``) against the numpy restatement of the rule (tests/layered_cases.py): every
matrix and every triplet array bit for bit, order included.  The 2-D weights are the device's own, downloaded; the
restatement is pinned on the CPU (tests/test_layered_cpu.py) to the reference's recorded output and to a brute force.
"""
import numpy as np
import pytest

import layered_cases as C
from conftest import same_or_nan
from xugrid_amd import meshgen
from xugrid_amd.engine import DeviceArray, DeviceCSR

pytestmark = pytest.mark.gpu

# (33, 2), (2, 33): rows and items of more than 32 entries; 65: past a wave; 8, 9, 16, 17: the edges of the tiles of eight source
# layers a thread holds at a time (xr_layered.hip: SOURCE_TILE)
LAYER_COUNTS = [(1, 1), (2, 3), (33, 2), (2, 33), (65, 3), (8, 2), (9, 2), (16, 3), (17, 3)]
# the apply tolerances of tests/test_gpu_parity.py (assert_apply_equal, test_apply_golden_g2): rows of up to 32 entries are
# reduced sequentially -- bit for bit; longer rows cooperatively in a fixed tree order; geometric_mean: device exp / log
LONG_ROW, RTOL_LONG, RTOL_GEOMETRIC = 32, 1e-13, 1e-13


def assert_apply_equal(got, exp, indptr, name):
    assert got.shape == exp.shape and got.dtype == np.float64
    if name == "geometric_mean":
        np.testing.assert_allclose(got, exp, rtol=RTOL_GEOMETRIC, equal_nan=True)
        return
    long_rows = np.diff(indptr) > LONG_ROW
    assert same_or_nan(got[:, ~long_rows], exp[:, ~long_rows]).all(), name
    if long_rows.any():
        rtol = 1e-9 if name == "harmonic_mean" else RTOL_LONG
        finite = exp[:, long_rows][np.isfinite(exp[:, long_rows])]
        atol = 1e-13 * (np.abs(finite).max() if finite.size else 1.0)
        np.testing.assert_allclose(got[:, long_rows], exp[:, long_rows], rtol=rtol, atol=atol, equal_nan=True, err_msg=name)


@pytest.fixture(scope="module")
def pair(hip):
    """~290 -> ~240 triangles and a raster target, with the 2-D regridders and their downloaded weights (built once)."""
    sxy, sf = meshgen.triangle_mesh(169, 0)
    txy, tf = meshgen.triangle_mesh(144, 1, 30.0, 0.7)
    source = hip.Ugrid2d(sxy[:, 0], sxy[:, 1], -1, sf)
    target = hip.Ugrid2d(txy[:, 0], txy[:, 1], -1, tf)
    raster = hip.Raster(np.linspace(0.2, 0.8, 13), np.linspace(0.75, 0.25, 11))
    out = {"source": source, "target": target, "raster_grid": raster, "n_s": source.n_face, "n_t": target.n_face, "n_r": 11 * 13}
    for name, cls, tgt in (("mesh", hip.OverlapRegridder, target), ("raster", hip.OverlapRegridder, raster),
                           ("relative", hip.RelativeOverlapRegridder, target)):
        rg = cls(source, tgt)
        w = rg._ensure_host_weights()
        assert w.nnz > 0
        out[name] = rg
        out[name + "_w"] = (w.indptr, w.indices, w.data)
    return out


def assert_matrix(device_weights, expected):
    data, indices, indptr, n, m = expected
    got_data, got_indices, got_indptr = device_weights.download()
    assert (device_weights.n, device_weights.m, device_weights.nnz) == (n, m, data.size)
    assert np.array_equal(got_indptr, indptr) and np.array_equal(got_indices, indices)
    assert np.array_equal(got_data, data)
    # the rows of more than 32 entries are listed for the cooperative reducers
    assert np.array_equal(np.sort(device_weights.long_rows()), np.flatnonzero(np.diff(indptr) > LONG_ROW))


def layered(hip, pair, which, bounds, relative=False):
    cls = hip.LayeredRelativeOverlapRegridder if relative else hip.LayeredOverlapRegridder
    rg = cls.from_regridder(pair[which], *bounds)
    return rg, C.layered_csr(*pair[which + "_w"], pair["n_s"], *bounds, relative=relative)


@pytest.mark.parametrize("n_layer_s,n_layer_t", LAYER_COUNTS)
def test_matrix_equals_restatement(hip, pair, n_layer_s, n_layer_t):
    bounds = C.columns(1, pair["n_s"], n_layer_s, "shared") + C.columns(2, pair["n_t"], n_layer_t, "shared")
    rg, exp = layered(hip, pair, "mesh", bounds)
    assert_matrix(rg._device_weights, exp)
    if (n_layer_s, n_layer_t) == (33, 2):
        assert (np.diff(exp[2]) > LONG_ROW).any()


@pytest.mark.parametrize("kind_s,kind_t", [("ragged", "nan"), ("nan", "descending"), ("shuffled", "ragged"), ("descending", "shuffled"),
                                           ("nan", "nan")])
def test_any_layer_order_nan_and_zero_thickness(hip, pair, kind_s, kind_t):
    bounds = C.columns(3, pair["n_s"], 5, kind_s) + C.columns(4, pair["n_t"], 4, kind_t)
    rg, exp = layered(hip, pair, "mesh", bounds)
    assert exp[0].size > 0
    assert_matrix(rg._device_weights, exp)
    # device arrays in (two of them: the host ones are uploaded), the same matrix out
    mixed = (DeviceArray.from_host(bounds[0]), bounds[1], bounds[2], DeviceArray.from_host(bounds[3]))
    assert_matrix(hip.LayeredOverlapRegridder.from_regridder(pair["mesh"], *mixed)._device_weights, exp)
    assert_matrix(hip.LayeredOverlapRegridder.from_regridder(pair["mesh"], *(DeviceArray.from_host(b) for b in bounds))._device_weights, exp)


def test_constructor_builds_the_2d_weights_of_the_pair(hip, pair):
    bounds = C.columns(5, pair["n_s"], 3, "shared") + C.columns(6, pair["n_t"], 2, "ragged")
    rg = hip.LayeredOverlapRegridder(hip.LayeredGrid(pair["source"], *bounds[:2]), hip.LayeredGrid(pair["target"], *bounds[2:]))
    assert_matrix(rg._device_weights, C.layered_csr(*pair["mesh_w"], pair["n_s"], *bounds))
    # a pure re-layering: the same grid on both sides, through the same path
    again = hip.LayeredOverlapRegridder(hip.LayeredGrid(pair["source"], *bounds[:2]),
                                        hip.LayeredGrid(pair["source"], *C.columns(7, pair["n_s"], 4, "shared")))
    w = hip.OverlapRegridder(pair["source"], pair["source"])._ensure_host_weights()
    assert_matrix(again._device_weights, C.layered_csr(w.indptr, w.indices, w.data, pair["n_s"], *bounds[:2],
                                                       *C.columns(7, pair["n_s"], 4, "shared")))


def test_raster_pair(hip, pair):
    """raster -> raster: the 2-D weights are the factored ones, taken as their materialised product"""
    source = hip.Raster(np.linspace(0.05, 0.95, 10), np.linspace(0.9, 0.1, 9))
    rg2d = hip.OverlapRegridder(source, pair["raster_grid"])
    w = rg2d._ensure_host_weights()
    top_s, bottom_s = (b.reshape(9, 9, 10) for b in C.columns(32, 90, 9, "nan"))
    top_t, bottom_t = C.columns(33, pair["n_r"], 3, "descending")
    rg = hip.LayeredOverlapRegridder(hip.LayeredGrid(source, top_s, bottom_s), hip.LayeredGrid(pair["raster_grid"], top_t, bottom_t))
    assert_matrix(rg._device_weights, C.layered_csr(w.indptr, w.indices, w.data, 90, top_s, bottom_s, top_t, bottom_t))
    assert rg.regrid(np.ones((2, 9, 9, 10))).shape == (2, 3, 11, 13)


def test_relative_weights(hip, pair):
    bounds = C.columns(8, pair["n_s"], 4, "ragged") + C.columns(9, pair["n_t"], 3, "shuffled")
    rg, exp = layered(hip, pair, "relative", bounds, relative=True)
    assert_matrix(rg._device_weights, exp)
    assert rg._method.name == "first_order_conservative"


def test_empty_matrix_and_empty_rows_at_both_ends(hip, pair):
    n_s, n_t = pair["n_s"], pair["n_t"]
    target = C.columns(10, n_t, 3, "shared")
    nothing = (np.full((2, n_s), np.nan), np.full((2, n_s), np.nan)) + target
    rg, exp = layered(hip, pair, "mesh", nothing)
    assert exp[0].size == 0
    assert_matrix(rg._device_weights, exp)
    assert np.isnan(rg.regrid(np.ones((2, n_s)))).all()
    # target layers above and below every source layer (first and last rows empty), uniform layering on the target
    source = C.columns(11, n_s, 4, "shared")
    uniform = (np.array([50.0, 40.0, 7.25, 0.0]), np.array([40.0, 7.25, 0.0, -3.0]))
    rg, exp = layered(hip, pair, "mesh", source + uniform)
    lengths = np.diff(exp[2]).reshape(4, n_t)
    assert (lengths[0] == 0).all() and (lengths[3] == 0).all() and lengths[1:3].any()
    assert_matrix(rg._device_weights, exp)
    # ... on the source, and on both sides, as device arrays too
    rg, exp = layered(hip, pair, "mesh", uniform + target)
    assert_matrix(rg._device_weights, exp)
    assert_matrix(pair["mesh"]._device_weights.layered(*(DeviceArray.from_host(u) for u in uniform + uniform)),
                  C.layered_csr(*pair["mesh_w"], n_s, *(uniform + uniform)))
    # one column without any layer on each side
    holed = [b.copy() for b in source + target]
    holed[0][:, 5] = holed[1][:, 5] = holed[2][:, 7] = holed[3][:, 7] = np.nan
    rg, exp = layered(hip, pair, "mesh", tuple(holed))
    assert exp[2][7] == exp[2][8]
    assert_matrix(rg._device_weights, exp)


def test_touching_layers(hip):
    w2 = DeviceCSR.from_arrays([2.0], [0], [0, 1], 1, 1)
    assert_matrix(w2.layered(*C.touching()), C.layered_csr([0, 1], [0], [2.0], 1, *C.touching()))


@pytest.mark.parametrize("n_layer_t,nnz2d", [(1, 2047), (1, 2048), (1, 2049), (23, 89), (32, 64), (3, 683)])
def test_item_counts_at_the_scan_tile(hip, n_layer_t, nnz2d):
    """count arrays of 2047, 2048 and 2049 items: the tile of the exclusive scan that turns them into offsets"""
    assert n_layer_t * nnz2d in (2047, 2048, 2049)
    n_t, n_s = 61, 47
    data2, indices2, indptr2 = C.random_csr(nnz2d, n_t, n_s, nnz2d)
    bounds = C.columns(12, n_s, 3, "ragged") + C.columns(13, n_t, n_layer_t, "ragged")
    w2 = DeviceCSR.from_arrays(data2, indices2, indptr2, n_t, n_s)
    assert_matrix(w2.layered(*bounds), C.layered_csr(indptr2, indices2, data2, n_s, *bounds))


def test_stored_order_of_the_2d_weights_does_not_matter(hip):
    """rows regrouped by keys and columns renumbered inside the 2-D handle: the matrix is read in the caller's ids"""
    n_t, n_s = 5000, 4100
    data2, indices2, indptr2 = C.random_csr(14, n_t, n_s, 9000)
    rng = np.random.default_rng(14)
    w2 = DeviceCSR.from_arrays(data2, indices2, indptr2, n_t, n_s)
    w2.set_row_keys(rng.integers(0, 16, n_t), 16)
    w2.set_col_keys(rng.integers(0, 16, n_s), 16)
    w2.apply(np.ones((8, n_s)))  # (eight variables: the rows are regrouped now)
    bounds = C.columns(15, n_s, 2, "ragged") + C.columns(16, n_t, 2, "nan")
    assert_matrix(w2.layered(*bounds), C.layered_csr(indptr2, indices2, data2, n_s, *bounds))


def test_int32_limits(hip):
    """sizes that leave the 32-bit internals raise OverflowError (XR_ERR_LIMIT): the products before anything is launched, the
    entry count -- known behind the count pass only -- from a 64-bit sum where the scan of the counts could wrap"""
    n_t, n_s = 61, 47
    data2, indices2, indptr2 = C.random_csr(40, n_t, n_s, 2000)
    w2 = DeviceCSR.from_arrays(data2, indices2, indptr2, n_t, n_s)
    n_layer = 1040  # 2000 entries x 1040 x 1040 layer pairs >= 2^31
    top, bottom = np.arange(1.0, n_layer + 1), np.arange(0.0, n_layer)
    # the same layering on both sides: every item has one entry, the 64-bit sum lets the build through
    data, indices, indptr = w2.layered(top, bottom, top, bottom).download()
    assert np.array_equal(data, np.tile(data2, n_layer))  # (w * 1.0)
    assert np.array_equal(indices, (np.arange(n_layer)[:, None] * n_s + indices2[None, :]).ravel())
    assert np.array_equal(indptr, (np.arange(n_layer)[:, None] * 2000 + indptr2[None, :-1]).ravel().tolist() + [2000 * n_layer])
    # every target layer spans the whole source column: 2000 x 1040 x 1040 entries
    with pytest.raises(OverflowError, match="entries"):
        w2.layered(top, bottom, np.full(n_layer, float(n_layer)), np.zeros(n_layer))
    many = 2 ** 31 // 2000 + 1
    with pytest.raises(OverflowError, match="target layers"):
        w2.layered(top, bottom, np.zeros(many), np.zeros(many))
    with pytest.raises(OverflowError, match="source"):
        w2.layered(np.zeros(2 ** 31 // n_s + 1), np.zeros(2 ** 31 // n_s + 1), top, bottom)


# ---- overlap_1d_nd --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"shared_{a}_{b}" for a, b in C.GOLDEN_LAYERS] + ["reference_test"])
def test_overlap_1d_nd_equals_the_reference(hip, name):
    case = C.load_golden()[name]
    s, t, w = hip.overlap_1d_nd(case["source_bounds"], case["target_bounds"], case["source_index"], case["target_index"])
    assert np.array_equal(s, case["source"]) and np.array_equal(t, case["target"]) and np.array_equal(w, case["overlap"])


def test_overlap_1d_nd_any_number_of_pairs(hip):
    sb = C.to_bounds(*C.columns(17, 9, 33, "nan"))
    tb = C.to_bounds(*C.columns(18, 4, 7, "shuffled"))
    rng = np.random.default_rng(17)
    for o in (0, 1, 3, 4, 300):  # (fewer and more pairs than target columns; 300 x 7 items: past one scan tile)
        si, ti = rng.integers(0, 9, o), rng.integers(0, 4, o)
        got, exp = hip.overlap_1d_nd(sb, tb, si, ti), C.pair_triplets(sb, tb, si, ti)
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)) and got[0].dtype.kind == "i" and got[2].dtype == np.float64
    assert exp[0].size > 300
    on_device = hip.overlap_1d_nd(DeviceArray.from_host(sb), DeviceArray.from_host(tb), si, ti)
    assert all(isinstance(a, DeviceArray) and np.array_equal(a.download(), b) for a, b in zip(on_device, exp))
    with pytest.raises(ValueError, match="outside"):
        hip.overlap_1d_nd(sb, tb, np.array([0, 9]), np.array([0, 1]))
    with pytest.raises(ValueError, match="source_bounds"):
        hip.overlap_1d_nd(sb[..., :1], tb, si, ti)
    with pytest.raises(ValueError, match="target_index"):
        hip.overlap_1d_nd(sb, tb, si, ti[:-1])


# ---- regrid ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def applied(hip, pair):
    """the regridders of the apply tests with the oracle's inputs: a mesh and a raster target, rows of more than 32 entries"""
    out = {}
    for which, n_t in (("mesh", pair["n_t"]), ("raster", pair["n_r"])):
        top_t, bottom_t = C.columns(20, n_t, 2, "shared")
        if which == "raster":
            top_t, bottom_t = top_t.reshape(2, 11, 13), bottom_t.reshape(2, 11, 13)
        bounds = C.columns(19, pair["n_s"], 12, "nan") + (top_t, bottom_t)
        out[which] = layered(hip, pair, which, bounds)
    rng = np.random.default_rng(21)
    data = rng.uniform(0.5, 2.0, (3, 12, pair["n_s"]))
    data[rng.random(data.shape) < 0.05] = np.nan
    out["data"] = data
    return out


@pytest.mark.parametrize("method", ["mean", "harmonic_mean", "geometric_mean", "sum", "minimum", "maximum", "mode", "median",
                                    "max_overlap", "p5", "p10", "p25", "p50", "p75", "p90", "p95"])
def test_regrid_every_reducer(hip, oracle, pair, applied, method):
    for which, shape in (("mesh", (2, pair["n_t"])), ("raster", (2, 11, 13))):
        rg, (data, indices, indptr, n, m) = applied[which]
        rg._setup_regrid(method)
        assert which == "raster" or ((np.diff(indptr) > LONG_ROW).any() and (np.diff(indptr) <= LONG_ROW).any())
        for dtype in (np.float64, np.float32):
            src = applied["data"].astype(dtype)
            exp3 = oracle.regrid_csr(method, src.reshape(3, m), data, indices, indptr, n)
            got3 = rg.regrid(src)  # K = 3
            assert got3.shape == (3,) + shape
            assert_apply_equal(got3.reshape(3, n), exp3, indptr, method)
            got1 = rg.regrid(src[1])  # K = 1: no leading dimension
            assert got1.shape == shape
            assert_apply_equal(got1.reshape(1, n), exp3[1:2], indptr, method)
    on_device = rg.regrid(DeviceArray.from_host(src))
    assert isinstance(on_device, DeviceArray) and np.array_equal(on_device.download(), got3, equal_nan=True)


def test_relative_regrid(hip, oracle, pair):
    bounds = C.columns(22, pair["n_s"], 3, "shared") + C.columns(23, pair["n_t"], 4, "shared")
    for method in ("first_order_conservative", "conductance"):
        rg = hip.LayeredRelativeOverlapRegridder.from_regridder(pair["relative"], *bounds, method=method)
        data, indices, indptr, n, m = C.layered_csr(*pair["relative_w"], pair["n_s"], *bounds, relative=True)
        src = np.random.default_rng(24).uniform(1.0, 2.0, (2, 3, pair["n_s"]))
        exp = oracle.regrid_csr(method, src.reshape(2, m), data, indices, indptr, n)
        assert_apply_equal(rg.regrid(src).reshape(2, n), exp, indptr, method)


def test_adjoint_of_the_mean_is_the_dense_transpose(hip, pair):
    bounds = C.columns(25, pair["n_s"], 1, "shared") + C.columns(26, pair["n_t"], 1, "shared")
    rg, (data, indices, indptr, n, m) = layered(hip, pair, "mesh", bounds)
    dense = np.zeros((n, m))
    dense[np.repeat(np.arange(n), np.diff(indptr)), indices] = data  # (a pair of faces has one entry)
    grad = np.random.default_rng(27).normal(size=(2, 1, pair["n_t"]))
    live = np.diff(indptr) > 0
    row_sum = np.add.reduceat(np.append(data, 0.0), indptr[:-1]) * live
    r = np.where(live, grad.reshape(2, n) / np.where(live, row_sum, 1.0), 0.0)
    got = rg.regrid_adjoint(grad)
    assert got.shape == (2, 1, pair["n_s"])
    # a column sums its entries in one fixed order, the dense product in another: (entries + 2) roundings of the sum of
    # the absolute terms; the row sums themselves differ from the device's sequential ones by as many
    entries = np.bincount(indices, minlength=m).max() + np.diff(indptr).max() + 4
    bound = entries * 2.0 ** -52 * (np.abs(r) @ np.abs(dense))
    assert (np.abs(got.reshape(2, m) - r @ dense) <= bound).all() and np.abs(got).max() > 0


def test_dataset_round_trip(hip, pair, tmp_path):
    for which in ("mesh", "raster"):
        n_t = pair["n_t"] if which == "mesh" else pair["n_r"]
        bounds = C.columns(28, pair["n_s"], 3, "nan") + C.columns(29, n_t, 2, "descending")
        rg, exp = layered(hip, pair, which, bounds)
        ds = rg.to_dataset()
        again = hip.LayeredOverlapRegridder.from_weights(ds, rg._target, method="sum")
        restored = hip.LayeredOverlapRegridder.from_dataset(ds)
        path = str(tmp_path / f"{which}.npz")
        rg.to_file(path)
        from_file = hip.LayeredOverlapRegridder.from_file(path)
        src = np.random.default_rng(30).uniform(size=(3, pair["n_s"]))
        rg._setup_regrid("sum")
        out = rg.regrid(src)
        for other in (again, restored, from_file):
            assert_matrix(other._ensure_device_weights(), exp)
            assert other._source.shape == rg._source.shape and other._target.shape == rg._target.shape
            assert np.array_equal(other._target.top, rg._target.top, equal_nan=True)
            other._setup_regrid("sum")
            assert np.array_equal(other.regrid(src), out, equal_nan=True)


def test_errors(hip, pair):
    n_s, n_t = pair["n_s"], pair["n_t"]
    top, bottom = C.columns(31, n_s, 3, "shared")
    with pytest.raises(ValueError, match="top"):
        hip.LayeredGrid(pair["source"], top[:, :-1], bottom[:, :-1])  # n_face mismatch
    with pytest.raises(ValueError, match="bottom"):
        hip.LayeredGrid(pair["source"], top, bottom[:2])
    with pytest.raises(ValueError, match="top"):
        hip.LayeredGrid(pair["raster_grid"], np.zeros((2, 13, 11)), np.zeros((2, 13, 11)))  # (ny, nx) swapped
    with pytest.raises(ValueError, match="top"):
        hip.LayeredOverlapRegridder.from_regridder(pair["mesh"], top, bottom, top, bottom)  # the target has n_t faces
    with pytest.raises(ValueError, match="top_s"):
        pair["mesh"]._device_weights.layered(top[:, :-1], bottom[:, :-1], top[:, :n_t], bottom[:, :n_t])
    with pytest.raises(TypeError, match="LayeredGrid"):
        hip.LayeredOverlapRegridder(pair["source"], pair["target"])
    locator = hip.CentroidLocatorRegridder(pair["source"], pair["target"])
    with pytest.raises(TypeError, match="OverlapRegridder"):
        hip.LayeredOverlapRegridder.from_regridder(locator, top, bottom, top[:, :n_t], bottom[:, :n_t])
    with pytest.raises(TypeError, match="RelativeOverlapRegridder"):
        hip.LayeredRelativeOverlapRegridder.from_regridder(pair["mesh"], top, bottom, top[:, :n_t], bottom[:, :n_t])
    rg = hip.LayeredOverlapRegridder.from_regridder(pair["mesh"], top, bottom, top[:, :n_t], bottom[:, :n_t])
    with pytest.raises(ValueError, match="source dimensions"):
        rg.regrid(np.zeros((2, n_s)))
    with pytest.raises(ValueError, match="Invalid regridding method"):
        hip.LayeredOverlapRegridder.from_regridder(pair["mesh"], top, bottom, top[:, :n_t], bottom[:, :n_t], method="conductance")
