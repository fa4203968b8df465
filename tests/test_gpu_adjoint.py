"""
GPU (-m gpu): the transposed weights and the adjoint apply (xr_adjoint.hip) against scipy's transpose and the exact rational
restatement of tests/adjoint_cases.py; the public classes' ``regrid_adjoint``; torch autograd through ``regrid`` (in a process
of its own, tests/adjoint_worker_gpu.py).
"""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse

import adjoint_cases as ac
import xugrid_amd as xa
from xugrid_amd import engine, meshgen
from xugrid_amd.engine import METHOD_IDS, DeviceArray, DeviceCSR, DeviceOuter

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "row_keys", "col_keys", "stored", "mesh", "empty")
METHODS = sorted(ac.METHOD_IDS)
SENTINEL = -1.2345e300


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def mesh_pair(n_source, n_target):
    sxy, sf = meshgen.triangle_mesh(n_source, 61)
    txy, tf = meshgen.triangle_mesh(n_target, 62, 30.0, 0.8)
    return xa.Ugrid2d(sxy[:, 0], sxy[:, 1], -1, sf), xa.Ugrid2d(txy[:, 0], txy[:, 1], -1, tf)


@functools.lru_cache(maxsize=None)
def host_matrix(base):
    """(data, indices, indptr, T, S) in the caller's ids"""
    if base == "synthetic":
        return ac.synthetic_matrix()
    if base == "empty":
        return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(6, dtype=np.int64), 5, 7
    src, tgt = mesh_pair(3000, 3000)
    rg = xa.OverlapRegridder(src, tgt, method="mean")
    w = rg._ensure_host_weights()
    return np.asarray(w.data), np.asarray(w.indices).astype(np.int64), np.asarray(w.indptr).astype(np.int64), w.n, w.m


def base_of(variant):
    return variant if variant in ("mesh", "empty") else "synthetic"


def device_matrix(variant):
    """-> (DeviceCSR, order): output row r of the device matrix is row order[r] of the host matrix (None: the same)"""
    data, indices, indptr, T, S = host_matrix(base_of(variant))
    rng = np.random.default_rng(5)
    if variant == "mesh":  # built on the device: a stored row order of its own
        src, tgt = mesh_pair(3000, 3000)
        return xa.OverlapRegridder(src, tgt, method="mean")._ensure_device_weights(), None
    d = DeviceCSR.from_arrays(data, indices, indptr, T, S)
    order = None
    if variant in ("row_keys", "stored"):
        d.set_row_keys(rng.integers(0, 64, size=T), 64)
    if variant == "row_keys":
        assert not np.array_equal(d.row_order(), np.arange(T))  # (settles the tiling: rows stored in another order)
    if variant == "col_keys":
        d.set_col_keys(rng.integers(0, 32, size=S), 32)
        assert not np.array_equal(d.col_order(), np.arange(S))
    if variant == "stored":
        d.output_stored_order(True)
        order = d.row_order()
        assert not np.array_equal(order, np.arange(T))
    return d, order


def permuted_rows(data, indices, indptr, order):
    """the CSR whose row r is row order[r]"""
    if order is None:
        return data, indices, indptr
    lens = np.diff(indptr)[order]
    new_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(indptr[i], indptr[i + 1]) for i in order]) if len(data) else np.zeros(0, dtype=np.int64)
    return data[take], indices[take], new_indptr


@functools.lru_cache(maxsize=None)
def reference(base, method):
    """(v, g, exact reference) for 17 variables, computed once; fewer variables use the leading planes"""
    data, indices, indptr, T, S = host_matrix(base)
    v, g = ac.case_data(T, S)
    g = ac.gradient_for(method, data, indices, indptr, v, g)
    return v, g, ac.adjoint_exact(method, data, indices, indptr, S, g, v)


# ---- 1. transposition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_transpose_equals_scipy(hip, variant):
    data, indices, indptr, T, S = host_matrix(base_of(variant))
    d, order = device_matrix(variant)
    down = d.download()
    assert np.array_equal(down[0], data) and np.array_equal(down[1], indices) and np.array_equal(down[2], indptr)
    pdata, pindices, pindptr = permuted_rows(data, indices, indptr, order)
    ref = scipy.sparse.csr_matrix((pdata, pindices, pindptr), shape=(T, S)).T.tocsr()
    t = d.transpose()
    assert (t.n, t.m, t.nnz) == (S, T, len(data))
    t_data, t_indices, t_indptr = t.download()
    assert np.array_equal(t_indptr, ref.indptr)
    assert np.array_equal(t_indices, ref.indices)
    assert np.array_equal(t_data, ref.data)
    if variant == "plain":
        lens = np.diff(t_indptr)
        assert tuple(lens[: len(ac.COLUMN_LENGTHS)]) == ac.COLUMN_LENGTHS and lens[-1] == 0
        assert sorted(t.long_rows().tolist()) == np.flatnonzero(lens > 32).tolist()
        # the transposed handle is an ordinary matrix: its forward apply is the adjoint of `first_order_conservative`
        g = np.random.default_rng(1).normal(size=(2, T))
        got = t.apply(g, METHOD_IDS["first_order_conservative"])
        exp = d.adjoint(None, g, METHOD_IDS["first_order_conservative"])
        filled = lens > 0
        filled[ac.ZERO_COLUMN] = False  # (only zero weights: NaN in the forward, +0.0 in the adjoint)
        np.testing.assert_allclose(got[:, filled], exp[:, filled], rtol=1e-12, atol=1e-13)


def test_transpose_follows_a_new_stored_order(hip):
    """The sequence xr_csr_set_row_keys prescribes for a matrix that delivers in stored order -- switch the stored output off,
    set new keys, switch it on again -- regroups the rows: a transposition cached in the old stored positions must not
    survive it.  No adjoint call in between."""
    data, indices, indptr, T, S = host_matrix("synthetic")
    rng = np.random.default_rng(9)
    d = DeviceCSR.from_arrays(data, indices, indptr, T, S)
    d.set_row_keys(rng.integers(0, 64, size=T), 64)
    d.output_stored_order(True)
    first = d.row_order()
    g = rng.normal(size=(9, T))

    def check(order):
        ref = scipy.sparse.csr_matrix(permuted_rows(data, indices, indptr, order), shape=(T, S)).T.tocsr()
        t_data, t_indices, t_indptr = d.transpose().download()
        assert np.array_equal(t_indptr, ref.indptr) and np.array_equal(t_indices, ref.indices) and np.array_equal(t_data, ref.data)
        got = d.adjoint(None, g if order is None else g[:, order], METHOD_IDS["first_order_conservative"])
        exp = ac.adjoint("first_order_conservative", data, indices, indptr, S, g)
        np.testing.assert_allclose(got, exp, rtol=1e-12, atol=1e-13)

    check(first)
    d.output_stored_order(False)
    d.set_row_keys(rng.integers(0, 97, size=T), 97)
    d.output_stored_order(True)
    second = d.row_order()
    assert not np.array_equal(first, second)
    check(second)
    # ... and with an adjoint in the caller's ids in between, then tiled by a many-variable forward apply
    d.output_stored_order(False)
    check(None)
    d.set_row_keys(rng.integers(0, 31, size=T), 31)
    d.apply(np.ones((8, S)), METHOD_IDS["mean"])
    check(None)
    d.output_stored_order(True)
    check(d.row_order())
    d.drop_transpose()
    check(d.row_order())


# ---- 2. adjoint against the exact restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_adjoint_against_exact_restatement(hip, variant, method):
    """|got - exact| <= (L_j + n_j + 4) 2^-53 M per (k, j) (adjoint_cases.bound), exactly +0.0 where that is 0; every K edge of
    the variable tiles, float32 and float64 sources.  NaN in one plane only (a NaN-free tile and a mixed one), NaN gradients on
    the rows that are not live, a zero-weight entry in a row, a column of zero weights."""
    base = base_of(variant)
    data, indices, indptr, T, S = host_matrix(base)
    d, order = device_matrix(variant)
    v, g, ref = reference(base, method)
    g_dev = g if order is None else g[:, order]
    for K in ac.K_EDGES:
        for dtype in (np.float64, np.float32):
            got = d.adjoint(v[:K].astype(dtype), g_dev[:K], ac.METHOD_IDS[method])
            assert got.shape == (K, S) and got.dtype == np.float64
            bad = ac.check_against_exact(got, ref, K)
            assert not bad, (variant, method, K, dtype.__name__, len(bad), bad[:5])
            if method != "select":
                assert (bits(got[np.isnan(v[:K])]) == 0).all()  # +0.0 where the forward input is NaN
    # no NaN pattern given = a source without NaN
    got = d.adjoint(None, np.nan_to_num(g_dev[:2]), ac.METHOD_IDS[method])
    exp = d.adjoint(np.ones((2, S)), np.nan_to_num(g_dev[:2]), ac.METHOD_IDS[method])
    assert np.array_equal(bits(got), bits(exp))


@pytest.mark.parametrize("method", METHODS)
def test_adjoint_on_the_dyadic_matrix_by_value(hip, method):
    data, indices, indptr, T, S = ac.dyadic_matrix()
    v = ac.dyadic_values()
    g = ac.gradient_for(method, data, indices, indptr, v, np.arange(1, 3 * T + 1, dtype=np.float64).reshape(3, T))
    d = DeviceCSR.from_arrays(data, indices, indptr, T, S)
    exp = ac.adjoint(method, data, indices, indptr, S, g, v)
    for dtype in (np.float64, np.float32):
        got = d.adjoint(v.astype(dtype), g, ac.METHOD_IDS[method])
        assert np.array_equal(bits(got), bits(exp)), (method, dtype.__name__)
    # plain IEEE on live rows: a NaN or inf gradient propagates; on rows that are not live it is ignored
    g2 = np.where(np.isnan(g), np.inf, g)
    assert np.array_equal(bits(d.adjoint(v, g2, ac.METHOD_IDS[method])), bits(exp))
    g3 = g.copy()
    g3[0, 0] = np.inf
    assert np.array_equal(bits(d.adjoint(v, g3, ac.METHOD_IDS[method])), bits(ac.adjoint(method, data, indices, indptr, S, g3, v)))


def test_unsupported_reducers_raise(hip):
    data, indices, indptr, T, S = ac.dyadic_matrix()
    d = DeviceCSR.from_arrays(data, indices, indptr, T, S)
    for name in ("harmonic_mean", "geometric_mean", "minimum", "maximum", "mode", "percentile", "max_overlap"):
        with pytest.raises(NotImplementedError, match=name):
            d.adjoint(None, np.ones((1, T)), METHOD_IDS[name])
        # ... and in the C ABI: XR_ERR_INVALID
        out = np.empty((1, S))
        rc = engine._lib.load().xr_apply_csr_adjoint(d._h, METHOD_IDS[name], None, engine.XR_F64, engine._ptr(np.ones((1, T))), 1,
                                                     engine._ptr(out))
        assert rc == -1


# ---- 3. output guard and reproducibility -----------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", ["plain", "col_keys", "mesh"])
def test_guard_words_and_reproducibility(hip, variant, method):
    base = base_of(variant)
    data, indices, indptr, T, S = host_matrix(base)
    d, _ = device_matrix(variant)
    v, g, _ = reference(base, method)
    K, GUARD = 9, 8
    v_dev, g_dev = DeviceArray.from_host(v[:K]), DeviceArray.from_host(np.ascontiguousarray(g[:K]))
    runs = []
    for call in range(3):
        if call == 2:
            d.drop_transpose()
        out = DeviceArray.from_host(np.full(K * S + GUARD, SENTINEL))
        d.adjoint_dev(v_dev.ptr, engine.XR_F64, g_dev.ptr, K, out.ptr, ac.METHOD_IDS[method])
        engine.dev_sync()
        host = out.download()
        assert (bits(host[K * S:]) == bits(np.full(GUARD, SENTINEL))).all(), "guard words behind the output were written"
        assert not (bits(host[: K * S]) == bits(np.float64(SENTINEL))).any(), "part of the output was not written"
        runs.append(host[: K * S].copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.array_equal(bits(runs[0]), bits(runs[2]))
    assert np.array_equal(bits(runs[0]), bits(d.adjoint(v[:K], g[:K], ac.METHOD_IDS[method]).ravel()))


# ---- 4. structured pair ----------------------------------------------------------------------------------------------------
def test_structured_pair_through_device_outer(hip):
    from xugrid_amd.regrid.structured import Raster, StructuredGrid2d

    s = StructuredGrid2d(Raster(x=np.arange(41) + 0.5, y=np.arange(37)[::-1] + 0.5))
    t = StructuredGrid2d(Raster(x=np.linspace(1.0, 40.0, 29), y=np.linspace(36.0, 1.0, 23)))
    w = s.overlap_device(t, False)
    assert isinstance(w, DeviceOuter) and (w.n, w.m) == (23 * 29, 37 * 41)
    data, indices, indptr = w.download()
    c = DeviceCSR.from_arrays(data, indices, indptr, w.n, w.m)
    rng = np.random.default_rng(2)
    v = rng.normal(size=(3, w.m))
    v[1, ::5] = np.nan
    g = rng.normal(size=(3, w.n))
    v_dev, g_dev = DeviceArray.from_host(v), DeviceArray.from_host(g)
    for method in METHODS:
        exp = c.adjoint(v, g, ac.METHOD_IDS[method])
        assert np.array_equal(bits(w.adjoint(v, g, ac.METHOD_IDS[method])), bits(exp)), method
        out = DeviceArray((3, w.m))
        w.adjoint_dev(v_dev.ptr, engine.XR_F64, g_dev.ptr, 3, out.ptr, ac.METHOD_IDS[method])
        engine.dev_sync()
        assert np.array_equal(bits(out.download()), bits(exp)), method
        ref = ac.adjoint(method, data, indices.astype(np.int64), indptr.astype(np.int64), w.m, g, v)
        np.testing.assert_allclose(exp, ref, rtol=1e-12, atol=1e-13)


# ---- 5. public classes -----------------------------------------------------------------------------------------------------
CLASSES = {
    "overlap_mean": (xa.OverlapRegridder, {"method": "mean"}, "mean"),
    "overlap_sum": (xa.OverlapRegridder, {"method": "sum"}, "sum"),
    "relative": (xa.RelativeOverlapRegridder, {}, "first_order_conservative"),
    "centroid": (xa.CentroidLocatorRegridder, {}, "select"),
    "barycentric": (xa.BarycentricInterpolator, {}, "mean"),
}


def _host_csr(rg):
    w = rg.weights
    data = np.asarray(w["__regrid_data"], dtype=np.float64)
    n, m = int(w["__regrid_n"]), int(w["__regrid_m"])
    if "__regrid_indptr" in w:
        return data, np.asarray(w["__regrid_indices"]).astype(np.int64), np.asarray(w["__regrid_indptr"]).astype(np.int64), n, m
    row = np.asarray(w["__regrid_row"]).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    return data, np.asarray(w["__regrid_col"]).astype(np.int64), indptr, n, m


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_public_classes_regrid_adjoint(hip, name):
    cls, kwargs, method = CLASSES[name]
    src, tgt = mesh_pair(1500, 1250)  # about 3000 -> 2500 faces
    rg = cls(src, tgt, **kwargs)
    data, indices, indptr, T, S = _host_csr(rg)
    assert (T, S) == (tgt.n_face, src.n_face)
    rng = np.random.default_rng(4)
    v = rng.normal(size=(2, 3, S))
    v[1, 1, ::9] = np.nan
    g = rng.normal(size=(2, 3, T))
    got = rg.regrid_adjoint(g, v)
    assert got.shape == (2, 3, S) and got.dtype == np.float64
    ref = ac.adjoint_exact(method, data, indices, indptr, S, np.where(ac.live_rows(method, data, indices, indptr, v.reshape(6, S)),
                                                                     g.reshape(6, T), 0.0), v.reshape(6, S))
    assert not ac.check_against_exact(got.reshape(6, S), ref)
    # a single field, no NaN pattern
    one = rg.regrid_adjoint(g[0, 0])
    assert one.shape == (S,)
    # the device path: same kind out as in, the same bits
    out = rg.regrid_adjoint(DeviceArray.from_host(g), DeviceArray.from_host(v))
    assert isinstance(out, DeviceArray) and out.shape == (2, 3, S)
    assert np.array_equal(bits(out.download()), bits(got))
    out32 = rg.regrid_adjoint(DeviceArray.from_host(g), DeviceArray.from_host(v.astype(np.float32)))
    assert np.array_equal(bits(out32.download()), bits(got))
    with pytest.raises(ValueError):
        rg.regrid_adjoint(g[..., :-1], v)
    with pytest.raises(ValueError):
        rg.regrid_adjoint(g, v[0])
    if method in ("mean", "first_order_conservative"):
        # <regrid(v), g> = <v, regrid_adjoint(g, v)> on NaN-free data.  Both inner products are formed exactly (Fractions of
        # the computed doubles), so the only errors are the two applies': the adjoint's bound summed over all columns, each
        # weighted by |v_j|, plus the same bound for the forward side -- row i has n_i entries and is its own longest row:
        # (n_i + n_i + 4) 2^-53 sum_e |g_i w v_j| / Wsum_i (first_order_conservative: without the division).
        v0, g0 = v[0, 0], g[0, 0]
        fwd = rg.regrid(v0)
        livef = ~np.isnan(fwd)
        g_live = np.where(livef, g0, 0.0)
        a = rg.regrid_adjoint(g_live, v0)
        lhs = sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(fwd[livef], g0[livef])), Fraction(0))
        rhs = sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(v0, a)), Fraction(0))
        ex = ac.adjoint_exact(method, data, indices, indptr, S, g_live[None, :], v0[None, :])
        tol = sum((ac.bound(ex[1][0][j], ex[2][j], ex[3][0][j]) * abs(Fraction(float(v0[j]))) for j in range(S)), Fraction(0))
        tol += ac.forward_bound(method, data, indices, indptr, g_live, v0)
        print(name, "inner products differ by", float(abs(lhs - rhs)), "bound", float(tol))
        assert abs(lhs - rhs) <= tol, (float(lhs), float(rhs), float(tol))


def test_centroid_locator_adjoint_with_unsorted_coo_weights(hip):
    """externally supplied COO weights in any order: ``regrid`` scatters them as they are, ``regrid_adjoint`` gives what the
    sorted weights give"""
    src, tgt = mesh_pair(1500, 1250)
    rg = xa.CentroidLocatorRegridder(src, tgt)
    ds = rg.to_dataset()
    perm = np.random.default_rng(6).permutation(np.asarray(ds["__regrid_row"]).size)
    for key in ("__regrid_data", "__regrid_row", "__regrid_col"):
        ds[key] = np.asarray(ds[key])[perm]
    rg2 = xa.CentroidLocatorRegridder.from_weights(ds, tgt)
    g = np.random.default_rng(7).normal(size=(2, tgt.n_face))
    assert np.array_equal(bits(rg2.regrid_adjoint(g)), bits(rg.regrid_adjoint(g)))
    v = np.random.default_rng(8).normal(size=(2, src.n_face))
    assert np.array_equal(bits(rg2.regrid(v)), bits(rg.regrid(v)))


def test_unsupported_method_on_a_regridder(hip):
    src, tgt = mesh_pair(1500, 1250)
    rg = xa.OverlapRegridder(src, tgt, method="maximum")
    with pytest.raises(NotImplementedError, match="maximum"):
        rg.regrid_adjoint(np.ones(tgt.n_face))
    rg = xa.OverlapRegridder(src, tgt, method=lambda values, weights, work: 0.0)
    with pytest.raises(NotImplementedError):
        rg.regrid_adjoint(np.ones(tgt.n_face))


# ---- 6. torch autograd -----------------------------------------------------------------------------------------------------
def test_torch_autograd_through_regrid():
    """torch has to initialise its HIP runtime before the engine binds the device: a process of its own."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adjoint_worker_gpu.py")
    res = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "TORCH_ADJOINT_OK" in res.stdout
