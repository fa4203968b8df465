"""
CPU: the oracle (oracle/xr_oracle.c) against golden set G12 (tests/golden/gen_reducer_edges.py): the reference's own
reducers (reduce.py) on crafted corner rows -- mode and max_overlap ties, the percentiles' w_max over all entries against
minimum / maximum's over the valid ones, geometric_mean's early NaN on a negative value, harmonic_mean's zero skip,
zero-weight rows, +-inf, +-0.0, float64 and float32 denormals, overflowing sums -- short (1 ... 32 entries) and long
(33 ... 4097 entries, a dyadic alphabet on which every reducer but geometric_mean is exact in any summation order).
G1 stops at 64 entries and holds no special value but NaN; every device test trusts the oracle at these corners.

Signed zeros compare equal throughout (same_or_nan compares by value): which of +0.0 and -0.0 the reference's `min` / `max`
return is a property of the interpreter that ran it, not of the method, and the goldens are made without numba.
"""
import numpy as np
import pytest

from conftest import same_or_nan
from test_oracle_goldens import method_arg

RTOL_GEOMETRIC = 1e-13        # test_gpu_parity.RTOL_GEOMETRIC: the bound on long rows (the summation order is free there)
RTOL_GEOMETRIC_SHORT = 1e-14  # test_g1_reducers_bit_exact: libm exp / log against numpy's on the same sequence

METHOD_NAMES = ["mean", "harmonic_mean", "geometric_mean", "sum", "minimum", "maximum", "mode", "median", "p5", "p10", "p25", "p50",
                "p75", "p90", "p95", "p33.3", "p0", "p100", "first_order_conservative", "conductance", "max_overlap"]


@pytest.fixture(scope="module")
def g12(golden):
    g = golden("g12_reducer_edges.npz")
    return {k: g[k] for k in g.files}


def assert_rows_equal(got, exp, is_long, name, what):
    """by value on every row; geometric_mean within RTOL_GEOMETRIC_SHORT on short and RTOL_GEOMETRIC on long rows"""
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp)), (what, np.flatnonzero(np.isnan(got) != np.isnan(exp))[:8])
    if name == "geometric_mean":
        np.testing.assert_allclose(got[..., ~is_long], exp[..., ~is_long], rtol=RTOL_GEOMETRIC_SHORT, atol=0, equal_nan=True, err_msg=str(what))
        np.testing.assert_allclose(got[..., is_long], exp[..., is_long], rtol=RTOL_GEOMETRIC, atol=0, equal_nan=True, err_msg=str(what))
    else:
        bad = ~same_or_nan(got, exp)
        assert not bad.any(), (what, np.argwhere(bad)[:8].tolist(), got[bad][:8], exp[bad][:8])


def test_g12_layout(g12):
    """what the device tests rely on: the row lengths at the kernels' thresholds, a NaN-free plane that keeps +-inf, and
    results that are not NaN throughout (no comparison here can pass on NaN = NaN alone)"""
    lens, is_long = np.diff(g12["indptr"]), g12["is_long"]
    assert g12["planes64"].shape == g12["planes32"].shape == (4, lens.sum()) and g12["planes32"].dtype == np.float32
    with np.errstate(over="ignore"):  # (1e308 -> inf)
        assert np.array_equal(g12["planes64"].astype(np.float32), g12["planes32"], equal_nan=True)
    assert np.array_equal(is_long, lens > 32)
    assert set(lens[is_long]) == {33, 34, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3073, 4097}
    assert {0, 1, 2, 3, 31, 32} <= set(lens)
    a, b, c, d = g12["planes64"]
    assert np.isnan(a).any() and np.isinf(a).any() and not np.isnan(b).any() and np.isinf(b).any() and np.isnan(c).all()
    assert np.signbit(b[b == 0]).any() and not np.signbit(b[b == 0]).all()
    assert np.isnan(d).any() and (d == 0).any() and (d[~np.isnan(d)] >= 0).all() and np.isfinite(d[~np.isnan(d)]).all()
    assert 0.0 < float(g12["geo_spread"]) < RTOL_GEOMETRIC / 10
    for name in METHOD_NAMES:
        for tag in ("64", "32"):
            fin = np.isfinite(g12[f"out{tag}_{name}"][:, is_long]).sum(axis=1)
            assert (fin[[0, 1, 3]] * 4 >= is_long.sum()).all(), (name, tag, fin)


@pytest.mark.parametrize("name", METHOD_NAMES)
def test_oracle_reduce_row_by_row(g12, oracle, name):
    indptr, data, is_long = g12["indptr"], g12["data"], g12["is_long"]
    T = indptr.size - 1
    for tag in ("64", "32"):
        planes = g12["planes" + tag].astype(np.float64)
        got = np.full((4, T), np.nan)
        for t in np.flatnonzero(np.diff(indptr) > 0):  # (an empty row never reaches a reducer: regridder.py:63)
            s, e = indptr[t], indptr[t + 1]
            for p in range(4):
                got[p, t] = oracle.reduce(method_arg(name), planes[p, s:e], data[s:e])
        assert_rows_equal(got, g12[f"out{tag}_{name}"], is_long, name, (name, tag))


@pytest.mark.parametrize("name", METHOD_NAMES)
def test_oracle_regrid_csr(g12, oracle, name):
    indptr, data, is_long = g12["indptr"], g12["data"], g12["is_long"]
    T, indices = indptr.size - 1, np.arange(data.size, dtype=np.int64)
    for tag in ("64", "32"):
        got = oracle.regrid_csr(method_arg(name), g12["planes" + tag], data, indices, indptr, T)
        assert_rows_equal(got, g12[f"out{tag}_{name}"], is_long, name, (name, tag))
