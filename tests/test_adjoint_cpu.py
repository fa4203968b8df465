"""The restatement of the adjoint apply (tests/adjoint_cases.py) pinned to the reference's reducers, and its transpose to
scipy's.  No GPU: what the device kernels are compared with has to be right first."""
import numpy as np
import pytest
import scipy.sparse

import adjoint_cases as ac

H = 2.0 ** -4


def _jacobian(method, data, indices, indptr, T, S, v_k):
    """J[i, j] = the coefficient of v[j] in row i, from the restatement applied to the unit gradients"""
    v = None if v_k is None else np.repeat(v_k[None, :], T, axis=0)
    return ac.adjoint(method, data, indices, indptr, S, np.eye(T), v)


@pytest.mark.parametrize("method", ["mean", "sum", "first_order_conservative"])
def test_difference_quotient_of_the_reference_reducers(oracle, method):
    """The three w-sum methods are linear in v for a fixed NaN pattern, so on dyadic inputs the difference quotient of the
    reference's reducer is exact: it equals the restatement's coefficients BY VALUE -- rows with NaN entries, zero-weight
    entries, all-NaN rows and empty rows included."""
    data, indices, indptr, T, S = ac.dyadic_matrix()
    values = ac.dyadic_values()
    for k in range(values.shape[0]):
        v = values[k]
        base = oracle.regrid_csr(method, v[None, :], data, indices, indptr, T)[0]
        J = _jacobian(method, data, indices, indptr, T, S, v)
        live = ac.live_rows(method, data, indices, indptr, v[None, :])[0]
        assert np.array_equal(np.isnan(base), ~live), "liveness differs from the reference's NaN rows"
        assert (J[~live] == 0).all()
        for j in np.flatnonzero(~np.isnan(v)):
            bumped = v.copy()
            bumped[j] += H
            dq = (oracle.regrid_csr(method, bumped[None, :], data, indices, indptr, T)[0] - base) / H
            assert np.array_equal(dq[live], J[live, j]), (method, k, j)
        for j in np.flatnonzero(np.isnan(v)):
            assert (J[:, j] == 0).all() and not np.signbit(J[:, j]).any()


def test_difference_quotient_of_the_coo_scatter(oracle):
    """select = the COO scatter of CentroidLocatorRegridder: out[row] = source[col], NaN included."""
    T, S = 7, 6
    row = np.array([0, 2, 3, 5, 6], dtype=np.int64)
    col = np.array([4, 1, 1, 0, 5], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=T))]).astype(np.int64)
    data = np.ones(row.size)
    v = np.array([3.0, np.nan, -2.0, 5.0, 1.0, 4.0])
    base = oracle.regrid_coo(v[None, :], row, col, T)[0]
    J = _jacobian("select", data, col, indptr, T, S, v)
    finite = np.isfinite(base)
    for j in np.flatnonzero(~np.isnan(v)):
        bumped = v.copy()
        bumped[j] += H
        dq = (oracle.regrid_coo(bumped[None, :], row, col, T)[0] - base) / H
        assert np.array_equal(dq[finite], J[finite, j])
    # NaN is copied, not masked: the rows that select column 1 keep their coefficient
    assert J[2, 1] == 1.0 and J[3, 1] == 1.0 and J[1].sum() == 0 and J[4].sum() == 0


def test_select_takes_the_last_entry_of_a_row():
    data = np.array([1.0, 1.0, 1.0])
    indices = np.array([2, 0, 1], dtype=np.int64)
    indptr = np.array([0, 2, 2, 3], dtype=np.int64)
    g = np.array([[5.0, np.nan, 7.0]])
    a = ac.adjoint("select", data, indices, indptr, 3, g, np.array([[np.nan, 1.0, 2.0]]))
    assert np.array_equal(a, [[5.0, 7.0, 0.0]])


def test_transpose_equals_scipy_with_duplicates():
    """scipy keeps duplicates in .T.tocsr() and orders the rows ascending, stably: array for array the same."""
    rng = np.random.default_rng(0)
    T, S, nnz = 40, 17, 300
    row = np.sort(rng.integers(0, T, size=nnz))
    col = rng.integers(0, S, size=nnz)
    col[1::7] = col[0::7][: col[1::7].size]
    row[1::7] = row[0::7][: row[1::7].size]
    order = np.argsort(row, kind="stable")
    row, col = row[order], col[order]
    data = rng.uniform(0.5, 1.5, size=nnz)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=T))])
    pairs = list(zip(row.tolist(), col.tolist()))
    assert len(set(pairs)) < len(pairs), "the matrix must hold duplicate (i, j) entries"
    ref = scipy.sparse.csr_matrix((data, col, indptr), shape=(T, S)).T.tocsr()
    t_data, t_rows, t_indptr, _ = ac.transpose(data, col, indptr, S)
    assert ref.nnz == nnz
    assert np.array_equal(ref.indptr, t_indptr) and np.array_equal(ref.indices, t_rows) and np.array_equal(ref.data, t_data)
    w, c, ip, T2, S2 = ac.synthetic_matrix()
    ref = scipy.sparse.csr_matrix((w, c, ip), shape=(T2, S2)).T.tocsr()
    t_data, t_rows, t_indptr, _ = ac.transpose(w, c, ip, S2)
    assert np.array_equal(ref.indptr, t_indptr) and np.array_equal(ref.indices, t_rows) and np.array_equal(ref.data, t_data)
    assert tuple(np.diff(t_indptr)[: len(ac.COLUMN_LENGTHS)]) == ac.COLUMN_LENGTHS and np.diff(t_indptr)[-1] == 0


@pytest.mark.parametrize("method", sorted(ac.METHOD_IDS))
def test_float_restatement_within_the_bound_of_the_exact_one(method):
    """The float restatement (sequential order) stays inside the bound the device kernels are held to, and is exactly +0.0
    where the bound is 0 -- on a cut of the synthetic matrix small enough for the CPU suite."""
    w, c, ip, T, S = ac.synthetic_matrix(T=300, S=60, seed=11, column_lengths=(0, 1, 32, 33, 64, 65), long_rows=(33, 40))
    v, g = ac.case_data(T, S, K=3)
    g = ac.gradient_for(method, w, c, ip, v, g)
    ref = ac.adjoint_exact(method, w, c, ip, S, g, v)
    got = ac.adjoint(method, w, c, ip, S, g, v)
    assert ac.check_against_exact(got, ref) == []
    if method != "select":
        assert (got[np.isnan(v)] == 0).all()
    # a NaN gradient on a live row propagates (plain IEEE), on a row that is not live it is ignored
    live = ac.live_rows(method, w, c, ip, v)
    i = int(np.flatnonzero(live[0])[0])
    g2 = g.copy()
    g2[0, i] = np.nan
    got2 = ac.adjoint(method, w, c, ip, S, g2, v)
    assert np.isnan(got2[0, c[ip[i]:ip[i + 1]]]).all()  # (plane 0 holds no NaN; select: 0 * NaN on the other entries)
    dead = np.flatnonzero(~live[0])
    assert dead.size and np.isnan(g[0, dead]).all() and np.isfinite(got[0]).all()


def test_dyadic_restatement_is_exact():
    data, indices, indptr, T, S = ac.dyadic_matrix()
    v = ac.dyadic_values()
    g = np.arange(1, 3 * T + 1, dtype=np.float64).reshape(3, T)
    for method in ac.METHOD_IDS:
        gm = ac.gradient_for(method, data, indices, indptr, v, g)
        exact = ac.adjoint_exact(method, data, indices, indptr, S, gm, v)[0]
        got = ac.adjoint(method, data, indices, indptr, S, gm, v)
        assert all(float(exact[k][j]) == got[k, j] and exact[k][j] == got[k, j] for k in range(3) for j in range(S))


def test_unsupported_reducers_are_named():
    from xugrid_amd import engine

    for name in ("harmonic_mean", "geometric_mean", "minimum", "maximum", "mode", "percentile", "max_overlap"):
        with pytest.raises(NotImplementedError, match=name):
            engine.check_adjoint_method(engine.METHOD_IDS[name])
    for name in ("mean", "sum", "first_order_conservative", "conductance", "select"):
        engine.check_adjoint_method(engine.METHOD_IDS[name])
