"""The yardstick of the partial-state tests (tests/partial_cases.py) pinned against hand-written rows and against the oracle:
states per column shard, combined and finalised, are what the reference's reducers give on the whole matrix."""
import numpy as np
import pytest

import partial_cases as PC

NAN = np.nan


def reduce_row(name, v, w):
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    mid = PC.IDS[name]
    return float(PC.finalize(mid, PC.states(mid, v, w, np.zeros(v.size, dtype=np.int64), 1))[0])


def test_hand_written_rows():
    expect = {"mean": 5.0, "harmonic_mean": 3.2, "geometric_mean": 4.0, "sum": 10.0, "minimum": 2.0, "maximum": 8.0,
              "first_order_conservative": 10.0}
    for name, value in expect.items():
        got = reduce_row(name, [2, 8], [1, 1])
        assert got == value if name != "geometric_mean" else abs(got - value) <= 4 * np.spacing(value), (name, got)
    assert reduce_row("mean", [1, 3], [3, 1]) == 1.5
    assert reduce_row("first_order_conservative", [1, 3], [0.25, 0.5]) == 1.75
    assert reduce_row("harmonic_mean", [1, 4], [1, 2]) == 2.0  # 3 / (1 + 0.5)
    assert reduce_row("mean", [NAN, 3], [5, 1]) == 3.0  # NaN entries are skipped, weight and all
    assert reduce_row("sum", [NAN, 3, 4], [1, 1, 1]) == 7.0
    assert reduce_row("minimum", [NAN, 3, -4], [1, 1, 1]) == -4.0
    assert reduce_row("maximum", [NAN, 3, -4], [1, 1, 1]) == 3.0
    assert reduce_row("harmonic_mean", [0, 2, NAN], [1, 1, 1]) == 2.0  # zeros are skipped
    assert abs(reduce_row("geometric_mean", [0, 4, 9], [1, 1, 1]) - 6.0) < 1e-14  # ... and here (with their weight)
    assert abs(reduce_row("geometric_mean", [NAN, 4, 9], [1, 1, 1]) - 6.0) < 1e-14


def test_nan_rules():
    for name in PC.NAMES:
        assert np.isnan(reduce_row(name, [], [])), name  # an empty row
        assert np.isnan(reduce_row(name, [1.0, 2.0], [0.0, 0.0])), name  # zero weight sum
        assert np.isnan(reduce_row(name, [NAN, NAN], [1.0, 2.0])), name  # nothing valid
    assert np.isnan(reduce_row("harmonic_mean", [0.0, 0.0], [1.0, 1.0]))
    assert np.isnan(reduce_row("harmonic_mean", [np.inf], [1.0]))  # v_agg = 0
    assert np.isnan(reduce_row("geometric_mean", [4.0, -1.0], [1.0, 0.0]))  # a negative value, even of weight 0
    assert np.isnan(reduce_row("geometric_mean", [0.0, 0.0], [1.0, 1.0]))  # no positive value
    assert reduce_row("geometric_mean", [4.0, 0.0], [1.0, 0.0]) == pytest.approx(4.0, rel=1e-15)
    assert reduce_row("minimum", [1.0, -2.0], [0.0, 1.0]) == -2.0  # zero-weight entries count while one weight is positive
    assert reduce_row("sum", [1.0, 2.0], [0.0, 1.0]) == 3.0
    assert reduce_row("maximum", [-np.inf, NAN], [1.0, 1.0]) == -np.inf


def test_signed_zeros_and_combine_order():
    z = PC.states(PC.MAXIMUM, [-0.0, 0.0, -0.0], [1, 1, 1], [0, 0, 1], 2)
    assert not np.signbit(z[0, 0]) and np.signbit(z[0, 1])
    z = PC.states(PC.MINIMUM, [-0.0, 0.0], [1, 1], [0, 1], 2)  # the state holds -v
    assert not np.signbit(z[0, 0]) and np.signbit(z[0, 1])
    a, b = np.array([[-0.0], [0.0]]), np.array([[0.0], [0.0]])
    assert not np.signbit(PC.combine(PC.MAXIMUM, [a, b])[0, 0]) and not np.signbit(PC.combine(PC.MAXIMUM, [b, a])[0, 0])
    assert np.signbit(PC.combine(PC.MAXIMUM, [a, a])[0, 0])
    assert not np.signbit(PC.combine(PC.SUM, [a])[0, 0])  # 0.0 + -0.0
    big = [np.array([[1e16], [1.0]]), np.array([[1.0], [1.0]]), np.array([[-1e16], [1.0]])]
    assert PC.combine(PC.SUM, big)[0, 0] == 0.0 and PC.combine(PC.SUM, big[::-1])[0, 0] == 0.0
    assert PC.combine(PC.SUM, [big[0], big[2], big[1]])[0, 0] == 1.0  # sequential, in the given order
    assert PC.combine(PC.MEAN, []) is None


def test_cases_have_the_edges():
    data, indices, indptr, T, S = PC.edges()
    n = np.diff(indptr)
    assert T % 64 and T % 128 and T % 256 and indices.max() < S
    assert n[0] == 0 and (n == 0).sum() >= 40 and (n[list(PC.WINDOW_ROWS)] == 32).all()
    assert {33, 64, 65, 384, 385, 880, 600} <= set(n.tolist()) and n[-1] > PC.LONG
    w = n[list(PC.JUMPY_WINDOW)]
    assert (w <= 8).sum() > 50 and (w == 33).sum() == 2 and (w == 600).sum() == 1
    assert 0.01 < (data == 0).mean() < 0.03
    for t in range(T):
        assert (np.diff(indices[indptr[t]:indptr[t + 1]]) > 0).all()
    n_short = np.diff(PC.short_only()[2])
    assert n_short.max() == 32 and np.array_equal(n_short, np.minimum(n, 32))
    for P in (1, 2, 3, 8):
        shards = PC.column_shards(S, P)
        assert len(shards) == P and np.array_equal(np.sort(np.concatenate(shards)), np.arange(S))
        assert (min(s.size for s in shards) == 0) == (P > 1)
    block, names = PC.stack(S, 17)
    assert block.shape == (17, S) and names[7] == names[0] and not np.array_equal(block[0], block[7], equal_nan=True)
    assert np.isnan(block[0]).mean() > 0.02 and np.isinf(block[5]).sum() == 40 and (block[6] == 0).all()
    assert np.signbit(block[6]).any() and not np.signbit(block[6]).all()


@pytest.fixture(scope="module")
def whole(oracle):
    data, indices, indptr, T, S = PC.edges()
    block = np.stack([PC.source(nm, S) for nm in PC.SOURCES])
    return {name: oracle.regrid_csr(name, block, data, indices, indptr, T) for name in PC.NAMES}, block


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_column_splits_give_the_oracle(whole, P):
    expect, block = whole
    data, indices, indptr, T, S = PC.edges()
    rows = PC.row_ids(indptr)
    shards = []
    for cols in PC.column_shards(S, P):
        d, i, p = PC.shard_csr(data, indices, indptr, cols, S)
        shards.append((d, i, PC.row_ids(p), cols))
    assert sum(s[0].size for s in shards) == data.size
    worst = {}
    for name in PC.NAMES:
        mid = PC.IDS[name]
        for k, src in enumerate(PC.SOURCES):
            got = PC.finalize(mid, PC.combine(mid, [PC.states(mid, block[k][cols][i], d, r, T) for d, i, r, cols in shards]))
            ref = expect[name][k]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (name, src)
            if PC.is_max(mid):  # equal as numbers: the reference's min(v, v_min) keeps whichever zero came first, the state
                assert np.array_equal(got, ref, equal_nan=True), (name, src)  # the IEEE maximum; the sign of a zero is not compared
            if P == 1 and name != "geometric_mean":  # one shard: the reference's own loop, operation for operation
                assert np.array_equal(got, ref, equal_nan=True), (name, src)
            if src == "positive":
                ok = ~np.isnan(ref)
                rel = np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])
                worst[name] = rel.max()
                assert rel.max() <= (1e-9 if name == "harmonic_mean" else 1e-12), (name, rel.max())
    print(f"P={P} worst relative difference on 'positive':", {k: f"{v:.1e}" for k, v in worst.items()})
    # the same rows through the long-row yardstick: fsum within the any-order bound of the sequential sum
    mid = PC.MEAN
    long_rows = np.flatnonzero(np.diff(indptr) > PC.LONG)
    seq = PC.states(mid, block[0][indices], data, rows, T)
    mag = PC.magnitudes(mid, block[0][indices], data, rows, T)
    exact = PC.fsum_states(mid, block[0][indices], data, indptr, long_rows)
    for c in PC.summed(mid):
        bound = (np.diff(indptr)[long_rows] + 2) * 2.0 ** -52 * mag[c][long_rows]
        assert (np.abs(seq[c][long_rows] - exact[c]) <= bound).all()
