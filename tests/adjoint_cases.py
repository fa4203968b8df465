"""The adjoint of the regrid apply restated in numpy / plain Python, and exactly in ``fractions.Fraction`` -- what
tests/test_adjoint_cpu.py pins to the reference's reducers and tests/test_gpu_adjoint.py holds the device kernels to.

Notation (include/xugrid_amd.h, "the adjoint of the apply"): W is the T x S weight matrix as CSR ``(data, indices, indptr)``
with entries e = (i, j, w) at storage position p -- rows ascending, storage order kept inside a row, duplicates allowed;
v the forward input (K, S), g the upstream gradient (K, T); the result a is (K, S) float64.

    valid(k, e)  = not isnan(v[k, j])
    Wsum[k, i]   = sum of w over the valid entries of row i (sequential, storage order)
    live(k, i)   = Wsum[k, i] != 0            (select: the row is not empty)
    r[k, i]      = g[k, i] / Wsum[k, i]       (mean);  g[k, i] (sum, first_order_conservative, select)
    coef(e)      = w (mean, first_order_conservative);  1 (sum);  1 on the row's last entry, else 0 (select)
    a[k, j]      = sum of r[k, i] * coef(e) over the entries of column j whose row is live, ascending (i, p);
                   +0.0 for an empty sum and where v[k, j] is NaN (select ignores NaN: its forward copies them)
"""
import functools
import math
from fractions import Fraction

import numpy as np

METHOD_IDS = {"mean": 0, "sum": 3, "first_order_conservative": 8, "select": 10}
K_EDGES = (1, 2, 7, 8, 9, 17)  # the tile edges of the forward tests
U = Fraction(1, 2 ** 53)


def row_ids(indptr):
    indptr = np.asarray(indptr)
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr))


def transpose(data, indices, indptr, m):
    """-> (t_data, t_rows, t_indptr, position): per column the entries in ascending (row, storage position)."""
    indices = np.asarray(indices)
    position = np.argsort(indices, kind="stable")  # storage positions ascend with the row: stable = (i, p)
    t_indptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=m))]).astype(np.int64)
    return np.asarray(data)[position], row_ids(indptr)[position], t_indptr, position


def _is_last(indptr, nnz):
    last = np.zeros(nnz, dtype=bool)
    indptr = np.asarray(indptr)
    ends = indptr[1:][indptr[1:] > indptr[:-1]] - 1
    last[ends] = True
    return last


def _coef(method, w, last):
    if method == "sum":
        return 1.0
    if method == "select":
        return 1.0 if last else 0.0
    return w


def row_state(method, data, indices, indptr, v_k):
    """One variable: (Wsum[i], live[i], valid entries per row) by the sequential walk of the forward reducers."""
    T = len(indptr) - 1
    wsum, live, n_valid = [0.0] * T, [False] * T, [0] * T
    for i in range(T):
        s, e = int(indptr[i]), int(indptr[i + 1])
        acc, cnt = 0.0, 0
        for p in range(s, e):
            if v_k is None or not math.isnan(v_k[indices[p]]):
                acc += data[p]
                cnt += 1
        wsum[i], n_valid[i] = acc, cnt
        live[i] = (e > s) if method == "select" else (acc != 0.0)
    return wsum, live, n_valid


def live_rows(method, data, indices, indptr, v):
    """(K, T) bool"""
    data, indices = [float(x) for x in data], [int(x) for x in indices]
    return np.array([row_state(method, data, indices, indptr, None if v is None else [float(x) for x in v[k]])[1]
                     for k in range(v.shape[0])])


def adjoint(method, data, indices, indptr, m, g, v=None):
    """The restatement in float64: every division, product and sum one IEEE operation, in the order of the contract."""
    assert method in METHOD_IDS
    g = np.asarray(g, dtype=np.float64)
    K, T = g.shape
    nnz = len(data)
    t_data, t_rows, t_indptr, position = transpose(data, indices, indptr, m)
    last = _is_last(indptr, nnz)[position]
    data_l, indices_l = [float(x) for x in data], [int(x) for x in indices]
    t_w, t_i, t_last, t_ip = [float(x) for x in t_data], [int(x) for x in t_rows], [bool(x) for x in last], [int(x) for x in t_indptr]
    out = np.zeros((K, m), dtype=np.float64)
    for k in range(K):
        v_k = None if v is None else [float(x) for x in v[k]]
        wsum, live, _ = row_state(method, data_l, indices_l, indptr, v_k)
        g_k = [float(x) for x in g[k]]
        r = [0.0] * T
        for i in range(T):
            if live[i]:
                r[i] = g_k[i] / wsum[i] if method == "mean" else g_k[i]
        for j in range(m):
            if method != "select" and v_k is not None and math.isnan(v_k[j]):
                continue
            acc = 0.0
            for q in range(t_ip[j], t_ip[j + 1]):
                if live[t_i[q]]:
                    acc += r[t_i[q]] * _coef(method, t_w[q], t_last[q])
            out[k, j] = acc
    return out


def _tree_sum(terms):
    """exact sum of Fractions, pairwise: few additions meet the large denominators"""
    if not terms:
        return Fraction(0)
    while len(terms) > 1:
        nxt = [terms[a] + terms[a + 1] for a in range(0, len(terms) - 1, 2)]
        if len(terms) & 1:
            nxt.append(terms[-1])
        terms = nxt
    return terms[0]


def adjoint_exact(method, data, indices, indptr, m, g, v=None):
    """The same in exact rational arithmetic.  g must be finite on live rows.  -> (exact, M, n, L):
    exact[k][j] Fraction; M[k][j] = sum |terms| (Fraction); n[j] = entries of column j; L[k][j] = entries of the longest live
    row among the valid contributions of column j (0: none)."""
    assert method in METHOD_IDS
    g = np.asarray(g, dtype=np.float64)
    K, T = g.shape
    nnz = len(data)
    t_data, t_rows, t_indptr, position = transpose(data, indices, indptr, m)
    last = _is_last(indptr, nnz)[position]
    data_l, indices_l = [float(x) for x in data], [int(x) for x in indices]
    data_f = [Fraction(x) for x in data_l]
    row_len = np.diff(np.asarray(indptr)).tolist()
    t_w, t_i, t_last, t_ip = [Fraction(float(x)) for x in t_data], [int(x) for x in t_rows], [bool(x) for x in last], [int(x) for x in t_indptr]
    one, zero = Fraction(1), Fraction(0)
    exact, M, L = [], [], []
    for k in range(K):
        v_k = None if v is None else [float(x) for x in v[k]]
        _, live, _ = row_state(method, data_l, indices_l, indptr, v_k)
        r = [zero] * T
        for i in range(T):
            if not live[i]:
                continue
            assert math.isfinite(g[k, i]), "the exact restatement takes finite gradients on live rows"
            gi = Fraction(float(g[k, i]))
            if method == "mean":
                s, e = int(indptr[i]), int(indptr[i + 1])
                ws = sum((data_f[p] for p in range(s, e) if v_k is None or not math.isnan(v_k[indices_l[p]])), zero)
                gi = gi / ws
            r[i] = gi
        ex_k, m_k, l_k = [zero] * m, [zero] * m, [0] * m
        for j in range(m):
            if method != "select" and v_k is not None and math.isnan(v_k[j]):
                continue
            terms, longest = [], 0
            for q in range(t_ip[j], t_ip[j + 1]):
                i = t_i[q]
                if not live[i]:
                    continue
                c = one if method == "sum" else ((one if t_last[q] else zero) if method == "select" else t_w[q])
                terms.append(r[i] * c)
                longest = max(longest, row_len[i])
            ex_k[j] = _tree_sum(terms)
            m_k[j] = _tree_sum([abs(t) for t in terms])
            l_k[j] = longest
        exact.append(ex_k), M.append(m_k), L.append(l_k)
    return exact, M, np.diff(t_indptr), L


def bound(M, n_j, L_j):
    """|got - exact| <= (L_j + n_j + 4) 2^-53 M: the first-order summation bound for ANY order -- n_j - 1 additions, two
    roundings per term (the division, the product), and Wsum's relative error (L_j - 1) u for positive weights."""
    return (int(L_j) + int(n_j) + 4) * U * M


def forward_bound(method, data, indices, indptr, g_k, v_k):
    """The bound of ``bound`` for the FORWARD apply of one NaN-free variable, weighted by |g|: row i has n_i entries and is its
    own longest row, its terms are w v / Wsum (mean) or w v (first_order_conservative) -> sum_i (n_i + n_i + 4) 2^-53 |g_i| M_i
    as a Fraction (rows whose weights sum to zero return NaN in the forward and take no part)."""
    assert method in ("mean", "first_order_conservative")
    total = Fraction(0)
    for i in range(len(indptr) - 1):
        s, e = int(indptr[i]), int(indptr[i + 1])
        w = [Fraction(float(data[p])) for p in range(s, e)]
        wsum = sum(w, Fraction(0))
        if wsum == 0:
            continue
        M = sum((abs(w[p - s] * Fraction(float(v_k[indices[p]]))) for p in range(s, e)), Fraction(0))
        if method == "mean":
            M /= abs(wsum)
        total += bound(M, e - s, e - s) * abs(Fraction(float(g_k[i])))
    return total


def check_against_exact(got, ref, K=None):
    """got (K, m) float64 against ``ref = adjoint_exact(...)`` (its first K variables).  -> list of violations (empty: fine).
    Where the bound is 0 the result must be exactly +0.0."""
    exact, M, n, L = ref
    bad = []
    K = got.shape[0] if K is None else K
    for k in range(K):
        row = got[k].tolist()
        for j, x in enumerate(row):
            b = bound(M[k][j], n[j], L[k][j])
            if b == 0:
                if not (x == 0.0 and math.copysign(1.0, x) > 0):
                    bad.append((k, j, x, 0.0, 0.0))
                continue
            if not math.isfinite(x):
                bad.append((k, j, x, float(exact[k][j]), float(b)))
                continue
            # quick acceptance in floats (each side rounded against the claim), the exact comparison otherwise
            ef, bf = float(exact[k][j]), float(b)
            if abs(x - ef) + abs(ef) * 2.0 ** -51 <= bf * (1 - 2.0 ** -50):
                continue
            if abs(Fraction(x) - exact[k][j]) > b:
                bad.append((k, j, x, ef, bf))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# matrices and data
# ---------------------------------------------------------------------------------------------------------------------------
COLUMN_LENGTHS = (0, 1, 32, 33, 64, 65, 512, 513, 2048, 2049)  # columns 0 .. 9; the last column is empty too
ZERO_COLUMN = 10                                               # holds only zero weights
LONG_ROWS = (33, 40, 513, 600, 2100)                           # rows walked by lane groups, a wave, a block


@functools.lru_cache(maxsize=None)
def synthetic_matrix(T=4100, S=1000, seed=7, column_lengths=COLUMN_LENGTHS, long_rows=LONG_ROWS):
    """(data, indices, indptr, T, S): the first columns hold ``column_lengths`` entries, column S - 1 none, the others 0..5; duplicate
    (i, j) entries of different weights; rows unsorted inside; a few long rows; positive weights except ZERO_COLUMN's and one
    zero-weight entry in a row that has other entries."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for j in range(S - 1):
        n = column_lengths[j] if j < len(column_lengths) else int(rng.integers(0, 6))
        r = rng.choice(T - len(long_rows), size=n, replace=False)
        if n >= 2 and j % 3 == 1:
            r[1] = r[0]  # a duplicate (i, j)
        rows.append(r), cols.append(np.full(n, j))
    for a, n in enumerate(long_rows):  # the last rows: long, over the ordinary columns only (duplicates when n > their number)
        rows.append(np.full(n, T - len(long_rows) + a)), cols.append(rng.integers(len(COLUMN_LENGTHS) + 1, S - 1, size=n))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    w = rng.uniform(0.1, 2.0, size=rows.size)
    w[cols == ZERO_COLUMN] = 0.0
    shuffle = rng.permutation(rows.size)
    rows, cols, w = rows[shuffle], cols[shuffle], w[shuffle]
    order = np.argsort(rows, kind="stable")
    rows, cols, w = rows[order], cols[order], w[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=T))]).astype(np.int64)
    # one zero-weight entry in a row with other entries (what `sum` still adds)
    i = int(np.flatnonzero((np.diff(indptr) >= 3) & (np.diff(indptr) < 10))[0])
    w[indptr[i] + 1] = 0.0
    for a in (w, cols, indptr):
        a.setflags(write=False)
    return w, cols.astype(np.int64), indptr, T, S


def case_data(T, S, K=17, seed=3):
    """v (K, S): small dyadic values (exact in float32 too), NaN in plane 1 only; g (K, T) normal."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, size=(K, S)).astype(np.float64) / 4.0
    if K > 1:
        v[1, rng.random(S) < 0.15] = np.nan
    g = rng.normal(size=(K, T))
    return v, g


def gradient_for(method, data, indices, indptr, v, g):
    """g with NaN on the rows that are not live (what a caller's masked loss leaves there)"""
    return np.where(live_rows(method, data, indices, indptr, v), g, np.nan)


def dyadic_matrix():
    """Dyadic weights with power-of-two sums over every row's valid entries under ``dyadic_values``: the
    forward, its difference quotient and the adjoint are all exact.  Rows: plain, with a NaN entry, with a zero-weight entry,
    all-NaN, only zero weights, empty, a duplicate (i, j)."""
    S = 8
    rows = [
        [(0, 2.0), (1, 1.0), (2, 1.0)],            # plain, sum 4
        [(3, 0.5), (4, 3.0), (1, 0.25), (2, 0.25)],  # column 4 is NaN in plane 1: sum 1 without it, 4 with it
        [(5, 1.0), (0, 0.0), (6, 1.0)],            # a zero-weight entry
        [(4, 2.0)],                                # all-NaN in plane 1
        [(6, 0.0), (7, 0.0)],                      # only zero weights: never live for the w-sum methods
        [],                                        # empty
        [(2, 0.5), (2, 1.0), (2, 0.5)],            # duplicate (i, j) with different weights
        [(7, 8.0)],                                # all-NaN in plane 2
    ]
    data = np.array([w for r in rows for _, w in r], dtype=np.float64)
    indices = np.array([j for r in rows for j, _ in r], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return data, indices, indptr, len(rows), S


def dyadic_values():
    """v (3, 8) small integers; plane 1 has NaN in column 4, plane 2 in columns 0 and 7"""
    v = np.array([[3, -2, 5, 1, 4, -7, 2, 6], [1, 4, -3, 2, np.nan, 5, -1, 3], [np.nan, 2, 1, -4, 3, 2, 5, np.nan]], dtype=np.float64)
    return v
