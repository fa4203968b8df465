"""The yardstick and the cases of the partial-state tests (test_partial_cpu.py, test_gpu_partial.py).

The yardstick restates, in numpy, the component table of include/xugrid_amd.h ("Multi-GPU (source faces sharded over
ranks ...)") and the reducers of xugrid/regrid/reduce.py:16-123, 206-222.  Nothing here calls the code under test;
the one import from the package is its host-side numpy mesh generator (built_meshes).

A partial state of a reducer is C numbers per (target row, variable); over the row's valid entries (v = value, w = weight):

  mean, first_order_conservative   [sum w v, sum w]                                     -> c0 / c1 resp. c0
  sum                              [sum v,   sum w]                                     -> c0
  harmonic_mean                    [sum w,   sum w / v]      (v != 0, w > 0)            -> c0 / c1
  geometric_mean                   [sum w (all entries), sum w ln v, sum w (v > 0, w > 0), #(v < 0)]  -> exp(c1 / c2)
  minimum / maximum                [max(-v) resp. max v, max w]                         combined with MAX

Sums run left to right in CSR order from +0.0 (np.bincount with weights adds exactly so); a product or a quotient is
rounded once.  MAX is the IEEE 754-2019 `maximum` on non-NaN numbers: -0.0 < +0.0.
"""
import math

import numpy as np

IDS = {"mean": 0, "harmonic_mean": 1, "geometric_mean": 2, "sum": 3, "minimum": 4, "maximum": 5, "first_order_conservative": 8}
NAMES = tuple(IDS)
MEAN, HARMONIC, GEOMETRIC, SUM, MINIMUM, MAXIMUM, CONSERVATIVE = (IDS[n] for n in NAMES)
LONG = 32  # rows beyond this many entries are reduced by a wave: another summation order


def components(method_id):
    return 4 if method_id == GEOMETRIC else 2


def is_max(method_id):
    return method_id in (MINIMUM, MAXIMUM)


def summed(method_id):
    """the components that are sums of rounded terms (the others are maxima or counts: exact in any order)"""
    if is_max(method_id):
        return ()
    return (0, 1, 2) if method_id == GEOMETRIC else (0, 1)


def identity(method_id, shape):
    out = np.zeros((components(method_id),) + tuple(shape))
    if is_max(method_id):
        out[0] = -np.inf
    return out


def max2(a, b):
    """IEEE maximum of non-NaN arrays: of two zeros of different sign the positive one"""
    r = np.maximum(a, b)
    both = (a == 0) & (b == 0)
    return np.where(both, np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), r)


def _row_max(rows, x, T, init):
    out = np.full(T, init)
    np.maximum.at(out, rows, x)
    plus = np.bincount(rows[(x == 0) & ~np.signbit(x)], minlength=T) > 0
    if init == 0:
        plus[:] = True
    zero = out == 0
    out[zero] = np.where(plus[zero], 0.0, -0.0)
    return out


def _terms(method_id, values, weights):
    """-> [(selection, term per entry)] for every summed component, in component order"""
    v, w = np.asarray(values, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    valid = ~np.isnan(v)
    with np.errstate(all="ignore"):
        if method_id in (MEAN, CONSERVATIVE):
            return [(valid, w * v), (valid, w)]
        if method_id == SUM:
            return [(valid, v), (valid, w)]
        if method_id == HARMONIC:
            sel = valid & (v != 0) & (w > 0)
            return [(sel, w), (sel, w / np.where(sel, v, 1.0))]
        if method_id == GEOMETRIC:
            sel = (v > 0) & (w > 0)
            return [(np.ones(v.size, dtype=bool), w), (sel, w * np.log(np.where(sel, v, 1.0))), (sel, w)]
    raise ValueError(method_id)


def states(method_id, values, weights, rows, T):
    """values, weights, rows: one per entry, in CSR order (values = the source gathered through the column ids; float32
    sources widened first).  -> (C, T)"""
    v, w = np.asarray(values).astype(np.float64), np.asarray(weights, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    out = identity(method_id, (T,))
    if is_max(method_id):
        valid = ~np.isnan(v)
        x = v[valid] if method_id == MAXIMUM else -v[valid]
        out[0] = _row_max(rows[valid], x, T, -np.inf)
        out[1] = _row_max(rows[valid], w[valid], T, 0.0)
        return out
    with np.errstate(all="ignore"):
        for c, (sel, term) in enumerate(_terms(method_id, v, w)):
            out[c] = np.bincount(rows[sel], weights=term[sel], minlength=T)
    if method_id == GEOMETRIC:
        out[3] = np.bincount(rows[v < 0], minlength=T)
    return out


def magnitudes(method_id, values, weights, rows, T):
    """sum |term| per summed component (zeros elsewhere) -> (C, T)"""
    out = np.zeros((components(method_id), T))
    if is_max(method_id):
        return out
    rows = np.asarray(rows, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c, (sel, term) in enumerate(_terms(method_id, np.asarray(values).astype(np.float64), weights)):
            out[c] = np.bincount(rows[sel], weights=np.abs(term[sel]), minlength=T)
    return out


def _exact_sum(terms):
    if np.isfinite(terms).all():
        return math.fsum(terms)
    with np.errstate(all="ignore"):
        return float(np.sum(terms))  # NaN, or an infinity: the same in any order


def fsum_states(method_id, values, weights, indptr, which):
    """The summed components of the rows `which`, each the correctly rounded sum of its (rounded) terms.
    -> {component: array over `which`}"""
    out = {}
    if is_max(method_id):
        return out
    for c, (sel, term) in enumerate(_terms(method_id, np.asarray(values).astype(np.float64), weights)):
        out[c] = np.array([_exact_sum(term[indptr[t]:indptr[t + 1]][sel[indptr[t]:indptr[t + 1]]]) for t in which])
    return out


def combine(method_id, list_of_states):
    """element-wise, from the identity, in the given (sender) order"""
    list_of_states = list(list_of_states)
    out = identity(method_id, np.shape(list_of_states[0])[1:]) if list_of_states else None
    with np.errstate(all="ignore"):
        for s in list_of_states:
            out = max2(out, np.asarray(s)) if is_max(method_id) else out + np.asarray(s)
    return out


def finalize(method_id, c):
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        if method_id == MEAN:
            return np.where(c[1] == 0, np.nan, c[0] / c[1])
        if method_id in (SUM, CONSERVATIVE):
            return np.where(c[1] == 0, np.nan, c[0])
        if method_id == HARMONIC:
            return np.where((c[1] == 0) | (c[0] == 0), np.nan, c[0] / c[1])
        if method_id == GEOMETRIC:
            return np.where((c[0] == 0) | (c[3] > 0) | (c[2] == 0), np.nan, np.exp(c[1] / c[2]))
        if method_id == MINIMUM:
            return np.where(c[1] == 0, np.nan, -c[0])
        if method_id == MAXIMUM:
            return np.where(c[1] == 0, np.nan, c[0])
    raise ValueError(method_id)


# ---- matrices ----------------------------------------------------------------------------------------------------------------
T_EDGES, S_EDGES = 1101, 907  # T: no multiple of 64, 128 or 256
WINDOW_ROWS = range(128, 192)  # 64 rows x 32 entries: one wave window of 2048 entries, six chunks of 384
JUMPY_WINDOW = range(256, 320)  # short rows around rows of 33 and 600 entries
SINGLE_LONG = {400: 33, 450: 64, 520: 65, 590: 384, 660: 385, 730: 880}


def edge_lengths(seed=7, long_rows=True):
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 9, T_EDGES)
    n[0] = 0
    n[rng.choice(np.arange(1, T_EDGES), 40, replace=False)] = 0
    n[list(WINDOW_ROWS)] = 32
    n[262], n[280], n[301] = 33, 600, 33
    for r, length in SINGLE_LONG.items():
        n[r] = length
    n[T_EDGES - 1] = 100
    return n if long_rows else np.minimum(n, LONG)


def csr_from_lengths(n, S, seed):
    """columns ascending and distinct inside a row, weights in (0.1, 1) with 2 % exact zeros -> (data, indices, indptr)"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(S, int(k), replace=False)) for k in n]).astype(np.int64)
    data = rng.uniform(0.1, 1.0, indices.size)
    data[rng.random(indices.size) < 0.02] = 0.0
    return data, indices, indptr


def edges():
    return csr_from_lengths(edge_lengths(), S_EDGES, 11) + (T_EDGES, S_EDGES)


def short_only():
    return csr_from_lengths(edge_lengths(long_rows=False), S_EDGES, 11) + (T_EDGES, S_EDGES)


def row_ids(indptr):
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr))


def built_meshes():
    """(source xy, faces), (target xy, faces): a fine target plus two faces that cover nearly the whole source"""
    from xugrid_amd import meshgen  # (mesh generation only: host numpy)

    sxy, sf = meshgen.triangle_mesh(3000, 0)
    fxy, ff = meshgen.triangle_mesh(1000, 4, 10.0, 0.9)
    big = np.array([[0.02, 0.02], [0.98, 0.03], [0.97, 0.99], [0.03, 0.96]])
    n0 = fxy.shape[0]
    return (sxy, sf), (np.vstack([fxy, big]), np.vstack([ff, [[n0, n0 + 1, n0 + 2], [n0, n0 + 2, n0 + 3]]]))


# ---- sources -----------------------------------------------------------------------------------------------------------------
SOURCES = ("mixed", "positive", "zeros", "negative", "all_nan", "inf", "signed_zero")


def source(name, S, seed=3):
    rng = np.random.default_rng([seed, SOURCES.index(name)])
    if name == "mixed":
        v = rng.normal(size=S)
        v[rng.random(S) < 0.05] = np.nan
    elif name == "positive":
        v = rng.uniform(0.5, 3.0, S)
    elif name == "zeros":
        v = rng.uniform(0.5, 3.0, S)
        v[rng.random(S) < 0.3] = 0.0
    elif name == "negative":
        v = -rng.uniform(0.5, 3.0, S)
    elif name == "all_nan":
        v = np.full(S, np.nan)
    elif name == "inf":
        v = rng.normal(size=S)
        at = rng.choice(S, 40, replace=False)
        v[at[:20]], v[at[20:]] = np.inf, -np.inf
    elif name == "signed_zero":
        v = np.where(rng.random(S) < 0.5, 0.0, -0.0)
    else:
        raise ValueError(name)
    return v


def stack(S, K, seed=3):
    """(K, S): variable k is source k mod 7 (a fresh draw per turn) -> (block, names)"""
    names = [SOURCES[k % len(SOURCES)] for k in range(K)]
    return np.stack([source(nm, S, seed + k // len(SOURCES)) for k, nm in enumerate(names)]), names


def column_shards(S, P, seed=5):
    """P disjoint column sets covering 0..S-1, ascending inside a shard, scattered over the shards; with P > 1 one is empty"""
    rng = np.random.default_rng([seed, P])
    owner = rng.integers(0, max(P - 1, 1), S)
    empty = P // 2 if P > 1 else -1
    owner = np.where(owner >= empty, owner + 1, owner) if P > 1 else owner
    return [np.flatnonzero(owner == p) for p in range(P)]


def shard_csr(data, indices, indptr, cols, S):
    """the columns `cols` of the matrix in shard-local column ids, entry order kept -> (data, indices, indptr)"""
    local = np.full(S, -1, dtype=np.int64)
    local[cols] = np.arange(cols.size)
    keep = local[indices] >= 0
    counts = np.bincount(row_ids(indptr)[keep], minlength=indptr.size - 1)
    return data[keep], local[indices[keep]], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
