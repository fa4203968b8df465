"""
The rule of the layered (3-D) overlap weights restated in vectorised numpy, a triple-loop brute force
of the same rule, and the seeded column generators the layered tests share.

    dz = min(top_s[ls, i], top_t[lt, j]) - max(bottom_s[ls, i], bottom_t[lt, j]),  kept where dz > 0

(np.minimum / np.maximum hand a NaN on and ``NaN > 0`` is false: a NaN bound removes the layer; ``top <= bottom`` gives
``dz <= 0``.)  Weights are single IEEE operations, so the device must return the same bits.
"""
import json
import os

import numpy as np

QUARTER = 0.25  # every generated bound is a multiple of it: overlaps, products with dyadic areas and their sums are exact


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _columns(a, n_col):
    """(n_layer, n_col) view of top / bottom given as (n_layer,), (n_layer, n_col) or (n_layer, ny, nx)"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return np.broadcast_to(a[:, None], (a.shape[0], n_col))
    return a.reshape(a.shape[0], n_col)


def layered_csr(indptr2, indices2, data2, n_s, top_s, bottom_s, top_t, bottom_t, relative=False):
    """The 3-D matrix of the 2-D CSR (rows = target cells, in the caller's ids): -> (data, indices, indptr, n, m) with row
    ``lt * n_t + j``, column ``ls * n_s + i``; a row keeps the 2-D row's order of i, ls ascending within one i."""
    indptr2, indices2, data2 = np.asarray(indptr2, dtype=np.int64), np.asarray(indices2, dtype=np.int64), np.asarray(data2)
    n_t = indptr2.size - 1
    ts, bs, tt, bt = _columns(top_s, n_s), _columns(bottom_s, n_s), _columns(top_t, n_t), _columns(bottom_t, n_t)
    n_layer_s, n_layer_t = ts.shape[0], tt.shape[0]
    j = np.repeat(np.arange(n_t), np.diff(indptr2))
    # axes (lt, p, ls): C order of the kept entries is the order of the matrix
    st, sb = ts[:, indices2].T[None, :, :], bs[:, indices2].T[None, :, :]
    with np.errstate(invalid="ignore"):
        dz = np.minimum(st, tt[:, j][:, :, None]) - np.maximum(sb, bt[:, j][:, :, None])
        lt, p, ls = np.nonzero(dz > 0)
        dz = dz[lt, p, ls]
        if relative:
            data = data2[p] * (dz / (ts[ls, indices2[p]] - bs[ls, indices2[p]]))
        else:
            data = data2[p] * dz
    indices = ls * n_s + indices2[p]
    indptr = np.zeros(n_layer_t * n_t + 1, dtype=np.int64)
    np.cumsum(np.bincount(lt * n_t + j[p], minlength=n_layer_t * n_t), out=indptr[1:])
    return data, indices, indptr, n_layer_t * n_t, n_layer_s * n_s


def pair_triplets(source_bounds, target_bounds, source_index, target_index):
    """The rule on (n, Ls, 2) / (m, Lt, 2) bounds of (lower, upper) for the column pairs (source_index[k], target_index[k]):
    -> (source column * Ls + ls, target column * Lt + lt, dz), ordered by pair, lt, ls -- overlap_1d_nd's ids and order."""
    source_bounds, target_bounds = np.asarray(source_bounds, dtype=np.float64), np.asarray(target_bounds, dtype=np.float64)
    source_index, target_index = np.asarray(source_index, dtype=np.int64), np.asarray(target_index, dtype=np.int64)
    n_layer_s, n_layer_t = source_bounds.shape[1], target_bounds.shape[1]
    s, t = source_bounds[source_index], target_bounds[target_index]  # (o, L, 2)
    with np.errstate(invalid="ignore"):
        dz = np.minimum(s[:, None, :, 1], t[:, :, None, 1]) - np.maximum(s[:, None, :, 0], t[:, :, None, 0])  # (o, lt, ls)
        k, lt, ls = np.nonzero(dz > 0)
    return source_index[k] * n_layer_s + ls, target_index[k] * n_layer_t + lt, dz[k, lt, ls]


def pair_triplets_brute(source_bounds, target_bounds, source_index, target_index):
    """The same, one scalar comparison at a time."""
    out = []
    n_layer_s, n_layer_t = source_bounds.shape[1], target_bounds.shape[1]
    for i, j in zip(source_index, target_index):
        for lt in range(n_layer_t):
            tl, tu = target_bounds[j, lt]
            for ls in range(n_layer_s):
                sl, su = source_bounds[i, ls]
                if np.isnan(tl) or np.isnan(tu) or np.isnan(sl) or np.isnan(su):
                    continue
                dz = (su if su < tu else tu) - (sl if sl > tl else tl)
                if dz > 0:
                    out.append((i * n_layer_s + ls, j * n_layer_t + lt, dz))
    if not out:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    s, t, w = zip(*out)
    return np.array(s, dtype=np.int64), np.array(t, dtype=np.int64), np.array(w, dtype=np.float64)


def layered_csr_brute(indptr2, indices2, data2, n_s, top_s, bottom_s, top_t, bottom_t, relative=False):
    """``layered_csr`` as loops over rows (lt, j), the entries of 2-D row j and the source layers."""
    n_t = len(indptr2) - 1
    ts, bs, tt, bt = _columns(top_s, n_s), _columns(bottom_s, n_s), _columns(top_t, n_t), _columns(bottom_t, n_t)
    data, indices, indptr = [], [], [0]
    for lt in range(tt.shape[0]):
        for j in range(n_t):
            for p in range(indptr2[j], indptr2[j + 1]):
                i = indices2[p]
                for ls in range(ts.shape[0]):
                    bounds = (ts[ls, i], bs[ls, i], tt[lt, j], bt[lt, j])
                    if any(np.isnan(b) for b in bounds):
                        continue
                    dz = min(bounds[0], bounds[2]) - max(bounds[1], bounds[3])
                    if dz > 0:
                        indices.append(ls * n_s + i)
                        data.append(data2[p] * (dz / (bounds[0] - bounds[1])) if relative else data2[p] * dz)
            indptr.append(len(indices))
    return (np.array(data, dtype=np.float64), np.array(indices, dtype=np.int64), np.array(indptr, dtype=np.int64),
            tt.shape[0] * n_t, ts.shape[0] * n_s)


def to_bounds(top, bottom):
    """(n_layer, n_col) top / bottom -> (n_col, n_layer, 2) bounds of (lower, upper)"""
    return np.ascontiguousarray(np.stack([np.asarray(bottom).T, np.asarray(top).T], axis=-1))


# ---- the columns ----------------------------------------------------------------------------------------------------------------
EXTENT = 160  # quarter steps of the shared extent [0, 40]: room for 65 layers of positive thickness


def columns(seed, n_col, n_layer, kind="shared"):
    """-> (top, bottom) float64 (n_layer, n_col), every bound a multiple of QUARTER.

    shared      NaN-free, positive thickness, bottom-up, every column fills [0, EXTENT * QUARTER] (where the reference's
                overlap_1d_nd is a valid oracle)
    ragged      columns of different extent, some layers of zero thickness
    nan         ``shared`` with layers missing (NaN top and bottom), some columns entirely
    descending  ``ragged``, top-down
    shuffled    ``ragged`` with the layers of every column in an order of its own
    """
    rng = np.random.default_rng(seed)
    edges = np.empty((n_layer + 1, n_col))
    for c in range(n_col):
        if kind in ("shared", "nan"):
            cuts = np.sort(rng.choice(np.arange(1, EXTENT), n_layer - 1, replace=False))
            edges[:, c] = np.concatenate(([0], cuts, [EXTENT]))
        else:
            lo = rng.integers(0, EXTENT // 4)
            edges[:, c] = lo + np.sort(rng.integers(0, EXTENT // 2, n_layer + 1))  # repeats: zero thickness
            edges[0, c] = lo
    bottom, top = edges[:-1] * QUARTER, edges[1:] * QUARTER
    if kind == "nan":
        gone = rng.random((n_layer, n_col)) < 0.3
        gone[:, rng.integers(0, n_col)] = True
        top, bottom = np.where(gone, np.nan, top), np.where(gone, np.nan, bottom)
    elif kind == "descending":
        top, bottom = top[::-1], bottom[::-1]
    elif kind == "shuffled":
        order = np.argsort(rng.random((n_layer, n_col)), axis=0)
        top, bottom = np.take_along_axis(top, order, axis=0), np.take_along_axis(bottom, order, axis=0)
    return np.ascontiguousarray(top), np.ascontiguousarray(bottom)


KINDS = ("shared", "ragged", "nan", "descending", "shuffled")

# the layer counts (source, target) of the golden file
GOLDEN_LAYERS = ((1, 1), (1, 5), (5, 1), (4, 7), (9, 3), (31, 17))
GOLDEN_COLUMNS = 6


def golden_case(n_layer_s, n_layer_t):
    """The inputs of one golden case: shared-extent columns, one pair per target column."""
    seed = 1000 * n_layer_s + n_layer_t
    source_bounds = to_bounds(*columns(seed, GOLDEN_COLUMNS + 1, n_layer_s))
    target_bounds = to_bounds(*columns(seed + 500, GOLDEN_COLUMNS, n_layer_t))
    source_index = np.random.default_rng(seed).integers(0, GOLDEN_COLUMNS + 1, GOLDEN_COLUMNS)
    return source_bounds, target_bounds, source_index, np.arange(GOLDEN_COLUMNS)


def random_csr(seed, n_t, n_s, nnz):
    """A 2-D weight matrix with exactly nnz entries: rows of random length (some empty), columns in random order, weights that
    are multiples of 1 / 16."""
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.integers(0, n_t, nnz))
    indptr = np.zeros(n_t + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_t), out=indptr[1:])
    return rng.integers(1, 64, nnz) / 16.0, rng.integers(0, n_s, nnz), indptr


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layered_known.json")


def load_golden():
    with open(GOLDEN) as f:
        cases = json.load(f)
    out = {}
    for name, case in cases.items():
        out[name] = {k: np.array(v, dtype=np.float64 if k.endswith("bounds") or k == "overlap" else np.int64)
                     for k, v in case.items()}  # (None -> NaN)
    return out


def touching():
    """two layers on each side that meet at 1.0 and a target that only touches the source from above"""
    top_s, bottom_s = np.array([[1.0], [2.0]]), np.array([[0.0], [1.0]])
    top_t, bottom_t = np.array([[1.0], [3.0], [2.5]]), np.array([[0.5], [2.0], [1.0]])
    return top_s, bottom_s, top_t, bottom_t
