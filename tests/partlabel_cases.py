"""Yardstick and fixtures of the part-label tests (test_partlabel_cpu.py, test_gpu_partlabel.py): numpy / scipy only.

``label`` is the rule of include/xugrid_amd.h (xr_graph_partition_dev) restated in numpy: ``hilbert_keys`` and ``seed`` are its
steps 1 and 2, ``refine`` its step 3 with counters, ``cut`` the edge cut.  The device must give these labels exactly."""
import numpy as np
from scipy import sparse

import rcm_cases as rc

MAX_ROUNDS = 16
EPS = (3, 100)  # a part may weigh 1.03 T / P
CELLS = 65536


def canonical(A):
    return rc.canonical(A)


# ---- step 1: the curve key
def hilbert_index(cx, cy):
    """The xy -> d walk over a CELLS x CELLS raster, on integer arrays."""
    x, y = np.array(cx, dtype=np.int64), np.array(cy, dtype=np.int64)
    d = np.zeros(x.shape, dtype=np.int64)
    s = CELLS // 2
    while s > 0:
        rx = ((x & s) > 0).astype(np.int64)
        ry = ((y & s) > 0).astype(np.int64)
        d += s * s * ((3 * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x = np.where(flip, CELLS - 1 - x, x)
        y = np.where(flip, CELLS - 1 - y, y)
        x, y = np.where(ry == 0, y, x), np.where(ry == 0, x, y)
        s >>= 1
    return d


def cells(xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    side = max(hi[0] - lo[0], hi[1] - lo[1])
    scale = 65536.0 / max(side, 1e-300)
    return np.clip(np.floor((xy - lo) * scale), 0, CELLS - 1).astype(np.int64)


def hilbert_keys(xy):
    c = cells(xy)
    return hilbert_index(c[:, 0], c[:, 1])


# ---- step 2: order and split
def used_weights(w, n):
    """int64 weights; absent or all-zero weights count as all ones."""
    if w is None:
        return np.ones(n, dtype=np.int64)
    w = np.asarray(w).astype(np.int64)
    return w if w.sum() > 0 else np.ones(n, dtype=np.int64)


def seed(xy, w, P):
    n = len(xy)
    w = used_weights(w, n)
    order = np.lexsort((np.arange(n), hilbert_keys(xy)))
    before = np.cumsum(w[order]) - w[order]
    labels = np.empty(n, dtype=np.int64)
    labels[order] = np.minimum(P - 1, before * P // w.sum())
    return labels


# ---- step 3: refinement
def bounds(T, P):
    """-> (Lmin, L) in integers."""
    num, den = EPS
    L = max(-(-T // P), T * (den + num) // (den * P))
    Lmin = min(T // P, -(-(T * (den - num)) // (den * P)))
    return int(Lmin), int(L)


def _entries(A):
    """(row, column) of the stored entries off the diagonal."""
    A = canonical(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = rows != A.indices
    return rows[keep], A.indices[keep].astype(np.int64)


def cut(A, labels):
    r, c = _entries(A)
    return int((labels[r] != labels[c]).sum()) // 2


def part_weights(labels, w, P):
    W = np.zeros(P, dtype=np.int64)
    np.add.at(W, labels, 1 if w is None else w)
    return W


def _ranked_sums(part, gain, ids, w):
    """For the movers ``ids`` with their ``part`` and ``gain``: the inclusive sum of ``w`` over the movers of the same part ranked
    by (gain descending, id ascending) up to and including each."""
    by = np.lexsort((ids, -gain, part))
    incl = np.cumsum(w[ids[by]])
    start = np.concatenate(([True], part[by][1:] != part[by][:-1]))
    base = np.maximum.accumulate(np.where(start, incl - w[ids[by]], 0))  # (the sums ascend: the last start's value is the largest)
    out = np.empty(len(ids), dtype=np.int64)
    out[by] = incl - base
    return out


def one_round(r, c, labels, w, P, Lmin, L, capped=True):
    """-> (new labels, accepted moves, movers rejected by a budget, the sum of the accepted gains)."""
    n = labels.size
    pair, counts = np.unique(r * P + labels[c], return_counts=True)
    row, lab = pair // P, pair % P
    own = np.zeros(n, dtype=np.int64)
    mine = lab == labels[row]
    own[row[mine]] = counts[mine]
    row, lab, counts = row[~mine], lab[~mine], counts[~mine]
    by = np.lexsort((lab, -counts, row))  # per row: the largest count first, the smallest label on a tie
    row, lab, counts = row[by], lab[by], counts[by]
    first = np.concatenate(([True], row[1:] != row[:-1])) if row.size else np.zeros(0, dtype=bool)
    gain = np.zeros(n, dtype=np.int64)
    dest = labels.copy()
    gain[row[first]] = counts[first] - own[row[first]]
    dest[row[first]] = lab[first]
    gain[gain < 0] = 0
    candidate = gain > 0
    outranked = candidate[c] & ((gain[c] > gain[r]) | ((gain[c] == gain[r]) & (c < r)))
    blocked = np.zeros(n, dtype=bool)
    blocked[r[outranked]] = True
    movers = np.nonzero(candidate & ~blocked)[0]
    if movers.size == 0:
        return labels, 0, 0, 0
    W = part_weights(labels, w, P)
    if capped:
        into = _ranked_sums(dest[movers], gain[movers], movers, w) <= L - W[dest[movers]]
        out_of = _ranked_sums(labels[movers], gain[movers], movers, w) <= W[labels[movers]] - Lmin
        accepted = movers[into & out_of]
    else:
        accepted = movers
    new = labels.copy()
    new[accepted] = dest[accepted]
    return new, int(accepted.size), int(movers.size - accepted.size), int(gain[accepted].sum())


def refine(A, labels, w, P, capped=True):
    """-> (labels, counters): ``rounds`` run (a last round without a move counts), ``accepted`` moves per round, ``rejected``
    movers per round (failed a budget), ``gains`` the sum of the accepted gains per round, ``cuts`` the cut before the first
    round and behind every round."""
    n = A.shape[0]
    w = used_weights(w, n)
    T = int(w.sum())
    Lmin, L = bounds(T, P)
    r, c = _entries(A)
    counters = dict(rounds=0, accepted=[], rejected=[], gains=[], cuts=[cut(A, labels)])
    labels = labels.copy()
    if P == 1 or T // P == 0:
        return labels, counters
    while counters["rounds"] < MAX_ROUNDS:
        labels, accepted, rejected, gains = one_round(r, c, labels, w, P, Lmin, L, capped)
        counters["rounds"] += 1
        counters["accepted"].append(accepted)
        counters["rejected"].append(rejected)
        counters["gains"].append(gains)
        counters["cuts"].append(cut(A, labels))
        if accepted == 0:
            break
    return labels, counters


_LABELLED = {}


def label(A, xy, P, w=None, name=None):
    """-> (labels, counters) of the whole rule; with ``name`` computed once and kept (treat as read-only)."""
    if name is not None and name in _LABELLED:
        return _LABELLED[name]
    A = canonical(A)
    out = refine(A, seed(xy, w, P), w, P)
    if name is not None:
        out[0].setflags(write=False)
        _LABELLED[name] = out
    return out


# ---- fixtures
def generate_mesh_2d(nx, ny):
    """The quad mesh of the reference's tests/test_partitioning.py -> (node_xy, faces)."""
    points = np.array([(x, y) for y in range(ny + 1) for x in range(nx + 1)], dtype=np.float64)
    faces = np.array([[i + j * (nx + 1), i + 1 + j * (nx + 1), i + 1 + (j + 1) * (nx + 1), i + (j + 1) * (nx + 1)]
                      for j in range(ny) for i in range(nx)], dtype=np.int64)
    return points, faces


def generate_mesh_1d(n):
    """The chain of the reference's tests -> (node_xy, edges)."""
    p = np.linspace(0, n, n + 1)
    return np.column_stack([p, p]), np.column_stack([np.arange(n), np.arange(1, n + 1)]).astype(np.int64)


def face_centroids(xy, faces):
    """The vertex mean of every face (what the grids' centroids are for triangles and for the quads used here)."""
    faces = np.asarray(faces)
    valid = faces >= 0
    pts = np.where(valid[..., None], xy[np.where(valid, faces, 0)], 0.0)
    return pts.sum(axis=1) / valid.sum(axis=1)[:, None]


def edge_graph(edges):
    """Edges that share a node -> canonical CSR (n_edge, n_edge), no diagonal."""
    edges = np.asarray(edges, dtype=np.int64)
    n_edge, n_node = len(edges), int(edges.max()) + 1 if len(edges) else 0
    B = sparse.coo_matrix((np.ones(2 * n_edge), (np.repeat(np.arange(n_edge), 2), edges.ravel())), shape=(n_edge, n_node)).tocsr()
    A = (B @ B.T).tolil()
    A.setdiag(0)
    A = canonical(A.tocsr())
    A.eliminate_zeros()
    A.data[:] = 1.0
    return A


def edge_midpoints(xy, edges):
    return 0.5 * (xy[edges[:, 0]] + xy[edges[:, 1]])


def half_weights(n):
    w = np.ones(n, dtype=np.int64)
    w[: n // 2] = 2
    return w


def chain_graph(n):
    """A path of n vertices on the x axis -> (A, xy)."""
    i = np.arange(max(n - 1, 0))
    A = sparse.coo_matrix((np.ones(2 * i.size), (np.concatenate([i, i + 1]), np.concatenate([i + 1, i]))), shape=(n, n))
    return canonical(A), np.column_stack([np.arange(n, dtype=np.float64), np.zeros(n)])


def raster_graph(nx, ny):
    """The 4-neighbour graph of an nx x ny raster of unit cells, row-major -> (A, xy of the cell centres)."""
    k = np.arange(nx * ny).reshape(ny, nx)
    a = np.concatenate([k[:, :-1].ravel(), k[:-1, :].ravel()])
    b = np.concatenate([k[:, 1:].ravel(), k[1:, :].ravel()])
    A = sparse.coo_matrix((np.ones(2 * a.size), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(nx * ny, nx * ny))
    j, i = np.divmod(np.arange(nx * ny), nx)
    return canonical(A), np.column_stack([i + 0.5, j + 0.5])


def hub_network(n_spokes=40, tail=3):
    """A network with one junction of ``n_spokes`` edges, every spoke continued by ``tail`` further edges -> (node_xy, edges)."""
    angle = 2 * np.pi * np.arange(n_spokes) / n_spokes
    xy, edges = [np.zeros((1, 2))], []
    for k in range(n_spokes):
        previous = 0
        for t in range(1, tail + 2):
            xy.append(t * np.array([[np.cos(angle[k]), np.sin(angle[k])]]))
            edges.append((previous, len(xy) - 1))
            previous = len(xy) - 1
    return np.vstack(xy), np.array(edges, dtype=np.int64)
