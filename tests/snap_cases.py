"""
Yardsticks and cases of the snapping tests (xugrid_amd/snap.py, csrc/xr_snap.hip).

The restatements say what ``snap_nodes`` and ``snap_to_nodes`` compute in this project's own words, with numpy and scipy:
tests/test_snap_cpu.py pins them to what the reference's functions return (tests/golden/snap_known.json, written by
tests/golden/gen_snap.py), and tests/test_gpu_snap.py compares the device with them, exactly.

"Within the distance" is ``dx * dx + dy * dy <= d * d`` in float64, inclusive.  The KD-tree is only used to find candidates, with
a slightly larger radius; every pair is then tested here with that expression.
"""
import numpy as np
from scipy.spatial import cKDTree

from netedit_cases import DIGEST_FROM, digest, equals_known, random_network  # noqa: F401

BAD_TIEBREAKER = 'Invalid tiebreaker: {}, should be one of {{None, "nearest"}} instead.'
TIES = "Ties detected: multiple options to snap to, given max distance: set a smaller tolerance or specify a tiebreaker."


# ---- restatements -----------------------------------------------------------------------------------------------------------------
def pairs_within(x, y, to_x, to_y, d):
    """-> (i, j, squared distance) of every pair of a point i of (x, y) and a point j of (to_x, to_y) within ``d``, sorted by i,
    then j."""
    a, b = np.column_stack([x, y]), np.column_stack([to_x, to_y])
    if len(a) == 0 or len(b) == 0:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0)
    found = cKDTree(a).sparse_distance_matrix(cKDTree(b), max_distance=d * (1.0 + 1e-9) + 1e-300, output_type="ndarray")
    i, j = found["i"].astype(np.int64), found["j"].astype(np.int64)
    dx, dy = b[j, 0] - a[i, 0], b[j, 1] - a[i, 1]
    d2 = dx * dx + dy * dy
    keep = d2 <= d * d
    i, j, d2 = i[keep], j[keep], d2[keep]
    order = np.lexsort((j, i))
    return i[order], j[order], d2[order]


def snap_nodes_ref(x, y, d):
    """-> (inverse or None, kept ids ascending, x_snapped, y_snapped).

    Point i is kept iff no kept point with a lower number lies within ``d`` (taken in ascending order, that is one pass).  Every
    other point goes to the kept point within ``d`` whose distance, the rounded square root, is smallest; the lowest number
    among equal ones."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    i, j, d2 = pairs_within(x, y, x, y, d)
    other = i != j
    i, j, dist = i[other], j[other], np.sqrt(d2[other])
    if len(i) == 0:
        return None, np.arange(n), x.copy(), y.copy()
    start = np.searchsorted(i, np.arange(n + 1))
    kept = np.zeros(n, dtype=bool)
    covered = np.zeros(n, dtype=bool)
    for p in range(n):
        if not covered[p]:
            kept[p] = True
            covered[j[start[p]:start[p + 1]]] = True
    goes_to = np.arange(n)
    to_kept = kept[j] & ~kept[i]
    pi, pj, pd = i[to_kept], j[to_kept], dist[to_kept]
    order = np.lexsort((pj, pd, pi))  # by point, then distance, then number: the first row of a point is its answer
    pi, pj = pi[order], pj[order]
    first = np.ones(len(pi), dtype=bool)
    first[1:] = pi[1:] != pi[:-1]
    goes_to[pi[first]] = pj[first]
    ids = np.flatnonzero(kept)
    rank = np.cumsum(kept) - 1
    return rank[goes_to], ids, x[ids], y[ids]


def snap_to_nodes_ref(x, y, to_x, to_y, d):
    """-> (x_snapped, y_snapped, index, count): per point the number of nodes within ``d`` and the nearest of them by squared
    distance, the lowest number among equal squares (-1 and a copy of the point without one)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    to_x, to_y = np.asarray(to_x, dtype=np.float64), np.asarray(to_y, dtype=np.float64)
    i, j, d2 = pairs_within(x, y, to_x, to_y, d)
    count = np.bincount(i, minlength=len(x))
    order = np.lexsort((j, d2, i))
    i, j = i[order], j[order]
    first = np.ones(len(i), dtype=bool)
    first[1:] = i[1:] != i[:-1]
    index = np.full(len(x), -1, dtype=np.int64)
    index[i[first]] = j[first]
    hit = index >= 0
    xs, ys = x.copy(), y.copy()
    xs[hit], ys[hit] = to_x[index[hit]], to_y[index[hit]]
    return xs, ys, index, count


# ---- snap_nodes cases: name -> (x, y, d) --------------------------------------------------------------------------------------------
def lattice(n, seed=0):
    """Points on a quarter-unit lattice with about 0.7 points per site: duplicates, and squares that are exact in float64."""
    side = max(2, int(np.ceil(np.sqrt(n / 0.7))))
    at = np.random.default_rng(seed).integers(0, side, (n, 2))
    return at[:, 0] * 0.25, at[:, 1] * 0.25


def scattered(n, seed=1):
    """Random points, about one per unit square."""
    xy = np.random.default_rng(seed).random((n, 2)) * np.sqrt(n)
    return xy[:, 0], xy[:, 1]


def chain(n, d=0.25):
    """Points spaced exactly ``d`` along a line, numbered along it: every decision waits for the one before."""
    return np.arange(n) * d, np.zeros(n)


def chain_reversed(n, d=0.25):
    x, y = chain(n, d)
    return x[::-1].copy(), y


def chain_interleaved(n, d=0.25):
    """The same line with the even places numbered first: no place has a lower-numbered neighbour on both sides."""
    x, y = chain(n, d)
    return np.concatenate([x[0::2], x[1::2]]), y


def index_cell(extent, n):
    """The cell size of the nearest index over ``n`` points in a square of side ``extent`` (csrc/xr_sample.hip: size_grid)."""
    return np.sqrt(extent * extent / max(1.0, n / 2.0))


def spread(n=200, seed=2):
    """Few points over a large square (most cells of the index are empty) and a tight cluster of 9 around a corner of its cells."""
    extent = 4096.0
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 4096, (n, 2)).astype(np.float64)
    xy[0], xy[1] = (0.0, 0.0), (extent, extent)  # the box is exactly the square
    h = index_cell(extent, n + 9)
    corner = np.array([7 * h, 5 * h])
    cluster = corner + 0.125 * np.array([[a, b] for a in (-1, 0, 1) for b in (-1, 0, 1)])
    xy = np.concatenate([xy[: n // 2], cluster, xy[n // 2:]])
    return xy[:, 0], xy[:, 1]


def coincident(n=100):
    return np.full(n, 3.5), np.full(n, -1.25)


REFERENCE_NODES = {  # the reference's own tests (tests/test_snap.py), inputs; the expected outputs are part of the goldens
    "horizontal": (np.array([0.0, 1.0, 2.0]), np.zeros(3), (0.1, 1.0, 2.0)),
    "diagonal": (np.array([0.0, 1.0, 1.5]), np.array([0.0, 1.0, 1.5]), (0.1, 0.71, 1.42)),
    "two_lines": (np.array([0.0, 1.0, 1.02, 2.0]), np.array([1.0, 0.0, 0.0, 1.0]), (0.1,)),
}
TWO_LINES_EDGES = np.array([[0, 1], [2, 3]], dtype=np.int64)
LATTICE_SIZES = (63, 64, 65, 257, 2049, 4097)
LATTICE_DISTANCES = (0.25, 0.5, 0.75, 1.0)


def _nodes_cases():
    cases = {}
    for name, (x, y, distances) in REFERENCE_NODES.items():
        for d in distances:
            cases[f"ref_{name}_{d}"] = lambda x=x, y=y, d=d: (x, y, d)
    for n in LATTICE_SIZES:
        for d in LATTICE_DISTANCES:
            cases[f"lattice{n}_{d}"] = lambda n=n, d=d: lattice(n, seed=n) + (d,)
    cases["scattered2049"] = lambda: scattered(2049) + (0.5,)
    cases["chain70"] = lambda: chain(70) + (0.25,)
    cases["chain2050"] = lambda: chain(2050) + (0.25,)
    cases["chain2050_reversed"] = lambda: chain_reversed(2050) + (0.25,)
    cases["chain2050_interleaved"] = lambda: chain_interleaved(2050) + (0.25,)
    cases["spread"] = lambda: spread() + (0.25,)
    cases["coincident_d0"] = lambda: coincident() + (0.0,)
    cases["coincident_d05"] = lambda: coincident() + (0.5,)
    cases["apart"] = lambda: scattered(300, seed=5) + (1e-6,)
    cases["one"] = lambda: (np.array([1.5]), np.array([2.5]), 1.0)
    cases["two_near"] = lambda: (np.array([1.5, 1.75]), np.array([2.5, 2.5]), 0.25)
    cases["two_far"] = lambda: (np.array([1.5, 1.75]), np.array([2.5, 2.5]), 0.2)
    cases["none"] = lambda: (np.empty(0), np.empty(0), 1.0)
    return cases


NODES_CASES = _nodes_cases()


# ---- snap_to_nodes cases: name -> (x, y, to_x, to_y, d) -----------------------------------------------------------------------------
_P = np.array([1.0, 2.0, 3.0])
REFERENCE_TO = {  # tests/test_snap.py: test_snap_to_nodes, block by block
    "none_snapped": (_P, _P, _P + 0.1, _P + 0.1, 0.1),
    "all_snapped": (_P, _P, _P + 0.1, _P + 0.1, 0.2),
    "take_nearest": (_P, _P, _P + 0.1, _P + 0.1, 3.0),
    "more_ties": (_P, _P, np.array([1.01, 2.01, 2.002, 3.01]), np.array([1.01, 2.01, 2.002, 3.01]), 0.5),
    "exact_ties": (_P, _P, np.array([1.01, 2.002, 2.002, 3.01]), np.array([1.01, 2.002, 2.002, 3.01]), 0.5),
    "multiple_ties": (_P, _P, np.array([1.01, 2.01, 2.002, 3.002, 3.01]), np.array([1.01, 2.01, 2.002, 3.002, 3.01]), 0.5),
}
RANDOM_SIZES = ((1, 1), (65, 63), (2049, 300), (300, 2049))


def random_to(n, m, seed):
    """``n`` points and ``m`` nodes in one square with about one node per unit."""
    rng = np.random.default_rng(seed)
    side = np.sqrt(m)
    p, t = rng.random((n, 2)) * side, rng.random((m, 2)) * side
    return p[:, 0], p[:, 1], t[:, 0], t[:, 1]


def duplicates_to(seed=7):
    """Nodes on the quarter-unit lattice, every third one repeated; the points are nodes themselves (distance 0) and lattice
    sites next to nodes."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 24, (200, 2)) * 0.25
    t = np.concatenate([t, t[::3]])
    p = np.concatenate([t[rng.permutation(len(t))[:80]], rng.integers(0, 24, (120, 2)) * 0.25])
    return p[:, 0], p[:, 1], t[:, 0], t[:, 1]


def _to_cases():
    cases = {}
    for name, case in REFERENCE_TO.items():
        cases[f"ref_{name}"] = lambda case=case: case
    for n, m in RANDOM_SIZES:
        for label, d in (("none", 1e-4), ("one", 0.3), ("several", 1.5)):
            cases[f"random{n}x{m}_{label}"] = lambda n=n, m=m, d=d: random_to(n, m, seed=n + m) + (d,)
    cases["duplicates_d0"] = lambda: duplicates_to() + (0.0,)
    cases["duplicates_d025"] = lambda: duplicates_to() + (0.25,)
    # exactly at the distance from the only node: it snaps
    cases["at_distance"] = lambda: (np.array([0.75, 4.0]), np.array([1.0, 4.0]), np.array([0.0, 4.0]), np.array([0.0, 4.5]), 1.25)
    return cases


TO_CASES = _to_cases()
# Two distinct nodes at exactly the same distance: the lower number wins HERE; the reference's choice follows its tree, so this
# case is compared with the restatement only
EQUIDISTANT = (np.array([2.0, 5.0]), np.array([1.0, 1.0]), np.array([2.5, 1.5, 5.0, 5.0]), np.array([1.0, 1.0, 1.25, 0.75]), 0.5)


# ---- Ugrid1d.snap_nodes -----------------------------------------------------------------------------------------------------------------
def doubled_network(n_node=2000, offset=1e-5):
    """``random_network`` with every node repeated at a small offset and every edge repeated on the copies."""
    xy, edges = random_network(n_node)
    shift = np.random.default_rng(9).uniform(-offset, offset, xy.shape)
    return np.concatenate([xy, xy + shift]), np.concatenate([edges, edges + n_node]), 4.0 * offset
