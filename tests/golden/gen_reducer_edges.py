"""
Generate golden set G12: the reference's reducers on crafted corner rows, short and long, for the device apply paths.

Runs ONLY in the build container (needs /root/reference, which does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_reducer_edges.py

Like gen_goldens.py it imports xugrid 0.15.3's `reduce` module from /root/reference (pure Python, numba absent ->
xugrid.constants.NoOpNumba) and writes DATA only -- inputs and the reference's outputs -- to
tests/golden/g12_reducer_edges.npz.  No reference source is stored in this repository.

Layout.  A ragged CSR (indptr, data) of T rows whose entry j has column j (S = nnz): every entry has a source cell of its
own, so each row's values are chosen freely.  `indices` is arange(nnz) and NOT stored: deflated it takes 190 KB, two thirds
of the file's budget, for no information.  P = 4 source planes of length S, `planes64[P, S]`, and their float32 casts
`planes32[P, S]`:
  A  every special value, NaN included
  B  A with its NaN replaced by other values (keeps +-inf and +-0.0): the NaN-free plane
  C  all NaN
  D  positive finite values with some NaN and some 0.0 (harmonic and geometric means finite)
and per method name `out64_<name>[P, T]`, `out32_<name>[P, T]` (float32 results from the cast values widened back to
float64, as G2 does).  `is_long[T]` marks the rows of more than 32 entries, `geo_spread` is the largest relative spread
of the reference's geometric_mean over three entry orders of a long row.

Rows (seeded):
  sparse, 0 ... 3 entries    the first 512 rows, every fourth with zero weights only: the row blocks the many-variable apply plan
                            can take (see sparse_rows)
  short, 1 ... 32 entries   G1's crafted rows; rows over the EXTREME alphabet (values +-1e308, 5e-324, 1e-45, 1e-300, 0.1,
                            1/3, 3, +-inf, +-0.0, NaN; weights 0, 1e-300, 1e300, 0.1, random); dyadic rows with tied weights;
                            one run of 64 consecutive rows of 32 entries; some empty rows
  long, 33 ... 4097 entries  shuffled among the short ones.  The DYADIC alphabet only (values +-inf, +-0.0, NaN, +-0.25, +-0.5,
                            +-1, +-2, 4, 4; weights 0, 0.25, 0.5, 1, 1, 2): every partial sum of w v, w, v and w / v is
                            exact, ties are common.  Per length two random rows and six families (see long_rows); the random
                            fill of a long row repeats with a prime period (see Rows.draw)

Asserted here (conditions, not measurements): every method but geometric_mean gives the same value on every long row for
the entry order, the reversed order and a random permutation; every method is finite on at least a quarter of the long
rows of each of the planes A, B and D, geometric_mean on at least half of plane D's; geo_spread < 1e-14, a tenth of the
tests' RTOL_GEOMETRIC; the file stays under 300 KB.
"""
import os
import sys
import types
import warnings

import numpy as np

warnings.simplefilter("ignore")
np.seterr(all="ignore")
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

pkg = types.ModuleType("xugrid")
pkg.__path__ = [f"{REF}/xugrid"]
sys.modules["xugrid"] = pkg
from xugrid.regrid import reduce  # noqa: E402

METHODS = dict(reduce.ABSOLUTE_OVERLAP_METHODS)
METHODS.update(reduce.RELATIVE_OVERLAP_METHODS)
METHODS["p33.3"] = reduce.create_percentile_method(33.3)
METHODS["p0"] = reduce.create_percentile_method(0)
METHODS["p100"] = reduce.create_percentile_method(100)

NAN, INF = np.nan, np.inf
LONG_LENGTHS = (33, 34, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3073, 4097)
LONG_ROW = 32
GEO_SPREAD_MAX = 1e-14  # a tenth of RTOL_GEOMETRIC (tests/test_gpu_parity.py)
SIZE_MAX = 300 * 1024
SPARSE_ROWS = 512           # two row blocks of the many-variable apply plan (AP_BLOCK = 256), one pair of its merged form
SPARSE_BLOCK_ENTRIES = 512  # PLAN_UMAX: distinct columns per planned block

EXTREME_V = np.array([1e308, -1e308, 5e-324, 1e-45, 1e-300, 0.1, 1.0 / 3.0, 3.0, INF, -INF, 0.0, -0.0, NAN])
EXTREME_POS = np.array([1e308, 5e-324, 1e-45, 1e-300, 0.1, 1.0 / 3.0, 3.0])
EXTREME_W = np.array([0.0, 1e-300, 1e300, 0.1])
DYADIC_V = np.array([INF, -INF, 0.0, -0.0, NAN, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, 4.0])
DYADIC_FINITE = np.array([0.0, -0.0, NAN, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, 4.0])
DYADIC_POS = np.array([0.25, 0.5, 1.0, 2.0, 4.0, 4.0])
DYADIC_W = np.array([0.0, 0.25, 0.5, 1.0, 1.0, 2.0])
DYADIC_WPOS = np.array([0.25, 0.5, 1.0, 1.0, 2.0])


class Rows:
    """rows as (weights, plane A, plane B, plane D); plane C is NaN throughout.  `period`: the row's random fill repeats with
    this period (see draw)"""

    def __init__(self, rng):
        self.rng = rng
        self.rows = []

    def draw(self, alphabet, n, period=None):
        """n draws from the alphabet; with a period, that many draws repeated to length n.  Long rows are drawn this way:
        independent draws from a 15-letter alphabet cannot be stored in less than half a byte per entry and plane, which
        alone would be the file's whole budget, a repeated motif costs next to nothing.  The periods are primes, so every
        lane of a 16-lane group, a wave or a block still meets every letter of the motif."""
        if period is None or period >= n:
            return self.rng.choice(alphabet, n)
        return np.resize(self.rng.choice(alphabet, period), n)

    def plane_d(self, n, pos, period):
        return self.draw(np.concatenate([np.tile(pos, 8 // len(pos) + 1)[:8], [NAN, 0.0]]), n, period)

    def add(self, a, w, extreme=False, b_from=None, period=None):
        a = np.asarray(a, dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        assert a.shape == w.shape and a.ndim == 1
        pos = EXTREME_POS if extreme else DYADIC_POS
        b = a.copy()
        hole = np.isnan(b)
        b[hole] = self.draw(pos if b_from is None else b_from, a.size, period)[hole]
        self.rows.append((w, a, b, self.plane_d(a.size, pos, period)))


def short_rows(rng):
    R = Rows(rng)
    g1 = np.load(f"{OUT}/g1_reducers.npz")
    for i in range(15):  # G1's crafted rows (gen_goldens.py: g1_reducers)
        s, e = g1["offsets"][i], g1["offsets"][i + 1]
        R.add(g1["values"][s:e], g1["weights"][s:e])
    # the extreme alphabet, every length 1 ... 32 three times over
    lengths = np.tile(np.arange(1, 33), 3)
    for i, n in enumerate(lengths):
        v = rng.choice(EXTREME_V, n)
        w = rng.choice(EXTREME_W, n)
        rnd = rng.random(n) < 0.3
        w[rnd] = rng.random(int(rnd.sum()))
        if i % 5 == 1:  # positive values only, with NaN: finite geometric and harmonic means next to overflowing sums
            v = np.where(np.isnan(v) | (v <= 0), rng.choice(EXTREME_POS, n), v)
            v[rng.random(n) < 0.2] = NAN
        if i % 5 == 2:
            w[:] = 0.0
        if i % 5 == 3:  # the only positive weight on a NaN value
            w[:] = 0.0
            j = int(rng.integers(n))
            v[j], w[j] = NAN, 1e300
        R.add(v, w, extreme=True, b_from=EXTREME_V[:-1])
    # dyadic short rows: tied weights and tied values in the thread-per-row kernels
    for i in range(48):
        n = int(rng.integers(1, 33))
        R.add(rng.choice(DYADIC_V if i % 2 else DYADIC_FINITE, n), rng.choice(DYADIC_W, n))
    return R.rows


def run_of_32(rng):
    """64 rows of 32 entries each, kept consecutive: a whole wave of the longest thread-per-row rows"""
    R = Rows(rng)
    for i in range(64):
        if i % 2:
            v, w = rng.choice(EXTREME_V, 32), rng.choice(EXTREME_W, 32)
            R.add(v, w, extreme=True, b_from=EXTREME_V[:-1])
        else:
            R.add(rng.choice(DYADIC_V if i % 4 else DYADIC_FINITE, 32), rng.choice(DYADIC_W, 32))
    return R.rows


def long_rows(rng):
    R = Rows(rng)
    periods = (53, 59, 61, 67, 71, 73)
    for n in LONG_LENGTHS:
        mid = n // 2

        def draw(alphabet, period=None):
            return R.draw(alphabet, n, period or int(rng.choice(periods)))

        def add(v, w):
            R.add(v, w, period=int(rng.choice(periods)))

        # two random rows: the whole alphabet (a long period); the alphabet without inf (finite sums)
        add(draw(DYADIC_V, 251), draw(DYADIC_W, 241))
        add(draw(DYADIC_FINITE), draw(DYADIC_W))
        # one valid value, in the last entry, among NaN
        v = np.full(n, NAN)
        v[-1] = rng.choice(DYADIC_POS)
        w = draw(DYADIC_W)
        w[-1] = rng.choice(DYADIC_WPOS)
        add(v, w)
        # one negative value in the middle of positives
        v = draw(DYADIC_POS)
        v[mid] = -rng.choice(DYADIC_POS)
        w = draw(DYADIC_W)
        w[mid] = rng.choice(DYADIC_WPOS)
        add(v, w)
        # all weights zero
        add(draw(DYADIC_FINITE), np.zeros(n))
        # one positive weight, in the last entry (values non-negative or NaN, the last one positive)
        v = draw(np.concatenate([DYADIC_POS, [0.0, NAN]]))
        v[-1] = rng.choice(DYADIC_POS)
        w = np.zeros(n)
        w[-1] = rng.choice(DYADIC_WPOS)
        add(v, w)
        # the only positive weight on a NaN value, the valid values carry weight zero
        v = draw(np.concatenate([DYADIC_POS, [0.0, -0.0, NAN]]))
        v[mid] = NAN
        v[0] = 1.0
        w = np.zeros(n)
        w[mid] = 2.0
        add(v, w)
        # several real +inf values together with NaN and finite values: +inf must stay apart from the sort's padding -- the
        # positive weights sit on the +inf and NaN entries only, so maximum and p100 are +inf where padding would give NaN
        v = draw(np.concatenate([DYADIC_POS, [NAN, NAN, NAN, INF, INF]]))
        v[[0, mid, n - 1]] = INF, NAN, INF
        w = draw(DYADIC_WPOS)
        w[np.isfinite(v)] = 0.0
        add(v, w)
    return R.rows


def sparse_rows(rng):
    """The first SPARSE_ROWS rows hold 0 ... 3 entries each, at most SPARSE_BLOCK_ENTRIES per 256 of them: with a column per
    entry, only such row blocks fit the many-variable apply plan's distinct-column lists (512 per block of 256 rows, 1024
    per pair of blocks); every block with a long row in it is left to the direct kernel.  Every fourth row has zero
    weights only: NaN by the rule, whatever the values."""
    R = Rows(rng)
    for i in range(SPARSE_ROWS):
        n = int(rng.choice([0, 1, 1, 1, 1, 2, 2, 2, 3, 3]))
        extreme = i % 2 == 1
        v = rng.choice(EXTREME_V if extreme else DYADIC_V, n)
        w = rng.choice(EXTREME_W if extreme else DYADIC_W, n)
        if i % 4 == 0:
            w[:] = 0.0
        R.add(v, w, extreme=extreme, b_from=EXTREME_V[:-1] if extreme else None)
    return R.rows


def assemble(rng):
    rows = short_rows(rng) + long_rows(rng) + [(np.zeros(0),) * 4 for _ in range(24)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    at = int(rng.integers(len(rows) // 3, 2 * len(rows) // 3))
    rows[at:at] = run_of_32(rng)
    rows = sparse_rows(rng) + rows
    lens = np.array([r[0].size for r in rows])
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    data = np.concatenate([r[0] for r in rows])
    planes = np.stack([np.concatenate([r[k] for r in rows]) for k in (1, 2, 1, 3)])
    planes[2] = NAN
    return indptr, data, planes


def by_value(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def call(f, v, w):
    wc = w.copy()
    res = float(f(v.copy(), wc, np.empty(max(v.size, 1))))
    assert np.array_equal(wc, w)
    return res


G = {}  # the assembled inputs, shared with the forked workers of main()


def reference_rows(name):
    """-> (name, {"64": out[P, T], "32": ...}, largest geometric spread) with the conditions on the long rows asserted"""
    f, indptr, data, is_long, perms = METHODS[name], G["indptr"], G["data"], G["is_long"], G["perms"]
    T, n_long = indptr.size - 1, int(is_long.sum())
    results, spread = {}, 0.0
    for tag, planes in (("64", G["planes64"]), ("32", G["planes32"].astype(np.float64))):
        P = planes.shape[0]
        res = np.full((P, T), NAN)
        for p in range(P):
            for t in range(T):
                s, e = indptr[t], indptr[t + 1]
                if e == s:
                    continue  # regridder.py: an empty row keeps the NaN the output was filled with
                v, w = planes[p, s:e], data[s:e]
                res[p, t] = call(f, v, w)
                if not is_long[t]:
                    continue
                others = [call(f, v[::-1], w[::-1]), call(f, v[perms[t]], w[perms[t]])]
                allr = np.array([res[p, t]] + others)
                if name == "geometric_mean" and np.isfinite(allr).all() and (allr > 0).all():
                    spread = max(spread, float((allr.max() - allr.min()) / allr.min()))
                else:  # the same by value in every order (geometric_mean: where it is NaN, inf or 0)
                    assert all(by_value(res[p, t], o) for o in others), (name, tag, p, t, allr)
        fin = np.isfinite(res[:, is_long]).sum(axis=1)
        assert fin[0] * 4 >= n_long and fin[1] * 4 >= n_long and fin[3] * 4 >= n_long, (name, tag, fin, n_long)
        if name == "geometric_mean":
            assert fin[3] * 2 >= n_long, (name, tag, fin, n_long)
        results[tag] = res
    print(name, "finite long rows per plane (float32):", fin.tolist(), "of", n_long, flush=True)
    return name, results, spread


def main():
    import multiprocessing

    rng = np.random.default_rng(1212)
    indptr, data, planes64 = assemble(rng)
    T, nnz = indptr.size - 1, int(indptr[-1])
    lens = np.diff(indptr)
    is_long = lens > LONG_ROW
    planes32 = planes64.astype(np.float32)
    assert not np.isnan(planes64[1]).any() and np.isinf(planes64[1]).any() and np.isnan(planes64[2]).all()
    assert np.isfinite(planes64[3][~np.isnan(planes64[3])]).all() and (planes64[3][~np.isnan(planes64[3])] >= 0).all()
    assert sorted(set(lens[is_long])) == sorted(LONG_LENGTHS) and is_long.sum() == 8 * len(LONG_LENGTHS)
    assert {1, 2, 3, 31, 32} <= set(lens) and (lens == 0).sum() >= 24
    run = np.flatnonzero(lens == 32)
    assert max(len(r) for r in np.split(run, np.flatnonzero(np.diff(run) != 1) + 1)) >= 64
    for b in range(0, SPARSE_ROWS, 256):  # the sparse blocks fit the apply plan, per block and per pair of blocks
        assert 256 < indptr[b + 256] - indptr[b] <= SPARSE_BLOCK_ENTRIES, (b, indptr[b + 256] - indptr[b])
    zero_w = np.array([lens[t] > 0 and not data[indptr[t]:indptr[t + 1]].any() for t in range(SPARSE_ROWS)])
    assert zero_w.sum() >= SPARSE_ROWS // 8
    G.update(indptr=indptr, data=data, planes64=planes64, planes32=planes32, is_long=is_long,
             perms={t: rng.permutation(lens[t]) for t in np.flatnonzero(is_long)})

    # (`indices` is not stored: it is arange(nnz) by construction, and as such -- 190 KB deflated -- would take two thirds of
    # the file's budget for no information)
    out = {"indptr": indptr, "data": data, "planes64": planes64, "planes32": planes32, "is_long": is_long}
    geo_spread = 0.0
    with multiprocessing.get_context("fork").Pool(min(len(METHODS), os.cpu_count() or 1)) as pool:
        for name, results, spread in pool.map(reference_rows, list(METHODS), chunksize=1):
            for tag, res in results.items():
                out[f"out{tag}_{name}"] = res
            geo_spread = max(geo_spread, spread)
    assert 0.0 < geo_spread < GEO_SPREAD_MAX, geo_spread
    out["geo_spread"] = np.float64(geo_spread)
    path = f"{OUT}/g12_reducer_edges.npz"
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < SIZE_MAX, size
    print(f"G12 T {T} nnz {nnz} long rows {int(is_long.sum())} geo_spread {geo_spread:.3g} file {size} bytes")


if __name__ == "__main__":
    main()
