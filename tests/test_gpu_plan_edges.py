"""
GPU (-m gpu): the apply plan's builder (k_plan_build, xr_apply_plan.hip) at and one past each of its limits, in both plan
forms.  A row block is planned iff it has at most 2048 entries and 512 distinct columns; a group of PLAN_GROUP = 2 row blocks
iff each block has at most 2048 entries and the group at most 1024 distinct columns.  The Delaunay matrices of the other
apply tests cannot tell whether a block sat at a limit or past it; these two are made for it (uploaded, no mesh):

  T = 4 * 256 + 3 rows -- five row blocks, three groups, the last a single ragged block with an empty row --, S = 4096 columns,
  at most 32 entries per row (no long-row kernel takes part: every path reduces a row in the reference's order).
  A, at the limits      block 0: 512 distinct columns (2 per row); block 1: 512 others (the group: exactly 1024); blocks 2 and 3:
                        exactly 2048 entries each (8 per row) from one set of 512 columns.  Everything is planned in both forms.
  B, one past each      block 0: 513 distinct columns (one row takes a third entry) -- unplanned per block, and with block 1 the
                        group has 1025: unplanned when merged; block 2: 2049 entries -- unplanned per block, its group unplanned
                        when merged.

Every result is compared bit for bit (same_or_nan) with oracle.regrid_csr on the same arrays, whichever kernel took a block:
k_apply_plan (its NaN-free short path and its general path: one variable is all NaN, one has scattered NaNs) or k_apply_direct
over the list of unplanned blocks.  K = 8 is one full tile, K = 9 a ragged one, K = 65 more than the 64 variables of one work
item (the L2-blocked order of k_apply_plan).
"""
import numpy as np
import pytest

from conftest import same_or_nan

pytestmark = pytest.mark.gpu

BLOCK, T, S = 256, 4 * 256 + 3, 4096
REDUCERS = ("mean", "sum", "maximum", "first_order_conservative")
KS = (8, 9, 65)


def build_matrix(past):
    """-> data, indices, indptr of matrix A (past = False) or B (past = True)"""
    rng = np.random.default_rng(2048 + 512)
    pool = rng.permutation(S)
    p0, p1, p2, rest = pool[:513], pool[513:1025], pool[1025:1537], pool[1537:]
    rows = []
    for r in range(BLOCK):  # block 0: two columns per row, 512 in all
        rows.append(list(p0[2 * r:2 * r + 2]))
    for r in range(BLOCK):  # block 1: 512 others
        rows.append(list(p1[2 * r:2 * r + 2]))
    for r in range(2 * BLOCK):  # blocks 2 and 3: 8 per row, distinct within the row, from one set of 512
        rows.append(list(rng.choice(p2, 8, replace=False)))
    rows += [list(rest[:32]), [], list(rest[32:35])]  # the ragged block: a row at the long-row limit, an empty one, a short one
    if past:
        rows[100].append(p0[512])  # the 513th distinct column of block 0
        rows[2 * BLOCK + 7].append(next(c for c in p2 if c not in rows[2 * BLOCK + 7]))  # entry 2049 of block 2
    rows = [sorted(int(c) for c in row) for row in rows]
    assert len(rows) == T and max(len(row) for row in rows) == 32
    indptr = np.concatenate([[0], np.cumsum([len(row) for row in rows])]).astype(np.int64)
    indices = np.array([c for row in rows for c in row], dtype=np.int64)
    data = rng.uniform(0.125, 1.0, indices.size)
    data[indptr[300]:indptr[301]] = 0.0  # a row of zero weights
    # what the matrix is made for
    distinct = [np.unique(indices[indptr[b * BLOCK]:indptr[min((b + 1) * BLOCK, T)]]).size for b in range(5)]
    entries = [int(indptr[min((b + 1) * BLOCK, T)] - indptr[b * BLOCK]) for b in range(5)]
    pair01 = np.unique(indices[indptr[0]:indptr[2 * BLOCK]]).size
    assert distinct[:2] == [513 if past else 512, 512] and pair01 == (1025 if past else 1024), (distinct, pair01)
    assert entries[2:4] == [2049 if past else 2048, 2048] and distinct[2] <= 512 and distinct[3] <= 512, (entries, distinct)
    return data, indices, indptr


def sources(K, dtype):
    rng = np.random.default_rng(K)
    src = rng.normal(size=(K, S))
    src[1] = np.nan                           # one variable all NaN
    src[2, rng.random(S) < 0.1] = np.nan      # one with scattered NaNs
    return src.astype(dtype)


@pytest.fixture(scope="module")
def cases(oracle):
    """the two matrices, the source stacks and the oracle's results, computed once"""
    mats = {"A": build_matrix(False), "B": build_matrix(True)}
    stacks = {(K, "f64"): sources(K, np.float64) for K in KS}
    stacks[(9, "f32")] = sources(9, np.float32)
    expected = {}
    for m, (data, indices, indptr) in mats.items():
        for key, src in stacks.items():
            for name in REDUCERS:
                expected[(m, name) + key] = oracle.regrid_csr(name, src.astype(np.float64), data, indices, indptr, T)
    return mats, stacks, expected


@pytest.mark.parametrize("plan_merge", [0, 1, -1])  # per block, merged, the default (per block here: 5 blocks < 4 * PLAN_GROUP)
@pytest.mark.parametrize("matrix", ["A", "B"])
def test_plan_limits(hip, xr_option, cases, matrix, plan_merge):
    from xugrid_amd import engine

    mats, stacks, expected = cases
    data, indices, indptr = mats[matrix]
    xr_option("plan_merge", plan_merge)
    csr = engine.DeviceCSR.from_arrays(data, indices, indptr, T, S)  # (fresh: the plan is built once per matrix, under this option)
    with engine.KernelTimer() as timer:
        first = csr.apply(stacks[(8, "f64")], engine.METHOD_IDS["mean"], 0.0)
    launched = {name for name, (launches, _) in timer.records.items() if launches > 0}
    assert {"plan_build", "apply_plan"} <= launched, launched
    assert ("apply_direct" in launched) == (matrix == "B"), launched  # B's unplanned blocks; A has none
    assert not launched & {"apply_wave", "apply_long"}, launched
    same = same_or_nan(first, expected[(matrix, "mean", 8, "f64")])
    assert same.all(), ("first apply", np.argwhere(~same)[:8].tolist())
    for name in REDUCERS:
        for key, src in stacks.items():
            got = csr.apply(src, engine.METHOD_IDS[name], 0.0)
            exp = expected[(matrix, name) + key]
            assert got.dtype == np.float64 and got.shape == exp.shape == (key[0], T)
            same = same_or_nan(got, exp)
            assert same.all(), (name, key, np.argwhere(~same)[:8].tolist(), got[~same][:4].tolist(), exp[~same][:4].tolist())
