"""
GPU (-m gpu): every device apply path on the reference's own answers at the reducers' corners -- golden set G12
(tests/golden/gen_reducer_edges.py; pinned on the CPU side by test_reducer_edges_cpu.py).  The rows hold the mode and
max_overlap ties, zero-weight rows, the only positive weight on a NaN value, +-inf (k_apply_sorted pads with +inf), +-0.0,
float64 and float32 denormals and overflowing sums; their lengths sit one below, at and one above every threshold between two
kernel families (32 | 33, 64 | 65, 512 | 513, 2048 | 2049, 4 x 256 per block pass).  The long rows use a dyadic alphabet on
which every partial sum is exact, so the cooperative kernels' summation order needs NO tolerance: every comparison is by
value on every row, against the GOLDEN (not the oracle); geometric_mean (device exp / log) is held to RTOL_GEOMETRIC.

The first 512 rows of G12 are sparse enough for the many-variable apply plan (k_apply_plan), the others reach the direct
kernel through the plan's list of unplanned blocks; the K = 17 stack starts with a NaN-free tile (plane B keeps +-inf and
+-0.0), so the plan's NaN-free short path and its general path both see the zero-weight rows.

Signed zeros compare equal throughout (same_or_nan compares by value): which of +0.0 and -0.0 the reference's `min` / `max`
return is a property of the interpreter that ran it, not of the method, and the goldens are made without numba.
"""
import numpy as np
import pytest

from conftest import same_or_nan
from test_gpu_parity import METHODS, RTOL_GEOMETRIC
from test_gpu_structured import ALL_METHODS

pytestmark = pytest.mark.gpu

A, B, C, D = range(4)
STACK_17 = [B] * 8 + [A, B, C, D, A, B, C, D] + [A]  # a NaN-free tile, a mixed tile, a partial tile (tiles of 8; of 4 when merged)
# (stack, options set before the matrix is uploaded: they are read when its plan is built)
STACKS = {
    "K1": ([A], [B], [C], [D]),                       # k_apply_rows1 with its long-row blocks
    "K2": ([A, D],),                                  # k_apply_direct<16>, k_apply_wave<8>, k_apply_long
    "K7": ([A, B, C, D, B, A, D],),
    "K8": ([B, A, D, C, A, B, D, A],),                # one whole tile of the plan
    "K9": ([B] * 8 + [A],),                           # ... and a tile of one variable behind a NaN-free one
    "K17": (STACK_17,),
    "K17_merged": (STACK_17,),                        # one distinct-column list per pair of row blocks
    "K17_per_block": (STACK_17,),
    "K17_direct": (STACK_17,),                        # no plan: the direct kernel across its KT = 16 edge
}
OPTIONS = {"K17_merged": {"plan_merge": 1}, "K17_per_block": {"plan_merge": 0}, "K17_direct": {"apply_plan": 0}}


@pytest.fixture(scope="module")
def g12(golden):
    g = golden("g12_reducer_edges.npz")
    return {k: g[k] for k in g.files}


def upload(hip, g12):
    indptr, data = g12["indptr"], g12["data"]
    return hip.engine.DeviceCSR.from_arrays(data, np.arange(data.size, dtype=np.int64), indptr, indptr.size - 1, data.size)


def assert_rows_equal(got, exp, name, what):
    """the NaN pattern, then every row by value; geometric_mean within RTOL_GEOMETRIC.  No atol, no row left out."""
    assert got.dtype == np.float64 and got.shape == exp.shape, what
    nan_differs = np.isnan(got) != np.isnan(exp)
    assert not nan_differs.any(), (what, "NaN pattern", np.argwhere(nan_differs)[:8].tolist())
    if name == "geometric_mean":
        np.testing.assert_allclose(got, exp, rtol=RTOL_GEOMETRIC, atol=0, equal_nan=True, err_msg=str(what))
    else:
        bad = ~same_or_nan(got, exp)
        assert not bad.any(), (what, np.argwhere(bad)[:8].tolist(), got[bad][:8].tolist(), exp[bad][:8].tolist())


@pytest.mark.parametrize("stack", list(STACKS))
@pytest.mark.parametrize("tag", ["64", "32"])
@pytest.mark.parametrize("name,mid,p", METHODS)
def test_apply_csr_reducer_edges(hip, g12, xr_option, name, mid, p, tag, stack):
    for option, value in OPTIONS.get(stack, {}).items():
        xr_option(option, value)
    csr = upload(hip, g12)  # (a fresh matrix: its plan is built on its first many-variable apply, under these options)
    planes, exp = g12["planes" + tag], g12[f"out{tag}_{name}"]
    for ids in STACKS[stack]:
        got = csr.apply(np.ascontiguousarray(planes[ids]), mid, p)
        assert_rows_equal(got, exp[ids], name, (name, tag, stack, ids))


@pytest.mark.parametrize("tag", ["64", "32"])
@pytest.mark.parametrize("name,mid,p", METHODS)
def test_apply_csr_stack_equals_planes_one_by_one(hip, g12, name, mid, p, tag):
    """a stack applied at once == its planes applied one by one, whatever tile of whatever kernel a plane falls into"""
    csr = upload(hip, g12)
    planes = g12["planes" + tag]
    single = np.concatenate([csr.apply(planes[k:k + 1], mid, p) for k in range(4)])
    for stack in ("K2", "K7", "K8", "K9", "K17"):
        for ids in STACKS[stack]:
            got = csr.apply(np.ascontiguousarray(planes[ids]), mid, p)
            assert_rows_equal(got, single[ids], name, (name, tag, stack, "against K = 1"))


@pytest.fixture(scope="module")
def outer_case():
    """per-axis lists of 0 ... 12 entries for 40 x 30 target cells over 24 x 20 source cells, dyadic weights with zeros; a
    (4, S) field over the dyadic alphabets of planes A - D"""
    rng = np.random.default_rng(1213)
    weights = np.array([0.0, 0.25, 0.5, 1.0, 1.0, 2.0])

    def axis(n_target, n_source):
        counts = rng.integers(0, 13, n_target)
        counts[:3] = 12, 0, 1
        indptr = np.concatenate([[0], np.cumsum(counts)])
        source = np.concatenate([np.sort(rng.choice(n_source, c, replace=False)) for c in counts]).astype(np.int64)
        w = rng.choice(weights, source.size)
        w[indptr[3]:indptr[4]] = 0.0  # a list of zero weights only: every cell of that target row / column is NaN
        return indptr, source, w

    ny, nx = 24, 20
    ay, ax = axis(40, ny), axis(30, nx)
    a = rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, 4.0]), ny * nx)
    b = np.where(np.isnan(a), rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0]), a.size), a)
    d = rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0, 4.0, 1.0, 0.5, np.nan, 0.0]), a.size)
    return ay, ny, ax, nx, np.stack([a, b, np.full(a.size, np.nan), d])


@pytest.mark.parametrize("path", ["free", "csr"])
@pytest.mark.parametrize("name,mid", ALL_METHODS)
def test_apply_outer_reducer_edges(hip, oracle, xr_option, outer_case, name, mid, path):
    """The matrix-free apply of separable weights (xr_outer.hip) and the stored product, on special values, ties and zero
    weights: the oracle (pinned at these corners by test_reducer_edges_cpu.py) on the downloaded product, by value."""
    xr_option("outer_apply", path)
    ay, ny, ax, nx, field = outer_case
    outer = hip.engine.DeviceOuter(ay, ny, ax, nx)
    data, indices, indptr = outer.download()
    assert outer.n == 40 * 30 and np.diff(indptr).max() == 144 and (np.diff(indptr) == 0).any() and (data == 0).any()
    p = 30.0 if name == "p30" else 0.0
    method = ("percentile", p) if name == "p30" else name
    for dtype in (np.float64, np.float32):
        src = field.astype(dtype)
        exp = oracle.regrid_csr(method, src.astype(np.float64), data, indices.astype(np.int64), indptr.astype(np.int64), outer.n)
        assert np.isfinite(exp[D]).sum() > outer.n // 4  # (not NaN = NaN alone)
        assert_rows_equal(outer.apply(src, mid, p), exp, name, (name, path, dtype.__name__))
