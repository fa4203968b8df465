"""GPU (-m gpu): the partial-state kernels of the source-sharded apply (xr_partial.hip: k_apply_partial*, k_reduce_partial_rows*,
k_partial_identity, k_finalize_partial) called in process through their entry points, against the numpy yardstick of
tests/partial_cases.py: the STATES themselves, every kernel form (K = 1 wave windows, K = 2..7 thread per row, K >= 8 tiles of
eight variables in both layouts, the long-row kernel), the combine / finalize kernels on given tables, the whole route over
column shards and the fused weight build + partial apply.

Bounds.  Min / max components and counts are exact in any order: bit-equal.  Sums of rows of at most 32 entries are added left to
right by one thread: bit-equal (geometric c1 apart: device log).  Longer rows are summed in another order: against the correctly
rounded sum (math.fsum) of the rounded terms, |got - fsum| <= (n + 2) 2^-52 sum |term| -- n - 1 additions in any order
cost at most (n - 1) u sum |term| to first order, the rounding of fsum itself and of each term's own product is covered by the
rest (u = 2^-53, so the bound has a factor two in hand); geometric c1 gets n + 4 (2 ulp for log: HIP documents 1 ulp for the
double-precision log, libm stays within 1)."""
import numpy as np
import pytest

import partial_cases as PC
from conftest import same_or_nan

pytestmark = pytest.mark.gpu

RTOL_GEOMETRIC = 1e-13  # device exp against libm (the project's figure, tests/test_gpu_parity.py)
EPS = 2.0 ** -52
UNWRITTEN = -7.25e300  # what the output buffers hold before a call: every state has to be written
K_MAX = 17
GUARD = 8  # doubles behind every table a kernel writes: a tile of eight variables that ignores K ends there
MATRICES = ("edges", "short_only", "built", "keyed", "ordered", "colkeyed")


def same_bits(a, b):
    """bit for bit, signed zeros included; any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


class Matrix:
    """A matrix on the device with what the yardstick needs: the CSR in the CALLER's numbering, the column order the source
    block has to be handed over in and the row order the states come back in (identities unless the engine's order is on)."""

    def __init__(self, E, name):
        self.name = name
        if name == "built":
            (sxy, sf), (txy, tf) = PC.built_meshes()
            self.meshes = E.DeviceMesh(sxy, sf, -1), E.DeviceMesh(txy, tf, -1)
            self.csr = self.meshes[0].overlap(self.meshes[1])
            self.data, self.indices, self.indptr = self.csr.download()
            self.T, self.S = self.csr.n, self.csr.m
        else:
            self.data, self.indices, self.indptr, self.T, self.S = PC.short_only() if name == "short_only" else PC.edges()
            self.csr = E.DeviceCSR.from_arrays(self.data, self.indices, self.indptr, self.T, self.S)
        self.col_order, self.row_order = np.arange(self.S), np.arange(self.T)
        rng = np.random.default_rng(17)
        if name == "keyed":  # a stored row order on an uploaded matrix; the states still come in the caller's order
            self.csr.set_row_keys(rng.integers(0, 37, self.T), 37)
            stored = self.csr.row_order()
            assert not np.array_equal(stored, np.arange(self.T)) and np.array_equal(np.sort(stored), np.arange(self.T))
        if name == "ordered":  # rows AND columns in the engine's order: permuted source in, stored row order out
            self.col_order, self.row_order = self.csr.engine_order(rng.random((self.S, 2)), rng.random((self.T, 2)))
            assert not np.array_equal(self.col_order, np.arange(self.S)) and not np.array_equal(self.row_order, np.arange(self.T))
        if name == "colkeyed":  # stored rows AND columns permuted, caller's numbering kept on both sides: the call itself puts
            self.csr.set_row_keys(rng.integers(0, 37, self.T), 37)  # the source block into the stored column order
            self.csr.set_col_keys(rng.integers(0, 29, self.S), 29)
            stored_rows, stored_cols = self.csr.row_order(), self.csr.col_order()
            assert not np.array_equal(stored_rows, np.arange(self.T)) and not np.array_equal(stored_cols, np.arange(self.S))
            assert np.array_equal(np.sort(stored_cols), np.arange(self.S))
            for a, b in zip(self.csr.download(), (self.data, self.indices, self.indptr)):
                assert np.array_equal(a, b)  # (the matrix still downloads in the caller's ids)
        self.n = np.diff(self.indptr)
        self.rows = PC.row_ids(self.indptr)
        self.long = np.flatnonzero(self.n > PC.LONG)
        self.short = self.n <= PC.LONG
        self.block = {np.float64: PC.stack(self.S, K_MAX)[0]}
        self.block[np.float32] = self.block[np.float64].astype(np.float32)
        self._ref = {}

    def ref(self, mid, dtype):
        """-> (states (C, K_MAX, T) left to right, fsum {c: (K_MAX, rows)}, its rows, magnitudes (C, K_MAX, T))"""
        if (mid, dtype) not in self._ref:
            C = PC.components(mid)
            st, mag = np.empty((C, K_MAX, self.T)), np.empty((C, K_MAX, self.T))
            which = np.arange(self.T) if mid == PC.GEOMETRIC else self.long
            exact = {c: np.empty((K_MAX, which.size)) for c in PC.summed(mid)}
            for k in range(K_MAX):
                v = self.block[dtype][k].astype(np.float64)[self.indices]
                st[:, k] = PC.states(mid, v, self.data, self.rows, self.T)
                mag[:, k] = PC.magnitudes(mid, v, self.data, self.rows, self.T)
                for c, x in PC.fsum_states(mid, v, self.data, self.indptr, which).items():
                    exact[c][k] = x
            self._ref[mid, dtype] = st, exact, which, mag
        return self._ref[mid, dtype]


@pytest.fixture(scope="module")
def matrices(hip):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Matrix(hip.engine, name)
        return made[name]

    return get


def device_states(E, csr, block, mid, rows_layout, T):
    """partial_dev on a host block (K, S) -> (C, K, T), t in the order the call delivers"""
    K, C = block.shape[0], PC.components(mid)
    d_src = E.DeviceArray.from_host(block)
    d_out = E.DeviceArray.from_host(np.full(C * K * T + GUARD, UNWRITTEN))
    csr.partial_dev(d_src.ptr, E.XR_F32 if block.dtype == np.float32 else E.XR_F64, K, d_out.ptr, mid, rows_layout)
    return unpack_states(d_out.download(), C, K, T, rows_layout)


def unpack_states(out, C, K, T, rows_layout):
    assert (out[C * K * T:] == UNWRITTEN).all(), "written past the end of the state table"
    out = out[: C * K * T]
    out = out.reshape(T, C, K).transpose(1, 2, 0) if rows_layout else out.reshape(C, K, T)
    assert not (out == UNWRITTEN).any(), "states left unwritten"
    return out


def matrix_states(E, M, mid, dtype, ks, rows_layout):
    """the states of the variables `ks` of the matrix' stack, one call, in the CALLER's row order"""
    got = device_states(E, M.csr, M.block[dtype][ks][:, M.col_order], mid, rows_layout, M.T)
    out = np.empty_like(got)
    out[:, :, M.row_order] = got
    return out


# ---- a. the states of every form against the yardstick ------------------------------------------------------------------------
@pytest.mark.parametrize("rows_layout", [False, True], ids=["planes", "rows"])
@pytest.mark.parametrize("name", MATRICES)
def test_states_against_yardstick(hip, matrices, name, rows_layout):
    E, M = hip.engine, matrices(name)
    if name == "built":
        assert M.n.max() > 2048 and M.n[-2:].min() > 2048
    worst = {}
    for method in PC.NAMES:
        mid = PC.IDS[method]
        for dtype in (np.float64, np.float32):
            ref, exact, which, mag = M.ref(mid, dtype)
            for K in (1, 2, 7, 8, 9, 16, 17):
                got = matrix_states(E, M, mid, dtype, np.arange(K), rows_layout)
                tag = (name, method, dtype.__name__, K)
                for c in range(PC.components(mid)):
                    if c not in PC.summed(mid):  # maxima and counts: exact whatever the order
                        assert same_bits(got[c], ref[c, :K]).all(), tag + (c,)
                        continue
                    log_term = mid == PC.GEOMETRIC and c == 1
                    if not log_term:
                        bad = ~same_bits(got[c][:, M.short], ref[c, :K][:, M.short])
                        assert not bad.any(), tag + (c, "short rows", np.argwhere(bad)[:4].tolist())
                    if which.size == 0:
                        continue
                    g, x, m = got[c][:, which], exact[c][:K], mag[c, :K][:, which]
                    bound = (M.n[which] + (4 if log_term else 2)) * EPS * m
                    loose = ~np.isfinite(x) | ~np.isfinite(m)  # an infinity or NaN among the terms: the same in any order
                    assert same_or_nan(g[loose], x[loose]).all(), tag + (c, "non-finite rows")
                    err = np.abs(g[~loose] - x[~loose])
                    assert (err <= bound[~loose]).all(), tag + (c, float((err / np.maximum(bound[~loose], 1e-300)).max()))
                    ratio = err[bound[~loose] > 0] / bound[~loose][bound[~loose] > 0]
                    key = f"{method}.c{c}"
                    worst[key] = max(worst.get(key, 0.0), float(ratio.max()) if ratio.size else 0.0)
    print(f"\n[{name}/{'rows' if rows_layout else 'planes'}] worst |got - fsum| / bound:",
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- b. the forms agree with each other ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "built", "keyed", "colkeyed"])
def test_forms_agree_bitwise(hip, matrices, name):
    """w1 (K = 1, long rows in its own first blocks), thread per row + k_apply_partial_long (K = 7) and the tiles of eight
    (K = 9: one full tile, one of a single variable), planes and rows: the same additions in the same order per variable."""
    E, M = hip.engine, matrices(name)
    assert M.long.size > 0
    for method in PC.NAMES:
        mid = PC.IDS[method]
        for dtype in (np.float64, np.float32):
            base = matrix_states(E, M, mid, dtype, np.arange(9), False)
            for K in (7, 9):
                for rows_layout in (False, True):
                    got = matrix_states(E, M, mid, dtype, np.arange(K), rows_layout)
                    assert same_bits(got, base[:, :K]).all(), (name, method, dtype.__name__, K, rows_layout)
            for k in range(9):
                for rows_layout in (False, True):
                    one = matrix_states(E, M, mid, dtype, np.array([k]), rows_layout)
                    bad = ~same_bits(one[:, 0], base[:, k])
                    assert not bad.any(), (name, method, dtype.__name__, k, rows_layout, np.argwhere(bad)[:4].tolist(),
                                           "long" if bad[:, M.long].any() else "short")


# ---- c. which kernel ran -------------------------------------------------------------------------------------------------------
def test_which_path_ran(hip, matrices):
    E = hip.engine
    for name, has_long in (("edges", True), ("built", True), ("keyed", True), ("short_only", False)):
        M = matrices(name)
        assert (M.long.size > 0) == has_long
        for K in (1, 2, 7, 8, 9):
            for rows_layout in (False, True):
                d_src = E.DeviceArray.from_host(M.block[np.float64][:K])
                d_out = E.DeviceArray((2 * K * M.T + GUARD,))
                with E.KernelTimer() as timer:
                    M.csr.partial_dev(d_src.ptr, E.XR_F64, K, d_out.ptr, PC.MEAN, rows_layout)
                launches = {k: v[0] for k, v in timer.records.items() if v[0]}
                assert launches.get("apply_partial", 0) == 1, (name, K, launches)
                assert launches.get("apply_partial_long", 0) == (1 if has_long and K >= 2 else 0), (name, K, launches)


def test_source_permuted_on_the_device(hip, matrices):
    """A matrix whose stored columns are renumbered (set_col_keys) takes the caller's block as it is: k_permute_source writes
    the stored-order copy the partial kernels read -- one launch per call, whatever K, dtype and layout; the states equal those
    of the plain matrix bit for bit.  With expect_permuted (engine_order) the caller hands the permuted block over: no launch."""
    E = hip.engine
    plain, M, ordered = matrices("edges"), matrices("colkeyed"), matrices("ordered")
    for method in PC.NAMES:
        mid = PC.IDS[method]
        for dtype in (np.float64, np.float32):
            for K in (1, 7, 9):
                base = matrix_states(E, plain, mid, dtype, np.arange(K), False)
                for rows_layout in (False, True):
                    for X, n_permute in ((M, 1), (ordered, 0)):
                        with E.KernelTimer() as timer:
                            got = matrix_states(E, X, mid, dtype, np.arange(K), rows_layout)
                        tag = (X.name, method, dtype.__name__, K, rows_layout)
                        assert timer.records.get("permute_source", (0, 0.0))[0] == n_permute, tag + (timer.records,)
                        assert timer.records.get("apply_partial", (0, 0.0))[0] == 1, tag
                        assert same_bits(got, base).all(), tag


# ---- d. combine and finalize on given state tables ---------------------------------------------------------------------------
def state_table(mid, R, K, rng):
    """(R, C, K) states: random, then the edges of finalize sprinkled over them"""
    C = PC.components(mid)
    tab = np.empty((R, C, K))

    def sprinkle(x, values, share=0.06):
        for v in values:
            x[rng.random(x.shape) < share] = v

    if PC.is_max(mid):
        tab[:, 0], tab[:, 1] = rng.normal(size=(R, K)), rng.uniform(0.1, 1.0, (R, K))
        sprinkle(tab[:, 0], (0.0, -0.0, np.inf, -np.inf))
        sprinkle(tab[:, 1], (0.0,), 0.4)
    elif mid == PC.GEOMETRIC:
        tab[:, 2] = rng.uniform(0.5, 2.0, (R, K))
        tab[:, 0] = tab[:, 2] + rng.uniform(0.0, 1.0, (R, K))
        tab[:, 1] = rng.normal(size=(R, K))
        tab[:, 3] = 0.0
        sprinkle(tab[:, 2], (0.0,), 0.3)
        sprinkle(tab[:, 0], (0.0,), 0.3)
        sprinkle(tab[:, 1], (0.0, -0.0, np.inf, -np.inf), 0.03)
        sprinkle(tab[:, 3], (1.0, 3.0), 0.05)
    else:
        tab[:, 0], tab[:, 1] = rng.normal(size=(R, K)), rng.uniform(0.1, 1.0, (R, K))
        sprinkle(tab[:, 0], (0.0, -0.0), 0.15)
        sprinkle(tab[:, 0], (np.inf, -np.inf), 0.03)
        sprinkle(tab[:, 1], (0.0,), 0.4)
    return tab


def assert_final(mid, got, exp, tag):
    assert np.array_equal(np.isnan(got), np.isnan(exp)), tag
    if mid == PC.GEOMETRIC:
        np.testing.assert_allclose(got, exp, rtol=RTOL_GEOMETRIC, atol=0, equal_nan=True, err_msg=str(tag))
    else:
        bad = ~same_bits(got, exp)
        assert not bad.any(), tag + (np.argwhere(bad)[:4].tolist(),)


def reduce_rows(E, mid, table, indptr, order, K, offset=0):
    """reduce_partial_rows_dev on a host table (R, C, K); `offset` doubles in front of the table -> (K, n_targets)"""
    n_targets = indptr.size - 1
    d_rows = E.DeviceArray.from_host(np.concatenate([np.zeros(offset), table.ravel()]))
    d_indptr, d_order = E.DeviceArray.from_host(indptr), E.DeviceArray.from_host(order)
    d_out = E.DeviceArray.from_host(np.full(K * n_targets + GUARD, UNWRITTEN))
    E.reduce_partial_rows_dev(mid, d_rows.ptr + 8 * offset, d_indptr.ptr, d_order.ptr, n_targets, K, d_out.ptr)
    out = d_out.download()
    assert (out[K * n_targets:] == UNWRITTEN).all(), "written past the end of the output"
    out = out[: K * n_targets].reshape(K, n_targets)
    assert not (out == UNWRITTEN).any(), "outputs left unwritten"
    return out


@pytest.mark.parametrize("K", [1, 2, 7, 8, 31, 32, 33, 65, 2080])
def test_reduce_partial_rows_on_given_tables(hip, K):
    """K = 1 aligned: the specialised kernel; K = 1 eight bytes off and K = 2 .. 7: the generic one; K >= 8: 64 targets x 32
    variables per block, gridDim.y capped at 64 (K = 2080: 65 chunks, block row 0 takes a second turn)."""
    E = hip.engine
    rng = np.random.default_rng(K)
    for method in PC.NAMES:
        mid = PC.IDS[method]
        for n_targets in (1, 63, 64, 65, 130):
            for shift in range(4 if n_targets == 1 else 1):
                lens = np.array([(0, 1, 2, 8)[(t + shift) % 4] for t in range(n_targets)])
                indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                R = int(lens.sum()) + 3
                order = rng.permutation(R)[: lens.sum()].astype(np.int64)  # shuffled: no sender list is a stretch of rows
                table = state_table(mid, R, K, rng)
                exp = np.full((K, n_targets), np.nan)
                for t in range(n_targets):
                    senders = order[indptr[t]:indptr[t + 1]]
                    if senders.size:
                        exp[:, t] = PC.finalize(mid, PC.combine(mid, [table[r] for r in senders]))
                tag = (method, K, n_targets, shift)
                got = reduce_rows(E, mid, table, indptr, order, K)
                assert np.isnan(got[:, lens == 0]).all(), tag  # a target nobody sent a row for
                assert_final(mid, got, exp, tag)
                if K == 1:  # the table 8 bytes off a 16-byte boundary: no 16-byte loads, the generic kernel
                    off = reduce_rows(E, mid, table, indptr, order, K, offset=1)
                    assert same_bits(off, got).all(), tag
                    assert_final(mid, off, exp, tag + ("offset",))


def test_reduce_partial_rows_which_kernel(hip):
    """One launch per call: the specialised kernel only for K = 1 on a 16-byte aligned table (its loads are 16 bytes wide), the
    tiles from K = 8 on, the generic kernel for the rest."""
    E = hip.engine
    assert E.DeviceArray((64,)).ptr % 16 == 0
    rng = np.random.default_rng(1)
    indptr, order = np.array([0, 2, 5], dtype=np.int64), np.array([4, 0, 1, 3, 2], dtype=np.int64)
    cases = ((1, 0, "reduce_partial_rows_k1"), (1, 1, "reduce_partial_rows"), (1, 2, "reduce_partial_rows_k1"),
             (2, 0, "reduce_partial_rows"), (7, 0, "reduce_partial_rows"), (8, 0, "reduce_partial_rows_t"),
             (2080, 0, "reduce_partial_rows_t"))
    for method in ("mean", "geometric_mean", "minimum"):
        for K, offset, label in cases:
            table = state_table(PC.IDS[method], 5, K, rng)
            with E.KernelTimer() as timer:
                reduce_rows(E, PC.IDS[method], table, indptr, order, K, offset)
            launches = {k: v[0] for k, v in timer.records.items() if k.startswith("reduce_partial_rows") and v[0]}
            assert launches == {label: 1}, (method, K, offset, launches)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_planes_identity_and_finalize(hip, n):
    """K * T = n elements per component (one block of 256 threads and its neighbours)"""
    E = hip.engine
    rng = np.random.default_rng(n)
    shapes = [(1, n)] + ([(3, 85)] if n == 255 else []) + ([(257, 1)] if n == 257 else [])
    for method in PC.NAMES:
        mid = PC.IDS[method]
        C = PC.components(mid)
        for K, T in shapes:
            d_planes = E.DeviceArray.from_host(np.full(C * n + 1, UNWRITTEN))
            E.partial_fill_identity_dev(mid, d_planes.ptr, K, T)
            ident = d_planes.download()
            assert ident[-1] == UNWRITTEN, "identity fill wrote past its planes"
            ident = ident[:-1].reshape(C, n)
            assert same_bits(ident, PC.identity(mid, (n,))).all(), method
            d_out = E.DeviceArray.from_host(np.full(n + 1, UNWRITTEN))
            E.finalize_partial_dev(mid, d_planes.ptr, K, T, d_out.ptr)
            out = d_out.download()
            assert out[-1] == UNWRITTEN and np.isnan(out[:-1]).all(), method
            planes = state_table(mid, n, 1, rng)[:, :, 0].T.copy()  # (C, n)
            d_planes = E.DeviceArray.from_host(planes)
            E.finalize_partial_dev(mid, d_planes.ptr, K, T, d_out.ptr)
            out = d_out.download()
            assert out[-1] == UNWRITTEN
            assert_final(mid, out[:-1], PC.finalize(mid, planes), (method, K, T))


# ---- e. end to end over column shards -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_matrix(oracle, matrices):
    made = {}

    def get(name):
        if name not in made:
            M = matrices(name)
            made[name] = {m: oracle.regrid_csr(m, M.block[np.float64][:8], M.data, M.indices, M.indptr, M.T) for m in PC.NAMES}
        return made[name]

    return get


@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["edges", "built"])
def test_column_shards_end_to_end(hip, matrices, whole_matrix, name, P):
    E, M = hip.engine, matrices(name)
    T = M.T
    shards = []
    for cols in PC.column_shards(M.S, P):
        d, i, p = PC.shard_csr(M.data, M.indices, M.indptr, cols, M.S)
        shards.append((E.DeviceCSR.from_arrays(d, i, p, T, cols.size), cols))
    assert sum(s.nnz for s, _ in shards) == M.data.size and (min(s.nnz for s, _ in shards) == 0) == (P > 1)
    # sender lists of the sparse route: target t combines row t of every shard's table, in shard order
    indptr = np.arange(T + 1, dtype=np.int64) * P
    order = (np.arange(P, dtype=np.int64)[None, :] * T + np.arange(T, dtype=np.int64)[:, None]).ravel()
    for ks in (np.arange(8), np.array([1])):  # all seven sources and one more; `positive` alone
        K = ks.size
        block = M.block[np.float64][ks]
        for method in PC.NAMES:
            mid = PC.IDS[method]
            C = PC.components(mid)
            planes = [device_states(E, csr, block[:, cols], mid, False, T) for csr, cols in shards]
            tables = [device_states(E, csr, block[:, cols], mid, True, T) for csr, cols in shards]
            for a, b in zip(planes, tables):
                assert same_bits(a, b).all(), (method, "layouts")
            # dense route: identity buffer, element-wise combine (here on the host), finalize
            d_planes = E.DeviceArray((C, K, T))
            E.partial_fill_identity_dev(mid, d_planes.ptr, K, T)
            acc = d_planes.download()
            with np.errstate(all="ignore"):
                for s in planes:
                    acc = PC.max2(acc, s) if PC.is_max(mid) else acc + s
            d_planes, d_out = E.DeviceArray.from_host(acc), E.DeviceArray((K, T))
            E.finalize_partial_dev(mid, d_planes.ptr, K, T, d_out.ptr)
            dense = d_out.download()
            assert_final(mid, dense, PC.finalize(mid, acc), (name, P, K, method, "dense"))
            # sparse route: the concatenated tables through reduce_partial_rows_dev
            table = np.concatenate([s.transpose(2, 0, 1) for s in planes])  # (P * T, C, K)
            sparse = reduce_rows(E, mid, table, indptr, order, K)
            assert_final(mid, sparse, PC.finalize(mid, PC.combine(mid, planes)), (name, P, K, method, "sparse"))
            assert same_or_nan(dense, sparse).all() if mid != PC.GEOMETRIC else True
            exp = whole_matrix(name)[method][ks]
            for got in (dense, sparse):
                assert np.array_equal(np.isnan(got), np.isnan(exp)), (name, P, K, method)
                if PC.is_max(mid):  # (as numbers: the sign of a zero result depends on entry order in the reference)
                    assert np.array_equal(got, exp, equal_nan=True), (name, P, K, method)
                k = int(np.flatnonzero(ks == 1)[0])  # `positive`
                np.testing.assert_allclose(got[k], exp[k], rtol=1e-9 if method == "harmonic_mean" else 1e-12, atol=0,
                                           equal_nan=True, err_msg=str((name, P, K, method)))


# ---- f. weight build + partial state in one call ------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [None, 1], ids=["default", "queue_margin=1"])
def test_overlap_partial_matches_two_calls(hip, matrices, xr_option, margin):
    """K = 1 is enqueued behind the build before the host knows the sizes (gated: with a queue margin of 1 the first attempt
    fails and the host redoes both -- two `apply_partial` launches per call instead of one, which is asserted so that the margin
    cannot stop forcing the retry unnoticed); K = 3 runs once, behind the finished build.  States and matrix equal the two-call
    route.  What this does NOT show: that the gate kept the first, failed attempt's kernel from writing -- the second attempt
    overwrites every state, so a dropped gate leaves the same final table."""
    E, M = hip.engine, matrices("built")
    source_mesh, target_mesh = M.meshes
    two_calls = {}
    for method in PC.NAMES:
        for dtype in (np.float64, np.float32):
            for rows_layout in (False, True):
                for K in (1, 3):
                    two_calls[method, dtype, rows_layout, K] = device_states(E, M.csr, M.block[dtype][:K], PC.IDS[method],
                                                                             rows_layout, M.T)
    if margin is not None:
        xr_option("queue_margin", margin)
    for (method, dtype, rows_layout, K), exp in two_calls.items():
        mid = PC.IDS[method]
        C = PC.components(mid)
        d_src = E.DeviceArray.from_host(M.block[dtype][:K])
        d_out = E.DeviceArray.from_host(np.full(C * K * M.T + GUARD, UNWRITTEN))
        with E.KernelTimer() as timer:
            csr = source_mesh.overlap_partial_dev(target_mesh, d_src.ptr, E.XR_F32 if dtype == np.float32 else E.XR_F64, K,
                                                  d_out.ptr, mid, rows_layout)
        attempts = 2 if (margin is not None and K == 1) else 1
        assert timer.records.get("apply_partial", (0, 0.0))[0] == attempts, (method, K, margin, timer.records)
        got = unpack_states(d_out.download(), C, K, M.T, rows_layout)
        assert same_bits(got, exp).all(), (method, dtype.__name__, rows_layout, K)
        if dtype == np.float64 and not rows_layout:
            for a, b in zip(csr.download(), (M.data, M.indices, M.indptr)):
                assert np.array_equal(a, b), (method, K)
