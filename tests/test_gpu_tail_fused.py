"""
GPU (-m gpu): the tail of the fused weight build with a K = 1 apply enqueued behind it (overlap_apply_dev).

tail_fused = 1  the apply's launch leads with the blocks that copy the big faces' rows behind the regular ones and reads those
                rows from the big faces' own CSR (k_apply_tail1); no place_big launch
tail_fused = 0  place_big -> publish -> apply_rows1, three launches

Source: a 64 x 64 lattice split into 8192 triangles.  Targets: 162 (or 512) tiny triangles that are regular faces for certain
(a cell of theirs is smaller than a source cell) plus hand-placed triangles that are big faces for certain (a row of more
than 16 entries has more than SLOTS = 16 candidates), sized on the CPU oracle so that their rows have exactly the lengths at
which the apply changes its path: 32 | 33 (one lane | 16 lanes), 512 | 513 (16 lanes | a wave), 2048 | 2049 (a wave | the
block).  The lengths are asserted, so a source mesh that came out differently fails here and not silently.

Every case runs through overlap_apply_dev with the option at 1 and at 0; regridded values, indptr, indices, data and
row_order are compared bit for bit between the two, the list of long rows as a set, and the values against the CPU oracle's
reference loop on the downloaded matrix with the bar of test_gpu_parity.py (rows of at most 32 entries bit for bit, longer rows
RTOL_LONG; geometric_mean -- device exp / log against libm -- RTOL_GEOMETRIC on every row, as there).
"""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import RTOL_GEOMETRIC, assert_apply_equal
from xugrid_amd import meshgen

pytestmark = pytest.mark.gpu

METHODS = [("mean", 0), ("maximum", 5), ("geometric_mean", 2)]
SENTINEL = -12345.678
SLACK = 64  # doubles behind the T results, which no apply may touch
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def source_mesh():
    def make():
        sxy, sf = meshgen.triangle_mesh(65 * 65, 0, delaunay=False)
        assert sf.shape[0] == 8192
        return sxy, sf

    return cached("source", make)


def source_values(dtype):
    """positive (geometric_mean), 1 % NaN; the float32 block is what the device reads, its float64 image what the oracle reads"""

    def make():
        rng = np.random.default_rng(11)
        v = np.exp(rng.normal(0.0, 0.3, size=(1, 8192)))
        v[0, rng.choice(8192, 80, replace=False)] = np.nan
        return np.ascontiguousarray(v.astype(dtype))

    return cached(("values", np.dtype(dtype).name), make)


def skew(x0, y0, a, b, L):
    """the triangle family the lengths were tuned on: (x0, y0), (x0 + L, y0 + a L), (x0 + b L, y0 + L), counter-clockwise"""
    return [(x0, y0), (x0 + L, y0 + a * L), (x0 + b * L, y0 + L)]


# (leg, entries of the row) -- counted with the CPU oracle on source_mesh()
ROW_32 = skew(0.025, 0.036, 0.1, 0.12, 0.0608101)
ROW_33 = skew(0.025, 0.036, 0.1, 0.12, 0.0608105)
ROW_512 = skew(0.045, 0.051, 0.2, 0.28, 0.338795)
ROW_513 = skew(0.045, 0.051, 0.2, 0.28, 0.3387954)
ROW_2048 = skew(0.059, 0.051, 0.25, 0.24, 0.7024836)
ROW_2049 = skew(0.059, 0.051, 0.25, 0.24, 0.702484)
ROW_SMALL = [skew(0.31, 0.62, 0.1, 0.12, 0.045), skew(0.71, 0.22, 0.19, 0.12, 0.05), skew(0.52, 0.13, 0.2, 0.05, 0.055)]
WHOLE = [(-1.0, -1.0), (3.5, -1.0), (-1.0, 3.5)]  # covers the source: 8192 entries, more candidates than BIG_STAGE = 5120
SLIVER = [(0.012, 0.021), (0.991, 0.968), (0.984, 0.977)]  # long, thin, diagonal: a box over most of the source

CASES = {
    # name: (points per side of the regular part, extra triangles, row lengths that must occur)
    "no_big": (10, [], []),
    "big_rows_up_to_32": (10, ROW_SMALL + [ROW_32], [32]),
    "rows_33_and_512": (10, [ROW_32, ROW_33, ROW_512], [32, 33, 512]),
    "rows_513_and_2048": (10, [ROW_513, ROW_2048], [513, 2048]),
    "rows_2049_and_whole_source": (10, [ROW_2049, WHOLE], [2049, 8192]),
    "sliver": (10, [SLIVER], []),
    "every_class_behind_512_regular_rows": (17, ROW_SMALL + [ROW_32, ROW_33, ROW_512, ROW_513, ROW_2048, ROW_2049, WHOLE, SLIVER],
                                            [32, 33, 512, 513, 2048, 2049, 8192]),
}


def target_mesh(name):
    """-> (node_xy, faces): 2 (side - 1)^2 tiny triangles around the source's centre, then the extra triangles.  162 regular rows
    (side 10; the sliver may or may not be one more): the last block of 64 stored regular rows is partial, as is the block of 256;
    512 (side 17): both are full."""

    def make():
        side, extra, _ = CASES[name]
        xy, faces = meshgen.triangle_mesh(side * side, 5, 30.0, 0.06 * (side - 1) / 9, delaunay=False)
        assert faces.shape[0] == 2 * (side - 1) ** 2
        for tri in extra:
            n = xy.shape[0]
            xy = np.vstack([xy, np.asarray(tri, dtype=np.float64)])
            faces = np.vstack([faces, [[n, n + 1, n + 2]]])
        return np.ascontiguousarray(xy), np.ascontiguousarray(faces)

    return cached(("target", name), make)


class DeviceBlocks:
    """a (1, S) source block on the device and T + SLACK doubles for the result, through the C ABI's raw allocations"""

    def __init__(self, v, T):
        from xugrid_amd import _lib

        self._lib, self.lib = _lib, _lib.load()
        self.v, self.T = np.ascontiguousarray(v), T

    def __enter__(self):
        src, out = ctypes.c_void_p(), ctypes.c_void_p()
        self._lib.check(self.lib.xr_dev_alloc(self.v.nbytes, ctypes.byref(src)))
        self._lib.check(self.lib.xr_dev_alloc(8 * (self.T + SLACK), ctypes.byref(out)))
        self._lib.check(self.lib.xr_dev_upload(src, self.v.ctypes.data_as(ctypes.c_void_p), self.v.nbytes))
        self._src, self._out = src, out
        self.src, self.out = src.value, out.value
        return self

    def fill(self, value):
        host = np.full(self.T + SLACK, value)
        self._lib.check(self.lib.xr_dev_upload(self._out, host.ctypes.data_as(ctypes.c_void_p), host.nbytes))

    def fetch(self):
        """-> (1, T) results; the words behind them must still hold what fill() put there"""
        out = np.empty(self.T + SLACK)
        self._lib.check(self.lib.xr_dev_download(out.ctypes.data_as(ctypes.c_void_p), self._out, out.nbytes))
        assert (out[self.T:] == SENTINEL).all(), "an apply wrote behind its T results"
        return out[None, : self.T].copy()

    def __exit__(self, *exc):
        self.lib.xr_dev_free(self._src)
        self.lib.xr_dev_free(self._out)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def dtype_id(E, v):
    return E.XR_F32 if v.dtype == np.float32 else E.XR_F64


def launches_of(timer):
    return {k: v[0] for k, v in timer.records.items() if v[0]}


def step(hip, dev, sxy, sf, txy, tf, method_id):
    """one overlap_apply_dev on fresh handles, the output pre-filled -> (matrix parts, long rows, regridded, launches)"""
    E = hip.engine
    ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
    dev.fill(SENTINEL)
    with E.KernelTimer() as timer:
        csr = ms.overlap_apply_dev(mt, dev.src, dtype_id(E, dev.v), 1, dev.out, method_id)
        E.dev_sync()
    out = dev.fetch()
    listed = csr.long_rows()  # the builder's list; row_order() settles a pending regrouping of the rows, which lists them anew
    data, indices, indptr = csr.download()
    row_order = csr.row_order()
    return (indptr, indices, data, row_order), (listed, csr.long_rows()), out, launches_of(timer)


def assert_same_matrix(a, b, tag):
    for name, x, y in zip(("indptr", "indices", "data", "row_order"), a, b):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (tag, name)


def assert_same_long_rows(a, b, matrix, tag):
    """a, b: (the builder's list, the list that goes with row_order()) of the two forms.  The builders' lists are equal as sets
    and without repeats; the list that goes with the stored order -- the builder's own unless the rows were regrouped -- holds
    exactly the stored rows of more than 32 entries."""
    assert a[0].size == np.unique(a[0]).size and b[0].size == np.unique(b[0]).size, (tag, "a long row is listed twice")
    assert np.array_equal(np.sort(a[0]), np.sort(b[0])), (tag, "long rows differ")
    indptr, _, _, row_order = matrix
    assert a[0].size == (np.diff(indptr) > 32).sum(), (tag, "not as many long rows as rows of more than 32 entries")
    assert np.array_equal(np.sort(row_order[a[1]]), np.flatnonzero(np.diff(indptr) > 32)), (tag, "long rows are not the rows of more than 32 entries")


def assert_oracle(oracle, name, v, matrix, out, tag):
    indptr, indices, data, _ = matrix
    exp = oracle.regrid_csr(name, v.astype(np.float64), data, indices, indptr, indptr.size - 1)
    assert np.array_equal(np.isnan(out), np.isnan(exp)), tag
    if name == "geometric_mean":
        np.testing.assert_allclose(out, exp, rtol=RTOL_GEOMETRIC, equal_nan=True, err_msg=str(tag))
    else:
        assert_apply_equal(out, exp, indptr, name)


TAIL_ONE = {"place_big": 0, "publish": 1, "apply_rows1": 1}
TAIL_THREE = {"place_big": 1, "publish": 1, "apply_rows1": 1}


def tail_launches(launches):
    return {k: launches.get(k, 0) for k in ("place_big", "publish", "apply_rows1")}


@pytest.mark.parametrize("name", list(CASES))
def test_tail_one_launch_equals_three(hip, oracle, xr_option, name):
    sxy, sf = source_mesh()
    txy, tf = target_mesh(name)
    T = tf.shape[0]
    for dtype in (np.float64, np.float32):
        v = source_values(dtype)
        with DeviceBlocks(v, T) as dev:
            for method, method_id in METHODS:
                got = {}
                for value in (1, 0):
                    xr_option("tail_fused", value)
                    got[value] = step(hip, dev, sxy, sf, txy, tf, method_id)
                    assert tail_launches(got[value][3]) == (TAIL_ONE if value else TAIL_THREE), (name, value, got[value][3])
                xr_option("tail_fused", None)
                tag = (name, method, np.dtype(dtype).name)
                (m1, l1, o1, _), (m0, l0, o0, _) = got[1], got[0]
                assert_same_matrix(m1, m0, tag)
                assert_same_long_rows(l1, l0, m1, tag)
                assert np.array_equal(bits(o1), bits(o0)), (tag, "regridded values differ between the two forms")
                assert not (o1 == SENTINEL).any(), (tag, "a row was not written")
                assert_oracle(oracle, method, v, m1, o1, tag)
                lengths = np.diff(m1[0])
                for n in CASES[name][2]:
                    assert (lengths == n).any(), (tag, "no row of %d entries" % n, sorted(lengths[lengths > 16]))
                if name == "no_big":
                    assert lengths.max() <= 16 and l1[0].size == 0
                if name == "big_rows_up_to_32":
                    assert lengths.max() == 32 and (lengths > 16).sum() >= 3 and l1[0].size == 0  # (big faces, none of them listed)
                if name == "sliver":
                    assert lengths[-1] > 32  # (the sliver's row)


def test_tail_failed_first_attempt_leaves_the_output_alone(hip, oracle, xr_option):
    """A margin of one pair for the big faces' queue makes the first attempt fail AFTER the apply was enqueued behind it: every
    block of that apply must find the attempt not final.  What can be seen from outside: the retry's launches are there (two
    applies), the result is the final attempt's and equals the three-launch form's bit for bit, and the words behind the T results
    still hold the sentinel (fetch) -- a first attempt that followed its half-built rows would scatter through a row_order the
    retry has not written yet."""
    sxy, sf = source_mesh()
    name = "every_class_behind_512_regular_rows"
    txy, tf = target_mesh(name)
    v = source_values(np.float64)
    xr_option("queue_margin", 1)
    got = {}
    with DeviceBlocks(v, tf.shape[0]) as dev:
        for value in (1, 0):
            xr_option("tail_fused", value)
            got[value] = step(hip, dev, sxy, sf, txy, tf, 0)
            launches = got[value][3]
            assert launches["apply_rows1"] >= 2 and launches["publish"] == launches["apply_rows1"], launches
            assert launches.get("place_big", 0) == (0 if value else launches["publish"]), launches
    (m1, l1, o1, _), (m0, l0, o0, _) = got[1], got[0]
    assert_same_matrix(m1, m0, "regrow")
    assert_same_long_rows(l1, l0, m1, "regrow")
    assert np.array_equal(bits(o1), bits(o0)) and not (o1 == SENTINEL).any()
    assert_oracle(oracle, "mean", v, m1, o1, "regrow")


def test_tail_three_asynchronous_steps_then_the_general_chain(hip, oracle, xr_option):
    """Three steps back to back without host synchronisation, then a general-chain build: every step must start from a control
    block that is zero again, whichever launch came last."""
    E = hip.engine
    sxy, sf = source_mesh()
    txy, tf = target_mesh("every_class_behind_512_regular_rows")
    nxy, nf = target_mesh("no_big")
    v = source_values(np.float64)
    got = {}
    with DeviceBlocks(v, tf.shape[0]) as dev:
        for value in (1, 0):
            xr_option("tail_fused", value)
            ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
            dev.fill(SENTINEL)
            kept = []
            E.set_async(True)
            try:
                for _ in range(3):
                    ms.invalidate()
                    mt.invalidate()
                    kept.append(ms.overlap_apply_dev(mt, dev.src, E.XR_F64, 1, dev.out, 0))
                E.dev_sync()
            finally:
                E.set_async(False)
            out = dev.fetch()
            matrices = []
            for csr in kept:
                data, indices, indptr = csr.download()
                matrices.append((indptr, indices, data, csr.row_order()))
            xr_option("overlap_fused", 0)
            with E.KernelTimer() as timer:
                general = E.DeviceMesh(sxy, sf).overlap(E.DeviceMesh(nxy, nf))
            xr_option("overlap_fused", None)
            assert "place_big" not in launches_of(timer) and "row_fill" in launches_of(timer), launches_of(timer)
            got[value] = (matrices, out, general.download())
    for k in range(3):
        assert_same_matrix(got[1][0][k], got[0][0][k], ("async step", k))
        assert_same_matrix(got[1][0][k], got[1][0][0], ("async step against the first", k))
    assert np.array_equal(bits(got[1][1]), bits(got[0][1]))
    assert_oracle(oracle, "mean", v, got[1][0][2], got[1][1], "async")
    for x, y in zip(got[1][2], got[0][2]):
        assert np.array_equal(bits(x), bits(y)), "general chain behind the fused steps"
    fused = E.DeviceMesh(sxy, sf).overlap(E.DeviceMesh(nxy, nf)).download()
    for x, y in zip(got[1][2], fused):
        assert np.array_equal(bits(x), bits(y)), "general chain against the fused build"


def test_tail_other_entries_keep_their_three_launches(hip, oracle, xr_option):
    """overlap() alone and overlap_partial_dev have no K = 1 apply that could take the tail: place_big runs as before, whatever
    the option says, and their matrices do not depend on it."""
    E = hip.engine
    sxy, sf = source_mesh()
    txy, tf = target_mesh("every_class_behind_512_regular_rows")
    T = tf.shape[0]
    v = source_values(np.float64)
    got = {}
    for value in (1, 0):
        xr_option("tail_fused", value)
        ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
        with E.KernelTimer() as timer:
            csr = ms.overlap(mt)
        assert tail_launches(launches_of(timer)) == {"place_big": 1, "publish": 1, "apply_rows1": 0}, launches_of(timer)
        data, indices, indptr = csr.download()
        alone = (indptr, indices, data, csr.row_order())
        from xugrid_amd import _lib

        lib = _lib.load()
        n_comp = lib.xr_partial_components(0)
        src, out = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.xr_dev_alloc(v.nbytes, ctypes.byref(src)))
        _lib.check(lib.xr_dev_alloc(8 * n_comp * T, ctypes.byref(out)))
        try:
            _lib.check(lib.xr_dev_upload(src, v.ctypes.data_as(ctypes.c_void_p), v.nbytes))
            ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
            with E.KernelTimer() as timer:
                csr = ms.overlap_partial_dev(mt, src.value, E.XR_F64, 1, out.value, 0, False)
                E.dev_sync()
            launches = launches_of(timer)
            assert launches.get("place_big", 0) == 1 and launches.get("publish", 0) == 1 and "apply_rows1" not in launches, launches
            state = np.empty((n_comp, 1, T))
            _lib.check(lib.xr_dev_download(state.ctypes.data_as(ctypes.c_void_p), out, state.nbytes))
        finally:
            lib.xr_dev_free(src)
            lib.xr_dev_free(out)
        data, indices, indptr = csr.download()
        got[value] = (alone, (indptr, indices, data, csr.row_order()), state)
    assert_same_matrix(got[1][0], got[0][0], "overlap alone")
    assert_same_matrix(got[1][1], got[0][1], "overlap_partial_dev")
    assert_same_matrix(got[1][0], got[1][1], "overlap alone against overlap_partial_dev")
    assert np.array_equal(bits(got[1][2]), bits(got[0][2])), "partial states"
