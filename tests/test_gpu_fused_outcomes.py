"""
GPU (-m gpu): the outcome "the matrix is denser than the CSR the attempt reserved" of the fused weight build, with an apply
enqueued behind the failed attempt (overlap_apply_dev, overlap_partial_dev; K = 1).  k_publish_all and overlap_tri reach the
verdict with one function (xr_overlap_tail.h: fused_outcome; tests/test_fused_outcome_host.py tables it): the device keeps the
gate of the enqueued apply shut, the host doubles the entries reserved per face and runs a second attempt, which is final.

Source: an exact 64 x 64 lattice on [0, 1]^2, nodes at k / 64, every cell split into two counter-clockwise triangles (8192).
Targets "quads": 260 rectangles with four nodes of their own each, rectangle (i, j) of a 13 x 20 grid =
[(3i + 4.05) h, (3i + 6.95) h] x [(2j + 4.05) h, (2j + 5.95) h], h = 1 / 64: strictly inside its own block of 3 x 2 source cells
with a margin of 0.05 cell (~1e4 float32 ulp of the coordinates), so the search's float boxes hit exactly 12 records, every face
is regular and every row has 12 entries, nnz = 3120 -- the clip of KIND 1 (launch "clip_small").  Targets "tris": the same
rectangles cut into (p0, p1, p2) and (p0, p2, p3), 520 triangles, rows of 8 or 9 entries -- KIND 0 (launch "clip_tri").
(The CPU oracle gives nnz = 4196 for them here, 36 rows of 9 entries: p0 lies on a source diagonal up to rounding, and where it
rounds above it the triangle (p0, p1, p2) touches the source triangle across that diagonal in a sliver of 1e-34 that passes the
reference's pre-clip tests.  The request for this test quoted 4264 entries; no way of writing the coordinates above gave that
figure.  Either lies above the first attempt's capacity.)  The lengths are asserted on the oracle's pairs and the
downloaded matrix is compared with those pairs, so a mesh that came out differently fails here and not silently.

With queue_margin = 1 the first attempt's CSR holds 8 T + 1 entries: 2081 against 3120, 4161 against 4196.  It fails on capacity
with the apply already enqueued; the second attempt, at 16 T + 1, is final.  No face is big, so the big faces' queue of one
pair is never the reason.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_tail_fused import SENTINEL, DeviceBlocks, assert_oracle, assert_same_matrix, bits, cached, dtype_id, launches_of, step

pytestmark = pytest.mark.gpu

N = 64
H = 1.0 / N
MEAN = 0
# name: (row lengths that occur -- all of them --, nnz, the regular clip's launch, the other KIND's)
EXPECTED = {"quads": ([12], 3120, "clip_small", "clip_tri"), "tris": ([8, 9], 4196, "clip_tri", "clip_small")}


def source_mesh():
    def make():
        k = np.arange(N + 1) / N
        x, y = np.meshgrid(k, k, indexing="xy")
        idx = np.arange((N + 1) * (N + 1)).reshape(N + 1, N + 1)
        a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
        faces = np.empty((2 * N * N, 3), dtype=np.int64)
        faces[0::2] = np.column_stack([a, b, c])
        faces[1::2] = np.column_stack([a, c, d])
        return np.ascontiguousarray(np.column_stack([x.ravel(), y.ravel()])), faces

    return cached("lattice source", make)


def target_mesh(name):
    def make():
        rect = []
        for i in range(13):
            for j in range(20):
                x0, x1, y0, y1 = (3 * i + 4.05) * H, (3 * i + 6.95) * H, (2 * j + 4.05) * H, (2 * j + 5.95) * H
                rect.append([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
        xy = np.asarray(rect, dtype=np.float64).reshape(-1, 2)
        quads = np.arange(4 * len(rect), dtype=np.int64).reshape(-1, 4)
        if name == "quads":
            return xy, quads
        return xy, np.ascontiguousarray(np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3))

    return cached(("lattice target", name), make)


def source_values(dtype):
    def make():
        rng = np.random.default_rng(23)
        v = rng.normal(1.0, 0.5, size=(1, 2 * N * N))
        v[0, rng.choice(2 * N * N, 80, replace=False)] = np.nan
        return np.ascontiguousarray(v.astype(dtype))

    return cached(("lattice values", np.dtype(dtype).name), make)


def oracle_pairs(oracle, name):
    """-> (target face, source face, area) of the CPU oracle, rows ascending; the lengths the docstring promises are checked here"""

    def make():
        sxy, sf = source_mesh()
        txy, tf = target_mesh(name)
        q, s, a = oracle.CellTree2d(sxy, sf).intersect_faces(txy, tf)
        order = np.lexsort((s, q))
        q, s, a = q[order], s[order], a[order]
        lengths = np.bincount(q, minlength=tf.shape[0])
        assert sorted(np.unique(lengths)) == EXPECTED[name][0] and q.size == EXPECTED[name][1], (name, np.unique(lengths, return_counts=True), q.size)
        return q, s, a

    return cached(("lattice oracle", name), make)


def assert_is_oracle_matrix(oracle, name, matrix, tag):
    indptr, indices, data, _ = matrix
    q, s, a = oracle_pairs(oracle, name)
    lengths = np.diff(indptr)
    print(tag, "row lengths", dict(zip(*np.unique(lengths, return_counts=True))), "nnz", indices.size)
    assert sorted(np.unique(lengths)) == EXPECTED[name][0] and indices.size == EXPECTED[name][1], (tag, np.unique(lengths, return_counts=True))
    assert np.array_equal(np.repeat(np.arange(lengths.size), lengths), q) and np.array_equal(indices, s), (tag, "pairs differ from the oracle's")
    assert np.array_equal(bits(data), bits(a)), (tag, "areas differ from the oracle's")


@pytest.mark.parametrize("name", list(EXPECTED))
def test_csr_capacity_fails_behind_an_enqueued_apply(hip, oracle, xr_option, name):
    E = hip.engine
    sxy, sf = source_mesh()
    txy, tf = target_mesh(name)
    T = tf.shape[0]
    regular_clip, other_clip = EXPECTED[name][2:]
    assert 8 * T + 1 < EXPECTED[name][1] <= 16 * T + 1  # the first attempt cannot hold the matrix, the second can
    for dtype in (np.float64, np.float32):
        v = source_values(dtype)
        tag = (name, np.dtype(dtype).name)
        with DeviceBlocks(v, T) as dev:
            plain = step(hip, dev, sxy, sf, txy, tf, MEAN)  # default margin: one attempt
            assert {k: plain[3].get(k, 0) for k in ("publish", "apply_rows1", "place_big")} == {"publish": 1, "apply_rows1": 1, "place_big": 0}, plain[3]
            xr_option("queue_margin", 1)
            forced = {}
            for value in (1, 0):
                xr_option("tail_fused", value)
                forced[value] = step(hip, dev, sxy, sf, txy, tf, MEAN)  # (fetch: the slack behind the T results is untouched)
                launches = forced[value][3]
                print(tag, "tail_fused", value, launches)
                assert launches.get("publish", 0) == 2 and launches.get("apply_rows1", 0) == 2, (tag, launches)
                assert launches.get("place_big", 0) == (0 if value else 2), (tag, launches)
                assert launches.get(regular_clip, 0) == 2 and other_clip not in launches and "row_fill" not in launches, (tag, launches)
            xr_option("tail_fused", None)
            # the two-call form, its build failing once too
            ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
            with E.KernelTimer() as timer:
                csr = ms.overlap(mt)
            assert launches_of(timer).get("publish", 0) == 2 and "apply_rows1" not in launches_of(timer), launches_of(timer)
            dev.fill(SENTINEL)
            csr.apply_dev(dev.src, dtype_id(E, v), 1, dev.out, MEAN)
            E.dev_sync()
            two_call = dev.fetch()
            data, indices, indptr = csr.download()
            two_call_matrix = (indptr, indices, data, csr.row_order())
            xr_option("queue_margin", None)
        m, _, out, _ = forced[1]
        assert not (out == SENTINEL).any(), (tag, "a row was not written")
        assert_is_oracle_matrix(oracle, name, m, tag)
        assert_same_matrix(m, plain[0], (tag, "against the build without a failed attempt"))
        assert_same_matrix(m, forced[0][0], (tag, "against tail_fused = 0"))
        assert_same_matrix(m, two_call_matrix, (tag, "against overlap alone"))
        assert forced[1][1][0].size == 0 and plain[1][0].size == 0, (tag, "a long row is listed")
        for other, what in ((plain[2], "the build without a failed attempt"), (forced[0][2], "tail_fused = 0"), (two_call, "overlap, then apply_dev")):
            assert np.array_equal(bits(out), bits(other)), (tag, "regridded values differ from " + what)
        assert_oracle(oracle, "mean", v, m, out, tag)  # (every row has at most 32 entries: bit for bit)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_csr_capacity_fails_behind_an_enqueued_partial_apply(hip, xr_option, name):
    """overlap_partial_dev, K = 1: the gate path of xr_partial.hip.  The planes equal those of partial_dev on the finished matrix."""
    from xugrid_amd import _lib

    E = hip.engine
    lib = _lib.load()
    sxy, sf = source_mesh()
    txy, tf = target_mesh(name)
    T = tf.shape[0]
    v = source_values(np.float64)
    n_comp = lib.xr_partial_components(MEAN)
    assert n_comp > 0
    src, early, late = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.xr_dev_alloc(v.nbytes, ctypes.byref(src)))
    _lib.check(lib.xr_dev_alloc(8 * n_comp * T, ctypes.byref(early)))
    _lib.check(lib.xr_dev_alloc(8 * n_comp * T, ctypes.byref(late)))
    try:
        _lib.check(lib.xr_dev_upload(src, v.ctypes.data_as(ctypes.c_void_p), v.nbytes))
        for block, value in ((early, SENTINEL), (late, np.nan)):  # (filled differently: planes nobody wrote cannot compare equal)
            host = np.full(n_comp * T, value)
            _lib.check(lib.xr_dev_upload(block, host.ctypes.data_as(ctypes.c_void_p), host.nbytes))
        xr_option("queue_margin", 1)
        ms, mt = E.DeviceMesh(sxy, sf), E.DeviceMesh(txy, tf)
        with E.KernelTimer() as timer:
            csr = ms.overlap_partial_dev(mt, src.value, E.XR_F64, 1, early.value, MEAN, False)
            E.dev_sync()
        launches = launches_of(timer)
        print(name, launches)
        assert launches.get("publish", 0) == 2 and launches.get("apply_partial", 0) == 2 and launches.get("place_big", 0) == 2, launches
        xr_option("queue_margin", None)
        csr.partial_dev(src.value, E.XR_F64, 1, late.value, MEAN, False)
        E.dev_sync()
        got, exp = np.empty((n_comp, 1, T)), np.empty((n_comp, 1, T))
        _lib.check(lib.xr_dev_download(got.ctypes.data_as(ctypes.c_void_p), early, got.nbytes))
        _lib.check(lib.xr_dev_download(exp.ctypes.data_as(ctypes.c_void_p), late, exp.nbytes))
    finally:
        for block in (src, early, late):
            lib.xr_dev_free(block)
    assert csr.nnz == EXPECTED[name][1]
    assert not (got == SENTINEL).any(), "a plane was not written"
    assert np.array_equal(bits(got), bits(exp)), "partial states differ from partial_dev on the finished matrix"
